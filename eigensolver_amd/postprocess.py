"""Root-table post-processing and result formats -- what every analysis script of the
reference does first with a result pickle (e.g. Cylinder/Non-uniform flow/Coronal/Eigenfunctions/
analysis_cylinder_flow_coronal.py:216-250 and the commented classifiers :282-372): sort the (k, omega) pairs by
wavenumber, split them into branches by phase-speed bands, fit a polynomial per branch; plus the pickle layout
`[omega_sausage, k_sausage, omega_kink, k_kink]` the solver scripts dump (Density_cylinder.py:1182-1183) so that the
reference's own analysis / movie scripts can consume the GPU results unchanged.  Host-side NumPy: the tables hold a
few thousand roots."""
import pickle

import numpy as np


def sort_by_wavenumber(omegas, ks):
    """`[x for _, x in sorted(zip(ks, omegas))]`, `np.sort(ks)` (analysis_cylinder_flow_coronal.py:224-228): pairs
    ordered by k, ties by omega."""
    omegas, ks = np.asarray(omegas, dtype=np.float64), np.asarray(ks, dtype=np.float64)
    order = np.lexsort((omegas, ks))
    return omegas[order], ks[order]


def split_branches(omegas, ks, bands):
    """Classify roots by phase speed: bands = {name: (lo, hi)} -> {name: (omegas, ks)} with lo < omega/k < hi
    (the commented classifier blocks, e.g. fast body vA_i < w/k < vA_e, :244-372)."""
    omegas, ks = np.asarray(omegas, dtype=np.float64), np.asarray(ks, dtype=np.float64)
    with np.errstate(all="ignore"):
        W = omegas / ks
    out = {}
    for name, (lo, hi) in bands.items():
        sel = (W > lo) & (W < hi)
        out[name] = (omegas[sel], ks[sel])
    return out


def fit_branch(ks, omegas, deg=6):
    """Polynomial fit omega(k) of one branch (np.polyfit / np.poly1d as in the analysis scripts)."""
    if len(ks) <= deg:
        raise ValueError("not enough points for the requested degree")
    return np.poly1d(np.polyfit(np.asarray(ks, dtype=np.float64), np.asarray(omegas, dtype=np.float64), deg))


def pickle_layout(result):
    """`solve()` output {"sausage": (w, k), "kink": (w, k)} -> the list the reference dumps:
    [sol_omegas1, sol_ks1, sol_omegas_kink1, sol_ks_kink1]; single-mode scripts (rotational) dump [w, k]."""
    if "sausage" in result and "kink" in result:
        return [np.asarray(result["sausage"][0]), np.asarray(result["sausage"][1]),
                np.asarray(result["kink"][0]), np.asarray(result["kink"][1])]
    (w, k), = result.values()
    return [np.asarray(w), np.asarray(k)]


def save_pickle(path, result):
    """Write the result in the reference's pickle layout (Density_cylinder.py:1182-1183)."""
    with open(path, "wb") as f:
        pickle.dump(pickle_layout(result), f)


def from_root_table(roots, accepted_only=True):
    """Grid-mode root table (ShootProblem.find_roots) -> (omegas, ks) NumPy arrays."""
    w = roots["w"].detach().cpu().numpy()
    k = roots["k"].detach().cpu().numpy()
    if accepted_only:
        sel = roots["flag"].detach().cpu().numpy() == 1
        w, k = w[sel], k[sel]
    return w, k


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def split_by_signature(roots, sig, accepted_only=True):
    """Root table + its ShootProblem.label_roots signature -> {(nodes_value, nodes_flux): (omegas, ks)}, one k-sorted curve
    (sort_by_wavenumber) per branch label: what the analysis scripts cut out with hand-picked phase-speed cut-offs per data
    set (fast_sausage_branch1/2/3, ..., :244-372).  Each entry is ready for fit_branch; {"kink": entry} for pickle_layout.
    accepted_only drops the entries with flag == 0 and the pairs that are not ES_PT_OK (label (-1, -1))."""
    w, k = _host(roots["w"]).astype(np.float64), _host(roots["k"]).astype(np.float64)
    nv, nf, st = (_host(a).astype(np.int64) for a in (sig.nodes_value, sig.nodes_flux, sig.status))
    assert len(w) == len(k) == len(nv) == len(nf) == len(st), "the signature must be aligned with the table"
    keep = np.ones(len(w), dtype=bool)
    if accepted_only:
        keep = (_host(roots["flag"]) == 1) & (st == 0)
    out = {}
    for label in sorted(set(zip(nv[keep].tolist(), nf[keep].tolist()))):
        sel = keep & (nv == label[0]) & (nf == label[1])
        out[label] = sort_by_wavenumber(w[sel], k[sel])
    return out


def curves_with_slopes(roots, sig, slopes, accepted_only=True):
    """split_by_signature with the group speed riding along: root table + its label_roots signature + its root_slopes
    (ShootProblem.root_slopes, or anything with group_velocity and status) -> {label: (omegas, ks, cg)}, each curve ordered
    by k (ties by omega).  accepted_only drops the entries with flag == 0 and the pairs either call did not find ES_PT_OK."""
    w, k = _host(roots["w"]).astype(np.float64), _host(roots["k"]).astype(np.float64)
    nv, nf, st = (_host(a).astype(np.int64) for a in (sig.nodes_value, sig.nodes_flux, sig.status))
    cg, st2 = _host(slopes.group_velocity).astype(np.float64), _host(slopes.status).astype(np.int64)
    assert len(w) == len(k) == len(nv) == len(nf) == len(st) == len(cg) == len(st2), \
        "signature and slopes must be aligned with the table"
    keep = np.ones(len(w), dtype=bool)
    if accepted_only:
        keep = (_host(roots["flag"]) == 1) & (st == 0) & (st2 == 0)
    out = {}
    for label in sorted(set(zip(nv[keep].tolist(), nf[keep].tolist()))):
        sel = np.nonzero(keep & (nv == label[0]) & (nf == label[1]))[0]
        sel = sel[np.lexsort((w[sel], k[sel]))]
        out[label] = (w[sel], k[sel], cg[sel])
    return out


def traced_curves(branches):
    """The flagged points of ShootProblem.trace_branches (its `branches`, or the TracedBranches itself) in the layout of
    curves_with_slopes: {label: (omegas, ks, cg)} with cg the dwdk of the final Newton point, each curve ordered by k --
    ready for hermite_branch, fit_branch and, as {"kink": entry[:2]}, pickle_layout.  This is the one host read."""
    branches = getattr(branches, "branches", branches)
    out = {}
    for label, b in branches.items():
        w, k, cg = (_host(b[a]).astype(np.float64) for a in ("w", "k", "dwdk"))
        sel = np.nonzero(_host(b["flag"]) == 1)[0]
        sel = sel[np.argsort(k[sel], kind="stable")]
        out[label] = (w[sel], k[sel], cg[sel])
    return out


def hermite_branch(ks, omegas, cg):
    """omega(k) of one branch as the piecewise-cubic Hermite interpolant through the roots (ks strictly increasing) with
    the slopes cg = d omega / dk (ShootProblem.group_velocity): what a degree-6 fit_branch stands in for when the slopes are
    not known.  Returns f(k, nu=0): omega (nu = 0) or d omega / dk (nu = 1) at scalar or array k; outside [ks[0], ks[-1]]
    the cubic of the end interval is continued."""
    x, y, d = (np.asarray(a, dtype=np.float64) for a in (ks, omegas, cg))
    if not (x.ndim == 1 and x.shape == y.shape == d.shape and len(x) >= 2):
        raise ValueError("ks, omegas, cg must be 1-D arrays of one length >= 2")
    if not np.all(np.diff(x) > 0):
        raise ValueError("ks must be strictly increasing")
    h = np.diff(x)

    def f(k, nu=0):
        k = np.asarray(k, dtype=np.float64)
        j = np.clip(np.searchsorted(x, k, side="right") - 1, 0, len(x) - 2)
        hj = h[j]
        t = (k - x[j]) / hj
        if nu == 0:
            return ((2 * t ** 3 - 3 * t ** 2 + 1) * y[j] + (t ** 3 - 2 * t ** 2 + t) * hj * d[j]
                    + (-2 * t ** 3 + 3 * t ** 2) * y[j + 1] + (t ** 3 - t ** 2) * hj * d[j + 1])
        if nu == 1:
            return ((6 * t ** 2 - 6 * t) * (y[j] - y[j + 1]) / hj + (3 * t ** 2 - 4 * t + 1) * d[j]
                    + (3 * t ** 2 - 2 * t) * d[j + 1])
        raise ValueError("nu must be 0 or 1")
    return f


def hermite_branch_quintic(ks, omegas, cg, curv):
    """hermite_branch with the curvature known as well: omega(k) of one branch as the piecewise-quintic Hermite interpolant
    through the roots (ks strictly increasing) with the slopes cg = d omega / dk and the second derivatives
    curv = d2 omega / dk2 (ShootProblem.root_curvature).  Returns f(k, nu=0): omega (nu = 0), d omega / dk (nu = 1) or
    d2 omega / dk2 (nu = 2) at scalar or array k, all three continuous at the knots; outside [ks[0], ks[-1]] the quintic of
    the end interval is continued."""
    x, y, d, c = (np.asarray(a, dtype=np.float64) for a in (ks, omegas, cg, curv))
    if not (x.ndim == 1 and x.shape == y.shape == d.shape == c.shape and len(x) >= 2):
        raise ValueError("ks, omegas, cg, curv must be 1-D arrays of one length >= 2")
    if not np.all(np.diff(x) > 0):
        raise ValueError("ks must be strictly increasing")
    h = np.diff(x)
    # per interval, in t = (k - k_j) / h: a0 + a1 t + ... + a5 t^5 with the six end conditions
    dy, d0, d1, c0, c1 = y[1:] - y[:-1], h * d[:-1], h * d[1:], h * h * c[:-1], h * h * c[1:]
    a = np.array([y[:-1], d0, 0.5 * c0,
                  10.0 * dy - 6.0 * d0 - 4.0 * d1 - 0.5 * (3.0 * c0 - c1),
                  -15.0 * dy + 8.0 * d0 + 7.0 * d1 + 0.5 * (3.0 * c0 - 2.0 * c1),
                  6.0 * dy - 3.0 * d0 - 3.0 * d1 - 0.5 * (c0 - c1)])

    def f(k, nu=0):
        if nu not in (0, 1, 2):
            raise ValueError("nu must be 0, 1 or 2")
        k = np.asarray(k, dtype=np.float64)
        j = np.clip(np.searchsorted(x, k, side="right") - 1, 0, len(x) - 2)
        t = (k - x[j]) / h[j]
        out = np.zeros_like(t)
        for p in range(5, nu - 1, -1):                          # Horner on the nu-th derivative in t
            fac = float(np.prod(np.arange(p - nu + 1, p + 1))) if nu else 1.0
            out = out * t + fac * a[p][j]
        return out / h[j] ** nu
    return f


def _hermite_complex_arrays(ks, omegas, dwdk):
    x = np.asarray(ks, dtype=np.float64)
    y, d = np.asarray(omegas, dtype=np.complex128), np.asarray(dwdk, dtype=np.complex128)
    if not (x.ndim == 1 and x.shape == y.shape == d.shape and len(x) >= 2):
        raise ValueError("ks, omegas, dwdk must be 1-D arrays of one length >= 2")
    if not np.all(np.diff(x) > 0):
        raise ValueError("ks must be strictly increasing")
    return x, y, d


def hermite_branch_complex(ks, omegas, dwdk):
    """hermite_branch for a branch of complex roots (SlabComplexFlow.find_roots / densify): the piecewise-cubic Hermite
    interpolant through the complex omegas (ks real, strictly increasing) with the complex slopes dwdk = d omega / dk
    (SlabComplexFlow.group_velocity).  Returns f(k, nu=0): omega (nu = 0) or d omega / dk (nu = 1), complex, at scalar or
    array k; outside [ks[0], ks[-1]] the cubic of the end interval is continued."""
    x, y, d = _hermite_complex_arrays(ks, omegas, dwdk)
    h = np.diff(x)

    def f(k, nu=0):
        k = np.asarray(k, dtype=np.float64)
        j = np.clip(np.searchsorted(x, k, side="right") - 1, 0, len(x) - 2)
        hj = h[j]
        t = (k - x[j]) / hj
        if nu == 0:
            return ((2 * t ** 3 - 3 * t ** 2 + 1) * y[j] + (t ** 3 - 2 * t ** 2 + t) * hj * d[j]
                    + (-2 * t ** 3 + 3 * t ** 2) * y[j + 1] + (t ** 3 - t ** 2) * hj * d[j + 1])
        if nu == 1:
            return ((6 * t ** 2 - 6 * t) * (y[j] - y[j + 1]) / hj + (3 * t ** 2 - 4 * t + 1) * d[j]
                    + (3 * t ** 2 - 2 * t) * d[j + 1])
        raise ValueError("nu must be 0 or 1")
    return f


def most_unstable(ks, omegas, dwdk):
    """The growth-rate maxima of one branch of complex roots: in every interval of ks (strictly increasing) where
    Im d omega / dk goes from positive to non-positive, the maximum of Im omega of that interval's Hermite cubic
    (hermite_branch_complex), found in closed form as the root of the derivative quadratic at which the derivative falls.
    Returns (k*, omega*): a float64 and a complex128 array with one entry per such interval, empty when there is none."""
    x, y, d = _hermite_complex_arrays(ks, omegas, dwdk)
    f = hermite_branch_complex(x, y, d)
    k_out = []
    for j in range(len(x) - 1):
        d0, d1 = d[j].imag, d[j + 1].imag
        if not (d0 > 0.0 and d1 <= 0.0):
            continue
        h, dy = x[j + 1] - x[j], y[j].imag - y[j + 1].imag
        # h (Im omega)'(t) = A t^2 + B t + C on t in [0, 1]; C > 0 and A + B + C = h d1 <= 0: it falls through zero once
        A, B, C = 6.0 * dy + 3.0 * h * (d0 + d1), -6.0 * dy - 4.0 * h * d0 - 2.0 * h * d1, h * d0
        if A == 0.0:
            cand = [-C / B]
        else:
            q = -0.5 * (B + np.copysign(np.sqrt(max(B * B - 4.0 * A * C, 0.0)), B))
            cand = [q / A, C / q]
        cand = [t for t in cand if 2.0 * A * t + B <= 0.0]      # where the derivative falls: the maximum
        t = min(cand, key=lambda t: abs(t - 0.5))
        k_out.append(x[j] + min(max(t, 0.0), 1.0) * h)
    k_out = np.array(k_out, dtype=np.float64)
    return k_out, (np.asarray(f(k_out), dtype=np.complex128) if len(k_out) else np.zeros(0, dtype=np.complex128))


def write_vtk(dump_file, x, y, z, variables, names):
    """Legacy-VTK structured-grid dump of scalar fields on an irregular grid, byte for byte what the reference's
    `makeDumpVTK(x, y, z, variables, varList, dumpFile)` writes (Cylinder/Non-uniform density/Coronal/Movies/
    Export_vtk.py:70-112): header lines as there (trailing blanks included), BINARY, big-endian float32, points as
    interleaved (x, y, z) with the first index fastest, one `SCALARS <name> float` block per variable.
    x, y, z and every variable are arrays of the same shape (ax, ay, az).  Writes `<dump_file>.vtk`."""
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    if not (x.ndim == 3 and x.shape == y.shape == z.shape):
        raise ValueError("x, y, z must be 3-D arrays of one shape")
    if len(variables) != len(names):
        raise ValueError("one name per variable")
    ax, ay, az = x.shape
    n = ax * ay * az

    def packed(a):                     # loop order k, j, i with i fastest = Fortran order of an (i, j, k) array
        return np.asarray(a, dtype=np.float64).astype(">f4").ravel(order="F")

    with open(str(dump_file) + ".vtk", "wb") as f:
        f.write(b"# vtk DataFile Version 3.0 \n")
        f.write(b"vtk output \n")
        f.write(b"BINARY \n")
        f.write(b"DATASET STRUCTURED_GRID \n")
        f.write(("DIMENSIONS  %s %s %s  \n" % (ax, ay, az)).encode())
        f.write(("POINTS %s float  \n" % n).encode())
        pts = np.empty((n, 3), dtype=">f4")
        pts[:, 0], pts[:, 1], pts[:, 2] = packed(x), packed(y), packed(z)
        f.write(pts.tobytes())
        f.write(("\nPOINT_DATA %s  " % n).encode())
        for name, var in zip(names, variables):
            var = np.asarray(var)
            if var.shape != x.shape:
                raise ValueError(f"variable {name!r} has shape {var.shape}, grid is {x.shape}")
            f.write(("\nSCALARS %s float \n" % name).encode())
            f.write(b"LOOKUP_TABLE default \n")
            f.write(packed(var).tobytes())
    return str(dump_file) + ".vtk"


def _payload(a):
    """bytes of an already-packed big-endian payload: bytes-like, a NumPy array or a CPU torch tensor (any dtype: its
    memory is written as it stands)."""
    if isinstance(a, (bytes, bytearray, memoryview)):
        return a
    if hasattr(a, "detach"):                     # torch tensor
        if a.is_cuda:
            raise ValueError("packed payloads must be in host memory (tensor.cpu())")
        a = a.detach().contiguous().numpy()
    return np.ascontiguousarray(a).tobytes()


def write_vtk_packed(dump_file, dims, points_be, variables_be, names):
    """`write_vtk` for payloads that are already packed: the same header lines around big-endian float32 buffers in VTK's
    point order (first index fastest), e.g. what ShootProblem.fields(..., big_endian=True) produces on the GPU.
    dims = (ax, ay, az); points_be holds ax*ay*az interleaved (x, y, z) triples, every entry of variables_be ax*ay*az
    values.  Byte for byte the file write_vtk gives for the same numbers.  Writes `<dump_file>.vtk`."""
    ax, ay, az = (int(v) for v in dims)
    n = ax * ay * az
    if len(variables_be) != len(names):
        raise ValueError("one name per variable")
    pts = _payload(points_be)
    if len(pts) != 12 * n:
        raise ValueError(f"points payload has {len(pts)} bytes, the grid needs {12 * n}")
    with open(str(dump_file) + ".vtk", "wb") as f:
        f.write(b"# vtk DataFile Version 3.0 \n")
        f.write(b"vtk output \n")
        f.write(b"BINARY \n")
        f.write(b"DATASET STRUCTURED_GRID \n")
        f.write(("DIMENSIONS  %s %s %s  \n" % (ax, ay, az)).encode())
        f.write(("POINTS %s float  \n" % n).encode())
        f.write(pts)
        f.write(("\nPOINT_DATA %s  " % n).encode())
        for name, var in zip(names, variables_be):
            buf = _payload(var)
            if len(buf) != 4 * n:
                raise ValueError(f"variable {name!r} has {len(buf)} bytes, the grid needs {4 * n}")
            f.write(("\nSCALARS %s float \n" % name).encode())
            f.write(b"LOOKUP_TABLE default \n")
            f.write(buf)
    return str(dump_file) + ".vtk"


def write_vtk_frames(prefix, fields_iter, names=None):
    """One legacy-VTK file per frame from ShootProblem.fields(..., big_endian=True): `<prefix><t>.vtk` with t the frame
    number counted over all chunks, the naming of Export_vtk.py:989.  fields_iter is the dict `fields` returns or the
    generator it returns with frames_per_call; names defaults to the variables of the chunks.  Each chunk is copied to
    the host once.  Returns the list of files written."""
    if isinstance(fields_iter, dict):
        fields_iter = [fields_iter]
    files, frame, pts = [], 0, None
    for chunk in fields_iter:
        use = list(chunk["names"]) if names is None else list(names)
        if pts is None:
            n_z, n_theta, n_r = chunk["points"].shape[:3]
            pts = chunk["points"].cpu()
        host = {v: chunk[v].cpu() for v in use}
        for i in range(chunk["frames"].shape[0]):
            files.append(write_vtk_packed(str(prefix) + str(frame), (n_r, n_theta, n_z), pts,
                                          [host[v][i] for v in use], use))
            frame += 1
    return files


def write_vtk_rectilinear(dump_file, x, y, z, variables_be, names):
    """Legacy-VTK RECTILINEAR_GRID, BINARY, of scalar fields on the Cartesian mesh x [n_x], y [n_y], z [n_z] (host arrays,
    written as big-endian float32 `X_COORDINATES n float` etc.).  Every entry of variables_be is an already-packed
    payload of n_x*n_y*n_z big-endian float32 values, x fastest -- one frame of one variable of
    ShootProblem.cartesian_fields(..., big_endian=True), copied to the host.  Writes `<dump_file>.vtk`."""
    x, y, z = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (x, y, z))
    if len(variables_be) != len(names):
        raise ValueError("one name per variable")
    n = x.size * y.size * z.size
    with open(str(dump_file) + ".vtk", "wb") as f:
        f.write(b"# vtk DataFile Version 3.0\n")
        f.write(b"vtk output\n")
        f.write(b"BINARY\n")
        f.write(b"DATASET RECTILINEAR_GRID\n")
        f.write(("DIMENSIONS %d %d %d\n" % (x.size, y.size, z.size)).encode())
        for axis, a in (("X", x), ("Y", y), ("Z", z)):
            f.write(("%s_COORDINATES %d float\n" % (axis, a.size)).encode())
            f.write(a.astype(">f4").tobytes())
            f.write(b"\n")
        f.write(("POINT_DATA %d\n" % n).encode())
        for name, var in zip(names, variables_be):
            buf = _payload(var)
            if len(buf) != 4 * n:
                raise ValueError(f"variable {name!r} has {len(buf)} bytes, the grid needs {4 * n}")
            f.write(("SCALARS %s float\n" % name).encode())
            f.write(b"LOOKUP_TABLE default\n")
            f.write(buf)
            f.write(b"\n")
    return str(dump_file) + ".vtk"


def write_vtk_rectilinear_frames(prefix, x, y, z, fields_iter, names=None):
    """One RECTILINEAR_GRID file per frame from ShootProblem.cartesian_fields(..., big_endian=True): `<prefix><t>.vtk`
    with t the frame number counted over all chunks, as write_vtk_frames names them.  fields_iter is the dict
    `cartesian_fields` returns or the generator it returns with frames_per_call; x, y, z are the host arrays the mesh was
    built from; names defaults to the variables of the chunks.  Each chunk is copied to the host once.  Returns the list
    of files written."""
    if isinstance(fields_iter, dict):
        fields_iter = [fields_iter]
    files, frame = [], 0
    for chunk in fields_iter:
        use = list(chunk["names"]) if names is None else list(names)
        host = {v: chunk[v].cpu() for v in use}
        for i in range(chunk["frames"].shape[0]):
            files.append(write_vtk_rectilinear(str(prefix) + str(frame), x, y, z, [host[v][i] for v in use], use))
            frame += 1
    return files
