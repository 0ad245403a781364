"""NumPy restatement of include/eigensolver_amd.h section 8 (es_cyl_vorticity_amplitudes, es_cyl_cartesian_synthesis),
taking the same arrays as the C calls: np.gradient(..., edge_order=2) per region, np.searchsorted + linear interpolation
per region, the tie and fill rules, the one rounding to float32.  Every function takes the floating type to compute in
(`dtype=np.longdouble` gives the yardstick E_round of the tests: the model against itself in extended precision).

The angle factors come from arctan2 and cos / sin of m theta, not from the angle-addition recurrence the kernel uses.

Pinned on the CPU by tests/test_cartesian_model.py: analytic curl of quadratic amplitudes, and np.gradient of the sampled
velocity with the mesh coordinates."""
import numpy as np

from tests.field_model import AMP_NAMES

VORT_NAMES = ("Wr_C", "Wr_S", "Wphi_C", "Wphi_S", "Wz_C")
CVAR_NAMES = ("P_T", "xi_x", "xi_y", "xi_z", "v_x", "v_y", "v_z", "vort_x", "vort_y", "vort_z")


def region_gradient(a, r, n_nodes, dtype=np.float64):
    """d a / d r by np.gradient(a, r, edge_order=2) on [0, n_nodes) and [n_nodes, n_r) separately."""
    a, r = np.asarray(a, dtype=dtype), np.asarray(r, dtype=dtype)
    out = np.empty_like(a)
    for s in (slice(0, n_nodes), slice(n_nodes, a.size)):
        if a[s].size:
            if a[s].size < 3:
                raise ValueError("a region that is present needs at least 3 points")
            with np.errstate(all="ignore"):
                out[s] = np.gradient(a[s], r[s], edge_order=2)
    return out


def vorticity_amplitudes(radius, amp, n_nodes, m, k, dtype=np.float64):
    """One mode: radius [n_r], amp [7, n_r] -> vort [5, n_r] in the order VORT_NAMES."""
    r = np.asarray(radius, dtype=dtype)
    A = dict(zip(AMP_NAMES, np.asarray(amp, dtype=dtype)))
    a_r, a_p, a_z = A["v_r"], A["v_phi"], A["v_z"]
    m, k = dtype(m), dtype(k)
    d_az = region_gradient(a_z, r, n_nodes, dtype)
    d_ap = region_gradient(a_p, r, n_nodes, dtype)
    with np.errstate(all="ignore"):
        return np.stack([-m * a_z / r, -k * a_p, -d_az, -k * a_r, (m * a_r - a_p - r * d_ap) / r])


def locate(radius, n_nodes, r):
    """Region and bracket of every r: (valid, j) with j the index into radius of the lower bracketing node, `last` true where
    r sits exactly on the last node of its region.  Interior radius[0] <= r <= radius[n_nodes-1] (ties on the boundary
    radius are interior), exterior radius[n_nodes-1] < r <= radius[n_r-1]; r = 0, NaN and everything else is invalid."""
    radius = np.asarray(radius)
    n_r, n_ext = radius.size, radius.size - n_nodes
    r = np.asarray(r)
    with np.errstate(invalid="ignore"):
        inside = (r >= radius[0]) & (r <= radius[n_nodes - 1]) if n_nodes else np.zeros(r.shape, bool)
        if n_ext:
            outside = (r <= radius[n_r - 1]) & ((r > radius[n_nodes - 1]) if n_nodes else (r >= radius[0]))
        else:
            outside = np.zeros(r.shape, bool)
        valid = (inside | outside) & (r > 0)
    j = np.zeros(r.shape, dtype=np.int64)
    last = np.zeros(r.shape, dtype=bool)
    for sel, base, length in ((inside & valid, 0, n_nodes), (outside & valid, n_nodes, n_ext)):
        if length and sel.any():
            reg = radius[base:base + length]
            jj = np.clip(np.searchsorted(reg, r[sel], side="right") - 1, 0, length - 2)
            j[sel] = base + jj
            last[sel] = r[sel] >= reg[jj + 1]
    return valid, j, last


def synthesis(radius, amp, vort, n_nodes, m, k, w, x, y, z, t, variables=None, v_scale=1.0, fill=np.nan,
              dtype=np.float64):
    """Fields [n_t, n_sel, n_z, n_y, n_x] in `dtype`, not yet rounded, in ascending order of the mask bits (CVAR_NAMES),
    `fill` where the point is outside the tabulated radii; also the names and the valid mask [n_y, n_x]."""
    names = [v for v in CVAR_NAMES if variables is None or v in variables]
    radius = np.asarray(radius, dtype=dtype)
    x, y, z, t = (np.asarray(a, dtype=dtype).reshape(-1) for a in (x, y, z, t))
    X, Y = x[None, :], y[:, None]
    with np.errstate(all="ignore"):
        r = np.hypot(X, Y) + np.zeros_like(X * Y)
        valid, j, last = locate(radius, n_nodes, r)
        rj, rj1 = radius[j], radius[np.minimum(j + 1, radius.size - 1)]
        frac = (r - rj) / (rj1 - rj)

        def interp(a):
            a = np.asarray(a, dtype=dtype)
            a1 = a[np.minimum(j + 1, a.size - 1)]
            return np.where(last, a1, a[j] + (a1 - a[j]) * frac)

        th = np.arctan2(Y + np.zeros_like(r), X + np.zeros_like(r))
        ct, st = X / r, Y / r
        cm, sm = np.cos(dtype(m) * th), np.sin(dtype(m) * th)
        A = {n: interp(a) for n, a in zip(AMP_NAMES, amp)}
        vs = dtype(v_scale)
        cC, cS = {}, {}
        cC["P_T"] = A["P_T"] * cm
        cC["xi_x"] = A["xi_r"] * cm * ct - A["xi_phi"] * (-sm) * st
        cC["xi_y"] = A["xi_r"] * cm * st + A["xi_phi"] * (-sm) * ct
        cC["xi_z"] = A["xi_z"] * cm
        cC["v_x"] = vs * (A["v_r"] * cm * ct - A["v_phi"] * (-sm) * st)
        cC["v_y"] = vs * (A["v_r"] * cm * st + A["v_phi"] * (-sm) * ct)
        cC["v_z"] = vs * A["v_z"] * cm
        if vort is not None:
            V = {n: interp(a) for n, a in zip(VORT_NAMES, vort)}
            wr_c, wr_s = sm * V["Wr_C"], sm * V["Wr_S"]                          # omega_r   = wr_c C + wr_s S
            wp_c, wp_s = cm * V["Wphi_C"], cm * V["Wphi_S"]                      # omega_phi = wp_c C + wp_s S
            cC["vort_x"], cS["vort_x"] = vs * (wr_c * ct - wp_c * st), vs * (wr_s * ct - wp_s * st)
            cC["vort_y"], cS["vort_y"] = vs * (wr_c * st + wp_c * ct), vs * (wr_s * st + wp_s * ct)
            cC["vort_z"] = vs * sm * V["Wz_C"]
        ph = dtype(k) * z[None, :, None, None] - dtype(w) * t[:, None, None, None]
        C, S = np.cos(ph), np.sin(ph)
        out = np.empty((t.size, len(names), z.size, y.size, x.size), dtype=dtype)
        for i, v in enumerate(names):
            f = cC[v][None, None] * C
            if v in cS:
                f = f + cS[v][None, None] * S
            out[:, i] = np.where(valid[None, None], f, dtype(fill))
    return out, names, valid


def to_f32(a):
    """The one rounding to float32."""
    with np.errstate(all="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32)


def synthesis_bound(model, amp, vort, v_scale):
    """Section 7's bound |gpu - model| <= 2^-23 |model| + 1e-12 max|A|, A over the amplitudes and the vorticity amplitudes
    as the synthesis scales them (velocities and vorticity by v_scale)."""
    scale = np.array([1.0, 1.0, 1.0, 1.0, v_scale, v_scale, v_scale])[:, None]
    top = np.nanmax(np.abs(np.asarray(amp, dtype=np.float64) * scale))
    if vort is not None:
        top = max(top, np.nanmax(np.abs(np.asarray(vort, dtype=np.float64) * v_scale)))
    return 2.0 ** -23 * np.abs(model) + 1e-12 * top


def nonuniform_radii(rng, lo, hi, n):
    """n ascending radii from lo to hi exactly, spacings between 0.4 and 1.6 of the mean."""
    h = rng.uniform(0.4, 1.6, n - 1)
    r = lo + (hi - lo) * np.concatenate(([0.0], np.cumsum(h))) / np.sum(h)
    r[-1] = hi
    return r


def smooth_table(n_nodes, n_ext, seed=5):
    """Smooth synthetic amplitudes on non-uniform radii 0.15 .. 1 .. 3, the boundary radius 1.0 twice; xi_phi, xi_z,
    v_phi and v_z jump at the interface."""
    rng = np.random.default_rng(seed)
    radius = np.concatenate((nonuniform_radii(rng, 0.15, 1.0, n_nodes),
                             nonuniform_radii(rng, 1.0, 3.0, n_ext) if n_ext else []))
    r = radius
    amp = np.stack([np.sin(2 * r) + 0.5, r * np.cos(1.5 * r), r * r * np.exp(-r), np.cos(r) + 2.0,
                    0.7 * np.cos(2.2 * r) + 0.2, r * np.sin(1.7 * r) + 0.4, np.exp(-0.5 * r) * (1 + r * r)])
    amp[:, n_nodes:] *= np.array([1.0, -0.6, 1.7, 1.0, 1.0, 0.45, -1.3])[:, None]
    return radius, amp


FD_NAMES = ["v_x", "v_y", "v_z", "vort_x", "vort_y", "vort_z"]


def fd_curl_error(frames, names, x, y, z):
    """max |curl_fd(v) - vort| over the mesh and the three components, relative to the largest |vort| component; frames
    [n_sel, n_z, n_y, n_x] of one time, curl by np.gradient with the mesh coordinates (second order, ends included)."""
    f = {v: np.asarray(frames[i], dtype=np.float64) for i, v in enumerate(names)}
    g = lambda a: np.gradient(a, z, y, x, edge_order=2)                       # noqa: E731  -> d/dz, d/dy, d/dx
    dvx, dvy, dvz = g(f["v_x"]), g(f["v_y"]), g(f["v_z"])
    curl = {"vort_x": dvz[1] - dvy[0], "vort_y": dvx[0] - dvz[2], "vort_z": dvy[2] - dvx[1]}
    top = max(np.max(np.abs(f[c])) for c in curl)
    return max(np.max(np.abs(curl[c] - f[c])) for c in curl) / top


def read_vtk_rectilinear(path, names):
    """(x, y, z, {name: [n_z, n_y, n_x] float32}) of a file written by postprocess.write_vtk_rectilinear; every header
    line is checked on the way."""
    raw = open(path, "rb").read()
    pos = 0

    def line():
        nonlocal pos
        end = raw.index(b"\n", pos)
        s = raw[pos:end].decode()
        pos = end + 1
        return s

    def block(count):
        nonlocal pos
        a = np.frombuffer(raw, dtype=">f4", count=count, offset=pos).astype(np.float32)
        pos += 4 * count
        assert raw[pos:pos + 1] == b"\n"
        pos += 1
        return a

    assert [line() for _ in range(4)] == ["# vtk DataFile Version 3.0", "vtk output", "BINARY", "DATASET RECTILINEAR_GRID"]
    dims = line().split()
    assert dims[0] == "DIMENSIONS"
    nx, ny, nz = (int(v) for v in dims[1:])
    axes = []
    for axis, n in zip("XYZ", (nx, ny, nz)):
        assert line() == f"{axis}_COORDINATES {n} float"
        axes.append(block(n))
    assert line() == f"POINT_DATA {nx * ny * nz}"
    out = {}
    for name in names:
        assert line() == f"SCALARS {name} float"
        assert line() == "LOOKUP_TABLE default"
        out[name] = block(nx * ny * nz).reshape(nz, ny, nx)
    assert pos == len(raw)
    return axes[0], axes[1], axes[2], out


def min_distance_to_region_edges(radius, n_nodes, x, y):
    """min over the mesh of |r - radius[0]|, |r - boundary radius|, |r - radius[n_r-1]|: where a point this close to an
    edge would change region by rounding (a selection flip, not a rounding error)."""
    r = np.hypot(np.asarray(x)[None, :], np.asarray(y)[:, None])
    edges = [radius[0], radius[n_nodes - 1], radius[-1]]
    return float(min(np.min(np.abs(r - e)) for e in edges))
