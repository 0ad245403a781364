"""Host side of the shooting path: builds the es_shoot_desc / profile tables from an equilibrium object and calls
the HIP kernels through the C ABI (es_problem_create, es_shoot_eval_grid, es_shoot_eval_points,
es_shoot_find_roots)."""
import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _lib
from . import equilibrium as eqm

GEOM_CYL, GEOM_CYL_TWIST, GEOM_SLAB_DENSITY, GEOM_SLAB_FLOW = 0, 1, 2, 3
AXIS_KINK, AXIS_SAUSAGE, AXIS_ROTATION_KINK = 0, 1, 2
W_ABSOLUTE, W_PHASE_SPEED, W_PER_ROW = 0, 1, 2
PT_OK, PT_LEAKY, PT_NONFINITE, PT_CONTINUUM = 0, 1, 2, 3
# refinement rule of the context every search below picks up (Context.refine_rule, Context.refine_stats)
from ._lib import REFINE_SECTION, REFINE_HYBRID, RefineStats  # noqa: E402,F401


class ScreenCounts(NamedTuple):
    """The count words of find_roots_screened_async / find_roots_mixed_async, read on the host."""
    count: int          # brackets (may exceed the table capacity)
    unsure: int         # fp64 re-evaluations of unsure grid points
    ends: int           # fp64 re-evaluations of bracket ends
    violations: int     # brackets whose fp64 ends do not confirm them
    overflow: bool      # count > capacity: only the first `capacity` brackets were written and refined


class ModeSignature(NamedTuple):
    """es_shoot_mode_signature: one entry per (k, omega) pair, CUDA tensors.  (nodes_value, nodes_flux) is the branch label
    of a root; a pair that is not PT_OK carries -1 in the four integer fields and NaN in the two peaks."""
    nodes_value: object       # int32: sign changes of value (P / Vx) over the interior nodes
    nodes_flux: object        # int32: sign changes of flux (xi_r / P_T)
    peak_node_value: object   # int32: smallest node index that attains max|value| (node 0 = boundary)
    peak_node_flux: object
    peak_value: object        # float64: max|value|, exterior boundary value = +-1 (1.0 at node 0: a surface-like mode)
    peak_flux: object
    status: object            # uint8: PT_* of the exterior


class RootSlopes(NamedTuple):
    """es_shoot_root_slopes: the two sides of the matching condition with their exact partial derivatives, CUDA tensors.
    outer, inner are [3, n] (value, d/d omega, d/dk); d, d_w, d_k [n] are D = outer - inner and its derivatives.  A pair
    that is not PT_OK, or whose outputs are not finite, carries NaN throughout."""
    outer: object
    inner: object
    d: object
    d_w: object
    d_k: object
    status: object            # uint8: PT_* of the exterior

    @property
    def group_velocity(self):
        """d omega / dk along the branch through each pair: -D_k / D_w."""
        return -self.d_k / self.d_w

    @property
    def newton_dw(self):
        """The Newton correction -D / D_w: how far in omega each pair lies from the root of its row."""
        return -self.d / self.d_w


class RootCurvature(NamedTuple):
    """es_shoot_root_curvature: RootSlopes with the exact second partial derivatives, CUDA tensors.  outer, inner are [6, n]
    (value, d/d omega, d/dk, d2/d omega2, d2/d omega dk, d2/dk2); the other fields [n] are D = outer - inner and its
    derivatives.  A pair that is not PT_OK, or whose outputs are not finite, carries NaN throughout."""
    outer: object
    inner: object
    D: object
    D_w: object
    D_k: object
    D_ww: object
    D_wk: object
    D_kk: object
    status: object            # uint8: PT_* of the exterior

    @property
    def group_velocity(self):
        """d omega / dk along the branch through each pair: -D_k / D_w."""
        return -self.D_k / self.D_w

    @property
    def curvature(self):
        """d2 omega / dk2 = d c_g / dk along the branch through each pair: -(D_kk + 2 D_wk c_g + D_ww c_g^2) / D_w."""
        cg = self.group_velocity
        return -(self.D_kk + 2.0 * self.D_wk * cg + self.D_ww * cg * cg) / self.D_w

    @property
    def newton_dw(self):
        """The Newton correction -D / D_w."""
        return -self.D / self.D_w

    @property
    def halley_dw(self):
        """The Halley correction -2 D D_w / (2 D_w^2 - D D_ww): Newton's with the curvature of D in omega taken along."""
        return -2.0 * self.D * self.D_w / (2.0 * self.D_w * self.D_w - self.D * self.D_ww)


class TracedBranches(NamedTuple):
    """ShootProblem.trace_branches: `branches` {label: dict of CUDA tensors k, w, dwdk, resid, iters, flag, status, predicted,
    max_shift}, views into the tensors of the one Newton launch; `skipped` the labels that were not traced (a single row,
    or wavenumbers that repeat: two roots of a row share the label)."""
    branches: dict
    skipped: list


def _host_array(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def hermite_guess(k, w, s, k_fine, shift_factor=4.0):
    """The prediction a Newton trace starts from, on the device, for real or complex roots: k [n] strictly increasing
    (float64), the roots w [n] on it with their slopes s = d omega / dk, k_fine [m] -- CUDA tensors.  Returns
    (predicted [m], bound [m]): the piecewise-cubic Hermite interpolant at k_fine (the cubic of the end interval continued
    outside [k[0], k[-1]]) and, per fine point, the shift bound of its coarse interval [k_j, k_j+1]: shift_factor times the
    larger of the interval's two end-point Hermite defects
        |w_j+1 - w_j - h s_j|,  |w_j+1 - w_j - h s_j+1|      (h = k_j+1 - k_j)
    -- how far the tangent from one end misses the root at the other, a scale for how far the curve bends inside the
    interval and so for how far the cubic can lie from it -- and no less than 1e-8 max(1, |w_j|)."""
    import torch
    j = torch.clamp(torch.searchsorted(k, k_fine, right=True) - 1, 0, k.numel() - 2)
    return hermite_guess_in(k, w, s, j, k_fine, shift_factor)


def hermite_guess_in(k, w, s, j, k_fine, shift_factor=4.0):
    """hermite_guess with the coarse interval [k_j, k_j+1] of every fine point given (int64 [m]): k need then be increasing
    only inside the intervals that are used, so several branches can lie one after the other in k, w and s."""
    import torch
    h = k[1:] - k[:-1]
    hj = h[j]
    t = (k_fine - k[j]) / hj
    t2, t3 = t * t, t * t * t
    pred = ((2 * t3 - 3 * t2 + 1) * w[j] + (t3 - 2 * t2 + t) * hj * s[j]
            + (-2 * t3 + 3 * t2) * w[j + 1] + (t3 - t2) * hj * s[j + 1])
    dw = w[1:] - w[:-1]
    defect = torch.maximum((dw - h * s[:-1]).abs(), (dw - h * s[1:]).abs())
    bound = torch.maximum(shift_factor * defect, 1e-8 * torch.clamp(w[:-1].abs(), min=1.0))[j]
    return pred, bound


def read_screen_counts(counts, capacity):
    """Read the four count words once (a CUDA tensor: this is the host synchronisation the async calls leave to the
    caller; a CPU tensor works the same).  Raises EsError, naming the failure of the synchronous call's
    ES_ERR_SCREENING, when a bracket was not confirmed by the fp64 values at its ends."""
    c = [int(x) for x in counts.reshape(-1)[:4].tolist()]
    assert len(c) == 4, "counts must have four words"
    r = ScreenCounts(c[0], c[1], c[2], c[3], c[0] > int(capacity))
    if r.violations > 0:
        raise _lib.EsError("libeigensolver_amd: fp32-screened bracket not confirmed in fp64 (fp32 screening: "
                           f"{r.violations} bracket(s) not confirmed by the fp64 values at their ends)")
    return r


def audit_arrays(ctx, D_scr, st_scr, D64, st64, rel64=None, capacity=1024, rows=None):
    """es_shoot_audit_screening on (nk, nw) CUDA tensors: the screened grid (float64 D_scr, uint8 st_scr) against the fp64
    grid (D64, st64, optional rel64) -> _lib.ScreenAudit.  capacity bounds the table of flagged cells (0: counts only).
    rows[i] is the row of the caller's full grid that row i of the arrays holds (None: the arrays are the full grid).
    The call itself is asynchronous; reading the report is the host synchronisation."""
    import torch
    nk, nw = D64.shape
    for t, dt in ((D_scr, torch.float64), (st_scr, torch.uint8), (D64, torch.float64), (st64, torch.uint8)):
        assert t.is_cuda and t.dtype == dt and tuple(t.shape) == (nk, nw), "the four grids are (nk, nw) CUDA tensors"
    assert rel64 is None or (rel64.is_cuda and rel64.dtype == torch.float64 and tuple(rel64.shape) == (nk, nw))
    cap = int(capacity)
    counts = torch.empty(10, dtype=torch.int64, device=D64.device)
    worst = torch.empty(2, dtype=torch.float64, device=D64.device)
    cell = torch.empty(cap, dtype=torch.int64, device=D64.device) if cap > 0 else None
    kind = torch.empty(cap, dtype=torch.uint8, device=D64.device) if cap > 0 else None
    D_scr, st_scr, D64, st64 = (t.contiguous() for t in (D_scr, st_scr, D64, st64))
    rel64 = rel64.contiguous() if rel64 is not None else None
    rc = ctx.lib.es_shoot_audit_screening(ctx.handle, nk, nw, _lib.ptr(D_scr), _lib.ptr(st_scr), _lib.ptr(D64),
                                          _lib.ptr(st64), _lib.ptr(rel64) if rel64 is not None else None, cap,
                                          _lib.ptr(cell) if cap > 0 else None, _lib.ptr(kind) if cap > 0 else None,
                                          _lib.ptr(counts), _lib.ptr(worst))
    _lib.check(ctx.handle, rc)
    c = [int(x) for x in counts.tolist()]
    wv = worst.tolist()
    n = min(c[0], cap)
    cells = cell[:n].cpu().numpy() if cap > 0 else np.zeros(0, dtype=np.int64)
    kinds = kind[:n].cpu().numpy() if cap > 0 else np.zeros(0, dtype=np.uint8)
    full_row = (lambda r: r) if rows is None else (lambda r: np.asarray(rows, dtype=np.int64)[r])
    at = lambda x: None if x < 0 else (int(full_row(x // nw)), int(x % nw))     # noqa: E731
    return _lib.ScreenAudit(*c[:8], float(wv[0]), at(c[8]), float(wv[1]), at(c[9]),
                            full_row(cells // max(nw, 1)), cells % max(nw, 1), kinds)


def _mask_of(table, variables, what):
    """Bit mask of `variables` (None: all) over the name tuple `table` and the names in ascending bit order, the order
    in which a synthesis call stores them."""
    names = list(table) if variables is None else list(variables)
    unknown = [v for v in names if v not in table]
    if unknown:
        raise ValueError(f"unknown {what}(s) {unknown}: choose from {table}")
    mask = 0
    for v in names:
        mask |= 1 << table.index(v)
    return mask, [v for b, v in enumerate(table) if (mask >> b) & 1]


def _frames_out(out, shape, device):
    """The float32 frames tensor of a synthesis call: allocated, or the caller's `out` checked."""
    import torch
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=device)
    assert out.shape == shape and out.dtype == torch.float32 and out.is_contiguous()
    return out


def _frame_chunks(synth, t, frames_per_call, names, **mesh):
    """The dict of a fields call (mesh entries, t, names, frames, <name>: frames[:, i]), or with frames_per_call the
    generator of such dicts, at most that many frames each.  synth(t_part, carry) -> (frames, carry); carry is a dict of
    further entries that a chunk hands on to the next one (None before the first)."""
    def one(t_part, carry):
        out, carry = synth(t_part, carry)
        d = dict(carry, **mesh, t=t_part, names=names, frames=out)
        d.update({v: out[:, i] for i, v in enumerate(names)})
        return d, carry

    if frames_per_call is None:
        return one(t, None)[0]
    step = int(frames_per_call)
    if step < 1:
        raise ValueError("frames_per_call must be >= 1")

    def chunks():
        carry = None
        for a in range(0, t.numel(), step):
            d, carry = one(t[a:a + step], carry)
            yield d
    return chunks()


def var_mask(variables):
    """Mask of es_cyl_field_synthesis and the names in the order it stores them (ascending bit, _lib.VAR_NAMES)."""
    return _mask_of(_lib.VAR_NAMES, variables, "field variable")


def field_profiles(eq, r, reference_quirks=True):
    """The es_field_profiles arrays of cylinder equilibrium `eq` at the radii r (> 0) as NumPy arrays, formed as
    es_problem_create forms the determinant's (bA = B_z/sqrt(rho), qc = c^2/(c^2 + vA^2) with vA as written, CF:173-174).
    reference_quirks: q is the constant c_i0^2/(c_i0^2 + vA_i0^2) and s_z = d(v_z/r)/dr, as the export scripts write
    them (Export_vtk.py:780, :812-813); otherwise the local ratio and dv_z/dr."""
    r = np.ascontiguousarray(r, dtype=np.float64)
    rho, Bz, Bphi, c2 = eq.rho(r), eq.B_z(r), eq.B_phi(r), eq.c2(r)
    sr = np.sqrt(rho)
    vA = (Bz + Bphi) / sr
    qc = c2 / (c2 + vA * vA)
    out = dict(r=r, rho=rho, Bz=Bz, Bphi=Bphi, vz=eq.v_z(r), vphi=eq.v_phi(r), bA=Bz / sr, qc=qc,
               s_phi=eq.dv_phi_over_r_dr(r))
    if reference_quirks:
        out["q"] = np.full_like(r, eq.c_i0 ** 2 / (eq.c_i0 ** 2 + eq.vA_i0 ** 2))
        out["s_z"] = eq.dv_z_over_r_dr(r)
    else:
        out["q"] = qc
        out["s_z"] = eq.dv_z_dr(r)
    return {n: np.ascontiguousarray(out[n], dtype=np.float64) for n in _lib._FIELD_PROFILE_FIELDS}


def field_synthesis(ctx, radius, amp, m, k, w, theta, z, t, variables=None, v_scale=1.0, flags=0, want_points=True,
                    out=None):
    """es_cyl_field_synthesis for the amplitude table of one mode (radius [n_r], amp [7, n_r], CUDA float64): float32
    frames out[n_t, n_sel, n_z, n_theta, n_r] in the order of var_mask(variables)[1] and, with want_points, the mesh
    points[n_z, n_theta, n_r, 3].  theta, z, t: CUDA float64 vectors.  `out`: a preallocated contiguous float32 tensor
    of that shape (4-byte alignment suffices).  Enqueued on the context's stream; returns (out, points, names)."""
    return _field_synthesis(_REAL_TABLES, ctx, radius, amp, m, k, w, theta, z, t, variables, v_scale, flags, want_points, out)


def cartesian_var_mask(variables):
    """Mask of es_cyl_cartesian_synthesis and the names in the order it stores them (ascending bit, _lib.CVAR_NAMES)."""
    return _mask_of(_lib.CVAR_NAMES, variables, "Cartesian field variable")


def vorticity_amplitudes(ctx, radius, amp, n_nodes, n_ext, m, k):
    """es_cyl_vorticity_amplitudes on the tables of es_cyl_polarisation (radius [n, n_r], amp [n, 7, n_r], k [n], CUDA
    float64, n_r = n_nodes + n_ext): the five radial amplitudes of curl v, vort [n, 5, n_r] in the order _lib.VORT_NAMES.
    Enqueued on the context's stream."""
    return _vorticity_amplitudes(_REAL_TABLES, ctx, radius, amp, n_nodes, n_ext, m, k)


def cartesian_synthesis(ctx, radius, amp, vort, n_nodes, n_ext, m, k, w, x, y, z, t, variables=None, v_scale=1.0,
                        fill=float("nan"), flags=0, out=None):
    """es_cyl_cartesian_synthesis for the tables of one mode (radius [n_r], amp [7, n_r], vort [5, n_r] or None, CUDA
    float64): float32 frames out[n_t, n_sel, n_z, n_y, n_x] in the order of cartesian_var_mask(variables)[1].  x, y, z,
    t: CUDA float64 vectors.  `out`: a preallocated contiguous float32 tensor of that shape (4-byte alignment suffices).
    Enqueued on the context's stream; returns (out, names)."""
    return _cartesian_synthesis(_REAL_TABLES, ctx, radius, amp, vort, n_nodes, n_ext, m, k, w, x, y, z, t, variables, v_scale,
                                fill, flags, out)


class _Tables(NamedTuple):
    """The two kinds of amplitude tables the field entry points of a cylinder mode take, and what differs between their
    wrappers: real tables at real omega (C ABI sections 7 and 8), complex ones at complex omega (sections 16 and 20)."""
    prefix: str                                     # <prefix>field_synthesis, vorticity_amplitudes, cartesian_synthesis
    dtype: str                                      # torch dtype of amp and vort
    n_vort: int                                     # vorticity channels: _lib.VORT_NAMES / _lib.CVORT_NAMES
    w_pair: bool                                    # omega goes in as (re, im), not as one double

    def call(self, ctx, name, *args):
        _lib.check(ctx.handle, getattr(ctx.lib, self.prefix + name)(ctx.handle, *args))

    def w_args(self, w):
        return (complex(w).real, complex(w).imag) if self.w_pair else (float(w),)


_REAL_TABLES = _Tables("es_cyl_", "float64", 5, False)
_COMPLEX_TABLES = _Tables("es_cyl_complex_", "complex128", 3, True)


def _field_synthesis(tables, ctx, radius, amp, m, k, w, theta, z, t, variables, v_scale, flags, want_points, out):
    import torch
    mask, names = var_mask(variables)
    n_r, n_theta, n_z, n_t = radius.numel(), theta.numel(), z.numel(), t.numel()
    assert amp.shape == (7, n_r) and amp.dtype == getattr(torch, tables.dtype) and radius.dtype == torch.float64
    out = _frames_out(out, (n_t, len(names), n_z, n_theta, n_r), radius.device)
    pts = torch.empty((n_z, n_theta, n_r, 3), dtype=torch.float32, device=radius.device) if want_points else None
    tables.call(ctx, "field_synthesis", _lib.ptr(radius), _lib.ptr(amp), n_r, int(m), float(k), *tables.w_args(w),
                _lib.ptr(theta), n_theta, _lib.ptr(z), n_z, _lib.ptr(t), n_t, mask, float(v_scale), int(flags),
                _lib.ptr(pts) if want_points else None, _lib.ptr(out))
    return out, pts, names


def _vorticity_amplitudes(tables, ctx, radius, amp, n_nodes, n_ext, m, k):
    import torch
    n, n_r = radius.shape
    assert n_r == int(n_nodes) + int(n_ext) and amp.shape == (n, 7, n_r) and k.shape == (n,)
    dtype = getattr(torch, tables.dtype)
    for a, dt in ((radius, torch.float64), (amp, dtype), (k, torch.float64)):
        assert a.is_cuda and a.dtype == dt and a.is_contiguous()
    vort = torch.empty((n, tables.n_vort, n_r), dtype=dtype, device=radius.device)
    tables.call(ctx, "vorticity_amplitudes", _lib.ptr(radius), _lib.ptr(amp), n, int(n_nodes), int(n_ext), int(m),
                _lib.ptr(k), _lib.ptr(vort))
    return vort


def _cartesian_synthesis(tables, ctx, radius, amp, vort, n_nodes, n_ext, m, k, w, x, y, z, t, variables, v_scale, fill, flags,
                         out):
    import torch
    mask, names = cartesian_var_mask(variables)
    n_r = radius.numel()
    assert n_r == int(n_nodes) + int(n_ext) and amp.shape == (7, n_r) and (vort is None or vort.shape == (tables.n_vort, n_r))
    dtype = getattr(torch, tables.dtype)
    for a, dt in ((radius, torch.float64), (amp, dtype), (vort, dtype), (x, torch.float64), (y, torch.float64),
                  (z, torch.float64), (t, torch.float64)):
        assert a is None or (a.is_cuda and a.dtype == dt and a.is_contiguous())
    out = _frames_out(out, (t.numel(), len(names), z.numel(), y.numel(), x.numel()), radius.device)
    tables.call(ctx, "cartesian_synthesis", _lib.ptr(radius), _lib.ptr(amp), _lib.ptr(vort) if vort is not None else None,
                int(n_nodes), int(n_ext), int(m), float(k), *tables.w_args(w), _lib.ptr(x), x.numel(), _lib.ptr(y), y.numel(),
                _lib.ptr(z), z.numel(), _lib.ptr(t), t.numel(), mask, float(v_scale), float(fill), int(flags), _lib.ptr(out))
    return out, names


def _require_exterior_points(n_ext):
    if int(n_ext) != 0 and int(n_ext) < 3:
        raise ValueError(f"n_ext = {n_ext}: the exterior needs at least 3 points (radial derivative and interpolation "
                         "per region), or 0 to leave it out")


def cartesian_split(ctx, n_x, n_y, n_z, n_t):
    """The launch shape of es_cyl_cartesian_synthesis for a mesh (es_cyl_cartesian_split): dict of pieces, z_chunk, z_parts,
    items_per_group, groups."""
    v = [C.c_int(0) for _ in range(5)]
    rc = ctx.lib.es_cyl_cartesian_split(int(n_x), int(n_y), int(n_z), int(n_t), *[C.byref(a) for a in v])
    _lib.check(ctx.handle, rc)
    return dict(zip(("pieces", "z_chunk", "z_parts", "items_per_group", "groups"), (a.value for a in v)))


def slab_var_mask(variables):
    """Mask of es_slab_field_synthesis and the names in the order it stores them (ascending bit, _lib.SVAR_NAMES)."""
    mask, names = _mask_of(_lib.SVAR_NAMES, variables, "slab field variable")
    if not names:
        raise ValueError(f"empty list of slab field variables: choose from {_lib.SVAR_NAMES}")
    return mask, names


def slab_field_profiles(eq):
    """The es_slab_field_profiles arrays of slab equilibrium `eq` at its N nodes (node 0 is x = -1) as NumPy arrays:
    the equilibrium's own profiles() at every second sample (the others are the mid-points of the march), constants
    where a family has none (the flow slab's rho, c^2, vA^2; the density slab's U = 0, U' = 0)."""
    if not isinstance(eq, eqm._SlabBase):
        raise ValueError("slab field profiles exist for slab equilibria only")
    N = int(eq.n_nodes)
    prof = eq.profiles()
    const = {"rho": eq.rho_i0, "c2": eq.c_i0 ** 2, "vA2": eq.vA_i0 ** 2, "U": 0.0, "dU": 0.0}
    out = {}
    for name in _lib._SLAB_FIELD_PROFILE_FIELDS:
        a = np.asarray(prof[name], dtype=np.float64)[::2] if name in prof else np.full(N, const[name])
        assert a.shape == (N,)
        out[name] = np.ascontiguousarray(a, dtype=np.float64)
    return out


def slab_polarisation(ctx, k, w_re, w_im, eig, prof, rho_e, vA_e, c_e, U_e, parity, flags=0):
    """es_slab_polarisation on the arrays of an eigenfunction call.  k, w_re [n] and w_im [n] or None: CUDA float64; eig:
    the dict of ShootProblem.eigenfunction (float64 arrays) or SlabComplexFlow.eigenfunction (complex128 arrays); prof:
    dict of CUDA float64 arrays [N] named _lib._SLAB_FIELD_PROFILE_FIELDS.  Returns dict of CUDA tensors x [n, n_tab]
    (float64, ascending: left exterior, interior, right exterior, n_tab = 2 n_ext + N) and amp [n, 6, n_tab]
    (complex128, channels _lib.SAMP_NAMES).  Enqueued on the context's stream."""
    import torch
    vi, fi, xe, ve, fe = (eig[a] for a in ("value_int", "flux_int", "x_ext", "value_ext", "flux_ext"))
    n, N = vi.shape
    n_ext = xe.shape[1]
    cplx = vi.dtype == torch.complex128
    for a in (vi, fi, ve, fe):
        assert a.is_cuda and a.is_contiguous() and a.dtype == (torch.complex128 if cplx else torch.float64)
    assert fi.shape == (n, N) and ve.shape == (n, n_ext) and fe.shape == (n, n_ext) and k.shape == (n,) and w_re.shape == (n,)
    assert w_im is None or w_im.shape == (n,)
    assert all(prof[a].shape == (N,) and prof[a].dtype == torch.float64 for a in _lib._SLAB_FIELD_PROFILE_FIELDS)
    fp = _lib.SlabFieldProfiles(*[prof[a].data_ptr() for a in _lib._SLAB_FIELD_PROFILE_FIELDS])
    n_tab = N + 2 * n_ext
    x = torch.empty((n, n_tab), dtype=torch.float64, device=vi.device)
    amp = torch.empty((n, 6, n_tab), dtype=torch.complex128, device=vi.device)
    P = lambda a: _lib.ptr(a) if a is not None and a.numel() else None      # noqa: E731
    rc = ctx.lib.es_slab_polarisation(ctx.handle, P(k), P(w_re), P(w_im), n, N, P(vi), P(fi), n_ext, P(xe), P(ve), P(fe),
                                      1 if cplx else 0, C.byref(fp), float(rho_e), float(vA_e), float(c_e), float(U_e),
                                      int(parity), int(flags), P(x), P(amp))
    _lib.check(ctx.handle, rc)
    return dict(x=x, amp=amp)


def slab_field_synthesis(ctx, xtab, amp, n_nodes, n_ext, k, w, x, z, t, variables=None, v_scale=1.0, fill=float("nan"),
                         flags=0, out=None):
    """es_slab_field_synthesis for the table of one mode (xtab [n_tab] float64, amp [6, n_tab] complex128, CUDA): float32
    frames out[n_t, n_sel, n_z, n_x] in the order of slab_var_mask(variables)[1].  w may be complex.  x, z, t: CUDA float64
    vectors.  `out`: a preallocated contiguous float32 tensor of that shape (4-byte alignment suffices).  Enqueued on the
    context's stream; returns (out, names)."""
    import torch
    mask, names = slab_var_mask(variables)
    n_tab = xtab.numel()
    if n_tab != int(n_nodes) + 2 * int(n_ext) or tuple(amp.shape) != (6, n_tab):
        raise ValueError(f"(n_nodes, n_ext) = ({n_nodes}, {n_ext}) does not match the table: xtab has {n_tab} points, amp "
                         f"the shape {tuple(amp.shape)}; expected 2 n_ext + n_nodes points and (6, that)")
    assert amp.dtype == torch.complex128
    for a in (xtab, x, z, t):
        assert a.is_cuda and a.dtype == torch.float64 and a.is_contiguous()
    assert amp.is_cuda and amp.is_contiguous()
    out = _frames_out(out, (t.numel(), len(names), z.numel(), x.numel()), xtab.device)
    w = complex(w)
    rc = ctx.lib.es_slab_field_synthesis(ctx.handle, _lib.ptr(xtab), _lib.ptr(amp), int(n_nodes), int(n_ext), float(k),
                                         w.real, w.imag, _lib.ptr(x), x.numel(), _lib.ptr(z), z.numel(), _lib.ptr(t),
                                         t.numel(), mask, float(v_scale), float(fill), int(flags), _lib.ptr(out))
    _lib.check(ctx.handle, rc)
    return out, names


def slab_frames(ctx, xtab, amp, n_nodes, n_ext, k, w, dx, dz, dt, names, v_scale, fill, big_endian, frames_per_call):
    """The dict (or, with frames_per_call, the generator of dicts) that ShootProblem.slab_fields and
    SlabComplexFlow.fields return, from the table of one mode."""
    flags = _lib.FIELD_BIG_ENDIAN if big_endian else 0

    def synth(t_part, _):
        return slab_field_synthesis(ctx, xtab, amp, n_nodes, n_ext, k, w, dx, dz, t_part, names, v_scale, fill, flags)[0], {}

    return _frame_chunks(synth, dt, frames_per_call, names, x=dx, z=dz)


def make_desc(eq, mode, m=None):
    """es_shoot_desc + profile dict for equilibrium `eq` and mode "kink" / "sausage" (azimuthal order m for
    cylinders defaults to the reference's 1 / 0)."""
    d = _lib.ShootDesc()
    d.n_nodes = int(eq.n_nodes)
    d.x_boundary, d.x_end = float(eq.x_boundary), float(eq.x_end)
    d.rho_e, d.vA_e, d.c_e, d.cT_e, d.U_e = eq.rho_e, eq.vA_e, eq.c_e, eq.cT_e, eq.U_e
    d.L_factor = eq.L_factor
    d.ic_value, d.ic_slope = eq.ic
    prof = eq.profiles()
    if isinstance(eq, eqm._CylinderBase):
        d.geometry = GEOM_CYL_TWIST if eq.twisted else GEOM_CYL
        mm = (1 if mode == "kink" else 0) if m is None else int(m)
        d.m = mm
        d.m_ext = mm                      # the reference hard-codes 1 / 0 in the exterior ODE (CF:769, :1065)
        if mode == "sausage":
            d.axis_bc = AXIS_SAUSAGE
        elif eq.twisted:
            d.axis_bc = AXIS_ROTATION_KINK
        else:
            d.axis_bc = AXIS_KINK
        d.c1_power = eq.c1_power
        d.bc_const = eq.bc_const(d.axis_bc)
    elif isinstance(eq, eqm.SlabDensity):
        d.geometry = GEOM_SLAB_DENSITY
        d.slab_mode = 0 if mode == "sausage" else 1
    elif isinstance(eq, eqm.SlabFlow):
        d.geometry = GEOM_SLAB_FLOW
        d.slab_mode = 0 if mode == "sausage" else 1
        d.c_i, d.vA_i, d.rho_i = eq.c_i0, eq.vA_i0, eq.rho_i0
    else:
        raise TypeError(type(eq))
    return d, prof


class ShootProblem:
    """One reference worker configuration resident on the GPU (profile tables in HBM)."""

    def __init__(self, eq, mode, m=None, ctx=None, accept_norm=0):
        """accept_norm = 1: `rel` is normalised by |outer| only (CR-KS:722) instead of max(|outer|, |inner|)."""
        self.ctx = ctx if ctx is not None else _lib.Context()
        self.eq, self.mode = eq, mode
        self.desc, prof = make_desc(eq, mode, m)
        self.desc.accept_norm = int(accept_norm)
        self._prof_np = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in prof.items()}
        p = _lib.Profiles()
        for name in _lib._PROFILE_FIELDS:
            a = self._prof_np.get(name)
            setattr(p, name, a.ctypes.data if a is not None else None)
        h = C.c_void_p()
        st = self.ctx.lib.es_problem_create(self.ctx.handle, C.byref(self.desc), C.byref(p), C.byref(h))
        _lib.check(self.ctx.handle, st)
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.es_problem_destroy(self.ctx.handle, self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _dev(self, a):
        import torch
        dev = f"cuda:{self.ctx.device}"
        if isinstance(a, torch.Tensor):
            return a.to(device=dev, dtype=torch.float64).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)

    def _grid_args(self, k, w, w_mode):
        """(dk, dw, nk, nw): k and omega on the device and the grid size, as every grid entry point takes them."""
        dk, dw = self._dev(k).reshape(-1), self._dev(w)
        return dk, dw, dk.numel(), dw.shape[-1] if w_mode == W_PER_ROW else dw.numel()

    def eval_grid(self, k, w, w_mode=W_PHASE_SPEED, want_rel=False, skip_continuum=False):
        """D[ik, iw], status[ik, iw] (and rel) on the (k, omega) grid; w_mode selects how omega is formed.
        skip_continuum: ES_EVAL_SKIP_CONTINUUM -- points inside a continuum band get D = NaN and are not marched."""
        import torch
        dk, dw, nk, nw = self._grid_args(k, w, w_mode)
        if w_mode == W_PER_ROW:
            assert dw.numel() == nk * nw
        D = torch.empty((nk, nw), dtype=torch.float64, device=dk.device)
        st = torch.empty((nk, nw), dtype=torch.uint8, device=dk.device)
        rel = torch.empty((nk, nw), dtype=torch.float64, device=dk.device) if want_rel else None
        rc = self.ctx.lib.es_shoot_eval_grid_ex(self.ctx.handle, self.handle, _lib.ptr(dk), nk, _lib.ptr(dw), nw,
                                                w_mode, 1 if skip_continuum else 0, _lib.ptr(D),
                                                _lib.ptr(rel) if want_rel else None, _lib.ptr(st))
        _lib.check(self.ctx.handle, rc)
        return (D, st, rel) if want_rel else (D, st)

    def grid_kernel_name(self, nw):
        """The instantiation of the grid kernel es_shoot_eval_grid launches for rows of nw frequencies (es_shoot_grid_shape),
        spelled as tools/codeobj_table.py and rocprofv3 print it."""
        pts, wpe, trk = C.c_int(0), C.c_int(0), C.c_int(0)
        _lib.check(self.ctx.handle, self.ctx.lib.es_shoot_grid_shape(self.ctx.handle, self.handle, int(nw), C.byref(pts),
                                                                     C.byref(wpe), C.byref(trk)))
        if pts.value < 0:                                   # two k-rows per workgroup (es_shoot_grid_shape)
            return f"shoot_grid_kernel_r2<{int(self.desc.geometry)},{-pts.value},{'true' if trk.value else 'false'},{wpe.value}>"
        return f"shoot_grid_kernel<{int(self.desc.geometry)},{pts.value},256,{'true' if trk.value else 'false'},{wpe.value}>"

    def eval_points(self, k, w, want_rel=False):
        import torch
        dk, dw = self._dev(k).reshape(-1), self._dev(w).reshape(-1)
        n = dk.numel()
        assert dw.numel() == n
        D = torch.empty(n, dtype=torch.float64, device=dk.device)
        st = torch.empty(n, dtype=torch.uint8, device=dk.device)
        rel = torch.empty(n, dtype=torch.float64, device=dk.device) if want_rel else None
        rc = self.ctx.lib.es_shoot_eval_points(self.ctx.handle, self.handle, _lib.ptr(dk), _lib.ptr(dw), n,
                                               _lib.ptr(D), _lib.ptr(rel) if want_rel else None, _lib.ptr(st))
        _lib.check(self.ctx.handle, rc)
        return (D, st, rel) if want_rel else (D, st)

    def eigenfunction(self, k, w, n_ext=500):
        """Two-region solution at the (k, omega) pairs: dict of CUDA tensors x_int [N], value_int/flux_int [n, N],
        x_ext/value_ext/flux_ext [n, n_ext] (cylinders: P and xi_r; slabs: Vx and P_T), exterior boundary value +-1."""
        import torch
        dk, dw = self._dev(k).reshape(-1), self._dev(w).reshape(-1)
        n, N = dk.numel(), int(self.desc.n_nodes)
        dev = dk.device
        vi = torch.empty((n, N), dtype=torch.float64, device=dev)
        fi = torch.empty((n, N), dtype=torch.float64, device=dev)
        xe = torch.empty((n, n_ext), dtype=torch.float64, device=dev)
        ve = torch.empty((n, n_ext), dtype=torch.float64, device=dev)
        fe = torch.empty((n, n_ext), dtype=torch.float64, device=dev)
        rc = self.ctx.lib.es_shoot_eigenfunction(self.ctx.handle, self.handle, _lib.ptr(dk), _lib.ptr(dw), n,
                                                 _lib.ptr(vi), _lib.ptr(fi), int(n_ext), _lib.ptr(xe), _lib.ptr(ve),
                                                 _lib.ptr(fe))
        _lib.check(self.ctx.handle, rc)
        x_int = torch.linspace(self.desc.x_boundary, self.desc.x_end, N, dtype=torch.float64, device=dev)
        return dict(x_int=x_int, value_int=vi, flux_int=fi, x_ext=xe, value_ext=ve, flux_ext=fe)

    def mode_signature(self, k, w, count=None):
        """es_shoot_mode_signature at the (k, omega) pairs: the sign changes of the interior value and flux rows of
        `eigenfunction`, their peaks and the nodes of the peaks, reduced inside the march -> ModeSignature.  Nothing is
        written per node and nothing is read back.  count: an int32 CUDA tensor of one element holding the number of valid
        pairs (the count word of find_roots_async, or the four words of the screened searches, whose first is the count);
        entries past min(count, n) are left as allocated."""
        import torch
        dk, dw = self._dev(k).reshape(-1), self._dev(w).reshape(-1)
        n = dk.numel()
        assert dw.numel() == n
        if count is not None:
            assert count.is_cuda and count.numel() >= 1 and count.dtype == torch.int32
        ints = [torch.empty(n, dtype=torch.int32, device=dk.device) for _ in range(4)]
        peaks = [torch.empty(n, dtype=torch.float64, device=dk.device) for _ in range(2)]
        st = torch.empty(n, dtype=torch.uint8, device=dk.device)
        rc = self.ctx.lib.es_shoot_mode_signature(self.ctx.handle, self.handle, _lib.ptr(dk), _lib.ptr(dw), n,
                                                  _lib.ptr(count) if count is not None else None,
                                                  *[_lib.ptr(t) for t in ints + peaks], _lib.ptr(st))
        _lib.check(self.ctx.handle, rc)
        return ModeSignature(*ints, *peaks, st)

    def label_roots(self, roots, count=None):
        """ModeSignature of every entry of a root table: `roots` is the dict find_roots / find_roots_mixed return, or the
        (dict, RootTable) of alloc_root_table filled by an _async search together with its device count word (no read-back:
        the launch is sized for the capacity and takes the count on the device)."""
        t = roots[0] if isinstance(roots, tuple) else roots
        return self.mode_signature(t["k"], t["w"], count=count)

    def root_slopes(self, k, w, count=None):
        """es_shoot_root_slopes at the (k, omega) pairs: the determinant of eval_points with its exact derivatives in omega
        and k (a tangent-linear march, no difference step) -> RootSlopes.  count as in mode_signature: entries past
        min(count, n) are left as allocated.  Nothing is read back."""
        import torch
        dk, dw = self._dev(k).reshape(-1), self._dev(w).reshape(-1)
        n = dk.numel()
        assert dw.numel() == n
        if count is not None:
            assert count.is_cuda and count.numel() >= 1 and count.dtype == torch.int32
        outer = torch.empty((3, n), dtype=torch.float64, device=dk.device)
        inner = torch.empty((3, n), dtype=torch.float64, device=dk.device)
        st = torch.empty(n, dtype=torch.uint8, device=dk.device)
        rc = self.ctx.lib.es_shoot_root_slopes(self.ctx.handle, self.handle, _lib.ptr(dk), _lib.ptr(dw), n,
                                               _lib.ptr(count) if count is not None else None, _lib.ptr(outer),
                                               _lib.ptr(inner), _lib.ptr(st))
        _lib.check(self.ctx.handle, rc)
        diff = outer - inner
        return RootSlopes(outer, inner, diff[0], diff[1], diff[2], st)

    def group_velocity(self, roots, count=None):
        """d omega / dk of every entry of a root table (the forms label_roots takes): -D_k / D_w, a CUDA tensor."""
        t = roots[0] if isinstance(roots, tuple) else roots
        return self.root_slopes(t["k"], t["w"], count=count).group_velocity

    # ---- Newton tracing (C ABI section 13) ---------------------------------------------------------------------------
    def newton(self, k, w0, max_iter=8, step_cap=None, max_shift=None, tol_percent=None, count=None):
        """es_shoot_newton from the guesses w0 at fixed k (broadcast against w0; tensors are taken as they are): dict of CUDA
        tensors w, resid (percent), iters, flag (int32), dwdk (-D_k / D_w at the final w) and status (uint8, that of
        eval_points at the final pair).  step_cap caps the length of a step, max_shift the distance |w - w0| an accepted
        root may have travelled (both default to no limit); tol_percent defaults to the 1e-3 of find_roots.  flag = 1: the
        iteration met no leaky or singular point, the final point is PT_OK, resid < tol_percent and |w - w0| <= max_shift.
        count as in mode_signature.  Nothing is read back."""
        import torch
        dmax = np.finfo(np.float64).max
        g = self._dev(w0).reshape(-1)
        dk = torch.broadcast_to(self._dev(k).reshape(-1), g.shape).contiguous()
        n, dev = g.numel(), g.device
        if count is not None:
            assert count.is_cuda and count.numel() >= 1 and count.dtype == torch.int32
        w, resid, dwdk = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
        iters, flag = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        rc = self.ctx.lib.es_shoot_newton(self.ctx.handle, self.handle, _lib.ptr(dk), _lib.ptr(g), n,
                                          _lib.ptr(count) if count is not None else None, int(max_iter),
                                          dmax if step_cap is None else min(float(step_cap), dmax),
                                          dmax if max_shift is None else min(float(max_shift), dmax),
                                          1e-3 if tol_percent is None else float(tol_percent), _lib.ptr(w), _lib.ptr(resid),
                                          _lib.ptr(dwdk), _lib.ptr(iters), _lib.ptr(flag), _lib.ptr(st))
        _lib.check(self.ctx.handle, rc)
        return dict(w=w, resid=resid, iters=iters, flag=flag, dwdk=dwdk, status=st)

    def _newton_from_prediction(self, kf, pred, bound, newton_kw):
        """newton from the Hermite prediction; without a max_shift of the caller's the flag is cleared, on the device, where
        |w - predicted| exceeds the bound of the point's coarse interval."""
        import torch
        given = newton_kw.get("max_shift") is not None
        out = self.newton(kf, pred, **newton_kw)
        if given:
            out["max_shift"] = torch.full_like(kf, float(newton_kw["max_shift"]))
        else:
            out["flag"] = torch.where((out["w"] - pred).abs() <= bound, out["flag"], torch.zeros_like(out["flag"]))
            out["max_shift"] = bound
        out["k"] = kf
        out["predicted"] = pred
        return out

    def densify(self, k, w, k_fine, cg=None, shift_factor=4.0, **newton_kw):
        """One branch traced to the wavenumbers k_fine from a coarse scan: k strictly increasing with the roots w on it, as
        SlabComplexFlow.densify does for complex roots.  (1) root_slopes at the coarse roots unless their group speed cg is
        given, (2) the piecewise-cubic Hermite prediction at k_fine (hermite_guess), formed on the device, (3) one newton
        call over all fine points.  Dict of CUDA tensors k, w, dwdk, resid, iters, flag, status, predicted and max_shift.
        max_shift: a number from the caller goes to newton as it is; left out, every fine point gets the bound of its coarse
        interval (hermite_guess, shift_factor), newton runs without a limit and the flag is cleared where |w - predicted|
        exceeds the bound.  Nothing is read back."""
        import torch
        with torch.cuda.stream(self.ctx.torch_stream):
            dk, dw, kf = (self._dev(a).reshape(-1) for a in (k, w, k_fine))
            if dk.numel() < 2 or dw.numel() != dk.numel():
                raise ValueError("densify needs at least two coarse rows, one root on each")
            s = self.root_slopes(dk, dw).group_velocity if cg is None else self._dev(cg).reshape(-1)
            pred, bound = hermite_guess(dk, dw, s, kf, shift_factor)
            return self._newton_from_prediction(kf, pred, bound, newton_kw)

    def trace_branches(self, curves, k_fine, check_signature=True, shift_factor=4.0, **newton_kw):
        """Every branch of a coarse scan traced to the wavenumbers k_fine in ONE Newton launch.  curves: the
        {label: (omegas, ks, cg)} of postprocess.curves_with_slopes (host arrays); k_fine: a host array.  For every label
        whose ks are at least two and strictly increasing, the points of k_fine inside [ks[0], ks[-1]] are predicted by the
        branch's Hermite cubic (hermite_guess_in) and handed to newton, all branches in one call, with densify's rule for
        max_shift.  check_signature: one mode_signature call over the traced roots, and the flag is cleared, on the device,
        where (nodes_value, nodes_flux) is not the label of the branch -- a step onto a neighbouring branch.
        Returns TracedBranches(branches, skipped): branches[label] is a dict of views (k, w, dwdk, resid, iters, flag,
        status, predicted, max_shift) into the tensors of the one launch, in the order of the selected k_fine; skipped lists
        the labels with a single row or with repeated ks (two roots of a row sharing a label are never guessed at).
        The host arrays go to the device in one copy from pinned memory that is not waited for; nothing is read back."""
        import torch
        kfh = np.asarray(_host_array(k_fine), dtype=np.float64).reshape(-1)
        spans, skipped, kc, wc, sc, kf, jj, lv, lf = {}, [], [], [], [], [], [], [], []
        n_coarse = n_fine = 0
        for label, (om, ks, cg) in curves.items():
            om, ks, cg = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (om, ks, cg))
            if len(ks) < 2 or not np.all(np.diff(ks) > 0):
                skipped.append(label)
                continue
            sel = kfh[(kfh >= ks[0]) & (kfh <= ks[-1])]
            kc.append(ks); wc.append(om); sc.append(cg); kf.append(sel)
            jj.append(n_coarse + np.clip(np.searchsorted(ks, sel, side="right") - 1, 0, len(ks) - 2))
            lv.append(np.full(len(sel), label[0])); lf.append(np.full(len(sel), label[1]))
            spans[label] = (n_fine, n_fine + len(sel))
            n_coarse += len(ks)
            n_fine += len(sel)
        if not spans:
            return TracedBranches({}, skipped)
        host = np.concatenate([np.concatenate(a).astype(np.float64) for a in (kc, wc, sc, kf, jj, lv, lf)])
        with torch.cuda.stream(self.ctx.torch_stream):
            d = torch.from_numpy(host).pin_memory().to(f"cuda:{self.ctx.device}", non_blocking=True)
            dkc, dwc, dsc, dkf, dj, dlv, dlf = torch.split(d, [n_coarse] * 3 + [n_fine] * 4)
            dkf = dkf.contiguous()
            pred, bound = hermite_guess_in(dkc, dwc, dsc, dj.to(torch.int64), dkf, shift_factor)
            out = self._newton_from_prediction(dkf, pred.contiguous(), bound, newton_kw)
            if check_signature:
                sig = self.mode_signature(dkf, out["w"])
                same = (sig.nodes_value == dlv.to(torch.int32)) & (sig.nodes_flux == dlf.to(torch.int32))
                out["flag"] = torch.where(same, out["flag"], torch.zeros_like(out["flag"]))
        return TracedBranches({label: {key: v[a:b] for key, v in out.items()} for label, (a, b) in spans.items()}, skipped)

    # ---- curvature and group-speed extrema (C ABI section 21) ---------------------------------------------------------
    @staticmethod
    def _check_count(count):
        import torch
        if count is not None:
            assert count.is_cuda and count.numel() >= 1 and count.dtype == torch.int32

    def root_curvature(self, k, w, count=None):
        """es_shoot_root_curvature at the (k, omega) pairs: root_slopes with the exact second derivatives of both sides in
        omega and k (a second-order forward-mode march, no difference step) -> RootCurvature.  count as in mode_signature:
        entries past min(count, n) are left as allocated.  Nothing is read back."""
        import torch
        dk, dw = self._dev(k).reshape(-1), self._dev(w).reshape(-1)
        n = dk.numel()
        assert dw.numel() == n
        self._check_count(count)
        outer = torch.empty((6, n), dtype=torch.float64, device=dk.device)
        inner = torch.empty((6, n), dtype=torch.float64, device=dk.device)
        st = torch.empty(n, dtype=torch.uint8, device=dk.device)
        rc = self.ctx.lib.es_shoot_root_curvature(self.ctx.handle, self.handle, _lib.ptr(dk), _lib.ptr(dw), n,
                                                  _lib.ptr(count) if count is not None else None, _lib.ptr(outer),
                                                  _lib.ptr(inner), _lib.ptr(st))
        _lib.check(self.ctx.handle, rc)
        diff = outer - inner
        return RootCurvature(outer, inner, *diff, st)

    def cg_extrema(self, k_lo, w_lo, k_hi, w_hi, max_iter=40, tol_percent=None, count=None):
        """es_shoot_cg_extrema: per entry a bracket (k_lo, w_lo), (k_hi, w_hi) on one branch, k_lo < k_hi, both roots or
        near-roots; the wavenumber between them at which d2 omega / dk2 changes sign -- an extremum of the group speed --
        by regula falsi (Illinois) on the exact curvature, every point polished by Newton in omega.  Dict of CUDA tensors
        k, w, cg, q (the curvature there), resid (percent), iters, flag (int32) and status (uint8).  flag = 1: the curvature
        changed sign over the bracket, every polish succeeded, the point is PT_OK and resid < tol_percent (default 1e-3);
        without a sign change the end with the smaller |q| is reported, flag 0.  count as in mode_signature.  Nothing is
        read back."""
        import torch
        kl, wl, kh, wh = (self._dev(a).reshape(-1) for a in (k_lo, w_lo, k_hi, w_hi))
        n, dev = kl.numel(), kl.device
        assert wl.numel() == n and kh.numel() == n and wh.numel() == n
        self._check_count(count)
        k, w, cg, q, resid = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(5))
        iters, flag = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        rc = self.ctx.lib.es_shoot_cg_extrema(self.ctx.handle, self.handle, _lib.ptr(kl), _lib.ptr(wl), _lib.ptr(kh),
                                              _lib.ptr(wh), n, _lib.ptr(count) if count is not None else None, int(max_iter),
                                              1e-3 if tol_percent is None else float(tol_percent), _lib.ptr(k), _lib.ptr(w),
                                              _lib.ptr(cg), _lib.ptr(q), _lib.ptr(resid), _lib.ptr(iters), _lib.ptr(flag),
                                              _lib.ptr(st))
        _lib.check(self.ctx.handle, rc)
        return dict(k=k, w=w, cg=cg, q=q, resid=resid, iters=iters, flag=flag, status=st)

    def group_speed_extrema(self, branch, max_iter=40, tol_percent=None):
        """The extrema of the group speed along one traced branch: `branch` is an entry of TracedBranches.branches, or any
        dict of CUDA tensors k (increasing), w and flag.  (1) root_curvature at the flagged points, (2) the neighbouring
        flagged points between which the curvature changes sign, selected and moved to the front on the device, (3) one
        cg_extrema call over them.  Returns the dict of cg_extrema, its tensors as long as the branch less one, with
        `count` (int32 CUDA tensor of one element): the number of extrema, which lie in the leading entries in the order of
        k; the entries past it are left as allocated.  A change of sign is strict, as in cg_extrema: a traced point whose
        curvature is exactly zero is an extremum by itself and is not reported (root_curvature at the branch shows it).
        k, w and flag may be tensors on any device or arrays.  Nothing is read back."""
        import torch
        with torch.cuda.stream(self.ctx.torch_stream):
            k, w = self._dev(branch["k"]).reshape(-1), self._dev(branch["w"]).reshape(-1)
            n = k.numel()
            if n < 2 or w.numel() != n:
                raise ValueError("group_speed_extrema needs a branch of at least two points")
            ok = self._dev(branch["flag"]).reshape(-1) != 0
            if ok.numel() != n:
                raise ValueError("group_speed_extrema needs one flag per point of the branch")
            order = torch.argsort((~ok).to(torch.int8), stable=True)         # the flagged points first, in their order
            n_ok = ok.sum().to(torch.int32).reshape(1)
            k, w = k[order].contiguous(), w[order].contiguous()
            q = self.root_curvature(k, w, count=n_ok).curvature
            pair = torch.arange(n - 1, device=k.device) < n_ok - 1          # both points of the pair flagged
            change = pair & (((q[:-1] < 0) & (q[1:] > 0)) | ((q[:-1] > 0) & (q[1:] < 0)))
            sel = torch.argsort((~change).to(torch.int8), stable=True)
            n_change = change.sum().to(torch.int32).reshape(1)
            out = self.cg_extrema(k[:-1][sel], w[:-1][sel], k[1:][sel], w[1:][sel], max_iter=max_iter,
                                  tol_percent=tol_percent, count=n_change)
            out["count"] = n_change
            return out

    def _require_positive_cylinder(self):
        if not isinstance(self.eq, eqm._CylinderBase):
            raise ValueError("perturbation fields exist for cylinders only (the reference has no slab movies)")
        if self.desc.x_boundary < 0:
            raise ValueError("perturbation fields need positive radii: build the equilibrium with r_sign=+1")

    def field_profiles(self, reference_quirks=True):
        """field_profiles(eq, r, ...) at this problem's interior nodes (node 0 = boundary)."""
        self._require_positive_cylinder()
        return field_profiles(self.eq, self._prof_np["r"][::2], reference_quirks)

    def polarisation(self, k, w, n_ext=500, reference_quirks=True):
        """Radial amplitudes of the modes at the (k, omega) pairs (es_cyl_polarisation on the arrays of `eigenfunction`):
        dict of CUDA tensors radius [n, N + n_ext] and amp [n, 7, N + n_ext], channels _lib.AMP_NAMES, on the
        reference's grid concatenate(ix[::-1], lx[::-1]).  A pair that is not ES_PT_OK gets NaN amplitudes."""
        import torch
        self._require_positive_cylinder()
        e = self.eigenfunction(k, w, n_ext=n_ext)
        dk, dw = self._dev(k).reshape(-1), self._dev(w).reshape(-1)
        n, N = dk.numel(), int(self.desc.n_nodes)
        prof = {a: self._dev(b) for a, b in self.field_profiles(reference_quirks).items()}
        fp = _lib.FieldProfiles(*[prof[a].data_ptr() for a in _lib._FIELD_PROFILE_FIELDS])
        radius = torch.empty((n, N + n_ext), dtype=torch.float64, device=dk.device)
        amp = torch.empty((n, 7, N + n_ext), dtype=torch.float64, device=dk.device)
        d = self.desc
        rc = self.ctx.lib.es_cyl_polarisation(self.ctx.handle, _lib.ptr(dk), _lib.ptr(dw), n, N,
                                              _lib.ptr(e["value_int"]), _lib.ptr(e["flux_int"]), int(n_ext),
                                              _lib.ptr(e["x_ext"]), _lib.ptr(e["value_ext"]), _lib.ptr(e["flux_ext"]),
                                              C.byref(fp), int(d.m), d.rho_e, d.vA_e, d.c_e, d.cT_e,
                                              _lib.FIELD_REFERENCE if reference_quirks else 0, _lib.ptr(radius),
                                              _lib.ptr(amp))
        _lib.check(self.ctx.handle, rc)
        return dict(radius=radius, amp=amp)

    def fields(self, k, w, theta, z, t, variables=None, v_scale=1.0, big_endian=False, frames_per_call=None, n_ext=500,
               reference_quirks=True):
        """Perturbation fields of ONE root (k, omega) on the mesh (r, theta, z, t): float32 CUDA tensors in VTK's point
        order (Export_vtk.py:930-950 on the GPU).  Returns a dict
            points [n_z, n_theta, n_r, 3], t [n_t], names, frames [n_t, n_sel, n_z, n_theta, n_r], <name>: frames[:, i]
        with r on polarisation's grid; `variables` defaults to all of _lib.VAR_NAMES and is stored in that order.
        frames_per_call: a generator of such dicts, at most that many frames each (the frames tensor of a chunk is
        released with its dict, so a long movie never holds more than one chunk on the device).
        reference_quirks: the export scripts as written, -sin(m theta) on the z-components included; v_scale multiplies
        every velocity.  big_endian: every float32 is byte-swapped on the device, ready for postprocess.write_vtk_frames."""
        import torch
        self._require_positive_cylinder()
        if np.ndim(k) != 0 or np.ndim(w) != 0:
            raise ValueError("fields() takes one root: scalar k and omega")
        mask, names = var_mask(variables)
        pol = self.polarisation([float(k)], [float(w)], n_ext=n_ext, reference_quirks=reference_quirks)
        radius, amp = pol["radius"][0], pol["amp"][0]
        dth, dz, dt = (self._dev(a).reshape(-1) for a in (theta, z, t))
        flags = (_lib.FIELD_Z_REFERENCE_ANGLE if reference_quirks else 0) | (_lib.FIELD_BIG_ENDIAN if big_endian else 0)

        def synth(t_part, carry):                     # the points are produced once and handed to the later chunks
            out, pts, _ = field_synthesis(self.ctx, radius, amp, int(self.desc.m), k, w, dth, dz, t_part, names, v_scale,
                                          flags, want_points=carry is None)
            return out, carry or dict(points=pts)

        return _frame_chunks(synth, dt, frames_per_call, names)

    def vorticity_amplitudes(self, k, w, n_ext=500, reference_quirks=False):
        """`polarisation` followed by es_cyl_vorticity_amplitudes: dict of CUDA tensors radius [n, n_r], amp [n, 7, n_r] and
        vort [n, 5, n_r] (channels _lib.VORT_NAMES), the radial amplitudes of curl v in the linear-theory convention;
        radial derivatives per region, never across the interface.  reference_quirks selects the polarisation's profile
        quirks 1 - 3 only.  The exterior, when present, needs n_ext >= 3."""
        self._require_positive_cylinder()
        _require_exterior_points(n_ext)
        pol = self.polarisation(k, w, n_ext=n_ext, reference_quirks=reference_quirks)
        dk = self._dev(k).reshape(-1)
        pol["vort"] = vorticity_amplitudes(self.ctx, pol["radius"], pol["amp"], int(self.desc.n_nodes), int(n_ext),
                                           int(self.desc.m), dk)
        return pol

    def cartesian_fields(self, k, w, x, y, z, t, variables=None, v_scale=1.0, fill=float("nan"), big_endian=False,
                         frames_per_call=None, n_ext=500, reference_quirks=False):
        """Fields of ONE root (k, omega) on the Cartesian mesh (x, y, z, t), the vorticity of the velocity included:
        float32 CUDA tensors in the point order of a legacy-VTK RECTILINEAR_GRID (x fastest).  Returns a dict
            x [n_x], y [n_y], z [n_z], t [n_t], names, frames [n_t, n_sel, n_z, n_y, n_x], <name>: frames[:, i]
        `variables` defaults to all of _lib.CVAR_NAMES and is stored in that order.  Points outside the tabulated radii
        (the hole inside the axis node, beyond the far field of n_ext points, r = 0) carry `fill`.
        frames_per_call: a generator of such dicts, at most that many frames each.  reference_quirks selects only the
        polarisation's profile quirks 1 - 3; the angular factor of the z-components is always linear theory's cos(m theta).
        v_scale multiplies the velocities and the vorticity.  big_endian: every float32 is byte-swapped on the device,
        ready for postprocess.write_vtk_rectilinear_frames."""
        self._require_positive_cylinder()
        if np.ndim(k) != 0 or np.ndim(w) != 0:
            raise ValueError("cartesian_fields() takes one root: scalar k and omega")
        _require_exterior_points(n_ext)
        mask, names = cartesian_var_mask(variables)
        want_vort = any(v.startswith("vort_") for v in names)
        if want_vort:
            tab = self.vorticity_amplitudes([float(k)], [float(w)], n_ext=n_ext, reference_quirks=reference_quirks)
        else:
            tab = self.polarisation([float(k)], [float(w)], n_ext=n_ext, reference_quirks=reference_quirks)
        radius, amp = tab["radius"][0], tab["amp"][0]
        vort = tab["vort"][0] if want_vort else None
        dx, dy, dz, dt = (self._dev(a).reshape(-1) for a in (x, y, z, t))
        flags = _lib.FIELD_BIG_ENDIAN if big_endian else 0

        def synth(t_part, _):
            return cartesian_synthesis(self.ctx, radius, amp, vort, int(self.desc.n_nodes), int(n_ext), int(self.desc.m),
                                       k, w, dx, dy, dz, t_part, names, v_scale, fill, flags)[0], {}

        return _frame_chunks(synth, dt, frames_per_call, names, x=dx, y=dy, z=dz)

    def _require_slab(self):
        if not isinstance(self.eq, eqm._SlabBase):
            raise ValueError("slab_polarisation / slab_fields are for slab equilibria only (cylinders: polarisation, "
                             "fields, cartesian_fields)")

    def slab_field_profiles(self):
        """slab_field_profiles(eq) of this problem's equilibrium as CUDA tensors."""
        self._require_slab()
        return {a: self._dev(b) for a, b in slab_field_profiles(self.eq).items()}

    def _slab_polarisation_of(self, eig, dk, w_re, w_im, reference_quirks):
        d = self.desc
        return slab_polarisation(self.ctx, dk, w_re, w_im, eig, self.slab_field_profiles(), d.rho_e, d.vA_e, d.c_e, d.U_e,
                                 int(d.slab_mode), 0 if reference_quirks else _lib.SLAB_FIELD_SHEAR_PT)

    def slab_polarisation(self, k, w, n_ext=500, reference_quirks=True):
        """Complex amplitudes of the slab modes at the real (k, omega) pairs (es_slab_polarisation on the arrays of
        `eigenfunction`): dict of CUDA tensors x [n, 2 n_ext + N] (ascending: left exterior, interior, mirrored right
        exterior, each boundary abscissa twice) and amp [n, 6, 2 n_ext + N] (complex128, channels _lib.SAMP_NAMES); every
        field is Re[amp e^{i (k z - w t)}].  reference_quirks: the flux as the determinant uses it; False adds the shear
        term (F/Om)(k U'/Om) Vx of linear theory to it (ES_SLAB_FIELD_SHEAR_PT).  A pair that is not ES_PT_OK gets NaN
        amplitudes.  n_ext is 0 (no exteriors) or at least 3."""
        self._require_slab()
        _require_exterior_points(n_ext)
        dk, dw = self._dev(k).reshape(-1), self._dev(w).reshape(-1)
        return self._slab_polarisation_of(self.eigenfunction(dk, dw, n_ext=n_ext), dk, dw, None, reference_quirks)

    def slab_fields(self, k, w, x, z, t, variables=None, v_scale=1.0, fill=float("nan"), big_endian=False,
                    frames_per_call=None, n_ext=500, reference_quirks=True):
        """Fields of ONE slab root (k, omega) on the mesh (x, z, t): float32 CUDA tensors, x fastest -- with y = [0.0] the
        point order postprocess.write_vtk_rectilinear_frames writes.  Returns a dict
            x [n_x], z [n_z], t [n_t], names, frames [n_t, n_sel, n_z, n_x], <name>: frames[:, i]
        `variables` defaults to all of _lib.SVAR_NAMES and is stored in that order.  Points outside [-R, R], R = L 2 pi / k
        (or outside [-1, 1] with n_ext = 0) carry `fill`.  frames_per_call: a generator of such dicts, at most that many
        frames each.  v_scale multiplies v_x, v_z and vort_y.  big_endian: every float32 is byte-swapped on the device."""
        self._require_slab()
        if np.ndim(k) != 0 or np.ndim(w) != 0:
            raise ValueError("slab_fields() takes one root: scalar k and omega")
        mask, names = slab_var_mask(variables)
        tab = self.slab_polarisation([float(k)], [float(w)], n_ext=n_ext, reference_quirks=reference_quirks)
        dx, dz, dt = (self._dev(a).reshape(-1) for a in (x, z, t))
        return slab_frames(self.ctx, tab["x"][0], tab["amp"][0], int(self.desc.n_nodes), int(n_ext), float(k), float(w),
                           dx, dz, dt, names, v_scale, fill, big_endian, frames_per_call)

    def alloc_root_table(self, capacity):
        import torch
        dev = f"cuda:{self.ctx.device}"
        t = {n: torch.empty(capacity, dtype=torch.float64, device=dev) for n in ("k", "w", "w_lo", "w_hi", "resid")}
        t["row"] = torch.empty(capacity, dtype=torch.int32, device=dev)
        t["flag"] = torch.empty(capacity, dtype=torch.uint8, device=dev)
        rt = _lib.RootTable(t["k"].data_ptr(), t["w"].data_ptr(), t["w_lo"].data_ptr(), t["w_hi"].data_ptr(),
                            t["resid"].data_ptr(), t["row"].data_ptr(), t["flag"].data_ptr(), capacity)
        return t, rt

    def find_roots(self, k, w, D, status, w_mode=W_PHASE_SPEED, n_bisect=40, tol_percent=1e-3, capacity=None,
                   table=None):
        """Brackets + bisection + classification on the grid evaluated by eval_grid. Returns (dict, count)."""
        dk, dw, nk, nw = self._grid_args(k, w, w_mode)
        cap = int(capacity) if capacity is not None else max(1024, 16 * nk)
        while True:
            t, rt = table if table is not None else self.alloc_root_table(cap)
            n = C.c_int(0)
            rc = self.ctx.lib.es_shoot_find_roots(self.ctx.handle, self.handle, _lib.ptr(dk), nk, _lib.ptr(dw), nw,
                                                  w_mode, _lib.ptr(D), _lib.ptr(status), int(n_bisect),
                                                  float(tol_percent), C.byref(rt), C.byref(n))
            _lib.check(self.ctx.handle, rc, allow_capacity=True)
            if rc == 3 and capacity is None and table is None:
                cap = n.value
                continue
            m = min(n.value, rt.capacity)
            return {key: v[:m] for key, v in t.items()}, n.value

    def find_roots_async(self, k, w, D, status, table, count, w_mode=W_PHASE_SPEED, n_bisect=40, tol_percent=1e-3):
        """es_shoot_find_roots_async: everything enqueued on the context's stream, nothing read back.  `table` is
        (dict, RootTable) from alloc_root_table, `count` an int32 CUDA tensor of one element that receives the bracket
        count (it may exceed the capacity: check when reading it).  Returns the full-capacity dict of the table."""
        dk, dw, nk, nw = self._grid_args(k, w, w_mode)
        t, rt = table
        assert count.is_cuda and count.numel() == 1 and count.element_size() == 4
        rc = self.ctx.lib.es_shoot_find_roots_async(self.ctx.handle, self.handle, _lib.ptr(dk), nk, _lib.ptr(dw), nw,
                                                    w_mode, _lib.ptr(D), _lib.ptr(status), int(n_bisect),
                                                    float(tol_percent), C.byref(rt), _lib.ptr(count))
        _lib.check(self.ctx.handle, rc)
        return t

    def screen_grid(self, k, w, w_mode=W_PHASE_SPEED):
        """Step 1 of the mixed search alone (es_shoot_screen_grid): the fp32 screening march, enqueued.  Returns the
        screened (D, status) for find_roots_screened."""
        import torch
        dk, dw, nk, nw = self._grid_args(k, w, w_mode)
        D = torch.empty((nk, nw), dtype=torch.float64, device=dk.device)
        st = torch.empty((nk, nw), dtype=torch.uint8, device=dk.device)
        rc = self.ctx.lib.es_shoot_screen_grid(self.ctx.handle, self.handle, _lib.ptr(dk), nk, _lib.ptr(dw), nw, w_mode,
                                               _lib.ptr(D), _lib.ptr(st))
        _lib.check(self.ctx.handle, rc)
        return D, st

    def find_roots_screened(self, k, w, D, st, w_mode=W_PHASE_SPEED, n_bisect=40, tol_percent=1e-3, table=None, capacity=None):
        """Steps 2 - 5 of the mixed search on a grid screened by screen_grid; returns what find_roots_mixed returns."""
        dk, dw, nk, nw = self._grid_args(k, w, w_mode)
        t, rt = table if table is not None else self.alloc_root_table(int(capacity) if capacity is not None else max(1024, 16 * nk))
        n = C.c_int(0)
        stats = (C.c_int * 3)()
        rc = self.ctx.lib.es_shoot_find_roots_screened(self.ctx.handle, self.handle, _lib.ptr(dk), nk, _lib.ptr(dw), nw,
                                                       w_mode, int(n_bisect), float(tol_percent), _lib.ptr(D), _lib.ptr(st),
                                                       C.byref(rt), C.byref(n), stats)
        _lib.check(self.ctx.handle, rc, allow_capacity=True)
        m = min(n.value, rt.capacity)
        return {key: v[:m] for key, v in t.items()}, n.value, D, st, tuple(stats)

    def find_roots_mixed(self, k, w, w_mode=W_PHASE_SPEED, n_bisect=40, tol_percent=1e-3, capacity=None, table=None):
        """fp32 screening of the grid + fp64 re-evaluation of every unsure point and of both ends of every bracket +
        fp64 refinement (es_shoot_find_roots_mixed).  Returns (root dict, bracket count, D, status, stats) with
        stats = (fp64 re-evaluations of unsure grid points, of bracket ends, unconfirmed brackets)."""
        import torch
        dk, dw, nk, nw = self._grid_args(k, w, w_mode)
        D = torch.empty((nk, nw), dtype=torch.float64, device=dk.device)
        st = torch.empty((nk, nw), dtype=torch.uint8, device=dk.device)
        cap = int(capacity) if capacity is not None else max(1024, 16 * nk)
        while True:
            t, rt = table if table is not None else self.alloc_root_table(cap)
            n = C.c_int(0)
            stats = (C.c_int * 3)()
            rc = self.ctx.lib.es_shoot_find_roots_mixed(self.ctx.handle, self.handle, _lib.ptr(dk), nk, _lib.ptr(dw), nw,
                                                        w_mode, int(n_bisect), float(tol_percent), _lib.ptr(D),
                                                        _lib.ptr(st), C.byref(rt), C.byref(n), stats)
            _lib.check(self.ctx.handle, rc, allow_capacity=True)
            if rc == 3 and capacity is None and table is None:
                cap = n.value
                continue
            m = min(n.value, rt.capacity)
            return {key: v[:m] for key, v in t.items()}, n.value, D, st, tuple(stats)

    def audit_screening(self, k, w, w_mode=W_PHASE_SPEED, rows=None, screened=None, capacity=1024):
        """The fp32 screening of this grid against its fp64 evaluation, on the device (es_shoot_audit_screening): the check
        that no fp64 bracket is missed, which find_roots_mixed itself cannot give.  Returns a _lib.ScreenAudit.
        rows: the k-rows audited (rows are independent) -- None: all; an int s: rows 0, s, 2s, ...; an ascending index
        array: those rows (with W_PER_ROW the same rows of w).  The audited rows are evaluated in fp64 (eval_grid) and,
        with screened=None, screened with screen_grid; screened=(D, status) audits those rows of arrays the caller holds,
        e.g. the merged output of find_roots_mixed.  Reported rows are indices into the full grid."""
        import torch
        dk, dw, nk, nw = self._grid_args(k, w, w_mode)
        sel = None
        if rows is not None:
            if isinstance(rows, (int, np.integer)):
                if rows < 1:
                    raise ValueError("rows: a stride is at least 1")
                sel = np.arange(0, nk, int(rows), dtype=np.int64)
            else:
                sel = np.asarray(rows, dtype=np.int64).reshape(-1)
                if sel.size and (sel[0] < 0 or sel[-1] >= nk or np.any(np.diff(sel) <= 0)):
                    raise ValueError("rows: ascending indices into the k-rows of the grid")
            idx = torch.as_tensor(sel, device=dk.device)
            dk = dk[idx]
            if w_mode == W_PER_ROW:
                dw = dw.reshape(nk, nw)[idx].contiguous()
        D64, st64, rel64 = self.eval_grid(dk, dw, w_mode, want_rel=True)
        if screened is None:
            Ds, sts = self.screen_grid(dk, dw, w_mode)
        else:
            Ds, sts = (t.reshape(nk, nw) for t in screened)
            if sel is not None:
                Ds, sts = Ds[idx], sts[idx]
        return audit_arrays(self.ctx, Ds, sts, D64, st64, rel64, capacity=capacity, rows=sel)

    def find_roots_mixed_audited(self, k, w, w_mode=W_PHASE_SPEED, n_bisect=40, tol_percent=1e-3, capacity=None, table=None,
                                 rows=None):
        """find_roots_mixed, then audit_screening of its merged (D, status) on `rows`.  Returns find_roots_mixed's tuple
        plus the ScreenAudit; raises EsError (the failure of ES_ERR_SCREENING) when the audit finds a missed or false
        bracket or a wrong status."""
        out = self.find_roots_mixed(k, w, w_mode=w_mode, n_bisect=n_bisect, tol_percent=tol_percent, capacity=capacity,
                                    table=table)
        report = self.audit_screening(k, w, w_mode=w_mode, rows=rows, screened=(out[2], out[3]))
        _lib.check_audit(report)
        return out + (report,)

    @staticmethod
    def _check_counts(counts):
        import torch
        assert counts.is_cuda and counts.dtype == torch.int32 and counts.numel() == 4 and counts.is_contiguous()

    def find_roots_screened_async(self, k, w, D, st, table, counts, w_mode=W_PHASE_SPEED, n_bisect=40, tol_percent=1e-3):
        """es_shoot_find_roots_screened_async: find_roots_screened with everything enqueued on the context's stream and
        nothing read back.  `table` is (dict, RootTable) from alloc_root_table, `counts` a 4-element int32 CUDA tensor
        that receives (brackets, unsure re-evaluations, bracket-end re-evaluations, unconfirmed brackets); read it with
        read_screen_counts.  Returns the full-capacity dict of the table."""
        import torch
        self._check_counts(counts)
        with torch.cuda.stream(self.ctx.torch_stream):      # temporaries are released to the context's stream
            dk, dw, nk, nw = self._grid_args(k, w, w_mode)
            t, rt = table
            rc = self.ctx.lib.es_shoot_find_roots_screened_async(self.ctx.handle, self.handle, _lib.ptr(dk), nk, _lib.ptr(dw),
                                                                 nw, w_mode, int(n_bisect), float(tol_percent), _lib.ptr(D),
                                                                 _lib.ptr(st), C.byref(rt), _lib.ptr(counts))
        _lib.check(self.ctx.handle, rc)
        return t

    def find_roots_mixed_async(self, k, w, table, counts, w_mode=W_PHASE_SPEED, n_bisect=40, tol_percent=1e-3):
        """es_shoot_find_roots_mixed_async: find_roots_mixed with everything enqueued on the context's stream and nothing
        read back (see find_roots_screened_async).  Returns (full-capacity dict of the table, D, status)."""
        import torch
        self._check_counts(counts)
        with torch.cuda.stream(self.ctx.torch_stream):
            dk, dw, nk, nw = self._grid_args(k, w, w_mode)
            D = torch.empty((nk, nw), dtype=torch.float64, device=dk.device)
            st = torch.empty((nk, nw), dtype=torch.uint8, device=dk.device)
            t, rt = table
            rc = self.ctx.lib.es_shoot_find_roots_mixed_async(self.ctx.handle, self.handle, _lib.ptr(dk), nk, _lib.ptr(dw),
                                                              nw, w_mode, int(n_bisect), float(tol_percent), _lib.ptr(D),
                                                              _lib.ptr(st), C.byref(rt), _lib.ptr(counts))
        _lib.check(self.ctx.handle, rc)
        return t, D, st
