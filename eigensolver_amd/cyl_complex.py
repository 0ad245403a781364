"""Complex frequencies on the untwisted cylinder (C ABI sections 14 and 15 of include/eigensolver_amd.h): the determinant of the
shooting path at omega = omega_r + i omega_i on (k, Re omega, Im omega) grids and point lists, and the root search -- the
unstable (Kelvin-Helmholtz) modes of a cylinder whose axial jet is fast enough, where the root leaves the real axis and
ShootProblem.find_roots / trace_branches report nothing.

For equilibrium.CylinderDensity and equilibrium.CylinderFlow, any azimuthal order m, "kink" and "sausage" axis conditions,
both signs of r.  Shapes and return conventions are those of complex_flow.SlabComplexFlow.  Section 15 adds the exact slopes
D_w, D_k of a root, Newton's iteration and `densify`, which turns a few unstable_roots rows into the growth-rate curve that
postprocess.most_unstable reads.  Section 16 adds what the mode looks like: `eigenfunction` (P and xi_r at complex roots),
`polarisation` (the seven complex amplitudes) and `fields` (growing float32 frames ready for postprocess.write_vtk_frames).
Section 20 puts the mode on a Cartesian mesh with the vorticity of its velocity: `vorticity_amplitudes`, `cartesian_synthesis`
and `cartesian_fields` (ready for postprocess.write_vtk_rectilinear_frames).  DESIGN.md sections 8i, 8j, 8k and 8o.
"""
import ctypes as C

import numpy as np

from . import _lib
from .complex_flow import ComplexTracing, _distinct
from .shooting import (ShootProblem, W_ABSOLUTE, W_PHASE_SPEED, _COMPLEX_TABLES, _cartesian_synthesis,  # noqa: F401
                       _field_synthesis, _frame_chunks, _require_exterior_points, _vorticity_amplitudes, cartesian_var_mask,
                       var_mask)


class CylinderEvaluation:
    """The evaluation and root-search plumbing of sections 14 and 17, written once over the three entry points
    <_PREFIX>eval_grid, <_PREFIX>eval_points and <_PREFIX>find_roots (same signatures), and the two calls ComplexTracing
    asks for over <_PREFIX>root_slopes and <_PREFIX>newton (sections 15 and 18): CylinderComplex and
    cylt_complex.RotatingCylinderComplex.  One ShootProblem per (mode, m), created on first use."""
    _PREFIX = None                                  # "es_cyl_complex_" / "es_cylt_complex_"
    P_TOL = 4.0                                     # acceptance of a refined root, percent: that of SlabComplexFlow

    def _init(self, equilibrium, ctx):
        self.eq = equilibrium
        self.ctx = ctx or _lib.Context()
        self._problems = {}

    def _entry(self, name):
        return getattr(self.ctx.lib, self._PREFIX + name)

    def problem(self, mode, m=None):
        key = (mode, (1 if mode == "kink" else 0) if m is None else int(m))
        if key not in self._problems:
            self._problems[key] = ShootProblem(self.eq, mode, m=key[1], ctx=self.ctx)
        return self._problems[key]

    def close(self):
        for p in self._problems.values():
            p.close()
        self._problems = {}

    # ---- evaluation ------------------------------------------------------------------------------------------------
    def eval_grid(self, mode, k, w_re, w_im, w_mode=W_ABSOLUTE, m=None):
        """D_c[nk, n_im, n_re] (complex128 tensor), status[nk, n_im, n_re], rel[nk, n_im, n_re]."""
        import torch
        p = self.problem(mode, m)
        dk, dre, dim = p._dev(k).reshape(-1), p._dev(w_re).reshape(-1), p._dev(w_im).reshape(-1)
        nk, nre, nim = dk.numel(), dre.numel(), dim.numel()
        Dre = torch.empty((nk, nim, nre), dtype=torch.float64, device=dk.device)
        Dim = torch.empty_like(Dre)
        rel = torch.empty_like(Dre)
        st = torch.empty((nk, nim, nre), dtype=torch.uint8, device=dk.device)
        rc = self._entry("eval_grid")(self.ctx.handle, p.handle, _lib.ptr(dk), nk, _lib.ptr(dre), nre, _lib.ptr(dim), nim,
                                      int(w_mode), _lib.ptr(Dre), _lib.ptr(Dim), _lib.ptr(rel), _lib.ptr(st))
        _lib.check(self.ctx.handle, rc)
        return torch.complex(Dre, Dim), st, rel

    def eval_points(self, mode, k, w, m=None, parts=False):
        """D_c, status, rel at the complex w (k is broadcast against it); parts=True: also outer (xi_e) and inner (xi_i),
        complex128 tensors with D_c = outer - inner."""
        import torch
        p = self.problem(mode, m)
        w = np.asarray(w, dtype=complex).reshape(-1)
        dk = p._dev(np.broadcast_to(np.asarray(k, dtype=float), w.shape).copy())
        dre, dim = p._dev(w.real.copy()), p._dev(w.imag.copy())
        n = dk.numel()
        Dre = torch.empty(n, dtype=torch.float64, device=dk.device)
        Dim, rel = torch.empty_like(Dre), torch.empty_like(Dre)
        st = torch.empty(n, dtype=torch.uint8, device=dk.device)
        outer = torch.empty(n, dtype=torch.complex128, device=dk.device) if parts else None
        inner = torch.empty(n, dtype=torch.complex128, device=dk.device) if parts else None
        rc = self._entry("eval_points")(self.ctx.handle, p.handle, _lib.ptr(dk), _lib.ptr(dre), _lib.ptr(dim), n,
                                        _lib.ptr(Dre), _lib.ptr(Dim), _lib.ptr(rel), _lib.ptr(st),
                                        _lib.ptr(outer) if parts else None, _lib.ptr(inner) if parts else None)
        _lib.check(self.ctx.handle, rc)
        D = torch.complex(Dre, Dim)
        return (D, st, rel, outer, inner) if parts else (D, st, rel)

    def find_roots(self, mode, k, w_re, w_im, D, status, w_mode=W_ABSOLUTE, n_iter=12, tol_percent=None, capacity=None, m=None):
        """Cells of the (Re, Im) grid around which D_c winds once, refined by complex secant steps.
        Returns ({k, w (complex), resid, row, flag}, count)."""
        import torch
        p = self.problem(mode, m)
        dk, dre, dim = p._dev(k).reshape(-1), p._dev(w_re).reshape(-1), p._dev(w_im).reshape(-1)
        nk, nre, nim = dk.numel(), dre.numel(), dim.numel()
        Dre, Dim = D.real.contiguous(), D.imag.contiguous()
        tol = self.P_TOL if tol_percent is None else float(tol_percent)
        cap = int(capacity) if capacity is not None else max(256, 4 * nk)
        while True:
            dev = dk.device
            t = {"k": torch.empty(cap, dtype=torch.float64, device=dev), "w_re": torch.empty(cap, dtype=torch.float64, device=dev),
                 "w_im": torch.empty(cap, dtype=torch.float64, device=dev), "resid": torch.empty(cap, dtype=torch.float64, device=dev),
                 "row": torch.empty(cap, dtype=torch.int32, device=dev), "flag": torch.empty(cap, dtype=torch.int32, device=dev)}
            rt = _lib.ComplexRootTable(_lib.ptr(t["k"]), _lib.ptr(t["w_re"]), _lib.ptr(t["w_im"]), _lib.ptr(t["resid"]),
                                       _lib.ptr(t["row"]), _lib.ptr(t["flag"]), cap)
            n = C.c_int(0)
            rc = self._entry("find_roots")(self.ctx.handle, p.handle, _lib.ptr(dk), nk, _lib.ptr(dre), nre, _lib.ptr(dim), nim,
                                           int(w_mode), _lib.ptr(Dre), _lib.ptr(Dim), _lib.ptr(status), int(n_iter), tol,
                                           C.byref(rt), C.byref(n))
            _lib.check(self.ctx.handle, rc, allow_capacity=True)
            if rc == 3 and capacity is None:
                cap = n.value
                continue
            cnt = min(n.value, cap)
            out = {"k": t["k"][:cnt], "w": torch.complex(t["w_re"][:cnt], t["w_im"][:cnt]), "resid": t["resid"][:cnt],
                   "row": t["row"][:cnt], "flag": t["flag"][:cnt]}
            return out, n.value

    def unstable_roots(self, mode, k, w_re, w_im, w_mode=W_ABSOLUTE, m=None, n_iter=12, tol_percent=None):
        """Grid, search, and the accepted (flag == 1), de-duplicated roots of every k-row: a list with one complex NumPy
        array per k (a root on a cell edge is found from both neighbouring cells and reported once)."""
        k = np.atleast_1d(np.asarray(k, dtype=float))
        D, st, _ = self.eval_grid(mode, k, w_re, w_im, w_mode, m=m)
        roots, _ = self.find_roots(mode, k, w_re, w_im, D, st, w_mode, n_iter=n_iter, tol_percent=tol_percent, m=m)
        ok = roots["flag"].cpu().numpy() == 1
        w, row = roots["w"].cpu().numpy()[ok], roots["row"].cpu().numpy()[ok]
        return [_distinct(w[row == r]) for r in range(len(k))]

    # ---- slopes and Newton tracing (C ABI sections 15 and 18): ComplexTracing over these two calls -------------------------
    def _slopes_call(self, p, *args):
        return self._entry("root_slopes")(self.ctx.handle, p.handle, *args)

    def _newton_call(self, p, *args):
        return self._entry("newton")(self.ctx.handle, p.handle, *args)


def vorticity_amplitudes(ctx, radius, amp, n_nodes, n_ext, m, k):
    """es_cyl_complex_vorticity_amplitudes on the tables of es_cyl_complex_polarisation (radius [n, n_r] and k [n] float64,
    amp [n, 7, n_r] complex128, CUDA, n_r = n_nodes + n_ext): the three complex radial amplitudes of curl v, vort [n, 3, n_r]
    complex128 in the order _lib.CVORT_NAMES, as shooting.vorticity_amplitudes.  Enqueued on the context's stream."""
    return _vorticity_amplitudes(_COMPLEX_TABLES, ctx, radius, amp, n_nodes, n_ext, m, k)


def cartesian_synthesis(ctx, radius, amp, vort, n_nodes, n_ext, m, k, w, x, y, z, t, variables=None, v_scale=1.0,
                        fill=float("nan"), flags=0, out=None):
    """es_cyl_complex_cartesian_synthesis for the tables of one mode (radius [n_r] float64, amp [7, n_r] and vort [3, n_r]
    complex128 or None, CUDA; w complex): float32 frames out[n_t, n_sel, n_z, n_y, n_x] in the order of
    cartesian_var_mask(variables)[1], as shooting.cartesian_synthesis.  Enqueued on the context's stream; returns (out, names)."""
    return _cartesian_synthesis(_COMPLEX_TABLES, ctx, radius, amp, vort, n_nodes, n_ext, m, k, w, x, y, z, t, variables, v_scale,
                                fill, flags, out)


class CylinderEigenfunctions:
    """What a mode looks like (C ABI sections 16 and 19), written once for CylinderComplex and
    cylt_complex.RotatingCylinderComplex beside CylinderEvaluation: `eigenfunction` through <_PREFIX>eigenfunction (same
    signature in both families), `polarisation` and `field_synthesis` through es_cyl_complex_polarisation and
    es_cyl_complex_field_synthesis, which take no problem handle and serve both families, and `fields`; on the Cartesian mesh
    (section 20) `vorticity_amplitudes`, `cartesian_synthesis` and `cartesian_fields`, likewise without a problem handle."""

    def eigenfunction(self, mode, k, w, n_ext=500, m=None):
        """Two-region solution at the complex (k, omega) pairs (es_cyl_complex_eigenfunction; es_cylt_complex_eigenfunction on
        a twisted equilibrium).  `w` is complex and `k` is broadcast against it; both may be tensors, e.g. roots["k"],
        roots["w"] of find_roots.  Dict of CUDA tensors as SlabComplexFlow.eigenfunction: x_int [N], value_int / flux_int [n, N] (complex128: P and xi_r on the node grid, node 0 =
        boundary), x_ext [n, n_ext], value_ext / flux_ext [n, n_ext] (complex128, far field to boundary), status [n] (uint8,
        that of eval_points; rows that are not ES_PT_OK are NaN).  Scaled per unit P_e(boundary): value_ext[:, -1] = 1,
        value_int[:, 0] = 1 and flux_ext[:, -1] - flux_int[:, 0] = D_c (to rounding where the axis target is zero, to the RK4
        truncation of the grid on a twisted problem with bc_const != 0: section 19)."""
        import torch
        p, dk, dre, dim = self._pairs(mode, k, w, m=m)
        dev = dk.device
        n, N, n_ext = dk.numel(), int(p.desc.n_nodes), int(n_ext)
        vi = torch.empty((n, N), dtype=torch.complex128, device=dev)
        fi = torch.empty((n, N), dtype=torch.complex128, device=dev)
        xe = torch.empty((n, n_ext), dtype=torch.float64, device=dev)
        ve = torch.empty((n, n_ext), dtype=torch.complex128, device=dev)
        fe = torch.empty((n, n_ext), dtype=torch.complex128, device=dev)
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        rc = self._entry("eigenfunction")(self.ctx.handle, p.handle, _lib.ptr(dk), _lib.ptr(dre), _lib.ptr(dim), n, _lib.ptr(vi),
                                          _lib.ptr(fi), n_ext, _lib.ptr(xe), _lib.ptr(ve), _lib.ptr(fe), _lib.ptr(st))
        _lib.check(self.ctx.handle, rc)
        x_int = torch.linspace(p.desc.x_boundary, p.desc.x_end, N, dtype=torch.float64, device=dev)
        return dict(x_int=x_int, value_int=vi, flux_int=fi, x_ext=xe, value_ext=ve, flux_ext=fe, status=st)

    def polarisation(self, mode, k, w, n_ext=500, reference_quirks=True, m=None):
        """Complex radial amplitudes of the modes at the complex (k, omega) pairs (es_cyl_complex_polarisation on the arrays
        of `eigenfunction`): dict of CUDA tensors radius [n, N + n_ext], amp [n, 7, N + n_ext] (complex128, channels
        _lib.AMP_NAMES, on the grid of ShootProblem.polarisation) and status [n].  The amplitudes are the analytic
        continuation in omega of ShootProblem.polarisation's: every field is Re[amp Theta(theta) e^{i (k z - w t)}] with
        section 7's angular factors.  Rows that are not ES_PT_OK are NaN.  Positive radii (r_sign=+1) only."""
        import torch
        p = self.problem(mode, m)
        p._require_positive_cylinder()
        e = self.eigenfunction(mode, k, w, n_ext=n_ext, m=m)
        _, dk, dre, dim = self._pairs(mode, k, w, m=m)
        n, N, n_ext = dk.numel(), int(p.desc.n_nodes), int(n_ext)
        prof = {a: p._dev(b) for a, b in p.field_profiles(reference_quirks).items()}
        fp = _lib.FieldProfiles(*[prof[a].data_ptr() for a in _lib._FIELD_PROFILE_FIELDS])
        radius = torch.empty((n, N + n_ext), dtype=torch.float64, device=dk.device)
        amp = torch.empty((n, 7, N + n_ext), dtype=torch.complex128, device=dk.device)
        d = p.desc
        rc = self.ctx.lib.es_cyl_complex_polarisation(self.ctx.handle, _lib.ptr(dk), _lib.ptr(dre), _lib.ptr(dim), n, N,
                                                      _lib.ptr(e["value_int"]), _lib.ptr(e["flux_int"]), n_ext,
                                                      _lib.ptr(e["x_ext"]), _lib.ptr(e["value_ext"]), _lib.ptr(e["flux_ext"]),
                                                      C.byref(fp), int(d.m), d.rho_e, d.vA_e, d.c_e, d.cT_e,
                                                      _lib.FIELD_REFERENCE if reference_quirks else 0, _lib.ptr(radius),
                                                      _lib.ptr(amp))
        _lib.check(self.ctx.handle, rc)
        return dict(radius=radius, amp=amp, status=e["status"])

    def field_synthesis(self, radius, amp, m, k, w, theta, z, t, variables=None, v_scale=1.0, flags=0, want_points=True,
                        out=None):
        """es_cyl_complex_field_synthesis for the amplitude table of one mode (radius [n_r] float64, amp [7, n_r] complex128,
        CUDA; w complex): float32 frames out[n_t, n_sel, n_z, n_theta, n_r] and, with want_points, points[n_z, n_theta, n_r, 3],
        as shooting.field_synthesis.  Returns (out, points, names)."""
        assert amp.is_contiguous()
        return _field_synthesis(_COMPLEX_TABLES, self.ctx, radius, amp, m, k, w, theta, z, t, variables, v_scale, flags,
                                want_points, out)

    def fields(self, mode, k, w, theta, z, t, variables=None, v_scale=1.0, big_endian=False, frames_per_call=None, n_ext=500,
               reference_quirks=True, m=None):
        """Perturbation fields of ONE complex root (k, omega) on the mesh (r, theta, z, t), the growth factor e^{Im w t}
        included: the dict of ShootProblem.fields -- points [n_z, n_theta, n_r, 3], t [n_t], names, frames [n_t, n_sel, n_z,
        n_theta, n_r], <name>: frames[:, i], float32 CUDA tensors in VTK's point order -- or with frames_per_call the generator
        of such dicts; the points are produced once.  big_endian: ready for postprocess.write_vtk_frames."""
        p = self.problem(mode, m)
        p._require_positive_cylinder()
        if np.ndim(k) != 0 or np.ndim(w) != 0:
            raise ValueError("fields() takes one root: scalar k and omega")
        k, w = float(k), complex(w)
        mask, names = var_mask(variables)
        pol = self.polarisation(mode, [k], [w], n_ext=n_ext, reference_quirks=reference_quirks, m=m)
        radius, amp = pol["radius"][0], pol["amp"][0]
        dth, dz, dt = (p._dev(a).reshape(-1) for a in (theta, z, t))
        flags = (_lib.FIELD_Z_REFERENCE_ANGLE if reference_quirks else 0) | (_lib.FIELD_BIG_ENDIAN if big_endian else 0)

        def synth(t_part, carry):                     # the points are produced once and handed to the later chunks
            out, pts, _ = self.field_synthesis(radius, amp, int(p.desc.m), k, w, dth, dz, t_part, names, v_scale, flags,
                                               want_points=carry is None)
            return out, carry or dict(points=pts)

        return _frame_chunks(synth, dt, frames_per_call, names)

    # ---- Cartesian sampling and vorticity (C ABI section 20) -------------------------------------------------------------
    def vorticity_amplitudes(self, mode, k, w, n_ext=500, reference_quirks=False, m=None):
        """`polarisation` followed by es_cyl_complex_vorticity_amplitudes: its dict with vort [n, 3, n_r] (complex128, channels
        _lib.CVORT_NAMES) added, the complex radial amplitudes of curl v: omega_r = Re[W_r sin(m theta) e^{i (k z - w t)}],
        omega_phi with cos(m theta), omega_z with sin(m theta).  Radial derivatives per region, never across the interface.
        The exterior, when present, needs n_ext >= 3."""
        import torch
        p, dk, dre, dim = self._pairs(mode, k, w, m=m)          # on the device once: _pairs takes tensors as they are
        p._require_positive_cylinder()
        _require_exterior_points(n_ext)
        pol = self.polarisation(mode, dk, torch.complex(dre, dim), n_ext=n_ext, reference_quirks=reference_quirks, m=m)
        pol["vort"] = vorticity_amplitudes(self.ctx, pol["radius"], pol["amp"], int(p.desc.n_nodes), int(n_ext), int(p.desc.m), dk)
        return pol

    def cartesian_synthesis(self, radius, amp, vort, n_nodes, n_ext, m, k, w, x, y, z, t, variables=None, v_scale=1.0,
                            fill=float("nan"), flags=0, out=None):
        """The module's cartesian_synthesis on this object's context.  Returns (out, names)."""
        return cartesian_synthesis(self.ctx, radius, amp, vort, n_nodes, n_ext, m, k, w, x, y, z, t, variables, v_scale, fill,
                                   flags, out)

    def cartesian_fields(self, mode, k, w, x, y, z, t, variables=None, v_scale=1.0, fill=float("nan"), big_endian=False,
                         frames_per_call=None, n_ext=500, reference_quirks=False, m=None):
        """Fields of ONE complex root (k, omega) on the Cartesian mesh (x, y, z, t), the vorticity of the velocity and the
        growth factor e^{Im w t} included: the dict of ShootProblem.cartesian_fields -- x, y, z, t, names, frames [n_t, n_sel,
        n_z, n_y, n_x], <name>: frames[:, i], float32 CUDA tensors in the point order of a legacy-VTK RECTILINEAR_GRID -- or
        with frames_per_call the generator of such dicts.  `variables`, `fill`, `v_scale`, `reference_quirks` as there.
        big_endian: ready for postprocess.write_vtk_rectilinear_frames.  Positive radii (r_sign=+1) only."""
        p = self.problem(mode, m)
        p._require_positive_cylinder()
        if np.ndim(k) != 0 or np.ndim(w) != 0:
            raise ValueError("cartesian_fields() takes one root: scalar k and omega")
        _require_exterior_points(n_ext)
        k, w = float(k), complex(w)
        mask, names = cartesian_var_mask(variables)
        want_vort = any(v.startswith("vort_") for v in names)
        tables = self.vorticity_amplitudes if want_vort else self.polarisation
        tab = tables(mode, [k], [w], n_ext=n_ext, reference_quirks=reference_quirks, m=m)
        radius, amp = tab["radius"][0], tab["amp"][0]
        vort = tab["vort"][0] if want_vort else None
        dx, dy, dz, dt = (p._dev(a).reshape(-1) for a in (x, y, z, t))
        flags = _lib.FIELD_BIG_ENDIAN if big_endian else 0

        def synth(t_part, _):
            return self.cartesian_synthesis(radius, amp, vort, int(p.desc.n_nodes), int(n_ext), int(p.desc.m), k, w, dx, dy,
                                            dz, t_part, names, v_scale, fill, flags)[0], {}

        return _frame_chunks(synth, dt, frames_per_call, names, x=dx, y=dy, z=dz)


class CylinderComplex(CylinderEvaluation, CylinderEigenfunctions, ComplexTracing):
    """D_c(k, omega) of one cylinder equilibrium at complex omega: grids, point lists, roots (CylinderEvaluation), and through
    ComplexTracing the slopes and the Newton tracing of section 15 -- root_slopes(mode, k, w, count=None, m=None),
    group_velocity(mode, roots, count=None, m=None), newton(mode, k, w0, ..., m=None) and densify(mode, k, w, k_fine,
    shift_factor=4.0, m=None, **newton_kw), with the return conventions of SlabComplexFlow; through CylinderEigenfunctions
    eigenfunction, polarisation, field_synthesis and fields of section 16, vorticity_amplitudes, cartesian_synthesis and
    cartesian_fields of section 20."""
    _SELECT = ("m",)
    _PREFIX = "es_cyl_complex_"

    def __init__(self, equilibrium, ctx=None):
        if getattr(equilibrium, "twisted", True):
            raise TypeError("CylinderComplex takes an untwisted cylinder equilibrium (CylinderDensity, CylinderFlow)")
        self._init(equilibrium, ctx)
