"""Complex frequencies on the untwisted cylinder (C ABI sections 14 and 15 of include/eigensolver_amd.h): the determinant of the
shooting path at omega = omega_r + i omega_i on (k, Re omega, Im omega) grids and point lists, and the root search -- the
unstable (Kelvin-Helmholtz) modes of a cylinder whose axial jet is fast enough, where the root leaves the real axis and
ShootProblem.find_roots / trace_branches report nothing.

For equilibrium.CylinderDensity and equilibrium.CylinderFlow, any azimuthal order m, "kink" and "sausage" axis conditions,
both signs of r.  Shapes and return conventions are those of complex_flow.SlabComplexFlow.  Section 15 adds the exact slopes
D_w, D_k of a root, Newton's iteration and `densify`, which turns a few unstable_roots rows into the growth-rate curve that
postprocess.most_unstable reads.  DESIGN.md sections 8i and 8j.
"""
import ctypes as C

import numpy as np

from . import _lib
from .complex_flow import ComplexTracing, _distinct
from .shooting import ShootProblem, W_ABSOLUTE, W_PHASE_SPEED  # noqa: F401


class CylinderComplex(ComplexTracing):
    """D_c(k, omega) of one cylinder equilibrium at complex omega: grids, point lists, roots, and through ComplexTracing
    the slopes and the Newton tracing of section 15 -- root_slopes(mode, k, w, count=None, m=None), group_velocity(mode,
    roots, count=None, m=None), newton(mode, k, w0, ..., m=None) and densify(mode, k, w, k_fine, shift_factor=4.0, m=None,
    **newton_kw), with the return conventions of SlabComplexFlow.  One ShootProblem per (mode, m), created on first use."""
    _SELECT = ("m",)
    P_TOL = 4.0                                     # acceptance of a refined root, percent: that of SlabComplexFlow

    def __init__(self, equilibrium, ctx=None):
        if getattr(equilibrium, "twisted", True):
            raise TypeError("CylinderComplex takes an untwisted cylinder equilibrium (CylinderDensity, CylinderFlow)")
        self.eq = equilibrium
        self.ctx = ctx or _lib.Context()
        self._problems = {}

    def problem(self, mode, m=None):
        key = (mode, (1 if mode == "kink" else 0) if m is None else int(m))
        if key not in self._problems:
            self._problems[key] = ShootProblem(self.eq, mode, m=key[1], ctx=self.ctx)
        return self._problems[key]

    def close(self):
        for p in self._problems.values():
            p.close()
        self._problems = {}

    # ---- slopes and Newton tracing (C ABI section 15): ComplexTracing over these two calls ----------------------------------
    def _slopes_call(self, p, *args):
        return self.ctx.lib.es_cyl_complex_root_slopes(self.ctx.handle, p.handle, *args)

    def _newton_call(self, p, *args):
        return self.ctx.lib.es_cyl_complex_newton(self.ctx.handle, p.handle, *args)

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
        rc = self.ctx.lib.es_cyl_complex_eval_grid(self.ctx.handle, p.handle, _lib.ptr(dk), nk, _lib.ptr(dre), nre,
                                                   _lib.ptr(dim), nim, int(w_mode), _lib.ptr(Dre), _lib.ptr(Dim),
                                                   _lib.ptr(rel), _lib.ptr(st))
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
        rc = self.ctx.lib.es_cyl_complex_eval_points(self.ctx.handle, p.handle, _lib.ptr(dk), _lib.ptr(dre), _lib.ptr(dim), n,
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
            rc = self.ctx.lib.es_cyl_complex_find_roots(self.ctx.handle, p.handle, _lib.ptr(dk), nk, _lib.ptr(dre), nre,
                                                        _lib.ptr(dim), nim, int(w_mode), _lib.ptr(Dre), _lib.ptr(Dim),
                                                        _lib.ptr(status), int(n_iter), tol, C.byref(rt), C.byref(n))
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
