"""Host-side mirror of the reference's complex-frequency workers (unstable / Kelvin-Helmholtz modes of the flow slab)

    Slab/Non uniform flow/COMPLEX ANALYSIS/flow_multiprocessor_complex_coronal.py
      :348  sausage(wavenumber, sausage_ws, sausage_ks, sausage_ws_imag, sausage_ks_imag, freq)
      :737  kink(wavenumber, kink_ws, kink_ks, kink_ws_imag, kink_ks_imag, freq)
      :1127 driver: freq = linspace(s_i k, s_{i+1} k, 10) + 1j * linspace(-0.25, 0.25, 10)

over the C ABI of include/eigensolver_amd.h section (6).  `freq` is the complex array the reference's driver builds:
its real parts are the Re(omega) samples and its imaginary parts the Im(omega) samples of a rectangular grid.  (The
reference forms `freq[j] + 1j*freq[m]` from that array, which shears the grid; the rectangular reading is the one its
comments and plots describe.)  A root is where the complex mismatch D_c vanishes -- the reference accepts a grid point
whose REAL part of the mismatch is below p_tol = 4 %; here every grid cell around which D_c winds once is refined by
complex secant steps and accepted if 100 |D_c| / max(|outer|, |inner|) < tol.
"""
import ctypes as C
import math
import sys
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from . import _lib, equilibrium as eqm
from .shooting import ShootProblem, W_ABSOLUTE, W_PHASE_SPEED, hermite_guess

CX_SFX, CX_SFG = 0, 1
DBL_MAX = sys.float_info.max


class ComplexRootSlopes(NamedTuple):
    """es_complex_root_slopes: the two sides of the matching condition with their exact derivatives, complex128 CUDA tensors.
    outer, inner are [3, n] (value, d/d omega, d/dk); d, d_w, d_k [n] are D_c = outer - inner and its derivatives.  A pair
    that is not PT_OK, or whose outputs are not finite, carries NaN throughout."""
    outer: object
    inner: object
    d: object
    d_w: object
    d_k: object
    status: object            # uint8: the status of eval_points

    @property
    def group_velocity(self):
        """d omega / dk along the branch through each pair, -D_k / D_w (complex): the real part is the group speed, the
        imaginary part the slope of the growth rate."""
        return -self.d_k / self.d_w

    @property
    def newton_dw(self):
        """The Newton correction -D / D_w: how far in omega each pair lies from the root of its row."""
        return -self.d / self.d_w


@dataclass
class SlabFlowKH(eqm.SlabFlow):
    """Constants of the complex script (SF-X:96-121): densities given, c_e from them (not from pressure balance)."""
    c_i0: float = 1.3
    vA_i0: float = 1.0
    vA_e: float = 0.0
    c_e: float = float("nan")
    rho_i0: float = 9.0
    rho_e_value: float = 5.0
    U_i0: float = 1.4
    U_e: float = 0.0

    def __post_init__(self):
        if math.isnan(self.c_e):
            self.c_e = math.sqrt((self.rho_i0 / self.rho_e_value) * self.c_i0 ** 2 + eqm.GAMMA * 0.5 * self.vA_i0 ** 2)   # SF-X:111

    @property
    def rho_e(self):
        return self.rho_e_value


def _distinct(w, tol=1e-8):
    """A root on a cell edge is found from both neighbouring cells: keep the first of each cluster."""
    keep = []
    for z in w:
        if all(abs(z - y) > tol * max(1.0, abs(z)) for y in keep):
            keep.append(z)
    return np.array(keep, dtype=complex)


class ComplexTracing:
    """Slopes and Newton tracing of complex roots, written once for the geometries that have the two C calls (sections 12, 15
    and 18 of include/eigensolver_amd.h): root_slopes, group_velocity, newton and densify.  A class that mixes this in has ctx,
    P_TOL, problem(mode, **select) and the two calls, _slopes_call(problem, *args) and _newton_call(problem, *args), args
    being the C arguments after the problem (and, for the slab, the variant).  `select` stands for the keywords that pick the
    problem beside the mode (_SELECT: none for the slab, m for the cylinder)."""
    _SELECT = ()

    def _pairs(self, mode, k, w, **select):
        """(problem, k, Re w, Im w) on the device, k broadcast against the complex w; tensors are taken as they are."""
        import torch
        p = self.problem(mode, **select)
        dev = f"cuda:{self.ctx.device}"
        if isinstance(w, torch.Tensor):
            w = w.to(device=dev, dtype=torch.complex128).reshape(-1)
        else:
            w = torch.as_tensor(np.asarray(w, dtype=complex).reshape(-1), device=dev)
        dk = torch.broadcast_to(p._dev(k).reshape(-1), w.shape).contiguous()
        return p, dk, w.real.contiguous(), w.imag.contiguous()

    @staticmethod
    def _count_ptr(count):
        import torch
        if count is None:
            return None
        assert count.is_cuda and count.numel() >= 1 and count.dtype == torch.int32
        return _lib.ptr(count)

    def root_slopes(self, mode, k, w, count=None, **select):
        """The root-slopes call at the complex (k, omega) pairs: D_c of eval_points with its exact derivatives in omega
        (holomorphic) and k, a tangent-linear march with no difference step -> ComplexRootSlopes.  k is broadcast against
        w; both may be tensors.  count: an int32 CUDA tensor holding the number of valid pairs; entries past
        min(count, n) are left as allocated.  Nothing is read back."""
        import torch
        p, dk, dre, dim = self._pairs(mode, k, w, **select)
        n, dev = dk.numel(), dk.device
        outer = torch.empty((3, n), dtype=torch.complex128, device=dev)
        inner = torch.empty((3, n), dtype=torch.complex128, device=dev)
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        rc = self._slopes_call(p, _lib.ptr(dk), _lib.ptr(dre), _lib.ptr(dim), n, self._count_ptr(count), _lib.ptr(outer),
                               _lib.ptr(inner), _lib.ptr(st))
        _lib.check(self.ctx.handle, rc)
        diff = outer - inner
        return ComplexRootSlopes(outer, inner, diff[0], diff[1], diff[2], st)

    def group_velocity(self, mode, roots, count=None, **select):
        """d omega / dk (complex) of every entry of a find_roots table: -D_k / D_w, a CUDA tensor."""
        t = roots[0] if isinstance(roots, tuple) else roots
        return self.root_slopes(mode, t["k"], t["w"], count=count, **select).group_velocity

    def newton(self, mode, k, w0, max_iter=8, step_cap=None, max_shift=None, tol_percent=None, count=None, **select):
        """The Newton call from the guesses w0 at fixed k (broadcast against w0): dict of CUDA tensors w (complex128),
        resid (percent), iters, flag (int32) and dwdk (complex128, -D_k / D_w at the final w).  step_cap caps the length
        of a step, max_shift the distance |w - w0| an accepted root may have travelled (both default to no limit);
        tol_percent defaults to P_TOL.  flag = 1: the iteration met no leaky or singular point, the final point is
        ES_PT_OK, resid < tol_percent and |w - w0| <= max_shift.  Nothing is read back."""
        import torch
        p, dk, gre, gim = self._pairs(mode, k, w0, **select)
        n, dev = dk.numel(), dk.device
        wre, wim, resid = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
        dwdk = torch.empty(n, dtype=torch.complex128, device=dev)
        iters, flag = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        rc = self._newton_call(p, _lib.ptr(dk), _lib.ptr(gre), _lib.ptr(gim), n, self._count_ptr(count), int(max_iter),
                               DBL_MAX if step_cap is None else min(float(step_cap), DBL_MAX),
                               DBL_MAX if max_shift is None else min(float(max_shift), DBL_MAX),
                               self.P_TOL if tol_percent is None else float(tol_percent), _lib.ptr(wre), _lib.ptr(wim),
                               _lib.ptr(resid), _lib.ptr(dwdk), _lib.ptr(iters), _lib.ptr(flag))
        _lib.check(self.ctx.handle, rc)
        return dict(w=torch.complex(wre, wim), resid=resid, iters=iters, flag=flag, dwdk=dwdk)

    def densify(self, mode, k, w, k_fine, shift_factor=4.0, **newton_kw):
        """One branch traced to the wavenumbers k_fine from a coarse scan: k strictly increasing with the roots w on it.
        (1) root_slopes at the coarse roots, (2) the complex piecewise-cubic Hermite prediction at k_fine (the cubic of the
        end interval continued outside [k[0], k[-1]]), formed on the device, (3) one newton call over all fine points.
        Dict of CUDA tensors k, w, dwdk, resid, iters, flag, predicted and max_shift.  Nothing is read back.
        max_shift: a number from the caller goes to newton as it is.  Left out, every fine point gets the bound of its
        coarse interval [k_j, k_j+1], shift_factor (4) times the larger of the interval's two end-point Hermite defects
            |w_j+1 - w_j - h s_j|,  |w_j+1 - w_j - h s_j+1|      (s = d omega / dk, h = k_j+1 - k_j)
        -- how far the tangent from one end misses the root at the other, a scale for how far the curve bends inside the
        interval and so for how far the cubic can lie from it -- and no less than 1e-8 max(1, |w_j|); newton then runs
        without a limit and the flag is cleared, on the device, where |w - predicted| exceeds the bound."""
        import torch
        select = {name: newton_kw.pop(name) for name in self._SELECT if name in newton_kw}
        p, dk, dre, dim = self._pairs(mode, k, w, **select)
        wc = torch.complex(dre, dim)
        if dk.numel() < 2:
            raise ValueError("densify needs at least two coarse rows")
        kf = p._dev(k_fine).reshape(-1)
        s = self.root_slopes(mode, dk, wc, **select).group_velocity
        pred, bound = hermite_guess(dk, wc, s, kf, shift_factor)
        given = newton_kw.get("max_shift") is not None
        out = self.newton(mode, kf, pred, **newton_kw, **select)
        if given:
            out["max_shift"] = torch.full_like(kf, float(newton_kw["max_shift"]))
        else:
            out["flag"] = torch.where((out["w"] - pred).abs() <= bound, out["flag"], torch.zeros_like(out["flag"]))
            out["max_shift"] = bound
        out["k"] = kf
        out["predicted"] = pred
        return out


class SlabComplexFlow(ComplexTracing):
    """Complex-frequency flow slab: D_c on (k, Re omega, Im omega) grids, roots, and the reference's worker signature."""
    P_TOL = 4.0                                     # SF-X:301

    def __init__(self, U_i0=1.4, width=1e5, variant="sfx", ctx=None, equilibrium=None, **kw):
        self.eq = equilibrium if equilibrium is not None else SlabFlowKH(U_i0=U_i0, width=width, **kw)
        self.variant = {"sfx": CX_SFX, "sfg": CX_SFG}[variant]
        self.ctx = ctx or _lib.Context()
        self._problems = {}

    def problem(self, mode):
        if mode not in self._problems:
            self._problems[mode] = ShootProblem(self.eq, mode, ctx=self.ctx)
        return self._problems[mode]

    def close(self):
        for p in self._problems.values():
            p.close()
        self._problems = {}

    # ---- evaluation ------------------------------------------------------------------------------------------------
    def eval_grid(self, mode, k, w_re, w_im, w_mode=W_ABSOLUTE):
        """D_c[nk, n_im, n_re] (complex128 tensor), status[nk, n_im, n_re], rel[nk, n_im, n_re]."""
        import torch
        p = self.problem(mode)
        dk, dre, dim = p._dev(k).reshape(-1), p._dev(w_re).reshape(-1), p._dev(w_im).reshape(-1)
        nk, nre, nim = dk.numel(), dre.numel(), dim.numel()
        Dre = torch.empty((nk, nim, nre), dtype=torch.float64, device=dk.device)
        Dim = torch.empty_like(Dre)
        rel = torch.empty_like(Dre)
        st = torch.empty((nk, nim, nre), dtype=torch.uint8, device=dk.device)
        rc = self.ctx.lib.es_complex_eval_grid(self.ctx.handle, p.handle, self.variant, _lib.ptr(dk), nk, _lib.ptr(dre), nre,
                                               _lib.ptr(dim), nim, int(w_mode), _lib.ptr(Dre), _lib.ptr(Dim),
                                               _lib.ptr(rel), _lib.ptr(st))
        _lib.check(self.ctx.handle, rc)
        return torch.complex(Dre, Dim), st, rel

    def eval_points(self, mode, k, w):
        import torch
        p = self.problem(mode)
        w = np.asarray(w, dtype=complex).reshape(-1)
        dk = p._dev(np.broadcast_to(np.asarray(k, dtype=float), w.shape).copy())
        dre, dim = p._dev(w.real.copy()), p._dev(w.imag.copy())
        n = dk.numel()
        Dre = torch.empty(n, dtype=torch.float64, device=dk.device)
        Dim, rel = torch.empty_like(Dre), torch.empty_like(Dre)
        st = torch.empty(n, dtype=torch.uint8, device=dk.device)
        rc = self.ctx.lib.es_complex_eval_points(self.ctx.handle, p.handle, self.variant, _lib.ptr(dk), _lib.ptr(dre),
                                                 _lib.ptr(dim), n, _lib.ptr(Dre), _lib.ptr(Dim), _lib.ptr(rel), _lib.ptr(st))
        _lib.check(self.ctx.handle, rc)
        return torch.complex(Dre, Dim), st, rel

    def find_roots(self, mode, k, w_re, w_im, D, status, w_mode=W_ABSOLUTE, n_iter=12, tol_percent=None, capacity=None):
        """Cells of the (Re, Im) grid around which D_c winds once, refined by complex secant steps.
        Returns ({k, w (complex), resid, row, flag}, count)."""
        import torch
        p = self.problem(mode)
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
            rc = self.ctx.lib.es_complex_find_roots(self.ctx.handle, p.handle, self.variant, _lib.ptr(dk), nk, _lib.ptr(dre), nre,
                                                    _lib.ptr(dim), nim, int(w_mode), _lib.ptr(Dre), _lib.ptr(Dim),
                                                    _lib.ptr(status), int(n_iter), tol, C.byref(rt), C.byref(n))
            _lib.check(self.ctx.handle, rc, allow_capacity=True)
            if rc == 3 and capacity is None:
                cap = n.value
                continue
            m = min(n.value, cap)
            out = {"k": t["k"][:m], "w": torch.complex(t["w_re"][:m], t["w_im"][:m]), "resid": t["resid"][:m],
                   "row": t["row"][:m], "flag": t["flag"][:m]}
            return out, n.value

    def eigenfunction(self, mode, k, w, n_ext=500):
        """Two-region solution at the complex (k, omega) pairs (es_complex_eigenfunction; replaces the solves of
        complex_imag_flow_analysis.py:998-1043).  `w` is complex and `k` is broadcast against it, as in eval_points;
        both may be tensors, e.g. roots["k"], roots["w"] of find_roots.  Dict of CUDA tensors: x_int [N],
        value_int / flux_int [n, N] (complex128: Vx and P_T on the node grid, node 0 = boundary), x_ext [n, n_ext],
        value_ext / flux_ext [n, n_ext] (complex128, far field to boundary), status [n] (uint8, that of eval_points;
        rows that are not ES_PT_OK are NaN).  Scaled per unit V_e(-1): value_ext[:, -1] = 1 and
        flux_ext[:, -1] - flux_int[:, 0] = D_c.  The reference's plot normalisation -- real and imaginary parts divided by
        the maxima of the exterior real and imaginary parts, :1009-1043 -- is a host-side step on these arrays."""
        import torch
        p = self.problem(mode)
        dev = f"cuda:{self.ctx.device}"
        if isinstance(w, torch.Tensor):
            w = w.to(device=dev, dtype=torch.complex128).reshape(-1)
        else:
            w = torch.as_tensor(np.asarray(w, dtype=complex).reshape(-1), device=dev)
        dk = torch.broadcast_to(p._dev(k).reshape(-1), w.shape).contiguous()
        dre, dim = w.real.contiguous(), w.imag.contiguous()
        n, N, n_ext = w.numel(), int(p.desc.n_nodes), int(n_ext)
        vi = torch.empty((n, N), dtype=torch.complex128, device=dev)
        fi = torch.empty((n, N), dtype=torch.complex128, device=dev)
        xe = torch.empty((n, n_ext), dtype=torch.float64, device=dev)
        ve = torch.empty((n, n_ext), dtype=torch.complex128, device=dev)
        fe = torch.empty((n, n_ext), dtype=torch.complex128, device=dev)
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        rc = self.ctx.lib.es_complex_eigenfunction(self.ctx.handle, p.handle, self.variant, _lib.ptr(dk), _lib.ptr(dre),
                                                   _lib.ptr(dim), n, _lib.ptr(vi), _lib.ptr(fi), n_ext, _lib.ptr(xe),
                                                   _lib.ptr(ve), _lib.ptr(fe), _lib.ptr(st))
        _lib.check(self.ctx.handle, rc)
        x_int = torch.linspace(p.desc.x_boundary, p.desc.x_end, N, dtype=torch.float64, device=dev)
        return dict(x_int=x_int, value_int=vi, flux_int=fi, x_ext=xe, value_ext=ve, flux_ext=fe, status=st)

    # ---- slopes and Newton tracing (C ABI section 12): ComplexTracing over these two calls ----------------------------------
    def _slopes_call(self, p, *args):
        return self.ctx.lib.es_complex_root_slopes(self.ctx.handle, p.handle, self.variant, *args)

    def _newton_call(self, p, *args):
        return self.ctx.lib.es_complex_newton(self.ctx.handle, p.handle, self.variant, *args)

    # ---- perturbation fields (C ABI section 9) -----------------------------------------------------------------------
    def polarisation(self, mode, k, w, n_ext=500, reference_quirks=True):
        """Complex amplitudes of the modes at the complex (k, omega) pairs (es_slab_polarisation on the arrays of
        `eigenfunction`; k is broadcast against w): dict of CUDA tensors x [n, 2 n_ext + N], amp [n, 6, 2 n_ext + N]
        (complex128, channels _lib.SAMP_NAMES) and status [n].  Every field is Re[amp e^{i (k z - w t)}], growth factor
        e^{Im w t} included.  reference_quirks=False adds the shear term of linear theory to the "sfg" flux; the "sfx" flux
        carries the script's own term already, so False is an error for it.  Rows that are not ES_PT_OK are NaN."""
        import torch
        from . import shooting
        if not reference_quirks and self.variant == CX_SFX:
            raise ValueError('the "sfx" flux already carries its U\' term (SF-X:401): reference_quirks=False is for "sfg"')
        shooting._require_exterior_points(n_ext)
        p = self.problem(mode)
        e = self.eigenfunction(mode, k, w, n_ext=n_ext)
        dev = e["value_int"].device
        if isinstance(w, torch.Tensor):
            wt = w.to(device=dev, dtype=torch.complex128).reshape(-1)
        else:
            wt = torch.as_tensor(np.asarray(w, dtype=complex).reshape(-1), device=dev)
        dk = torch.broadcast_to(p._dev(k).reshape(-1), wt.shape).contiguous()
        out = p._slab_polarisation_of(e, dk, wt.real.contiguous(), wt.imag.contiguous(), reference_quirks)
        out["status"] = e["status"]
        return out

    def fields(self, mode, k, w, x, z, t, variables=None, v_scale=1.0, fill=float("nan"), big_endian=False,
               frames_per_call=None, n_ext=500, reference_quirks=True):
        """Fields of ONE complex root (k, omega) of `mode` on the mesh (x, z, t), as ShootProblem.slab_fields returns them:
        dict of x, z, t, names, frames [n_t, n_sel, n_z, n_x] float32 and <name>: frames[:, i], or with frames_per_call a
        generator of such dicts.  The frames grow (or decay) as e^{Im w t}."""
        from . import shooting
        if np.ndim(k) != 0 or np.ndim(w) != 0:
            raise ValueError("fields() takes one root: scalar k and omega")
        mask, names = shooting.slab_var_mask(variables)
        tab = self.polarisation(mode, [float(k)], [complex(w)], n_ext=n_ext, reference_quirks=reference_quirks)
        p = self.problem(mode)
        dx, dz, dt = (p._dev(a).reshape(-1) for a in (x, z, t))
        return shooting.slab_frames(self.ctx, tab["x"][0], tab["amp"][0], int(p.desc.n_nodes), int(n_ext), float(k),
                                    complex(w), dx, dz, dt, names, v_scale, fill, big_endian, frames_per_call)

    # ---- the reference's worker signature --------------------------------------------------------------------------
    def _worker(self, mode, wavenumber, ws, ks, ws_imag, ks_imag, freq):
        freq = np.asarray(freq, dtype=complex).reshape(-1)
        k = np.array([float(wavenumber)])
        w_re, w_im = np.ascontiguousarray(freq.real), np.ascontiguousarray(freq.imag)
        D, st, rel = self.eval_grid(mode, k, w_re, w_im, W_ABSOLUTE)
        roots, n = self.find_roots(mode, k, w_re, w_im, D, st, W_ABSOLUTE)
        ok = roots["flag"].cpu().numpy() == 1
        w = _distinct(roots["w"].cpu().numpy()[ok])
        kk = [float(wavenumber)] * len(w)
        ks.put(list(kk)); ws.put([float(x) for x in w.real])                       # SF-X:1095-1096
        ks_imag.put(list(kk)); ws_imag.put([float(x) for x in w.imag])             # SF-X:1097-1098

    def sausage(self, wavenumber, sausage_ws, sausage_ks, sausage_ws_imag, sausage_ks_imag, freq):
        self._worker("sausage", wavenumber, sausage_ws, sausage_ks, sausage_ws_imag, sausage_ks_imag, freq)

    def kink(self, wavenumber, kink_ws, kink_ks, kink_ws_imag, kink_ks_imag, freq):
        self._worker("kink", wavenumber, kink_ws, kink_ks, kink_ws_imag, kink_ks_imag, freq)

    def solve(self, wavenumbers, speeds=(-0.5, 0.0, 0.5, 1.0), n_re=10, im_range=(-0.25, 0.25), n_im=10, modes=("kink",),
              n_iter=12, tol_percent=None):
        """The driver block SF-X:1115-1135 in one batch per (mode, band): returns {mode: (omega complex array, k array)}."""
        ks = np.asarray(wavenumbers, dtype=float)
        sp = sorted(speeds)                                                        # SF-X:231-235
        out = {}
        for mode in modes:
            w_all, k_all = [], []
            for i in range(len(sp) - 1):
                W_re = np.linspace(sp[i], sp[i + 1], n_re)
                # Re(omega) scales with k but Im(omega) is absolute in the reference's driver (SF-X:1127), so the
                # (Re, Im) grid differs per k: one call per (k, band) with absolute frequencies.
                for k in ks:
                    w_re, w_im = W_re * k, np.linspace(im_range[0], im_range[1], n_im)
                    D, st, rel = self.eval_grid(mode, np.array([k]), w_re, w_im, W_ABSOLUTE)
                    roots, n = self.find_roots(mode, np.array([k]), w_re, w_im, D, st, W_ABSOLUTE, n_iter=n_iter,
                                               tol_percent=tol_percent)
                    ok = roots["flag"].cpu().numpy() == 1
                    w = _distinct(roots["w"].cpu().numpy()[ok])
                    w_all.append(w)
                    k_all.append(np.full(len(w), k))
            out[mode] = (np.concatenate(w_all) if w_all else np.zeros(0, complex), np.concatenate(k_all) if k_all else np.zeros(0))
        return out
