"""Uniform cylinder in closed form (Bessel I/K/J/Y on the GPU, es_cyl_uniform_eval): the benchmark case of the
reference's cylinder scripts (profile width 1e5) without integrating any ODE; es_cyl_uniform_find_roots searches the
(order, k, omega) grid for its roots in one pass."""
import ctypes as C

import numpy as np

from . import _lib
from . import equilibrium as eqm


class CylinderUniform:
    def __init__(self, eq=None, mode="kink", m=None, U_i=0.0, ctx=None):
        self.ctx = ctx if ctx is not None else _lib.Context()
        eq = eq if eq is not None else eqm.CylinderFlow()
        mm = (1 if mode == "kink" else 0) if m is None else int(m)
        self.params = _lib.CylUniformParams(eq.c_i0, eq.vA_i0, eq.rho_i0, float(U_i), eq.rho_e, eq.vA_e, eq.c_e,
                                            eq.cT_e, eq.x_boundary, eq.r_axis, eq.L_factor, eq.ic[0], eq.ic[1],
                                            mm, mm, 1 if mode == "sausage" else 0, 0)

    def eval_grid(self, k, w, w_mode=1, want_rel=False):
        import torch
        dev = f"cuda:{self.ctx.device}"
        def to_dev(a):
            if isinstance(a, torch.Tensor):
                return a.to(device=dev, dtype=torch.float64).contiguous()
            return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
        dk = to_dev(k).reshape(-1)
        dw = to_dev(w)
        nk = dk.numel()
        nw = dw.shape[-1] if w_mode == 2 else dw.numel()
        D = torch.empty((nk, nw), dtype=torch.float64, device=dev)
        st = torch.empty((nk, nw), dtype=torch.uint8, device=dev)
        rel = torch.empty((nk, nw), dtype=torch.float64, device=dev) if want_rel else None
        rc = self.ctx.lib.es_cyl_uniform_eval(self.ctx.handle, C.byref(self.params), _lib.ptr(dk), nk, _lib.ptr(dw),
                                              nw, w_mode, _lib.ptr(D), _lib.ptr(rel) if want_rel else None,
                                              _lib.ptr(st))
        _lib.check(self.ctx.handle, rc)
        return (D, st, rel) if want_rel else (D, st)

    # ---- root search over (order, k, omega): es_cyl_uniform_find_roots ------------------------------------------------
    def _dev(self, a):
        import torch
        dev = f"cuda:{self.ctx.device}"
        if isinstance(a, torch.Tensor):
            return a.to(device=dev, dtype=torch.float64).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)

    def _orders(self, orders):
        """(m_first, n_orders) of `orders`: None = the order of this object, else a contiguous ascending range or list."""
        if orders is None:
            return int(self.params.m), 1
        ms = [int(m) for m in orders]
        if not ms:
            return 0, 0
        if ms != list(range(ms[0], ms[0] + len(ms))):
            raise ValueError("orders must be contiguous and ascending (m_first, m_first + 1, ...)")
        return ms[0], len(ms)

    def alloc_root_table(self, capacity):
        """(dict, RootTable) as ShootProblem.alloc_root_table, with the int32 column `order` beside it."""
        import torch
        dev = f"cuda:{self.ctx.device}"
        t = {n: torch.empty(capacity, dtype=torch.float64, device=dev) for n in ("k", "w", "w_lo", "w_hi", "resid")}
        t["row"] = torch.empty(capacity, dtype=torch.int32, device=dev)
        t["order"] = torch.empty(capacity, dtype=torch.int32, device=dev)
        t["flag"] = torch.empty(capacity, dtype=torch.uint8, device=dev)
        rt = _lib.RootTable(t["k"].data_ptr(), t["w"].data_ptr(), t["w_lo"].data_ptr(), t["w_hi"].data_ptr(),
                            t["resid"].data_ptr(), t["row"].data_ptr(), t["flag"].data_ptr(), capacity)
        return t, rt

    def _grid(self, dk, dw, w_mode, n_orders, want_grid):
        import torch
        nk = dk.numel()
        nw = dw.shape[-1] if w_mode == 2 else dw.numel()
        if not want_grid:
            return nk, nw, None, None
        D = torch.empty((n_orders, nk, nw), dtype=torch.float64, device=dk.device)
        st = torch.empty((n_orders, nk, nw), dtype=torch.uint8, device=dk.device)
        return nk, nw, D, st

    def find_roots(self, k, w, orders=None, w_mode=1, n_bisect=40, tol_percent=1e-3, capacity=None, want_grid=False):
        """Evaluate, bracket, refine and classify in one call.  Returns (dict, count) with the tensors k, w, w_lo, w_hi,
        resid, row, order, flag (order outer, row next, omega inner), count the number of brackets; with want_grid=True
        (dict, count, D, status), D and status of shape (n_orders, nk, nw).  capacity=None: the table is sized by a guess
        and the call repeated once at the returned count if that was too small; a given capacity is kept, and the count
        may then exceed the length of the tensors."""
        dk, dw = self._dev(k).reshape(-1), self._dev(w)
        m_first, n_orders = self._orders(orders)
        nk, nw, D, st = self._grid(dk, dw, w_mode, n_orders, want_grid)
        cap = int(capacity) if capacity is not None else max(1024, 16 * nk * max(n_orders, 1))
        while True:
            t, rt = self.alloc_root_table(cap)
            n = C.c_int(0)
            rc = self.ctx.lib.es_cyl_uniform_find_roots(
                self.ctx.handle, C.byref(self.params), m_first, n_orders, _lib.ptr(dk), nk, _lib.ptr(dw), nw, w_mode,
                int(n_bisect), float(tol_percent), _lib.ptr(D) if want_grid else None,
                _lib.ptr(st) if want_grid else None, C.byref(rt), _lib.ptr(t["order"]), C.byref(n))
            _lib.check(self.ctx.handle, rc, allow_capacity=True)
            if rc == 3 and capacity is None:
                cap = n.value
                continue
            m = min(n.value, rt.capacity)
            out = {key: v[:m] for key, v in t.items()}
            return (out, n.value, D, st) if want_grid else (out, n.value)

    def find_roots_async(self, k, w, table, count, orders=None, w_mode=1, n_bisect=40, tol_percent=1e-3, D=None,
                         status=None):
        """es_cyl_uniform_find_roots_async: everything enqueued on the context's stream, nothing read back.  `table` is
        (dict, RootTable) from alloc_root_table, `count` an int32 CUDA tensor of one element that receives the bracket
        count (it may exceed the capacity: check when reading it).  D / status: optional (n_orders, nk, nw) float64 /
        uint8 CUDA tensors that receive the grid.  Returns the full-capacity dict of the table."""
        dk, dw = self._dev(k).reshape(-1), self._dev(w)
        m_first, n_orders = self._orders(orders)
        nk, nw, _, _ = self._grid(dk, dw, w_mode, n_orders, False)
        t, rt = table
        assert count.is_cuda and count.numel() == 1 and count.element_size() == 4
        for a, size in ((D, 8), (status, 1)):
            assert a is None or (a.is_cuda and a.numel() == n_orders * nk * nw and a.element_size() == size)
        rc = self.ctx.lib.es_cyl_uniform_find_roots_async(
            self.ctx.handle, C.byref(self.params), m_first, n_orders, _lib.ptr(dk), nk, _lib.ptr(dw), nw, w_mode,
            int(n_bisect), float(tol_percent), _lib.ptr(D) if D is not None else None,
            _lib.ptr(status) if status is not None else None, C.byref(rt), _lib.ptr(t["order"]), _lib.ptr(count))
        _lib.check(self.ctx.handle, rc)
        return t
