"""CPU-side checks of es_shoot_newton (include/eigensolver_amd.h section 13): the header declares it with the arguments the
ctypes binding passes, the built library exports it, and the host pieces of the tracing -- postprocess.traced_curves and the
shared Hermite helper -- do what the GPU path relies on, on CPU tensors."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "es_shoot_newton"


def test_header_declares_and_library_exports_the_newton_call():
    txt = open(os.path.join(ROOT, "include", "eigensolver_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\);", txt)
    assert m, NAME
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["es_context* ctx", "const es_problem* prob", "const double* d_k", "const double* d_guess", "int n",
                      "const int32_t* d_count", "int max_iter", "double step_cap", "double max_shift", "double tol_percent",
                      "double* d_w", "double* d_resid", "double* d_dwdk", "int32_t* d_iters", "int32_t* d_flag",
                      "uint8_t* d_status"], params
    from eigensolver_amd import build
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, NAME)
    assert hasattr(ctypes.CDLL(build.LIB_IEEE), NAME)


def test_ctypes_signature_covers_the_newton_call():
    from eigensolver_amd import _lib

    class Fake:
        def __getattr__(self, name):
            f = type("F", (), {})()
            object.__setattr__(self, name, f)
            return f
    lib = _lib._sig(Fake())
    args = getattr(lib, NAME).argtypes
    assert len(args) == 16 and args[7:10] == [ctypes.c_double] * 3 and args[4] == args[6] == ctypes.c_int


def test_hermite_guess_is_the_numpy_hermite_real_and_complex():
    import torch
    from eigensolver_amd import postprocess as pp
    from eigensolver_amd.shooting import hermite_guess, hermite_guess_in
    from tests import real_newton_model as N
    rng = np.random.default_rng(5)
    k = np.cumsum(rng.uniform(0.2, 0.6, 7))
    kf = np.concatenate([k, rng.uniform(k[0] - 0.1, k[-1] + 0.1, 40)])
    for cplx in (False, True):
        w = np.sin(k) + (0.3j * np.cos(2 * k) if cplx else 0.0)
        s = np.cos(k) - (0.6j * np.sin(2 * k) if cplx else 0.0)
        pred, bound = (t.numpy() for t in hermite_guess(*(torch.as_tensor(a) for a in (k, w, s, kf))))
        want = (pp.hermite_branch_complex if cplx else pp.hermite_branch)(k, w, s)(kf)
        assert pred.dtype == (np.complex128 if cplx else np.float64) and np.max(np.abs(pred - want)) <= 1e-14
        assert bound.dtype == np.float64 and np.all(bound >= 1e-8)
        if not cplx:
            p2, b2 = N.hermite(k, w, s, kf)
            assert np.max(np.abs(pred - p2)) <= 1e-14 and np.max(np.abs(bound - b2) / b2) <= 1e-12
    # two branches one after the other, the interval of every fine point given
    k2 = np.concatenate([k, k[:4]])
    w2, s2 = np.concatenate([np.sin(k), np.cos(k[:4])]), np.concatenate([np.cos(k), -np.sin(k[:4])])
    kq = np.array([k[0] + 0.05, k[1] + 0.01, k[2] + 0.1])
    j = torch.as_tensor([0, len(k) + 1, len(k) + 2])
    pred, _ = hermite_guess_in(*(torch.as_tensor(a) for a in (k2, w2, s2)), j, torch.as_tensor(kq))
    want = [pp.hermite_branch(k, np.sin(k), np.cos(k))(kq[0]), *pp.hermite_branch(k[:4], np.cos(k[:4]), -np.sin(k[:4]))(kq[1:])]
    assert np.max(np.abs(pred.numpy() - np.array(want))) <= 1e-14


def test_traced_curves_layout():
    import torch
    from eigensolver_amd import postprocess as pp
    from eigensolver_amd.shooting import TracedBranches
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)     # noqa: E731
    b = dict(k=f64([0.5, 1.0, 1.5, 2.0]), w=f64([1.0, 2.1, 3.3, 4.6]), dwdk=f64([2.0, 2.2, 2.4, 2.6]),
             flag=torch.tensor([1, 0, 1, 1], dtype=torch.int32))
    for arg in ({(1, 0): b}, TracedBranches({(1, 0): b}, [(2, 2)])):
        out = pp.traced_curves(arg)
        w, k, cg = out[(1, 0)]
        assert list(out) == [(1, 0)] and k.tolist() == [0.5, 1.5, 2.0] and w.tolist() == [1.0, 3.3, 4.6]
        assert cg.tolist() == [2.0, 2.4, 2.6] and w.dtype == np.float64
        assert abs(pp.hermite_branch(k, w, cg)(1.5) - 3.3) == 0.0
        assert [a.tolist() for a in pp.pickle_layout({"kink": out[(1, 0)][:2]})] == [w.tolist(), k.tolist()]
