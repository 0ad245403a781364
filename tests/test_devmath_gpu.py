"""The device build of csrc/es_bessel.hpp, one evaluation per thread (tests/devmath/devmath_probe.hip, built by
eigensolver_amd/build.py into lib/libes_devmath_probe.so), against correctly rounded values (tests/golden/bessel_truth.npz:
mpmath at 40 digits).  On the GPU the header takes paths the host build of tests/test_hostmath.py never sees -- qdiv on
v_rcp_f64, the __constant__ reciprocal and Chebyshev tables, the device log / exp / sqrt -- and the product reaches them
only through D.

Bound: the worst error of the host build on the same fixture, E_host (tests/bessel_truth.py::E_HOST, held by
tests/test_hostmath.py::test_truth), plus one u = 2^-52 for every operation of the device path that differs from the host's
(bessel_truth.device_margin: 3 + n for ke_pair and ie_pair_from_k, 1 for ie_pair and jy_pair).

Worst errors of the host build in u per order 0, 1, 2, 3, 5, 10, 11, 20, 40 (I, K: relative; J, Y: relative to
hypot(J_n, Y_n)), E_host:
  ke_pair         11.88  9.47  8.00  8.87  9.83 12.44 12.44 16.90 25.85
  ie_pair          9.69  9.55 11.26 12.13  9.13  9.32  6.79  6.28  6.27
  ie_pair_from_k  12.26 14.99 13.99 11.37 11.90 14.16 12.97 17.72 27.72
  jy_pair         32.07 31.76 32.37 29.87 33.48 33.11 27.81 30.94 20.96
Worst errors of the device build (MI355X, gfx950) on the same rows, both launches (same bits); the tests print them
(pytest -s) with the argument where each occurs, next to E_host and the bound:
  ke_pair         11.88  8.52  8.00  8.87  9.83 12.44 12.44 16.90 25.85
  ie_pair          9.69  9.55 11.26 12.13  9.13  9.32  6.79  6.28  6.27
  ie_pair_from_k  12.26 14.99 13.99 11.37 11.90 14.16 12.97 17.72 26.45
  jy_pair         32.07 31.76 32.37 29.87 33.48 33.11 27.81 30.94 20.96
The worst rows are the host's (x = 2 - 2^-52 for K, 47.5 for the I series, 63.2 for J/Y): the error there is the
algorithm's, and the device's own operations move it by less than one u.
qdiv: worst 1.467 ulp of the exact quotient, 1 ulp of the correctly rounded one, 74 % of 10^6 results correctly rounded.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import bessel_truth as bt

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PROBE = os.path.join(HERE, "..", "eigensolver_amd", "lib", "libes_devmath_probe.so")


@pytest.fixture(scope="module")
def probe(es_ctx):
    """The probe library (after torch, as the product library: one HIP runtime in the process) and the stream of the
    session's context."""
    import torch  # noqa: F401
    assert os.path.exists(PROBE), f"{PROBE} not found: build it with `python -m eigensolver_amd.build`"
    lib = C.CDLL(PROBE)
    vp, i = C.c_void_p, C.c_int
    for name in ("dm_ke_pair", "dm_ie_pair", "dm_ie_pair_from_k"):
        getattr(lib, name).argtypes = [vp, i, vp, i, vp, vp, vp]
    lib.dm_jy_pair.argtypes = [vp, i, vp, i, vp, vp, vp, vp, vp]
    lib.dm_qdiv.argtypes = [vp, vp, i, vp, vp]
    return lib, es_ctx.torch_stream


def _evaluate(probe, func, n, x):
    """func at the rows (n[i], x[i]) on the device -> tuple of NumPy arrays.  n: an int (one order for the whole launch,
    passed as a kernel argument) or an int array (an order per thread)."""
    import torch
    lib, stream = probe
    with torch.cuda.stream(stream):
        dx = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda")
        dn = None if np.isscalar(n) else torch.as_tensor(np.ascontiguousarray(n, dtype=np.int32), device="cuda")
        outs = [torch.full((dx.numel(),), float("nan"), dtype=torch.float64, device="cuda")
                for _ in range(4 if func == "jy_pair" else 2)]
        rc = getattr(lib, "dm_" + func)(C.c_void_p(dn.data_ptr()) if dn is not None else None, int(n) if dn is None else 0,
                                        C.c_void_p(dx.data_ptr()), int(dx.numel()), *[C.c_void_p(o.data_ptr()) for o in outs],
                                        C.c_void_p(stream.cuda_stream))
        assert rc == 0, rc
        stream.synchronize()
        return tuple(o.cpu().numpy() for o in outs)


@pytest.mark.parametrize("func", bt.FUNCTIONS)
def test_device_bessel_against_truth(probe, func):
    """Each function twice -- one order per launch (wave-uniform order, as in the product) and all rows shuffled, so that
    orders and arguments differ within a wave and its lanes leave the loops at different trip counts -- gives the same
    bits per row, and the error against the correctly rounded values stays within E_host + device_margin(n)."""
    truth = bt.load()
    n, x, true = bt.points(truth, func)
    assert len(x) > 1200
    uniform = [np.full(len(x), np.nan) for _ in true]
    for order in bt.ORDERS:
        sel = np.where(n == order)[0]
        for dst, src in zip(uniform, _evaluate(probe, func, int(order), x[sel])):
            dst[sel] = src
    perm = np.random.default_rng(20240607).permutation(len(x))
    assert len(set(n[perm[:64]])) > 4                          # the first wave alone holds more than four orders
    shuffled = [np.full(len(x), np.nan) for _ in true]
    for dst, src in zip(shuffled, _evaluate(probe, func, n[perm], x[perm])):
        dst[perm] = src
    for a, b in zip(uniform, shuffled):
        differ = np.where(a.view(np.int64) != b.view(np.int64))[0]
        assert differ.size == 0, (func, differ.size, n[differ[:5]], x[differ[:5]], a[differ[:5]], b[differ[:5]])
    worst = bt.worst_per_order(n, x, bt.errors(func, tuple(uniform), true))
    for order, (err, x_at) in worst.items():
        print(f"{func} order {order}: device {err:.2f} u at x = {x_at!r}, E_host {bt.E_HOST[func][order]:.2f}, "
              f"bound {bt.E_HOST[func][order] + bt.device_margin(func, order):.2f}")
    for order, (err, x_at) in worst.items():
        # E_host + one u per device operation that differs from the host's: 3 + n (ke_pair, ie_pair_from_k), 1 (ie_pair, jy_pair)
        assert err <= bt.E_HOST[func][order] + bt.device_margin(func, order), (func, order, err, x_at)


def test_qdiv_within_two_ulp(probe):
    """qdiv(a, b) = a * (corrected v_rcp_f64 of b) on 10^6 random pairs, |a|, |b| log-uniform in [1e-150, 1e150], both
    signs: within 2 ulp of the correctly rounded quotient (the source claims about 1.5 ulp of the exact one)."""
    import torch
    assert np.finfo(np.longdouble).nmant >= 63, "the reference quotient needs an extended-precision long double"
    lib, stream = probe
    rng = np.random.default_rng(7)
    count = 1_000_000

    def operands():
        mant = rng.uniform(1.0, 10.0, count)
        return mant * 10.0 ** rng.integers(-150, 150, count) * rng.choice([-1.0, 1.0], count)
    a, b = operands(), operands()
    assert 1e-150 <= np.abs(b).min() and np.abs(b).max() <= 1e151
    with torch.cuda.stream(stream):
        da, db = torch.as_tensor(a, device="cuda"), torch.as_tensor(b, device="cuda")
        do = torch.full((count,), float("nan"), dtype=torch.float64, device="cuda")
        rc = lib.dm_qdiv(C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()), count, C.c_void_p(do.data_ptr()),
                         C.c_void_p(stream.cuda_stream))
        assert rc == 0, rc
        stream.synchronize()
        got = do.cpu().numpy()
    exact = a.astype(np.longdouble) / b.astype(np.longdouble)      # 64-bit significand: exact to 2^-12 ulp of a double
    rounded = a / b                                                # the IEEE quotient of the host: correctly rounded
    ulp = np.spacing(np.abs(rounded))
    err_rounded = np.abs(got - rounded) / ulp
    err_exact = (np.abs(got.astype(np.longdouble) - exact) / ulp.astype(np.longdouble)).astype(np.float64)
    i = int(np.argmax(err_exact))
    print(f"qdiv: worst {err_exact[i]:.3f} ulp of the exact quotient (a = {a[i]!r}, b = {b[i]!r}), "
          f"{err_rounded.max():.0f} ulp of the rounded one; {np.mean(got == rounded):.4f} of the results correctly rounded")
    assert np.all(np.isfinite(got))
    assert err_rounded.max() <= 2.0 and err_exact.max() <= 2.0
