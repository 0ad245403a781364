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

Complex argument: csrc/es_bessel_complex.hpp and es_cjet.hpp -- cke_pair, cie_pair_from_k fed by it, their CJet<1> forms with z
the variable, and the primitives of the complex scalar -- against tests/golden/bessel_complex_truth.npz (mpmath at 40 digits;
tests/bessel_complex_truth.py).  The product reaches these only through D_c, whose tests compare with a scipy model at
1e-10 of the scale.
  A  one order per launch against all rows shuffled (more than four orders and both sides of |z| = 2 and of |z| = 0.5 in the
     first wave -- the product never has both sides of a branch in one wave): the same bits per row; component 0 of the jet
     forms is the plain routine bit for bit
  B  the error of each row with |z| <= 700 stays within E_HOST_C[func][order] + device_margin_c(row): 39 u on the series side
     of |z| = 2, 2 + P + max(0, P - 62) u beyond, P the most CF2 passes at the row's radius (144 u next to 2 ... 10 u at
     700); the rows with |z| > 700 within E_HOST_C_FAR + 7 u
  C  the primitives within the bounds of the host leg (2 u; exp 2 u + |Im z| u; divisions 3 u), signs on the cut exact
Worst errors in u per order 0, 1, 2, 3, 5, 10, 11, 20, 40 (values relative to |f|, derivatives to the terms of their identity),
host build (E_HOST_C, E_HOST_C_FAR) and device build (MI355X, gfx950; uniform and shuffled launches: same bits), as the tests
print them (pytest -s) with the argument where each occurs:
  |z| <= 700   cke_pair              host  32.08 24.04 15.60 15.60 15.08 13.67 14.13 22.26 41.54
                                     device 32.08 24.04 15.60 15.60 15.08 14.69 14.69 22.26 41.54
               cie_pair_from_k       host  16.11 15.66 14.84 15.97 15.89 14.27 14.91 20.74 37.60
                                     device 16.11 15.66 14.84 15.97 15.89 14.69 14.24 17.97 35.10
               cke_pair, d/dz        host  12.62  5.46  4.43  5.71  7.56 12.16 14.74 22.81 41.94
                                     device 12.62  5.46  4.43  5.71  7.56 12.16 14.74 22.81 41.94
               cie_pair_from_k, d/dz host   2.13  1.15  1.68  3.10  5.84  8.63 10.08 17.20 34.74
                                     device  2.13  1.15  1.54  3.10  5.84  8.43  8.71 14.09 31.92
  |z| > 700    cke_pair              both   2.86  2.86  2.86  2.86  3.51  3.46  3.46  3.35  3.10
               cie_pair_from_k       both   3.32  3.76  3.49  3.40  4.38  2.94  2.63  3.00  3.39
               cke_pair, d/dz        both   0.50  0.44  0.50  0.63  0.74  0.80  0.92  0.91  0.72
               cie_pair_from_k, d/dz both   2.17  1.47  1.91  1.74  1.76  2.50  1.97  1.68  1.08
The worst rows are the host's (|z| = 2 and 1.98 for K and I of orders up to 5, the small |z| of the upward recurrence for
K of orders 20 and 40); where the device's worst row is another one (orders 10, 11: z = 1.98 e^{0.196 i}; I of orders 20,
40: z = sqrt 2 (1 - i), the row with the most CF2 passes) it is within 1.1 u above or 2.8 u below the host's figure.
Primitives, worst in u of the modulus, device (host): cz_sqrt 0.89 (0.89), cz_log 0.67 (0.61), cz_exp 1.00 (1.00),
cz / cz 1.42 (1.42), double / cz 1.45 (1.45).

Real jets: csrc/es_jet.hpp (Jet<ND>) and es_jet2.hpp (Jet2<NV>), operator by operator, against tests/golden/jet_truth.npz
(tools/gen_bessel_truth.py jets; tests/jet_truth.py has the codes, the counting rule and the two tables of counts).  The
product reaches these only through the derivatives of D, and only the overloads its formula text happens to call.
  1  the Bessel lifts ke_pair, ie_pair_from_k (fed by ke_pair) with x the variable, in Jet<1> and Jet2<1>, on every ik row of
     bessel_truth.npz: one order per launch against all rows shuffled (more than four orders in the first wave), same bits
  2  their value components are the plain routine bit for bit, and the j part of Jet2<1> is the Jet<1> result bit for bit
  3  d/dx and d2/dx2 within E_HOST[routine][order] + device_margin + c of the identities summed at 40 digits, in u times the
     identity's magnitude (the sum of the magnitudes of its terms); c = 5 resp. 15, the operations of the identity as written
  4  the same error relative to the derivative itself, bounded only by 4 x what the magnitude predicts for the row
  5  every operator and overload (dm_jet_op, 33 codes) in Jet2<2> and Jet2<1>: the first-order part of the result is the
     Jet<NV> operator's result bit for bit, the value the plain double operation bit for bit (fast_rcp: fast_rcp of the value);
     fabs gives +0.0 and -0.0 the sign +1, pinned as the header has it
  6  every component of every row within c_op u magnitude of Taylor-polynomial arithmetic at 40 digits, c_op <= 11 the count of
     roundings of jet_truth.C_OP; jet_finite, val, the constant and the variable have exact answers
Measured on the device (MI355X, gfx950), as the tests print them (pytest -s); per order 0, 1, 2, 3, 5, 10, 11, 20, 40.
Bessel lifts, worst error in u x the identity's magnitude (bound E_HOST + margin + c: 18.0 ... 75.7 for d/dx,
28.0 ... 85.7 for d2/dx2); uniform and shuffled launches: same bits:
  ke_pair         d/dx      4.06   2.56   2.56   3.86   4.70   8.38   8.43  14.20  22.91
  ke_pair         d2/dx2    3.19   2.53   3.17   4.44   4.14   6.87   6.76  12.36  20.92
  ie_pair_from_k  d/dx      9.92   8.98   7.05   6.35   6.45   8.15   7.99  13.46  22.21
  ie_pair_from_k  d2/dx2    9.85   7.60   6.13   5.24   4.93   4.48   4.48  10.22  18.77
The same relative to the true derivative itself, in u, on x <= 60 and on x > 60, with the argument of the worst row:
  ke_pair         d1 x <= 60      38.5     64.8     86.6     70.3     29.5     13.4       12     17.2     25.6
                     at x =        1.93     47.5     47.5     47.5     41.8     47.5        2        2        2
  ke_pair         d1 x > 60        942      840      866      682      662      829      935      426      166
                     at x =         700      325      700      325      419      700      700      477      700
  ke_pair         d2 x <= 60  2.33e+03 4.02e+03 5.07e+03 3.79e+03  1.1e+03      412      335       63     25.4
                     at x =        47.5     47.5     47.5     47.5     41.8     47.5       54     41.8        2
  ke_pair         d2 x > 60   8.79e+05 6.87e+05 8.04e+05 3.89e+05 5.42e+05 6.81e+05 7.52e+05 1.77e+05  7.2e+04
                     at x =         700      700      700      700      700      700      700      477      700
  ie_pair_from_k  d1 x <= 60  1.37e+03 3.16e+03 3.09e+03  3.7e+03  4.7e+04      403      294      160     91.3
                     at x =         1.5     4.74     8.99     17.1     36.8     47.5     47.5     47.5     47.5
  ie_pair_from_k  d1 x > 60   5.76e+03 3.85e+03 4.54e+03 3.79e+03    4e+03 3.48e+04 1.78e+04    1e+05 4.11e+03
                     at x =         700      542      616      286      616      102      151      419      542
  ie_pair_from_k  d2 x <= 60  8.45e+05 3.08e+05 1.31e+06 9.81e+05 4.72e+05 4.85e+04 6.04e+04 8.13e+03      748
                     at x =       1e-06 1.67e-06     17.1     17.1     47.5       22     28.5     47.5     47.5
  ie_pair_from_k  d2 x > 60   5.38e+06  3.5e+06 3.78e+06 1.82e+06  3.5e+06 1.72e+08 1.56e+08 7.86e+07 7.63e+06
                     at x =         700      700      616      616      616      221      221      700      286
Operators, worst error in u x magnitude over all components, Jet2<2> / Jet2<1> (c_op):
  neg 0.00 / 0.00 (0), add 0.00 / 0.00 (1), sub 0.00 / 0.00 (1), add_jd 0.00 / 0.00 (1), add_dj 0.00 / 0.00 (1),
  sub_jd 0.00 / 0.00 (1), sub_dj 0.00 / 0.00 (1), mul_jd 0.00 / 0.00 (1), mul_dj 0.00 / 0.00 (1),
  mul_assign 0.00 / 0.00 (1), mul 0.99 / 0.99 (4), fma_jjj 0.99 / 0.97 (5), fma_djj 0.00 / 0.00 (1),
  fma_jjd 0.98 / 0.98 (4), fma_djd 0.00 / 0.00 (1), fma_jdj 0.00 / 0.00 (1), fma_jdd 0.00 / 0.00 (1),
  rcp_from 1.84 / 1.82 (8), rcp 1.84 / 1.49 (8), fast_rcp 1.48 / 1.43 (11), div 1.93 / 1.39 (11), div_dj 1.28 / 1.28 (9),
  div_jd 0.00 / 0.00 (1), sqrt 3.05 / 3.05 (10), exp 0.99 / 0.99 (3), ldexp 0.00 / 0.00 (0), lift_onto 1.00 / 0.96 (3),
  lift 1.00 / 1.00 (3), fabs 0.00 / 0.00 (0)
In the identity's own units the lifts stay below the value error of their routine at every order; relative to the derivative
the K pair loses x (d/dx) resp. x^2 (d2/dx2) -- 5e3 u = 1.1e-12 at x = 47.5, 8.8e5 u = 2e-10 at 700 -- and the I pair the same
away from the sign changes of its derivatives, beside which (x = 17.1, 221, the smallest x of order 0) the relative figure
has no meaning.  No operator is above a third of its count; a single correctly rounded operation shows as 0.00 because the
truth rounds to the same double.
"""

import ctypes as C
import os

import numpy as np
import pytest

from tests import bessel_complex_truth as bc
from tests import bessel_truth as bt
from tests import jet_truth as jt

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
    for name in ("dm_cke_pair", "dm_cie_pair_from_k"):
        getattr(lib, name).argtypes = [vp, i, vp, i, vp, vp, vp]
    for name in ("dm_cke_pair_jet", "dm_cie_pair_from_k_jet"):
        getattr(lib, name).argtypes = [vp, i, vp, i, vp, vp, vp, vp, vp]
    lib.dm_cz_primitive.argtypes = [i, vp, vp, i, vp, vp]
    for name in ("dm_ke_pair_jets", "dm_ie_pair_from_k_jets"):
        getattr(lib, name).argtypes = [vp, i, vp, i, vp, vp]
    lib.dm_jet_op.argtypes = [i, i] + [vp] * 7 + [i] + [vp] * 4
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


# ---- complex argument ------------------------------------------------------------------------------------------------------------
def _evaluate_complex(probe, launcher, n, z):
    """launcher (dm_cke_pair ... dm_cie_pair_from_k_jet) at the rows (n[i], z[i]) -> tuple of complex NumPy arrays: the two
    values, for a jet launcher also the two derivatives.  n: an int (one order for the launch) or an int array."""
    import torch
    lib, stream = probe
    with torch.cuda.stream(stream):
        dz = torch.as_tensor(np.ascontiguousarray(z, dtype=np.complex128), device="cuda")
        dn = None if np.isscalar(n) else torch.as_tensor(np.ascontiguousarray(n, dtype=np.int32), device="cuda")
        assert dn is None or dn.numel() == dz.numel()
        outs = [torch.full((dz.numel(),), complex("nan+nanj"), dtype=torch.complex128, device="cuda")
                for _ in range(4 if launcher.endswith("_jet") else 2)]
        rc = getattr(lib, launcher)(C.c_void_p(dn.data_ptr()) if dn is not None else None, int(n) if dn is None else 0,
                                    C.c_void_p(dz.data_ptr()), int(dz.numel()), *[C.c_void_p(o.data_ptr()) for o in outs],
                                    C.c_void_p(stream.cuda_stream))
        assert rc == 0, rc
        stream.synchronize()
        return tuple(o.cpu().numpy() for o in outs)


COMPLEX_LAUNCHERS = ("dm_cke_pair", "dm_cie_pair_from_k", "dm_cke_pair_jet", "dm_cie_pair_from_k_jet")


def complex_permutation(truth):
    """All rows shuffled so that the first wave (64 rows) holds more than four orders and, within 1e-9 of either branch
    point, rows on both sides of re^2 + im^2 <= 4 (cke01) and of hypot < 0.5 (cie_pair_from_k)."""
    n, z = truth["c_n"], truth["c_z"]
    perm = np.random.default_rng(4).permutation(len(z))
    first = perm[:64]
    abs2, hyp = (z.real * z.real + z.imag * z.imag)[first], np.hypot(z.real, z.imag)[first]
    near2, near05 = np.abs(hyp - 2.0) < 1e-9, np.abs(hyp - 0.5) < 1e-9
    assert len(set(n[first])) > 4
    assert (abs2[near2] <= 4.0).any() and (abs2[near2] > 4.0).any()
    assert (hyp[near05] < 0.5).any() and (hyp[near05] >= 0.5).any()
    return perm


@pytest.fixture(scope="module")
def complex_runs(probe):
    """(truth, uniform, shuffled): per launcher the device results on every row of the fixture, once with one order per
    launch and once with all rows shuffled into one launch"""
    truth = bc.load()
    n, z = truth["c_n"], truth["c_z"]
    assert len(z) > 3500
    perm = complex_permutation(truth)
    uniform, shuffled = {}, {}
    for launcher in COMPLEX_LAUNCHERS:
        nout = 4 if launcher.endswith("_jet") else 2
        uniform[launcher] = [np.full(len(z), complex(np.nan, np.nan)) for _ in range(nout)]
        for order in bc.ORDERS:
            sel = np.where(n == order)[0]
            for dst, src in zip(uniform[launcher], _evaluate_complex(probe, launcher, int(order), z[sel])):
                dst[sel] = src
        shuffled[launcher] = [np.full(len(z), complex(np.nan, np.nan)) for _ in range(nout)]
        for dst, src in zip(shuffled[launcher], _evaluate_complex(probe, launcher, n[perm], z[perm])):
            dst[perm] = src
    return truth, uniform, shuffled


def _differ(a, b):
    return np.where(np.any(a.view(np.int64).reshape(-1, 2) != b.view(np.int64).reshape(-1, 2), axis=1))[0]


@pytest.mark.parametrize("launcher", COMPLEX_LAUNCHERS)
def test_complex_uniform_against_shuffled(complex_runs, launcher):
    """A: every row gives the same bits with a wave-uniform order, as in the product, and in a launch whose waves mix orders,
    both sides of either branch and loops of every length."""
    truth, uniform, shuffled = complex_runs
    for a, b in zip(uniform[launcher], shuffled[launcher]):
        d = _differ(a, b)
        assert d.size == 0, (launcher, d.size, truth["c_n"][d[:5]], truth["c_z"][d[:5]], a[d[:5]], b[d[:5]])


@pytest.mark.parametrize("pair", ("cke_pair", "cie_pair_from_k"))
def test_complex_jet_component_0_is_the_plain_routine(complex_runs, pair):
    """es_cjet.hpp: "component 0 of a jet evaluation is the cz evaluation" -- bit for bit, in both launches."""
    truth, uniform, shuffled = complex_runs
    for runs in (uniform, shuffled):
        for j in (0, 1):
            d = _differ(runs["dm_" + pair][j], runs["dm_" + pair + "_jet"][j])
            assert d.size == 0, (pair, j, d.size, truth["c_n"][d[:5]], truth["c_z"][d[:5]])


@pytest.mark.parametrize("func", bc.FUNCTIONS)
def test_complex_device_against_truth(complex_runs, func):
    """B: per row, the error against the correctly rounded values stays within E_HOST_C[func][order] + device_margin_c(row)
    on |z| <= 700 and within E_HOST_C_FAR[func][order] + device_margin_c(row) beyond."""
    truth, uniform, _ = complex_runs
    n, z, far = truth["c_n"], truth["c_z"], truth["c_far"]
    got = uniform["dm_" + func[:-2] + "_jet"][2:] if func.endswith("_d") else uniform["dm_" + func]
    err = bc.errors(truth, func, got)
    for is_far, table in ((False, bc.E_HOST_C), (True, bc.E_HOST_C_FAR)):
        worst = bc.worst_per_order(truth, err, is_far)
        print(f"{func}, {'|z| > 700' if is_far else '|z| <= 700'}: device " + " ".join(f"{e:6.2f}" for e, _ in worst.values())
              + "\n" + " " * 34 + "E_host " + " ".join(f"{table[func][o]:6.2f}" for o in worst))
        print("    worst at", {o: za for o, (_, za) in worst.items()})
    bound = np.array([(bc.E_HOST_C_FAR if f else bc.E_HOST_C)[func][int(o)] for o, f in zip(n, far)]) + bc.device_margin_c(func, z)
    over = np.where(~(err <= bound))[0]
    assert over.size == 0, (func, over.size, n[over[:5]], z[over[:5]], err[over[:5]], bound[over[:5]])


@pytest.mark.parametrize("name", bc.PRIMITIVES)
def test_complex_primitives(probe, name):
    """C: cz_sqrt, cz_log, cz_exp, cz / cz and double / cz on the device within the bounds of the host leg, the sign of the
    imaginary part on the cut of sqrt and log exact."""
    import torch
    lib, stream = probe
    truth = bc.load()
    want = truth[name + "_w"]
    with torch.cuda.stream(stream):
        if name in ("div", "rdiv"):
            da = torch.as_tensor(np.ascontiguousarray(truth[name + "_a"]), device="cuda")
            db = torch.as_tensor(np.ascontiguousarray(truth[name + "_b"]), device="cuda")
            assert da.dtype == (torch.complex128 if name == "div" else torch.float64) and da.numel() == len(want)
        else:
            da, db = None, torch.as_tensor(np.ascontiguousarray(truth[name + "_z"]), device="cuda")
        assert db.dtype == torch.complex128 and db.numel() == len(want)
        do = torch.full((len(want),), complex("nan+nanj"), dtype=torch.complex128, device="cuda")
        rc = lib.dm_cz_primitive(bc.PRIMITIVES.index(name), C.c_void_p(da.data_ptr()) if da is not None else None,
                                 C.c_void_p(db.data_ptr()), len(want), C.c_void_p(do.data_ptr()), C.c_void_p(stream.cuda_stream))
        assert rc == 0, rc
        stream.synchronize()
        got = do.cpu().numpy()
    bc.primitive_checks(truth, name, got)


# ---- the real jets: es_jet.hpp, es_jet2.hpp ---------------------------------------------------------------------------------------
BESSEL_JET_LAUNCHERS = tuple(jt.BESSEL_JETS)


def _evaluate_bessel_jets(probe, launcher, n, x):
    """launcher (dm_ke_pair_jets, dm_ie_pair_from_k_jets) at the rows (n[i], x[i]) -> [rows, 10]; n: an int or an int array"""
    import torch
    lib, stream = probe
    with torch.cuda.stream(stream):
        dx = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda")
        dn = None if np.isscalar(n) else torch.as_tensor(np.ascontiguousarray(n, dtype=np.int32), device="cuda")
        assert dn is None or dn.numel() == dx.numel()
        do = torch.full((dx.numel(), 10), float("nan"), dtype=torch.float64, device="cuda")
        rc = getattr(lib, launcher)(C.c_void_p(dn.data_ptr()) if dn is not None else None, int(n) if dn is None else 0,
                                    C.c_void_p(dx.data_ptr()), int(dx.numel()), C.c_void_p(do.data_ptr()),
                                    C.c_void_p(stream.cuda_stream))
        assert rc == 0, rc
        stream.synchronize()
        return do.cpu().numpy()


@pytest.fixture(scope="module")
def bessel_jet_runs(probe):
    """(n, x, uniform, shuffled, plain): per launcher the [rows, 10] device results on every ik row of the fixture, once with
    one order per launch and once with all rows shuffled into one launch; plain: the two outputs of the plain routine"""
    truth = bt.load()
    n, x = truth["ik_n"], truth["ik_x"]
    assert len(x) > 1200
    perm = np.random.default_rng(20240607).permutation(len(x))
    assert len(set(n[perm[:64]])) > 4                          # the first wave alone holds more than four orders
    uniform, shuffled, plain = {}, {}, {}
    for launcher in BESSEL_JET_LAUNCHERS:
        uniform[launcher] = np.full((len(x), 10), np.nan)
        for order in bt.ORDERS:
            sel = np.where(n == order)[0]
            uniform[launcher][sel] = _evaluate_bessel_jets(probe, launcher, int(order), x[sel])
        shuffled[launcher] = np.full((len(x), 10), np.nan)
        shuffled[launcher][perm] = _evaluate_bessel_jets(probe, launcher, n[perm], x[perm])
        plain[launcher] = _evaluate(probe, jt.BESSEL_JETS[launcher][0], n, x)
    return n, x, uniform, shuffled, plain


def _bits_differ(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return np.where((a.view(np.int64) != b.view(np.int64)).reshape(len(a), -1).any(axis=1))[0]


@pytest.mark.parametrize("launcher", BESSEL_JET_LAUNCHERS)
def test_bessel_jets_uniform_against_shuffled(bessel_jet_runs, launcher):
    """1: every row gives the same bits, all ten outputs, with a wave-uniform order and in a launch whose waves mix orders."""
    n, x, uniform, shuffled, _ = bessel_jet_runs
    d = _bits_differ(uniform[launcher], shuffled[launcher])
    assert d.size == 0, (launcher, d.size, n[d[:5]], x[d[:5]], uniform[launcher][d[:5]], shuffled[launcher][d[:5]])


@pytest.mark.parametrize("launcher", BESSEL_JET_LAUNCHERS)
def test_bessel_jets_value_is_the_plain_routine(bessel_jet_runs, launcher):
    """2: the value component of Jet<1> and of Jet2<1> is esb::ke_pair / esb::ie_pair_from_k bit for bit, and the j part of
    Jet2<1> is the Jet<1> result bit for bit -- es_jet2.hpp: "BY CALLING the Jet<NV> one"."""
    n, x, uniform, shuffled, plain = bessel_jet_runs
    for runs in (uniform, shuffled):
        got = runs[launcher]
        for member, (c1, c2) in enumerate(((0, 4), (2, 7))):
            for col in (c1, c2):
                d = _bits_differ(got[:, col], plain[launcher][member])
                assert d.size == 0, (launcher, member, col, d.size, n[d[:5]], x[d[:5]])
        d = _bits_differ(got[:, (4, 5, 7, 8)], got[:, (0, 1, 2, 3)])
        assert d.size == 0, (launcher, d.size, n[d[:5]], x[d[:5]])


def _worst(n, x, err, sel):
    out = {}
    for order in bt.ORDERS:
        rows = np.where((n == order) & sel)[0]
        assert rows.size > 10, (order, rows.size)
        i = rows[np.argmax(err[rows])]
        out[order] = (float(err[i]), float(x[i]), int(i))
    return out


@pytest.mark.parametrize("nu", (1, 2))
@pytest.mark.parametrize("launcher", BESSEL_JET_LAUNCHERS)
def test_bessel_jets_against_truth(bessel_jet_runs, launcher, nu):
    """3: d/dx (nu = 1) and d2/dx2 (nu = 2) against the identities summed at 40 digits, in u times the identity's magnitude,
    within E_HOST + device_margin + c (jet_truth.BESSEL_JET_C: the operations of the identity as written)."""
    n, x, uniform, _, _ = bessel_jet_runs
    routine = jt.BESSEL_JETS[launcher][0]
    err, _, _ = jt.bessel_errors(jt.load(), launcher, uniform[launcher], nu)
    bound = jt.bessel_bound(routine, n, nu)
    worst = _worst(n, x, err, np.ones(len(x), dtype=bool))
    print(f"{launcher} d{nu}, u x magnitude: " + " ".join(f"{e:6.2f}" for e, _, _ in worst.values()))
    for order, (e, x_at, i) in worst.items():
        print(f"    order {order}: {e:.2f} at x = {x_at!r}, bound {bound[i]:.2f}")
    over = np.where(~(err <= bound))[0]
    assert over.size == 0, (launcher, nu, over.size, n[over[:5]], x[over[:5]], err[over[:5]], bound[over[:5]])


@pytest.mark.parametrize("nu", (1, 2))
@pytest.mark.parametrize("launcher", BESSEL_JET_LAUNCHERS)
def test_bessel_jets_relative_to_the_derivative(bessel_jet_runs, launcher, nu):
    """4: the same error relative to the true derivative itself, the figure a user of D_w and D_ww feels.  It is printed per
    order on x <= 60 and beyond and bounded by no number chosen in advance: only by 4 x what the identity's magnitude
    predicts for the row, (E_HOST + margin + c) u magnitude / |true|."""
    n, x, uniform, _, _ = bessel_jet_runs
    routine = jt.BESSEL_JETS[launcher][0]
    _, rel, cond = jt.bessel_errors(jt.load(), launcher, uniform[launcher], nu)
    predicted = jt.bessel_bound(routine, n, nu) * cond
    for label, sel in (("x <= 60", x <= 60.0), ("x > 60 ", x > 60.0)):
        worst = _worst(n, x, rel, sel)
        print(f"{launcher} d{nu}, u x |true|, {label}: " + " ".join(f"{e:9.3g}" for e, _, _ in worst.values()))
        print("    at x = " + " ".join(f"{x_at:9.3g}" for _, x_at, _ in worst.values()))
        print("    magnitude / |true| there: " + " ".join(f"{cond[i]:9.3g}" for _, _, i in worst.values()))
    over = np.where(~(rel <= 4.0 * predicted))[0]
    assert over.size == 0, (launcher, nu, over.size, n[over[:5]], x[over[:5]], rel[over[:5]], predicted[over[:5]])


def _run_jet_op(probe, code, nv, ops):
    """dm_jet_op on the operand dict ops (jet_truth.op_operands) -> (Jet2 rows [rows, 6], Jet rows [rows, 3], doubles [rows]);
    the outputs are NaN where the launch does not write"""
    import torch
    lib, stream = probe
    rows = len(ops["a"])
    with torch.cuda.stream(stream):
        dev = {k: torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32 if k == "e" else np.float64), device="cuda")
               for k, v in ops.items()}
        assert all(dev[k].shape == (rows, 6) for k in "xyz") and all(dev[k].shape == (rows,) for k in "abce")
        outs = [torch.full(shape, float("nan"), dtype=torch.float64, device="cuda") for shape in ((rows, 6), (rows, 3), (rows,))]
        rc = lib.dm_jet_op(code, nv, *[C.c_void_p(dev[k].data_ptr()) for k in ("x", "y", "z", "a", "b", "c", "e")], rows,
                           *[C.c_void_p(o.data_ptr()) for o in outs], C.c_void_p(stream.cuda_stream))
        assert rc == 0, rc
        stream.synchronize()
        return tuple(o.cpu().numpy() for o in outs)


@pytest.fixture(scope="module")
def jet_op_runs(probe):
    """(fixture, {(code, nv): (Jet2 rows, Jet rows, doubles)}) for every operator with a fixture, in Jet2<2> and Jet2<1>"""
    jets = jt.load()
    assert dict(zip(jets["op_codes"].tolist(), jets["op_names"].tolist())) == jt.OPS
    assert sum(len(jets[f"op_{name}_t"]) for name in jt.OPS.values()) >= 1900
    return jets, {(code, nv): _run_jet_op(probe, code, nv, jt.op_operands(jets, code)) for code in jt.OPS for nv in (2, 1)}


# the plain double operation where it is an IEEE operation NumPy has as well: the probe's own third output is held to it
_NUMPY_VALUE = {"neg": lambda o: -o["x"][:, 0], "add": lambda o: o["x"][:, 0] + o["y"][:, 0],
                "sub": lambda o: o["x"][:, 0] - o["y"][:, 0], "add_jd": lambda o: o["x"][:, 0] + o["a"],
                "sub_dj": lambda o: o["a"] - o["x"][:, 0], "mul_jd": lambda o: o["x"][:, 0] * o["a"],
                "mul": lambda o: o["x"][:, 0] * o["y"][:, 0], "rcp": lambda o: 1.0 / o["x"][:, 0],
                "rcp_from": lambda o: o["a"], "div": lambda o: o["x"][:, 0] / o["y"][:, 0],
                "div_dj": lambda o: o["a"] / o["x"][:, 0], "div_jd": lambda o: o["x"][:, 0] / o["a"],
                "sqrt": lambda o: np.sqrt(o["x"][:, 0]), "ldexp": lambda o: np.ldexp(o["x"][:, 0], o["e"]),
                "lift_onto": lambda o: o["y"][:, 0], "lift": lambda o: o["a"], "fabs": lambda o: np.abs(o["x"][:, 0])}


@pytest.mark.parametrize("code", sorted(jt.OPS))
def test_jet_operator_bit_for_bit_claims(jet_op_runs, code):
    """5: the first-order part of the Jet2 result is the Jet result of the same operator on the operands' first-order parts,
    bit for bit, and the value component is the plain double operation on the values (fast_rcp: fast_rcp of the value),
    in Jet2<2> and in Jet2<1>."""
    jets, runs = jet_op_runs
    name = jt.OPS[code]
    for nv in (2, 1):
        j2, j1, plain = runs[(code, nv)]
        first = [0, 1, 2][:nv + 1]
        assert np.isfinite(j2[:, first + ([3, 4, 5] if nv == 2 else [3])]).all(), (name, nv)
        if nv == 1:                                            # the components of the second variable: not written
            assert np.isnan(j2[:, (2, 4, 5)]).all() and np.isnan(j1[:, 2]).all()
        d = _bits_differ(j2[:, first], j1[:, first])
        assert d.size == 0, (name, nv, d.size, j2[d[:3]], j1[d[:3]])
        d = _bits_differ(j2[:, 0], plain)
        assert d.size == 0, (name, nv, d.size, j2[d[:3], 0], plain[d[:3]])
        if name in _NUMPY_VALUE:
            d = _bits_differ(plain, _NUMPY_VALUE[name](jt.op_operands(jets, code)))
            assert d.size == 0, (name, nv, d.size, plain[d[:3]])
    if name == "fabs":
        # pinned: the header's rule (v < 0 ? -1 : 1) gives the sign +1 to +0.0 and to -0.0 -- the value is +0.0 and every
        # derivative passes unchanged, where d|x| at 0 has no value to be right about
        x = jets["op_fabs_x"]
        assert x[-2, 0] == 0.0 and not np.signbit(x[-2, 0]) and x[-1, 0] == 0.0 and np.signbit(x[-1, 0])
        j2 = runs[(code, 2)][0]
        assert not np.signbit(j2[-2:, 0]).any() and _bits_differ(j2[-2:, 1:], x[-2:, 1:]).size == 0
        neg = x[:, 0] < 0.0
        assert neg.sum() >= 10 and _bits_differ(j2[neg], -x[neg]).size == 0


@pytest.mark.parametrize("code", sorted(jt.OPS))
def test_jet_operator_against_truth(jet_op_runs, code):
    """6: every component of every row within c_op u magnitude of the truth (Taylor-polynomial arithmetic at 40 digits),
    c_op the count of roundings of jet_truth.C_OP; no row is excluded, a NaN is an infinite error."""
    jets, runs = jet_op_runs
    name = jt.OPS[code]
    for nv in (2, 1):
        err = jt.op_errors(jets, code, runs[(code, nv)][0], nv)
        i, c = np.unravel_index(int(np.argmax(err)), err.shape)
        print(f"{name} Jet2<{nv}>: worst {err[i, c]:.2f} u x magnitude (row {i}, component {c}), c_op {jt.C_OP[name]}; "
              f"per component " + " ".join(f"{e:.2f}" for e in err.max(axis=0)))
        assert err.shape == (len(jets[f"op_{name}_t"]), 6 if nv == 2 else 3)
        assert np.all(err <= jt.C_OP[name]), (name, nv, int(i), int(c), float(err[i, c]))


@pytest.mark.parametrize("nv", (2, 1))
def test_jet_finite_val_constant_variable(probe, nv):
    """The codes with exact answers: jet_finite sees a NaN or an infinity in every component it has and in no other; val, the
    constant and the variable number `comp` (outside 0 .. NV - 1: a constant)."""
    rng = np.random.default_rng(11)
    rows = 6 * 3 + 8
    x = np.exp2(rng.uniform(-40.0, 40.0, (rows, 6))) * rng.choice([-1.0, 1.0], (rows, 6))
    for p in range(6):
        x[3 * p, p], x[3 * p + 1, p], x[3 * p + 2, p] = np.inf, -np.inf, np.nan
    planted = np.repeat(np.arange(6), 3)
    ops = dict(x=x, y=np.ones((rows, 6)), z=np.ones((rows, 6)), a=x[::-1, 3].copy(), b=np.ones(rows), c=np.ones(rows),
               e=(np.arange(rows) % 4 - 1).astype(np.int32))
    has2, has1 = ((0, 1, 2, 3, 4, 5), (0, 1, 2)) if nv == 2 else ((0, 1, 3), (0, 1))
    j2, j1, plain = _run_jet_op(probe, jt.OP_JET_FINITE, nv, ops)
    want2 = np.array([0.0 if p in has2 else 1.0 for p in planted] + [1.0] * 8)
    want1 = np.array([0.0 if p in has1 else 1.0 for p in planted] + [1.0] * 8)
    want0 = np.array([0.0 if p == 0 else 1.0 for p in planted] + [1.0] * 8)
    assert np.array_equal(j2[:, 0], want2) and np.array_equal(j1[:, 0], want1) and np.array_equal(plain, want0)
    fin = dict(ops, x=np.where(np.isfinite(x), x, 1.5))
    zero2, zero1 = list(has2[1:]), list(has1[1:])
    for code, value in ((jt.OP_VAL, fin["x"][:, 0]), (jt.OP_CONSTANT, fin["a"])):
        j2, j1, plain = _run_jet_op(probe, code, nv, fin)
        for got in (j2[:, 0], j1[:, 0], plain):
            assert _bits_differ(got, value).size == 0, code
        assert np.all(j2[:, zero2] == 0.0) and np.all(j1[:, zero1] == 0.0), code
    j2, j1, plain = _run_jet_op(probe, jt.OP_VARIABLE, nv, fin)
    for got in (j2[:, 0], j1[:, 0], plain):
        assert _bits_differ(got, fin["a"]).size == 0
    unit = np.array([[1.0 if fin["e"][i] == comp else 0.0 for comp in range(nv)] for i in range(rows)])
    assert np.array_equal(j2[:, 1:1 + nv], unit) and np.array_equal(j1[:, 1:1 + nv], unit)
    assert np.all(j2[:, [3, 4, 5] if nv == 2 else [3]] == 0.0)
    assert {-1, 0, 1, 2} == set(fin["e"].tolist())


def test_jet_op_argument_errors(probe):
    import torch
    lib, stream = probe
    with torch.cuda.stream(stream):
        t = torch.ones((4, 6), dtype=torch.float64, device="cuda")
        e = torch.zeros((4,), dtype=torch.int32, device="cuda")
        args = [C.c_void_p(t.data_ptr())] * 6 + [C.c_void_p(e.data_ptr()), 4] + [C.c_void_p(t.data_ptr())] * 3
        for op, nv in ((-1, 2), (jt.N_OPS, 2), (0, 0), (0, 3)):
            assert lib.dm_jet_op(op, nv, *args, C.c_void_p(stream.cuda_stream)) == 1           # hipErrorInvalidValue
        assert lib.dm_jet_op(0, 2, None, *args[1:], C.c_void_p(stream.cuda_stream)) == 1
        assert lib.dm_jet_op(0, 2, *args[:7], 0, *args[8:], C.c_void_p(stream.cuda_stream)) == 0  # nothing to do
        stream.synchronize()
