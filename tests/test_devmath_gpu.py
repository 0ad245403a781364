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
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import bessel_complex_truth as bc
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
    for name in ("dm_cke_pair", "dm_cie_pair_from_k"):
        getattr(lib, name).argtypes = [vp, i, vp, i, vp, vp, vp]
    for name in ("dm_cke_pair_jet", "dm_cie_pair_from_k_jet"):
        getattr(lib, name).argtypes = [vp, i, vp, i, vp, vp, vp, vp, vp]
    lib.dm_cz_primitive.argtypes = [i, vp, vp, i, vp, vp]
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
