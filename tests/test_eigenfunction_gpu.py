"""es_shoot_eigenfunction (include/eigensolver_amd.h section 5) on all four families.

Yardsticks (tests/real_eigen_model.py, pinned on the CPU by tests/test_real_eigen_model.py):
  truth     DOP853 at rtol 1e-12 -- oracle.cylinder.eigenfunction_outward (from the axis point outwards, the stable
            direction) and oracle.slab.eigenfunction -- and the closed-form exterior with scipy's ive / kve, its decaying
            and its growing term kept apart;
  restate   NumPy RK4 on the node grid from the kernel's own state at the node where its writing march starts.
Pairs are fixed (k, omega) drawn with a seed inside each case's window, not roots: the two-region solution is defined at
every ES_PT_OK pair.  Roots are used for the continuity checks only.

Bounds, none of them measured on the kernel:
  a  2e-6 max(1, (1000/N)^4) of max|field| per array: RK4 on the reference grid against DOP853, the project's figure from
     the first version of this file.  CR_kink (singular solution kept by its axis condition) keeps its 1e-3 on the whole
     interval and 2e-5 on |r| >= 0.02.  The NumPy model of the kernel's algorithm meets all of them (E_trunc below).
  b  1e-10 of max|field| at every node: a GPU kernel against a NumPy restatement of the same algorithm
     (tests/test_complex_gpu.py); the model's own fp64 rounding E_round is <= 1e-11 for every pair used.
  c  1e-12 (|decaying term| + |growing term|) at every exterior point: three Bessel factors per term at <= 28 u each
     (tests/test_devmath_gpu.py, n <= 40), two exponentials with arguments up to 80, ~20 roundings: ~300 u = 7e-14.
  d  large gaps mu (R - 1) >= 40: as a and c; where mu (R - |x|) < 20 the kernel has dropped the growing term on purpose
     (below e^-40 of the boundary value): 1e-15 absolute there.  D against truth.mismatch at tests/test_shoot_gpu.py's bound.
  e  jump of the flux arrays at the boundary against es_shoot_eval_points' D: 1e-10 of max(|outer|, |inner|), for cylinders
     plus 4 x the difference of the inward and the outward NumPy march at the boundary (real_eigen_model.
     boundary_flux_spread; below 1e-11 for every pair used, so the bound is 1e-10 in effect).

CPU figures of the model, worst pair per family (python -m pytest tests/test_real_eigen_model.py -s):
  family      E_trunc (bound)        E_round
  FAM_CYL0    2.95e-6 (3.2e-5, CDC_w095_kink, N = 500); 8.2e-7 (2e-6, CF_flow_m3)     1.2e-14
  FAM_CYLT    9.6e-5 (1e-3, CR_kink); 3.8e-12 (2e-6, CR_sausage)                      2.4e-14
  FAM_SLABD   2.0e-11 (2e-6)                                                          1.5e-14
  FAM_SLABF   7.2e-9 (3.2e-5)                                                         1.9e-14
  the former inward march, pair 0: m = 1 6.9e-8, m = 3 6.5e-2, m = 5 2.6e+5 (E_round 6e-11, 3e-4, 4e-4).
GPU figures: every check prints its measured value, its bound and their ratio with `pytest -s` (lines starting "a ", "b ",
"c ", "d ", "e ", "f "); none has been recorded here yet -- the kernel change and these tests were written against the CPU
model above and have not been run on a GPU.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import cases  # noqa: E402
from tests import real_eigen_model as M  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

KEYS = ("value_int", "flux_int", "value_ext", "flux_ext")
FAMILY = {0: "FAM_CYL0", 1: "FAM_CYLT", 2: "FAM_SLABD", 3: "FAM_SLABF"}


class _Pool:
    """ShootProblems and their eigenfunctions at the fixed pairs, one per case and module run."""

    def __init__(self, ctx):
        self.ctx, self.gp, self.ef = ctx, {}, {}

    def problem(self, name):
        if name not in self.gp:
            from eigensolver_amd import ShootProblem
            eq, mode, m, _ = M.all_cases()[name]
            self.gp[name] = ShootProblem(eq, mode, m, ctx=self.ctx)
        return self.gp[name]

    def pairs(self, name, large_gap=False):
        return (M.large_gap_pairs if large_gap else M.pairs)(name)

    def eigen(self, name, large_gap=False):
        """dict of numpy arrays at the case's pairs (n_ext = 500) plus D and status of eval_points there."""
        key = (name, large_gap)
        if key not in self.ef:
            gp = self.problem(name)
            k, w = self.pairs(name, large_gap)
            e = {a: b.cpu().numpy() for a, b in gp.eigenfunction(k, w, n_ext=500).items()}
            D, st = gp.eval_points(k, w)
            e["D"], e["status"] = D.cpu().numpy(), st.cpu().numpy()
            self.ef[key] = e
        return self.ef[key]

    def close(self):
        for gp in self.gp.values():
            gp.close()


@pytest.fixture(scope="module")
def pool(es_ctx):
    p = _Pool(es_ctx)
    yield p
    p.close()


def _family(pool, name):
    return FAMILY[int(pool.problem(name).desc.geometry)]


def _ok_rows(e, name):
    ok = [i for i in range(len(e["status"])) if e["status"][i] == 0]
    assert len(ok) >= 3, (name, e["status"])            # the pairs are OK for the oracle; a continuum flag may differ at an edge
    return ok


# ---- a. every family against truth ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.STANDARD)
def test_every_family_against_truth(pool, name):
    eq = M.all_cases()[name][0]
    e = pool.eigen(name)
    k, w = pool.pairs(name)
    sgn = -1.0 if eq.x_boundary < 0 else 1.0
    worst = 0.0
    for i in _ok_rows(e, name):
        t = M.truth(name, i)
        assert np.allclose(e["x_int"], t["x_int"], rtol=0, atol=1e-15)
        assert np.allclose(e["x_ext"][i], t["x_ext"], rtol=1e-15, atol=1e-15)
        R = eq.L_factor * 2.0 * np.pi / k[i]
        assert e["x_ext"][i, -1] == sgn * 1.0 and abs(e["x_ext"][i, 0] - sgn * R) <= 1e-15 * R      # also for r_sign = +1
        for key in KEYS:
            if key.endswith("_int"):
                checks = M.interior_error(name, key, e[key][i], t[key], t["x_int"])      # whole interval, axis node included
            else:
                checks = [(float(np.max(np.abs(e[key][i] - t[key])) / np.max(np.abs(t[key]))), M.bound(eq.n_nodes))]
            for got, b in checks:
                print(f"a {_family(pool, name)} {name} pair {i} {key}: {got:.2e} of max|field| (bound {b:.1e}, ratio {got / b:.2e})")
                worst = max(worst, got / b)
                assert got <= b, (name, i, key, got, b)
    print(f"a {_family(pool, name)} {name}: worst ratio {worst:.2e}")


# ---- b. the writing march against its restatement --------------------------------------------------------------------
@pytest.mark.parametrize("name", M.STANDARD)
def test_writing_march_against_restatement(pool, name):
    e = pool.eigen(name)
    k, w = pool.pairs(name)
    worst = 0.0
    for i in _ok_rows(e, name)[:2]:
        value, flux = M.restate(name, float(k[i]), float(w[i]), e["value_int"][i], e["flux_int"][i])
        for key, ref in (("value_int", value), ("flux_int", flux)):
            got = float(np.max(np.abs(e[key][i] - ref)) / np.max(np.abs(ref)))
            print(f"b {_family(pool, name)} {name} pair {i} {key}: {got:.2e} of max|field| (bound 1.0e-10, ratio {got / 1e-10:.2e})")
            worst = max(worst, got / 1e-10)
            assert got <= 1e-10, (name, i, key, got)
    print(f"b {_family(pool, name)} {name}: worst ratio {worst:.2e}")


# ---- c. pointwise exterior -------------------------------------------------------------------------------------------------
def _pointwise(e, t, i, lo=None):
    """worst |gpu - truth| / (|term 1| + |term 2|) over the exterior points (those with index >= lo)."""
    worst = 0.0
    for key in ("value_ext", "flux_ext"):
        size = np.abs(t[key + "_terms"][0]) + np.abs(t[key + "_terms"][1])
        r = np.abs(e[key][i] - t[key]) / size
        worst = max(worst, float(np.max(r[lo:])))
    return worst


@pytest.mark.parametrize("name", M.STANDARD)
def test_exterior_pointwise(pool, name):
    e = pool.eigen(name)
    n = 0
    for i in _ok_rows(e, name):
        t = M.truth(name, i)
        if t["gap"] >= 40.0:
            continue
        got = _pointwise(e, t, i)
        print(f"c {_family(pool, name)} {name} pair {i} gap {t['gap']:.1f}: {got:.2e} of the two terms (bound 1.0e-12, ratio {got / 1e-12:.2e})")
        assert got <= 1e-12, (name, i, got)
        n += 1
    assert n >= 3


# ---- d. large-gap branch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.LARGE_GAP)
def test_large_gap_branch(pool, name):
    eq = M.all_cases()[name][0]
    e = pool.eigen(name, large_gap=True)
    k, w = pool.pairs(name, large_gap=True)
    prob = M.problem(name)
    gaps = [M.truth(name, i, True)["gap"] for i in range(len(k))]
    assert min(gaps) < 40.0 <= max(gaps), gaps                       # both branches of the exterior in one call
    assert np.all(e["status"] == 0), e["status"]
    for i in range(len(k)):
        t = M.truth(name, i, True)
        d, outer, inner, st = prob.mismatch(float(k[i]), float(w[i]))
        assert st == 0
        tol = 3e-8 * max(1.0, (1000.0 / eq.n_nodes) ** 4)           # tests/test_shoot_gpu.py, test_grid_vs_truth_oracle
        got = abs(e["D"][i] - d) / max(abs(outer), abs(inner))
        print(f"d {name} gap {gaps[i]:.1f} D: {got:.2e} (bound {tol:.1e})")
        assert got <= tol, (name, i, e["D"][i], d)
        for key in KEYS:
            checks = M.interior_error(name, key, e[key][i], t[key], t["x_int"]) if key.endswith("_int") else \
                [(float(np.max(np.abs(e[key][i] - t[key])) / np.max(np.abs(t[key]))), M.bound(eq.n_nodes))]
            for g, b in checks:
                print(f"d {name} gap {gaps[i]:.1f} {key}: {g:.2e} of max|field| (bound {b:.1e})")
                assert g <= b, (name, i, key, g, b)
        mu = t["gap"] / (eq.L_factor * 2.0 * np.pi / k[i] - 1.0)
        R = eq.L_factor * 2.0 * np.pi / k[i]
        near = mu * (R - np.abs(t["x_ext"])) >= 20.0                 # x_ext runs from the far field in: a suffix of the row
        lo = int(np.argmax(near))
        assert near[lo:].all() and not near[:lo].any()
        if gaps[i] < 40.0:
            lo = 0                                                   # both terms kept: every point, as in c
        got = _pointwise(e, t, i, lo)
        print(f"d {name} gap {gaps[i]:.1f} pointwise from point {lo} (mu (R - |x|) >= 20 where the gap is >= 40): {got:.2e} (bound 1.0e-12)")
        assert got <= 1e-12, (name, i, got)
        if gaps[i] >= 40.0:
            for key in ("value_ext", "flux_ext"):
                far = float(np.max(np.abs(e[key][i, :lo] - t[key][:lo]))) if lo else 0.0
                print(f"d {name} gap {gaps[i]:.1f} {key} near the far end: {far:.2e} absolute (bound 1.0e-15)")
                assert far <= 1e-15, (name, i, key, far)


# ---- e. identity with the determinant ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.STANDARD + ("CF_flow_kink_target",))
def test_identity_with_determinant(pool, name):
    """flux_ext at the boundary - flux_int at the boundary is the mismatch es_shoot_eval_points returns, and the values meet:
    |value_ext| = 1 there, value_int equal to it (flow slabs: times Omega(-1) / Omega_e)."""
    from eigensolver_amd import equilibrium as q
    eq = M.all_cases()[name][0]
    e = pool.eigen(name)
    k, w = pool.pairs(name)
    for i in _ok_rows(e, name)[:2]:
        outer, inner = e["flux_ext"][i, -1], e["flux_int"][i, 0]
        scale = max(abs(outer), abs(inner))
        b = 1e-10
        if M.is_cyl(eq):
            b += 4.0 * M.boundary_flux_spread(name, float(k[i]), float(w[i])) / scale
        got = abs((outer - inner) - e["D"][i]) / scale
        print(f"e {_family(pool, name)} {name} pair {i}: {got:.2e} of max(|outer|, |inner|) (bound {b:.2e}, ratio {got / b:.2e})")
        assert got <= b, (name, i, outer - inner, e["D"][i])
        vb = e["value_ext"][i, -1]
        assert abs(abs(vb) - 1.0) <= 1e-12
        ratio = 1.0
        if isinstance(eq, q.SlabFlow):
            ratio = (w[i] - k[i] * float(eq.profiles()["U"][0])) / (w[i] - k[i] * eq.U_e)
        assert abs(e["value_int"][i, 0] - ratio * vb) <= 1e-12 * max(1.0, abs(ratio)), (name, i, e["value_int"][i, 0], ratio * vb)


@pytest.mark.parametrize("name", ["CF_flow_kink", "CR_kink", "SD_w15_kink", "SFG_flow_kink"])
def test_flux_is_continuous_at_refined_roots(pool, name):
    """At a root the two flux arrays meet at the boundary to the root's own residual (resid is |D| in percent of
    max(|outer|, |inner|)); cylinders: plus the 4 x spread of e, their boundary flux no longer comes from the determinant's
    march."""
    eq, _, _, (lo, hi) = M.all_cases()[name]
    gp = pool.problem(name)
    kg = np.linspace(0.8, 3.6, 5)
    W = lo + (np.arange(128) + 0.5) * (hi - lo) / 128
    D, st = gp.eval_grid(kg, W)
    roots, cnt = gp.find_roots(kg, W, D, st, n_bisect=40, tol_percent=1e-4)
    acc = (roots["flag"] == 1).cpu().numpy()
    kk, ww, rs = (roots[a].cpu().numpy()[acc][:2] for a in ("k", "w", "resid"))
    assert len(kk) == 2
    ef = gp.eigenfunction(kk, ww, n_ext=2)
    for i in range(2):
        fi, fe = ef["flux_int"][i, 0].item(), ef["flux_ext"][i, -1].item()
        scale = max(abs(fi), abs(fe))
        b = rs[i] / 100.0 + 1e-10
        if M.is_cyl(eq):
            b += 4.0 * M.boundary_flux_spread(name, float(kk[i]), float(ww[i])) / scale
        print(f"e {_family(pool, name)} {name} root {i}: jump {abs(fi - fe) / scale:.2e} (resid/100 {rs[i] / 100:.2e}, bound {b:.2e})")
        assert abs(fi - fe) <= b * scale, (name, i, fi, fe, rs[i])


# ---- the checks this file has made from the start (roots of four cylinder cases, the reference's own end state) -------------
@pytest.mark.parametrize("name", ["CF_flow_kink", "CF_flow_sausage", "CDC_w095_kink", "CR_kink"])
def test_eigenfunction_vs_oracle(pool, name):
    from oracle import cylinder as oc
    eq, mode, m, (lo, hi) = M.all_cases()[name]
    gp = pool.problem(name)
    truth = M.problem(name)
    # refine a few roots first
    k = np.linspace(0.8, 3.6, 5)
    W = lo + (np.arange(128) + 0.5) * (hi - lo) / 128
    D, st = gp.eval_grid(k, W)
    roots, cnt = gp.find_roots(k, W, D, st, n_bisect=40, tol_percent=1e-4)
    acc = (roots["flag"] == 1).cpu().numpy()
    kk, ww = roots["k"].cpu().numpy()[acc][:4], roots["w"].cpu().numpy()[acc][:4]
    assert len(kk) >= 2
    ef = gp.eigenfunction(kk, ww, n_ext=500)
    for i in range(len(kk)):
        o = oc.eigenfunction_outward(truth, kk[i], ww[i], eq.n_nodes, n_ext=500)
        assert np.allclose(ef["x_int"].cpu().numpy(), o["r_int"], rtol=0, atol=1e-15)
        for key_g, key_o in (("value_int", "P_int"), ("flux_int", "xi_int"), ("value_ext", "P_ext"), ("flux_ext", "xi_ext")):
            a, b = ef[key_g][i].cpu().numpy(), o[key_o]
            # RK4 on the reference grid vs DOP853
            tol = 2e-6 * max(1.0, (1000.0 / eq.n_nodes) ** 4)
            if name.startswith("CR") and key_g.endswith("_int"):
                # the rotational axis condition P(r_ax) = -c xi_e keeps the singular solution (xi ~ 1/r^2): on the
                # reference's uniform grid h/r ~ 0.5 at the last nodes, where RK4 is only good to ~1e-3 of the (huge)
                # axis value; away from the axis the usual bound holds
                far = np.abs(o["r_int"]) >= 0.02
                assert np.max(np.abs(a - b)[far]) <= 2e-5 * np.max(np.abs(b[far])), (name, key_g)
                tol = 1e-3
            assert np.max(np.abs(a - b)) <= tol * np.max(np.abs(b)), (name, key_g, np.max(np.abs(a - b)), np.max(np.abs(b)))
        assert np.allclose(ef["x_ext"][i].cpu().numpy(), o["r_ext"], rtol=1e-15, atol=1e-15)
        # at a root the displacement is continuous across the boundary: xi_i(r_b) = xi_e(r_b)
        fi, fe = ef["flux_int"][i, 0].item(), ef["flux_ext"][i, -1].item()
        assert abs(fi - fe) <= 1e-5 * max(abs(fi), abs(fe))
        assert abs(abs(ef["value_ext"][i, -1].item()) - 1.0) < 1e-12
        assert abs(ef["value_int"][i, 0].item() - ef["value_ext"][i, -1].item()) < 1e-12


def test_interior_end_state_vs_reference_trace(es_ctx):
    """The reference's last interior odeint of every evaluation (CF:802) ends at r_ax with (P, P'); with its own
    boundary state as input, P'(r_ax)/P_b of the reference must equal ours (kink: P(r_ax) = 0, P' = Xi/F)."""
    import eigensolver_amd as E
    tr = json.load(open(os.path.join(G, "trace_CF_flow.json")))
    eq = E.equilibrium.CylinderFlow(U_i0=0.6, width=1.0)
    gp = E.ShootProblem(eq, "kink", ctx=es_ctx)
    truth = cases.truth_problem(eq, "kink")
    n = 0
    for call in tr["calls"]:
        if call["fn"] != "kink":
            continue
        for ev in call["evals"][:6]:
            if ev["ier"] != 1 or ev["int_end"] is None:
                continue
            k, w = call["k"], ev["omega"]
            ef = gp.eigenfunction([k], [w], n_ext=2)
            ra = eq.x_end
            Dc, C1, C2, C3, _, _ = truth.coefficients(np.array([ra]), k, w)
            dP_mine = (C3[0] / (ra * Dc[0])) * (ef["flux_int"][0, -1].item() * ra)      # P' = C3/(r D) Xi at r_ax
            A = ev["int_y0"][0]
            # ours is normalised by |P_e(r_b)| with the closed-form exterior; the reference's own boundary slope differs
            # by its LSODA exterior error, so compare the interior map: P'(r_ax) per unit boundary flux
            ref_ratio = ev["int_end"][1] / A
            mine_ratio = dP_mine / ef["value_int"][0, 0].item()
            assert abs(mine_ratio - ref_ratio) <= 2e-2 * abs(ref_ratio), (k, w, mine_ratio, ref_ratio)
            assert abs(ef["value_int"][0, -1].item()) < 1e-8 * max(1.0, abs(mine_ratio))     # kink: P(r_ax) = 0
            n += 1
    assert n >= 6
    gp.close()


# ---- f. launch shapes --------------------------------------------------------------------------------------------------------
SENTINEL = -7.25e77


def _raw(pool, name, k, w, n, n_ext, n_alloc=None):
    """es_shoot_eigenfunction through the raw ABI on n pairs, into buffers of n_alloc >= n rows pre-filled with SENTINEL.
    Returns the five arrays whole (interior value, flux, exterior x, value, flux), pad rows included."""
    import torch
    from eigensolver_amd import _lib
    gp = pool.problem(name)
    N = int(gp.desc.n_nodes)
    n_alloc = n + 1 if n_alloc is None else n_alloc
    dk, dw = gp._dev(k[:max(n, 1)]), gp._dev(w[:max(n, 1)])
    bufs = [torch.full((n_alloc, c), SENTINEL, dtype=torch.float64, device=dk.device) for c in (N, N, max(n_ext, 1), max(n_ext, 1), max(n_ext, 1))]
    ext = [_lib.ptr(b) if n_ext else None for b in bufs[2:]]
    rc = pool.ctx.lib.es_shoot_eigenfunction(pool.ctx.handle, gp.handle, _lib.ptr(dk), _lib.ptr(dw), n, _lib.ptr(bufs[0]),
                                             _lib.ptr(bufs[1]), n_ext, *ext)
    _lib.check(pool.ctx.handle, rc)
    pool.ctx.synchronize()
    return [b.cpu().numpy() for b in bufs]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("name", ["CF_flow_kink_N130", "SFG_flow_kink_N130"])
def test_launch_shapes(pool, name):
    """n in {1, 64, 65, 130} pairs (one lane; a full workgroup; one lane into the second; a partial third) with a different k
    in every lane and n_ext in {0, 2, 3, 500}: every row bitwise equal to the same pair evaluated alone, nothing written past
    row n, nothing at all for n = 0."""
    _, _, _, (lo, hi) = M.all_cases()[name]
    k = np.linspace(0.8, 3.6, 130)
    w = k * (lo + (0.2 + 0.6 * ((np.arange(130) * 37) % 130) / 130.0) * (hi - lo))
    for n_ext in (0, 2, 3, 500):
        alone = [_raw(pool, name, k[i:i + 1], w[i:i + 1], 1, n_ext) for i in (0, 1, 63, 64, 65, 128, 129)]
        rows = {i: a for i, a in zip((0, 1, 63, 64, 65, 128, 129), alone)}
        assert all(np.isfinite(a[j][0]).all() for a in alone for j in range(5 if n_ext else 2))
        for n in (1, 64, 65, 130):
            out = _raw(pool, name, k, w, n, n_ext)
            for j, a in enumerate(out):
                if n_ext == 0 and j >= 2:
                    assert np.all(a == SENTINEL)
                    continue
                assert np.all(a[n:] == SENTINEL), (name, n, n_ext, j)            # the pad row
                assert not np.any(a[:n] == SENTINEL), (name, n, n_ext, j)
                for i, al in rows.items():
                    if i < n:
                        assert np.array_equal(_bits(a[i]), _bits(al[j][0])), (name, n, n_ext, j, i)
                # a row-shifted result (what a wrong pair / lane index would give) is NOT equal
                if n >= 2:
                    assert not np.array_equal(_bits(a[1]), _bits(rows[0][j][0])), (name, n, n_ext, j)
        out = _raw(pool, name, k, w, 0, n_ext, n_alloc=2)
        for a in out:
            assert np.all(a == SENTINEL), (name, n_ext)


@pytest.mark.parametrize("name", ["CF_flow_kink_N2", "CF_flow_kink_N3", "SFG_flow_kink_N2", "SFG_flow_kink_N3"])
def test_one_and_two_steps(pool, name):
    """N = 2 (one RK4 step) and N = 3 run and equal the NumPy model of the algorithm (1e-10 of max|field|, as b)."""
    k, w = M.pairs(name)
    e = pool.eigen(name)
    assert np.isin(e["status"], (0, 3)).all()              # bound exterior; a continuum flag does not stop the march
    for i in range(len(k)):
        value, flux = M.model(name, float(k[i]), float(w[i]))
        for key, ref in (("value_int", value), ("flux_int", flux)):
            got = float(np.max(np.abs(e[key][i] - ref)) / np.max(np.abs(ref)))
            print(f"f {name} pair {i} {key}: {got:.2e} of max|field| (bound 1.0e-10)")
            assert got <= 1e-10, (name, i, key, got, e[key][i], ref)


# ---- g. pairs that are not ES_PT_OK -----------------------------------------------------------------------------------------
def _leaky_w(name, k):
    prob = M.problem(name)
    for W in np.linspace(0.05, 8.0, 400):
        if M.exterior_m_e(prob, k, k * W) < 0.0:
            return k * W
    raise AssertionError(name)


@pytest.mark.parametrize("name", ["CF_flow_kink", "CR_kink", "SD_w15_kink", "SFG_flow_kink"])
def test_pairs_that_are_not_ok_return_nan(pool, name):
    """A leaky pair (m_e < 0) and a non-finite one (omega = 0 for the slabs: p_e = 1 / 0; omega = NaN for the cylinders)
    among good ones: all four value / flux rows of such a pair are NaN, its x_ext row is finite, and the neighbours are
    bitwise what a call without it returns (include/eigensolver_amd.h section 5)."""
    eq = M.all_cases()[name][0]
    gp = pool.problem(name)
    k, w = M.pairs(name)
    bad_w = [_leaky_w(name, 1.3), float("nan") if M.is_cyl(eq) else 0.0]
    kk = np.array([k[0], 1.3, k[1], 1.7, k[2]])
    ww = np.array([w[0], bad_w[0], w[1], bad_w[1], w[2]])
    _, st = gp.eval_points(kk, ww)
    assert st.cpu().numpy().tolist() == [0, 1, 0, 2, 0]
    e = {a: b.cpu().numpy() for a, b in gp.eigenfunction(kk, ww, n_ext=7).items()}
    good = {a: b.cpu().numpy() for a, b in gp.eigenfunction(kk[[0, 2, 4]], ww[[0, 2, 4]], n_ext=7).items()}
    for key in KEYS:
        assert np.isnan(e[key][[1, 3]]).all(), (name, key)
        assert np.array_equal(_bits(e[key][[0, 2, 4]]), _bits(good[key])), (name, key)
        assert np.isfinite(good[key]).all()
    assert np.isfinite(e["x_ext"]).all()
    assert np.array_equal(e["x_ext"][[0, 2, 4]], good["x_ext"])
