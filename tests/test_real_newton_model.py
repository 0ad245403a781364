"""CPU pins of the yardsticks of tests/real_newton_model.py (the GPU tests of es_shoot_newton, ShootProblem.densify and
trace_branches compare with them): Newton with exact slopes from the Hermite prediction through a coarse scan reaches every
fine point of every traced branch, on its own branch, at the C port's root; and which lanes of the offset-guess runs have a
step count that does not hinge on the last bits.  `pytest -s` prints every measured figure."""
import numpy as np
import pytest

from tests import mode_signature_model as S
from tests import real_newton_model as N

ROOT_BOUND = 1e-10                                           # the project's asserted root bound, DESIGN.md section 2


@pytest.mark.parametrize("name,which", N.trace_list())
def test_tracing_reaches_every_fine_point_on_its_branch(name, which):
    T = N.traced(name, which)
    n = len(T["k"])
    assert n == N.CUT * (len(T["coarse"][1]) - 1) + 1 and n >= 5
    assert T["flag"].tolist() == [1] * n and T["status"].tolist() == [0] * n            # every fine point converges
    roots = [N.port_root_near(name, float(k), float(w)) for k, w in zip(T["k"], T["w"])]
    assert all(r is not None for r in roots), (name, which, [i for i, r in enumerate(roots) if r is None])   # none left out
    err = np.abs(T["w"] - np.array(roots)) / np.maximum(1.0, np.abs(T["w"]))
    labels = {S.signature(name, float(k), float(w)).label for k, w in zip(T["k"], T["w"])}
    shift = np.abs(T["predicted"] - T["w"])
    print(f"{name} {which}: {n} points, worst |predicted - w| = {shift.max():.1e} ({(shift / T['bound']).max():.1e} of the "
          f"bound), steps <= {T['iters'].max()}, worst resid = {np.nanmax(T['resid']):.1e} %, worst |w - port root| / "
          f"max(1, |w|) = {err.max():.1e} (bound {ROOT_BOUND:.0e}), labels {sorted(labels)}")
    assert err.max() <= ROOT_BOUND, (name, which, err)
    assert labels == {T["label"]}, (name, which, labels)                                # the label is kept
    worst_shift, steps = N.TRACE_TABLE[name]
    assert (shift <= T["bound"]).all() and shift.max() <= worst_shift and T["iters"].max() <= steps
    assert np.nanmax(T["resid"]) <= N.RESID_CEILING


def test_split_case_has_two_roots_per_row():
    """CR_kink's (1, 0): ks repeat, so trace_branches must skip the label; the hand split gives two strictly increasing curves"""
    w, k, cg = N.coarse_curves(N.SPLIT_CASE)[N.SPLIT_LABEL]
    assert not np.all(np.diff(k) > 0)
    for w2, k2, _ in N.split_curves().values():
        assert len(k2) == 4 and np.all(np.diff(k2) > 0) and np.isclose(k2[0], N.SPLIT_K_MIN)
    lo, up = N.split_curves()["lower"], N.split_curves()["upper"]
    assert np.all(lo[0] < up[0])


def test_trace_cases_carry_their_labels():
    for name, labels in N.TRACE_CASES.items():
        curves = N.coarse_curves(name)
        for lab in labels:
            assert lab in curves and len(curves[lab][1]) >= 2 and np.all(np.diff(curves[lab][1]) > 0), (name, lab)


@pytest.mark.parametrize("name", N.MODEL_CASES)
def test_offset_guesses_leave_clear_lanes(name):
    """The lanes the GPU test compares `iters` on: no step within a factor 10 of the stopping threshold.  At least half of
    the case's lanes and at least one lane with three or more steps are clear, and every lane ends on its root flagged 1."""
    k, g, root = N.offset_guesses(name)
    m = N.offset_model(name)
    clear = [N.clear(s, w) for s, w in zip(m["steps"], m["w"])]
    print(f"{name}: {len(k)} lanes, iters {m['iters'].tolist()}, clear {sum(clear)}, clear with >= 3 steps "
          f"{sum(1 for c, it in zip(clear, m['iters']) if c and it >= 3)}")
    assert len(k) >= 6 and m["flag"].tolist() == [1] * len(k)
    assert 2 * sum(clear) >= len(k)
    assert any(c and it >= 3 for c, it in zip(clear, m["iters"]))
    assert all(len(s) == it for s, it in zip(m["steps"], m["iters"]))


def test_rule_details():
    """max_iter = 0 is the final evaluation alone; step_cap caps the first step; max_shift clears the flag only; a leaky and a
    non-finite guess stop with ok = false, NaN resid and slope, and change nothing beside them."""
    name = "CF_flow_kink_N130"
    eq = N.M.all_cases()[name][0]
    k, g, root = N.offset_guesses(name)
    m0 = N.newton_model(name, k, g, max_iter=0)
    assert m0["iters"].tolist() == [0] * len(k) and np.array_equal(m0["w"], g) and np.isfinite(m0["resid"]).all()
    full = N.offset_model(name)
    lane = int(np.argmax([s[0] for s in full["steps"]]))
    cap = 0.25 * full["steps"][lane][0]
    capped = N.newton_model(name, k, g, step_cap=cap)
    assert capped["steps"][lane][0] == cap and capped["iters"][lane] > full["iters"][lane]
    assert abs(capped["w"][lane] - full["w"][lane]) <= 1e-14 * max(1.0, abs(full["w"][lane]))
    shift = N.newton_model(name, k, g, max_shift=0.5 * np.abs(full["w"] - g).max())
    assert np.array_equal(shift["w"], full["w"]) and np.array_equal(shift["iters"], full["iters"])
    assert 0 < shift["flag"].sum() < len(k)
    g2 = g.copy()
    g2[1] = k[1] * 1.05 * max(eq.c_e, eq.vA_e)               # above both exterior speeds: m_e < 0
    g2[3] = np.nan
    bad = N.newton_model(name, k, g2)
    assert bad["status"][1] == N.ST_LEAKY and bad["status"][3] == N.ST_NONFINITE
    for i in (1, 3):
        assert bad["iters"][i] == 0 and bad["flag"][i] == 0 and np.isnan(bad["resid"][i]) and np.isnan(bad["dwdk"][i])
    keep = [i for i in range(len(k)) if i not in (1, 3)]
    for f in ("w", "resid", "iters", "flag", "dwdk"):
        assert np.array_equal(bad[f][keep], full[f][keep]), f


def test_shifted_window_finds_an_exact_root():
    """A window centred on a root of the port puts D = 0 (or a last-bit value of either sign) on a grid point; the window
    shifted by a third of a cell brackets it."""
    name = "SFG_flow_kink_N130"
    k, w, _ = S.port_roots(name)
    for i in range(len(k)):
        r = N.port_root_near(name, float(k[i]), float(w[i]))
        assert r is not None and abs(r - w[i]) <= 4e-16 * max(1.0, abs(w[i])), (i, r, w[i])
