"""CPU-side checks of the ES_REFINE_HYBRID refinement rule: the C ABI and its ctypes binding, and the rule itself through its
host model (tests/refine_hybrid_model.py, a NumPy restatement over the CPU port's evaluator) against the port's section
rule on all fourteen cases of tests/cases.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import cases, refine_hybrid_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"es_context_set_refine_rule": 2, "es_context_get_refine_rule": 2, "es_context_refine_stats": 2}
CASES = cases.all_cases()
ROOT_RTOL = 1e-10               # tests/test_shoot_gpu.py
SECTION_MARCHES = 66            # 4 rounds of 16 lanes + 2 polish steps at n_bisect = 16
FLOAT_COLS = ("k", "w", "w_lo", "w_hi", "resid")


def _header():
    txt = open(os.path.join(ROOT, "include", "eigensolver_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_and_library_exports_the_refine_rule_calls():
    txt = _header()
    for name, nargs in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", txt)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
    from eigensolver_amd import build
    lib = ctypes.CDLL(build.build())
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing
    lib.es_abi_version.restype = ctypes.c_int
    assert lib.es_abi_version() == 1


def test_ctypes_constants_and_signatures_match_the_header():
    from eigensolver_amd import _lib, shooting
    m = re.search(r"enum\s*\{\s*ES_REFINE_SECTION\s*=\s*(\d+)\s*,\s*ES_REFINE_HYBRID\s*=\s*(\d+)\s*\}", _header())
    assert m, "enum { ES_REFINE_SECTION, ES_REFINE_HYBRID } not found"
    assert (_lib.REFINE_SECTION, _lib.REFINE_HYBRID) == (int(m.group(1)), int(m.group(2))) == (0, 1)
    assert (shooting.REFINE_SECTION, shooting.REFINE_HYBRID) == (_lib.REFINE_SECTION, _lib.REFINE_HYBRID)

    class Fake:
        def __getattr__(self, name):
            f = type("F", (), {})()
            object.__setattr__(self, name, f)
            return f
    lib = _lib._sig(Fake())
    for name, nargs in NEW.items():
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert _lib.RefineStats._fields == ("brackets", "kept", "fallback", "evaluations")
    assert isinstance(_lib.Context.refine_rule, property) and _lib.Context.refine_rule.fset is not None


def test_model_constants_are_the_kernel_s():
    src = open(os.path.join(ROOT, "eigensolver_amd", "csrc", "es_refine.hip")).read()
    def const(name):
        return re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([0-9.eE+-]+)\s*;", src).group(1)
    assert int(const("kHybridSections")) == hm.HYBRID_SECTIONS and hm.HYBRID_SECTIONS in (1, 2)
    assert int(const("kHybridSteps")) == hm.ONE_LANE_STEPS == 8
    assert float(const("kHybridEps")) == hm.ONE_LANE_EPS == ROOT_RTOL / 100
    assert int(const("kRefineSections")) == hm.SECTIONS


def _grid(name):
    eq, mode, m, (lo, hi) = CASES[name]
    port = cases.port_problem(eq, mode, m)
    k = np.linspace(0.4, 3.9, 24)
    W = lo + (np.arange(192) + 0.5) * (hi - lo) / 192
    D, _, st = port.eval_grid(k, W, w_mode=1, nthreads=8)
    return port, k, W, D, st


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["CF_flow_kink", "SFG_flow_kink"])
@pytest.mark.parametrize("n_bisect", [16, 3])
def test_model_with_full_fallback_is_the_port(name, n_bisect):
    """Zero one-lane steps: every bracket takes the fallback, so the model's section rounds and polish steps alone must
    reproduce port.find_roots bit for bit."""
    port, k, W, D, st = _grid(name)
    Tp, cp = port.find_roots(k, W, D, st, w_mode=1, n_bisect=n_bisect, tol=1e-3, nthreads=8)
    Th, ch, info = hm.find_roots(port, k, W, D, st, n_bisect=n_bisect, tol=1e-3, steps=0, nthreads=8)
    assert ch == cp > 0
    assert not info["kept"].any()
    for c in Tp:
        assert _same(Th[c], Tp[c]), (name, n_bisect, c)


@pytest.mark.parametrize("name", list(CASES))
def test_hybrid_model_against_the_section_rule(name):
    port, k, W, D, st = _grid(name)
    Ts, cs = port.find_roots(k, W, D, st, w_mode=1, n_bisect=16, tol=1e-3, nthreads=8)
    Tc, cc = port.find_roots(k, W, D, st, w_mode=1, n_bisect=44, tol=1e-3, nthreads=8)
    Th, ch, info = hm.find_roots(port, k, W, D, st, n_bisect=16, tol=1e-3, nthreads=8)
    kept, fb = info["kept"], info["fallback"]
    assert ch == cs == cc > 0
    assert _same(Th["row"], Ts["row"]) and _same(Th["k"], Ts["k"])
    assert np.array_equal(kept, ~fb)
    assert np.all(Th["flag"] >= Ts["flag"])
    # rows the one-lane phase did not produce are the section rule's rows
    for mask, what in ((Th["flag"] == 0, "flag 0"), (fb, "fallback")):
        for c in FLOAT_COLS + ("flag",):
            assert _same(Th[c][mask], Ts[c][mask]), (name, what, c)
    # kept rows: accepted by the converged section table, and the same root
    assert np.all(Th["flag"][kept] == 1)
    assert np.all(Tc["flag"][kept] == 1), (name, np.nonzero(kept & (Tc["flag"] != 1))[0])
    err = np.abs(Th["w"][kept] - Tc["w"][kept]) / np.abs(Tc["w"][kept])
    worst = err.max() if kept.any() else 0.0
    mpb = hm.marches_per_bracket(16, ch, int(fb.sum()), int(info["evals"].sum()))
    ek = info["evals"][kept].mean() if kept.any() else 0.0
    print(f"{name}: {ch} brackets, {int(Ts['flag'].sum())} accepted, {int(kept.sum())} kept, {int(fb.sum())} fallback "
          f"({int(Ts['flag'][fb].sum())} of them accepted), max |dw/w| kept {worst:.2e}, {ek:.2f} evaluations per kept "
          f"bracket, {mpb:.1f} marches per bracket")
    assert worst < ROOT_RTOL, (name, worst)
    assert np.all((Th["w_lo"] <= Th["w"]) & (Th["w"] <= Th["w_hi"]))
    assert np.all((info["cell_lo"] <= Th["w_lo"]) & (Th["w_hi"] <= info["cell_hi"]))
    assert np.all((info["evals"] >= 1) & (info["evals"] <= hm.ONE_LANE_STEPS))
    assert mpb < SECTION_MARCHES, (name, mpb)
