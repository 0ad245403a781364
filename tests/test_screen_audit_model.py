"""The NumPy model of es_shoot_audit_screening (tests/screen_audit_model.py) on hand-worked cases, and the host side of
the feature: the header declares the entry and its enums, the library exports it, the ABI version and es_abi_sizeof are
untouched, and _lib.check_audit turns a failed audit into the error of ES_ERR_SCREENING.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import screen_audit_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
nan, inf = np.nan, np.inf


def _worked_example():
    D64 = np.array([[1, 2, -3, -1, .5, .7], [-1, -2, 4, nan, 1, -1]], dtype=np.float64)
    st64 = np.array([[0] * 6, [0, 0, 0, 2, 0, 1]], dtype=np.uint8)
    D_scr, st_scr = D64.copy(), st64.copy()
    D_scr[0, 2] = 1.5                  # vouched for with the wrong sign: the bracket at cell 1 moves to cell 2
    D_scr[0, 4] = -9                   # wrong, but marked unsure: the merged grid takes the fp64 value
    st_scr[0, 4] |= M.UNSURE
    st_scr[1, 5] = 0                   # a leaky point vouched for as OK: wrong status, and a false bracket at cell 10
    D_scr[1, 0] = -1.25                # right sign, margin 4
    return D_scr, st_scr, D64, st64


def test_worked_example():
    a = M.audit(*_worked_example())
    assert a.counts[:8].tolist() == [4, 1, 2, 1, 1, 9, 1, 3]
    assert a.cell.tolist() == [1, 2, 10, 11]
    assert a.kind.tolist() == [M.MISSED, M.FALSE | M.SIGN, M.FALSE, M.STATUS]
    assert a.counts[8] == 2 and a.worst[0] == 3.0 / 4.5
    assert a.counts[9] == -1 and a.worst[1] == 0.0                 # no rel64 given


def test_err_is_the_formula_of_the_mixed_test():
    D_scr, st_scr, D64, st64 = _worked_example()
    rel = np.full(D64.shape, 10.0)
    rel[1, 0] = 0.5                    # scale = |D64| 100 / rel = 200: err = 0.25 / 200
    rel[0, 2] = nan                    # no usable scale at the point with the largest difference
    a = M.audit(D_scr, st_scr, D64, st64, rel)
    assert a.counts[9] == 6 and a.worst[1] == 0.25 / (1.0 * 100.0 / 0.5)
    assert a.counts[8] == 2                                        # the margin does not depend on rel


def test_last_column_and_row_boundary_are_never_brackets():
    # a sign change from the end of row 0 to the start of row 1, in both grids and in one only
    D64 = np.array([[1.0, 1.0, 1.0], [-1.0, -1.0, -1.0]])
    st = np.zeros((2, 3), dtype=np.uint8)
    a = M.audit(D64, st, D64, st)
    assert a.counts[:8].tolist() == [0, 0, 0, 0, 0, 6, 0, 0]
    D_scr = D64.copy()
    D_scr[0, 2] = -1.0                 # wrong sign in the last column: a false bracket at cell 1, none at cell 2
    a = M.audit(D_scr, st, D64, st)
    assert a.cell.tolist() == [1, 2] and a.kind.tolist() == [M.FALSE, M.SIGN]
    assert a.counts[7] == 0 and a.counts[8] == 2 and a.worst[0] == 0.5
    # one column: no brackets at all
    a = M.audit(np.array([[1.0], [-1.0]]), np.zeros((2, 1), np.uint8), np.array([[-1.0], [1.0]]), np.zeros((2, 1), np.uint8))
    assert a.counts[:5].tolist() == [2, 0, 0, 0, 2]


def test_nan_and_signed_zero():
    D64 = np.array([[1.0, nan, -1.0, 0.0, -1.0, 2.0]])
    st = np.zeros((1, 6), dtype=np.uint8)
    D_scr = np.array([[1.0, -1.0, nan, -0.0, -1.0, 2.0]])
    a = M.audit(D_scr, st, D64, st)
    # cell 0: the merged product 1 * -1 is a bracket, the fp64 product 1 * nan is not; cell 1: signbit(-1) != signbit(nan)
    # cell 2: signbit(nan) != signbit(-1); cell 3: -0 against +0 is a sign difference, 0 * -1 is no bracket in either grid
    assert a.cell.tolist() == [0, 1, 2, 3]
    assert a.kind.tolist() == [M.FALSE, M.SIGN, M.SIGN, M.SIGN]
    # NaN points and -0 == +0 are not compared points: no margin
    assert a.counts[8] == -1 and a.worst[0] == inf
    # inf against a finite value is compared (margin 0); inf against -inf gives a NaN margin, which is skipped
    D64 = np.array([[1.0, inf, 2.0]])
    D_scr = np.array([[inf, -inf, 2.5]])
    a = M.audit(D_scr, np.zeros((1, 3), np.uint8), D64, np.zeros((1, 3), np.uint8))
    assert a.counts[8] == 0 and a.worst[0] == 0.0
    a = M.audit(D_scr[:, 1:], np.zeros((1, 2), np.uint8), D64[:, 1:], np.zeros((1, 2), np.uint8))
    assert a.counts[8] == 1 and a.worst[0] == 4.0


def test_capacity_below_the_count_keeps_the_first_cells():
    args = _worked_example()
    full = M.audit(*args)
    a = M.audit(*args, capacity=3)
    assert a.counts.tolist() == full.counts.tolist()
    assert a.cell.tolist() == [1, 2, 10] and a.kind.tolist() == full.kind[:3].tolist()
    a = M.audit(*args, capacity=0)
    assert a.counts[0] == 4 and a.cell.size == 0 and a.kind.size == 0


@pytest.mark.parametrize("shape", [(0, 5), (3, 0), (0, 0)])
def test_empty_grid(shape):
    z, s = np.zeros(shape), np.zeros(shape, dtype=np.uint8)
    a = M.audit(z, s, z, s, z)
    assert a.counts.tolist() == [0] * 8 + [-1, -1]
    assert a.worst.tolist() == [inf, 0.0] and a.cell.size == 0


def test_ties_go_to_the_smallest_cell():
    D64 = np.array([[4.0, 1.0, 4.0, -8.0], [4.0, 2.0, 4.0, 4.0]])
    D_scr = D64 + np.array([[0.0, 0.5, 2.0, 4.0], [2.0, 0.0, 1.0, 2.0]])       # margins -, 2, 2, 2 / 2, -, 4, 2
    st = np.zeros((2, 4), dtype=np.uint8)
    rel = 100.0 * np.ones((2, 4))                                              # scale = |D64|: err = 1 / margin
    a = M.audit(D_scr, st, D64, st, rel)
    assert a.worst.tolist() == [2.0, 0.5] and a.counts[8] == 1 and a.counts[9] == 1
    st_scr = st.copy()
    st_scr[0, 1] = M.UNSURE                                                    # the first of the tied points leaves
    a = M.audit(D_scr, st_scr, D64, st, rel)
    assert a.worst.tolist() == [2.0, 0.5] and a.counts[8] == 2 and a.counts[9] == 2 and a.counts[6] == 1


# ---- the host side of the feature ---------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "eigensolver_amd.h")).read()


def test_header_declares_the_entry_and_its_enums():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+es_shoot_audit_screening\s*\(\s*es_context\s*\*\s*ctx\s*,\s*int\s+nk\s*,\s*int\s+nw\s*,", code)
    assert re.search(r"ES_PT_SCREEN_UNSURE\s*=\s*0x80\b", code)
    assert re.search(r"ES_AUDIT_MISSED\s*=\s*1\s*,\s*ES_AUDIT_FALSE\s*=\s*2\s*,\s*ES_AUDIT_STATUS\s*=\s*4\s*,"
                     r"\s*ES_AUDIT_SIGN\s*=\s*8\b", code)
    assert re.search(r"#define\s+ES_ABI_VERSION\s+1\s", code)


def test_library_exports_the_entry_and_the_abi_is_unchanged():
    from eigensolver_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "es_shoot_audit_screening")
    lib.es_abi_version.restype = ctypes.c_int
    assert lib.es_abi_version() == 1
    lib.es_abi_sizeof.restype = ctypes.c_int
    lib.es_abi_sizeof.argtypes = [ctypes.c_int]
    assert lib.es_abi_sizeof(8) == -1                              # the audit takes plain arrays: no new ABI struct
    assert (_lib.PT_SCREEN_UNSURE, _lib.AUDIT_MISSED, _lib.AUDIT_FALSE, _lib.AUDIT_STATUS, _lib.AUDIT_SIGN) == \
        (M.UNSURE, M.MISSED, M.FALSE, M.STATUS, M.SIGN)
    # argument errors need no device: a null context is refused before anything else is looked at
    assert _lib.load().es_shoot_audit_screening(None, 1, 1, None, None, None, None, None, 0, None, None, None, None) == 1


def _report(a, nw):
    from eigensolver_amd import _lib
    at = lambda c: None if c < 0 else (int(c) // nw, int(c) % nw)          # noqa: E731
    return _lib.ScreenAudit(*[int(v) for v in a.counts[:8]], float(a.worst[0]), at(a.counts[8]), float(a.worst[1]),
                            at(a.counts[9]), a.cell // nw, a.cell % nw, a.kind)


def test_check_audit_raises_the_screening_error():
    from eigensolver_amd import _lib
    D_scr, st_scr, D64, st64 = _worked_example()
    clean = _report(M.audit(D64, st64, D64, st64), 6)
    assert clean.ok and _lib.check_audit(clean) is clean
    doctored = _report(M.audit(D_scr, st_scr, D64, st64), 6)
    assert not doctored.ok and (doctored.missed, doctored.false, doctored.status) == (1, 2, 1)
    with pytest.raises(_lib.EsError, match=r"screening.*row 0, col 1"):
        _lib.check_audit(doctored)
    # a wrong sign alone moves no bracket and is reported, not raised: ok is missed == false == status == 0
    sign_only = clean._replace(flagged=1, sign=1)
    assert sign_only.ok and _lib.check_audit(sign_only) is sign_only
    # counts without a table (capacity 0) still raise
    with pytest.raises(_lib.EsError, match="screening"):
        _lib.check_audit(doctored._replace(row=np.zeros(0, np.int64), col=np.zeros(0, np.int64), kind=np.zeros(0, np.uint8)))
