"""CPU-side checks of the mixed-precision search with device-side counts: the header declares
es_shoot_find_roots_screened_async / es_shoot_find_roots_mixed_async and the built library exports them (as
test_abi.py checks the whole header), and shooting.read_screen_counts reads the four count words."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("es_shoot_find_roots_screened_async", "es_shoot_find_roots_mixed_async")


def test_header_declares_and_library_exports_the_async_mixed_calls():
    txt = open(os.path.join(ROOT, "include", "eigensolver_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", txt)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == 13 and params[-1].replace(" ", "") == "int32_t*d_counts", params
    from eigensolver_amd import build
    lib = ctypes.CDLL(build.build())
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing


def test_ctypes_signatures_cover_the_async_mixed_calls():
    from eigensolver_amd import _lib

    class Fake:
        def __getattr__(self, name):
            f = type("F", (), {})()
            object.__setattr__(self, name, f)
            return f
    lib = _lib._sig(Fake())
    for name in NEW:
        assert len(getattr(lib, name).argtypes) == 13, name


def _counts(*v):
    import torch
    return torch.tensor(v, dtype=torch.int32)


def test_read_screen_counts_clean():
    from eigensolver_amd.shooting import read_screen_counts
    c = read_screen_counts(_counts(37, 1200, 74, 0), 64)
    assert (c.count, c.unsure, c.ends, c.violations, c.overflow) == (37, 1200, 74, 0, False)
    assert read_screen_counts(_counts(64, 0, 128, 0), 64).overflow is False     # exactly full is not an overflow
    assert read_screen_counts(_counts(0, 0, 0, 0), 0) == (0, 0, 0, 0, False)


def test_read_screen_counts_overflow():
    from eigensolver_amd.shooting import read_screen_counts
    c = read_screen_counts(_counts(90, 11, 10, 0), 5)
    assert c.overflow is True and c.count == 90 and c.ends == 10


def test_read_screen_counts_violation_raises():
    from eigensolver_amd import EsError
    from eigensolver_amd.shooting import read_screen_counts
    with pytest.raises(EsError, match="fp32-screened bracket not confirmed in fp64"):
        read_screen_counts(_counts(12, 40, 24, 2), 64)
