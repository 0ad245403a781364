"""The root search of the closed-form uniform cylinder is present at every layer: exported by the built library,
typed in the ctypes binding, and reachable from CylinderUniform (no GPU needed)."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("es_cyl_uniform_find_roots", "es_cyl_uniform_find_roots_async")


def test_header_declares_both_entry_points_and_keeps_the_abi_version():
    txt = open(os.path.join(ROOT, "include", "eigensolver_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", code), s
    assert re.search(r"#define\s+ES_ABI_VERSION\s+1\b", code)


def test_library_exports_and_binding_types_both_entry_points():
    from eigensolver_amd import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        fn = getattr(lib, s)                       # AttributeError if the shared object does not export it
        assert fn.argtypes is not None and len(fn.argtypes) == 16, s
        assert fn.argtypes[1] == C.POINTER(_lib.CylUniformParams)
        assert fn.argtypes[13] == C.POINTER(_lib.RootTable)
    assert lib.es_cyl_uniform_find_roots.argtypes[15] == C.POINTER(C.c_int)          # h_count
    assert lib.es_cyl_uniform_find_roots_async.argtypes[15] == C.c_void_p            # d_count
    assert lib.es_abi_version() == 1
    assert lib.es_abi_sizeof(5) == C.sizeof(_lib.CylUniformParams)


def test_cylinder_uniform_has_the_search_methods():
    from eigensolver_amd import CylinderUniform
    for name in ("find_roots", "find_roots_async", "alloc_root_table"):
        assert callable(getattr(CylinderUniform, name)), name


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="ROCm LLVM tools not present")
def test_search_kernels_have_no_scratch():
    """The fused evaluate-and-flag kernel and the kernels behind it keep everything in registers."""
    from eigensolver_amd import build
    build.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_table
    rows = {r["kernel"]: r for r in codeobj_table.table("cyl_uniform")}
    for name in ("cyl_uniform_flag_kernel", "cyl_uniform_emit_kernel", "cyl_uniform_ends_kernel",
                 "cyl_uniform_refine_kernel", "cyl_uniform_kernel"):
        assert rows[name].get(".vgpr_spill_count", 0) == 0, rows[name]
        assert rows[name].get(".private_segment_fixed_size", 0) == 0, rows[name]
