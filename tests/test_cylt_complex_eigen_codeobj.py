"""CPU-side checks of section 19 (eigenfunctions of complex roots of the twisted cylinder; no GPU needed, in the manner of
tests/test_cyl_complex_eigen_codeobj.py).

Code object: the interior kernel of the twisted family is there under its name in es_cyl_complex_eigen.o, spills no vector
register, has no private segment, holds the LDS of one staged chunk of the 20-field base table, runs workgroups of 64 and
keeps to the 512 registers a lane has at one wave per SIMD; the exterior kernel, which serves both families, is still in one
object only.  The figures -- scalar spills included, which are not bounded -- are printed.  Metadata only
(tools/codeobj_table.py).  As built: 176 VGPRs, no AGPR, nothing spilled, vector or scalar, 41 120 B of LDS.

ABI: the header declares es_cylt_complex_eigenfunction, the built library exports it with the signature of
es_cyl_complex_eigenfunction, and RotatingCylinderComplex has the four methods of CylinderComplex, the same functions."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

needs_llvm = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="ROCm LLVM tools not present")

KERNEL, OBJECT = "cylteig_interior_kernel", "es_cyl_complex_eigen.o"
CHUNK_LDS = 20 * (2 * 128 + 1) * 8                          # the 20 base fields at the nodes and mid-points of 128 steps
METHODS = ("eigenfunction", "polarisation", "field_synthesis", "fields")


@pytest.fixture(scope="module")
def codeobj_table():
    if os.environ.get("ES_BUILD_ALL_SHAPES") == "1" or os.environ.get("ES_BUILD_EXTRA_FLAGS"):
        pytest.skip("measuring build")
    from eigensolver_amd import build
    build.build()
    import codeobj_table
    return codeobj_table


@needs_llvm
def test_interior_kernel_of_the_twisted_family(codeobj_table):
    rows = codeobj_table.table("cylteig_")
    assert [(r["kernel"], r["object"]) for r in rows] == [(KERNEL, OBJECT)]
    r = rows[0]
    fig = (r[".vgpr_count"], r.get(".agpr_count", 0), r.get(".vgpr_spill_count", 0), r.get(".sgpr_spill_count", 0),
           r.get(".sgpr_count", 0), r.get(".private_segment_fixed_size", 0), r.get(".group_segment_fixed_size", 0))
    print(KERNEL, "VGPRs, AGPRs, spilled VGPRs, spilled SGPRs, SGPRs, scratch B/lane, LDS B:", fig)
    assert r.get(".group_segment_fixed_size", 0) == CHUNK_LDS == 41120, fig
    assert r.get(".vgpr_spill_count", 0) == 0 and r.get(".private_segment_fixed_size", 0) == 0, fig
    assert r.get(".max_flat_workgroup_size") == 64
    assert r[".vgpr_count"] + r.get(".agpr_count", 0) <= 512, fig


@needs_llvm
def test_exterior_kernel_is_shared_not_copied(codeobj_table):
    """Both entry points launch cyleig_exterior_kernel: one kernel in one object."""
    rows = codeobj_table.table("cyleig_exterior_kernel")
    assert [(r["kernel"], r["object"]) for r in rows] == [("cyleig_exterior_kernel", OBJECT)]


def test_header_declares_the_entry_point():
    with open(os.path.join(ROOT, "include", "eigensolver_amd.h")) as f:
        text = f.read()
    decl = re.search(r"^int es_cylt_complex_eigenfunction\(([^;]*)\);", text, re.M | re.S)
    untw = re.search(r"^int es_cyl_complex_eigenfunction\(([^;]*)\);", text, re.M | re.S)
    assert decl and untw
    strip = lambda s: re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", s, flags=re.S)).strip()      # noqa: E731
    assert strip(decl.group(1)) == strip(untw.group(1))                     # the signature of section 16, word for word


def test_library_exports_section_19():
    from eigensolver_amd import _lib, build
    build.build()
    lib = _lib.load()
    assert hasattr(lib, "es_cylt_complex_eigenfunction")
    assert len(lib.es_cylt_complex_eigenfunction.argtypes) == 13
    assert lib.es_cylt_complex_eigenfunction.argtypes == lib.es_cyl_complex_eigenfunction.argtypes


def test_both_classes_have_the_four_methods_once():
    from eigensolver_amd import CylinderComplex, RotatingCylinderComplex
    for name in METHODS:
        assert callable(getattr(RotatingCylinderComplex, name, None)), name
        assert getattr(RotatingCylinderComplex, name) is getattr(CylinderComplex, name), name
    assert CylinderComplex._PREFIX == "es_cyl_complex_" and RotatingCylinderComplex._PREFIX == "es_cylt_complex_"
