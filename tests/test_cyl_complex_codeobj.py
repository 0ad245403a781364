"""CPU-side checks of the code objects of the complex-frequency kernels of the cylinder (C ABI section 14; no GPU needed, in
the manner of tests/test_complex_slopes_codeobj.py): both kernels are there under their names, neither spills a VGPR or has a
private segment, each holds the LDS of one staged chunk of the untwisted cylinder's base table, and the refinement kernel
keeps to the registers of one wave per SIMD.  The figures are printed.  Metadata only (tools/codeobj_table.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="ROCm LLVM tools not present")

KERNELS = ("cylc_eval_kernel", "cylc_refine_kernel")
CHUNK_LDS = 7 * (2 * 128 + 1) * 8                           # the seven base fields at the nodes and mid-points of 128 steps


@pytest.fixture(scope="module")
def rows():
    if os.environ.get("ES_BUILD_ALL_SHAPES") == "1" or os.environ.get("ES_BUILD_EXTRA_FLAGS"):
        pytest.skip("measuring build")
    from eigensolver_amd import build
    build.build()
    import codeobj_table
    return {r["kernel"]: r for r in codeobj_table.table("cylc_")}


def test_kernels_present(rows):
    assert sorted(rows) == sorted(KERNELS)


def test_no_spill_and_no_private_segment(rows):
    for k in KERNELS:
        r = rows[k]
        fig = (r[".vgpr_count"], r.get(".agpr_count", 0), r.get(".vgpr_spill_count", 0), r.get(".private_segment_fixed_size", 0),
               r.get(".group_segment_fixed_size", 0))
        print(k, "VGPRs, AGPRs, spilled VGPRs, scratch B/lane, LDS B:", fig)
        assert r.get(".vgpr_spill_count", 0) == 0 and r.get(".private_segment_fixed_size", 0) == 0, (k, fig)
        assert r.get(".group_segment_fixed_size", 0) == CHUNK_LDS, (k, fig)
    assert rows["cylc_refine_kernel"][".vgpr_count"] <= 512
    assert rows["cylc_refine_kernel"].get(".max_flat_workgroup_size", 64) == 64
    assert rows["cylc_eval_kernel"].get(".max_flat_workgroup_size", 256) == 256


def test_slab_search_kernels_are_still_one_instance(rows):
    """The flag and emit kernels serve both geometries from es_complex.hip: no second copy in the cylinder's object."""
    import codeobj_table
    objs = {}
    for r in codeobj_table.table("cx_(flag|emit)_kernel"):
        objs.setdefault(r["kernel"], []).append(os.path.basename(r["object"]))
    assert objs == {"cx_flag_kernel": ["es_complex.o"], "cx_emit_kernel": ["es_complex.o"]}
