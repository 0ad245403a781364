"""CPU-side checks of the code objects of the complex-frequency kernels of the cylinder, both families (C ABI sections 14 and
17; no GPU needed, in the manner of tests/test_complex_slopes_codeobj.py): the evaluation and refinement kernels are there
once per family under their names, all in one object, none spills a vector register or has a private segment, each holds the
LDS of one staged chunk of its family's base table, the workgroup sizes are 256 and 64, and all keep to the 512 registers a
lane has at one wave per SIMD.  The twisted family's kernels spill no scalar register either.  The figures are printed.
Metadata only (tools/codeobj_table.py).

As built: cylc_eval_kernel<1> 164 VGPRs; cylc_refine_kernel<1> 264 VGPRs + 8 AGPRs; nothing spilled in either, no private
segment.  The refinement kernel holds four inlined copies of the evaluation (cx_refine_candidate calls it at four places) and
spilled 61 scalar registers to vector lanes as first written for the twisted family; es_cyl_complex.hip and DESIGN.md section
8l say what brought that to none."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="ROCm LLVM tools not present")

WORKGROUP = {"cylc_eval_kernel": 256, "cylc_refine_kernel": 64}
BASE_FIELDS = {0: 7, 1: 20}                                 # the kernels' template argument: FAM_CYL0, FAM_CYLT
CHUNK_LDS = {f: nb * (2 * 128 + 1) * 8 for f, nb in BASE_FIELDS.items()}    # the fields at the nodes and mid-points of 128 steps


@pytest.fixture(scope="module")
def table():
    if os.environ.get("ES_BUILD_ALL_SHAPES") == "1" or os.environ.get("ES_BUILD_EXTRA_FLAGS"):
        pytest.skip("measuring build")
    from eigensolver_amd import build
    build.build()
    import codeobj_table
    return codeobj_table.table("cylc_")


@pytest.mark.parametrize("fam", sorted(BASE_FIELDS))
def test_kernels_present(table, fam):
    """The filter `cylc_` finds the two kernels of the family, both in es_cyl_complex.o, and four kernels in all."""
    assert sorted((r["kernel"], r["object"]) for r in table if r["kernel"].endswith(f"<{fam}>")) == sorted(
        (f"{k}<{fam}>", "es_cyl_complex.o") for k in WORKGROUP)
    assert len(table) == 2 * len(BASE_FIELDS) == 4


@pytest.mark.parametrize("fam", sorted(BASE_FIELDS))
@pytest.mark.parametrize("k", sorted(WORKGROUP))
def test_no_spill_and_no_private_segment(table, k, fam):
    r = {row["kernel"]: row for row in table}[f"{k}<{fam}>"]
    fig = (r[".vgpr_count"], r.get(".agpr_count", 0), r.get(".vgpr_spill_count", 0), r.get(".sgpr_spill_count", 0),
           r.get(".private_segment_fixed_size", 0), r.get(".group_segment_fixed_size", 0))
    print(r["kernel"], "VGPRs, AGPRs, spilled VGPRs, spilled SGPRs, scratch B/lane, LDS B:", fig)
    assert r.get(".vgpr_spill_count", 0) == 0 and r.get(".private_segment_fixed_size", 0) == 0, (k, fam, fig)
    assert r.get(".group_segment_fixed_size", 0) == CHUNK_LDS[fam] == {0: 14392, 1: 41120}[fam], (k, fam, fig)
    assert r[".vgpr_count"] <= 512, (k, fam, fig)
    assert r.get(".max_flat_workgroup_size") == WORKGROUP[k], (k, fam)
    if fam == 1:
        assert r.get(".sgpr_spill_count", 0) == 0, (k, fam, fig)


def test_slab_search_kernels_are_still_one_instance(table):
    """The flag and emit kernels serve every geometry from es_complex.hip: no further copy in the cylinder's object."""
    import codeobj_table
    objs = {}
    for r in codeobj_table.table("cx_(flag|emit)_kernel"):
        objs.setdefault(r["kernel"], []).append(os.path.basename(r["object"]))
    assert objs == {"cx_flag_kernel": ["es_complex.o"], "cx_emit_kernel": ["es_complex.o"]}
