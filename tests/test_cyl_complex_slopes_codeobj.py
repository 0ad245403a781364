"""CPU-side checks of the code objects of the slope and Newton kernels of the cylinder's complex path, both families (C ABI
sections 15 and 18; no GPU needed, in the manner of tests/test_cyl_complex_codeobj.py): the two kernels are there once per
family under their names, all in one object, none spills a vector register or has a private segment, all keep to the 512
registers a lane has at one wave per SIMD at 64 threads per workgroup, and each holds the LDS of one staged chunk of its
family's base table -- the Newton kernels with the words of the workgroup vote that ends their loop on top.  The twisted
family's slopes kernel spills no scalar register either, and its Newton kernel is held to the count it was brought to.  The
figures are printed.  Metadata only (tools/codeobj_table.py).

As built: cyljet_slopes_kernel<1> 256 VGPRs + 1 AGPR, nothing spilled; cyljet_newton_kernel<1> 256 VGPRs + 80 AGPRs, 6 scalar
registers spilled to vector lanes, no vector register spilled, no private segment.  The Newton kernel holds two inlined copies
of the evaluation under the loop and vote of cx_newton_lane and spilled 53 scalar registers as first written for the twisted
family; es_cyl_complex_slopes.hip and DESIGN.md section 8m say what brought that to 6 and what the 6 are."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="ROCm LLVM tools not present")

KERNELS = ("cyljet_newton_kernel", "cyljet_slopes_kernel")
BASE_FIELDS = {0: 7, 1: 20}                                 # the kernels' template argument: FAM_CYL0, FAM_CYLT
CHUNK_LDS = {f: nb * (2 * 128 + 1) * 8 for f, nb in BASE_FIELDS.items()}    # the fields at the nodes and mid-points of 128 steps
NEWTON_SGPR_SPILLS = 6                                      # twisted family: the lowest count reached; as first written: 53


@pytest.fixture(scope="module")
def table():
    if os.environ.get("ES_BUILD_ALL_SHAPES") == "1" or os.environ.get("ES_BUILD_EXTRA_FLAGS"):
        pytest.skip("measuring build")
    from eigensolver_amd import build
    build.build()
    import codeobj_table
    return codeobj_table.table("cyljet_")


@pytest.mark.parametrize("fam", sorted(BASE_FIELDS))
def test_kernels_present_once(table, fam):
    """The filter `cyljet_` finds the two kernels of the family, each once and in es_cyl_complex_slopes.o, and four in all."""
    assert sorted((r["kernel"], r["object"]) for r in table if r["kernel"].endswith(f"<{fam}>")) == sorted(
        (f"{k}<{fam}>", "es_cyl_complex_slopes.o") for k in KERNELS)
    assert len(table) == 2 * len(BASE_FIELDS) == 4


@pytest.mark.parametrize("fam", sorted(BASE_FIELDS))
@pytest.mark.parametrize("k", KERNELS)
def test_spills_registers_and_lds(table, k, fam):
    r = {row["kernel"]: row for row in table}[f"{k}<{fam}>"]
    fig = (r[".vgpr_count"], r.get(".agpr_count", 0), r.get(".vgpr_spill_count", 0), r.get(".sgpr_spill_count", 0),
           r.get(".private_segment_fixed_size", 0), r.get(".group_segment_fixed_size", 0))
    print(r["kernel"], "VGPRs, AGPRs, spilled VGPRs, spilled SGPRs, scratch B/lane, LDS B:", fig)
    assert r.get(".vgpr_spill_count", 0) == 0 and r.get(".private_segment_fixed_size", 0) == 0, (k, fam, fig)
    assert r[".vgpr_count"] <= 512, (k, fam, fig)
    assert r.get(".max_flat_workgroup_size") == 64, (k, fam)
    lds, chunk = r.get(".group_segment_fixed_size", 0), CHUNK_LDS[fam]
    assert chunk == {0: 14392, 1: 41120}[fam]
    if k == "cyljet_slopes_kernel":
        assert lds == chunk, (k, fam, fig)
        if fam == 1:
            assert r.get(".sgpr_spill_count", 0) == 0, (k, fam, fig)
    else:
        assert chunk < lds <= chunk + 512, (k, fam, fig)                # the vote words of cx_newton_lane on top
        if fam == 1:
            assert r.get(".sgpr_spill_count", 0) <= NEWTON_SGPR_SPILLS <= 53, (k, fam, fig)


def test_filters_find_one_object_each_and_no_earlier_name(table):
    """`cylc_` names kernels of es_cyl_complex.o only, `cyljet_` of es_cyl_complex_slopes.o only, four each; no kernel of the
    library is named `cyltc_` or `cyltjet_` any more."""
    import codeobj_table
    assert [r["object"] for r in codeobj_table.table("cylc_")] == ["es_cyl_complex.o"] * 4
    assert [r["object"] for r in table] == ["es_cyl_complex_slopes.o"] * 4
    assert codeobj_table.table("cyltc_|cyltjet_") == []
