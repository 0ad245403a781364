"""CPU-side checks of the code objects of the slope and Newton kernels of the twisted cylinder's complex path (C ABI section 18;
no GPU needed, in the manner of tests/test_cyl_complex_slopes_codeobj.py): both kernels are there under their names, each in
one object, neither spills a vector register or has a private segment, both keep to the 512 registers a lane has at one wave
per SIMD at 64 threads per workgroup, and each holds the LDS of one staged chunk of the twisted family's 20-field base table --
the Newton kernel with the words of the workgroup vote that ends its loop on top.  The slopes kernel spills no scalar register
either.  The Newton kernel is held to the count it was brought to.  The figures are printed.  Metadata only
(tools/codeobj_table.py).

As built: cyltjet_slopes_kernel 256 VGPRs + 1 AGPR, nothing spilled; cyltjet_newton_kernel 256 VGPRs + 80 AGPRs, 6 scalar
registers spilled to vector lanes, no vector register spilled, no private segment.  The Newton kernel holds two inlined copies
of the evaluation under the loop and vote of cx_newton_lane and spilled 53 scalar registers as first written;
es_cylt_complex_slopes.hip and DESIGN.md section 8m say what brought that to 6 and what the 6 are."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="ROCm LLVM tools not present")

KERNELS = ("cyltjet_newton_kernel", "cyltjet_slopes_kernel")
CHUNK_LDS = 20 * (2 * 128 + 1) * 8                          # the 20 base fields at the nodes and mid-points of 128 steps: 41 120 B
NEWTON_SGPR_SPILLS = 6                                      # the lowest count reached; as first written: 53


@pytest.fixture(scope="module")
def table():
    if os.environ.get("ES_BUILD_ALL_SHAPES") == "1" or os.environ.get("ES_BUILD_EXTRA_FLAGS"):
        pytest.skip("measuring build")
    from eigensolver_amd import build
    build.build()
    import codeobj_table
    return codeobj_table.table("cyltjet_")


def test_kernels_present_once(table):
    objs = {}
    for r in table:
        objs.setdefault(r["kernel"], []).append(os.path.basename(r["object"]))
    assert objs == {k: ["es_cylt_complex_slopes.o"] for k in KERNELS}


@pytest.mark.parametrize("k", KERNELS)
def test_spills_registers_and_lds(table, k):
    r = {row["kernel"]: row for row in table}[k]
    fig = (r[".vgpr_count"], r.get(".agpr_count", 0), r.get(".vgpr_spill_count", 0), r.get(".sgpr_spill_count", 0),
           r.get(".private_segment_fixed_size", 0), r.get(".group_segment_fixed_size", 0))
    print(k, "VGPRs, AGPRs, spilled VGPRs, spilled SGPRs, scratch B/lane, LDS B:", fig)
    assert r.get(".vgpr_spill_count", 0) == 0 and r.get(".private_segment_fixed_size", 0) == 0, (k, fig)
    assert r[".vgpr_count"] <= 512, (k, fig)
    assert r.get(".max_flat_workgroup_size") == 64, k
    lds = r.get(".group_segment_fixed_size", 0)
    if k == "cyltjet_slopes_kernel":
        assert lds == CHUNK_LDS == 41120, (k, fig)
        assert r.get(".sgpr_spill_count", 0) == 0, (k, fig)
    else:
        assert CHUNK_LDS < lds <= CHUNK_LDS + 512, (k, fig)             # the vote words of cx_newton_lane on top
        assert r.get(".sgpr_spill_count", 0) <= NEWTON_SGPR_SPILLS <= 53, (k, fig)


def test_neighbouring_filters_keep_their_kernels(table):
    """The new kernels carry neither `cyltc_` nor `cyljet_` in their names: those filters find what they found before."""
    import codeobj_table
    assert sorted(r["kernel"] for r in codeobj_table.table("cyltc_")) == ["cyltc_eval_kernel", "cyltc_refine_kernel"]
    assert sorted(r["kernel"] for r in codeobj_table.table("cyljet_")) == ["cyljet_newton_kernel", "cyljet_slopes_kernel"]
