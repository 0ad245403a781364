"""CPU-side checks of the code objects of the slope and Newton kernels of the cylinder's complex path (C ABI section 15; no GPU
needed, in the manner of tests/test_cyl_complex_codeobj.py): both kernels are there under their names, each in one object,
neither spills a VGPR or has a private segment, both keep to the registers of one wave per SIMD at 64 threads per workgroup,
and each holds the LDS of one staged chunk of the untwisted cylinder's base table -- the Newton kernel with the words of the
workgroup vote that ends its loop on top.  The figures are printed.  Metadata only (tools/codeobj_table.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="ROCm LLVM tools not present")

KERNELS = ("cyljet_newton_kernel", "cyljet_slopes_kernel")
CHUNK_LDS = 7 * (2 * 128 + 1) * 8                           # the seven base fields at the nodes and mid-points of 128 steps


@pytest.fixture(scope="module")
def table():
    if os.environ.get("ES_BUILD_ALL_SHAPES") == "1" or os.environ.get("ES_BUILD_EXTRA_FLAGS"):
        pytest.skip("measuring build")
    from eigensolver_amd import build
    build.build()
    import codeobj_table
    return codeobj_table.table("cyljet_")


def test_kernels_present_once(table):
    objs = {}
    for r in table:
        objs.setdefault(r["kernel"], []).append(os.path.basename(r["object"]))
    assert objs == {k: ["es_cyl_complex_slopes.o"] for k in KERNELS}


def test_no_spill_and_no_private_segment(table):
    rows = {r["kernel"]: r for r in table}
    for k in KERNELS:
        r = rows[k]
        fig = (r[".vgpr_count"], r.get(".agpr_count", 0), r.get(".vgpr_spill_count", 0), r.get(".private_segment_fixed_size", 0),
               r.get(".group_segment_fixed_size", 0))
        print(k, "VGPRs, AGPRs, spilled VGPRs, scratch B/lane, LDS B:", fig)
        assert r.get(".vgpr_spill_count", 0) == 0 and r.get(".private_segment_fixed_size", 0) == 0, (k, fig)
        assert r[".vgpr_count"] <= 512, (k, fig)
        assert r.get(".max_flat_workgroup_size", 64) == 64, k
    assert rows["cyljet_slopes_kernel"].get(".group_segment_fixed_size", 0) == CHUNK_LDS
    assert CHUNK_LDS <= rows["cyljet_newton_kernel"].get(".group_segment_fixed_size", 0) <= CHUNK_LDS + 512
