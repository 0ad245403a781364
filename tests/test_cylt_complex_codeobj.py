"""CPU-side checks of the code objects of the complex-frequency kernels of the twisted cylinder (C ABI section 17; no GPU
needed, in the manner of tests/test_cyl_complex_codeobj.py): both kernels are there under their names, neither spills a
register -- vector or scalar -- or has a private segment, each holds the LDS of one staged chunk of the twisted family's
20-field base table, the workgroup sizes are 256 and 64, and both keep to the 512 registers a lane has at one wave per SIMD.
The figures are printed.  Metadata only (tools/codeobj_table.py).

As built: cyltc_eval_kernel 164 VGPRs; cyltc_refine_kernel 264 VGPRs + 8 AGPRs; nothing spilled in either, no private segment.
The refinement kernel holds four inlined copies of the evaluation (cx_refine_candidate calls it at four places) and spilled 61
scalar registers to vector lanes as first written; es_cylt_complex.hip and DESIGN.md section 8l say what brought that to none."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="ROCm LLVM tools not present")

KERNELS = ("cyltc_eval_kernel", "cyltc_refine_kernel")
CHUNK_LDS = 20 * (2 * 128 + 1) * 8                          # the 20 base fields at the nodes and mid-points of 128 steps: 41 120 B


@pytest.fixture(scope="module")
def rows():
    if os.environ.get("ES_BUILD_ALL_SHAPES") == "1" or os.environ.get("ES_BUILD_EXTRA_FLAGS"):
        pytest.skip("measuring build")
    from eigensolver_amd import build
    build.build()
    import codeobj_table
    return {r["kernel"]: r for r in codeobj_table.table("cyltc_")}


def test_kernels_present(rows):
    assert sorted(rows) == sorted(KERNELS)
    assert {r["object"] for r in rows.values()} == {"es_cylt_complex.o"}


@pytest.mark.parametrize("k", KERNELS)
def test_no_spill_and_no_private_segment(rows, k):
    r = rows[k]
    fig = (r[".vgpr_count"], r.get(".agpr_count", 0), r.get(".vgpr_spill_count", 0), r.get(".sgpr_spill_count", 0),
           r.get(".private_segment_fixed_size", 0), r.get(".group_segment_fixed_size", 0))
    print(k, "VGPRs, AGPRs, spilled VGPRs, spilled SGPRs, scratch B/lane, LDS B:", fig)
    assert r.get(".private_segment_fixed_size", 0) == 0, (k, fig)
    assert r.get(".group_segment_fixed_size", 0) == CHUNK_LDS == 41120, (k, fig)
    assert r[".vgpr_count"] <= 512, (k, fig)
    assert r.get(".max_flat_workgroup_size") == {"cyltc_eval_kernel": 256, "cyltc_refine_kernel": 64}[k]
    assert r.get(".vgpr_spill_count", 0) == 0 and r.get(".sgpr_spill_count", 0) == 0, (k, fig)


def test_search_kernels_are_still_one_instance(rows):
    """The flag and emit kernels serve every geometry from es_complex.hip: no further copy in the twisted cylinder's object."""
    import codeobj_table
    objs = {}
    for r in codeobj_table.table("cx_(flag|emit)_kernel"):
        objs.setdefault(r["kernel"], []).append(os.path.basename(r["object"]))
    assert objs == {"cx_flag_kernel": ["es_complex.o"], "cx_emit_kernel": ["es_complex.o"]}
