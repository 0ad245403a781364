"""CPU-side checks of the code objects of es_curvature.hip (no GPU needed; the pattern of tests/test_root_newton_codeobj.py):
root_curvature_kernel and cg_extremum_kernel are there for all four families, with no spilled VGPR, no private segment and
no LDS, 64-lane workgroups, and inside the 512 registers of one wave per SIMD.  The metadata's .vgpr_count is the size of
the unified register file the kernel asks for, accumulation registers included (the assembler's TotalNumVgprs); .agpr_count
is the part of it beyond the architectural VGPRs.  Metadata only (tools/codeobj_table.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="ROCm LLVM tools not present")

FAMILIES = (0, 1, 2, 3)
KERNELS = ("root_curvature_kernel", "cg_extremum_kernel")


@pytest.fixture(scope="module")
def rows():
    if os.environ.get("ES_BUILD_ALL_SHAPES") == "1" or os.environ.get("ES_BUILD_EXTRA_FLAGS"):
        pytest.skip("measuring build")
    from eigensolver_amd import build
    build.build()
    import codeobj_table
    return {r["kernel"]: r for p in KERNELS for r in codeobj_table.table(p)}


def test_kernels_present(rows):
    assert sorted(rows) == sorted(f"{k}<{f}>" for k in KERNELS for f in FAMILIES)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spill_no_private_segment_no_lds(rows, kernel):
    for f in FAMILIES:
        r = rows[f"{kernel}<{f}>"]
        fig = (r[".vgpr_count"], r.get(".agpr_count", 0), r.get(".vgpr_spill_count", 0), r.get(".private_segment_fixed_size", 0),
               r.get(".group_segment_fixed_size", 0))
        print(f"{kernel}<{f}>", "registers, of them AGPRs, spilled VGPRs, scratch B/lane, LDS B:", fig)
        assert r.get(".vgpr_spill_count", 0) == 0 and r.get(".private_segment_fixed_size", 0) == 0, (kernel, f, fig)
        assert r.get(".group_segment_fixed_size", 0) == 0, (kernel, f, fig)
        assert r.get(".agpr_count", 0) <= r[".vgpr_count"] <= 512, (kernel, f, fig)
        assert r.get(".max_flat_workgroup_size", 64) == 64, (kernel, f)
