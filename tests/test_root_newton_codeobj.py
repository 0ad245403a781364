"""CPU-side checks of the code objects of the real jet kernels (no GPU needed, as tests/test_complex_slopes_codeobj.py):
root_newton_kernel of es_newton.hip marches one text, jet_march of es_jet.hpp, at jet widths 1 and 2 -- three instances per
family -- and root_slopes_kernel of es_slopes.hip now calls the same function.  No spilled VGPR and no private segment in
either, no LDS (nothing is staged), 64-lane workgroups, and every instance still there under its name.
Metadata only (tools/codeobj_table.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="ROCm LLVM tools not present")

FAMILIES = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def rows():
    if os.environ.get("ES_BUILD_ALL_SHAPES") == "1" or os.environ.get("ES_BUILD_EXTRA_FLAGS"):
        pytest.skip("measuring build")
    from eigensolver_amd import build
    build.build()
    import codeobj_table
    return {r["kernel"]: r for p in ("root_newton_kernel", "root_slopes_kernel") for r in codeobj_table.table(p)}


def test_kernels_present(rows):
    assert sorted(rows) == sorted(f"{k}<{f}>" for k in ("root_newton_kernel", "root_slopes_kernel") for f in FAMILIES)


@pytest.mark.parametrize("kernel", ("root_newton_kernel", "root_slopes_kernel"))
def test_no_spill_no_private_segment_no_lds(rows, kernel):
    for f in FAMILIES:
        r = rows[f"{kernel}<{f}>"]
        fig = (r[".vgpr_count"], r.get(".agpr_count", 0), r.get(".vgpr_spill_count", 0), r.get(".private_segment_fixed_size", 0),
               r.get(".group_segment_fixed_size", 0))
        print(f"{kernel}<{f}>", "VGPRs, AGPRs, spilled VGPRs, scratch B/lane, LDS B:", fig)
        assert r.get(".vgpr_spill_count", 0) == 0 and r.get(".private_segment_fixed_size", 0) == 0, (kernel, f, fig)
        assert r.get(".group_segment_fixed_size", 0) == 0, (kernel, f, fig)
        assert r[".vgpr_count"] + r.get(".agpr_count", 0) <= 512, (kernel, f, fig)
        assert r.get(".max_flat_workgroup_size", 64) == 64, (kernel, f)
