"""CPU-side checks of the code objects of the complex-frequency kernels (no GPU needed, as
tests/test_refine_hybrid_codeobj.py).  They all run one text, es_complex_shared.hpp, at the scalars esb::cz, esb::CJet<1> and
esb::CJet<2>: no spilled VGPRs and no private segment in any kernel that marches, one wave per SIMD's worth of registers at the
most for the slope and Newton kernels at __launch_bounds__(64), the LDS of one staged chunk, and every kernel still there under
its name.
Metadata only (tools/codeobj_table.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="ROCm LLVM tools not present")

NEW = ("cx_newton_kernel", "cx_slopes_kernel")
VALUE_PATH = ("cx_eigen_exterior_kernel", "cx_eigen_interior_kernel", "cx_emit_kernel", "cx_eval_kernel", "cx_flag_kernel",
              "cx_refine_kernel")
MARCHING_VALUE = ("cx_eval_kernel", "cx_refine_kernel", "cx_eigen_interior_kernel")   # the esb::cz instances
CHUNK_LDS = 3 * (2 * 128 + 1) * 8                           # U, U', U'' at the nodes and mid-points of 128 steps


@pytest.fixture(scope="module")
def rows():
    if os.environ.get("ES_BUILD_ALL_SHAPES") == "1" or os.environ.get("ES_BUILD_EXTRA_FLAGS"):
        pytest.skip("measuring build")
    from eigensolver_amd import build
    build.build()
    import codeobj_table
    return {r["kernel"]: r for r in codeobj_table.table("cx_")}


def test_kernels_present(rows):
    assert sorted(rows) == sorted(NEW + VALUE_PATH)


def test_no_spill_and_no_private_segment(rows):
    for k in NEW + MARCHING_VALUE:
        r = rows[k]
        fig = (r[".vgpr_count"], r.get(".agpr_count", 0), r.get(".vgpr_spill_count", 0), r.get(".private_segment_fixed_size", 0),
               r.get(".group_segment_fixed_size", 0))
        print(k, "VGPRs, AGPRs, spilled VGPRs, scratch B/lane, LDS B:", fig)
        assert r.get(".vgpr_spill_count", 0) == 0 and r.get(".private_segment_fixed_size", 0) == 0, (k, fig)
        if k in NEW:
            assert r[".vgpr_count"] <= 512, (k, fig)
            assert r.get(".max_flat_workgroup_size", 64) == 64, k
    for k in MARCHING_VALUE + ("cx_slopes_kernel",):
        assert rows[k].get(".group_segment_fixed_size", 0) == CHUNK_LDS, k
    # the staged chunk plus the words of the workgroup vote that ends the Newton loop
    assert CHUNK_LDS <= rows["cx_newton_kernel"][".group_segment_fixed_size"] <= CHUNK_LDS + 512
