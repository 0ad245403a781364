"""CPU-side checks of the code objects of the hybrid refinement (no GPU needed, as tests/test_codeobj.py): the new kernels
have no spilled VGPRs and no private segment, and the section rule's kernels are the instantiations, with the register,
scratch and LDS figures, they had before the hybrid rule existed (tools/codeobj_table.py of that build)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="ROCm LLVM tools not present")

NEW = ("refine_superlinear_kernel<0,3>", "refine_superlinear_kernel<1,2>", "refine_superlinear_kernel<2,2>",
       "refine_superlinear_kernel<3,2>", "hybrid_flag_kernel", "hybrid_gather_kernel", "hybrid_scatter_kernel")
# kernel: (VGPRs, AGPRs, spilled VGPRs, spilled SGPRs, scratch B/lane, LDS B)
SECTION_RULE = {
    "refine_kernel<0,16,0,false,false,2>": (196, 0, 0, 126, 36, 14392),
    "refine_kernel<0,16,0,true,false,2>": (190, 0, 0, 120, 36, 14392),
    "refine_kernel<0,16,0,true,true,3>": (136, 0, 0, 66, 36, 14392),
    "refine_kernel<0,16,32,true,false,2>": (203, 0, 0, 148, 0, 58240),
    "refine_kernel<0,16,32,true,true,3>": (164, 0, 0, 107, 68, 58240),
    "refine_kernel<0,4,0,false,false,2>": (196, 0, 0, 126, 36, 14392),
    "refine_kernel<0,4,0,true,false,2>": (190, 0, 0, 120, 36, 14392),
    "refine_kernel<0,4,0,true,true,3>": (136, 0, 0, 66, 36, 14392),
    "refine_kernel<0,8,0,false,false,2>": (196, 0, 0, 126, 36, 14392),
    "refine_kernel<0,8,0,true,false,2>": (190, 0, 0, 120, 36, 14392),
    "refine_kernel<0,8,0,true,true,3>": (136, 0, 0, 66, 36, 14392),
    "refine_kernel<1,16,0,false,false,2>": (231, 0, 0, 128, 36, 41120),
    "refine_kernel<1,16,0,true,false,2>": (224, 0, 0, 150, 0, 41120),
    "refine_kernel<1,16,0,true,true,2>": (178, 0, 0, 89, 0, 41120),
    "refine_kernel<1,4,0,false,false,2>": (231, 0, 0, 128, 36, 41120),
    "refine_kernel<1,4,0,true,false,2>": (224, 0, 0, 150, 0, 41120),
    "refine_kernel<1,4,0,true,true,2>": (178, 0, 0, 89, 0, 41120),
    "refine_kernel<1,8,0,false,false,2>": (231, 0, 0, 128, 36, 41120),
    "refine_kernel<1,8,0,true,false,2>": (224, 0, 0, 150, 0, 41120),
    "refine_kernel<1,8,0,true,true,2>": (178, 0, 0, 89, 0, 41120),
    "refine_kernel<2,16,0,false,false,2>": (186, 0, 0, 118, 36, 6168),
    "refine_kernel<2,16,0,true,false,2>": (174, 0, 0, 120, 36, 6168),
    "refine_kernel<2,4,0,false,false,2>": (186, 0, 0, 118, 36, 6168),
    "refine_kernel<2,4,0,true,false,2>": (174, 0, 0, 120, 36, 6168),
    "refine_kernel<2,8,0,false,false,2>": (186, 0, 0, 118, 36, 6168),
    "refine_kernel<2,8,0,true,false,2>": (174, 0, 0, 120, 36, 6168),
    "refine_kernel<3,16,0,false,false,2>": (206, 0, 0, 130, 36, 6168),
    "refine_kernel<3,16,0,true,false,2>": (181, 0, 0, 151, 0, 6168),
    "refine_kernel<3,4,0,false,false,2>": (206, 0, 0, 130, 36, 6168),
    "refine_kernel<3,4,0,true,false,2>": (181, 0, 0, 151, 0, 6168),
    "refine_kernel<3,8,0,false,false,2>": (206, 0, 0, 130, 36, 6168),
    "refine_kernel<3,8,0,true,false,2>": (181, 0, 0, 151, 0, 6168),
    "refine_polish_kernel<0,false,2>": (191, 0, 0, 150, 0, 14392),
    "refine_polish_kernel<0,true,3>": (148, 0, 0, 106, 0, 14392),
    "refine_polish_kernel<1,false,2>": (225, 0, 0, 142, 0, 41120),
    "refine_polish_kernel<1,true,2>": (183, 0, 0, 112, 0, 41120),
    "refine_polish_kernel<2,false,2>": (181, 0, 0, 155, 0, 6168),
    "refine_polish_kernel<3,false,2>": (200, 0, 0, 157, 0, 6168),
}


@pytest.fixture(scope="module")
def rows():
    if os.environ.get("ES_BUILD_ALL_SHAPES") == "1" or os.environ.get("ES_BUILD_EXTRA_FLAGS"):
        pytest.skip("measuring build")
    from eigensolver_amd import build
    build.build()
    import codeobj_table
    return {r["kernel"]: r for r in codeobj_table.table("refine|hybrid")}


def _figures(r):
    return (r[".vgpr_count"], r.get(".agpr_count", 0), r.get(".vgpr_spill_count", 0), r.get(".sgpr_spill_count", 0),
            r.get(".private_segment_fixed_size", 0), r.get(".group_segment_fixed_size", 0))


def test_new_kernels_have_no_spill_and_no_private_segment(rows):
    new = {k: r for k, r in rows.items() if k.startswith(("refine_superlinear_kernel", "hybrid_"))}
    assert sorted(new) == sorted(NEW)
    for k, r in new.items():
        assert r.get(".vgpr_spill_count", 0) == 0 and r.get(".private_segment_fixed_size", 0) == 0, (k, _figures(r))
        assert r.get(".agpr_count", 0) == 0, k
    # occupancy of the polish kernel of the same family: three waves per SIMD (<= 168 VGPRs) for the untwisted cylinder, two
    # (<= 256) for the others
    assert new["refine_superlinear_kernel<0,3>"][".vgpr_count"] <= 168
    for k in NEW[1:4]:
        assert new[k][".vgpr_count"] <= 256, k
    assert not any(k.startswith("shoot_grid") for k in new)


def test_section_rule_kernels_are_unchanged(rows):
    old = {k: _figures(r) for k, r in rows.items() if k.startswith(("refine_kernel<", "refine_polish_kernel<"))}
    assert sorted(old) == sorted(SECTION_RULE), sorted(set(old) ^ set(SECTION_RULE))
    for k, v in SECTION_RULE.items():
        assert old[k] == v, (k, old[k], v)
