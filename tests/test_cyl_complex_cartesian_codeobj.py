"""Code-object checks of section 20 (Cartesian sampling of unstable cylinder modes; no GPU needed, in the manner of
tests/test_cylt_complex_eigen_codeobj.py).  Metadata only (tools/codeobj_table.py).

The synthesis kernel keeps the 2 x 10 complex coefficient sets of a lane's four points in registers.  It must spill no
vector register, have no private segment, run workgroups of 64, and stay within 256 VGPRs + AGPRs, so that two waves per
SIMD stay resident (floor(512 / allocation)).  The new kernels are in the new object only, and the kernels of section 8 and
section 16 are where they were.  The figures are printed.  As built: cylcart_synthesis_kernel 182 VGPRs in all four
instantiations, no AGPR, nothing spilled, vector or scalar; cylcart_vorticity_amplitudes_kernel 60 VGPRs."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

needs_llvm = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="ROCm LLVM tools not present")

OBJECT = "es_cyl_complex_cartesian.o"
SYNTHESIS = [f"cylcart_synthesis_kernel<{s},{w}>" for s in ("false", "true") for w in ("false", "true")]
AMPLITUDES = "cylcart_vorticity_amplitudes_kernel"


@pytest.fixture(scope="module")
def rows():
    if os.environ.get("ES_BUILD_ALL_SHAPES") == "1" or os.environ.get("ES_BUILD_EXTRA_FLAGS"):
        pytest.skip("measuring build")
    from eigensolver_amd import build
    build.build()
    import codeobj_table
    return codeobj_table.table("cylcart_")


def _figures(r):
    return (r[".vgpr_count"], r.get(".agpr_count", 0), r.get(".vgpr_spill_count", 0), r.get(".sgpr_spill_count", 0),
            r.get(".sgpr_count", 0), r.get(".private_segment_fixed_size", 0), r.get(".group_segment_fixed_size", 0))


@needs_llvm
def test_the_new_kernels_are_in_the_new_object_only(rows):
    assert [(r["kernel"], r["object"]) for r in rows] == [(k, OBJECT) for k in SYNTHESIS + [AMPLITUDES]]


@needs_llvm
def test_no_spill_no_scratch_and_two_waves_per_simd(rows):
    assert sorted(r["kernel"] for r in rows) == sorted(SYNTHESIS + [AMPLITUDES])
    for r in rows:
        fig = _figures(r)
        print(r["kernel"], "VGPRs, AGPRs, spilled VGPRs, spilled SGPRs, SGPRs, scratch B/lane, LDS B:", fig)
        assert r.get(".vgpr_spill_count", 0) == 0 and r.get(".private_segment_fixed_size", 0) == 0, fig
        assert r[".vgpr_count"] + r.get(".agpr_count", 0) <= 256, fig
        if r["kernel"] in SYNTHESIS:
            assert r.get(".max_flat_workgroup_size") == 64, fig


@needs_llvm
def test_the_kernels_of_sections_8_and_16_stay_where_they_were(rows):
    import codeobj_table
    old = codeobj_table.table("^cartesian_synthesis_kernel|^vorticity_amplitudes_kernel|^cyleig_field_synthesis_kernel")
    assert sorted({(r["kernel"].split("<")[0], r["object"]) for r in old}) == [
        ("cartesian_synthesis_kernel", "es_cartesian.o"), ("cyleig_field_synthesis_kernel", "es_cyl_complex_fields.o"),
        ("vorticity_amplitudes_kernel", "es_cartesian.o")]
