"""CPU-side checks of the code objects of the section-16 kernels (eigenfunctions and perturbation fields of complex cylinder
roots; no GPU needed, in the manner of tests/test_cyl_complex_codeobj.py): the kernels are there under their names, none spills
a VGPR or has a private segment, the interior kernel holds the LDS of one staged chunk of the untwisted cylinder's base table
and the others none, and the synthesis kernel -- 7 x 4 complex amplitudes per lane -- keeps to the registers of one wave per
SIMD.  The figures are printed.  Metadata only (tools/codeobj_table.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="ROCm LLVM tools not present")

KERNELS = {"cyleig_interior_kernel": "es_cyl_complex_eigen.o", "cyleig_exterior_kernel": "es_cyl_complex_eigen.o",
           "cyleig_polarisation_kernel": "es_cyl_complex_fields.o", "cyleig_field_synthesis_kernel<false>": "es_cyl_complex_fields.o",
           "cyleig_field_synthesis_kernel<true>": "es_cyl_complex_fields.o"}
CHUNK_LDS = 7 * (2 * 128 + 1) * 8                           # the seven base fields at the nodes and mid-points of 128 steps


@pytest.fixture(scope="module")
def rows():
    if os.environ.get("ES_BUILD_ALL_SHAPES") == "1" or os.environ.get("ES_BUILD_EXTRA_FLAGS"):
        pytest.skip("measuring build")
    from eigensolver_amd import build
    build.build()
    import codeobj_table
    return {r["kernel"]: r for r in codeobj_table.table("cyleig_")}


def test_kernels_present(rows):
    assert {k: r["object"] for k, r in rows.items()} == KERNELS


def test_no_spill_no_private_segment_one_chunk_of_lds(rows):
    for k in KERNELS:
        r = rows[k]
        fig = (r[".vgpr_count"], r.get(".agpr_count", 0), r.get(".vgpr_spill_count", 0), r.get(".sgpr_spill_count", 0),
               r.get(".private_segment_fixed_size", 0), r.get(".group_segment_fixed_size", 0))
        print(k, "VGPRs, AGPRs, spilled VGPRs, spilled SGPRs, scratch B/lane, LDS B:", fig)
        assert r.get(".vgpr_spill_count", 0) == 0 and r.get(".private_segment_fixed_size", 0) == 0, (k, fig)
        assert r.get(".group_segment_fixed_size", 0) == (CHUNK_LDS if k == "cyleig_interior_kernel" else 0), (k, fig)
    assert rows["cyleig_interior_kernel"].get(".max_flat_workgroup_size", 64) == 64
    for k in ("cyleig_field_synthesis_kernel<false>", "cyleig_field_synthesis_kernel<true>"):
        assert rows[k].get(".max_flat_workgroup_size", 64) == 64
        assert 112 <= rows[k][".vgpr_count"] + rows[k].get(".agpr_count", 0) <= 512      # the amplitudes alone are 112


def test_field_points_kernel_is_shared_not_copied(rows):
    """field_points_kernel and field_tables_kernel are one text (es_cyl_field_text.hpp) compiled into both field objects; the
    real kernels of section 7 keep their names."""
    import codeobj_table
    objs = {}
    for r in codeobj_table.table("^(field_points_kernel|field_tables_kernel|polarisation_kernel|field_synthesis_kernel)"):
        objs.setdefault(r["kernel"].split("<")[0], set()).add(r["object"])
    assert objs == {"field_points_kernel": {"es_fields.o", "es_cyl_complex_fields.o"},
                    "field_tables_kernel": {"es_fields.o", "es_cyl_complex_fields.o"},
                    "polarisation_kernel": {"es_fields.o"}, "field_synthesis_kernel": {"es_fields.o"}}
