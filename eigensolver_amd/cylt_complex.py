"""Complex frequencies on the twisted (rotating) cylinder (C ABI sections 17, 18 and 19 of include/eigensolver_amd.h): the
determinant of the shooting path at omega = omega_r + i omega_i on (k, Re omega, Im omega) grids and point lists, and the root
search -- the unstable (Kelvin-Helmholtz) modes of a tube with azimuthal shear, which rotates fast enough or is perturbed at
high enough m, where the root leaves the real axis and ShootProblem.find_roots / trace_branches report nothing.

For equilibrium.CylinderRotation (any equilibrium whose `twisted` is true), azimuthal order m >= 0, "kink" and "sausage" axis
conditions.  Arguments, shapes and return conventions are those of cyl_complex.CylinderComplex, whose plumbing this class
shares (cyl_complex.CylinderEvaluation, cyl_complex.CylinderEigenfunctions, complex_flow.ComplexTracing).  Section 18 adds the
exact slopes D_w, D_k of a root, Newton's iteration and `densify`, which turns a few unstable_roots rows into the growth-rate
curve that postprocess.most_unstable reads.  Section 19 adds what the mode looks like: `eigenfunction` (P and xi_r at complex
roots, es_cylt_complex_eigenfunction), `polarisation` (the seven complex amplitudes, here with B_phi and v_phi in them) and
`fields` (growing float32 frames ready for postprocess.write_vtk_frames).  DESIGN.md sections 8l, 8m and 8n.
"""
from .complex_flow import ComplexTracing
from .cyl_complex import CylinderEigenfunctions, CylinderEvaluation


class RotatingCylinderComplex(CylinderEvaluation, CylinderEigenfunctions, ComplexTracing):
    """D_c(k, omega) of one twisted cylinder equilibrium at complex omega: problem(mode, m), close, eval_grid, eval_points(...,
    parts=False), find_roots and unstable_roots as CylinderComplex has them, through ComplexTracing the slopes and the
    Newton tracing of section 18 -- root_slopes(mode, k, w, count=None, m=None), group_velocity(mode, roots, count=None,
    m=None), newton(mode, k, w0, ..., m=None) and densify(mode, k, w, k_fine, shift_factor=4.0, m=None, **newton_kw) --, and
    through CylinderEigenfunctions eigenfunction, polarisation, field_synthesis and fields of section 19 and
    vorticity_amplitudes, cartesian_synthesis and cartesian_fields of section 20, with the arguments and return dicts of
    CylinderComplex."""
    _SELECT = ("m",)
    _PREFIX = "es_cylt_complex_"

    def __init__(self, equilibrium, ctx=None):
        if not getattr(equilibrium, "twisted", False):
            raise TypeError("RotatingCylinderComplex takes a twisted cylinder equilibrium (CylinderRotation)")
        self._init(equilibrium, ctx)
