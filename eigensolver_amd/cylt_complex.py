"""Complex frequencies on the twisted (rotating) cylinder (C ABI sections 17 and 18 of include/eigensolver_amd.h): the
determinant of the shooting path at omega = omega_r + i omega_i on (k, Re omega, Im omega) grids and point lists, and the root
search -- the unstable (Kelvin-Helmholtz) modes of a tube with azimuthal shear, which rotates fast enough or is perturbed at
high enough m, where the root leaves the real axis and ShootProblem.find_roots / trace_branches report nothing.

For equilibrium.CylinderRotation (any equilibrium whose `twisted` is true), azimuthal order m >= 0, "kink" and "sausage" axis
conditions.  Arguments, shapes and return conventions are those of cyl_complex.CylinderComplex, whose plumbing this class
shares (cyl_complex.CylinderEvaluation, complex_flow.ComplexTracing).  Section 18 adds the exact slopes D_w, D_k of a root,
Newton's iteration and `densify`, which turns a few unstable_roots rows into the growth-rate curve that
postprocess.most_unstable reads.  Eigenfunctions and fields of the twisted family at complex frequency are not offered.
DESIGN.md sections 8l and 8m.
"""
from .complex_flow import ComplexTracing
from .cyl_complex import CylinderEvaluation


class RotatingCylinderComplex(CylinderEvaluation, ComplexTracing):
    """D_c(k, omega) of one twisted cylinder equilibrium at complex omega: problem(mode, m), close, eval_grid, eval_points(...,
    parts=False), find_roots and unstable_roots as CylinderComplex has them, and through ComplexTracing the slopes and the
    Newton tracing of section 18 -- root_slopes(mode, k, w, count=None, m=None), group_velocity(mode, roots, count=None,
    m=None), newton(mode, k, w0, ..., m=None) and densify(mode, k, w, k_fine, shift_factor=4.0, m=None, **newton_kw)."""
    _SELECT = ("m",)
    _PREFIX = "es_cylt_complex_"

    def __init__(self, equilibrium, ctx=None):
        if not getattr(equilibrium, "twisted", False):
            raise TypeError("RotatingCylinderComplex takes a twisted cylinder equilibrium (CylinderRotation)")
        self._init(equilibrium, ctx)
