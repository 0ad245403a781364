"""Complex frequencies on the twisted (rotating) cylinder (C ABI section 17 of include/eigensolver_amd.h): the determinant of
the shooting path at omega = omega_r + i omega_i on (k, Re omega, Im omega) grids and point lists, and the root search -- the
unstable (Kelvin-Helmholtz) modes of a tube with azimuthal shear, which rotates fast enough or is perturbed at high enough m,
where the root leaves the real axis and ShootProblem.find_roots / trace_branches report nothing.

For equilibrium.CylinderRotation (any equilibrium whose `twisted` is true), azimuthal order m >= 0, "kink" and "sausage" axis
conditions.  Arguments, shapes and return conventions are those of cyl_complex.CylinderComplex, whose plumbing this class
shares (cyl_complex.CylinderEvaluation).  Values and roots only: slopes, Newton tracing, eigenfunctions and fields of the
twisted family are not offered.  DESIGN.md section 8l.
"""
from .cyl_complex import CylinderEvaluation


class RotatingCylinderComplex(CylinderEvaluation):
    """D_c(k, omega) of one twisted cylinder equilibrium at complex omega: problem(mode, m), close, eval_grid, eval_points(...,
    parts=False), find_roots and unstable_roots as CylinderComplex has them."""
    _PREFIX = "es_cylt_complex_"

    def __init__(self, equilibrium, ctx=None):
        if not getattr(equilibrium, "twisted", False):
            raise TypeError("RotatingCylinderComplex takes a twisted cylinder equilibrium (CylinderRotation)")
        self._init(equilibrium, ctx)
