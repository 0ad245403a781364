"""The change of units, written once (helper of test_unit_scaling_cpu.py / test_unit_scaling_gpu.py; no tests in here).

Every dimensional input is multiplied by an exact power of two: speeds by V = 2^pv, densities by R = 4^pr (so that
sqrt(R) = 2^pr is exact as well), lengths and wavenumbers not at all.  An output of dimension speed^a density^b must then
come out multiplied by V^a R^b = 2^(a pv + 2 b pr) with every mantissa bit unchanged: a power of two commutes with every
IEEE rounding, with v_rcp_f64, with the square root of an even power and with exp / Bessel functions of dimensionless
arguments, as long as nothing overflows or goes subnormal.  LAW holds the exponents (a, b), from dimensional analysis:

  cylinders  the determinant is xi_r per unit total pressure at the boundary, 1 / (rho v^2)              -> (-2, -1)
  slabs      the determinant is P_T per unit v_x at the boundary, rho v^2 / v                            -> ( 1,  1)
  d/d omega  takes one speed off, d/dk none (k is not rescaled); frequencies and group speeds are speeds -> ( 1,  0)
  rel, resid, statuses, flags, rows, node counts and iteration counts do not change.

The one formula of the project that is not homogeneous is the flow slab with shear (ES_GEOM_SLAB_FLOW with dU != 0, and
its complex twin): the reference's D(x), flow_multiprocessor_coronal.py:423, adds Omega^2 - k^2 cT^2 (a speed squared)
to k^4 cT^2 c^2 / ((c^2 + vA^2)(Omega^2 - k^2 cT^2)) (dimensionless in speed), and coef_pre<FAM_SLABF> restates it as
G = S t^2 + k^4 cT^2 c^2.  That family takes part in the density scale only (pv = 0).

Two more formulas of the reference are not homogeneous, both in the axial displacement of es_cyl_polarisation (the export
scripts, Export_vtk.py): the exterior xi_z of :781 carries a factor omega^2 that the interior one has not (its law under
ES_FIELD_REFERENCE is therefore LAW's xi_z_ext_reference), and the interior xi_z of :780 subtracts
(2 Omega v_phi B_phi + f_B v_phi^2) xi_r / r, a speed^3 B, from terms that are a speed B, so that on a rotating tube
(v_phi != 0) the interior xi_z, and v_z with it, follow no law at all.
"""
import numpy as np

from eigensolver_amd import shooting as s
from tests.cases import desc_dict

# ---- (a, b) of every input: value * V^a R^b.  b = 1/2 is the magnetic field, B = vA sqrt(rho). ------------------------
DESC_LAW = {"vA_e": (1, 0), "c_e": (1, 0), "cT_e": (1, 0), "U_e": (1, 0), "c_i": (1, 0), "vA_i": (1, 0),
            "rho_e": (0, 1), "rho_i": (0, 1), "bc_const": (2, 1)}
PROFILE_LAW = {"vz": (1, 0), "vphi": (1, 0), "U": (1, 0), "dU": (1, 0), "ddU": (1, 0), "c2": (2, 0), "vA2": (2, 0),
               "rho": (0, 1), "Bz": (1, 0.5), "Bphi": (1, 0.5), "rdC3": (2, 1), "r": (0, 0)}
UNIFORM_LAW = {"c_i": (1, 0), "vA_i": (1, 0), "U_i": (1, 0), "vA_e": (1, 0), "c_e": (1, 0), "cT_e": (1, 0),
               "rho_i": (0, 1), "rho_e": (0, 1)}
FIELD_PROFILE_LAW = {"r": (0, 0), "rho": (0, 1), "Bz": (1, 0.5), "Bphi": (1, 0.5), "vz": (1, 0), "vphi": (1, 0),
                     "bA": (1, 0), "qc": (0, 0), "q": (0, 0), "s_phi": (1, 0), "s_z": (1, 0)}

# ---- (a, b) of every output, per family ("cyl": ES_GEOM_CYL, ES_GEOM_CYL_TWIST and the closed-form uniform cylinder; "slab")
_COMMON = {"w": (1, 0), "w_lo": (1, 0), "w_hi": (1, 0), "cg": (1, 0), "dwdk": (1, 0), "k": (0, 0), "x": (0, 0),
           "rel": (0, 0), "resid": (0, 0), "value": (0, 0), "peak_value": (0, 0)}
LAW = {
    "cyl": dict(_COMMON, D=(-2, -1), outer=(-2, -1), inner=(-2, -1), D_w=(-3, -1), D_k=(-2, -1), flux=(-2, -1),
                peak_flux=(-2, -1),
                # es_cyl_polarisation, per unit P_T at the boundary: xi = flux, v = -i Omega xi
                xi_r=(-2, -1), xi_phi=(-2, -1), xi_z=(-2, -1), P_T=(0, 0), v_r=(-1, -1), v_phi=(-1, -1), v_z=(-1, -1),
                # ES_FIELD_REFERENCE: the export scripts' exterior xi_z carries a factor omega^2 the interior one does not
                # (Export_vtk.py:781), and v_z = -omega xi_z follows it
                xi_z_ext_reference=(0, -1), v_z_ext_reference=(1, -1)),
    "slab": dict(_COMMON, D=(1, 1), outer=(1, 1), inner=(1, 1), D_w=(0, 1), D_k=(1, 1), flux=(1, 1), peak_flux=(1, 1)),
}
SLOPE_ROWS = ("D", "D_w", "D_k")                    # the rows of RootSlopes.outer / .inner / (d, d_w, d_k)


def family(geometry):
    return "cyl" if int(geometry) in (s.GEOM_CYL, s.GEOM_CYL_TWIST) else "slab"


def shift(a, b, pv, pr):
    """The binary exponent of V^a R^b."""
    e = a * pv + 2 * b * pr
    assert e == int(e)
    return int(e)


def scale_fields(fields, law, pv, pr):
    """dict -> dict with every entry named in `law` multiplied by its power of two (the others as they are)."""
    out = {}
    for name, v in fields.items():
        if name in law and v is not None:
            v = np.ldexp(np.asarray(v, dtype=np.float64), shift(*law[name], pv, pr))
            v = float(v) if v.ndim == 0 else v
        out[name] = v
    return out


def scaled(desc, profiles, pv, pr):
    """The es_shoot_desc fields (dict) and the es_profiles arrays (dict) of make_desc in the units V = 2^pv, R = 4^pr.
    Applied to the finished inputs, never through the equilibrium constructors, whose sqrt and divisions would leave the
    derived constants (cT_e, rho_e) not exactly scaled."""
    unknown = [n for n in profiles if n not in PROFILE_LAW]
    assert not unknown, unknown
    return scale_fields(desc, DESC_LAW, pv, pr), scale_fields(profiles, PROFILE_LAW, pv, pr)


def scale_uniform_params(params, pv, pr):
    """es_cyl_uniform_params (the ctypes struct) scaled in place; returns it."""
    for name, law in UNIFORM_LAW.items():
        setattr(params, name, float(np.ldexp(getattr(params, name), shift(*law, pv, pr))))
    return params


def port_problem(eq, mode, m=None, pv=0, pr=0):
    """The C port on the scaled inputs of (eq, mode, m)."""
    from oracle.port import PortProblem
    d, p = s.make_desc(eq, mode, m)
    return PortProblem(*scaled(desc_dict(d), p, pv, pr))


class ScaledShootProblem(s.ShootProblem):
    """ShootProblem on the scaled inputs of (eq, mode, m): the constructor runs around a make_desc that scales what the
    plain one returns, and the profiles of the polarisation are scaled alike."""

    def __init__(self, eq, mode, m=None, ctx=None, pv=0, pr=0, accept_norm=0):
        self.pv, self.pr = pv, pr
        plain = s.make_desc

        def make_desc(eq, mode, m=None):
            d, prof = plain(eq, mode, m)
            dd, prof = scaled(desc_dict(d), prof, pv, pr)
            for name in DESC_LAW:
                setattr(d, name, dd[name])
            return d, prof

        s.make_desc = make_desc
        try:
            super().__init__(eq, mode, m=m, ctx=ctx, accept_norm=accept_norm)
        finally:
            s.make_desc = plain

    def field_profiles(self, reference_quirks=True):
        return scale_fields(super().field_profiles(reference_quirks), FIELD_PROFILE_LAW, self.pv, self.pr)


def complex_solver(cls, eq, ctx, mode, m=None, pv=0, pr=0, **kw):
    """CylinderComplex / RotatingCylinderComplex / SlabComplexFlow (`cls`) whose problem of (mode, m) holds the scaled
    inputs."""
    from eigensolver_amd.complex_flow import SlabComplexFlow
    if cls is SlabComplexFlow:
        solver = cls(ctx=ctx, equilibrium=eq, **kw)
        solver._problems[mode] = ScaledShootProblem(eq, mode, ctx=ctx, pv=pv, pr=pr)
    else:
        solver = cls(eq, ctx=ctx)
        mm = (1 if mode == "kink" else 0) if m is None else int(m)
        solver._problems[(mode, mm)] = ScaledShootProblem(eq, mode, m=mm, ctx=ctx, pv=pv, pr=pr)
    return solver


def scaled_uniform(eq, mode, m, ctx, pv, pr):
    from eigensolver_amd.cyl_uniform import CylinderUniform
    u = CylinderUniform(eq, mode, m=m, ctx=ctx)
    scale_uniform_params(u.params, pv, pr)
    return u


# ---- the comparison --------------------------------------------------------------------------------------------------
def _host(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    if np.iscomplexobj(a):
        a = np.ascontiguousarray(a, dtype=np.complex128).view(np.float64)
    return np.ascontiguousarray(a, dtype=np.float64)


def assert_scaled(out_ref, out_scaled, a, b, pv, pr, ok=None, what=""):
    """out_scaled == ldexp(out_ref, a pv + 2 b pr) EXACTLY: the float64 bit patterns are equal after the shift, NaNs stand
    in the same places.  Every element is compared; `ok` (bool array, "status is ES_PT_OK in both") is the only mask.
    Complex arrays are compared as their (re, im) pairs."""
    cplx = hasattr(out_ref, "is_complex") and out_ref.is_complex() or np.iscomplexobj(out_ref)
    ref, got = _host(out_ref), _host(out_scaled)
    assert ref.shape == got.shape, (what, ref.shape, got.shape)
    if ok is not None:
        ok = np.asarray(ok.detach().cpu().numpy() if hasattr(ok, "detach") else ok, dtype=bool)
        if cplx:
            ok = np.repeat(ok, 2, axis=-1)
        ok = np.broadcast_to(ok, ref.shape)
        ref, got = ref[ok], got[ok]
    want = np.ldexp(ref, shift(a, b, pv, pr))
    nan_w, nan_g = np.isnan(want), np.isnan(got)
    assert np.array_equal(nan_w, nan_g), f"{what}: NaNs in different places ({nan_w.sum()} expected, {nan_g.sum()} found)"
    bw, bg = want[~nan_w].view(np.int64), got[~nan_g].view(np.int64)
    if not np.array_equal(bw, bg):
        bad = np.flatnonzero(bw != bg)
        i = bad[0]
        raise AssertionError(f"{what}: {bad.size} of {bw.size} values are not the exact 2^{shift(a, b, pv, pr)} multiple; "
                             f"first: expected {want[~nan_w][i]!r}, found {got[~nan_g][i]!r}")


def assert_same(ref, got, what=""):
    """Integer / status arrays: equal everywhere."""
    r = ref.detach().cpu().numpy() if hasattr(ref, "detach") else np.asarray(ref)
    g = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    assert r.shape == g.shape and np.array_equal(r, g), f"{what}: {np.count_nonzero(r != g) if r.shape == g.shape else 'shape'} differ"


ROOT_COLUMNS = (("w", "w"), ("w_lo", "w"), ("w_hi", "w"), ("k", "k"), ("resid", "resid"))


def assert_root_table_scaled(ref, got, pv, pr, fam, what="roots"):
    """A find_roots table (dict, count) obeys LAW: same count, w / w_lo / w_hi times V exactly, k, resid, row, flag equal."""
    (tr, nr), (tg, ng) = ref, got
    assert nr == ng, f"{what}: {nr} brackets at reference units, {ng} at scaled units"
    for col, law in ROOT_COLUMNS:
        assert_scaled(tr[col], tg[col], *LAW[fam][law], pv, pr, what=f"{what}.{col}")
    for col in ("row", "flag"):
        assert_same(tr[col], tg[col], f"{what}.{col}")


# ---- the grid of both legs ---------------------------------------------------------------------------------------------
def grid_of(case, nk=6, nw=96):
    """6 k-rows on linspace(0.3, 3.7, 6), 96 phase speeds at the mid-points of the case's window (tests/cases.py)."""
    lo, hi = case[3]
    k = np.linspace(0.3, 3.7, nk)
    W = lo + (hi - lo) * (np.arange(nw) + 0.5) / nw
    return k, W
