"""ctypes binding of libeigensolver_amd.so (the C ABI declared in include/eigensolver_amd.h).

The library is GPU-only.  Loading fails loudly when the shared object is missing -- there is no Python or
CPU fallback for any entry point.
"""
import ctypes as C
import os
from typing import NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libeigensolver_amd.so")


class SlabAnalyticParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in
                ("vA_i", "c_i", "vA_e", "c_e", "mach_i", "mach_e", "R1", "cT_i", "cT_e")]


class EsError(RuntimeError):
    pass


# refinement rule of a context (enum of include/eigensolver_amd.h; Context.refine_rule)
REFINE_SECTION, REFINE_HYBRID = 0, 1


class RefineStats(NamedTuple):
    """es_context_refine_stats: counts of the ES_REFINE_HYBRID searches since the last read."""
    brackets: int       # refined by the hybrid rule (more section rounds than the rule takes before its one-lane phase)
    kept: int           # kept by the one-lane phase
    fallback: int       # refined by the remaining section rounds and the polish steps
    evaluations: int    # determinant evaluations of the one-lane phase


# es_shoot_audit_screening: status bit of a point the fp32 screening does not vouch for, kind bits of a flagged cell
PT_SCREEN_UNSURE = 0x80
AUDIT_MISSED, AUDIT_FALSE, AUDIT_STATUS, AUDIT_SIGN = 1, 2, 4, 8
ERR_SCREENING = 7


class ScreenAudit(NamedTuple):
    """es_shoot_audit_screening read on the host (include/eigensolver_amd.h has the definitions).  Rows are indices into
    the caller's full grid, also when only a sample of rows was audited."""
    flagged: int        # cells with any kind bit (may exceed the table capacity)
    missed: int         # fp64 brackets the merged grid does not have
    false: int          # brackets of the merged grid that are not fp64 brackets
    status: int         # vouched-for points whose status differs from the fp64 status
    sign: int           # vouched-for points, both statuses OK, with the wrong sign
    vouched_ok: int     # points vouched for with both statuses OK
    unsure: int         # points sent back to fp64
    brackets64: int     # fp64 brackets
    min_margin: float   # least |D64| / |D_scr - D64| over the compared points (+inf: none)
    min_margin_at: object   # its (row, col), or None
    max_err: float      # largest fp32 error in units of max(|outer|, |inner|) (0: none)
    max_err_at: object      # its (row, col), or None
    row: object         # NumPy arrays: the first min(flagged, capacity) flagged cells in grid order ...
    col: object
    kind: object        # ... and their kind bits (AUDIT_*)

    @property
    def ok(self):
        """The screening lost nothing: no missed or false bracket and no wrong status."""
        return self.missed == 0 and self.false == 0 and self.status == 0


def check_audit(report):
    """Raise EsError, with the status string of ES_ERR_SCREENING and the first reported cell, unless report.ok."""
    if report.ok:
        return report
    msg = load().es_status_string(ERR_SCREENING).decode()
    first = (f"; first reported cell (row {int(report.row[0])}, col {int(report.col[0])}), kind {int(report.kind[0])}"
             if len(report.row) else "")
    raise EsError(f"libeigensolver_amd: {msg} (fp32 screening audit: {report.missed} missed and {report.false} false "
                  f"bracket(s), {report.status} wrong status(es){first})")


_lib = None


def load():
    """Load the shared library (once).  Raises EsError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EsError(f"{LIB_PATH} not found: build it with `python -m eigensolver_amd.build` "
                          "(hipcc, --offload-arch=gfx950). There is no CPU fallback.")
        # Device memory and streams come from torch, and the torch wheel carries its own HIP runtime: it has to be
        # the first one in the process (loading this library before torch leaves two runtimes, and the second one
        # finds no device).
        import torch  # noqa: F401
        _lib = _sig(C.CDLL(LIB_PATH))
    return _lib


def load_variant(path):
    """A second build of the library (tests only: lib/libeigensolver_amd_ieee.so, -DES_IEEE_DIVISION) with the same
    signatures; ctypes keeps the symbols of each handle apart."""
    import torch  # noqa: F401
    if not os.path.exists(path):
        raise EsError(f"{path} not found: build it with `python -m eigensolver_amd.build`")
    return _sig(C.CDLL(path))


def check(ctx, status, allow_capacity=False):
    if status == 0 or (allow_capacity and status == 3):
        return status
    lib = load()
    msg = lib.es_status_string(status).decode()
    detail = lib.es_last_error(ctx).decode() if ctx else ""
    raise EsError(f"libeigensolver_amd: {msg}" + (f" ({detail})" if detail else ""))


class Context:
    """Owns an es_context bound to a HIP device and (optionally) a torch stream."""

    def __init__(self, device=0, stream=None, lib=None):
        import torch
        if not torch.cuda.is_available():
            raise EsError("no HIP device visible: eigensolver_amd has no CPU path")
        self.lib = lib if lib is not None else load()
        self.device = int(device)
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        self.torch_stream = stream
        h = C.c_void_p()
        st = self.lib.es_context_create(self.device, C.c_void_p(stream.cuda_stream), C.byref(h))
        if st != 0:
            raise EsError("es_context_create: " + self.lib.es_status_string(st).decode())
        self.handle = h

    def synchronize(self):
        check(self.handle, self.lib.es_context_synchronize(self.handle))

    def grid_timer(self, enable=True):
        """HIP events around every grid-march launch of this context (es_context_grid_timer)."""
        check(self.handle, self.lib.es_context_grid_timer(self.handle, 1 if enable else 0))

    def grid_time(self):
        """(summed ms, launches) of the grid-march kernels since the last call; synchronises the stream."""
        ms, n = C.c_double(0.0), C.c_int(0)
        check(self.handle, self.lib.es_context_grid_time(self.handle, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    @property
    def refine_rule(self):
        """REFINE_SECTION (default) or REFINE_HYBRID: how every root search of this context refines its brackets."""
        r = C.c_int(0)
        check(self.handle, self.lib.es_context_get_refine_rule(self.handle, C.byref(r)))
        return r.value

    @refine_rule.setter
    def refine_rule(self, rule):
        check(self.handle, self.lib.es_context_set_refine_rule(self.handle, int(rule)))

    def refine_stats(self):
        """RefineStats of the hybrid searches since the last call; synchronises the stream and zeroes the counts."""
        h = (C.c_int64 * 4)()
        check(self.handle, self.lib.es_context_refine_stats(self.handle, h))
        return RefineStats(*[int(v) for v in h])

    def close(self):
        if getattr(self, "handle", None):
            self.lib.es_context_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ptr(t):
    """Device pointer of a contiguous torch tensor as c_void_p."""
    assert t.is_contiguous()
    return C.c_void_p(t.data_ptr())


# ---- shooting path structs (include/eigensolver_amd.h section 2) ---------------------------------------------
class ShootDesc(C.Structure):
    _fields_ = [("geometry", C.c_int32), ("n_nodes", C.c_int32),
                ("x_boundary", C.c_double), ("x_end", C.c_double),
                ("rho_e", C.c_double), ("vA_e", C.c_double), ("c_e", C.c_double), ("cT_e", C.c_double),
                ("U_e", C.c_double), ("L_factor", C.c_double), ("ic_value", C.c_double), ("ic_slope", C.c_double),
                ("m", C.c_int32), ("m_ext", C.c_int32), ("axis_bc", C.c_int32), ("c1_power", C.c_int32),
                ("bc_const", C.c_double),
                ("slab_mode", C.c_int32), ("accept_norm", C.c_int32),
                ("c_i", C.c_double), ("vA_i", C.c_double), ("rho_i", C.c_double)]


_PROFILE_FIELDS = ("r", "rho", "c2", "vA2", "Bz", "Bphi", "vz", "vphi", "rdC3", "U", "dU", "ddU")


class Profiles(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _PROFILE_FIELDS]


class RootTable(C.Structure):
    _fields_ = [("d_k", C.c_void_p), ("d_w", C.c_void_p), ("d_w_lo", C.c_void_p), ("d_w_hi", C.c_void_p),
                ("d_resid", C.c_void_p), ("d_row", C.c_void_p), ("d_flag", C.c_void_p), ("capacity", C.c_int32)]


class WorkerSpec(C.Structure):
    _fields_ = [("tol_percent", C.c_double), ("min_len", C.c_int32), ("itt_cap", C.c_int32),
                ("reset_loop_ws_each_iter", C.c_int32), ("break_on_accept", C.c_int32),
                ("stale_ext_const", C.c_int32), ("main_double_append", C.c_int32)]


class CylUniformParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("c_i", "vA_i", "rho_i", "U_i", "rho_e", "vA_e", "c_e", "cT_e",
                                           "r_boundary", "r_axis", "L_factor", "ic_value", "ic_slope")] + \
               [("m", C.c_int32), ("m_ext", C.c_int32), ("axis_bc", C.c_int32), ("reserved", C.c_int32)]


class ComplexRootTable(C.Structure):
    _fields_ = [("d_k", C.c_void_p), ("d_w_re", C.c_void_p), ("d_w_im", C.c_void_p), ("d_resid", C.c_void_p),
                ("d_row", C.c_void_p), ("d_flag", C.c_void_p), ("capacity", C.c_int32)]


# ---- perturbation fields (include/eigensolver_amd.h section 7) -------------------------------------------------
_FIELD_PROFILE_FIELDS = ("r", "rho", "Bz", "Bphi", "vz", "vphi", "bA", "qc", "q", "s_phi", "s_z")


class FieldProfiles(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _FIELD_PROFILE_FIELDS]


AMP_NAMES = ("xi_r", "xi_phi", "xi_z", "P_T", "v_r", "v_phi", "v_z")                       # ES_AMP_*
VAR_NAMES = ("xi_r", "xi_phi", "P_T", "v_r", "v_phi", "xi_x", "xi_y", "v_x", "v_y", "v_z", "xi_z")   # ES_VAR_* (mask bits)
FIELD_REFERENCE, FIELD_Z_REFERENCE_ANGLE, FIELD_BIG_ENDIAN = 1, 2, 4
# ---- Cartesian sampling and vorticity (section 8) ----------------------------------------------------------------
VORT_NAMES = ("Wr_C", "Wr_S", "Wphi_C", "Wphi_S", "Wz_C")                                     # ES_VORT_*
CVAR_NAMES = ("P_T", "xi_x", "xi_y", "xi_z", "v_x", "v_y", "v_z", "vort_x", "vort_y", "vort_z")   # ES_CVAR_* (mask bits)
CVORT_NAMES = ("W_r", "W_phi", "W_z")                                                         # ES_CVORT_* (section 20, complex)
# ---- perturbation fields of a slab mode (section 9) --------------------------------------------------------------
_SLAB_FIELD_PROFILE_FIELDS = ("rho", "c2", "vA2", "U", "dU")


class SlabFieldProfiles(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _SLAB_FIELD_PROFILE_FIELDS]


SAMP_NAMES = ("xi_x", "xi_z", "P_T", "v_x", "v_z", "vort_y")                                  # ES_SAMP_* (complex)
SVAR_NAMES = ("xi_x", "xi_z", "P_T", "v_x", "v_z", "vort_y")                                  # ES_SVAR_* (mask bits)
SLAB_MODE_SAUSAGE, SLAB_MODE_KINK = 0, 1
SLAB_FIELD_SHEAR_PT = 1


def _sig(lib):
    """Argument / result types of every entry point of include/eigensolver_amd.h (sections in header order)."""
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    lib.es_abi_version.restype = i
    lib.es_status_string.restype = C.c_char_p
    lib.es_status_string.argtypes = [i]
    lib.es_context_create.argtypes = [i, vp, C.POINTER(vp)]
    lib.es_context_destroy.argtypes = [vp]
    lib.es_last_error.restype = C.c_char_p
    lib.es_last_error.argtypes = [vp]
    lib.es_context_synchronize.argtypes = [vp]
    lib.es_context_grid_timer.argtypes = [vp, i]
    lib.es_context_grid_time.argtypes = [vp, C.POINTER(d), C.POINTER(i)]
    lib.es_context_set_refine_rule.argtypes = [vp, i]
    lib.es_context_get_refine_rule.argtypes = [vp, C.POINTER(i)]
    lib.es_context_refine_stats.argtypes = [vp, C.POINTER(C.c_int64)]
    # (1) closed-form slab
    P = C.POINTER(SlabAnalyticParams)
    lib.es_slab_analytic_eval.argtypes = [vp, P, i, vp, i, vp, i, vp]
    lib.es_slab_analytic_scan.argtypes = [vp, P, i, vp, i, vp, i, d, vp, vp, i, C.POINTER(i)]
    lib.es_slab_analytic_filter.argtypes = [vp, P, i, vp, vp, i, d, vp]
    # (2) shooting determinant, brackets, refinement; (3) worker
    lib.es_problem_create.argtypes = [vp, C.POINTER(ShootDesc), C.POINTER(Profiles), C.POINTER(vp)]
    lib.es_problem_destroy.argtypes = [vp, vp]
    lib.es_shoot_eval_grid.argtypes = [vp, vp, vp, i, vp, i, i, vp, vp, vp]
    lib.es_shoot_eval_grid_ex.argtypes = [vp, vp, vp, i, vp, i, i, i, vp, vp, vp]
    lib.es_shoot_eval_points.argtypes = [vp, vp, vp, vp, i, vp, vp, vp]
    lib.es_shoot_grid_shape.argtypes = [vp, vp, i, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    lib.es_shoot_find_roots.argtypes = [vp, vp, vp, i, vp, i, i, vp, vp, i, d, C.POINTER(RootTable), C.POINTER(i)]
    lib.es_shoot_find_roots_mixed.argtypes = [vp, vp, vp, i, vp, i, i, i, d, vp, vp, C.POINTER(RootTable), C.POINTER(i),
                                              C.POINTER(i)]
    lib.es_shoot_screen_grid.argtypes = [vp, vp, vp, i, vp, i, i, vp, vp]
    lib.es_shoot_find_roots_screened.argtypes = [vp, vp, vp, i, vp, i, i, i, d, vp, vp, C.POINTER(RootTable), C.POINTER(i),
                                                 C.POINTER(i)]
    lib.es_shoot_find_roots_async.argtypes = [vp, vp, vp, i, vp, i, i, vp, vp, i, d, C.POINTER(RootTable), vp]
    lib.es_shoot_find_roots_screened_async.argtypes = [vp, vp, vp, i, vp, i, i, i, d, vp, vp, C.POINTER(RootTable), vp]
    lib.es_shoot_find_roots_mixed_async.argtypes = [vp, vp, vp, i, vp, i, i, i, d, vp, vp, C.POINTER(RootTable), vp]
    lib.es_shoot_audit_screening.argtypes = [vp, i, i, vp, vp, vp, vp, vp, i, vp, vp, vp, vp]
    lib.es_root_table_pack.argtypes = [vp, C.POINTER(RootTable), i, d, vp, i, vp]
    lib.es_root_table_pack_async.argtypes = [vp, C.POINTER(RootTable), vp, d, vp, i, vp]
    lib.es_worker_run.argtypes = [vp, vp, C.POINTER(WorkerSpec), vp, i, vp, i, vp, vp, i, vp]
    # (4) closed-form uniform cylinder; (5) eigenfunctions
    lib.es_cyl_uniform_eval.argtypes = [vp, C.POINTER(CylUniformParams), vp, i, vp, i, i, vp, vp, vp]
    lib.es_cyl_uniform_find_roots.argtypes = [vp, C.POINTER(CylUniformParams), i, i, vp, i, vp, i, i, i, d, vp, vp,
                                              C.POINTER(RootTable), vp, C.POINTER(i)]
    lib.es_cyl_uniform_find_roots_async.argtypes = [vp, C.POINTER(CylUniformParams), i, i, vp, i, vp, i, i, i, d, vp, vp,
                                                    C.POINTER(RootTable), vp, vp]
    lib.es_shoot_eigenfunction.argtypes = [vp, vp, vp, vp, i, vp, vp, i, vp, vp, vp]
    # (6) complex frequencies
    lib.es_complex_eval_grid.argtypes = [vp, vp, i, vp, i, vp, i, vp, i, i, vp, vp, vp, vp]
    lib.es_complex_eval_points.argtypes = [vp, vp, i, vp, vp, vp, i, vp, vp, vp, vp]
    lib.es_complex_find_roots.argtypes = [vp, vp, i, vp, i, vp, i, vp, i, i, vp, vp, vp, i, d,
                                          C.POINTER(ComplexRootTable), C.POINTER(i)]
    lib.es_complex_eigenfunction.argtypes = [vp, vp, i, vp, vp, vp, i, vp, vp, i, vp, vp, vp, vp]
    # (7) perturbation fields
    lib.es_cyl_polarisation.argtypes = [vp, vp, vp, i, i, vp, vp, i, vp, vp, vp, C.POINTER(FieldProfiles), i, d, d, d, d,
                                        i, vp, vp]
    lib.es_cyl_field_synthesis.argtypes = [vp, vp, vp, i, i, d, d, vp, i, vp, i, vp, i, C.c_uint32, d, i, vp, vp]
    # (8) Cartesian sampling and vorticity
    lib.es_cyl_vorticity_amplitudes.argtypes = [vp, vp, vp, i, i, i, i, vp, vp]
    lib.es_cyl_cartesian_synthesis.argtypes = [vp, vp, vp, vp, i, i, i, d, d, vp, i, vp, i, vp, i, vp, i, C.c_uint32, d,
                                               C.c_float, i, vp]
    lib.es_cyl_cartesian_split.argtypes = [i, i, i, i] + [C.POINTER(i)] * 5
    # (9) perturbation fields of a slab mode
    lib.es_slab_polarisation.argtypes = [vp, vp, vp, vp, i, i, vp, vp, i, vp, vp, vp, i, C.POINTER(SlabFieldProfiles),
                                         d, d, d, d, i, i, vp, vp]
    lib.es_slab_field_synthesis.argtypes = [vp, vp, vp, i, i, d, d, d, vp, i, vp, i, vp, i, C.c_uint32, d, C.c_float, i,
                                            vp]
    # (10) branch labels
    lib.es_shoot_mode_signature.argtypes = [vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp, vp]
    # (11) dispersion slopes
    lib.es_shoot_root_slopes.argtypes = [vp, vp, vp, vp, i, vp, vp, vp, vp]
    # (12) slopes and Newton tracing of complex roots
    lib.es_complex_root_slopes.argtypes = [vp, vp, i, vp, vp, vp, i, vp, vp, vp, vp]
    lib.es_complex_newton.argtypes = [vp, vp, i, vp, vp, vp, i, vp, i, d, d, d, vp, vp, vp, vp, vp, vp]
    # (13) Newton tracing of real roots
    if hasattr(lib, "es_shoot_newton"):                     # absent from an earlier build loaded for an A/B (tools/, --lib)
        lib.es_shoot_newton.argtypes = [vp, vp, vp, vp, i, vp, i, d, d, d, vp, vp, vp, vp, vp, vp]
    # (14) complex frequencies on the untwisted cylinder
    if hasattr(lib, "es_cyl_complex_eval_grid"):            # likewise
        lib.es_cyl_complex_eval_grid.argtypes = [vp, vp, vp, i, vp, i, vp, i, i, vp, vp, vp, vp]
        lib.es_cyl_complex_eval_points.argtypes = [vp, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp]
        lib.es_cyl_complex_find_roots.argtypes = [vp, vp, vp, i, vp, i, vp, i, i, vp, vp, vp, i, d,
                                                  C.POINTER(ComplexRootTable), C.POINTER(i)]
    # (15) slopes and Newton tracing of complex cylinder roots
    if hasattr(lib, "es_cyl_complex_root_slopes"):          # likewise
        lib.es_cyl_complex_root_slopes.argtypes = [vp, vp, vp, vp, vp, i, vp, vp, vp, vp]
        lib.es_cyl_complex_newton.argtypes = [vp, vp, vp, vp, vp, i, vp, i, d, d, d, vp, vp, vp, vp, vp, vp]
    # (16) eigenfunctions and perturbation fields of complex cylinder roots
    if hasattr(lib, "es_cyl_complex_eigenfunction"):        # likewise
        lib.es_cyl_complex_eigenfunction.argtypes = [vp, vp, vp, vp, vp, i, vp, vp, i, vp, vp, vp, vp]
        lib.es_cyl_complex_polarisation.argtypes = [vp, vp, vp, vp, i, i, vp, vp, i, vp, vp, vp, C.POINTER(FieldProfiles), i,
                                                    d, d, d, d, i, vp, vp]
        lib.es_cyl_complex_field_synthesis.argtypes = [vp, vp, vp, i, i, d, d, d, vp, i, vp, i, vp, i, C.c_uint32, d, i, vp,
                                                       vp]
    # (17) complex frequencies on the twisted cylinder: the signatures of (14)
    if hasattr(lib, "es_cylt_complex_eval_grid"):           # likewise
        lib.es_cylt_complex_eval_grid.argtypes = lib.es_cyl_complex_eval_grid.argtypes
        lib.es_cylt_complex_eval_points.argtypes = lib.es_cyl_complex_eval_points.argtypes
        lib.es_cylt_complex_find_roots.argtypes = lib.es_cyl_complex_find_roots.argtypes
    # (18) slopes and Newton tracing of complex roots of the twisted cylinder: the signatures of (15)
    if hasattr(lib, "es_cylt_complex_root_slopes"):         # likewise
        lib.es_cylt_complex_root_slopes.argtypes = lib.es_cyl_complex_root_slopes.argtypes
        lib.es_cylt_complex_newton.argtypes = lib.es_cyl_complex_newton.argtypes
    # (19) eigenfunctions of complex roots of the twisted cylinder: the signature of (16); its polarisation and synthesis calls
    # take no problem handle and serve both families
    if hasattr(lib, "es_cylt_complex_eigenfunction"):       # likewise
        lib.es_cylt_complex_eigenfunction.argtypes = lib.es_cyl_complex_eigenfunction.argtypes
    # (20) Cartesian sampling and vorticity of complex cylinder roots: the signatures of (8) with complex tables and w_re, w_im
    if hasattr(lib, "es_cyl_complex_vorticity_amplitudes"):  # likewise
        lib.es_cyl_complex_vorticity_amplitudes.argtypes = [vp, vp, vp, i, i, i, i, vp, vp]
        lib.es_cyl_complex_cartesian_synthesis.argtypes = [vp, vp, vp, vp, i, i, i, d, d, d, vp, i, vp, i, vp, i, vp, i,
                                                           C.c_uint32, d, C.c_float, i, vp]
    # (21) dispersion curvature and group-speed extrema
    if hasattr(lib, "es_shoot_root_curvature"):             # likewise
        lib.es_shoot_root_curvature.argtypes = [vp, vp, vp, vp, i, vp, vp, vp, vp]
        lib.es_shoot_cg_extrema.argtypes = [vp, vp, vp, vp, vp, vp, i, vp, i, d, vp, vp, vp, vp, vp, vp, vp, vp]
    return lib
