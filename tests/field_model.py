"""NumPy restatement of include/eigensolver_amd.h section 7 (es_cyl_polarisation, es_cyl_field_synthesis), taking the
same arrays as the C calls.  The amplitude expressions are the reference's, written literally and in its order of
operations -- Cylinder/Non-uniform density/Coronal/Movies/Export_vtk.py (the same text in Gaussian_flow_export_vtk.py:
796-852 and v01_p1_kink_export_vtk.py:2179-2238); line numbers below are Export_vtk.py's.  The only departure: omega_A^2
and omega_c^2 are formed from the arrays bA and qc as the determinant kernels form them (for B_phi = 0, every reference
configuration, that is :622-630 up to rounding).

Pinned on the CPU by tests/test_field_model.py against the scripts' own arrays (tests/golden/fields_*.npz)."""
import numpy as np

AMP_NAMES = ("xi_r", "xi_phi", "xi_z", "P_T", "v_r", "v_phi", "v_z")
VAR_NAMES = ("xi_r", "xi_phi", "P_T", "v_r", "v_phi", "xi_x", "xi_y", "v_x", "v_y", "v_z", "xi_z")


def fixture_equilibrium(name, n_nodes=60):
    """Product equilibrium with the parameters of the export script behind tests/golden/fields_<name>.npz."""
    from eigensolver_amd import equilibrium as q
    return {"CDC": q.CylinderDensity(width=0.9, r_sign=1.0, n_nodes=n_nodes, ic=(1e-8, 1e-8)),              # Export_vtk.py:133-193
            "CF": q.CylinderFlow(U_i0=0.05, width=1e5, r_sign=1.0, r_axis=0.15, n_nodes=n_nodes),           # Gaussian_flow_export_vtk.py:135-211
            "CR": q.CylinderRotation(v_twist=0.1, power=1.0, n_nodes=n_nodes)}[name]                        # v01_p1_kink_export_vtk.py:154-250


def resonance_distance(k, w, m, prof):
    """min over the nodes of |Om^2 - omega_A^2| / Om^2 and |Om^2 - omega_c^2| / Om^2 (the denominators of :780, :786)."""
    r = prof["r"]
    Om = (w - (m * prof["vphi"] / r) - k * prof["vz"])
    wA2 = ((m * prof["Bphi"] / r) + k * prof["bA"]) ** 2
    wc2 = wA2 * prof["qc"]
    return float(min(np.min(np.abs(Om ** 2 - wA2) / Om ** 2), np.min(np.abs(Om ** 2 - wc2) / Om ** 2)))


def polarisation(k, w, int_value, int_flux, ext_x, ext_value, ext_flux, prof, m, rho_e, vA_e, c_e, cT_e,
                 reference=True):
    """One mode.  int_value / int_flux [N] (node 0 = boundary), ext_* [n_ext] (far field -> boundary), prof: dict of the
    es_field_profiles arrays.  reference: the flag ES_FIELD_REFERENCE (factor w^2 of the exterior xi_z, :781).
    Returns radius [n_r], amp [7, n_r] on spatial = concatenate(ix[::-1], lx[::-1]) (:723)."""
    m = float(m)
    ix = np.asarray(prof["r"], dtype=np.float64)[::-1]
    rho, B_i, B_iphi = prof["rho"][::-1], prof["Bz"][::-1], prof["Bphi"][::-1]
    v_iz, v_iphi = prof["vz"][::-1], prof["vphi"][::-1]
    q, dv_phi, dv_z = prof["q"][::-1], prof["s_phi"][::-1], prof["s_z"][::-1]
    P, xi = np.asarray(int_value)[::-1], np.asarray(int_flux)[::-1]          # inside_P_solution[::-1], inside_xi_solution[::-1]
    lx = np.asarray(ext_x)[::-1]
    left_P, left_xi = np.asarray(ext_value)[::-1], np.asarray(ext_flux)[::-1]
    with np.errstate(all="ignore"):
        f_B = (m * B_iphi / ix + k * B_i)                                      # :606-607
        g_B = (m * B_i / ix + k * B_iphi)                                      # :611-612
        shift = (w - (m * v_iphi / ix) - k * v_iz)                             # :617-618
        alfven2 = ((m * B_iphi / ix) + k * prof["bA"][::-1]) ** 2              # :622-623, as the determinant forms it
        cusp2 = alfven2 * prof["qc"][::-1]                                     # :627-628
        Q = ((-(shift ** 2 - alfven2) * rho * v_iphi ** 2 / ix) + (2 * shift ** 2 * B_iphi ** 2 / ix) +
             (2 * shift * B_iphi * v_iphi * ((m * B_iphi / ix) + (k * B_i)) / ix))                      # :637-638
        T = ((((m * B_iphi / ix) + (k * B_i)) * B_iphi) + rho * v_iphi * shift)                         # :642-643
        inside_v_r = -shift * xi                                               # :767
        inside_xi_z = ((f_B * q * (shift ** 2 * P - Q * xi) / (shift ** 2 * rho * (shift ** 2 - cusp2))) -
                       ((2. * shift * v_iphi * B_iphi + f_B * v_iphi ** 2) * (xi / ix)) -
                       (B_iphi * (g_B * P - 2. * B_i * T * (xi / ix)) / (B_i * rho * (shift ** 2 - alfven2)))) / \
                      (B_iphi ** 2 / B_i + B_i)                                # :780
        inside_xi_phi = (((g_B * P - 2. * B_i * T * (xi / ix)) / (rho * (shift ** 2 - alfven2))) +
                         (B_iphi * inside_xi_z)) / B_i                          # :786
        inside_v_phi = -(shift * inside_xi_phi) - (dv_phi * ix * xi)           # :804
        inside_v_z = -(shift * inside_xi_z) - (dv_z * xi)                      # :818
        outside_v_r = -w * left_xi                                             # :766
        wfac = w ** 2 if reference else 1.0
        outside_xi_z = k * c_e ** 2 * wfac * left_P / (rho_e * (w ** 2 - k ** 2 * cT_e ** 2) * (c_e ** 2 + vA_e ** 2))   # :781
        outside_xi_phi = (m * left_P / lx) / (rho_e * (w ** 2 - k ** 2 * vA_e ** 2))                                    # :787
        outside_v_phi = -w * outside_xi_phi                                    # :803
        outside_v_z = -w * outside_xi_z                                        # :817
    cat = lambda a, b: np.concatenate((a, b), axis=None)                       # noqa: E731
    radius = cat(ix, lx)                                                       # :723
    amp = np.stack([cat(xi, left_xi), cat(inside_xi_phi, outside_xi_phi), cat(inside_xi_z, outside_xi_z),
                    cat(P, left_P), cat(inside_v_r, outside_v_r), cat(inside_v_phi, outside_v_phi),
                    cat(inside_v_z, outside_v_z)])
    return radius, amp


def synthesis(radius, amp, m, k, w, theta, z, t, variables=None, v_scale=1.0, z_reference_angle=False):
    """fp64 fields [n_t, n_sel, n_z, n_theta, n_r] in ascending order of the mask bits (VAR_NAMES) and the points
    [n_z, n_theta, n_r, 3]: the loop body of :934-946 as broadcast expressions, v_scale on every velocity."""
    names = [v for v in VAR_NAMES if variables is None or v in variables]
    m = float(m)
    A = dict(zip(AMP_NAMES, np.asarray(amp, dtype=np.float64)))
    th = np.asarray(theta, dtype=np.float64)[None, None, :, None]
    zz = np.asarray(z, dtype=np.float64)[None, :, None, None]
    tt = np.asarray(t, dtype=np.float64)[:, None, None, None]
    R = lambda a: a[None, None, None, :]                                       # noqa: E731
    C = np.cos(k * zz - w * tt)
    cm, sm = np.cos(m * th), -np.sin(m * th)
    zf = sm if z_reference_angle else cm
    f = {}
    f["xi_r"] = R(A["xi_r"]) * cm * C                                          # :934
    f["xi_phi"] = R(A["xi_phi"]) * sm * C                                      # :935
    f["P_T"] = R(A["P_T"]) * cm * C                                            # :937
    f["v_r"] = v_scale * R(A["v_r"]) * cm * C                                  # :938
    f["v_phi"] = v_scale * R(A["v_phi"]) * sm * C                              # :939
    f["v_z"] = v_scale * R(A["v_z"]) * zf * C                                  # :940
    f["xi_z"] = R(A["xi_z"]) * zf * C                                          # :936
    f["xi_x"] = f["xi_r"] * np.cos(th) - f["xi_phi"] * np.sin(th)              # :943
    f["xi_y"] = f["xi_r"] * np.sin(th) + f["xi_phi"] * np.cos(th)              # :944
    f["v_x"] = f["v_r"] * np.cos(th) - f["v_phi"] * np.sin(th)                 # :945
    f["v_y"] = f["v_r"] * np.sin(th) + f["v_phi"] * np.cos(th)                 # :946
    shape = (len(tt), len(names), zz.shape[1], th.shape[2], len(radius))
    out = np.empty(shape, dtype=np.float64)
    for i, v in enumerate(names):
        out[:, i] = np.broadcast_to(f[v], (shape[0],) + shape[2:])
    r = np.asarray(radius, dtype=np.float64)[None, None, :]
    th3, z3 = th[0], zz[0]
    pts = np.empty(shape[2:] + (3,), dtype=np.float64)
    pts[..., 0] = r * np.cos(th3)                                              # :979
    pts[..., 1] = r * np.sin(th3)                                              # :980
    pts[..., 2] = np.broadcast_to(z3, shape[2:])
    return out, pts, names


def synthesis_bound(model, amp):
    """|gpu - model| <= 2^-23 |model| + 1e-12 max|A|: one fp32 rounding on each side plus the fp64 phase error."""
    return 2.0 ** -23 * np.abs(model) + 1e-12 * np.nanmax(np.abs(amp))
