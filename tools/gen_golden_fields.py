"""The export scripts' own radial amplitudes at one root per cylinder family (container only, like tools/gen_golden.py).

    python tools/gen_golden_fields.py      ->  tests/golden/fields_{CDC,CF,CR}.npz

Executes, from the text of the reference files and with the shims of tools/ref_harness.py, the profile and ODE slices of
  CDC  Cylinder/Non-uniform density/Coronal/Movies/Export_vtk.py                       (Gaussian density, width 0.9)
  CF   Cylinder/Non-uniform flow/Coronal/Movies/Gaussian_flow_export_vtk.py            (U_i0 = 0.05, width 1e5, r >= 0.15)
  CR   Cylinder/Rotational flow/Photospheric/vtk export/v01_p1_kink_export_vtk.py      (v_twist = 0.1, power 1)
with an injected (k, omega) instead of the pickled root tables the scripts read and with short grids (ix 60 nodes, lx 80
points), and records the scripts' own inside_P_solution, inside_xi_solution, left_P_solution, left_xi_solution, ix, lx
and the radial_* arrays they derive (Export_vtk.py:764-818).  Numbers only are written.

Two more textual shims, both needed by today's sympy and neither changing a number: `sym.diff(v_iphi(r)/r)` and
`sym.diff(v_iz(r)/r)` get the symbol spelled out (sym.diff of an expression without free symbols -- v_twist = 0, or
v_iphi/r constant -- raises instead of returning 0).

(k, omega): a root of the family's kink determinant found here with the DOP853 oracle (oracle/cylinder.py) in the window
given below; it is checked that no interior node lies within 1e-3 (relative) of Om^2 = omega_A^2 or Om^2 = omega_c^2."""
import os
import sys

import numpy as np
from scipy.optimize import brentq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_harness as H  # noqa: E402
from eigensolver_amd import shooting  # noqa: E402
from tests import cases, field_model  # noqa: E402

H.FILES["X-CDC"] = "Cylinder/Non-uniform density/Coronal/Movies/Export_vtk.py"
H.FILES["X-CF"] = "Cylinder/Non-uniform flow/Coronal/Movies/Gaussian_flow_export_vtk.py"
H.FILES["X-CR"] = "Cylinder/Rotational flow/Photospheric/vtk export/v01_p1_kink_export_vtk.py"

N_IX, N_LX = 60, 80
DIFF = [("sym.diff(v_iphi(r)/r)", "sym.diff(v_iphi(r)/r, r)"), ("sym.diff(v_iz(r)/r)", "sym.diff(v_iz(r)/r, r)")]

# numpy >= 1.24 rejects the ragged y0 = [scalar, array([x])] the scripts hand to odeintz (ref_harness flattens it for odeint)
ODEINTZ = [("z0 = np.array(z0, dtype=np.complex128, ndmin=1)",
            "z0 = np.array([complex(np.ravel(np.asarray(v))[0]) for v in z0], dtype=np.complex128, ndmin=1)")]

# family -> (file key, slices, grid replacements, the two lines that receive (k, omega), suffix of the radial_* names,
#            product equilibrium of the script's parameters, k, phase-speed window of the root)
FAMILIES = {
    "CDC": ("X-CDC", [(1, 24), (133, 294), (550, 729), (760, 820)],
            [("np.linspace(1., 0.001, 500.)", f"np.linspace(1., 0.001, {N_IX})"), ("700.)", f"{N_LX})")],
            ("k = test_k", "w = test_w"), "",
            field_model.fixture_equilibrium("CDC", N_IX), 1.2, (2.05, 4.3)),
    "CF": ("X-CF", [(1, 24), (135, 277), (569, 752), (788, 854)],
           [("np.linspace(1., 0.15, 500.)", f"np.linspace(1., 0.15, {N_IX})"), ("1500.)", f"{N_LX})")],
           ("k = test_k", "w = test_w"), "",
           field_model.fixture_equilibrium("CF", N_IX), 1.2, (2.1, 4.9)),
    "CR": ("X-CR", [(1, 99), (154, 304), (2012, 2240)],
           [("np.linspace(1., 0.001, 2e3)", f"np.linspace(1., 0.001, {N_IX})"), ("3500.)", f"{N_LX})")],
           ("wavenum = sol_ksv01_p1_singleplot_body_kink[0]", "frequency = sol_omegasv01_p1_singleplot_body_kink[0]"), "_v025_p1",
           field_model.fixture_equilibrium("CR", N_IX), 1.5, (1.02, 1.45)),
}


def find_root(eq, k, window):
    """First sign change of the DOP853 kink mismatch over 600 phase speeds of the window, refined with brentq."""
    prob = cases.truth_problem(eq, "kink")

    def d(W):
        r = prob.mismatch(k, k * W, rtol=1e-10)
        return float(r["d"]) if isinstance(r, dict) else float(r[0] if isinstance(r, tuple) else r)
    Ws = np.linspace(window[0], window[1], 600)
    prev = None
    for W in Ws:
        try:
            v = d(W)
        except Exception:
            v = float("nan")
        if prev is not None and np.isfinite(v) and np.isfinite(prev[1]) and v * prev[1] < 0:
            Wr = brentq(d, prev[0], W, xtol=1e-12)
            prof = shooting.field_profiles(eq, np.linspace(eq.x_boundary, eq.x_end, eq.n_nodes))
            if field_model.resonance_distance(k, k * Wr, 1, prof) > 1e-2 and abs(d(Wr)) < 1e-6 * max(abs(v), abs(prev[1])):
                return k * Wr
        prev = (W, v)
    raise RuntimeError("no root found in the window")


def run(name):
    key, slices, grids, kw_lines, suffix, eq, k, window = FAMILIES[name]
    w = find_root(eq, k, window)
    repl = list(grids) + DIFF + ODEINTZ + [(kw_lines[0], kw_lines[0].split("=")[0] + f"= {k!r}"),
                                           (kw_lines[1], kw_lines[1].split("=")[0] + f"= {w!r}")]
    cwd = os.getcwd()
    os.makedirs("/tmp/ref_scratch", exist_ok=True)
    os.chdir("/tmp/ref_scratch")
    try:
        ns = H.load_slices(key, slices, replacements=repl)
    finally:
        os.chdir(cwd)
    assert len(ns["ix"]) == N_IX and len(ns["lx"]) == N_LX, (len(ns["ix"]), len(ns["lx"]))

    def real(a):
        a = np.asarray(a)
        if np.iscomplexobj(a):
            assert np.all(a.imag == 0.0), "complex array with a non-zero imaginary part"
            a = a.real
        return np.ascontiguousarray(a, dtype=np.float64)
    rec = {n: real(ns[n]) for n in ("ix", "lx", "inside_P_solution", "inside_xi_solution", "left_P_solution",
                                    "left_xi_solution")}
    radial = {"radial_displacement": "xi_r", "radial_xi_phi": "xi_phi", "radial_xi_z": "xi_z", "radial_PT": "P_T",
              "radial_vr": "v_r", "radial_v_phi": "v_phi", "radial_v_z": "v_z"}
    for ref_name, ch in radial.items():
        rec["radial_" + ch] = real(ns[ref_name + suffix])
    rec["spatial"] = real(ns["spatial" + suffix])
    rec["k"], rec["w"], rec["m"] = np.float64(ns["k"]), np.float64(ns["w"]), np.float64(ns["m"])
    for c in ("rho_e", "vA_e", "c_e", "cT_e", "c_i0", "vA_i0"):
        rec[c] = np.float64(ns[c])
    prof = shooting.field_profiles(eq, rec["ix"])
    dist = field_model.resonance_distance(float(rec["k"]), float(rec["w"]), 1, prof)
    assert dist > 1e-3, dist
    out = os.path.join(ROOT, "tests", "golden", f"fields_{name}.npz")
    np.savez(out, **rec)
    print(name, "k", float(rec["k"]), "w", float(rec["w"]), "resonance distance", dist, "->", out, os.path.getsize(out),
          "bytes", flush=True)


if __name__ == "__main__":
    for fam in (sys.argv[1:] or list(FAMILIES)):
        run(fam)
