"""Helper (not a test): yardsticks for es_shoot_root_curvature and es_shoot_cg_extrema (include/eigensolver_amd.h section 21).

  cauchy      the Taylor coefficients of outer and inner of root_slope_model.parts up to second order by Cauchy's formula
              on a circle in omega and a circle in k: NS x NS samples, the 2-D trapezoid rule, read off a 2-D FFT.  parts is
              analytic in both variables, the rule converges geometrically in NS and there is no difference step: a route
              that shares nothing with the kernel's second-order forward mode.  Beside a pole or a continuum edge the
              circles must stay inside the region of analyticity: every pair has its radius (RADIUS), and the
              self-discrepancy of a pair is the disagreement of its second derivatives between that radius and half of it.
  curvature   d2 omega / dk2 of the root curve from the six derivatives of D.
  newton      the model's own root at fixed k (complex-step D_w of root_slope_model.jets).
  cg_extrema  a restatement of the rule of es_shoot_cg_extrema, step for step, on the model.

What the GPU tests compare against is stored in tests/golden/root_curvature_model.json (write_golden), so that they do not
run the model; tests/test_root_curvature_model.py holds the file to a fresh evaluation.
"""
import functools
import json
import os

import numpy as np

from tests import real_eigen_model as M
from tests import root_slope_model as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "root_curvature_model.json")
NS = 24

# all four families, both axis conditions, the rotation kink condition, a non-zero axis target, one / two RK4 steps and
# several rescaling chunks
CASES = ("CF_flow_kink_N2", "SFG_flow_kink_N2", "CF_flow_kink_N3", "SFG_flow_kink_N3", "CF_flow_kink_N130",
         "SFG_flow_kink_N130", "CF_flow_sausage", "CF_flow_m3", "CF_flow_m5", "CF_flow_kink_target", "CDC_w095_kink",
         "CR_kink", "CR_sausage", "SD_w15_sausage", "SD_w15_kink", "SFU_sausage") + M.LARGE_GAP
# the large-gap cases (far field at ten wavelengths) run on real_eigen_model.large_gap_pairs, one pair per target gap
# mu (R - 1) = 30, 39, 41, 50: both texts of exterior_cylinder, the one without an I pair from 40 on, and exp(-2 gap) just below
N_DRAWN = 12        # real_eigen_model.pairs(name, N_DRAWN): the first four are the pairs of the slope tests
# the pairs of a case, as indices into the drawn ones: 0 .. 3 unless a pair lies so close to a singularity that no radius of
# RADII brings its self-discrepancy below 1e-8; such a pair is replaced by a later draw (never dropped)
PAIRS = {name: (0, 1, 2, 3) for name in CASES}
RADII = (0.02, 0.005, 0.00125)
# radius of every pair (the one of RADII with the smallest self-discrepancy) and the self-discrepancy measured with it, in
# units of max(|outer_xx|, |inner_xx|) over the three second derivatives (measure() prints both tables)
RADIUS = {"CF_flow_kink_N2": (0.02, 0.02, 0.02, 0.02),
          "SFG_flow_kink_N2": (0.02, 0.02, 0.02, 0.02),
          "CF_flow_kink_N3": (0.02, 0.02, 0.02, 0.02),
          "SFG_flow_kink_N3": (0.02, 0.02, 0.02, 0.02),
          "CF_flow_kink_N130": (0.02, 0.02, 0.02, 0.02),
          "SFG_flow_kink_N130": (0.02, 0.02, 0.02, 0.02),
          "CF_flow_sausage": (0.02, 0.02, 0.02, 0.02),
          "CF_flow_m3": (0.02, 0.02, 0.02, 0.02),
          "CF_flow_m5": (0.02, 0.02, 0.005, 0.02),
          "CF_flow_kink_target": (0.02, 0.02, 0.02, 0.02),
          "CDC_w095_kink": (0.02, 0.02, 0.02, 0.02),
          "CR_kink": (0.005, 0.02, 0.02, 0.02),
          "CR_sausage": (0.02, 0.02, 0.02, 0.02),
          "SD_w15_sausage": (0.02, 0.02, 0.02, 0.02),
          "SD_w15_kink": (0.02, 0.02, 0.02, 0.02),
          "SFU_sausage": (0.00125, 0.005, 0.02, 0.005),
          "LG_flow_kink": (0.02, 0.02, 0.02, 0.02),
          "LG_flow_sausage": (0.02, 0.02, 0.02, 0.02),
          "LG_dens_kink": (0.02, 0.02, 0.02, 0.02),
          "LG_dens_sausage": (0.02, 0.02, 0.02, 0.02)}
SELF_MEASURED = {"CF_flow_kink_N2": (1.1e-12, 1.3e-13, 2.7e-12, 5.2e-13),
                 "SFG_flow_kink_N2": (3.6e-12, 7.5e-13, 2.1e-13, 1.2e-14),
                 "CF_flow_kink_N3": (5.7e-13, 1.3e-13, 9.9e-14, 5.8e-13),
                 "SFG_flow_kink_N3": (3.8e-14, 6.5e-14, 2.1e-14, 9e-13),
                 "CF_flow_kink_N130": (7.2e-13, 5.2e-12, 1.3e-13, 1.1e-13),
                 "SFG_flow_kink_N130": (7.9e-12, 1.2e-13, 4.4e-14, 5.2e-14),
                 "CF_flow_sausage": (1.8e-12, 1.4e-12, 5.8e-13, 1.1e-12),
                 "CF_flow_m3": (2e-12, 7.1e-12, 1.7e-12, 8e-13),
                 "CF_flow_m5": (5.2e-13, 3.7e-13, 1.5e-12, 8.7e-13),
                 "CF_flow_kink_target": (7.6e-13, 2.2e-13, 1.4e-13, 5.4e-13),
                 "CDC_w095_kink": (6e-12, 2.9e-12, 5.8e-12, 3.4e-12),
                 "CR_kink": (1.8e-10, 4.3e-12, 2e-12, 1.4e-11),
                 "CR_sausage": (3.6e-13, 6.2e-13, 2e-12, 1.2e-11),
                 "SD_w15_sausage": (7.9e-13, 5.2e-14, 1.3e-13, 1.2e-13),
                 "SD_w15_kink": (1.4e-12, 1.3e-13, 3.8e-14, 1.2e-13),
                 "SFU_sausage": (4.7e-12, 2.9e-13, 5.7e-14, 4.6e-13),
                 "LG_flow_kink": (1.3e-13, 2.1e-12, 6.7e-13, 3.8e-13),
                 "LG_flow_sausage": (2.7e-13, 5.7e-12, 9e-13, 1.4e-12),
                 "LG_dens_kink": (2.2e-13, 2e-13, 1.1e-12, 5.4e-13),
                 "LG_dens_sausage": (1.9e-13, 5.1e-13, 2e-13, 2.7e-13)}

# d2 omega / dk2 of the model at the model's roots against the Richardson-combined central difference of the model's c_g
# along its own Newton-traced root curve (k +- 1e-3, k +- 5e-4): the worst |difference| / max(1, |curvature|) per case,
# measured with this file; the tests allow 10 x
CURVE_CASES = ("CF_flow_kink_N130", "SFG_flow_kink_N130", "CF_flow_sausage", "SD_w15_sausage", "CR_kink")
# (CR_kink: one of its four roots lies beside a pole of the exterior term; with the radius of its pair, 0.02, the model was
# 1e-8 off the difference of its own c_g there; curve_roots chooses the radius of a root anew)
CURVE_MEASURED = {"CF_flow_kink_N130": 9e-12, "SFG_flow_kink_N130": 3.2e-12, "CF_flow_sausage": 7.6e-12,
                  "SD_w15_sausage": 3.2e-12, "CR_kink": 4.7e-12}

# the group-speed minimum of the fast sausage branch of the density slab: a bracket on the branch through
# (k, omega) = (3.4305002, 3.982627)
EXTREMUM_CASE = "SD_w15_sausage"
EXTREMUM_START = (3.4305002, 3.982627)
EXTREMUM_BRACKET = (1.8, 2.4)


def pairs(name):
    """(k, w) of a case: the drawn pairs PAIRS selects; the large-gap cases use their four gap-targeted pairs"""
    if name in M.LARGE_GAP:
        return M.large_gap_pairs(name)
    k, w = M.pairs(name, N_DRAWN)
    idx = list(PAIRS[name])
    return k[idx], w[idx]


def gaps(name):
    """mu (R - 1) at the pairs of a large-gap case: what exterior_cylinder compares with 40"""
    prob = M.problem(name)
    k, w = pairs(name)
    return np.array([np.sqrt(M.exterior_m_e(prob, kk, ww)) * (prob.L_factor * 2.0 * np.pi / kk - 1.0) for kk, ww in zip(k, w)])


def cauchy(name, k, w, radius, ns=NS):
    """(outer[6, p], inner[6, p]): value, d/d omega, d/dk, d2/d omega2, d2/d omega dk, d2/dk2 at the pairs k[p], w[p];
    radius: one per pair or a scalar, the same in omega and k."""
    k, w = np.atleast_1d(np.asarray(k, dtype=np.float64)), np.atleast_1d(np.asarray(w, dtype=np.float64))
    r = np.broadcast_to(np.asarray(radius, dtype=np.float64), k.shape)
    z = np.exp(2j * np.pi * np.arange(ns) / ns)
    W = np.broadcast_to(w[:, None, None] + r[:, None, None] * z[None, :, None], (len(k), ns, ns))
    K = np.broadcast_to(k[:, None, None] + r[:, None, None] * z[None, None, :], (len(k), ns, ns))
    out = []
    for f in R.parts(name, K.ravel(), W.ravel()):
        c = np.fft.fft2(f.reshape(len(k), ns, ns), axes=(1, 2)) / (ns * ns)      # c[p, a, b]: the term (dw / r)^a (dk / r)^b
        out.append(np.array([c[:, 0, 0].real, c[:, 1, 0].real / r, c[:, 0, 1].real / r, 2.0 * c[:, 2, 0].real / r ** 2,
                             c[:, 1, 1].real / r ** 2, 2.0 * c[:, 0, 2].real / r ** 2]))
    return out[0], out[1]


def discrepancy(a, b):
    """per pair: max over the three second derivatives and both sides of |a - b|, in units of max(|outer_xx|, |inner_xx|)"""
    (ao, ai), (bo, bi) = a, b
    scale = np.maximum(np.abs(bo[3:]), np.abs(bi[3:]))
    return np.max(np.maximum(np.abs(ao[3:] - bo[3:]), np.abs(ai[3:] - bi[3:])) / scale, axis=0)


def self_discrepancy(name, k, w, radius):
    """(jets at `radius`, their disagreement with the jets at half of it)"""
    half = cauchy(name, k, w, 0.5 * np.asarray(radius))
    full = cauchy(name, k, w, radius)
    return full, discrepancy(half, full)


@functools.lru_cache(maxsize=None)
def case_jets(name):
    """(outer[6, p], inner[6, p], self-discrepancy[p]) at pairs(name) with the stored radii, computed once per session"""
    (o, i), d = self_discrepancy(name, *pairs(name), np.array(RADIUS[name]))
    return o, i, d


def group_velocity(D):
    return -D[2] / D[1]


def curvature(D):
    """d2 omega / dk2 from the six derivatives D[6, p] of the determinant"""
    cg = group_velocity(D)
    return -(D[5] + 2.0 * D[4] * cg + D[3] * cg * cg) / D[1]


def newton(name, k, w, steps=8):
    """the model's root at fixed k from the guess w: (w, every step finite), the rule of the kernel's polish"""
    k, w = np.atleast_1d(np.asarray(k, dtype=np.float64)), np.array(np.atleast_1d(w), dtype=np.float64)
    live = np.ones(len(k), dtype=bool)
    ok = np.ones(len(k), dtype=bool)
    for _ in range(steps):
        if not live.any():
            break
        o, i = R.jets(name, k[live], w[live])
        s = -(o[0] - i[0]) / (o[1] - i[1])
        good = np.isfinite(s)
        idx = np.flatnonzero(live)
        ok[idx[~good]] = False
        w[idx[good]] += s[good]
        live[idx] = good & (np.abs(s) > 1e-14 * np.abs(w[idx]))
    return w, ok


def point(name, k, w, radius, ns=NS):
    """(w, c_g, q) of the model's root at k nearest the guess w: polish, then one second-order evaluation"""
    w, _ = newton(name, k, w)
    o, i = cauchy(name, k, w, radius, ns)
    D = o - i
    return w, group_velocity(D), curvature(D)


def curve_check(name, k, w, radius):
    """(w, cg, q, dq): the model's polished root, group speed and curvature at the roots (k, w), and the Richardson-combined
    central difference of its c_g along its own root curve"""
    w, cg, q = point(name, k, w, radius)
    s = []
    for h in (1e-3, 5e-4):
        side = []
        for sg in (+1.0, -1.0):
            wn, _ = newton(name, k + sg * h, w + sg * cg * h + 0.5 * q * h * h)
            side.append(group_velocity(np.subtract(*R.jets(name, k + sg * h, wn))))
        s.append((side[0] - side[1]) / (2.0 * h))
    return w, cg, q, (4.0 * s[1] - s[0]) / 3.0


def best_radius(name, k, w):
    """(radius[p], self-discrepancy[p]): per pair the radius of RADII whose jets agree best with those at half of it"""
    d = np.array([self_discrepancy(name, k, w, r)[1] for r in RADII])
    d = np.where(np.isnan(d), np.inf, d)
    best = np.argmin(d, axis=0)
    return np.array(RADII)[best], d[best, np.arange(len(best))]


@functools.lru_cache(maxsize=None)
def curve_roots(name):
    """(k, w, radius) of the roots the curvature check runs on: the model's own, from pairs(name) of a case by Newton (a
    pair is no root, but Newton from it lands on one); those that did not converge to an ES_PT_OK point are left out.  A
    root may lie beside a pole its pair was far from: the radius is chosen anew (best_radius)."""
    k, w0 = pairs(name)
    w, ok = newton(name, k, w0, steps=30)
    o, i = R.jets(name, k, w)
    keep = ok & (np.abs(o[0] - i[0]) <= 1e-9 * np.maximum(np.abs(o[0]), np.abs(i[0])))
    keep &= np.array([M.cpu_ok(name, kk, ww) for kk, ww in zip(k, w)])
    return k[keep], w[keep], best_radius(name, k[keep], w[keep])[0]


# ---- the rule of es_shoot_cg_extrema ----------------------------------------------------------------------------------------
# a larger circle and more samples: the rounding noise of parts (1e-14 of the value after 1000 RK4 steps) enters a second
# derivative divided by NS r^2, and q, a difference of terms a hundred times its size, decides the last iterates.  The nearest
# singularity, the exterior cut-off, lies 0.11 away in k
EXTREMUM_RADIUS, EXTREMUM_NS = 0.06, 64


def _differ(a, b):
    return (a < 0.0 and b > 0.0) or (a > 0.0 and b < 0.0)


def cg_extrema(name, k_lo, w_lo, k_hi, w_hi, max_iter=40):
    """dict k, w, cg, q, iters, changed and `trace` (the k of every iterate) for one bracket, following the kernel's loop"""
    def pt(k, w):
        w, cg, q = point(name, np.array([k]), np.array([w]), EXTREMUM_RADIUS, EXTREMUM_NS)
        return dict(k=float(k), w=float(w[0]), cg=float(cg[0]), q=float(q[0]))
    a, b = pt(k_lo, w_lo), pt(k_hi, w_hi)
    changed = _differ(a["q"], b["q"])
    high = not (abs(a["q"]) <= abs(b["q"]) or not np.isfinite(b["q"]))
    fa, fb, side, iters, trace = a["q"], b["q"], 0, 0, []
    while changed and iters < max_iter:
        kc = b["k"] - fb * (b["k"] - a["k"]) / (fb - fa)
        if not (a["k"] < kc < b["k"]):
            kc = 0.5 * (a["k"] + b["k"])
        e = a if kc - a["k"] <= b["k"] - kc else b
        dk = kc - e["k"]
        c = pt(kc, e["w"] + e["cg"] * dk + 0.5 * e["q"] * dk * dk)
        iters += 1
        trace.append(kc)
        high = _differ(c["q"], fa)
        if high:
            b, fb = c, c["q"]
            if side == 1:
                fa *= 0.5
            side = 1
        else:
            a, fa = c, c["q"]
            if side == -1:
                fb *= 0.5
            side = -1
        if not np.isfinite(c["q"]) or c["q"] == 0.0 or b["k"] - a["k"] <= 1e-12 * abs(c["k"]):
            break
    return dict(b if high else a, iters=iters, changed=changed, trace=trace)


@functools.lru_cache(maxsize=None)
def extremum_bracket():
    """(k_lo, w_lo, k_hi, w_hi): the model's roots at the ends of EXTREMUM_BRACKET on the branch through EXTREMUM_START,
    reached by continuation in steps of 0.05 in k"""
    k0, w0 = EXTREMUM_START
    ends = []
    for k_end in EXTREMUM_BRACKET:
        k, (w, cg, q) = k0, point(EXTREMUM_CASE, np.array([k0]), np.array([w0]), 0.01)
        while abs(k - k_end) > 1e-12:
            kn = k_end if abs(k_end - k) <= 0.05 else k + np.sign(k_end - k) * 0.05
            dk = kn - k
            k, (w, cg, q) = kn, point(EXTREMUM_CASE, np.array([kn]), w + cg * dk + 0.5 * q * dk * dk, 0.01)
        ends.append((k, float(w[0])))
    return ends[0] + ends[1]


# ---- the stored tables ---------------------------------------------------------------------------------------------------------
def measure():
    """print RADIUS, SELF_MEASURED and CURVE_MEASURED as this file holds them (run once when a case or a pair changes)"""
    radius, disc = {}, {}
    for name in CASES:
        k, w = pairs(name)
        r, d = best_radius(name, k, w)
        radius[name] = tuple(float(x) for x in r)
        disc[name] = tuple(float(f"{x:.1e}") for x in d)
    print("RADIUS =", json.dumps(radius).replace("],", "],\n         "))
    print("SELF_MEASURED =", json.dumps(disc).replace("],", "],\n                "))
    RADIUS.update(radius)
    curve = {}
    for name in CURVE_CASES:
        k, w, r = curve_roots(name)
        _, _, q, dq = curve_check(name, k, w, r)
        curve[name] = float(f"{np.max(np.abs(q - dq) / np.maximum(1.0, np.abs(q))):.1e}")
        print(name, "roots", len(k), "q", q, "difference", np.abs(q - dq))
    print("CURVE_MEASURED =", json.dumps(curve))


def golden():
    """what the GPU tests read: per case the pairs and the model's jets, the roots of the curvature check with their
    curvature, the extremum bracket and the restatement's answer"""
    out = {"cases": {}, "curve": {}}
    for name in CASES:
        k, w = pairs(name)
        o, i, d = case_jets(name)
        out["cases"][name] = dict(k=k.tolist(), w=w.tolist(), outer=o.tolist(), inner=i.tolist())
        if name in M.LARGE_GAP:
            out["cases"][name]["gap"] = gaps(name).tolist()
    for name in CURVE_CASES:
        k, w, r = curve_roots(name)
        w, cg, q = point(name, k, w, r)
        out["curve"][name] = dict(k=k.tolist(), w=w.tolist(), cg=cg.tolist(), q=q.tolist())
    br = extremum_bracket()
    out["extremum"] = dict(bracket=list(br), **cg_extrema(EXTREMUM_CASE, *br))
    return out


def write_golden():
    with open(GOLDEN, "w") as f:
        json.dump(golden(), f, indent=0)


@functools.lru_cache(maxsize=None)
def read_golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    import sys
    measure() if "--measure" in sys.argv else write_golden()
