"""Helper (not a test): yardsticks for es_shoot_newton and the tracing on top of it (include/eigensolver_amd.h section 13).

  exterior_status  ES_PT_OK / LEAKY / NONFINITE of the closed-form exterior, as the kernels decide it.
  newton_model     the iteration rule of es_shoot_newton, step for step, on root_slope_model.jets (complex-step derivatives: a
                   different route from the kernel's forward-mode jets); records the length of every step per lane.
  clear            which lanes the GPU test may compare `iters` on: the rule stops a lane when |s| <= 1e-14 |w|, and a
                   step within a factor 10 of that threshold can fall on either side of it in another arithmetic.
  hermite          the Hermite prediction and the default shift bound of ShootProblem.densify in NumPy.
  port_root_near   the C port's root next to a candidate; the window of root_slope_model._port_root_near shifted off the
                   candidate by a third of a cell (a window centred on a root that is exact to the last bit puts D = 0 on a
                   grid point, where no sign change is seen).
  coarse_curves    {label: (omegas, ks, cg)} of the port's roots on the 8 x 400 grid of mode_signature_model, labels from the
                   NumPy eigenfunction model, slopes from the jets: the layout of postprocess.curves_with_slopes.
"""
import functools

import numpy as np

from tests import cases
from tests import mode_signature_model as S
from tests import real_eigen_model as M
from tests import root_slope_model as R

ST_OK, ST_LEAKY, ST_NONFINITE, ST_CONTINUUM = 0, 1, 2, 3
STOP = 1e-14

# the branches of the tracing tests: case -> labels
TRACE_CASES = {
    "CF_flow_kink_N130": ((0, 0), (1, 1)),
    "SFG_flow_kink_N130": ((0, 1), (2, 3)),
    "CF_flow_sausage": ((1, 0), (2, 1)),
    "CF_flow_m3": ((0, 0),),
    "SD_w15_sausage": ((1, 0),),
    "SFU_sausage": ((1, 0), (1, 2), (3, 4)),
}
# CR_kink: two roots per row share the label (1, 0) on the rows k = 2.4 ... 3.6 -- roots beside a pole of the exterior term
# (DESIGN.md sections 8f, 9).  trace_branches skips such a label; the two curves are split by hand, lower and upper omega.
SPLIT_CASE, SPLIT_LABEL, SPLIT_K_MIN = "CR_kink", (1, 0), 2.4
CUT = 4                                                      # every coarse interval is cut in four
# per case: (worst |predicted - omega| over its traced curves, rounded up to two digits; Newton steps at the most), as measured
# with this file.  The prediction error is a property of the curve and the coarse spacing, the step count
# follows from it: both are asserted; the residuals (1e-13 ... 3e-10 %) are rounding noise and only bounded.
TRACE_TABLE = {
    "CF_flow_kink_N130": (2.0e-4, 3),
    "SFG_flow_kink_N130": (3.2e-4, 3),
    "CF_flow_sausage": (9.9e-4, 4),
    "CF_flow_m3": (1.4e-5, 3),
    "SD_w15_sausage": (1.3e-5, 3),
    "SFU_sausage": (3.9e-5, 4),
    "CR_kink": (6.4e-2, 5),
}
RESID_CEILING = 1e-8                                         # percent; the acceptance tolerance is 1e-3

# the Newton tests against this model: four families, m = 3, one and two RK4 steps, one chunk edge (N = 130 > CH = 128)
MODEL_CASES = ("CF_flow_kink_N2", "CF_flow_kink_N3", "CF_flow_kink_N130", "SFG_flow_kink_N2", "SFG_flow_kink_N3",
               "SFG_flow_kink_N130", "CF_flow_sausage", "CF_flow_m3", "CR_kink", "SD_w15_sausage", "SFU_sausage")
# guess = root (1 + offset), the offsets cycled over the roots of a case
OFFSETS = (1e-4, -3e-5, 1e-5, -3e-4)


def exterior_status(name, k, w):
    d = R._desc(name)
    eq = M.all_cases()[name][0]
    k, w = np.asarray(k, dtype=np.float64), np.asarray(w, dtype=np.float64)
    vAe2, ce2, cTe2 = d.vA_e ** 2, d.c_e ** 2, d.cT_e ** 2
    with np.errstate(all="ignore"):
        k2 = k * k
        Oe = w if M.is_cyl(eq) else w - k * d.U_e
        Oe2 = Oe * Oe
        m_e = ((k2 * vAe2 - Oe2) * (k2 * ce2 - Oe2)) / ((vAe2 + ce2) * (k2 * cTe2 - Oe2))
        cst = -1.0 / (d.rho_e * (k2 * vAe2 - Oe2)) if M.is_cyl(eq) else \
            d.rho_e * (vAe2 + ce2) * (k2 * cTe2 - Oe2) / (Oe * (k2 * ce2 - Oe2))
    bad = ~(m_e > 0.0) | ~np.isfinite(m_e) | ~np.isfinite(cst)
    return np.where(m_e < 0.0, ST_LEAKY, np.where(bad, ST_NONFINITE, ST_OK)).astype(np.int64)


def newton_model(name, k, guess, max_iter=8, step_cap=np.inf, max_shift=np.inf, tol_percent=1e-3):
    """dict of arrays w, resid, iters, flag, dwdk, status (that of the exterior) and `steps`, per lane the |s| of every step
    taken.  All lanes of an iteration are evaluated in one batch; a lane that has stopped is left out of the next."""
    guess = np.atleast_1d(np.asarray(guess, dtype=np.float64))
    k = np.broadcast_to(np.asarray(k, dtype=np.float64), guess.shape).copy()
    n = len(guess)
    w, iters = guess.copy(), np.zeros(n, dtype=np.int64)
    ok, active = np.ones(n, dtype=bool), np.ones(n, dtype=bool)
    steps = [[] for _ in range(n)]
    with np.errstate(all="ignore"):
        for _ in range(max_iter):
            idx = np.nonzero(active)[0]
            if len(idx) == 0:
                break
            o, i = R.jets(name, k[idx], w[idx])
            st = exterior_status(name, k[idx], w[idx])
            D, Dw = o[0] - i[0], o[1] - i[1]
            for a, lane in enumerate(idx):
                if st[a] != ST_OK or not np.isfinite(D[a]) or not np.isfinite(Dw[a]) or Dw[a] == 0.0:
                    ok[lane] = active[lane] = False
                    continue
                s = -D[a] / Dw[a]
                if abs(s) > step_cap:
                    s = np.copysign(step_cap, s)
                w[lane] += s
                iters[lane] += 1
                steps[lane].append(abs(s))
                if abs(s) <= STOP * abs(w[lane]):
                    active[lane] = False
        o, i = R.jets(name, k, w)
        st = exterior_status(name, k, w)
        D = o[0] - i[0]
        resid = 100.0 * np.abs(D) / np.maximum(np.abs(o[0]), np.abs(i[0]))
        dwdk = -(o[2] - i[2]) / (o[1] - i[1])
        st = np.where((st == ST_OK) & ~np.isfinite(D), ST_NONFINITE, st)
        resid, dwdk = np.where(st == ST_OK, resid, np.nan), np.where(st == ST_OK, dwdk, np.nan)
        flag = ok & (st == ST_OK) & (resid < tol_percent) & (np.abs(w - guess) <= max_shift)
    return dict(w=w, resid=resid, iters=iters, flag=flag.astype(np.int64), dwdk=dwdk, status=st, steps=steps)


def clear(steps, w):
    """no step of the lane within a factor 10 of the stopping threshold"""
    thr = STOP * abs(w)
    return all(not (0.1 <= s / thr <= 10.0) for s in steps)


def hermite(ks, ws, cg, k_fine, shift_factor=4.0):
    """(predicted, bound) at k_fine: ShootProblem.densify's prediction and default max_shift, in NumPy"""
    x, y, d, kf = (np.asarray(a, dtype=np.float64) for a in (ks, ws, cg, k_fine))
    h = np.diff(x)
    j = np.clip(np.searchsorted(x, kf, side="right") - 1, 0, len(x) - 2)
    hj = h[j]
    t = (kf - x[j]) / hj
    t2, t3 = t * t, t * t * t
    pred = ((2 * t3 - 3 * t2 + 1) * y[j] + (t3 - 2 * t2 + t) * hj * d[j]
            + (-2 * t3 + 3 * t2) * y[j + 1] + (t3 - t2) * hj * d[j + 1])
    dw = np.diff(y)
    defect = np.maximum(np.abs(dw - h * d[:-1]), np.abs(dw - h * d[1:]))
    bound = np.maximum(shift_factor * defect, 1e-8 * np.maximum(np.abs(y[:-1]), 1.0))[j]
    return pred, bound


def cut_in(ks, parts=CUT):
    """the coarse wavenumbers and parts - 1 points inside every interval"""
    ks = np.asarray(ks, dtype=np.float64)
    fr = np.arange(parts) / parts
    return np.concatenate([(ks[:-1, None] + fr[None, :] * np.diff(ks)[:, None]).reshape(-1), ks[-1:]])


@functools.lru_cache(maxsize=None)
def _port(name):
    eq, mode, m, _ = M.all_cases()[name]
    return cases.port_problem(eq, mode, m)


def port_root_near(name, k, w_pred):
    """the root of the port's determinant in the row k nearest to w_pred inside the shifted window; None if there is none"""
    port = _port(name)
    cell = 2.0 * R.WINDOW / (R.NWIN - 1)
    kk = np.array([k])
    wg = w_pred + cell / 3.0 + np.linspace(-R.WINDOW, R.WINDOW, R.NWIN)
    D, _, st = port.eval_grid(kk, wg, w_mode=0, nthreads=1)
    r, cnt = port.find_roots(kk, wg, D, st, w_mode=0, n_bisect=R.NBISECT, tol=1e-3, nthreads=1)
    if cnt == 0:
        return None
    return float(r["w"][int(np.argmin(np.abs(r["w"] - w_pred)))])


@functools.lru_cache(maxsize=None)
def coarse_curves(name):
    """{label: (omegas, ks, cg)}, every curve ordered by k (ties by omega); arrays are not to be modified"""
    k, w, _ = S.port_roots(name)
    cg = R.group_velocity(*R.jets(name, k, w))
    labels = [S.signature(name, float(a), float(b)).label for a, b in zip(k, w)]
    out = {}
    for label in sorted(set(labels)):
        sel = np.array([i for i, lab in enumerate(labels) if lab == label])
        sel = sel[np.lexsort((w[sel], k[sel]))]
        out[label] = (w[sel], k[sel], cg[sel])
    return out


@functools.lru_cache(maxsize=None)
def split_curves():
    """the two (1, 0) curves of CR_kink on the rows k >= 2.4, split by hand: {"lower": (omegas, ks, cg), "upper": ...}"""
    w, k, cg = coarse_curves(SPLIT_CASE)[SPLIT_LABEL]
    sel = k >= SPLIT_K_MIN - 1e-12
    w, k, cg = w[sel], k[sel], cg[sel]
    assert len(k) % 2 == 0 and np.array_equal(k[0::2], k[1::2]), "two roots on every row"
    return {"lower": (w[0::2], k[0::2], cg[0::2]), "upper": (w[1::2], k[1::2], cg[1::2])}


@functools.lru_cache(maxsize=None)
def traced(name, which=None):
    """The tracing of one curve in the model: dict with label, k (the coarse interval cut in four), predicted, bound and the
    newton_model result from the prediction under max_shift = bound.  which: a label of TRACE_CASES[name], or "lower" /
    "upper" of the split case."""
    w, k, cg = split_curves()[which] if name == SPLIT_CASE else coarse_curves(name)[which]
    kf = cut_in(k)
    pred, bound = hermite(k, w, cg, kf)
    out = newton_model(name, kf, pred)
    out["flag"] = out["flag"] * (np.abs(out["w"] - pred) <= bound)
    out.update(k=kf, predicted=pred, bound=bound, label=SPLIT_LABEL if name == SPLIT_CASE else which,
               coarse=(w, k, cg))
    return out


def trace_list():
    return [(n, lab) for n, labs in TRACE_CASES.items() for lab in labs] + [(SPLIT_CASE, "lower"), (SPLIT_CASE, "upper")]


@functools.lru_cache(maxsize=None)
def offset_guesses(name):
    """(k, guess, root): the port's roots of the case on the 8 x 400 grid with the offsets cycled over them"""
    k, w, _ = S.port_roots(name)
    off = np.array([OFFSETS[i % len(OFFSETS)] for i in range(len(k))])
    return k.copy(), w * (1.0 + off), w.copy()


@functools.lru_cache(maxsize=None)
def offset_model(name):
    """newton_model from offset_guesses(name), computed once per session; not to be modified"""
    k, g, _ = offset_guesses(name)
    return newton_model(name, k, g)
