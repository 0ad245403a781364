"""Host model of the ES_REFINE_HYBRID root refinement (helper of the tests, not a test): a NumPy restatement of the rule of
include/eigensolver_amd.h over oracle.port.PortProblem.eval_points.

    section_round  one 17-section round of refine_kernel (first sign change from the lower end)
    polish         the two regula-falsi steps of refine_polish_kernel
    one_lane       the one-lane phase of refine_superlinear_kernel: at most ONE_LANE_STEPS bracketing secant steps with
                   Illinois scaling of the retained end, stopped at a relative step or width of ONE_LANE_EPS
    find_roots     brackets of a grid + the whole rule -> table, kept / fallback masks, evaluation counts

With one_lane_steps = 0 every bracket takes the fallback and the table is port.find_roots' table bit for bit."""
import numpy as np

SECTIONS = 17
LANES = SECTIONS - 1
POLISH = 2
HYBRID_SECTIONS = 1          # kHybridSections of es_refine.hip
ONE_LANE_STEPS = 8           # kHybridSteps
ONE_LANE_EPS = 1e-12         # kHybridEps = ROOT_RTOL / 100
# Early fallback on a pole signature (an iterate with |D| above |D| at both ends): NOT part of the rule.  It saves 1 - 3
# marches per bracket but loses converging roots (one each on CDC_w095_kink, SD_w15_sausage and SFG_flow_sausage, S = 1);
# one_lane(early=True) is kept to show that.
EARLY_FALLBACK = False
PT_OK = 0


def rounds_for(n_bisect, sections=SECTIONS):
    rounds, span, need = 0, 1.0, np.ldexp(1.0, min(int(n_bisect), 1000))
    while span < need:
        span *= float(sections)
        rounds += 1
    return rounds


def marches_per_bracket(n_bisect, brackets, fallback, evals, s_rounds=HYBRID_SECTIONS):
    """16 S + h[3] / h[0] + (16 (R - S) + 2) h[2] / h[0]; the section rule costs 16 R + 2."""
    R = rounds_for(n_bisect)
    if brackets == 0:
        return 0.0
    if R <= s_rounds:
        return float(LANES * R + POLISH)
    return LANES * s_rounds + evals / brackets + (LANES * (R - s_rounds) + POLISH) * fallback / brackets


def brackets_of(k, w, D, st, w_mode=1):
    """(row, column) of every bracket, rows outer, and its ends as the emit kernel forms them (pick_w)."""
    D, st = np.asarray(D), np.asarray(st)
    ok = (st[:, :-1] == PT_OK) & (st[:, 1:] == PT_OK)
    with np.errstate(invalid="ignore", over="ignore"):
        sign = D[:, :-1] * D[:, 1:] < 0.0
    row, col = np.nonzero(ok & sign)
    kk = np.asarray(k, dtype=np.float64)[row]
    w = np.asarray(w, dtype=np.float64)
    if w_mode == 1:
        lo, hi = kk * w[col], kk * w[col + 1]
    elif w_mode == 2:
        lo, hi = w[row, col], w[row, col + 1]
    else:
        lo, hi = w[col], w[col + 1]
    return row.astype(np.int32), col, kk, lo, hi, D[row, col].copy(), D[row, col + 1].copy()


def section_round(port, kk, lo, hi, flo, fhi, nthreads=0):
    n = len(kk)
    if n == 0:
        return lo, hi, flo, fhi
    frac = (np.arange(LANES, dtype=np.float64) + 1.0) / float(SECTIONS)
    x = lo[:, None] + (hi - lo)[:, None] * frac[None, :]
    dv, _, _ = port.eval_points(np.repeat(kk, LANES), x.ravel(), nthreads=nthreads)
    dv = dv.reshape(n, LANES)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = dv * flo[:, None] < 0.0
    first = np.where(diff.any(axis=1), diff.argmax(axis=1), LANES)
    i = np.arange(n)
    lo, hi, flo, fhi = lo.copy(), hi.copy(), flo.copy(), fhi.copy()
    up = first > 0
    dl = dv[i, np.maximum(first - 1, 0)]
    lo[up] = x[i, np.maximum(first - 1, 0)][up]
    flo[up] = np.where(dl == dl, dl, flo)[up]
    dn = first < LANES
    hi[dn] = x[i, np.minimum(first, LANES - 1)][dn]
    fhi[dn] = dv[i, np.minimum(first, LANES - 1)][dn]
    return lo, hi, flo, fhi


def polish(port, kk, lo, hi, flo, fhi, tol, nthreads=0):
    """-> w, w_lo, w_hi, resid, flag"""
    n = len(kk)
    lo, hi, flo, fhi = lo.copy(), hi.copy(), flo.copy(), fhi.copy()
    root, r, s = lo + (hi - lo) * 0.5, np.full(n, np.nan), np.full(n, 2, dtype=np.uint8)
    for _ in range(POLISH):
        if n == 0:
            break
        with np.errstate(all="ignore"):
            x = lo - flo * (hi - lo) / (fhi - flo)
            inside = (x > lo) & (x < hi)
            end = np.where(np.abs(flo) <= np.abs(fhi), lo, hi)
            x = np.where(inside, x, np.where(x == x, end, lo + (hi - lo) * 0.5))
            d, r, s = port.eval_points(kk, x, nthreads=nthreads)
            root = x
            neg = d * flo < 0.0
        fin = (d == d) & ~neg
        hi, fhi = np.where(neg, x, hi), np.where(neg, d, fhi)
        lo, flo = np.where(fin, x, lo), np.where(fin, d, flo)
    with np.errstate(invalid="ignore"):
        flag = ((s == PT_OK) & (r < tol)).astype(np.uint8)
    return root, lo, hi, r, flag


def one_lane(port, kk, lo, hi, flo, fhi, tol, steps=ONE_LANE_STEPS, eps=ONE_LANE_EPS, nthreads=0, early=EARLY_FALLBACK):
    """The one-lane phase on the state the section rounds left.  -> kept mask, w, w_lo, w_hi, resid, evaluations per
    bracket.  Rows outside the mask hold no result."""
    n = len(kk)
    lo, hi, flo, fhi = lo.copy(), hi.copy(), flo.copy(), fhi.copy()
    side = np.zeros(n, dtype=np.int8)                   # -1: the lower end was retained by the last step, +1: the upper
    xprev = np.full(n, np.nan)
    active = np.ones(n, dtype=bool)
    kept = np.zeros(n, dtype=bool)
    w, resid = np.full(n, np.nan), np.full(n, np.nan)
    evals = np.zeros(n, dtype=np.int64)
    for _ in range(steps):
        a = np.nonzero(active)[0]
        if len(a) == 0:
            break
        l, h, fl, fh = lo[a], hi[a], flo[a], fhi[a]
        with np.errstate(all="ignore"):
            x = l - fl * (h - l) / (fh - fl)
            x = np.where((x > l) & (x < h), x, l + (h - l) * 0.5)
            d, r, s = port.eval_points(kk[a], x, nthreads=nthreads)
            evals[a] += 1
            nan = d != d
            if early:
                nan = nan | (np.abs(d) > np.maximum(np.abs(fl), np.abs(fh)))
            neg = d * fl < 0.0
            # Illinois: an end retained twice in a row has its value halved
            sd = side[a]
            fl2 = np.where(neg, np.where(sd < 0, fl * 0.5, fl), d)
            fh2 = np.where(neg, d, np.where(sd > 0, fh * 0.5, fh))
            l2, h2 = np.where(neg, l, x), np.where(neg, x, h)
            ax = np.abs(x)
            conv = (d == 0.0) | (np.abs(x - xprev[a]) <= eps * ax) | ((h2 - l2) <= eps * ax)
            conv &= ~nan
            good = conv & (s == PT_OK) & (r < tol)
        upd = ~nan
        au = a[upd]
        lo[au], hi[au], flo[au], fhi[au] = l2[upd], h2[upd], fl2[upd], fh2[upd]
        side[au] = np.where(neg[upd], -1, 1)
        xprev[a] = x
        ag = a[good]
        kept[ag] = True
        w[ag], resid[ag] = x[good], r[good]
        active[a[nan | conv]] = False
    return kept, w, lo, hi, resid, evals


def find_roots(port, k, w, D, st, w_mode=1, n_bisect=16, tol=1e-3, s_rounds=HYBRID_SECTIONS, steps=ONE_LANE_STEPS,
               nthreads=0):
    """The hybrid rule on the brackets of the grid.  -> (table dict, count, info) with info = dict(kept, fallback: masks
    over the brackets; evals: one-lane evaluations per bracket; cell_lo / cell_hi: the ends of the grid cell)."""
    row, _, kk, lo, hi, flo, fhi = brackets_of(k, w, D, st, w_mode)
    n = len(kk)
    cell_lo, cell_hi = lo.copy(), hi.copy()
    R = rounds_for(n_bisect)
    S = R if R <= s_rounds else s_rounds
    for _ in range(S):
        lo, hi, flo, fhi = section_round(port, kk, lo, hi, flo, fhi, nthreads)
    if R <= s_rounds:
        kept, evals = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64)
        fb = np.zeros(n, dtype=bool)                    # the section rule itself: no bracket counts as a fallback
        rest = np.ones(n, dtype=bool)
    else:
        kept, wk, lk, hk, rk, evals = one_lane(port, kk, lo, hi, flo, fhi, tol, steps=steps, nthreads=nthreads)
        fb = ~kept
        rest = fb
    out_w, out_lo, out_hi, out_r = np.empty(n), np.empty(n), np.empty(n), np.empty(n)
    out_f = np.zeros(n, dtype=np.uint8)
    if kept.any():
        out_w[kept], out_lo[kept], out_hi[kept], out_r[kept], out_f[kept] = wk[kept], lk[kept], hk[kept], rk[kept], 1
    if rest.any():
        l, h, fl, fh = lo[rest], hi[rest], flo[rest], fhi[rest]
        for _ in range(R - S):
            l, h, fl, fh = section_round(port, kk[rest], l, h, fl, fh, nthreads)
        out_w[rest], out_lo[rest], out_hi[rest], out_r[rest], out_f[rest] = polish(port, kk[rest], l, h, fl, fh, tol,
                                                                                 nthreads)
    tab = dict(k=kk, w=out_w, w_lo=out_lo, w_hi=out_hi, resid=out_r, row=row, flag=out_f)
    return tab, n, dict(kept=kept, fallback=fb, evals=evals, cell_lo=cell_lo, cell_hi=cell_hi)
