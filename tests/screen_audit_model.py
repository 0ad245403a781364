"""NumPy restatement of es_shoot_audit_screening (include/eigensolver_amd.h): the fp32-screened grid against the fp64
grid.  Written from the definitions of the header, array-wise and without a thought for speed, so that the kernel and
this model share nothing but the specification."""
from typing import NamedTuple

import numpy as np

UNSURE = 0x80
MISSED, FALSE, STATUS, SIGN = 1, 2, 4, 8
PT_OK = 0


class Audit(NamedTuple):
    counts: np.ndarray      # int64[10], the d_counts words
    worst: np.ndarray       # float64[2], the d_worst words
    cell: np.ndarray        # int64: the first min(counts[0], capacity) flagged cells, ascending
    kind: np.ndarray        # uint8: their kind bits
    kinds: np.ndarray       # uint8 (nk, nw): kind bits of every cell


def brackets(D, st):
    """B(D, st): sign change against the omega-neighbour of the same row, both ends ES_PT_OK; NaN products compare
    false; the last column is never a bracket."""
    D, st = np.asarray(D, dtype=np.float64), np.asarray(st)
    b = np.zeros(D.shape, dtype=bool)
    if D.shape[1] > 1:
        with np.errstate(invalid="ignore", over="ignore"):
            b[:, :-1] = (st[:, :-1] == PT_OK) & (st[:, 1:] == PT_OK) & (D[:, :-1] * D[:, 1:] < 0)
    return b


def _first_extremum(values, cells, largest):
    """(value, cell) of the extremum, ties to the smallest cell; NaN values are not candidates."""
    keep = ~np.isnan(values)
    values, cells = values[keep], cells[keep]
    if values.size == 0:
        return None
    best = values.max() if largest else values.min()
    return float(best), int(cells[values == best].min())


def audit(D_scr, st_scr, D64, st64, rel64=None, capacity=1024):
    D_scr, D64 = np.asarray(D_scr, dtype=np.float64), np.asarray(D64, dtype=np.float64)
    st_scr, st64 = np.asarray(st_scr, dtype=np.uint8), np.asarray(st64, dtype=np.uint8)
    nk, nw = D64.shape
    unsure = (st_scr & UNSURE) != 0
    vouched = ~unsure
    Dm = np.where(unsure, D64, D_scr)
    stm = np.where(unsure, st64, st_scr)
    b64, bm = brackets(D64, st64), brackets(Dm, stm)
    both_ok = vouched & (st_scr == PT_OK) & (st64 == PT_OK)
    kinds = np.zeros((nk, nw), dtype=np.uint8)
    kinds[b64 & ~bm] |= MISSED
    kinds[bm & ~b64] |= FALSE
    kinds[vouched & (stm != st64)] |= STATUS
    kinds[both_ok & (np.signbit(D_scr) != np.signbit(D64))] |= SIGN

    counts = np.zeros(10, dtype=np.int64)
    counts[0] = np.count_nonzero(kinds)
    for word, bit in ((1, MISSED), (2, FALSE), (3, STATUS), (4, SIGN)):
        counts[word] = np.count_nonzero(kinds & bit)
    counts[5] = np.count_nonzero(both_ok)
    counts[6] = np.count_nonzero(unsure)
    counts[7] = np.count_nonzero(b64)
    counts[8] = counts[9] = -1
    worst = np.array([np.inf, 0.0])

    compared = both_ok & (D_scr != D64) & ~np.isnan(D_scr) & ~np.isnan(D64)
    cells = np.flatnonzero(compared.reshape(-1))
    ds, d64 = D_scr.reshape(-1)[cells], D64.reshape(-1)[cells]
    with np.errstate(all="ignore"):
        diff = np.abs(ds - d64)
        m = _first_extremum(np.abs(d64) / diff, cells, largest=False)
        if m is not None:
            worst[0], counts[8] = m
        if rel64 is not None:
            rel = np.asarray(rel64, dtype=np.float64).reshape(-1)[cells]
            use = (d64 != 0) & np.isfinite(rel) & (rel > 0)
            e = _first_extremum(diff[use] / (np.abs(d64[use]) * 100.0 / rel[use]), cells[use], largest=True)
            if e is not None:
                worst[1], counts[9] = e

    flagged = np.flatnonzero(kinds.reshape(-1))[:capacity]
    return Audit(counts, worst, flagged.astype(np.int64), kinds.reshape(-1)[flagged], kinds)
