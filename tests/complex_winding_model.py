"""Plain restatement of the cell rule of es_complex_find_roots (include/eigensolver_amd.h section 6): test infrastructure.

A cell (row, i_im, i_re) of the [nk, n_im, n_re] grid has the corners (i_im, i_re), (i_im, i_re + 1), (i_im + 1, i_re + 1),
(i_im + 1, i_re) -- counter-clockwise in the (Re omega, Im omega) plane -- and exists for i_re < n_re - 1, i_im < n_im - 1.
It is flagged iff all four corners are ES_PT_OK and the quarter-turns of D_c between consecutive corners (the last one
back to the first) add up to +4 or -4, or to 6 or more; a jump across two quadrants counts 8, so every cell with such an
edge is flagged.  Quadrants are taken with `>= 0` on both parts: -0.0 is non-negative and a NaN part is "negative".

Written as one loop over (row, i_im, i_re) on Python scalars on purpose: it shares no code and no vectorisation with
oracle/slab_complex.py::find_roots, which tests/test_complex_winding_model.py compares it with.
"""
import numpy as np

PT_OK = 0


def quadrant(re, im):
    if re >= 0.0:
        return 0 if im >= 0.0 else 3
    return 1 if im >= 0.0 else 2


def quarter_turns(qa, qb):
    d = (qb - qa) % 4
    if d == 0:
        return 0
    if d == 1:
        return 1
    if d == 3:
        return -1
    return 8


def cell_total(D, status, row, i_im, i_re):
    """Sum of the quarter-turns around the cell, or None if a corner is not ES_PT_OK."""
    corners = ((i_im, i_re), (i_im, i_re + 1), (i_im + 1, i_re + 1), (i_im + 1, i_re))
    for (a, b) in corners:
        if int(status[row][a][b]) != PT_OK:
            return None
    q = [quadrant(D[row][a][b].real, D[row][a][b].imag) for (a, b) in corners]
    return sum(quarter_turns(q[j], q[(j + 1) % 4]) for j in range(4))


def flagged_cells(D, status):
    """Ordered list of the flagged cells (row, i_im, i_re) of D [nk, n_im, n_re] (complex) and status (same shape)."""
    D, status = np.asarray(D), np.asarray(status)
    assert D.ndim == 3 and D.shape == status.shape
    nk, n_im, n_re = D.shape
    Dl, Sl = D.tolist(), status.tolist()                  # Python complex / int scalars: the loop below is the rule itself
    out = []
    for row in range(nk):
        for i_im in range(n_im - 1):
            for i_re in range(n_re - 1):
                total = cell_total(Dl, Sl, row, i_im, i_re)
                if total is None:
                    continue
                if total in (4, -4) or total >= 6:
                    out.append((row, i_im, i_re))
    return out


def corner_quadrants(D, status):
    """Set of the (q00, q10, q11, q01) tuples that occur among the cells whose four corners are ES_PT_OK."""
    D, status = np.asarray(D), np.asarray(status)
    nk, n_im, n_re = D.shape
    Dl, Sl = D.tolist(), status.tolist()
    seen = set()
    for row in range(nk):
        for i_im in range(n_im - 1):
            for i_re in range(n_re - 1):
                corners = ((i_im, i_re), (i_im, i_re + 1), (i_im + 1, i_re + 1), (i_im + 1, i_re))
                if all(Sl[row][a][b] == PT_OK for (a, b) in corners):
                    seen.add(tuple(quadrant(Dl[row][a][b].real, Dl[row][a][b].imag) for (a, b) in corners))
    return seen
