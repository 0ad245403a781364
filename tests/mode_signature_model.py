"""Helper (not a test): yardsticks for es_shoot_mode_signature (include/eigensolver_amd.h section 10).

  count      the count rule in NumPy: entries that are exactly zero or NaN are skipped, a change is counted whenever the sign
             of an entry differs from the sign of the last entry kept.
  peak       (max|row|, smallest node index that attains it).
  signature  both applied to the (value, flux) rows of tests/real_eigen_model.model, the NumPy restatement of the kernel's
             interior algorithm.
  decided    a row whose count does not depend on how rounding settles its tiny entries: every entry with
             0 < |x| < 1e-9 max|row| lies in a run of such entries flanked on BOTH sides by larger entries of OPPOSITE sign
             (the centre node of an odd slab mode: 2e-16 of the peak).  One sign change is counted across such a run
             whichever sign its entry takes.  This file asks for more than that sentence: the run may hold only ONE non-zero
             entry (two tiny entries could take different signs and add two changes).
  port_roots the accepted roots of the C port of the determinant on the 8 x 400 grid the branch tests use.
"""
import functools
from typing import NamedTuple

import numpy as np

from tests import cases
from tests import real_eigen_model as M

TINY = 1e-9

# the cases tests/test_mode_signature_gpu.py compares with the model: short grids (one and two RK4 steps among them) and one
# case per family at its own N
SMALL_GRIDS = ("CF_flow_kink_N130", "SFG_flow_kink_N130", "CF_flow_kink_N2", "CF_flow_kink_N3", "SFG_flow_kink_N2",
               "SFG_flow_kink_N3")
FAMILIES = ("CF_flow_sausage", "CF_flow_m3", "CR_kink", "CR_sausage", "SD_w15_sausage", "SFG_flow_sausage", "SFU_sausage")
MODEL_CASES = SMALL_GRIDS + FAMILIES

# label sets of the accepted roots on the 8 x 400 grid
BRANCHES = {
    "CF_flow_kink_N130": {(0, 0), (1, 1)},
    "SFG_flow_kink_N130": {(0, 1), (2, 3), (4, 5)},
    "CF_flow_sausage": {(1, 0), (2, 1)},
}
ROOT_K = np.linspace(0.8, 3.6, 8)
ROOT_NW = 400


class Signature(NamedTuple):
    nodes_value: int
    nodes_flux: int
    peak_node_value: int
    peak_node_flux: int
    peak_value: float
    peak_flux: float
    value: np.ndarray
    flux: np.ndarray

    @property
    def label(self):
        return (self.nodes_value, self.nodes_flux)


def count(row):
    row = np.asarray(row, dtype=np.float64)
    s = np.sign(row[(row != 0.0) & ~np.isnan(row)])
    return int(np.count_nonzero(s[1:] != s[:-1]))


def peak(row):
    a = np.abs(np.asarray(row, dtype=np.float64))
    j = int(np.argmax(a))                               # the first index that attains the maximum
    return float(a[j]), j


def of_rows(value, flux):
    (pv, jv), (pf, jf) = peak(value), peak(flux)
    return Signature(count(value), count(flux), jv, jf, pv, pf, np.asarray(value), np.asarray(flux))


@functools.lru_cache(maxsize=None)
def signature(name, k, w):
    """The rule applied to real_eigen_model.model(name, k, w); computed once per (case, pair), rows are not to be modified."""
    return of_rows(*M.model(name, float(k), float(w)))


def decided(row):
    row = np.asarray(row, dtype=np.float64)
    a = np.abs(row)
    thr = TINY * np.nanmax(a)
    small = ~(a >= thr)                                 # tiny entries, exact zeros and NaNs: what a run is made of
    j, n = 0, len(row)
    while j < n:
        if not small[j]:
            j += 1
            continue
        e = j
        while e < n and small[e]:
            e += 1
        tiny = int(np.count_nonzero((a[j:e] > 0.0)))    # NaN > 0 is False: NaNs and zeros are skipped by the rule
        if tiny:
            if tiny > 1 or j == 0 or e == n or not (row[j - 1] * row[e] < 0.0):
                return False
        j = e
    return True


def pair_decided(name, k, w):
    s = signature(name, k, w)
    return decided(s.value) and decided(s.flux)


def root_grid(name):
    """(k[8], W[400]): the grid of the branch tests, phase speeds at the cell centres of the case's window."""
    lo, hi = M.all_cases()[name][3]
    return ROOT_K, lo + (np.arange(ROOT_NW) + 0.5) * (hi - lo) / ROOT_NW


@functools.lru_cache(maxsize=None)
def port_roots(name):
    """(k, w, row) of the accepted roots the C port finds on root_grid(name) at pairs the oracle calls ES_PT_OK."""
    eq, mode, m, _ = M.all_cases()[name]
    port = cases.port_problem(eq, mode, m)
    k, W = root_grid(name)
    D, _, st = port.eval_grid(k, W, w_mode=1, nthreads=4)
    r, cnt = port.find_roots(k, W, D, st, w_mode=1, n_bisect=40, tol=1e-3, nthreads=4)
    assert cnt == len(r["k"])
    keep = [i for i in range(cnt) if r["flag"][i] == 1 and M.cpu_ok(name, float(r["k"][i]), float(r["w"][i]))]
    return r["k"][keep].copy(), r["w"][keep].copy(), r["row"][keep].copy()


def all_pairs(name):
    """Every (k, omega) the GPU test evaluates for a case: its fixed pairs, and the port's roots where it labels roots."""
    k, w = M.pairs(name)
    out = list(zip(k.tolist(), w.tolist()))
    if name in BRANCHES:
        rk, rw, _ = port_roots(name)
        out += list(zip(rk.tolist(), rw.tolist()))
    return out
