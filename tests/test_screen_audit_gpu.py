"""es_shoot_audit_screening on the GPU against its NumPy model (tests/screen_audit_model.py): synthetic arrays at every
shape where the kernel takes another path, a miss planted into a real screened grid, one problem per family at the grids
of tests/test_mixed_gpu.py, the row sampling of ShootProblem.audit_screening and find_roots_mixed_audited."""
import ctypes as C

import numpy as np
import pytest

from tests import screen_audit_model as M

pytestmark = pytest.mark.gpu

# (1,64)/(1,65): one wave and its halo; (3,64): the lane-63 halo sits on a row boundary; (2,257): a block boundary;
# (9,1000): 36 blocks through the scan
SHAPES = [(1, 1), (7, 1), (1, 64), (1, 65), (3, 64), (2, 257), (5, 333), (9, 1000)]


def _synthetic(nk, nw, wild=True):
    """Seeded random grids.  wild: NaN, +-0 and inf sprinkled into both D arrays and bad entries into rel; otherwise every
    vouched-for point has a finite non-zero D64 and a usable rel (the extrema are then governed by the planted points)."""
    rng = np.random.default_rng(1000 * nk + nw)
    shape = (nk, nw)
    D64 = rng.standard_normal(shape)
    st64 = rng.choice(np.arange(4, dtype=np.uint8), size=shape, p=[0.7, 0.1, 0.1, 0.1])
    D_scr = D64 * (1.0 + 1e-3 * rng.standard_normal(shape))
    flip = rng.random(shape) < 0.06
    D_scr[flip] = -D_scr[flip]
    same = rng.random(shape) < 0.3
    D_scr[same] = D64[same]                                        # equal values are not compared points
    st_scr = st64.copy()
    other = rng.random(shape) < 0.05
    st_scr[other] = rng.integers(0, 4, size=shape, dtype=np.uint8)[other]
    st_scr[rng.random(shape) < 0.2] |= M.UNSURE
    rel = rng.uniform(0.1, 50.0, size=shape)
    if wild:
        for arr in (D64, D_scr):
            for value in (np.nan, 0.0, -0.0, np.inf, -np.inf):
                arr[rng.random(shape) < 0.02] = value
        for value in (np.nan, 0.0, -1.0, np.inf):
            rel[rng.random(shape) < 0.02] = value
    return D_scr, st_scr, D64, st64, rel


def _run(ctx, D_scr, st_scr, D64, st64, rel=None, capacity=1024):
    import torch
    from eigensolver_amd import shooting
    dev = [torch.from_numpy(np.array(a)).cuda() if a is not None else None
           for a in (D_scr, st_scr, D64, st64, rel)]
    return shooting.audit_arrays(ctx, *dev, capacity=capacity)


def _assert_equals_model(report, model, nw):
    got = [report.flagged, report.missed, report.false, report.status, report.sign, report.vouched_ok, report.unsure,
           report.brackets64]
    assert got == model.counts[:8].tolist()
    cell_of = lambda at: -1 if at is None else at[0] * nw + at[1]             # noqa: E731
    assert (cell_of(report.min_margin_at), cell_of(report.max_err_at)) == (model.counts[8], model.counts[9])
    np.testing.assert_allclose([report.min_margin, report.max_err], model.worst, rtol=1e-15, atol=0.0)
    assert np.array_equal(report.row * nw + report.col, model.cell)
    assert np.array_equal(report.kind, model.kind)


@pytest.mark.parametrize("with_rel", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_model_on_synthetic_arrays(es_ctx, shape, with_rel):
    D_scr, st_scr, D64, st64, rel = _synthetic(*shape)
    rel = rel if with_rel else None
    cells = shape[0] * shape[1]
    full = M.audit(D_scr, st_scr, D64, st64, rel, capacity=cells + 1)
    count = int(full.counts[0])
    if cells >= 500:
        assert count >= 4 and all(full.counts[1:5] > 0)            # every kind occurs
    _assert_equals_model(_run(es_ctx, D_scr, st_scr, D64, st64, rel, capacity=cells + 1), full, shape[1])
    for cap in sorted({max(count, 1), max(count // 2, 1), 1}):      # exactly the count, below it, a single entry
        _assert_equals_model(_run(es_ctx, D_scr, st_scr, D64, st64, rel, capacity=cap),
                             M.audit(D_scr, st_scr, D64, st64, rel, capacity=cap), shape[1])
    r0 = _run(es_ctx, D_scr, st_scr, D64, st64, rel, capacity=0)    # counts only: null table pointers
    _assert_equals_model(r0, M.audit(D_scr, st_scr, D64, st64, rel, capacity=0), shape[1])
    assert r0.flagged == count and r0.row.size == 0
    if not with_rel:
        assert r0.max_err_at is None and r0.max_err == 0.0


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] * s[1] >= 64])
def test_planted_extrema_are_found_at_their_cells(es_ctx, shape):
    D_scr, st_scr, D64, st64, rel = _synthetic(*shape, wild=False)
    nk, nw = shape
    cells = nk * nw
    p, q = cells - 3, cells // 2 + 1       # least margin in the last wave of the last block, largest err mid-grid
    for c in (p, q):
        st_scr.reshape(-1)[c] = st64.reshape(-1)[c] = 0
        D64.reshape(-1)[c] = 1.0
    D_scr.reshape(-1)[p], rel.reshape(-1)[p] = 101.0, 1e-3          # margin 1e-2, err 1e-3
    D_scr.reshape(-1)[q], rel.reshape(-1)[q] = 5.0, 1e4             # margin 0.25, err 400
    model = M.audit(D_scr, st_scr, D64, st64, rel)
    assert (model.counts[8], model.counts[9]) == (p, q)
    assert model.worst.tolist() == [1.0 / 100.0, 4.0 / (1.0 * 100.0 / 1e4)]
    # the runners-up (the model with the planted point marked unsure) are a factor of ten away
    for c, word in ((p, 0), (q, 1)):
        hide = st_scr.copy()
        hide.reshape(-1)[c] |= M.UNSURE
        rest = M.audit(D_scr, hide, D64, st64, rel).worst[word]
        assert rest >= 10 * model.worst[0] if word == 0 else 10 * rest <= model.worst[1]
    report = _run(es_ctx, D_scr, st_scr, D64, st64, rel)
    assert report.min_margin_at == (p // nw, p % nw) and report.max_err_at == (q // nw, q % nw)
    _assert_equals_model(report, model, nw)


@pytest.fixture(scope="module")
def flow_kink(es_ctx):
    """CF_flow_kink at the grid of test_mixed_gpu.py::test_mixed_equals_fp64_other_cylinders: the problem, its grid, the
    fp64 and the raw screened arrays on the host.  Shared and left unchanged."""
    from eigensolver_amd import ShootProblem
    from tests import cases
    eq, mode, m, (lo, hi) = cases.all_cases()["CF_flow_kink"]
    gp = ShootProblem(eq, mode, m, ctx=es_ctx)
    k = np.linspace(0.05, 3.9, 40)
    W = lo + (np.arange(700) + 0.5) * (hi - lo) / 700
    D64, st64, rel = (t.cpu().numpy() for t in gp.eval_grid(k, W, want_rel=True))
    D_scr, st_scr = (t.cpu().numpy() for t in gp.screen_grid(k, W))
    for a in (D64, st64, rel, D_scr, st_scr):
        a.setflags(write=False)
    yield gp, k, W, D_scr, st_scr, D64, st64, rel
    gp.close()


def test_planted_miss_in_a_real_problem(es_ctx, flow_kink):
    gp, k, W, D_scr, st_scr, D64, st64, rel = flow_kink
    nw = W.size
    raw = _run(es_ctx, D_scr, st_scr, D64, st64, rel)
    _assert_equals_model(raw, M.audit(D_scr, st_scr, D64, st64, rel), nw)
    assert raw.missed == raw.false == raw.status == 0 and raw.ok and raw.unsure > 0 and raw.brackets64 > 0
    c = int(np.flatnonzero(M.brackets(D64, st64).reshape(-1))[0])
    D_doc, st_doc = D_scr.copy(), st_scr.copy()
    st_doc.reshape(-1)[[c, c + 1]] &= 0x7f                          # fp32 now vouches for both ends ...
    D_doc.reshape(-1)[c] = D64.reshape(-1)[c + 1]                   # ... and has the sign of the lower one wrong
    doctored = _run(es_ctx, D_doc, st_doc, D64, st64, rel)
    _assert_equals_model(doctored, M.audit(D_doc, st_doc, D64, st64, rel), nw)
    at = (doctored.row * nw + doctored.col).tolist()
    assert not doctored.ok and doctored.missed >= 1 and c in at
    assert doctored.kind[at.index(c)] & M.MISSED


@pytest.mark.parametrize("name", ["CR_kink", "CF_flow_m3", "SD_w15_kink", "SFG_flow_kink"])
def test_one_problem_per_family(es_ctx, name):
    """The grids of test_mixed_equals_fp64_other_cylinders / _slabs.  The bounds are the ones those tests hold on these very
    grids: err_D < 0.25 there is min_margin > 4 here, err < 5e-3 (cylinders) and < 5e-2 (slabs) is max_err."""
    from eigensolver_amd import ShootProblem
    from tests import cases
    eq, mode, m, (lo, hi) = cases.all_cases()[name]
    slab = name.startswith("S")
    gp = ShootProblem(eq, mode, m, ctx=es_ctx)
    k = np.linspace(0.1, 3.5, 40) if slab else np.linspace(0.05, 3.9, 40)
    W = lo + (np.arange(700) + 0.5) * (hi - lo) / 700
    r = gp.audit_screening(k, W)
    st64 = gp.eval_grid(k, W)[1].cpu().numpy()
    st_scr = gp.screen_grid(k, W)[1].cpu().numpy()
    unsure = (st_scr & M.UNSURE) != 0
    print(f"{name}: {r.unsure} unsure, {r.brackets64} fp64 brackets, min margin {r.min_margin:.3g} at {r.min_margin_at}, "
          f"max err {r.max_err:.3g} at {r.max_err_at}, sign {r.sign}")
    assert r.ok, r
    assert r.brackets64 > 0 and r.unsure > 0
    assert r.unsure == np.count_nonzero(unsure) and r.unsure + np.count_nonzero(~unsure) == 40 * 700
    assert r.vouched_ok == np.count_nonzero(~unsure & (st_scr == 0) & (st64 == 0)) > 0
    assert r.min_margin > 4, r.min_margin
    assert r.max_err < (5e-2 if slab else 5e-3), r.max_err
    gp.close()


def test_rows_sample_the_grid_and_report_full_grid_rows(es_ctx, flow_kink):
    gp, k, W, D_scr, st_scr, D64, st64, rel = flow_kink
    nw = W.size
    sel = np.arange(0, k.size, 4)
    model = M.audit(D_scr[sel], st_scr[sel], D64[sel], st64[sel], rel[sel])
    r = gp.audit_screening(k, W, rows=4)
    assert [r.flagged, r.missed, r.false, r.status, r.sign, r.vouched_ok, r.unsure, r.brackets64] == \
        model.counts[:8].tolist()
    np.testing.assert_allclose([r.min_margin, r.max_err], model.worst, rtol=1e-15, atol=0.0)
    full = lambda c: (int(sel[c // nw]), int(c % nw))                        # noqa: E731
    assert r.min_margin_at == full(model.counts[8]) and r.max_err_at == full(model.counts[9])
    # an index array selects the same rows; every row is the default
    assert gp.audit_screening(k, W, rows=sel)[:12] == r[:12]
    everything = gp.audit_screening(k, W)
    assert everything.unsure == int(np.count_nonzero(st_scr & M.UNSURE)) and everything.ok
    # a miss planted into row 8 of arrays the caller holds is reported at row 8 of the full grid, also from a sample
    import torch
    b = M.brackets(D64, st64)
    c = 8 * nw + int(np.flatnonzero(b[8])[0])
    D_doc, st_doc = D_scr.copy(), st_scr.copy()
    st_doc.reshape(-1)[[c, c + 1]] &= 0x7f
    D_doc.reshape(-1)[c] = D64.reshape(-1)[c + 1]
    held = (torch.from_numpy(D_doc).cuda(), torch.from_numpy(st_doc).cuda())
    r = gp.audit_screening(k, W, rows=4, screened=held)
    model = M.audit(D_doc[sel], st_doc[sel], D64[sel], st64[sel], rel[sel])
    assert np.array_equal(r.row, sel[model.cell // nw]) and np.array_equal(r.col, model.cell % nw)
    assert np.array_equal(r.kind, model.kind)
    at = list(zip(r.row.tolist(), r.col.tolist()))
    assert (8, c % nw) in at and r.kind[at.index((8, c % nw))] & M.MISSED
    assert gp.audit_screening(k, W, rows=np.array([1, 2, 3]), screened=held).ok     # the planted row is not sampled
    # the merged output of find_roots_mixed has no unsure mark left and loses nothing
    _, _, Dm, stm, _ = gp.find_roots_mixed(k, W, n_bisect=24)
    merged = gp.audit_screening(k, W, screened=(Dm, stm))
    assert merged.unsure == 0 and merged.ok and merged.brackets64 == everything.brackets64
    assert merged.vouched_ok == int(np.count_nonzero(st64 == 0))


@pytest.mark.parametrize("name", ["CF_flow_kink", "SFG_flow_kink"])
def test_find_roots_mixed_audited(es_ctx, name):
    from eigensolver_amd import ShootProblem
    from tests import cases
    eq, mode, m, (lo, hi) = cases.all_cases()[name]
    gp = ShootProblem(eq, mode, m, ctx=es_ctx)
    k = np.linspace(0.1, 3.5, 24)
    W = lo + (np.arange(300) + 0.5) * (hi - lo) / 300
    plain = gp.find_roots_mixed(k, W, n_bisect=24)
    audited = gp.find_roots_mixed_audited(k, W, n_bisect=24, rows=3)
    assert len(audited) == len(plain) + 1
    assert audited[1] == plain[1] > 0 and audited[4] == plain[4]
    for key in ("k", "w", "w_lo", "w_hi", "resid", "row", "flag"):
        assert np.array_equal(plain[0][key].cpu().numpy(), audited[0][key].cpu().numpy(), equal_nan=True), key
    for a, b in zip(plain[2:4], audited[2:4]):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
    report = audited[5]
    assert report.ok and report.unsure == 0 and report.vouched_ok > 0
    gp.close()


def test_argument_errors_and_the_empty_grid(es_ctx):
    import torch
    from eigensolver_amd import shooting
    lib, h = es_ctx.lib, es_ctx.handle
    D = torch.zeros((2, 3), dtype=torch.float64, device="cuda")
    st = torch.zeros((2, 3), dtype=torch.uint8, device="cuda")
    counts = torch.full((10,), 77, dtype=torch.int64, device="cuda")
    worst = torch.full((2,), 77.0, dtype=torch.float64, device="cuda")
    cell = torch.full((4,), 77, dtype=torch.int64, device="cuda")
    kind = torch.full((4,), 77, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                                    # noqa: E731
    good = dict(ctx=h, nk=2, nw=3, Ds=p(D), ss=p(st), D64=p(D), s64=p(st), rel=None, cap=4, cell=p(cell), kind=p(kind),
                counts=p(counts), worst=p(worst))
    bad = [dict(ctx=None), dict(nk=-1), dict(nw=-1), dict(cap=-1), dict(Ds=None), dict(ss=None), dict(D64=None),
           dict(s64=None), dict(counts=None), dict(worst=None), dict(cell=None), dict(kind=None)]
    for change in bad:
        a = dict(good, **change)
        assert lib.es_shoot_audit_screening(*a.values()) == 1, change
    torch.cuda.synchronize()
    assert counts.tolist() == [77] * 10 and worst.tolist() == [77.0] * 2       # nothing was enqueued
    assert lib.es_shoot_audit_screening(*dict(good, cap=0, cell=None, kind=None).values()) == 0
    assert counts.tolist() == [0, 0, 0, 0, 0, 6, 0, 0, -1, -1] and worst.tolist() == [np.inf, 0.0]
    assert cell.tolist() == [77] * 4 and kind.tolist() == [77] * 4             # no flagged cell: the table is left alone
    for shape in [(0, 5), (3, 0), (0, 0)]:
        e, s = torch.empty(shape, dtype=torch.float64, device="cuda"), torch.empty(shape, dtype=torch.uint8, device="cuda")
        r = shooting.audit_arrays(es_ctx, e, s, e, s, e)
        assert r[:8] == (0,) * 8 and r.min_margin == np.inf and r.max_err == 0.0
        assert r.min_margin_at is None and r.max_err_at is None and r.row.size == 0 and r.ok
