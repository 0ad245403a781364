"""Cartesian sampling of a cylinder mode, with its vorticity, on the GPU (include/eigensolver_amd.h section 8) against the
NumPy restatement tests/cartesian_model.py, which tests/test_cartesian_model.py pins on closed forms.

Bounds, none of them measured on the kernels:
  amplitudes   1e-10 of each channel's max, the project's bound for a kernel against a NumPy restatement of the same
               expressions.  It means something only if the model's own rounding is well below it, so every case first
               asserts E_round = max |model(float64) - model(longdouble)| <= 1e-11 of the channel's max.
  synthesis    section 7's |gpu - model| <= 2^-23 |model| + 1e-12 max|A|, A over the amplitudes and the vorticity
               amplitudes as scaled by v_scale.  Every mesh point is compared; the meshes are asserted to keep every
               point 1e-9 away from radius[0], the boundary radius and radius[n_r-1], where rounding of r would change the
               region (a selection flip, not a rounding error).
  curl         finite-difference curl of the float32 GPU frames against their own vort_x, vort_y, vort_z: at most twice
               the error the float64 model shows on the same mesh with the same tables (the factor 2 is for the float32
               data, whose rounding contributes about 2^-24 / h, orders below the truncation error), and that model error
               itself at most the 1.729e-3 the CPU leg recorded at 41^3 for m = 1.
Every check prints its measured figure with `pytest -s`.  On an MI355X: the amplitudes of every case are bit-identical to
the model (-ffp-contract=off, np.gradient's coefficient form in the same order); the frames sit at 0.000 of their bound
(the model is rounded to float32 as well); the curl of the CF root on 41^3 points: 9.003e-4 for the float32 GPU frames,
8.998e-4 for the float64 model."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import cartesian_model as M  # noqa: E402
from tests import cases  # noqa: E402

ALL = list(M.CVAR_NAMES)
SHAPES = [(3, 3), (3, 0), (64, 65), (130, 257)]


def _T(es_ctx, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=f"cuda:{es_ctx.device}")


def _tables(n_nodes, n_ext, n):
    """n modes: radius [n, n_r], amp [n, 7, n_r] (another grid and other amplitudes per mode), k [n]."""
    rad, amp = zip(*[M.smooth_table(n_nodes, n_ext, seed=7 + i) for i in range(n)])
    scale = (1.0 + 0.5 * np.arange(n))[:, None, None]
    return np.stack(rad), np.stack(amp) * scale, 0.9 + 0.6 * np.arange(n)


def _check_amplitudes(tag, got, radius, amp, n_nodes, m, k):
    v64 = M.vorticity_amplitudes(radius, amp, n_nodes, m, k)
    vld = M.vorticity_amplitudes(radius, amp, n_nodes, m, k, dtype=np.longdouble)
    assert np.all(np.isfinite(v64)), "the model itself is not finite"
    for c, ch in enumerate(M.VORT_NAMES):
        scale = np.max(np.abs(v64[c]))
        e_round = float(np.max(np.abs(v64[c] - vld[c])))
        err = float(np.max(np.abs(got[c] - v64[c])))
        print(f"vort {tag} {ch:6s}: err {err:.3e} bound {1e-10 * scale:.3e}   E_round {e_round:.3e} bound {1e-11 * scale:.3e}")
        assert e_round <= 1e-11 * scale, (tag, ch, e_round, scale)
        assert err <= 1e-10 * scale, (tag, ch, err, scale)


# ---- amplitudes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_nodes,n_ext", SHAPES)
def test_vorticity_amplitudes_match_the_model(es_ctx, n_nodes, n_ext):
    from eigensolver_amd import shooting
    for n in (1, 3):
        radius, amp, k = _tables(n_nodes, n_ext, n)
        for m in (0, 1, 3):
            got = shooting.vorticity_amplitudes(es_ctx, _T(es_ctx, radius), _T(es_ctx, amp), n_nodes, n_ext, m,
                                                _T(es_ctx, k)).cpu().numpy()
            assert got.shape == (n, 5, n_nodes + n_ext)
            for i in range(n):
                _check_amplitudes(f"N={n_nodes} n_ext={n_ext} n={n} m={m} mode {i}", got[i], radius[i], amp[i], n_nodes, m, k[i])


def _problem(ctx, name, N):
    from eigensolver_amd import ShootProblem
    eq, mode, m, _ = cases.all_cases()[name]
    return ShootProblem(dataclasses.replace(eq, r_sign=1.0, n_nodes=N), mode, m, ctx=ctx)


@pytest.fixture(scope="module")
def cf_root(es_ctx):
    """CF_flow_kink on positive radii, 130 nodes, and one accepted root of its grid search (as tests/test_fields_gpu.py)."""
    gp = _problem(es_ctx, "CF_flow_kink", 130)
    k = np.array([1.1])
    Wv = 2.7 + (np.arange(96) + 0.5) * (4.95 - 2.7) / 96
    D, st = gp.eval_grid(k, Wv)
    roots, _ = gp.find_roots(k, Wv, D, st, n_bisect=40, tol_percent=1e-3)
    ok = roots["flag"].cpu().numpy() == 1
    assert ok.any(), "no accepted root in the window"
    yield gp, float(roots["k"].cpu().numpy()[ok][0]), float(roots["w"].cpu().numpy()[ok][0])
    gp.close()


@pytest.fixture(scope="module")
def cf_tables(cf_root):
    """radius [n_r], amp [7, n_r], vort [5, n_r] of the root on the host, 130 + 20 radial points."""
    gp, k, w = cf_root
    d = {a: b.cpu().numpy()[0] for a, b in gp.vorticity_amplitudes([k], [w], n_ext=20).items()}
    assert np.all(np.isfinite(d["amp"])) and d["radius"].shape == (150,)
    return d


def test_vorticity_amplitudes_of_a_real_root(cf_root, cf_tables):
    gp, k, w = cf_root
    _check_amplitudes("CF root", cf_tables["vort"], cf_tables["radius"], cf_tables["amp"], 130, gp.desc.m, k)


def test_a_nan_node_reaches_its_stencil_neighbours_only(es_ctx):
    from eigensolver_amd import shooting
    n_nodes, n_ext, m = 64, 65, 1
    radius, amp, k = _tables(n_nodes, n_ext, 1)
    bad = [2, n_nodes + 30]
    amp[0, :, bad] = np.nan
    got = shooting.vorticity_amplitudes(es_ctx, _T(es_ctx, radius), _T(es_ctx, amp), n_nodes, n_ext, m,
                                        _T(es_ctx, k)).cpu().numpy()[0]
    model = M.vorticity_amplitudes(radius[0], amp[0], n_nodes, m, k[0])
    assert np.array_equal(np.isnan(got), np.isnan(model)) and not np.any(np.isinf(got))
    # node 2 is in the one-sided stencil of node 0 and in the centred ones of 1 .. 3; the exterior node in three
    stencil = sorted([0, 1, 2, 3, n_nodes + 29, n_nodes + 30, n_nodes + 31])
    for c, ch in enumerate(M.VORT_NAMES):
        want = stencil if ch in ("Wphi_C", "Wz_C") else bad
        assert list(np.flatnonzero(np.isnan(got[c]))) == want, ch
        ok = ~np.isnan(model[c])
        assert np.max(np.abs(got[c][ok] - model[c][ok])) <= 1e-10 * np.max(np.abs(model[c][ok]))


# ---- synthesis ----------------------------------------------------------------------------------------------------
def _one_mode(es_ctx, n_nodes=64, n_ext=65, m=1, k=1.3):
    """Host and device tables of one synthetic mode, the vorticity amplitudes from the GPU."""
    from eigensolver_amd import shooting
    radius, amp = M.smooth_table(n_nodes, n_ext)
    d_radius, d_amp = _T(es_ctx, radius), _T(es_ctx, amp)
    d_vort = shooting.vorticity_amplitudes(es_ctx, d_radius[None], d_amp[None], n_nodes, n_ext, m, _T(es_ctx, [k]))[0]
    return radius, amp, d_vort.cpu().numpy(), d_radius, d_amp, d_vort.contiguous()


def _check(tag, got, model, amp, vort, v_scale):
    ref = M.to_f32(model).astype(np.float64)
    bound = M.synthesis_bound(ref, amp, vort, v_scale)
    err = np.abs(got.astype(np.float64) - ref)
    assert got.shape == model.shape and np.all(np.isfinite(got)) and np.all(np.isfinite(ref))
    worst = np.max(err / bound)
    print(f"cart {tag}: max |gpu - model| / bound = {worst:.3f} over {err.size} values")
    assert np.all(err <= bound), (tag, worst)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (5, 3, 2, 1), (64, 2, 1, 2), (257, 3, 2, 2), (66, 6, 3, 1)])
def test_synthesis_matches_the_model(es_ctx, shape):
    import torch
    from eigensolver_amd import shooting
    n_x, n_y, n_z, n_t = shape
    n_nodes, n_ext, k, w, v_scale, fill = 64, 65, 1.3, 3.7, 2.5, -7.5
    x, y = np.linspace(-1.7, 1.9, n_x), np.linspace(-1.6, 1.45, n_y)
    z, t = np.linspace(0.1, 2.3, n_z), np.linspace(0.01, 1.7, n_t)
    d_x, d_y, d_z, d_t = (_T(es_ctx, a) for a in (x, y, z, t))
    for m in (0, 1, 3):
        radius, amp, vort, d_radius, d_amp, d_vort = _one_mode(es_ctx, n_nodes, n_ext, m, k)
        assert M.min_distance_to_region_edges(radius, n_nodes, x, y) > 1e-9
        for mask in (ALL, ["v_x", "vort_y"]):
            model, names, valid = M.synthesis(radius, amp, vort, n_nodes, m, k, w, x, y, z, t, mask, v_scale, fill)
            out, got_names = shooting.cartesian_synthesis(es_ctx, d_radius, d_amp, d_vort, n_nodes, n_ext, m, k, w, d_x,
                                                          d_y, d_z, d_t, mask, v_scale, fill)
            assert got_names == names
            got = out.cpu().numpy()
            # every point is compared: the model carries `fill` where the point is outside the table, and so must the GPU
            assert np.array_equal(got == np.float32(fill), np.broadcast_to(~valid, got.shape))
            _check(f"{shape} m={m} {'all' if mask is ALL else '+'.join(mask)} ({int((~valid).sum())} fill points)", got,
                   model, amp, vort, v_scale)
    # an output that starts 4 bytes past a 16-byte boundary, sentinels on both sides: the same bits
    ref, _ = shooting.cartesian_synthesis(es_ctx, d_radius, d_amp, d_vort, n_nodes, n_ext, 3, k, w, d_x, d_y, d_z, d_t, ALL,
                                          v_scale, fill)
    total = ref.numel()
    buf = torch.full((total + 12,), -777.0, dtype=torch.float32, device=ref.device)
    off = (((4 - buf.data_ptr() % 16) % 16) // 4) % 4 + 4                    # data_ptr of buf[off] = 4 mod 16
    out = buf[off:off + total].view(ref.shape)
    assert out.data_ptr() % 16 == 4
    shooting.cartesian_synthesis(es_ctx, d_radius, d_amp, d_vort, n_nodes, n_ext, 3, k, w, d_x, d_y, d_z, d_t, ALL, v_scale,
                                 fill, out=out)
    assert torch.equal(ref.view(torch.int32), out.view(torch.int32))
    assert bool((buf[:off] == -777.0).all()) and bool((buf[off + total:] == -777.0).all())


def test_synthesis_with_several_planes_per_piece_and_items_per_workgroup(es_ctx):
    """The split every real-size call takes (the reference slice 267 x 267 x 31 x 8 has z_chunk 16, two items per workgroup):
    more than one z plane per piece with a shorter last piece, more than one (frame, piece) item per workgroup with a
    shorter last group -- on a mesh small enough to compare every value with the model."""
    from eigensolver_amd import shooting
    n_x, n_y, n_z, n_t = 73, 70, 137, 3
    s = shooting.cartesian_split(es_ctx, n_x, n_y, n_z, n_t)
    print(f"split of {(n_x, n_y, n_z, n_t)}: {s}")
    assert s["pieces"] == (n_x * n_y + 255) // 256 == 20
    assert s["z_chunk"] > 1 and n_z % s["z_chunk"] != 0 and s["z_parts"] == -(-n_z // s["z_chunk"])
    items = n_t * s["z_parts"]
    assert s["items_per_group"] > 1 and items % s["items_per_group"] != 0 and s["groups"] == -(-items // s["items_per_group"])
    assert s["z_parts"] % 2 == 1                                             # a group straddles two frames
    n_nodes, n_ext, m, k, w, v_scale, fill = 64, 65, 2, 1.3, 3.7, 2.5, -7.5
    x, y = np.linspace(-1.7, 1.9, n_x), np.linspace(-1.6, 1.45, n_y)
    z, t = np.linspace(0.0, 4.0, n_z), np.array([0.01, 0.8, 1.7])
    radius, amp, vort, d_radius, d_amp, d_vort = _one_mode(es_ctx, n_nodes, n_ext, m, k)
    assert M.min_distance_to_region_edges(radius, n_nodes, x, y) > 1e-9
    mask = ["xi_z", "v_x", "vort_y"]
    model, names, valid = M.synthesis(radius, amp, vort, n_nodes, m, k, w, x, y, z, t, mask, v_scale, fill)
    out, got_names = shooting.cartesian_synthesis(es_ctx, d_radius, d_amp, d_vort, n_nodes, n_ext, m, k, w,
                                                  *(_T(es_ctx, a) for a in (x, y, z, t)), mask, v_scale, fill)
    got = out.cpu().numpy()
    assert got_names == names and (~valid).any()
    assert np.array_equal(got == np.float32(fill), np.broadcast_to(~valid, got.shape))
    _check(f"{(n_x, n_y, n_z, n_t)} split {s}", got, model, amp, vort, v_scale)


def test_exact_ties_and_fill(es_ctx):
    from eigensolver_amd import _lib, shooting
    from tests.field_model import AMP_NAMES
    n_nodes, n_ext, m, k, w = 7, 6, 0, 1.0, 2.0
    radius, amp, vort, d_radius, d_amp, d_vort = _one_mode(es_ctx, n_nodes, n_ext, m, k)
    assert radius[n_nodes - 1] == 1.0 == radius[n_nodes] and radius[0] == 0.15 and radius[-1] == 3.0
    x, y = np.array([-1.0, 0.0, 1.0, 0.05, 3.5]), np.array([-1.0, 0.0, 1.0])
    ties = [(1, 0), (1, 2), (0, 1), (2, 1)]                                  # (iy, ix) of (-1, 0), (1, 0), (0, -1), (0, 1)
    outside = [(1, 1), (1, 3), (1, 4), (0, 4), (2, 4)]                       # origin, hole, beyond the far field (three)
    d_x, d_y, d_z, d_t = (_T(es_ctx, a) for a in (x, y, [0.0], [0.0]))
    iz = AMP_NAMES.index("xi_z")
    assert amp[iz, n_nodes - 1] != amp[iz, n_nodes]
    for fill in (np.nan, 0.0, -7.5):
        model, names, valid = M.synthesis(radius, amp, vort, n_nodes, m, k, w, x, y, [0.0], [0.0], None, 1.5, fill)
        assert all(valid[p] for p in ties) and not any(valid[p] for p in outside) and int((~valid).sum()) == len(outside)
        le, _ = shooting.cartesian_synthesis(es_ctx, d_radius, d_amp, d_vort, n_nodes, n_ext, m, k, w, d_x, d_y, d_z, d_t,
                                             None, 1.5, fill)
        be, _ = shooting.cartesian_synthesis(es_ctx, d_radius, d_amp, d_vort, n_nodes, n_ext, m, k, w, d_x, d_y, d_z, d_t,
                                             None, 1.5, fill, flags=_lib.FIELD_BIG_ENDIAN)
        le, be = le.cpu().numpy()[0, :, 0], be.cpu().numpy()[0, :, 0]        # [n_sel, n_y, n_x]
        assert np.array_equal(be.view(np.uint32).byteswap(), le.view(np.uint32))
        fill_bits = np.float32(fill).view(np.uint32)
        for p in outside:
            assert np.all(le[(slice(None),) + p].view(np.uint32) == fill_bits), (fill, p)
        # m = 0, z = t = 0: xi_z is the amplitude itself, rounded once; r == 1 takes the interior's last node
        for p in ties:
            assert le[(names.index("xi_z"),) + p] == np.float32(amp[iz, n_nodes - 1]), p
        ok = np.broadcast_to(valid, le.shape)
        ref = M.to_f32(model[0, :, 0]).astype(np.float64)
        assert np.all(np.isfinite(le[ok]))
        assert np.all(np.abs(le[ok] - ref[ok]) <= M.synthesis_bound(ref, amp, vort, 1.5)[ok])
        if np.isfinite(fill):
            assert np.all(np.isfinite(le)), "the 0/0 at the origin leaked into a finite fill"


def test_masks_are_slices_and_big_endian_is_the_swapped_result(es_ctx):
    from eigensolver_amd import _lib, shooting
    n_nodes, n_ext, m, k, w = 64, 65, 2, 0.8, 2.9
    radius, amp, vort, d_radius, d_amp, d_vort = _one_mode(es_ctx, n_nodes, n_ext, m, k)
    d_x, d_y, d_z, d_t = (_T(es_ctx, a) for a in (np.linspace(-1.7, 1.9, 37), np.linspace(-1.6, 1.45, 5),
                                                   [0.0, 0.7, 1.1], [0.2, 0.9]))
    args = (es_ctx, d_radius, d_amp, d_vort, n_nodes, n_ext, m, k, w, d_x, d_y, d_z, d_t)
    full, names = shooting.cartesian_synthesis(*args, None, 2.0)
    full = full.cpu().numpy()
    assert names == ALL
    for sub in (["P_T"], ["vort_x"], ["xi_y", "vort_z"], ["v_z", "xi_x", "vort_y", "v_x"]):
        got, got_names = shooting.cartesian_synthesis(*args, sub, 2.0)
        assert got_names == [v for v in ALL if v in sub]
        want = full[:, [ALL.index(v) for v in got_names]]
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), sub
    no_vort, _ = shooting.cartesian_synthesis(es_ctx, d_radius, d_amp, None, *args[4:], ["P_T", "v_y"], 2.0)
    assert np.array_equal(no_vort.cpu().numpy().view(np.uint32), full[:, [0, 5]].view(np.uint32))
    be, _ = shooting.cartesian_synthesis(*args, None, 2.0, flags=_lib.FIELD_BIG_ENDIAN)
    assert np.array_equal(be.cpu().numpy().view(np.uint32).byteswap(), full.view(np.uint32))


def test_vorticity_of_gpu_frames_is_the_curl_of_their_velocity(cf_root, cf_tables):
    gp, k, w = cf_root
    x = y = np.linspace(0.2, 0.65, 41)                                       # 0.28 <= r <= 0.92: inside the interior
    z, t = np.linspace(0.0, 0.45, 41), [0.3]
    f = gp.cartesian_fields(k, w, x, y, z, t, variables=M.FD_NAMES, n_ext=20)
    assert f["names"] == M.FD_NAMES and f["frames"].shape == (1, 6, 41, 41, 41)
    e_gpu = M.fd_curl_error(f["frames"][0].cpu().numpy(), M.FD_NAMES, x, y, z)
    radius, amp = cf_tables["radius"], cf_tables["amp"]
    vort = M.vorticity_amplitudes(radius, amp, 130, gp.desc.m, k)
    model, names, valid = M.synthesis(radius, amp, vort, 130, gp.desc.m, k, w, x, y, z, t, M.FD_NAMES)
    assert valid.all()
    e_model = M.fd_curl_error(model[0], names, x, y, z)
    print(f"fd curl of the CF root, 41^3: float32 GPU frames {e_gpu:.3e}, float64 model {e_model:.3e}")
    # the model's error on this mesh stays within what the CPU leg recorded at 41^3 for m = 1 (tests/test_cartesian_model.py,
    # 1.729e-3), so that a worse model cannot widen the bound below
    assert gp.desc.m == 1 and e_model <= 1.729e-3
    assert e_gpu <= 2.0 * e_model


# ---- the Python layer ---------------------------------------------------------------------------------------------
def test_chunked_frames_equal_the_one_call_result(cf_root):
    import torch
    gp, k, w = cf_root
    x, y, z, t = np.linspace(-1.7, 1.9, 9), np.linspace(-1.6, 1.45, 6), np.array([0.01, 1.2]), np.linspace(0.01, 2.0, 3)
    one = gp.cartesian_fields(k, w, x, y, z, t, n_ext=20, fill=0.0)
    chunks = list(gp.cartesian_fields(k, w, x, y, z, t, n_ext=20, fill=0.0, frames_per_call=1))
    assert [c["frames"].shape[0] for c in chunks] == [1, 1, 1]
    assert torch.equal(torch.cat([c["frames"] for c in chunks]).view(torch.int32), one["frames"].view(torch.int32))
    assert torch.equal(torch.cat([c["t"] for c in chunks]), one["t"])
    assert one["names"] == ALL and torch.equal(one["vort_z"], one["frames"][:, ALL.index("vort_z")])
    assert one["frames"].shape == (3, 10, 2, 6, 9) and bool(torch.isfinite(one["frames"]).all())
    # without a vorticity variable the vorticity amplitudes are not needed: the same bits
    few = gp.cartesian_fields(k, w, x, y, z, t, variables=["v_x", "P_T"], n_ext=20, fill=0.0)
    assert few["names"] == ["P_T", "v_x"]
    assert torch.equal(few["v_x"].contiguous().view(torch.int32), one["v_x"].contiguous().view(torch.int32))


def test_rectilinear_frames_parse_back(cf_root, tmp_path):
    from eigensolver_amd import postprocess
    gp, k, w = cf_root
    x, y, z, t = np.linspace(-1.7, 1.9, 9), np.linspace(-1.6, 1.45, 6), np.array([0.01, 1.2]), np.array([0.01, 0.9, 1.4])
    names = ["v_x", "vort_x", "vort_z"]
    plain = gp.cartesian_fields(k, w, x, y, z, t, variables=names, n_ext=20)["frames"].cpu().numpy()
    chunks = gp.cartesian_fields(k, w, x, y, z, t, variables=names, n_ext=20, big_endian=True, frames_per_call=2)
    files = postprocess.write_vtk_rectilinear_frames(str(tmp_path / "cf_cart_"), x, y, z, chunks)
    assert files == [str(tmp_path / "cf_cart_") + f"{i}.vtk" for i in range(3)]
    assert np.isfinite(plain).any()
    for i, path in enumerate(files):
        gx, gy, gz, got = M.read_vtk_rectilinear(path, names)
        assert np.array_equal(gx, x.astype(np.float32)) and np.array_equal(gy, y.astype(np.float32))
        assert np.array_equal(gz, z.astype(np.float32))
        for j, v in enumerate(names):
            assert np.array_equal(got[v].view(np.uint32), plain[i, j].view(np.uint32)), (i, v)


def test_cartesian_fields_reject_slabs_and_negative_radii(es_ctx):
    from eigensolver_amd import ShootProblem
    eq, mode, m, _ = cases.all_cases()["SD_w15_kink"]
    slab = ShootProblem(dataclasses.replace(eq, n_nodes=11), mode, m, ctx=es_ctx)
    eq, mode, m, _ = cases.all_cases()["CF_flow_kink"]
    neg = ShootProblem(dataclasses.replace(eq, n_nodes=11), mode, m, ctx=es_ctx)
    pos = _problem(es_ctx, "CF_flow_kink", 11)
    try:
        for gp, word in ((slab, "cylinders only"), (neg, r"r_sign=\+1")):
            with pytest.raises(ValueError, match=word):
                gp.vorticity_amplitudes([1.0], [3.3], n_ext=4)
            with pytest.raises(ValueError, match=word):
                gp.cartesian_fields(1.0, 3.3, [0.5], [0.0], [0.0], [0.0])
        for n_ext in (1, 2):                                                 # refused before anything is marched
            with pytest.raises(ValueError, match="at least 3 points"):
                pos.vorticity_amplitudes([1.0], [3.3], n_ext=n_ext)
            with pytest.raises(ValueError, match="at least 3 points"):
                pos.cartesian_fields(1.0, 3.3, [0.5], [0.0], [0.0], [0.0], n_ext=n_ext)
        with pytest.raises(ValueError, match="unknown Cartesian field variable"):
            pos.cartesian_fields(1.0, 3.3, [0.5], [0.0], [0.0], [0.0], variables=["xi_r"])
        with pytest.raises(ValueError, match="one root"):
            pos.cartesian_fields([1.0, 1.1], [3.3, 3.4], [0.5], [0.0], [0.0], [0.0])
        with pytest.raises(ValueError, match="frames_per_call"):
            pos.cartesian_fields(1.0, 3.3, [0.5], [0.0], [0.0], [0.0], frames_per_call=0)
    finally:
        for gp in (slab, neg, pos):
            gp.close()


# ---- the C interface: argument errors and empty calls -----------------------------------------------------------------
def test_argument_errors_and_empty_calls(es_ctx):
    import torch
    lib, h = es_ctx.lib, es_ctx.handle
    dev = f"cuda:{es_ctx.device}"
    N, n_ext, n_x, n_y, n_z, n_t = 4, 3, 5, 3, 2, 2
    n_r = N + n_ext
    d = lambda *s: torch.ones(s, dtype=torch.float64, device=dev)            # noqa: E731
    radius = torch.tensor([0.2, 0.5, 0.8, 1.0, 1.0, 2.0, 3.0], dtype=torch.float64, device=dev)
    amp, vort, kk = d(7, n_r), d(5, n_r), d(1)
    x, y, z, t = torch.linspace(-1.5, 1.5, n_x, dtype=torch.float64, device=dev), d(n_y) * 0.3, d(n_z), d(n_t)
    out = torch.full((n_t * 10 * n_z * n_y * n_x,), -5.0, dtype=torch.float32, device=dev)
    vout = torch.full((5, n_r), -77.0, dtype=torch.float64, device=dev)   # (-m / r is -5 at r = 0.2)
    P = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None        # noqa: E731

    def syn(rad=radius, amp_=amp, vort_=vort, N_=N, n_ext_=n_ext, m=1, x_=x, n_x_=n_x, y_=y, n_y_=n_y, z_=z, n_z_=n_z, t_=t,
            n_t_=n_t, mask=0x3ff, flags=0, out_=out, out_off=0):
        po = C.c_void_p(out_.data_ptr() + out_off) if out_ is not None else None
        return lib.es_cyl_cartesian_synthesis(h, P(rad), P(amp_), P(vort_), N_, n_ext_, m, 1.0, 2.0, P(x_), n_x_, P(y_), n_y_,
                                              P(z_), n_z_, P(t_), n_t_, mask, 1.0, float("nan"), flags, po)

    def amps(rad=radius, amp_=amp, n=1, N_=N, n_ext_=n_ext, m=1, k_=kk, v=vout):
        return lib.es_cyl_vorticity_amplitudes(h, P(rad), P(amp_), n, N_, n_ext_, m, P(k_), P(v))

    for bad in (dict(mask=0), dict(mask=1 << 10), dict(vort_=None), dict(vort_=None, mask=1 << 9), dict(flags=2),
                dict(flags=2 | 4), dict(flags=1), dict(flags=8), dict(N_=2, n_ext_=5), dict(N_=5, n_ext_=2),
                dict(N_=0, n_ext_=0), dict(N_=-1), dict(n_ext_=-1), dict(n_x_=-1), dict(n_y_=-1), dict(n_z_=-1),
                dict(n_t_=-1), dict(m=-1), dict(out_off=2), dict(rad=None), dict(amp_=None), dict(x_=None), dict(y_=None),
                dict(z_=None), dict(t_=None), dict(out_=None)):
        assert syn(**bad) == 1, bad
    assert b"invalid argument" in lib.es_last_error(h)
    for bad in (dict(n=-1), dict(N_=-1), dict(n_ext_=-1), dict(m=-1), dict(N_=2, n_ext_=5), dict(N_=5, n_ext_=2),
                dict(N_=1, n_ext_=0), dict(rad=None), dict(amp_=None), dict(k_=None), dict(v=None)):
        assert amps(**bad) == 1, bad
    assert b"invalid argument" in lib.es_last_error(h)
    # empty calls succeed and write nothing
    for empty in (dict(n_x_=0), dict(n_y_=0), dict(n_z_=0), dict(n_t_=0), dict(n_t_=0, t_=None, out_=None),
                  dict(n_x_=0, x_=None)):
        assert syn(**empty) == 0, empty
    assert amps(n=0) == 0 and amps(n=0, rad=None, amp_=None, k_=None, v=None) == 0 and amps(N_=0, n_ext_=0) == 0
    es_ctx.synchronize()
    assert bool((out == -5.0).all()) and bool((vout == -77.0).all())
    assert syn(vort_=None, mask=0x7f) == 0 and amps() == 0 and amps(N_=0, n_ext_=n_r) == 0 and amps(N_=n_r, n_ext_=0) == 0
    assert syn() == 0
    es_ctx.synchronize()
    assert bool((out != -5.0).all()) and bool((vout != -77.0).all())
