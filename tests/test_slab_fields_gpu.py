"""Perturbation fields of a slab mode on the GPU (include/eigensolver_amd.h section 9) against the NumPy restatement
tests/slab_field_model.py, which tests/test_slab_field_model.py pins on the oracle's eigenfunctions and on kinematics.

Bounds, none of them measured on the kernels:
  amplitudes   1e-10 of each channel's max |A|, the project's bound for a kernel against a NumPy restatement of the same
               expressions (sections 7 and 8).  Every case first asserts E_round = max |model(float64) - model(longdouble)|
               <= 1e-11 of the channel's max, so that the model's own rounding is well below the bound.
  frames       |gpu - model| <= 2^-23 |model| + 1e-12 max|A| max e^{w_im t}, A as the synthesis scales it.  Every mesh
               point is compared; x is an input of both sides, so the region and the bracket are the same comparisons.
Every check prints its measured figure with `pytest -s`.  On an MI355X: the amplitudes are within 1.6e-4 of their bound
on every case (worst: P_T of the unstable sfg pair with the shear term, 1.8e-13 on a channel of max 11; the model's own
rounding is 1.0e-13 there); the frames sit at 0.000 of their bound (the model is rounded to float32 as well); the envelopes
of the frames of the unstable pair grow by e^{Im w t} to within 5e-4."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import slab_field_model as M  # noqa: E402
from tests import cases  # noqa: E402

ALL = list(M.SVAR_NAMES)
DENSITY_KW, FLOW_KW = (1.5, 1.65), (1.2, 1.92)                              # (k, omega) of the two families


def _T(es_ctx, a, dtype=np.float64):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=f"cuda:{es_ctx.device}")


def _eq(family, n_nodes):
    from eigensolver_amd import equilibrium as q
    if family == "density":
        return q.SlabDensity(width=0.9, n_nodes=n_nodes), DENSITY_KW
    return q.SlabFlow(width=0.9, U_i0=0.35, n_nodes=n_nodes), FLOW_KW


def _model_rows(eq, mode, k, w, eig, shear, dtype=np.float64):
    """The model on the host copies of an eigenfunction dict: list of (x, amp) per pair."""
    from eigensolver_amd import shooting
    prof = shooting.slab_field_profiles(eq)
    e = {a: b.cpu().numpy() for a, b in eig.items() if a != "status"}
    k = np.broadcast_to(np.asarray(k, dtype=float).reshape(-1), (e["value_int"].shape[0],))
    w = np.asarray(w).reshape(-1)
    sigma = -1.0 if mode == "sausage" else 1.0
    return [M.polarisation(k[i], w[i], e["value_int"][i], e["flux_int"][i], e["x_ext"][i], e["value_ext"][i],
                           e["flux_ext"][i], prof, eq.rho_e, eq.vA_e, eq.c_e, eq.U_e, sigma, shear=shear, dtype=dtype)
            for i in range(len(w))]


def _check_amplitudes(tag, got_x, got, x64, a64, ald):
    assert np.array_equal(got_x, x64), tag
    assert np.all(np.isfinite(a64)), f"{tag}: the model itself is not finite"
    for c, ch in enumerate(M.SAMP_NAMES):
        scale = np.max(np.abs(a64[c]))
        e_round = float(np.max(np.abs(a64[c] - ald[c])))
        err = float(np.max(np.abs(got[c] - a64[c])))
        print(f"slab amp {tag} {ch:6s}: err {err:.3e} bound {1e-10 * scale:.3e}   E_round {e_round:.3e} bound {1e-11 * scale:.3e}")
        assert scale > 0 and e_round <= 1e-11 * scale, (tag, ch, e_round, scale)
        assert err <= 1e-10 * scale, (tag, ch, err, scale)


# ---- amplitudes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sausage", "kink"])
@pytest.mark.parametrize("family", ["density", "flow"])
def test_amplitudes_match_the_model(es_ctx, family, mode):
    from eigensolver_amd import ShootProblem, shooting
    for n_nodes in (11, 64):
        eq, (k, w) = _eq(family, n_nodes)
        gp = ShootProblem(eq, mode, ctx=es_ctx)
        try:
            for n_ext in (0, 3, 20):
                eig = gp.eigenfunction([k], [w], n_ext=n_ext)
                for quirks in (True, False):
                    tab = gp.slab_polarisation([k], [w], n_ext=n_ext, reference_quirks=quirks)
                    assert tab["x"].shape == (1, 2 * n_ext + n_nodes) and tab["amp"].shape == (1, 6, 2 * n_ext + n_nodes)
                    got = tab["amp"].cpu().numpy()[0]
                    (x64, a64), = _model_rows(eq, mode, k, w, eig, not quirks)
                    (_, ald), = _model_rows(eq, mode, k, w, eig, not quirks, dtype=np.longdouble)
                    _check_amplitudes(f"{family} {mode} N={n_nodes} n_ext={n_ext} shear={not quirks}",
                                      tab["x"].cpu().numpy()[0], got, x64, a64, ald)
                    # a real mode: v_x and xi_z go with cos(k z - w t), xi_x, P_T and v_z with -/+ sin
                    names = M.SAMP_NAMES
                    for ch in ("v_x", "xi_z"):
                        assert np.all(got[names.index(ch)].imag == 0.0), ch
                    for ch in ("xi_x", "P_T", "v_z"):
                        assert np.all(got[names.index(ch)].real == 0.0), ch
                    if family == "flow" and not quirks:                      # the flag matters where U' does not vanish
                        plain = gp.slab_polarisation([k], [w], n_ext=n_ext)["amp"].cpu().numpy()[0]
                        assert np.max(np.abs(plain[2] - got[2])) > 1e-3 * np.max(np.abs(got[2]))
        finally:
            gp.close()
    assert shooting.slab_var_mask(None)[1] == ALL


def test_a_leaky_row_is_nan_and_its_neighbour_is_unaffected(es_ctx):
    from eigensolver_amd import ShootProblem
    from eigensolver_amd.shooting import PT_LEAKY, PT_OK
    eq, (k, w) = _eq("density", 64)
    gp = ShootProblem(eq, "kink", ctx=es_ctx)
    try:
        ks, ws = [k, k], [1.1, w]
        st = gp.eval_points(ks, ws)[1].cpu().numpy()
        assert list(st) == [PT_LEAKY, PT_OK]
        two = gp.slab_polarisation(ks, ws, n_ext=20)
        one = gp.slab_polarisation([k], [w], n_ext=20)
        amp = two["amp"].cpu().numpy()
        # every amplitude of the leaky row is a complex NaN; of a real mode the part that is identically zero stays zero
        assert np.all(np.isnan(amp[0])) and np.all(np.isnan(amp[0].real) | (amp[0].real == 0.0))
        assert np.all(np.isnan(amp[0].imag) | (amp[0].imag == 0.0))
        nan_frames = gp.slab_fields(k, 1.1, [-2.0, 0.0, 0.5], [0.0, 0.3], [0.0, 1.0], n_ext=20, fill=0.0)["frames"]
        assert bool(nan_frames.isnan().all())                                # and so is every value synthesised from it
        assert np.array_equal(amp[1].view(np.float64), one["amp"].cpu().numpy()[0].view(np.float64))
        x = two["x"].cpu().numpy()
        R = eq.L_factor * 2.0 * np.pi / k
        assert np.all(np.isfinite(x)) and np.all(np.diff(x, axis=1) >= 0) and np.allclose(x[:, [0, -1]], [-R, R], rtol=1e-15)
        assert np.array_equal(x[0], x[1])
    finally:
        gp.close()


def _complex_pair(s, mode, k):
    """The first of the points tests/test_complex_roots_gpu.py evaluates at k = 0.5 that is ES_PT_OK with Im omega != 0."""
    w = np.array([0.2 + 0.1j, 0.35 - 0.05j, 0.1 + 0.2j, 0.5 + 0.02j])
    st = s.eval_points(mode, k, w)[1].cpu().numpy()
    ok = [z for z, f in zip(w, st) if f == 0 and z.imag != 0.0]
    assert ok, st
    return complex(ok[0])


@pytest.mark.parametrize("variant", ["sfx", "sfg"])
def test_amplitudes_of_an_unstable_pair(es_ctx, variant):
    from eigensolver_amd import SlabComplexFlow
    s = SlabComplexFlow(width=0.9, variant=variant, n_nodes=64, ctx=es_ctx)
    try:
        k = 0.5
        w = _complex_pair(s, "kink", k)
        eig = s.eigenfunction("kink", k, [w], n_ext=20)
        assert int(eig["status"][0]) == 0
        for quirks in ((True,) if variant == "sfx" else (True, False)):
            tab = s.polarisation("kink", k, [w], n_ext=20, reference_quirks=quirks)
            assert int(tab["status"][0]) == 0
            (x64, a64), = _model_rows(s.eq, "kink", k, [w], eig, not quirks)
            (_, ald), = _model_rows(s.eq, "kink", k, [w], eig, not quirks, dtype=np.longdouble)
            got = tab["amp"].cpu().numpy()[0]
            _check_amplitudes(f"{variant} kink w={w} shear={not quirks}", tab["x"].cpu().numpy()[0], got, x64, a64, ald)
            assert np.max(np.abs(got[M.SAMP_NAMES.index("v_x")].imag)) > 0      # the phase tilts: a complex amplitude
        if variant == "sfx":
            with pytest.raises(ValueError, match="sfx"):
                s.polarisation("kink", k, [w], n_ext=20, reference_quirks=False)
            with pytest.raises(ValueError, match="sfx"):
                s.fields("kink", k, w, [0.0], [0.0], [0.0], reference_quirks=False)
    finally:
        s.close()


def test_a_nan_node_reaches_its_stencil_neighbours_only(es_ctx):
    from eigensolver_amd import shooting
    N, n_ext, k, w = 11, 7, 1.2, 1.9 + 0.15j
    m = M.smooth_mode(N, n_ext)
    for name in ("V_ext", "Pf_ext"):
        m[name][-1] = np.nan
    for name in ("V_int", "Pf_int"):
        m[name][4] = np.nan
    eig = dict(value_int=_T(es_ctx, m["V_int"][None], complex), flux_int=_T(es_ctx, m["Pf_int"][None], complex),
               x_ext=_T(es_ctx, m["x_ext"][None]), value_ext=_T(es_ctx, m["V_ext"][None], complex),
               flux_ext=_T(es_ctx, m["Pf_ext"][None], complex))
    prof = {a: _T(es_ctx, b) for a, b in m["prof"].items()}
    tab = shooting.slab_polarisation(es_ctx, _T(es_ctx, [k]), _T(es_ctx, [w.real]), _T(es_ctx, [w.imag]), eig, prof,
                                     m["rho_e"], m["vA_e"], m["c_e"], m["U_e"], 1, shooting._lib.SLAB_FIELD_SHEAR_PT)
    got = tab["amp"].cpu().numpy()[0]
    x, model = M.polarisation(k, w, m["V_int"], m["Pf_int"], m["x_ext"], m["V_ext"], m["Pf_ext"], m["prof"], m["rho_e"],
                              m["vA_e"], m["c_e"], m["U_e"], 1.0, shear=True)
    assert np.array_equal(np.isnan(got), np.isnan(model)) and not np.any(np.isinf(got.real) | np.isinf(got.imag))
    stencil = [n_ext - 2, n_ext - 1, n_ext + 3, n_ext + 4, n_ext + 5, n_ext + N, n_ext + N + 1]
    assert list(np.flatnonzero(np.isnan(got[5]))) == stencil
    assert list(np.flatnonzero(np.isnan(got[4]))) == [n_ext - 1, n_ext + 4, n_ext + N]
    for c in range(6):
        ok = ~np.isnan(model[c])
        assert np.max(np.abs(got[c][ok] - model[c][ok])) <= 1e-10 * np.max(np.abs(model[c][ok]))


# ---- frames -------------------------------------------------------------------------------------------------------
K, W, V_SCALE, FILL = 1.2, 1.9 + 0.15j, 2.5, -7.5
N_NODES, N_EXT = 33, 20


@pytest.fixture(scope="module")
def table(es_ctx):
    """A synthetic complex table (non-uniform exteriors, kink) on the host and on the device."""
    x, amp, _ = M.smooth_table(N_NODES, N_EXT, k=K, w=W)
    return x, amp, _T(es_ctx, x), _T(es_ctx, amp, complex)


def _mesh(xt, n_x, n_z, n_t):
    """x over [-1.1 R, 1.1 R] with -R, -1, +1, R exactly, a NaN, and points beyond R on both sides."""
    R = xt[-1]
    x = np.linspace(-1.1 * R, 1.1 * R, n_x)
    x[[5, 17, 29, 41, 50]] = [-1.0, R, np.nan, 1.0, -R]
    assert np.sum(np.abs(x) > R) >= 4
    return x, np.linspace(0.1, 2.3, n_z), np.linspace(0.01, 1.7, n_t)


def _check_frames(tag, got, model, amp, w, t):
    ref = M.to_f32(model).astype(np.float64)
    bound = M.synthesis_bound(ref, amp, V_SCALE, w, t)
    err = np.abs(got.astype(np.float64) - ref)
    assert got.shape == model.shape and np.all(np.isfinite(got)) and np.all(np.isfinite(ref))
    worst = np.max(err / bound)
    print(f"slab frames {tag}: max |gpu - model| / bound = {worst:.3f} over {err.size} values")
    assert np.all(err <= bound), (tag, worst)


@pytest.mark.parametrize("n_x", [64, 73, 261])
def test_frames_match_the_model(es_ctx, table, n_x):
    import torch
    from eigensolver_amd import shooting
    xt, amp, d_xt, d_amp = table
    for n_z, n_t in ((1, 1), (5, 3), (1, 3), (5, 1)):
        x, z, t = _mesh(xt, n_x, n_z, n_t)
        d_x, d_z, d_t = (_T(es_ctx, a) for a in (x, z, t))
        for mask in (ALL, ["xi_z", "v_x", "vort_y"]):
            model, names, valid = M.synthesis(xt, amp, N_NODES, N_EXT, K, W, x, z, t, mask, V_SCALE, FILL)
            out, got_names = shooting.slab_field_synthesis(es_ctx, d_xt, d_amp, N_NODES, N_EXT, K, W, d_x, d_z, d_t, mask,
                                                           V_SCALE, FILL)
            assert got_names == names and out.shape == (n_t, len(names), n_z, n_x)
            got = out.cpu().numpy()
            assert (~valid).sum() >= 5 and valid[[5, 17, 41, 50]].all() and not valid[29]
            assert np.array_equal(got == np.float32(FILL), np.broadcast_to(~valid, got.shape))
            _check_frames(f"n_x={n_x} n_z={n_z} n_t={n_t} {'all' if mask is ALL else '+'.join(mask)}", got, model, amp, W, t)
    # an output that starts 4 bytes past a 16-byte boundary, sentinels on both sides: the same bits by the 4-byte stores
    ref, _ = shooting.slab_field_synthesis(es_ctx, d_xt, d_amp, N_NODES, N_EXT, K, W, d_x, d_z, d_t, ALL, V_SCALE, FILL)
    total = ref.numel()
    buf = torch.full((total + 12,), -777.0, dtype=torch.float32, device=ref.device)
    off = (((4 - buf.data_ptr() % 16) % 16) // 4) % 4 + 4                   # data_ptr of buf[off] = 4 mod 16
    out = buf[off:off + total].view(ref.shape)
    assert out.data_ptr() % 16 == 4
    shooting.slab_field_synthesis(es_ctx, d_xt, d_amp, N_NODES, N_EXT, K, W, d_x, d_z, d_t, ALL, V_SCALE, FILL, out=out)
    assert torch.equal(ref.view(torch.int32), out.view(torch.int32))
    assert bool((buf[:off] == -777.0).all()) and bool((buf[off + total:] == -777.0).all())


def test_rows_shared_among_workgroups_cross_frames(es_ctx, table):
    """More rows than row groups, so that a workgroup walks several rows and a group straddles two frames."""
    from eigensolver_amd import shooting
    xt, amp, d_xt, d_amp = table
    n_x, n_z, n_t = 300, 701, 3                                              # 2 column chunks -> 1052 groups of 2 rows
    x = np.linspace(-1.05 * xt[-1], 1.05 * xt[-1], n_x)
    z, t = np.linspace(0.0, 3.0, n_z), np.linspace(0.0, 1.1, n_t)
    mask = ["P_T", "v_z"]
    model, names, valid = M.synthesis(xt, amp, N_NODES, N_EXT, K, W, x, z, t, mask, V_SCALE, FILL)
    out, _ = shooting.slab_field_synthesis(es_ctx, d_xt, d_amp, N_NODES, N_EXT, K, W, *(_T(es_ctx, a) for a in (x, z, t)),
                                           mask, V_SCALE, FILL)
    got = out.cpu().numpy()
    rows = -(-(n_z * n_t) // min(n_z * n_t, -(-4096 // -(-n_x // 256))))     # the split of es_slab_field_synthesis
    assert rows == 2 and (n_z * n_t) % rows != 0 and n_z % rows != 0 and (~valid).any()
    assert np.array_equal(got == np.float32(FILL), np.broadcast_to(~valid, got.shape))
    _check_frames(f"{(n_x, n_z, n_t)}", got, model, amp, W, t)


def test_exact_ties_and_fill(es_ctx, table):
    from eigensolver_amd import _lib, shooting
    xt, amp, d_xt, d_amp = table
    R = xt[-1]
    x = np.array([-R, -1.0, 1.0, R, np.nextafter(R, np.inf), np.nextafter(-R, -np.inf), np.nan, 0.3])
    d_x, d_z, d_t = (_T(es_ctx, a) for a in (x, [0.0], [0.0]))
    a = amp[M.SAMP_NAMES.index("xi_z")].real
    assert a[N_EXT - 1] != a[N_EXT] and a[N_EXT + N_NODES - 1] != a[N_EXT + N_NODES]
    for fill in (np.nan, 0.0, -7.5):
        le, names = shooting.slab_field_synthesis(es_ctx, d_xt, d_amp, N_NODES, N_EXT, K, W, d_x, d_z, d_t, None, 1.0, fill)
        be, _ = shooting.slab_field_synthesis(es_ctx, d_xt, d_amp, N_NODES, N_EXT, K, W, d_x, d_z, d_t, None, 1.0, fill,
                                              flags=_lib.FIELD_BIG_ENDIAN)
        le, be = le.cpu().numpy()[0, :, 0], be.cpu().numpy()[0, :, 0]        # [n_sel, n_x]
        assert np.array_equal(be.view(np.uint32).byteswap(), le.view(np.uint32))
        assert np.all(le[:, 4:7].view(np.uint32) == np.float32(fill).view(np.uint32)), fill
        # z = t = 0: the value is Re A rounded once; x = -1 and +1 take the interior's nodes, -R and R the exteriors' ends
        want = np.array([a[0], a[N_EXT], a[N_EXT + N_NODES - 1], a[-1]]).astype(np.float32)
        assert np.array_equal(le[names.index("xi_z"), :4], want)
        assert np.all(np.isfinite(le[:, [0, 1, 2, 3, 7]]))
    # without exteriors everything outside [-1, 1] is fill
    d_xi, d_ai = d_xt[N_EXT:N_EXT + N_NODES].contiguous(), d_amp[:, N_EXT:N_EXT + N_NODES].contiguous()
    out, _ = shooting.slab_field_synthesis(es_ctx, d_xi, d_ai, N_NODES, 0, K, W, d_x, d_z, d_t, None, 1.0, -7.5)
    out = out.cpu().numpy()[0, :, 0]
    assert np.all(out[:, [0, 3, 4, 5, 6]] == np.float32(-7.5)) and np.all(out[:, [1, 2, 7]] != np.float32(-7.5))
    assert np.array_equal(out[1, 1:3], want[1:3])


def test_masks_are_slices_and_big_endian_is_the_swapped_result(es_ctx, table):
    from eigensolver_amd import _lib, shooting
    xt, amp, d_xt, d_amp = table
    x, z, t = _mesh(xt, 64, 3, 2)
    args = (es_ctx, d_xt, d_amp, N_NODES, N_EXT, K, W, *(_T(es_ctx, a) for a in (x, z, t)))
    full, names = shooting.slab_field_synthesis(*args, None, 2.0, FILL)
    full = full.cpu().numpy()
    assert names == ALL
    for sub in (["P_T"], ["vort_y"], ["xi_z", "v_x"], ["v_z", "xi_x", "vort_y", "v_x"]):
        got, got_names = shooting.slab_field_synthesis(*args, sub, 2.0, FILL)
        assert got_names == [v for v in ALL if v in sub]
        want = full[:, [ALL.index(v) for v in got_names]]
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), sub
    be, _ = shooting.slab_field_synthesis(*args, None, 2.0, FILL, flags=_lib.FIELD_BIG_ENDIAN)
    assert np.array_equal(be.cpu().numpy().view(np.uint32).byteswap(), full.view(np.uint32))
    # v_scale multiplies v_x, v_z and vort_y and nothing else
    unit, _ = shooting.slab_field_synthesis(*args, None, 1.0, FILL)
    unit = unit.cpu().numpy()
    for i, v in enumerate(ALL):
        same = np.array_equal(unit[:, i].view(np.uint32), full[:, i].view(np.uint32))
        assert same == (v not in M.SCALED), v
        ok = unit[:, i] != np.float32(FILL)
        if v in M.SCALED:                                                    # a power of two scales exactly
            assert np.array_equal(full[:, i][ok], 2.0 * unit[:, i][ok])


# ---- the Python layer ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def density_root(es_ctx):
    from eigensolver_amd import ShootProblem
    eq, (k, w) = _eq("density", 64)
    gp = ShootProblem(eq, "kink", ctx=es_ctx)
    yield gp, k, w
    gp.close()


def test_slab_fields_of_a_real_mode(density_root):
    import torch
    gp, k, w = density_root
    R = gp.eq.L_factor * 2.0 * np.pi / k
    x, z, t = np.linspace(-1.2 * R, 1.2 * R, 37), np.array([0.0, 0.4, 1.1]), np.linspace(0.0, 2.0, 5)
    one = gp.slab_fields(k, w, x, z, t, n_ext=20, fill=0.0, v_scale=V_SCALE)
    assert one["names"] == ALL and one["frames"].shape == (5, 6, 3, 37) and bool(torch.isfinite(one["frames"]).all())
    assert torch.equal(one["vort_y"], one["frames"][:, ALL.index("vort_y")])
    chunks = list(gp.slab_fields(k, w, x, z, t, n_ext=20, fill=0.0, v_scale=V_SCALE, frames_per_call=2))
    assert [c["frames"].shape[0] for c in chunks] == [2, 2, 1]
    assert torch.equal(torch.cat([c["frames"] for c in chunks]).view(torch.int32), one["frames"].view(torch.int32))
    assert torch.equal(torch.cat([c["t"] for c in chunks]), one["t"])
    # against the model on the table the GPU made
    tab = gp.slab_polarisation([k], [w], n_ext=20)
    xt, amp = tab["x"].cpu().numpy()[0], tab["amp"].cpu().numpy()[0]
    model, names, valid = M.synthesis(xt, amp, 64, 20, k, w, x, z, t, None, V_SCALE, 0.0)
    assert (~valid).sum() >= 2
    _check_frames("density root", one["frames"].cpu().numpy(), model, amp, w, t)
    few = gp.slab_fields(k, w, x, z, t, variables=["v_x", "P_T"], n_ext=20, fill=0.0, v_scale=V_SCALE)
    assert few["names"] == ["P_T", "v_x"]
    assert torch.equal(few["v_x"].contiguous().view(torch.int32), one["v_x"].contiguous().view(torch.int32))


def test_fields_of_an_unstable_mode_grow_and_parse_back_from_vtk(es_ctx, tmp_path):
    import torch
    from eigensolver_amd import SlabComplexFlow, postprocess
    s = SlabComplexFlow(width=0.9, variant="sfx", n_nodes=64, ctx=es_ctx)
    try:
        k = 0.5
        w = _complex_pair(s, "kink", k)
        x, z, t = np.linspace(-3.0, 3.0, 21), np.linspace(0.0, 2.0 * np.pi / k, 65), np.array([0.0, 0.9, 2.0])
        names = ["xi_x", "v_z", "vort_y"]
        plain = s.fields("kink", k, w, x, z, t, variables=names, n_ext=20)
        assert plain["names"] == names and plain["frames"].shape == (3, 3, 65, 21)
        tab = s.polarisation("kink", k, [w], n_ext=20)
        xt, amp = tab["x"].cpu().numpy()[0], tab["amp"].cpu().numpy()[0]
        model, _, valid = M.synthesis(xt, amp, 64, 20, k, w, x, z, t, names, 1.0)
        assert valid.all()
        got = plain["frames"].cpu().numpy()
        ref = M.to_f32(model).astype(np.float64)
        assert np.all(np.abs(got - ref) <= M.synthesis_bound(ref, amp, 1.0, w, t))
        # a later frame is the first one grown by e^{Im w t} and shifted in phase: the maxima over a wavelength sampled at
        # 64 points (each within 1 - cos(pi / 64) = 1.2e-3 of the envelope) grow by that factor
        env = np.max(np.abs(got.astype(np.float64)), axis=(2, 3))             # [n_t, n_sel]
        grow = np.exp(w.imag * (t[1:] - t[0]))[:, None]
        print(f"growth of the envelopes over e^(Im w t): {np.array2string(env[1:] / env[0] / grow, precision=5)}")
        assert np.all(np.abs(env[1:] / env[0] / grow - 1.0) <= 2.5e-3)
        chunks = s.fields("kink", k, w, x, z, t, variables=names, n_ext=20, big_endian=True, frames_per_call=2)
        files = postprocess.write_vtk_rectilinear_frames(str(tmp_path / "kh_"), x, [0.0], z, chunks)
        assert files == [str(tmp_path / "kh_") + f"{i}.vtk" for i in range(3)]
        for i, path in enumerate(files):
            gx, gy, gz, back = M.read_vtk_rectilinear(path, names)
            assert np.array_equal(gx, x.astype(np.float32)) and np.array_equal(gy, np.zeros(1, np.float32))
            assert np.array_equal(gz, z.astype(np.float32))
            for j, v in enumerate(names):
                assert np.array_equal(back[v][:, 0].view(np.uint32), got[i, j].view(np.uint32)), (i, v)
        assert torch.equal(plain["v_z"], plain["frames"][:, 1])
    finally:
        s.close()


# ---- argument errors ----------------------------------------------------------------------------------------------
def test_python_argument_errors(es_ctx, density_root):
    from eigensolver_amd import ShootProblem
    gp, k, w = density_root
    eq, mode, m, _ = cases.all_cases()["CF_flow_kink"]
    cyl = ShootProblem(dataclasses.replace(eq, r_sign=1.0, n_nodes=11), mode, m, ctx=es_ctx)
    try:
        with pytest.raises(ValueError, match="slab equilibria only"):
            cyl.slab_polarisation([1.0], [3.3], n_ext=4)
        with pytest.raises(ValueError, match="slab equilibria only"):
            cyl.slab_fields(1.0, 3.3, [0.5], [0.0], [0.0])
    finally:
        cyl.close()
    for n_ext in (1, 2):                                                     # refused before anything is marched
        with pytest.raises(ValueError, match="at least 3 points"):
            gp.slab_polarisation([k], [w], n_ext=n_ext)
        with pytest.raises(ValueError, match="at least 3 points"):
            gp.slab_fields(k, w, [0.5], [0.0], [0.0], n_ext=n_ext)
    with pytest.raises(ValueError, match="unknown slab field variable"):
        gp.slab_fields(k, w, [0.5], [0.0], [0.0], variables=["xi_r"])
    with pytest.raises(ValueError, match="empty list of slab field variables"):
        gp.slab_fields(k, w, [0.5], [0.0], [0.0], variables=[])
    with pytest.raises(ValueError, match="one root"):
        gp.slab_fields([k, k], [w, w], [0.5], [0.0], [0.0])
    with pytest.raises(ValueError, match="frames_per_call"):
        gp.slab_fields(k, w, [0.5], [0.0], [0.0], frames_per_call=0)


def test_c_argument_errors_and_empty_calls(es_ctx):
    import torch
    lib, h = es_ctx.lib, es_ctx.handle
    dev = f"cuda:{es_ctx.device}"
    from eigensolver_amd import _lib
    N, n_ext, n_x, n_z, n_t = 4, 3, 5, 2, 2
    n_tab = N + 2 * n_ext
    d = lambda *s: torch.ones(s, dtype=torch.float64, device=dev)            # noqa: E731
    xtab = torch.tensor([-3.0, -2.0, -1.0, -1.0, -0.3, 0.3, 1.0, 1.0, 2.0, 3.0], dtype=torch.float64, device=dev)
    amp = d(6, n_tab, 2)
    x, z, t = torch.linspace(-2.5, 2.5, n_x, dtype=torch.float64, device=dev), d(n_z), d(n_t)
    out = torch.full((n_t * 6 * n_z * n_x,), -5.0, dtype=torch.float32, device=dev)
    P = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None        # noqa: E731

    def syn(xt=xtab, amp_=amp, N_=N, n_ext_=n_ext, x_=x, n_x_=n_x, z_=z, n_z_=n_z, t_=t, n_t_=n_t, mask=0x3f, flags=0,
            out_=out, out_off=0):
        po = C.c_void_p(out_.data_ptr() + out_off) if out_ is not None else None
        return lib.es_slab_field_synthesis(h, P(xt), P(amp_), N_, n_ext_, 1.0, 2.0, 0.1, P(x_), n_x_, P(z_), n_z_, P(t_), n_t_,
                                           mask, 1.0, float("nan"), flags, po)

    # a table that does not match (n_nodes, n_ext) cannot be seen by the C call (it gets no length): the Python layer checks
    from eigensolver_amd import shooting
    with pytest.raises(ValueError, match="does not match the table"):
        shooting.slab_field_synthesis(es_ctx, xtab, torch.view_as_complex(amp), N + 1, n_ext, 1.0, 2.0, x, z, t)
    with pytest.raises(ValueError, match="does not match the table"):
        shooting.slab_field_synthesis(es_ctx, xtab, torch.view_as_complex(amp), N, n_ext + 1, 1.0, 2.0, x, z, t)
    for bad in (dict(mask=0), dict(mask=1 << 6), dict(flags=1), dict(flags=2), dict(flags=8), dict(n_ext_=1), dict(n_ext_=2),
                dict(N_=2), dict(N_=0), dict(N_=-1), dict(n_ext_=-1), dict(n_x_=-1), dict(n_z_=-1), dict(n_t_=-1),
                dict(out_off=2), dict(xt=None), dict(amp_=None), dict(x_=None), dict(z_=None), dict(t_=None),
                dict(out_=None)):
        assert syn(**bad) == 1, bad
    assert b"invalid argument" in lib.es_last_error(h)

    kk, wre, wim = d(1), d(1) * 2.0, d(1) * 0.1
    iv, ifl, ex, ev, ef = d(1, N), d(1, N), xtab[:n_ext].reshape(1, n_ext).contiguous(), d(1, n_ext), d(1, n_ext)
    prof = [d(N) for _ in range(5)]
    fp = _lib.SlabFieldProfiles(*[a.data_ptr() for a in prof])
    xo = torch.full((1, n_tab), -77.0, dtype=torch.float64, device=dev)
    ao = torch.full((1, 6, n_tab, 2), -77.0, dtype=torch.float64, device=dev)

    def pol(k_=kk, wre_=wre, wim_=wim, n=1, N_=N, iv_=iv, ifl_=ifl, n_ext_=n_ext, ex_=ex, ev_=ev, ef_=ef, cplx=0, fp_=fp,
            parity=1, flags=0, xo_=xo, ao_=ao):
        return lib.es_slab_polarisation(h, P(k_), P(wre_), P(wim_), n, N_, P(iv_), P(ifl_), n_ext_, P(ex_), P(ev_), P(ef_),
                                        cplx, C.byref(fp_) if fp_ is not None else None, 1.0, 2.0, 0.5, 0.0, parity, flags,
                                        P(xo_), P(ao_))

    null_prof = _lib.SlabFieldProfiles(prof[0].data_ptr(), None, prof[2].data_ptr(), prof[3].data_ptr(), prof[4].data_ptr())
    for bad in (dict(n=-1), dict(N_=2), dict(N_=-1), dict(n_ext_=1), dict(n_ext_=2), dict(n_ext_=-1), dict(cplx=2),
                dict(parity=2), dict(parity=-1), dict(flags=2), dict(k_=None), dict(wre_=None), dict(iv_=None),
                dict(ifl_=None), dict(ex_=None), dict(ev_=None), dict(ef_=None), dict(fp_=None), dict(fp_=null_prof),
                dict(xo_=None), dict(ao_=None)):
        assert pol(**bad) == 1, bad
    assert b"invalid argument" in lib.es_last_error(h)
    # empty calls succeed and write nothing
    for empty in (dict(n_x_=0), dict(n_z_=0), dict(n_t_=0), dict(n_t_=0, t_=None, out_=None), dict(n_x_=0, x_=None)):
        assert syn(**empty) == 0, empty
    assert pol(n=0) == 0 and pol(n=0, k_=None, wre_=None, iv_=None, ifl_=None, xo_=None, ao_=None) == 0
    es_ctx.synchronize()
    assert bool((out == -5.0).all()) and bool((xo == -77.0).all()) and bool((ao == -77.0).all())
    # the same arguments, unchanged, are valid calls; NULL w_im is a real mode; n_ext = 0 needs no exterior arrays
    assert syn() == 0 and pol() == 0 and pol(wim_=None) == 0
    es_ctx.synchronize()
    assert bool((out != -5.0).all()) and bool((xo != -77.0).all()) and bool((ao != -77.0).all())
    assert pol(n_ext_=0, ex_=None, ev_=None, ef_=None) == 0 and syn(xt=xtab[n_ext:n_ext + N].contiguous(), n_ext_=0) == 0
    es_ctx.synchronize()
