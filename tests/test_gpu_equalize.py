"""The per-view equalisation on the GPU (K19): the statistics kernel against the numpy integers exactly, the volume and the
dense forms against tests/equalize_ref.py bit for bit, pad and description included; the pyramid with equalize_views = m
against the same pyramid on the numpy-equalised field, plane by plane and byte by byte; off is off; both entries on a
non-default stream; the refusals, after which the context still computes.  Every equality is exact, by the rule."""
import ctypes as C

import numpy as np
import pytest

import equalize_ref as eref

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, UNSUPPORTED = -1, -2
ELEM_ID = {"f32": 0, "u8": 1, "u16": 2}
DTYPES = {"f32": np.float32, "u8": np.uint8, "u16": np.uint16}
# 1023, 1024, 1025: a tile of the kernels is 1024 pixels; 63, 64, 65: the pitch grows at U = 64; 2049: three tiles
WIDTHS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
SHAPES = [(1, 1), (1, 2), (2, 3), (3, 5), (5, 9), (17, 4)]


@pytest.fixture(scope="module")
def rs():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from remotesensingproject_amd import depth
    return depth


def _read_device(ptr, nbytes):
    """Device memory at a raw address -> host bytes, through the HIP runtime the library itself is bound to."""
    import torch
    from remotesensingproject_amd import _lib
    torch.cuda.synchronize()
    L = _lib.lib()
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.hipMemcpy.restype = C.c_int
    out = np.empty(nbytes, np.uint8)
    assert L.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), nbytes, 2) == 0   # hipMemcpyDeviceToHost
    return out


def _slab(vol):
    """The whole slab of a Volume, pad included -> ([V, S, pitch, C], its descriptor)."""
    d = vol.describe()
    assert d.bytes == d.V * d.S * d.C * d.pitch * 4 and d.pitch % 64 == 0 and d.pitch > d.U
    return _read_device(d.d_base, d.bytes).view(F).reshape(d.V, d.S, d.pitch, d.C), d


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(got, want, label):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
    g, w = got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (label, bad.size, bad[0] // got.itemsize, got.reshape(-1)[bad[0] // got.itemsize], want.reshape(-1)[bad[0] // got.itemsize])


def _source(elem, V, S, U, C_, seed=0):
    """A field whose views differ in gain and offset (so no coefficient is trivial), with its maximum below the top of the
    range: float elements in (0, 1], integer elements as integer levels held in float32."""
    rng = np.random.default_rng(1900 + 7 * U + 3 * V + S + 11 * C_ + seed)
    base = rng.uniform(0.1, 0.6, (V, 1, U, C_))
    gain = rng.uniform(0.6, 1.5, (1, S, 1, C_))
    off = rng.uniform(0.0, 0.1, (1, S, 1, C_))
    x = (base * gain + off + rng.uniform(0, 0.03, (V, S, U, C_))).astype(F)
    if elem == "u8":
        x = np.rint(x * 255.0).clip(0, 255).astype(F)
    elif elem == "u16":
        x = np.rint(x * 65535.0).clip(0, 65535).astype(F)
    return x


def _lib_():
    from remotesensingproject_amd import _lib
    return _lib.lib()


def _dense_stats(rs, ctx, t, elem, hi):
    """rslf_view_stats_dense on a CUDA tensor [V, S, U, C] -> uint64 [S, C, 3]."""
    import torch
    from remotesensingproject_amd import _lib
    V, S, U, C_ = t.shape
    d_stats = torch.full((S, C_, 3), -1, dtype=torch.int64, device=t.device)   # (the call zeroes it)
    ctx.use_current_stream()
    rs.check(_lib.lib().rslf_view_stats_dense(ctx._h, t.data_ptr(), ELEM_ID[elem], V, S, U, C_, float(hi), d_stats.data_ptr()),
             "rslf_view_stats_dense")
    return d_stats.cpu().numpy().view(np.uint64)


# ---- the statistics ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("elem", eref.ELEMS)
def test_the_statistics_equal_the_numpy_integers(rs, elem):
    """rslf_view_stats_dense for the three element types, and for float elements rslf_volume_view_stats of the volume made of
    the same array: the integers (n, s1, s2) of tests/equalize_ref.py, exactly, at every width and shape and C in {1, 3};
    once with NaNs among the samples and once from a base that is only 4-byte aligned."""
    import torch
    ctx = rs.default_context(0)
    for U in WIDTHS:
        for V, S in SHAPES:
            for C_ in (1, 3):
                x = _source(elem, V, S, U, C_)
                hi = eref.cap_of(x, elem)
                want = eref.view_stats(x, hi)
                t = torch.from_numpy(x).cuda()
                got = _dense_stats(rs, ctx, t, elem, hi)
                assert np.array_equal(got, want), (elem, V, S, U, C_, got.tolist()[:2], want.tolist()[:2])
                if elem == "f32":   # (a volume holds floats)
                    vs = rs.Volume.from_dense(x, 1.0, ctx).view_stats()
                    assert np.array_equal(vs.raw, want) and vs.hi == hi, (V, S, U, C_)
                    assert np.array_equal(vs.n, want[..., 0]) and vs.mean.shape == (S, C_)
                    m = want[..., 1].astype(np.float64) / want[..., 0] / 65535.0 * float(hi)
                    assert np.array_equal(vs.mean, m) and (vs.std >= 0).all()
    # NaNs are not counted (the dense form; a volume that holds a NaN is refused)
    x = _source(elem, 3, 4, 67, 3, seed=5)
    x[0, 1, 5:9] = np.nan
    x[2, 3] = np.nan
    hi = eref.cap_of(x, elem)
    want = eref.view_stats(x, hi)
    assert want[1, 0, 0] == 3 * 67 - 4 and want[3, 0, 0] == 2 * 67
    assert np.array_equal(_dense_stats(rs, ctx, torch.from_numpy(x).cuda(), elem, hi), want)
    # a level that starts one float after a 16-byte boundary: every row is peeled whole
    for C_ in (1, 3):
        x = _source(elem, 3, 2, 37, C_, seed=6)
        flat = torch.zeros(x.size + 1, dtype=torch.float32, device="cuda")
        flat[1:] = torch.from_numpy(x.reshape(-1)).cuda()
        view = flat[1:].view(*x.shape)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        hi = eref.cap_of(x, elem)
        assert np.array_equal(_dense_stats(rs, ctx, view, elem, hi), eref.view_stats(x, hi)), (elem, C_, "unaligned")
    # more views than the grid's cap of 2048 workgroups: a workgroup does a second view
    x = _source(elem, 2, 2100, 6, 1, seed=7)
    hi = eref.cap_of(x, elem)
    assert np.array_equal(_dense_stats(rs, ctx, torch.from_numpy(x).cuda(), elem, hi), eref.view_stats(x, hi)), (elem, "2100 views")


def test_no_accumulator_is_32_bits_wide(rs):
    """An all-hi field of V = 64, S = 2, U = 1100: s1 = 70400 * 65535 is beyond 32 bits, and two samples' q^2 already
    overflow 32 bits in a lane."""
    import torch
    ctx = rs.default_context(0)
    V, S, U = 64, 2, 1100
    for elem, C_ in (("u16", 1), ("f32", 3), ("u8", 1)):
        hi = {"u16": 65535.0, "f32": 0.75, "u8": 255.0}[elem]
        x = np.full((V, S, U, C_), hi, F)
        got = _dense_stats(rs, ctx, torch.from_numpy(x).cuda(), elem, hi)
        n = V * U
        assert n * 65535 > 2 ** 32 and 2 * 65535 ** 2 > 2 ** 32
        assert got.tolist() == [[[n, n * 65535, n * 65535 ** 2]] * C_] * S, (elem, got.tolist())
        assert np.array_equal(got, eref.view_stats(x, hi))
    vs = rs.Volume.from_dense(np.full((V, S, U), 0.75, F), 1.0, ctx).view_stats()
    assert vs.raw.tolist() == [[[V * U, V * U * 65535, V * U * 65535 ** 2]]] * S


# ---- the volume form ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("U", WIDTHS)
def test_the_volume_form_equals_the_rule(rs, U):
    """Volume.equalized_views, both modes, joint and per channel: the whole slab holds the bytes of Volume.from_dense of the
    numpy rule's array, pad floats included; the description is equal; .view_gains equals the numpy coefficients bit for bit;
    with_view_gains with those coefficients gives the same slab; the source volume is unchanged."""
    ctx = rs.default_context(0)
    for V, S in ((1, 1), (2, 3), (3, 5)) + (((17, 4),) if U in (5, 1025) else ()):
        for C_ in (1, 3):
            x = _source("f32", V, S, U, C_)
            src = rs.Volume.from_dense(x, 1.0, ctx)
            before, sd = _slab(src)
            hi = F(sd.max_value)
            assert hi == x.max()
            for mode in (rs.EQUALIZE_GAIN, rs.EQUALIZE_AFFINE):
                for joint in ((None, False) if C_ == 3 else (None,)):
                    for ref in ((None, "mean") if (V, S) == (3, 5) else (None,)):
                        label = (V, S, U, C_, mode, joint, ref)
                        want_arr, want_ab, _ = eref.equalize(x, mode, -1 if ref == "mean" else None, joint, 4.0, "f32", hi)
                        got_vol = src.equalized_views(mode, ref_view=ref, joint=joint)
                        got, d = _slab(got_vol)
                        want_vol = rs.Volume.from_dense(want_arr, 1.0, ctx)
                        want, wd = _slab(want_vol)
                        _same_bits(got, want, label)
                        _same_bits(want[:, :, :U], want_arr, label)                     # (the yardstick's own upload is the array)
                        assert not got[:, :, U:].any(), label
                        assert (d.V, d.S, d.U, d.C, d.pitch, d.bytes) == (wd.V, wd.S, wd.U, wd.C, wd.pitch, wd.bytes) == (V, S, U, C_, eref.pitch(U), got.nbytes)
                        assert _bits(np.array([d.min_value, d.max_value], F)).tolist() == _bits(np.array([wd.min_value, wd.max_value], F)).tolist(), label
                        _same_bits(got_vol.view_gains, want_ab, label)
                        if S > 1:
                            assert not np.array_equal(want_arr, x), label                # (it did something)
                        again = src.with_view_gains(want_ab)
                        _same_bits(_slab(again)[0], want, (label, "with_view_gains"))
                        _same_bits(again.view_gains, want_ab, label)
                        assert (got_vol.V, got_vol.S, got_vol.U, got_vol.C) == (V, S, U, C_) and got_vol.scale_used == src.scale_used
                        assert got_vol.u_dilation == 1 and got_vol.derivative_weight == 0.0 and src.view_gains is None
            after, sd2 = _slab(src)
            _same_bits(after, before, (V, S, U, C_))
            assert (sd2.min_value, sd2.max_value, sd2.C, sd2.d_base) == (sd.min_value, sd.max_value, C_, sd.d_base)


def test_gains_of_ones_copy_the_volume_and_a_computer_takes_the_result(rs):
    """(1, 0) everywhere copies the slab's bits; caller's gains that saturate clamp at [0, max_value]; the equalised volume
    goes on to dilated_u, with_derivative_channels and a computer like any volume."""
    ctx = rs.default_context(0)
    x = _source("f32", 3, 5, 70, 1)
    src = rs.Volume.from_dense(x, 1.0, ctx)
    ones = np.zeros((5, 1, 2), F)
    ones[..., 0] = 1
    _same_bits(_slab(src.with_view_gains(ones))[0], _slab(src)[0], "ones")
    a_b = ones.copy()
    a_b[1] = [3.0, 0.0]
    a_b[2] = [1.0, -0.6]
    a_b[3] = [0.5, 0.25]
    hi = F(x.max())
    got = _slab(src.with_view_gains(a_b))[0][:, :, :70]
    want = eref.apply(x, a_b, hi)
    _same_bits(got, want, "caller's gains")
    assert (want == hi).sum() > 50 and (want == 0).sum() > 50
    eq = src.equalized_views()
    assert eq.dilated_u(2).U == 139 and eq.with_derivative_channels(1.0).C == 3
    with pytest.raises(ValueError, match="derivative_weight"):
        eq.with_derivative_channels(1.0).equalized_views()
    a = rs.Depth2DComputer(eq, -1.0, 1.0, 8)
    b = rs.Depth2DComputer(rs.Volume.from_dense(eref.equalize(x, eref.AFFINE, hi=hi)[0], 1.0, ctx), -1.0, 1.0, 8)
    a.run()
    b.run()
    _same_bits(a.m_best_depth_s_v_u.cpu().numpy(), b.m_best_depth_s_v_u.cpu().numpy(), "a computer on the equalised volume")


# ---- the dense form ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("elem", eref.ELEMS)
def test_the_dense_form_equals_the_rule_in_place_and_out_of_place(rs, elem):
    """equalize_views on a dense level for the three element types: the numpy rule's array and coefficients bit for bit; in
    place equals out of place; the input of the out-of-place form is unchanged; once from an unaligned base, once over more
    rows than the grid's cap."""
    import torch
    ctx = rs.default_context(0)
    dt = DTYPES[elem]
    moved = 0
    for U in (1, 5, 66, 259, 1030, 2049):
        for V, S in ((1, 2), (3, 5), (4, 4)):
            for C_ in (1, 3):
                x = _source(elem, V, S, U, C_)
                for mode, ref, joint in ((rs.EQUALIZE_AFFINE, None, None), (rs.EQUALIZE_GAIN, "mean", False), (rs.EQUALIZE_AFFINE, 0, False)):
                    label = (elem, V, S, U, C_, mode, ref, joint)
                    want, want_ab, _ = eref.equalize(x, mode, -1 if ref == "mean" else ref, joint, 4.0, elem)
                    t = torch.from_numpy(x).cuda()
                    out, a_b = rs.equalize_views(ctx, t, mode, ref, joint, 4.0, dt)
                    assert out.data_ptr() != t.data_ptr()
                    _same_bits(out.cpu().numpy(), want, label)
                    _same_bits(a_b, want_ab, label)
                    _same_bits(t.cpu().numpy(), x, (label, "the input"))
                    same, a_b2 = rs.equalize_views(ctx, t, mode, ref, joint, 4.0, dt, inplace=True)
                    assert same.data_ptr() == t.data_ptr()
                    _same_bits(t.cpu().numpy(), want, (label, "in place"))
                    _same_bits(a_b2, want_ab, label)
                    moved += int((want != x).sum())
                    if (V, S) == (3, 5):   # the apply pass alone, with those coefficients: out of place, then in place
                        hi = float(eref.cap_of(x, elem))
                        alone = torch.full_like(t, -1.0)
                        t.copy_(torch.from_numpy(x))
                        ctx.use_current_stream()
                        apply_ = _lib_().rslf_apply_view_gains_dense
                        rs.check(apply_(ctx._h, t.data_ptr(), ELEM_ID[elem], V, S, U, C_, hi, want_ab.ctypes.data, alone.data_ptr()), "apply")
                        _same_bits(alone.cpu().numpy(), want, (label, "apply alone"))
                        _same_bits(t.cpu().numpy(), x, (label, "apply alone, the input"))
                        rs.check(apply_(ctx._h, t.data_ptr(), ELEM_ID[elem], V, S, U, C_, hi, want_ab.ctypes.data, t.data_ptr()), "apply")
                        _same_bits(t.cpu().numpy(), want, (label, "apply alone, in place"))
                    if elem != "f32":
                        assert (want == np.rint(want)).all()
    assert moved > 100000
    # [V, S, U] is the one-channel level; an unaligned base; 2100 rows
    x = _source(elem, 3, 2, 37, 1, seed=5)
    want = eref.equalize(x, eref.AFFINE, None, None, 4.0, elem)[0]
    _same_bits(rs.equalize_views(ctx, torch.from_numpy(x[..., 0]).cuda(), dtype=dt)[0].cpu().numpy(), want[..., 0], (elem, "[V,S,U]"))
    for C_ in (1, 3):
        x = _source(elem, 3, 2, 37, C_, seed=6)
        flat = torch.zeros(x.size + 1, dtype=torch.float32, device="cuda")
        flat[1:] = torch.from_numpy(x.reshape(-1)).cuda()
        view = flat[1:].view(*x.shape)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        rs.equalize_views(ctx, view, dtype=dt, inplace=True)
        _same_bits(view.cpu().numpy(), eref.equalize(x, eref.AFFINE, None, None, 4.0, elem)[0], (elem, C_, "unaligned"))
    x = _source(elem, 700, 3, 6, 1, seed=3)
    _same_bits(rs.equalize_views(ctx, torch.from_numpy(x).cuda(), dtype=dt)[0].cpu().numpy(),
               eref.equalize(x, eref.AFFINE, None, None, 4.0, elem)[0], (elem, "2100 rows"))
    # a NaN stays that NaN and is not counted
    x = _source(elem, 3, 4, 67, 1, seed=8)
    x[1, 2, 7] = np.nan
    _same_bits(rs.equalize_views(ctx, torch.from_numpy(x).cuda(), dtype=dt)[0].cpu().numpy(),
               eref.equalize(x, eref.AFFINE, None, None, 4.0, elem)[0], (elem, "NaN"))


# ---- a non-default stream ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def side(rs):
    """tests/stream_harness.py: a non-blocking side stream, a calibrated delay, and a context made under the stream."""
    import torch
    from tests import stream_harness as sh
    h = sh.Harness(0)
    with torch.cuda.stream(h.side):
        ctx = rs.Context(0)
    yield h, ctx
    torch.cuda.synchronize()
    ctx.close()


@pytest.mark.parametrize("kind", ["late_inputs", "busy_default"])
def test_on_a_non_default_stream(rs, side, kind):
    """The volume entry (read back through the slab) and the dense entry on inputs produced late on a non-blocking stream:
    a launch, memset, copy or wait on another stream reads poison or stale intermediates and computes a wrong answer."""
    from tests import stream_harness as sh
    h, ctx = side
    V, S, U = 7, 5, 70
    vol = _source("f32", V, S, U, 3, seed=29)
    raw = _source("u8", V, S, U, 1, seed=30)
    hi = F(vol.max())
    want_vol, want_vol_ab, _ = eref.equalize(vol, eref.AFFINE, None, None, 4.0, "f32", hi)
    want_raw, want_raw_ab, _ = eref.equalize(raw, eref.GAIN, -1, None, 4.0, "u8")
    L_vol, L_raw = sh.Late(vol, sh.POISON_RADIANCE), sh.Late(raw, sh.POISON_LEVEL_U8)
    with h.scenario(kind) as sc:
        v = rs.Volume.from_dense(sc.produce(L_vol), 1.0, ctx)
        h.side.synchronize()
        sc.arm()
        eq = v.equalized_views()
        stats = v.view_stats()
        h.side.synchronize()
        sc.arm()
        out, a_b = rs.equalize_views(ctx, sc.produce(L_raw), rs.EQUALIZE_GAIN, "mean", None, 4.0, np.uint8, inplace=True)
        got_raw = out.cpu().numpy()
        d = eq.describe()
        slab = _read_device(d.d_base, d.bytes).view(F).reshape(d.V, d.S, d.pitch, d.C)[:, :, :d.U]
    sh.assert_same(np.ascontiguousarray(slab), want_vol, "equalized_views in " + kind)
    sh.assert_same(eq.view_gains, want_vol_ab, "view_gains in " + kind)
    assert np.array_equal(stats.raw, eref.view_stats(vol, hi)), kind
    sh.assert_same(got_raw, want_raw, "equalize_views in " + kind)
    sh.assert_same(a_b, want_raw_ab, "dense view_gains in " + kind)
    assert (d.min_value, d.max_value) == (want_vol.min(), want_vol.max())
    out.fill_(0)


# ---- the pyramid -------------------------------------------------------------------------------------------------------

DMIN, DMAX, DIM_D = -1.0, 1.0, 10
_fields = {}


def _field(elem):
    """V = U = 44, S = 5 (three levels: 44, 22, 11), one channel, two views' brightness drifted -> (the V EPIs [S, U], their
    AFFINE-equalised EPIs, the coefficients)."""
    if elem not in _fields:
        from remotesensingproject_amd.synth import make_lightfield
        vol = make_lightfield(44, 44, 5, 1, seed=191, dmin=DMIN, dmax=DMAX, band=4, lo=0.1, hi=0.6)[0][..., 0]
        vol[:, 1] *= F(1.4)
        vol[:, 4] = vol[:, 4] * F(0.7) + F(0.05)
        if elem == "u8":
            vol = np.rint(vol * 255.0).astype(np.uint8)
        elif elem == "u16":
            vol = np.rint(vol * 65535.0).astype(np.uint16)
        epis = [np.ascontiguousarray(vol[v]) for v in range(vol.shape[0])]
        eq, a_b = eref.equalize_epis(epis, eref.AFFINE)
        assert not np.array_equal(np.stack(eq), np.stack(epis)) and abs(a_b[1, 0, 0] - 1 / 1.4) < 0.05
        _fields[elem] = (epis, eq, a_b)
    return _fields[elem]


def _kept_planes(run, names=("depth", "valid", "Ce", "Cd")):
    out = {}
    for l in range(run.n_levels):
        for name in names:
            out[(l, name)] = run.plane(l, name).cpu().numpy()
    out["fused_map"] = run.plane(0, "fused_map").cpu().numpy()
    out["fused_valid"] = run.plane(0, "fused_valid").cpu().numpy()
    return out


def _compare(got: dict, want: dict, label):
    assert got.keys() == want.keys(), label
    for k in want:
        _same_bits(got[k], want[k], (label, k))


@pytest.mark.parametrize("elem", eref.ELEMS)
def test_a_kept_pyramid_equals_the_pyramid_on_the_equalised_field(rs, elem):
    epis, eq, a_b = _field(elem)
    run = rs.fine_to_coarse_run_host(epis, DMIN, DMAX, DIM_D, keep=True, equalize_views=rs.EQUALIZE_AFFINE)
    ref = rs.fine_to_coarse_run_host(eq, DMIN, DMAX, DIM_D, keep=True)
    assert run.n_levels == ref.n_levels == 3 and run.dims == ref.dims == [(44, 44), (22, 22), (11, 11)]
    assert run.C == ref.C == 1 and run.equalize_views == (rs.EQUALIZE_AFFINE, 2) and ref.equalize_views is None and ref.view_gains is None
    got, want = _kept_planes(run), _kept_planes(ref)
    _compare(got, want, elem)
    _same_bits(run.view_gains, a_b, (elem, "view_gains"))
    # the equalisation changed something: the plain pyramid of the drifted field is another run
    plain = _kept_planes(rs.fine_to_coarse_run_host(epis, DMIN, DMAX, DIM_D, keep=True))
    assert any(not np.array_equal(plain[k], got[k]) for k in got), elem
    assert sum(int(want[(l, "valid")].astype(bool).sum()) for l in range(3)) > 500
    # GAIN towards the views' mean, per run
    eq2, a_b2 = eref.equalize_epis(epis, eref.GAIN, -1)
    run2 = rs.fine_to_coarse_run_host(epis, DMIN, DMAX, DIM_D, keep=True, equalize_views=rs.EQUALIZE_GAIN, equalize_ref_view="mean",
                                      equalize_max_gain=2.0)
    _compare(_kept_planes(run2), _kept_planes(rs.fine_to_coarse_run_host(eq2, DMIN, DMAX, DIM_D, keep=True)), (elem, "gain"))
    _same_bits(run2.view_gains, a_b2, (elem, "gain view_gains"))
    assert run2.equalize_views == (rs.EQUALIZE_GAIN, -1)


@pytest.mark.parametrize("elem", eref.ELEMS)
def test_the_host_planes_form_equals_it_too(rs, elem):
    epis, eq, _ = _field(elem)
    got = rs.fine_to_coarse_run_host(epis, DMIN, DMAX, DIM_D, want_levels=True, equalize_views=rs.EQUALIZE_AFFINE)
    want = rs.fine_to_coarse_run_host(eq, DMIN, DMAX, DIM_D, want_levels=True)
    assert got["n_levels"] == want["n_levels"] == 3
    _same_bits(got["out_map"], want["out_map"], elem)
    _same_bits(got["out_valid"], want["out_valid"], elem)
    for l in range(3):
        for k in ("depth", "valid", "edge_confidence"):
            _same_bits(got["levels"][l][k], want["levels"][l][k], (elem, l, k))


def _loop_planes(f2c):
    out = {}
    for l, comp in enumerate(f2c.m_computers):
        out[(l, "depth")] = comp.m_best_depth_s_v_u.cpu().numpy()
        out[(l, "valid")] = comp.get_valid_depths_mask_s_v_u().cpu().numpy()
        out[(l, "Ce")] = comp.m_edge_confidence_s_v_u.cpu().numpy()
        out[(l, "Cd")] = comp.m_disp_confidence_s_v_u.cpu().numpy()
    m, v = f2c.get_results()
    out["fused_map"], out["fused_valid"] = m.cpu().numpy(), v.cpu().numpy()
    return out


@pytest.mark.parametrize("elem", eref.ELEMS)
def test_the_python_level_loop_equals_it_too(rs, elem):
    """FineToCoarse(..., equalize_views=m).run(): the dense form once, in place, on f2c_input's output, then today's loop;
    equal to the loop on the equalised field and to the library's kept run."""
    epis, eq, a_b = _field(elem)
    a = rs.FineToCoarse(epis, DMIN, DMAX, DIM_D, equalize_views=rs.EQUALIZE_AFFINE)
    b = rs.FineToCoarse(eq, DMIN, DMAX, DIM_D)
    assert a.m_equalize_views == rs.EQUALIZE_AFFINE and b.m_equalize_views == 0 and b.m_view_gains is None
    _same_bits(a.m_view_gains, a_b, elem)
    a.run()
    b.run()
    got = _loop_planes(a)
    _compare(got, _loop_planes(b), elem)
    kept = _kept_planes(rs.fine_to_coarse_run_host(epis, DMIN, DMAX, DIM_D, keep=True, equalize_views=rs.EQUALIZE_AFFINE))
    _compare(got, kept, (elem, "kept"))


def test_with_derivative_channels_and_the_level_dilation(rs):
    """equalize_views with derivative_channels = 1 and level_dilation = 2: the features are derivatives of the equalised
    intensity, and the rest goes on unchanged."""
    for elem in ("f32", "u8"):
        epis, eq, a_b = _field(elem)
        more = dict(derivative_channels=1.0, level_dilation=2)
        run = rs.fine_to_coarse_run_host(epis, DMIN, DMAX, DIM_D, keep=True, equalize_views=rs.EQUALIZE_AFFINE, **more)
        ref = rs.fine_to_coarse_run_host(eq, DMIN, DMAX, DIM_D, keep=True, **more)
        assert run.C == ref.C == 3 and run.level_dilation[0] == 2 and run.view_gains.shape == (5, 1, 2)
        _compare(_kept_planes(run), _kept_planes(ref), (elem, "dv + dl"))
        _same_bits(run.view_gains, a_b, elem)
    epis, eq, _ = _field("u16")
    a = rs.FineToCoarse(epis, DMIN, DMAX, DIM_D, equalize_views=rs.EQUALIZE_AFFINE, derivative_channels=1.0, level_dilation=2)
    b = rs.FineToCoarse(eq, DMIN, DMAX, DIM_D, derivative_channels=1.0, level_dilation=2)
    a.run()
    b.run()
    _compare(_loop_planes(a), _loop_planes(b), "loop dv + dl")


def test_an_rgb_pyramid_joint_and_per_channel(rs):
    from remotesensingproject_amd.synth import make_lightfield
    vol = make_lightfield(44, 44, 5, 3, seed=192, dmin=DMIN, dmax=DMAX, band=4, lo=0.1, hi=0.6)[0]
    vol[:, 0] *= np.array([1.3, 1.2, 1.1], F)
    vol[:, 3] *= F(0.75)
    epis = [np.ascontiguousarray(np.rint(vol[v] * 255.0).astype(np.uint8)) for v in range(44)]
    for joint in (None, False):
        eq, a_b = eref.equalize_epis(epis, eref.AFFINE, None, joint)
        run = rs.fine_to_coarse_run_host(epis, DMIN, DMAX, DIM_D, keep=True, equalize_views=rs.EQUALIZE_AFFINE, equalize_joint=joint)
        _compare(_kept_planes(run), _kept_planes(rs.fine_to_coarse_run_host(eq, DMIN, DMAX, DIM_D, keep=True)), ("rgb", joint))
        _same_bits(run.view_gains, a_b, ("rgb", joint))
        assert (a_b[:, 0] == a_b[:, 1]).all() == (joint is None) and run.view_gains.shape == (5, 3, 2)
        # a KeptFineToCoarse made around the handle itself sizes its coefficients from the run
        bare = rs.KeptFineToCoarse(run._h, run.ctx, run.stats)
        _same_bits(bare.view_gains, a_b, ("rgb", joint, "bare"))
        bare._h = None   # (the handle is `run`'s)


@pytest.mark.parametrize("off", [0, None, False])
def test_off_is_off(rs, off):
    """equalize_views off gives the bytes of the call without the argument, in the three forms, and allocates nothing."""
    epis, _, _ = _field("f32")
    a = rs.fine_to_coarse_run_host(epis, DMIN, DMAX, DIM_D, keep=True, equalize_views=off, equalize_ref_view=99, equalize_max_gain=0.0)
    b = rs.fine_to_coarse_run_host(epis, DMIN, DMAX, DIM_D, keep=True)
    assert a.equalize_views is None and a.view_gains is None
    _compare(_kept_planes(a), _kept_planes(b), "kept")
    a = rs.fine_to_coarse_run_host(epis, DMIN, DMAX, DIM_D, equalize_views=off)
    b = rs.fine_to_coarse_run_host(epis, DMIN, DMAX, DIM_D)
    _same_bits(a["out_map"], b["out_map"], "host")
    _same_bits(a["out_valid"], b["out_valid"], "host")
    x = rs.FineToCoarse(epis, DMIN, DMAX, DIM_D, equalize_views=off)
    y = rs.FineToCoarse(epis, DMIN, DMAX, DIM_D)
    x.run()
    y.run()
    _compare(_loop_planes(x), _loop_planes(y), "loop")
    # the C entries: the _eq entry with mode 0 is the _dl entry, whatever the other three arguments hold
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    ctx = rs.default_context(0)
    keep_alive, ptrs, dt, V, S, U, C_, stride = rs.host_epis(epis, stride=True)
    p = rs.Depth1DParameters().to_c()
    planes = []
    for name, tail in (("rslf_fine_to_coarse_run_host_dl", ()), ("rslf_fine_to_coarse_run_host_eq", (0, 77, 1, -3.0))):
        om, ov, nl, st = np.empty((S, V, U), F), np.empty((S, V, U), np.uint8), C.c_int(), _lib.RslfStats()
        rs.check(getattr(L, name)(ctx._h, ptrs, 0, V, S, U, C_, stride, DMIN, DMAX, DIM_D, -1.0, C.byref(p), -1, 1, om.ctypes.data, ov.ctypes.data,
                                  C.byref(nl), C.byref(st), 0, None, 0, 0.0, 1, 1, *tail), name)
        planes.append((om, ov))
    _same_bits(planes[1][0], planes[0][0], "C entry, map")
    _same_bits(planes[1][1], planes[0][1], "C entry, valid")


# ---- the refusals ------------------------------------------------------------------------------------------------------

def test_the_refusals_leave_the_context_usable(rs):
    """Each refusal of include/rslf_hip.h, by its status and its words; the pyramid's before any device work; then a small
    pile step on the same context, compared with the one before."""
    import torch
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd.synth import make_lightfield
    L = _lib.lib()
    ctx = rs.default_context(0)
    vol = make_lightfield(80, 5, 7, 1, seed=42, dmin=-1.0, dmax=1.0, band=2)[0]
    v = rs.Volume.from_dense(vol, 1.0, ctx)
    comp = rs.Depth1DComputer_pile(v, -1.0, 1.0, 12)
    comp.run()
    before = comp.results()
    out = C.c_void_p()
    fn = L.rslf_volume_equalize_views
    ok = dict(ctx=ctx._h, src=v._h, mode=eref.AFFINE, ref=3, joint=0, gain=4.0)

    def refused(status, word=None, **kw):
        a = dict(ok, **kw)
        out.value = 5        # a failed call leaves *out NULL
        assert fn(a["ctx"], a["src"], a["mode"], a["ref"], a["joint"], a["gain"], C.byref(out), None) == status, kw
        assert not out.value and L.rslf_last_error()
        assert word is None or word in L.rslf_last_error(), (kw, L.rslf_last_error())

    refused(INVALID, b"NULL", ctx=None)
    refused(INVALID, b"NULL", src=None)
    for mode in (0, 3, -1):
        refused(INVALID, b"mode", mode=mode)
    for ref in (-2, 7, 1000):
        refused(INVALID, b"ref_view", ref=ref)
    for g in (0.99, 0.0, -4.0, float("nan"), float("inf")):
        refused(INVALID, b"max_gain", gain=g)
    refused(INVALID, b"joint", joint=1)                       # C == 1
    empty = rs.Volume(ctx, 2, 3, 10, 1)                       # never filled
    refused(INVALID, b"not been filled", src=empty._h, ref=1)
    assert fn(ctx._h, v._h, eref.AFFINE, 3, 0, 4.0, None, None) == INVALID
    alias = C.c_void_p(v._h.value)                            # out holds the source's handle: refused, and the handle stays
    assert fn(ctx._h, v._h, eref.AFFINE, 3, 0, 4.0, C.byref(alias), None) == INVALID and alias.value == v._h.value
    negative = rs.Volume.from_dense(vol - F(0.5), 1.0, ctx)   # min_value < 0
    refused(UNSUPPORTED, b"non-negative", src=negative._h)
    infinite = vol.copy()
    infinite[0, 0, 0, 0] = np.inf
    unbounded = rs.Volume.from_dense(infinite, 1.0, ctx)      # (held: the handle lives as long as the object)
    refused(UNSUPPORTED, b"finite", src=unbounded._h)
    # the statistics and the apply entries
    st = np.zeros((7, 1, 3), np.uint64)
    assert L.rslf_volume_view_stats(None, v._h, st.ctypes.data, None) == INVALID
    assert L.rslf_volume_view_stats(ctx._h, None, st.ctypes.data, None) == INVALID
    assert L.rslf_volume_view_stats(ctx._h, v._h, None, None) == INVALID
    assert L.rslf_volume_view_stats(ctx._h, empty._h, st.ctypes.data, None) == INVALID
    assert L.rslf_volume_view_stats(ctx._h, negative._h, st.ctypes.data, None) == UNSUPPORTED
    a_b = np.ones((7, 1, 2), F)
    apply_ = L.rslf_volume_apply_view_gains
    for args in ((None, v._h, a_b.ctypes.data), (ctx._h, None, a_b.ctypes.data), (ctx._h, v._h, None), (ctx._h, empty._h, a_b.ctypes.data)):
        out.value = 5
        assert apply_(*args, C.byref(out)) == INVALID and not out.value, args
    assert apply_(ctx._h, v._h, a_b.ctypes.data, None) == INVALID
    assert apply_(ctx._h, v._h, a_b.ctypes.data, C.byref(alias)) == INVALID and alias.value == v._h.value
    a_b[2, 0, 1] = np.nan
    assert apply_(ctx._h, v._h, a_b.ctypes.data, C.byref(out)) == INVALID and b"finite" in L.rslf_last_error()
    with pytest.raises(ValueError, match="finite"):
        v.with_view_gains(a_b)
    with pytest.raises(ValueError, match=r"\[S, C, 2\]"):
        v.with_view_gains(np.ones((6, 1, 2), F))
    for kw, word in ((dict(mode=0), "equalize_views"), (dict(ref_view=7), "ref_view"), (dict(joint=True), "joint"), (dict(max_gain=0.5), "max_gain")):
        with pytest.raises(ValueError, match=word):
            v.equalized_views(**kw)
    # the dense entries
    a = torch.ones((2, 3, 5), device="cuda")
    s = torch.zeros((3, 1, 3), dtype=torch.int64, device="cuda")
    dense, stats = L.rslf_equalize_views_dense, L.rslf_view_stats_dense
    good = (ctx._h, a.data_ptr(), 0, 2, 3, 5, 1, 1.0, eref.AFFINE, 1, 0, 4.0, None)

    def dense_refused(status, **kw):
        names = ("ctx", "d", "elem", "V", "S", "U", "C", "hi", "mode", "ref", "joint", "gain", "out")
        assert dense(*[kw.get(n, x) for n, x in zip(names, good)]) == status, kw

    assert dense(*good) == 0
    dense_refused(INVALID, ctx=None)
    dense_refused(INVALID, d=None)
    for elem in (-1, 3):
        dense_refused(INVALID, elem=elem)
    for hi in (0.0, -1.0, float("nan"), float("inf")):
        dense_refused(INVALID, hi=hi)
    assert dense(ctx._h, a.data_ptr(), 1, 2, 3, 5, 1, float("nan"), eref.AFFINE, 1, 0, 4.0, None) == 0     # integer elements: hi is the type's
    for kw in (dict(V=0), dict(S=0), dict(U=0), dict(C=2), dict(C=0), dict(mode=0), dict(mode=3), dict(ref=3), dict(ref=-2), dict(joint=1),
               dict(gain=0.5), dict(gain=float("nan"))):
        dense_refused(INVALID, **kw)
    dense_refused(UNSUPPORTED, V=65536, U=32768)          # V * U = 2^31: refused before the device is touched
    dense_refused(UNSUPPORTED, V=46341, U=30895, C=3, joint=1)   # beyond the joint cap
    alone = L.rslf_apply_view_gains_dense
    tab = np.ones((3, 1, 2), F)
    assert alone(ctx._h, a.data_ptr(), 0, 2, 3, 5, 1, 1.0, tab.ctypes.data, a.data_ptr()) == 0
    for bad in ((None, a.data_ptr(), 0, 2, 3, 5, 1, 1.0, tab.ctypes.data, a.data_ptr()), (ctx._h, None, 0, 2, 3, 5, 1, 1.0, tab.ctypes.data, a.data_ptr()),
                (ctx._h, a.data_ptr(), 0, 2, 3, 5, 1, 1.0, None, a.data_ptr()), (ctx._h, a.data_ptr(), 0, 2, 3, 5, 1, 1.0, tab.ctypes.data, None),
                (ctx._h, a.data_ptr(), 4, 2, 3, 5, 1, 1.0, tab.ctypes.data, a.data_ptr()), (ctx._h, a.data_ptr(), 0, 2, 3, 5, 1, 0.0, tab.ctypes.data, a.data_ptr()),
                (ctx._h, a.data_ptr(), 0, 2, 3, 0, 1, 1.0, tab.ctypes.data, a.data_ptr()), (ctx._h, a.data_ptr(), 0, 2, 3, 5, 2, 1.0, tab.ctypes.data, a.data_ptr())):
        assert alone(*bad) == INVALID, bad
    tab[1, 0, 0] = np.inf
    assert alone(ctx._h, a.data_ptr(), 0, 2, 3, 5, 1, 1.0, tab.ctypes.data, a.data_ptr()) == INVALID and b"finite" in L.rslf_last_error()
    assert alone(ctx._h, a.data_ptr(), 0, 65536, 3, 32768, 1, 1.0, tab.ctypes.data, a.data_ptr()) == UNSUPPORTED
    assert stats(ctx._h, a.data_ptr(), 0, 2, 3, 5, 1, 1.0, s.data_ptr()) == 0
    for args in ((None, a.data_ptr(), 0, 2, 3, 5, 1, 1.0, s.data_ptr()), (ctx._h, None, 0, 2, 3, 5, 1, 1.0, s.data_ptr()),
                 (ctx._h, a.data_ptr(), 0, 2, 3, 5, 1, 1.0, None), (ctx._h, a.data_ptr(), 5, 2, 3, 5, 1, 1.0, s.data_ptr()),
                 (ctx._h, a.data_ptr(), 0, 2, 3, 5, 1, 0.0, s.data_ptr()), (ctx._h, a.data_ptr(), 0, 2, 0, 5, 1, 1.0, s.data_ptr()),
                 (ctx._h, a.data_ptr(), 0, 2, 3, 5, 2, 1.0, s.data_ptr())):
        assert stats(*args) == INVALID, args
    assert stats(ctx._h, a.data_ptr(), 0, 65536, 3, 32768, 1, 1.0, s.data_ptr()) == UNSUPPORTED
    torch.cuda.synchronize()
    # the pyramid: refused before any device work, by the argument's name
    epis, _, _ = _field("f32")
    keep_alive, ptrs, dt, V, S, U, C_, stride = rs.host_epis(epis, stride=True)
    p, st_, h = rs.Depth1DParameters().to_c(), _lib.RslfStats(), C.c_void_p()
    args = (ctx._h, ptrs, 0, V, S, U, C_, stride, DMIN, DMAX, DIM_D, -1.0, C.byref(p), -1, 1, 0, 0, 0, C.byref(h), C.byref(st_), 0, 0, 0.0, 0.0,
            0.0, 0, 0, 0.0, 1, 1)
    om, ov, nl = np.empty((S, V, U), F), np.empty((S, V, U), np.uint8), C.c_int()
    hargs = (ctx._h, ptrs, 0, V, S, U, C_, stride, DMIN, DMAX, DIM_D, -1.0, C.byref(p), -1, 1, om.ctypes.data, ov.ctypes.data, C.byref(nl),
             C.byref(st_), 0, None, 0, 0.0, 1, 1)
    free0 = torch.cuda.mem_get_info()[0]
    for eq, word in (((3, 0, 0, 4.0), b"mode"), ((-1, 0, 0, 4.0), b"mode"), ((eref.GAIN, 5, 0, 4.0), b"ref_view"),
                     ((eref.GAIN, -2, 0, 4.0), b"ref_view"), ((eref.AFFINE, 0, 0, 0.5), b"max_gain"),
                     ((eref.AFFINE, 0, 0, float("nan")), b"max_gain"), ((eref.AFFINE, 0, 0, float("inf")), b"max_gain"),
                     ((eref.AFFINE, 0, 1, 4.0), b"joint")):
        assert L.rslf_f2c_run_host_eq(*args, *eq) == INVALID and word in L.rslf_last_error() and not h.value, eq
        assert L.rslf_fine_to_coarse_run_host_eq(*hargs, *eq) == INVALID and word in L.rslf_last_error(), eq
    # a field whose views the statistic cannot count exactly: V * U = 2^31 (the pointers are never read); with joint, the
    # tighter cap of three channels' sums in one uint64
    big = (ctx._h, ptrs, 0, 65536, S, 32768, 1, 0) + args[8:]
    assert L.rslf_f2c_run_host_eq(*big, eref.AFFINE, 0, 0, 4.0) == UNSUPPORTED and b"2^31" in L.rslf_last_error() and not h.value
    hbig = (ctx._h, ptrs, 0, 65536, S, 32768, 1, 0) + hargs[8:]
    assert L.rslf_fine_to_coarse_run_host_eq(*hbig, eref.AFFINE, 0, 0, 4.0) == UNSUPPORTED and b"2^31" in L.rslf_last_error()
    jbig = (ctx._h, ptrs, 0, 46341, S, 30895, 3, 0) + args[8:]          # 1431705195 samples: below 2^31, beyond the joint cap
    assert L.rslf_f2c_run_host_eq(*jbig, eref.AFFINE, 0, 1, 4.0) == UNSUPPORTED and b"joint" in L.rslf_last_error() and not h.value
    assert torch.cuda.mem_get_info()[0] == free0          # nothing was allocated
    md = object.__new__(rs.MultiDevice)
    with pytest.raises(ValueError, match="equalize_views=2 is not built here"):
        md.fine_to_coarse(epis, DMIN, DMAX, DIM_D, equalize_views=rs.EQUALIZE_AFFINE)
    # the context still computes what it computed
    again = rs.Depth1DComputer_pile(v, -1.0, 1.0, 12)
    again.run()
    after = again.results()
    for k in before:
        _same_bits(after[k], before[k], k)
