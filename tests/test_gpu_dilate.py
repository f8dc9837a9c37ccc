"""The dilation along u on the GPU (K16): rslf_volume_dilate_u against tests/dilate_ref.py bit for bit, pad included;
undilate_u; Depth1DComputer_pile and Depth2DComputer with u_dilation against the oracle on the dilated field and against the
same computer built on the pre-dilated volume; the point of the feature on the device; u_dilation = 1 changes nothing; the
error paths, after which the context still computes."""
import ctypes as C

import numpy as np
import pytest

import dilate_ref as dr

pytestmark = pytest.mark.gpu
F = np.float32


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


def _source(V, S, U, Cc, negative=False, seed=0):
    """Plateaus and noise in [0, 1] (or [-0.5, 1]): the sums of the cubic and Lanczos kinds leave the range next to a step."""
    rng = np.random.default_rng(1000 + 7 * U + Cc + seed)
    lo = -0.5 if negative else 0.0
    x = rng.uniform(lo, 1.0, (V, S, U, Cc)).astype(F)
    steps = rng.uniform(size=(V, S, (U + 4) // 5, Cc))
    plate = np.repeat(np.where(steps < 0.4, lo, 1.0), 5, axis=2)[:, :, :U].astype(F)
    keep = np.repeat(steps < 0.8, 5, axis=2)[:, :, :U]
    x = np.where(keep, plate, x).astype(F)
    x.reshape(-1)[0], x.reshape(-1)[-1] = lo, 1.0
    return x


SHAPES = [(3, 4, 1, 1, 2), (3, 4, 2, 3, 4), (2, 3, 33, 1, 2), (2, 3, 22, 1, 3), (2, 3, 64, 3, 2), (2, 2, 700, 1, 4), (2, 2, 700, 3, 3),
          (2, 2, 130, 1, 8)]


@pytest.mark.parametrize("kind", dr.KINDS, ids=[dr.NAMES[k] for k in dr.KINDS])
@pytest.mark.parametrize("V,S,U,Cc,f", SHAPES, ids=["V%dS%dU%dC%df%d" % s for s in SHAPES])
def test_k16_equals_the_yardstick_bit_for_bit(rs, V, S, U, Cc, f, kind):
    """The whole slab, pad included.  (2,3,33,1,2): U' = 65, the pitch grows to 128; (2,3,22,1,3): U' = 64, the pitch must be
    128; the 700-column shapes take several tiles per row.  The U = 130 volume has negative values."""
    x = _source(V, S, U, Cc, negative=(U == 130))
    src = rs.Volume.from_dense(x, 1.0)
    sd = src.describe()
    assert sd.min_value == x.min() and sd.max_value == x.max()
    dil = src.dilated_u(f, kind)
    got, d = _slab(dil)
    want = dr.slab(x, f, kind)
    Ud = dr.dilated_width(U, f)
    assert (d.V, d.S, d.U, d.C, d.pitch) == (V, S, Ud, Cc, dr.pitch(Ud)) and (dil.V, dil.S, dil.U, dil.C) == (V, S, Ud, Cc)
    assert got.shape == want.shape
    assert not got[:, :, Ud:].any(), "the pad is not zero"
    bad = np.flatnonzero(_bits(got).reshape(-1) != _bits(want).reshape(-1))
    assert bad.size == 0, (bad.size, np.unravel_index(bad[0], want.shape), got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])
    assert d.min_value == sd.min_value and d.max_value == sd.max_value
    assert got[:, :, :Ud].min() == sd.min_value and got[:, :, :Ud].max() == sd.max_value
    assert dil.u_dilation == f and dil.u_source is src and dil.scale_used == src.scale_used
    # f = 1: the source's slab
    one, d1 = _slab(src.dilated_u(1, kind))
    assert d1.pitch == sd.pitch and np.array_equal(_bits(one), _bits(_slab(src)[0]))


@pytest.mark.parametrize("dtype", ["float32", "int32", "uint8"])
def test_undilate_u(rs, dtype):
    import torch
    ctx = rs.default_context(0)
    rng = np.random.default_rng(3)
    for shape, f in (((3, 2, 13), 4), ((5, 1), 8), ((4, 601), 3), ((2, 3, 2, 77), 2), ((7, 9), 1), ((70000, 3), 2)):
        a = rng.integers(0, 250, shape).astype(dtype)
        t = torch.from_numpy(a).cuda()
        out = rs.undilate_u(ctx, t, f)
        assert out.dtype == t.dtype and out.is_contiguous()
        assert np.array_equal(out.cpu().numpy(), a[..., ::f]), (shape, f)
    # a view that is not contiguous
    a = rng.integers(0, 250, (6, 26)).astype(dtype)
    t = torch.from_numpy(a).cuda()[:, :25]
    assert np.array_equal(rs.undilate_u(ctx, t, 3).cpu().numpy(), a[:, :25:3])
    with pytest.raises(ValueError, match="not factor"):
        rs.undilate_u(ctx, torch.zeros((2, 12), device="cuda"), 4)
    with pytest.raises(ValueError, match="uint8, float32 or int32"):
        rs.undilate_u(ctx, torch.zeros((2, 13), device="cuda", dtype=torch.float64), 4)


def _pile_field(Cc):
    from remotesensingproject_amd.synth import make_lightfield
    return make_lightfield(80, 5, 7, Cc, seed=41 + Cc, dmin=-1.0, dmax=1.0, band=2)[0]


@pytest.mark.parametrize("Cc", [1, 3])
def test_the_pile_path_in_the_dilated_frame(rs, oracle_mod, Cc):
    """Depth1DComputer_pile(vol, u_dilation=2) on V=5, S=7, U=80: the oracle on dilate_ref(vol) with slope factor 2, held to
    it as tests/test_gpu_golden.py holds an undilated run; and the same computer built on the pre-dilated volume with slope
    factor 2, bit for bit."""
    from tests.test_gpu_golden import _check_against
    from tests.test_oracle import KEYS
    vol = _pile_field(Cc)
    D = 12
    params = rs.Depth1DParameters()
    comp = rs.Depth1DComputer_pile(vol, -1.0, 1.0, D, epi_scale_factor=1.0, parameters=params, u_dilation=2)
    comp.run()
    got = comp.results()
    assert params.par_slope_factor == 1.0 and comp.m_parameters.par_slope_factor == 2.0       # the caller's object is not modified
    assert comp.m_epis.U == 159 and got["depth"].shape == (5, 159)
    dil = dr.dilate(vol, 2, dr.CUBIC)
    p = oracle_mod.default_params()
    p.slope_factor = 2.0
    ref = oracle_mod.depth1d_pile_run(dil, -1.0, 1.0, D, params=p)
    _check_against(got, {k: getattr(ref, k) for k in KEYS}, "pile u_dilation=2 C=%d" % Cc)
    assert (ref.depth_idx >= 0).sum() > 100
    pre = rs.Depth1DComputer_pile(rs.Volume.from_dense(dil, 1.0), -1.0, 1.0, D, parameters=rs.Depth1DParameters(par_slope_factor=2.0))
    pre.run()
    want = pre.results()
    for k in KEYS:
        assert np.array_equal(_bits(got[k]) if got[k].dtype == F else got[k], _bits(want[k]) if want[k].dtype == F else want[k]), k
    # back on the source grid
    for name, key in (("depth", "depth"), ("valid", "edge_mask"), ("edge_confidence", "edge_confidence"),
                      ("disp_confidence", "disp_confidence"), ("rbar", "rbar"), ("depth_raw", "depth_raw"), ("depth_idx", "depth_idx")):
        u = comp.undilated(name).cpu().numpy()
        assert u.shape[:2] == (5, 80) and u.tobytes() == np.ascontiguousarray(got[key][:, ::2]).tobytes(), name
    with pytest.raises(ValueError, match="no plane 'nothing'"):
        comp.undilated("nothing")
    # the single-EPI class the same way
    one = rs.Depth1DComputer(vol[2, :, :, 0] if Cc == 1 else vol[2], -1.0, 1.0, D, epi_scale_factor=1.0, u_dilation=2)
    one.run()
    o = one.results()
    assert o["depth"].shape == (159,) and np.array_equal(one.undilated("depth").cpu().numpy(), o["depth"][::2])
    assert one.undilated("rbar").shape == (80, Cc)
    q = oracle_mod.default_params()
    q.slope_factor = 2.0
    r1 = oracle_mod.depth1d_pile_run(dr.dilate(vol[2:3], 2, dr.CUBIC), -1.0, 1.0, D, params=q)   # (the range clamp is this EPI's min and max)
    assert np.array_equal(o["depth_idx"], r1.depth_idx[0]) and np.array_equal(_bits(o["score"]), _bits(r1.score[0]))


def _same(a, b, label):
    """Two getters' answers -- NamedTuples of tensors, numbers and Nones -- bit for bit."""
    import torch
    if isinstance(a, tuple):
        assert type(a) is type(b) and len(a) == len(b), label
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%s]" % (label, getattr(a, "_fields", range(len(a)))[k]))
    elif isinstance(a, torch.Tensor):
        x, y = a.cpu().numpy(), b.cpu().numpy()
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), label
    elif isinstance(a, np.ndarray):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), label
    else:
        assert a == b or (a != a and b != b), (label, a, b)


@pytest.mark.parametrize("Cc,S,U,V,D", [(1, 7, 80, 5, 12), (3, 5, 70, 4, 8)])
def test_the_sweep_in_the_dilated_frame(rs, oracle_mod, Cc, S, U, V, D):
    """Depth2DComputer(u_dilation=2) on two of tests/test_gpu_sweep2d.py's struct fields: the oracle's sweep on the dilated
    field with slope factor 2 by that file's _check (every plane bit-exact, C_d within 1e-5); consistency, view prediction
    and novel-view prediction equal those of the computer built from the pre-dilated volume; undilated("depth")."""
    from remotesensingproject_amd.synth import make_lightfield
    from tests.test_gpu_sweep2d import _check
    vol, _ = make_lightfield(U, V, S, Cc, seed=200 + S, dmin=-1.0, dmax=1.0, band=2)
    dil = dr.dilate(vol, 2, dr.CUBIC)
    p = oracle_mod.default_params()
    p.slope_factor = 2.0
    ref = oracle_mod.depth2d_run(dil, -1.0, 1.0, D, params=p)
    comp = rs.Depth2DComputer(vol, -1.0, 1.0, D, epi_scale_factor=1.0, u_dilation=2)
    comp.run()
    got = comp.results()
    Ud = 2 * (U - 1) + 1
    assert got["depth"].shape == (S, V, Ud)
    _check(got, ref, "sweep u_dilation=2 C%d_S%d" % (Cc, S))
    pre = rs.Depth2DComputer(rs.Volume.from_dense(dil, 1.0), -1.0, 1.0, D, parameters=rs.Depth1DParameters(par_slope_factor=2.0))
    pre.run()
    want = pre.results()
    for k in got:
        assert got[k].tobytes() == want[k].tobytes(), k
    _same(comp.get_consistency(), pre.get_consistency(), "get_consistency")
    _same(comp.get_view_prediction(), pre.get_view_prediction(), "get_view_prediction")
    _same(comp.get_novel_view_prediction(), pre.get_novel_view_prediction(), "get_novel_view_prediction")
    assert np.array_equal(comp.undilated("depth").cpu().numpy(), got["depth"][..., ::2])
    assert np.array_equal(comp.undilated("valid").cpu().numpy(), comp.get_valid_depths_mask_s_v_u().cpu().numpy()[..., ::2])
    assert np.array_equal(comp.undilated("rbar").cpu().numpy(), got["rbar"][:, :, ::2])
    assert comp.get_disparity_map().shape == (V, Ud, 3)                    # the renderers answer in the dilated frame


def test_the_point_of_the_feature_on_the_device(rs):
    """tests/test_dilate_cpu.py's field and conditions, seed 1, through Depth1DComputer_pile: MAE of depth_raw relative to
    the plain run <= 0.80 with cubic x2, <= 0.65 with Lanczos-3 x2, within [0.95, 1.05] with linear x2."""
    vol, delta = dr.small_slope_field(1)

    def mae(f, kind):
        comp = rs.Depth1DComputer_pile(vol, dr.FIELD_DMIN, dr.FIELD_DMAX, dr.FIELD_D, epi_scale_factor=1.0, u_dilation=f, dilation_kind=kind)
        comp.run()
        r = comp.results()
        return dr.field_mae(r["depth_raw"], r["edge_mask"], delta, f)

    plain = mae(1, dr.CUBIC)
    ratios = {dr.NAMES[k]: mae(2, k) / plain for k in dr.KINDS}
    print("plain MAE %.5f; ratios %s" % (plain, {k: round(v, 4) for k, v in ratios.items()}))
    assert plain > 0
    assert ratios["cubic"] <= 0.80
    assert ratios["lanczos3"] <= 0.65
    assert 0.95 <= ratios["linear"] <= 1.05


def test_factor_one_changes_nothing(rs):
    """u_dilation = 1 against a computer built without the argument: the same planes bit for bit on a pile case and a sweep
    case, the same Volume object (no launch, no allocation)."""
    vol = _pile_field(1)
    v = rs.Volume.from_dense(vol, 1.0)
    a = rs.Depth1DComputer_pile(v, -1.0, 1.0, 12, u_dilation=1, dilation_kind=rs.DILATE_LANCZOS3)
    b = rs.Depth1DComputer_pile(v, -1.0, 1.0, 12)
    assert a.m_epis is v and b.m_epis is v and a.m_parameters.par_slope_factor == 1.0
    a.run()
    b.run()
    ra, rb = a.results(), b.results()
    for k in ra:
        assert ra[k].tobytes() == rb[k].tobytes(), k
    assert a.undilated("depth") is a.m_best_depth_v_u
    a2 = rs.Depth2DComputer(v, -1.0, 1.0, 12, u_dilation=1)
    b2 = rs.Depth2DComputer(v, -1.0, 1.0, 12)
    assert a2.m_epis is v
    a2.run()
    b2.run()
    ra, rb = a2.results(), b2.results()
    for k in ra:
        assert ra[k].tobytes() == rb[k].tobytes(), k
    assert a2.undilated("depth") is a2.m_best_depth_s_v_u


def test_the_error_paths_leave_the_context_usable(rs):
    """Every RSLF_ERR_INVALID_ARG of the C-ABI's three device entries and the line-confidence refusal; then a small pile step
    on the same context, compared with the one before."""
    import torch
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    ctx = rs.default_context(0)
    vol = _pile_field(1)
    v = rs.Volume.from_dense(vol, 1.0, ctx)
    comp = rs.Depth1DComputer_pile(v, -1.0, 1.0, 12, u_dilation=2)
    comp.run()
    before = comp.results()
    out = C.c_void_p()
    INVALID = -1

    def refused(*args):
        out.value = 5        # a failed call leaves *out NULL
        assert L.rslf_volume_dilate_u(*args, C.byref(out)) == INVALID, args
        assert not out.value and L.rslf_last_error()

    refused(None, v._h, 2, 1)
    refused(ctx._h, None, 2, 1)
    for f in (0, -1, 9):
        refused(ctx._h, v._h, f, 1)
    for kind in (-1, 3):
        refused(ctx._h, v._h, 2, kind)
    empty = rs.Volume(ctx, 2, 3, 10, 1)          # never filled
    refused(ctx._h, empty._h, 2, 1)
    assert L.rslf_volume_dilate_u(ctx._h, v._h, 2, 1, None) == INVALID
    alias = C.c_void_p(v._h.value)               # out holds the source's handle: refused, and the handle stays
    assert L.rslf_volume_dilate_u(ctx._h, v._h, 2, 1, C.byref(alias)) == INVALID and alias.value == v._h.value
    for bad in (0, 9, 2.5):
        with pytest.raises(ValueError, match="u_dilation"):
            v.dilated_u(bad)
    with pytest.raises(ValueError, match="dilation_kind"):
        v.dilated_u(2, 5)
    a = torch.zeros((4, 13), device="cuda")
    b = torch.zeros((4, 4), device="cuda")
    und = L.rslf_planes_undilate_u
    assert und(None, a.data_ptr(), 4, 4, 13, 4, b.data_ptr()) == INVALID
    assert und(ctx._h, None, 4, 4, 13, 4, b.data_ptr()) == INVALID
    assert und(ctx._h, a.data_ptr(), 4, 4, 13, 4, None) == INVALID
    assert und(ctx._h, a.data_ptr(), 4, 4, 13, 4, a.data_ptr()) == INVALID
    for eb in (0, 2, 8):
        assert und(ctx._h, a.data_ptr(), eb, 4, 13, 4, b.data_ptr()) == INVALID
    for f in (0, 9):
        assert und(ctx._h, a.data_ptr(), 4, 4, 13, f, b.data_ptr()) == INVALID
    for Ud in (12, 14, 0, -3):
        assert und(ctx._h, a.data_ptr(), 4, 4, Ud, 4, b.data_ptr()) == INVALID
    assert und(ctx._h, a.data_ptr(), 4, 0, 13, 4, b.data_ptr()) == 0       # no rows: nothing to do
    with pytest.raises(_lib.RslfError) as ei:
        rs.Volume(ctx, 2, 3, 10, 1).dilated_u(2)
    assert ei.value.status == INVALID and "filled" in str(ei.value)
    # the line confidence takes no slope factor: refused by name, in the constructor and when set afterwards
    p = rs.Depth1DParameters(par_line_confidence_mode=rs.LINE_CONF_AS_BUILT)
    with pytest.raises(ValueError, match="par_line_confidence_mode=1 together with u_dilation=2"):
        rs.Depth2DComputer(v, -1.0, 1.0, 12, parameters=p, u_dilation=2)
    late = rs.Depth2DComputer(v, -1.0, 1.0, 12, u_dilation=2)
    late.m_parameters.par_line_confidence_mode = rs.LINE_CONF_GATE
    with pytest.raises(ValueError, match="together with u_dilation=2"):
        late.run()
    # the context still computes
    comp.run()
    after = comp.results()
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
