"""The novel view on the device (rslf_novel_view, k15_novel_view) against tests/novel_view_ref.py, the numpy yardstick written
from the rule: every plane, every pixel, bit for bit; row_err, whose order of summation the rule leaves open, at 1e-9 relative.
tests/test_novel_view_cpu.py shows, on the yardstick alone, that the hole fields make the fill and the blend decide: none of
these tests passes on an idle fill stage."""
import ctypes as C

import numpy as np
import pytest

import consistency_ref as cr
import novel_view_ref as nr
import view_warp_ref as wr

pytestmark = pytest.mark.gpu
F = np.float32
CAP = 8192   # plan::kWarpMaxU
FIELDS = [("planted",) + sh[:3] for sh in cr.SHAPES if sh[0] >= 5] + [("hole", 9, 2, 160), ("hole", 5, 1, 300), ("hole", 5, 11, 41)]
IDS = ["%s_S%d_V%d_U%d" % f for f in FIELDS]


def groups(S):
    """The issue's five targets, by the radius they are asked with -> [(radius, targets, exclude)]."""
    c = S // 2
    return [(0, (float(c), -3.0), (c, -1)), (1, (0.0, c + 0.5), (0, -1)), (4, (S + 1.5,), (-1,))]


@pytest.fixture(scope="module")
def rs():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from remotesensingproject_amd import depth
    return depth


def _host(out):
    return {k: t.cpu().numpy() for k, t in zip(nr.NAMES, out) if t is not None}


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()   # (a copy: the shared fields are read-only)


def _shape_of(k, T, V, U, Cn):
    return (T, V) if k.startswith("row_") else (T, V, U, Cn) if k == "colour" else (T, V, U)


def run_entry(rs, depth, valid, slope, targets, exclude=None, radius=0, nearer=1, max_gap=0, sources=4, tol=np.inf, want=nr.PLANES,
              host=False, volume=None, params=True):
    """rslf_novel_view (or its host form) with exactly the planes of `want`; every plane starts from a sentinel, and the ones not
    asked for are handed over as NULL -> (status, dict of the planes asked for)."""
    import torch
    from remotesensingproject_amd import _lib
    L, ctx = _lib.lib(), rs.default_context(0)
    S, V, U = depth.shape
    T = len(targets)
    depth, valid = np.ascontiguousarray(depth, F), None if valid is None else np.ascontiguousarray(valid, np.uint8)
    outs = {k: np.full(_shape_of(k, T, V, U, volume.C if volume is not None else 1), 77, nr.DTYPES[k]) for k in want}
    if host:
        keep = dict(outs)
        ptr = lambda a: None if a is None else a.ctypes.data
        entry, d_in, v_in = L.rslf_novel_view_host, depth, valid
    else:
        keep = {k: _dev(a) for k, a in outs.items()}
        ptr = lambda t: None if t is None else t.data_ptr()
        entry, d_in, v_in = L.rslf_novel_view, _dev(depth), _dev(valid)
    c_out = _lib.RslfNovelViewOut(*(ptr(keep.get(k)) for k in nr.NAMES))
    c_par = _lib.RslfNovelViewParams(int(radius), int(nearer), int(max_gap), int(sources), float(tol))
    c_t = (C.c_float * T)(*[float(t) for t in targets])
    c_ex = None if exclude is None else (C.c_int * T)(*[int(e) for e in exclude])
    ctx.use_current_stream()
    rc = entry(ctx._h, ptr(d_in), ptr(v_in), S, V, U, float(slope), volume._h if volume is not None else None, c_t, c_ex, T,
               C.byref(c_par) if params else None, C.byref(c_out))
    torch.cuda.synchronize()
    return rc, {k: (a if host else a.cpu().numpy()) for k, a in keep.items()}


def both_forms(rs, depth, valid, slope, targets, exclude, want, label, volume=None, **kw):
    """The device form through novel_view and the host form through the C-ABI, against `want`."""
    err = "err" in want
    got = rs.novel_view(rs.default_context(0), _dev(depth), _dev(valid), volume, slope, targets, exclude, err=err, rows=True, **kw)
    nr.assert_equal(_host(got), want, "novel_view " + label)
    rc, got = run_entry(rs, depth, valid, slope, targets, exclude, want=tuple(k for k in nr.NAMES if k in want), host=True, volume=volume, **kw)
    assert rc == 0
    nr.assert_equal(got, want, "host form " + label)


# ---- 1: the fields -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", FIELDS, ids=IDS)
def test_fields(rs, field):
    """The planted fields (nearly every column hit: stage C), the hole fields (fill and blend; V = 11: more than one XCD round
    with surplus blocks), each with the five targets: the centre view leave-one-out, view 0 leave-one-out within a radius, two
    positions outside the view range and one between two views."""
    kind, S, V, U = field
    depth, valid = nr.field(*field)
    for radius, targets, exclude in groups(S):
        for kw in (dict(max_gap=3, sources=4, tol=0.1), dict(max_gap=0, sources=1, tol=np.inf)):
            want = nr.field_novel(kind, S, V, U, targets, exclude, radius, **kw)
            both_forms(rs, depth, valid, 1.0, targets, exclude, want, "%s radius %d %s" % (field, radius, kw), radius=radius, **kw)


@pytest.mark.parametrize("max_gap", [0, 3])
@pytest.mark.parametrize("sources", [1, 4])
@pytest.mark.parametrize("tol", [0.1, np.inf])
def test_parameter_grid(rs, max_gap, sources, tol):
    S, V, U = 9, 2, 160
    depth, valid = nr.field("hole", S, V, U)
    for radius, targets, exclude in groups(S):
        want = nr.field_novel("hole", S, V, U, targets, exclude, radius, max_gap=max_gap, sources=sources, tol=tol)
        got = rs.novel_view(rs.default_context(0), _dev(depth), _dev(valid), None, 1.0, targets, exclude, radius, 1, max_gap, sources, tol, rows=True)
        nr.assert_equal(_host(got), want, "radius %d" % radius)


@pytest.mark.parametrize("nearer,slope,masked", [(-1, 1.0, True), (1, -0.5, True), (1, 1.0, False), (-1, -0.5, False)])
def test_depth_order_slope_and_no_validity_plane(rs, nearer, slope, masked):
    S, V, U = 9, 2, 160
    depth, valid = nr.field("hole", S, V, U)
    for radius, targets, exclude in groups(S):
        want = nr.field_novel("hole", S, V, U, targets, exclude, radius, nearer=nearer, max_gap=3, slope=slope, masked=masked)
        both_forms(rs, depth, valid if masked else None, slope, targets, exclude, want, "nearer %d slope %g masked %s radius %d" % (
            nearer, slope, masked, radius), radius=radius, nearer=nearer, max_gap=3, tol=0.1)


def test_many_targets(rs):
    """More targets than one launch carries (T = 300)."""
    S, V, U = 17, 2, 37
    depth, valid = nr.field("planted", S, V, U)
    targets = tuple(-2.0 + k * 0.07 for k in range(300))
    exclude = tuple(k % (S + 1) - 1 for k in range(300))
    want = nr.field_novel("planted", S, V, U, targets, exclude, 3, max_gap=2)
    both_forms(rs, depth, valid, 1.0, targets, exclude, want, "T = 300", radius=3, max_gap=2, tol=0.1)


# ---- 2: shapes, values, volumes -------------------------------------------------------------------------------------------------

def _volume(rs, V, S, U, channels, dtype, seed=0):
    """A volume of random radiances -> (Volume, what its slab holds [V, S, U, C] f32)."""
    rng = np.random.RandomState(60 + seed + channels)
    ctx = rs.default_context(0)
    if dtype == np.uint8:
        raw = rng.randint(0, 256, (V, S, U, channels)).astype(np.uint8)
        vol = rs.Volume.from_epis(list(raw[..., 0] if channels == 1 else raw), ctx=ctx)
        slab = _slab(vol.describe())
        assert np.array_equal(slab, wr.normalised(raw))
        return vol, slab
    vol = rs.Volume.from_dense(rng.uniform(0.0, 1.0, (V, S, U, channels)).astype(F), 1.0, ctx)
    return vol, _slab(vol.describe())


@pytest.mark.parametrize("U", [1, 37, 513])
def test_widths(rs, U):
    """One column; below one stride and no multiple of four; across strides and chunks of three columns."""
    S, V = 5, 2
    depth, valid = nr.hole_field(S, V, U)
    vol, slab = _volume(rs, V, S, U, 1, F)
    for radius, targets, exclude in groups(S)[:2]:
        targets, exclude = targets[:1], exclude[:1]      # the views among them: err needs a view
        want = nr.novel(depth, valid, 1.0, targets, exclude, radius, tol=0.1, volume=slab, want_err=True)
        both_forms(rs, depth, valid, 1.0, targets, exclude, want, "U = %d radius %d" % (U, radius), volume=vol, radius=radius, tol=0.1)


def test_the_width_cap(rs):
    """U = the cap with S = 2, V = 1 runs and matches (64 KiB of LDS, chunks of 32 columns); cap + 1 is refused."""
    from remotesensingproject_amd import _lib
    rng = np.random.RandomState(5)
    depth = rng.uniform(-3.0, 3.0, (2, 1, CAP)).astype(F)
    depth[:, :, ::2] = 1.0
    valid = np.where(rng.uniform(size=depth.shape) < 0.3, 0, 255).astype(np.uint8)
    valid[:, :, 1000:1200] = 0       # a run across several chunks
    targets, exclude = (0.0, 1.0, 0.5, 3.0), (0, 1, -1, -1)
    want = nr.novel(depth, valid, 1.0, targets, exclude, max_gap=0, tol=0.5)
    assert (want["fill"] == nr.LEFT).any() and (want["fill"] == nr.RIGHT).any() and (want["n_src"] >= 2).any()
    both_forms(rs, depth, valid, 1.0, targets, exclude, want, "U = cap", tol=0.5)
    want = nr.novel(depth, valid, 1.0, targets, exclude, max_gap=40, tol=0.5)
    assert (want["fill"] == nr.HOLE).any()
    both_forms(rs, depth, valid, 1.0, targets, exclude, want, "U = cap, max_gap 40", max_gap=40, tol=0.5)
    rc, got = run_entry(rs, np.zeros((2, 1, CAP + 1), F), None, 1.0, targets, exclude)
    assert rc == -2 and b"z-buffer" in _lib.lib().rslf_last_error() and (got["fill"] == 77).all()


def test_one_view_and_that_one_excluded(rs):
    depth, valid = cr.planted(1, 2, 70)
    vol, slab = _volume(rs, 2, 1, 70, 3, F)
    rc, got = run_entry(rs, depth, valid, 1.0, [0.0], [0], want=nr.NAMES, volume=vol)
    assert rc == 0
    for k in nr.NAMES:
        assert not got[k].any(), k          # all holes: every plane holds its empty value
    want = nr.novel(depth, valid, 1.0, [0.0], None, volume=slab, want_err=True)     # nobody excluded: the view itself
    assert (want["fill"] == nr.HIT).any() and (want["n_src"] == 1).any()
    both_forms(rs, depth, valid, 1.0, [0.0], None, want, "S = 1", volume=vol)


def test_infinities_huge_values_and_nans(rs):
    """+-inf, +-1e30, NaN and signed zeros in the planes, and a slope of 1e30: none of them reaches an address, and the planes
    match the yardstick."""
    S, V, U = 9, 2, 160
    depth, valid = nr.field("hole", S, V, U)
    wild = depth.copy()
    wild[::2, :, ::7] = np.inf
    wild[1::2, :, 3::11] = -np.inf
    wild[:, :, 5::13] = 1e30
    wild[:, :, 6::17] = -1e30
    wild[:, :, 9::23] = np.nan
    wild[:, :, 2::19] = -0.0
    wild[::3, :, 4::29] = 0.0
    vol, slab = _volume(rs, V, S, U, 3, F)
    loo = wr.leave_one_out(S)
    for tol in (0.1, np.inf):
        want = nr.novel(wild, valid, 1.0, *loo, max_gap=3, tol=tol, volume=slab, want_err=True)
        assert np.isfinite(want["depth"]).all() and np.isfinite(want["colour"]).all() and (want["n_src"] > 0).mean() > 0.3
        both_forms(rs, wild, valid, 1.0, *loo, want, "wild values, tol %g" % tol, volume=vol, max_gap=3, tol=tol)
    for slope in (1e30, -1e30):
        want = nr.novel(wild, valid, slope, *loo, volume=slab, want_err=True)
        assert (want["fill"] != nr.HOLE).any() and not want["depth"].any()    # only zeros stay in field
        both_forms(rs, wild, valid, slope, *loo, want, "slope %g" % slope, volume=vol)
    tiny = nr.novel(wild, None, 2e-38, (4.0, 8.5), None, volume=slab)     # huge values come into field (2e-38 is a normal float)
    assert (np.abs(tiny["depth"]) >= 1e29).any()
    both_forms(rs, wild, None, 2e-38, (4.0, 8.5), None, tiny, "wild values, tiny slope", volume=vol)


@pytest.mark.parametrize("dtype", [np.uint8, F], ids=["u8", "f32"])
@pytest.mark.parametrize("channels", [1, 3])
def test_volumes(rs, channels, dtype):
    """colour, err and the row sums on uint8 and float volumes of one and three channels; U = 150 is no multiple of four
    (scalar stores), 160 is (16-byte stores).  All seven planes together, device and host forms, and the radiance planes alone."""
    for U in (150, 160):
        V, S = 2, 9
        vol, slab = _volume(rs, V, S, U, channels, dtype, seed=U)
        depth, valid = nr.field("hole", S, V, U)
        loo = wr.leave_one_out(S)
        kw = dict(radius=2, max_gap=3, sources=3, tol=0.1)
        want = nr.novel(depth, valid, 1.0, *loo, volume=slab, want_err=True, **kw)
        assert (want["err"] > 0).mean() > 0.5 and (want["n_src"] >= 2).mean() > 0.3 and ((want["fill"] >= 2) & (want["n_src"] == 0)).any()
        both_forms(rs, depth, valid, 1.0, *loo, want, "U = %d" % U, volume=vol, **kw)
        for k in ("colour", "err", "row_err"):
            for host in (False, True):
                rc, got = run_entry(rs, depth, valid, 1.0, *loo, want=(k,), host=host, volume=vol, **kw)
                assert rc == 0 and list(got) == [k]
                nr.assert_equal(got, want, "%s alone, host=%s" % (k, host), names=(k,))
        targets = (4.5, -1.0)      # colour needs no view among the targets
        got = rs.novel_view(rs.default_context(0), _dev(depth), _dev(valid), vol, 1.0, targets, **kw)
        nr.assert_equal(_host(got), nr.novel(depth, valid, 1.0, targets, volume=slab, **kw), "colour between views",
                        names=("colour", "depth", "fill", "n_src"))


def test_each_output_alone_and_the_warp_underneath(rs):
    """Only the planes asked for are written; each alone holds what it holds among all.  fill == 1 and depth there are
    rslf_view_warp's hit and depth of the same call, bit for bit."""
    S, V, U = 9, 2, 160
    depth, valid = nr.field("hole", S, V, U)
    loo = wr.leave_one_out(S)
    want = nr.field_novel("hole", S, V, U, *loo, 1, max_gap=3)
    for host in (False, True):
        for k in nr.PLANES:
            rc, got = run_entry(rs, depth, valid, 1.0, *loo, radius=1, max_gap=3, tol=0.1, want=(k,), host=host)
            assert rc == 0 and list(got) == [k]
            nr.assert_equal(got, want, "%s alone, host=%s" % (k, host), names=(k,))
    got = rs.novel_view(rs.default_context(0), _dev(depth), _dev(valid), None, 1.0, *loo, radius=1, max_gap=3, tol=0.1, depth=False, n_src=False)
    assert got.fill is not None and [t for t in got if t is not None] == [got.fill]
    novel = _host(rs.novel_view(rs.default_context(0), _dev(depth), _dev(valid), None, 1.0, *loo, radius=1, max_gap=3, tol=0.1))
    warp = rs.view_warp(rs.default_context(0), _dev(depth), _dev(valid), 1.0, *loo, radius=1)
    hit, wdepth = warp.hit.cpu().numpy() != 0, warp.depth.cpu().numpy()
    assert np.array_equal(novel["fill"] == nr.HIT, hit) and 0 < hit.mean() < 1
    assert np.array_equal(cr.bits(novel["depth"])[hit], cr.bits(wdepth)[hit])


def test_the_error_returns(rs):
    """RSLF_ERR_INVALID_ARG (-1), the argument named, nothing launched (the sentinel planes stay), and the context usable
    afterwards; RSLF_ERR_UNSUPPORTED (-2) as the warp's."""
    import torch
    from remotesensingproject_amd import _lib
    L, ctx = _lib.lib(), rs.default_context(0)
    S, V, U = 9, 2, 160
    depth, valid = nr.field("hole", S, V, U)
    err = lambda: L.rslf_last_error()
    for host in (False, True):
        rc, got = run_entry(rs, depth, valid, 1.0, [0.0], host=host, params=False)
        assert rc == -1 and b"params" in err() and (got["fill"] == 77).all()
        rc, got = run_entry(rs, depth, valid, 1.0, [0.0], host=host, sources=0)
        assert rc == -1 and b"sources" in err() and (got["fill"] == 77).all()
        for bad in (-0.5, float("nan"), -float("inf")):
            rc, got = run_entry(rs, depth, valid, 1.0, [0.0], host=host, tol=bad)
            assert rc == -1 and b"tol" in err() and (got["n_src"] == 77).all()
        rc, got = run_entry(rs, depth, valid, 1.0, [0.0], host=host, nearer=0)
        assert rc == -1 and b"nearer" in err() and (got["fill"] == 77).all()
        rc, _ = run_entry(rs, depth, valid, 1.0, [0.0], host=host, want=())
        assert rc == -1 and b"NULL" in err()
        for bad in (float("nan"), float("inf"), 65537.0):
            rc, got = run_entry(rs, depth, valid, 1.0, [1.0, bad], host=host)
            assert rc == -1 and b"targets[1]" in err() and (got["fill"] == 77).all()
    vol, _ = _volume(rs, V, S, U, 1, F)
    other, _ = _volume(rs, V, S + 1, U, 1, F)
    for k in ("colour", "err", "row_err"):
        rc, got = run_entry(rs, depth, valid, 1.0, [0.0], want=(k,))
        assert rc == -1 and b"volume is NULL" in err() and (got[k] == 77).all()
        rc, got = run_entry(rs, depth, valid, 1.0, [0.0], want=(k,), volume=other)
        assert rc == -1 and b"volume is V=" in err() and (got[k] == 77).all()
    for k in ("err", "row_err"):
        for bad in (0.5, -1.0, float(S)):
            rc, got = run_entry(rs, depth, valid, 1.0, [0.0, bad], want=(k,), volume=vol)
            assert rc == -1 and b"targets[1]" in err() and b"view index" in err() and (got[k] == 77).all()
    rc, got = run_entry(rs, depth, valid, 1.0, [0.5, float(S)], want=("colour",), volume=vol)   # colour alone takes any target
    assert rc == 0
    d, v = _dev(depth), _dev(valid)
    t1, par = (C.c_float * 1)(0.0), _lib.RslfNovelViewParams(0, 1, 0, 4, 0.1)
    call = lambda o, dp=None, U_=U, S_=S, V_=V, T=1, t=t1: L.rslf_novel_view(ctx._h, d.data_ptr() if dp is None else dp, v.data_ptr(), S_, V_, U_, 1.0,
                                                                            None, t, None, T, C.byref(par), o)
    assert call(C.byref(_lib.RslfNovelViewOut(fill=v.data_ptr()))) == -1 and b"input plane" in err()
    assert call(C.byref(_lib.RslfNovelViewOut(depth=d.data_ptr()))) == -1 and b"input plane" in err()
    assert call(C.byref(_lib.RslfNovelViewOut())) == -1 and call(None) == -1
    torch.cuda.synchronize()
    assert np.array_equal(v.cpu().numpy(), valid) and cr.bits(d.cpu().numpy()).tolist() == cr.bits(depth).tolist()
    out = torch.zeros((1, V, U), dtype=torch.uint8, device="cuda")
    o = C.byref(_lib.RslfNovelViewOut(fill=out.data_ptr()))
    assert L.rslf_novel_view(ctx._h, None, v.data_ptr(), S, V, U, 1.0, None, t1, None, 1, C.byref(par), o) == -1
    assert call(o, t=None) == -1 and b"targets" in err()
    assert call(o, T=0) == -1 and b"T=" in err()
    assert call(o, S_=0) == -1 and call(o, V_=0) == -1 and call(o, U_=-1) == -1
    assert call(o, U_=CAP + 1) == -2 and b"z-buffer" in err()
    assert call(o, S_=65537) == -2 and b"views" in err()
    assert call(o, V_=1 << 28, T=8) == -2 and b"grid" in err()
    with pytest.raises(ValueError, match="contiguous float32 CUDA"):
        rs.novel_view(ctx, d.double(), None, None, 1.0, [0.0])
    with pytest.raises(ValueError, match="uint8 CUDA tensor of depth_s_v_u's shape"):
        rs.novel_view(ctx, d, v[:, :1], None, 1.0, [0.0])
    with pytest.raises(ValueError, match="pass volume"):
        rs.novel_view(ctx, d, v, None, 1.0, [0.0], err=True)
    # the context is usable
    loo = wr.leave_one_out(S)
    got = rs.novel_view(ctx, d, v, None, 1.0, *loo, radius=1, max_gap=3, tol=0.1, rows=True)
    nr.assert_equal(_host(got), nr.field_novel("hole", S, V, U, *loo, 1, max_gap=3), "after the refusals")


# ---- 3: the objects ----------------------------------------------------------------------------------------------------------

def _read_device(ptr, nbytes):
    """Device memory at a raw address -> host bytes, through the HIP runtime the library itself is bound to."""
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.hipMemcpy.restype = C.c_int
    out = np.empty(nbytes, np.uint8)
    assert L.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), nbytes, 2) == 0   # hipMemcpyDeviceToHost
    return out


def _slab(d):
    """A volume as it holds its radiances, from rslf_volume_describe's pointer and pitch -> [V, S, U, C]."""
    import torch
    torch.cuda.synchronize()
    return np.ascontiguousarray(_read_device(d.d_base, d.bytes).view(F).reshape(d.V, d.S, d.pitch, d.C)[:, :, :d.U])


def _field(S=9, V=12, U=150, seed=11):
    from remotesensingproject_amd.synth import make_lightfield
    return make_lightfield(U, V, S, 1, seed=seed, dmin=-2.0, dmax=2.0, band=4)[0]


def _check_prediction(pred, want, label):
    nr.assert_equal(dict(err=pred.err.cpu().numpy(), fill=pred.fill.cpu().numpy(), n_src=pred.n_src.cpu().numpy(),
                         row_err=pred.row_err.cpu().numpy(), row_cov=pred.row_cov.cpu().numpy()), want, label,
                    names=("err", "fill", "n_src", "row_err", "row_cov"))
    cov = want["row_cov"].astype(np.int64).sum(axis=1)
    assert np.array_equal(pred.coverage, cov / float(want["fill"].shape[1] * want["fill"].shape[2])), label
    some = cov > 0
    assert np.allclose(pred.mean_abs_error[some], want["row_err"].sum(axis=1)[some] / cov[some], rtol=1e-9, atol=0), label
    assert np.isnan(pred.mean_abs_error[~some]).all(), label


def test_depth2d_computer_getters(rs):
    """Depth2DComputer(...).run() on a synthetic field: get_novel_views and get_novel_view_prediction equal the yardstick on
    the object's own downloaded planes, default mask, tolerance (one grid step) and volume; the sweep's planes are what they
    were before the calls."""
    import torch
    vol, D, lo, hi = _field(), 17, -2.0, 2.0
    comp = rs.Depth2DComputer(rs.Volume.from_dense(vol, 1.0, rs.default_context(0)), lo, hi, D)
    comp.run()
    before = comp.results()
    S = vol.shape[1]
    depth, mask = before["depth"], comp.get_valid_depths_mask_s_v_u().cpu().numpy()
    slab = _slab(comp.m_epis.describe())
    step = (hi - lo) / (D - 1)
    targets = (4.0, 3.5, -0.5, 0.0)
    got = _host(comp.get_novel_views(targets, exclude=(4, -1, -1, -1)))
    want = nr.novel(depth, mask, 1.0, targets, (4, -1, -1, -1), tol=step, volume=slab)
    nr.assert_equal(got, want, "get_novel_views", names=("colour", "depth", "fill", "n_src"))
    assert (want["fill"] >= 2).any() and (want["n_src"] >= 2).any()
    own = (np.arange(depth.size).reshape(depth.shape) % 5 != 0).astype(np.uint8) * 255
    got = _host(comp.get_novel_views([2.0], mask=torch.from_numpy(own).cuda(), radius=2, nearer=-1, max_gap=2, sources=2, tol=0.5, colour=False))
    nr.assert_equal(got, nr.novel(depth, own, 1.0, [2.0], None, 2, -1, 2, 2, 0.5), "get_novel_views(mask, ...)", names=("depth", "fill", "n_src"))
    assert "colour" not in got
    loo = wr.leave_one_out(S)
    pred = comp.get_novel_view_prediction()
    _check_prediction(pred, nr.novel(depth, mask, 1.0, *loo, tol=step, volume=slab, want_err=True), "get_novel_view_prediction()")
    warp = comp.get_view_prediction()
    print("novel view: mean abs error", pred.mean_abs_error, "coverage", pred.coverage)
    print("view warp:  mean abs error", warp.mean_abs_error, "coverage", warp.coverage)
    pred = comp.get_novel_view_prediction(targets=[1, 7], radius=3, max_gap=3, sources=2)
    _check_prediction(pred, nr.novel(depth, mask, 1.0, (1.0, 7.0), (1, 7), 3, 1, 3, 2, step, volume=slab, want_err=True),
                      "get_novel_view_prediction(targets, radius, ...)")
    after = comp.results()
    for k in before:
        assert cr.bits(before[k]).tolist() == cr.bits(after[k]).tolist(), k


def test_kept_fine_to_coarse_getters(rs):
    """A kept fine-to-coarse run: the fused result and one coarser level, each with the slope factor its sweep ran with and
    its own kept volume, against the yardstick on the run's own planes; a run without volumes refuses colour and err by name."""
    vol = _field(S=7, V=40, U=96, seed=5)
    kept = rs.fine_to_coarse_run_host(list(vol[..., 0]), -2.0, 2.0, 17, keep=True)
    assert kept.n_levels >= 2 and kept.keep_volumes
    S = kept.S
    loo = wr.leave_one_out(S)
    step = 4.0 / 16
    fused = kept.plane(0, "fused_map").cpu().numpy(), kept.plane(0, "fused_valid").cpu().numpy()
    slab = _slab(kept.volume_desc(0))
    targets = (3.0, 2.5, float(S))
    got = _host(kept.get_novel_views(targets, exclude=(3, -1, -1), max_gap=3))
    want = nr.novel(*fused, 1.0, targets, (3, -1, -1), max_gap=3, tol=step, volume=slab)
    nr.assert_equal(got, want, "fused result", names=("colour", "depth", "fill", "n_src"))
    assert (want["n_src"] >= 2).any()
    _check_prediction(kept.get_novel_view_prediction(), nr.novel(*fused, 1.0, *loo, tol=step, volume=slab, want_err=True), "fused prediction")
    level = kept.n_levels - 1
    slope = F(kept.dims[level][1] / kept.dims[0][1])
    planes = kept.plane(level, "depth").cpu().numpy(), kept.plane(level, "valid").cpu().numpy()
    slab = _slab(kept.volume_desc(level))
    got = _host(kept.get_novel_views(targets, level=level, fused_result=False, radius=2, exclude=(3, -1, -1), tol=0.3))
    want = nr.novel(*planes, slope, targets, (3, -1, -1), 2, tol=0.3, volume=slab)
    nr.assert_equal(got, want, "level %d, slope %g" % (level, slope), names=("colour", "depth", "fill", "n_src"))
    _check_prediction(kept.get_novel_view_prediction(level=level, fused_result=False, nearer=-1, sources=2),
                      nr.novel(*planes, slope, *loo, 0, -1, 0, 2, step, volume=slab, want_err=True), "level prediction")
    with pytest.raises(ValueError, match="finest size"):
        kept.get_novel_views([0.0], level=1)
    with pytest.raises(ValueError, match="level 9"):
        kept.get_novel_view_prediction(level=9, fused_result=False)
    assert cr.bits(fused[0]).tolist() == cr.bits(kept.plane(0, "fused_map").cpu().numpy()).tolist()
    kept.close()
    bare = rs.fine_to_coarse_run_host(list(vol[..., 0]), -2.0, 2.0, 17, keep=True, keep_volumes=False)
    got = _host(bare.get_novel_views(targets, exclude=(3, -1, -1), max_gap=3))
    nr.assert_equal(got, nr.novel(*fused, 1.0, targets, (3, -1, -1), max_gap=3, tol=step), "without volumes", names=("depth", "fill", "n_src"))
    with pytest.raises(ValueError, match="keep_volumes"):
        bare.get_novel_view_prediction()
    with pytest.raises(ValueError, match="keep_volumes"):
        bare.get_novel_views([0.0], colour=True)
    from remotesensingproject_amd import _lib
    err = np.zeros((1,) + bare.dims[0], F)
    o = _lib.RslfNovelViewOut(err=err.ctypes.data)
    par = _lib.RslfNovelViewParams(0, 1, 0, 4, 0.1)
    assert _lib.lib().rslf_f2c_run_novel_view_host(bare._h, bare.ctx._h, 0, 1, (C.c_float * 1)(0.0), None, 1, C.byref(par), C.byref(o)) == -1
    assert b"keep_volumes" in _lib.lib().rslf_last_error()
    bare.close()
