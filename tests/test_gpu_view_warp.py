"""The view warp on the device (rslf_view_warp, k14_view_warp) against tests/view_warp_ref.py, the numpy yardstick written from
the rule: every plane, every pixel, bit for bit; row_err, whose order of summation the rule leaves open, at 1e-9 relative.
tests/test_view_warp_cpu.py shows, on the yardstick alone, that the planted fields make the z-buffer decide: none of these
tests passes on an idle kernel."""
import ctypes as C

import numpy as np
import pytest

import consistency_ref as cr
import view_warp_ref as wr

pytestmark = pytest.mark.gpu
F = np.float32
IDS = ["S%d_V%d_U%d_r%d" % sh for sh in cr.SHAPES]
CAP = 8192   # plan::kWarpMaxU


@pytest.fixture(scope="module")
def rs():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from remotesensingproject_amd import depth
    return depth


def _host(out):
    return {k: t.cpu().numpy() for k, t in zip(wr.NAMES, out) if t is not None}


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()   # (a copy: the planted planes are read-only)


def _shape_of(k, T, V, U, Cn):
    return (T, V) if k.startswith("row_") else (T, V, U, Cn) if k == "colour" else (T, V, U)


def run_entry(rs, depth, valid, slope, targets, exclude=None, radius=0, nearer=1, want=wr.PLANES + ("row_hits",), host=False, volume=None):
    """rslf_view_warp (or its host form) with exactly the planes of `want`; every plane starts from a sentinel, and the ones not
    asked for are handed over as NULL -> (status, dict of the planes asked for)."""
    import torch
    from remotesensingproject_amd import _lib
    L, ctx = _lib.lib(), rs.default_context(0)
    S, V, U = depth.shape
    T = len(targets)
    depth, valid = np.ascontiguousarray(depth, F), None if valid is None else np.ascontiguousarray(valid, np.uint8)
    outs = {k: np.full(_shape_of(k, T, V, U, volume.C if volume is not None else 1), 77, wr.DTYPES[k]) for k in want}
    if host:
        keep = dict(outs)
        ptr = lambda a: None if a is None else a.ctypes.data
        entry, d_in, v_in = L.rslf_view_warp_host, depth, valid
    else:
        keep = {k: _dev(a) for k, a in outs.items()}
        ptr = lambda t: None if t is None else t.data_ptr()
        entry, d_in, v_in = L.rslf_view_warp, _dev(depth), _dev(valid)
    c_out = _lib.RslfViewWarpOut(*(ptr(keep.get(k)) for k in wr.NAMES))
    c_t = (C.c_float * T)(*[float(t) for t in targets])
    c_ex = None if exclude is None else (C.c_int * T)(*[int(e) for e in exclude])
    ctx.use_current_stream()
    rc = entry(ctx._h, ptr(d_in), ptr(v_in), S, V, U, float(slope), volume._h if volume is not None else None, c_t, c_ex, T, int(radius),
               int(nearer), C.byref(c_out))
    torch.cuda.synchronize()
    return rc, {k: (a if host else a.cpu().numpy()) for k, a in keep.items()}


def both_forms(rs, depth, valid, slope, targets, exclude, radius, nearer, want, label):
    """The device form through view_warp (with the counts) and the host form through the C-ABI, against `want`."""
    got = rs.view_warp(rs.default_context(0), _dev(depth), _dev(valid), slope, targets, exclude, radius, nearer, count=True, rows=True)
    wr.assert_equal(_host(got), want, "view_warp " + label)
    rc, got = run_entry(rs, depth, valid, slope, targets, exclude, radius, nearer, host=True)
    assert rc == 0
    wr.assert_equal(got, want, "host form " + label)


# ---- 1: the planted fields ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", cr.SHAPES, ids=IDS)
def test_planted_fields(rs, shape):
    """U below one stride, 300 and 513 across strides and no multiple of four, one view, a radius: every integral target
    leave-one-out in ONE call (T = S); then t = c + 0.5, -1 and S in a second, nobody excluded."""
    S, V, U, radius = shape
    depth, valid = cr.planted(S, V, U)
    loo = wr.leave_one_out(S)
    want = wr.planted_warp(S, V, U, radius, *loo)
    both_forms(rs, depth, valid, 1.0, *loo, radius, 1, want, "leave-one-out %s" % (shape,))
    if S == 1:   # its only view excluded: every plane holds its empty value
        assert not want["hit"].any() and (want["src_view"] == -1).all() and (want["src_col"] == -1).all()
        assert not want["depth"].any() and not want["count"].any() and not want["row_hits"].any()
    targets = (S // 2 + 0.5, -1.0, float(S))
    both_forms(rs, depth, valid, 1.0, targets, None, radius, 1, wr.planted_warp(S, V, U, radius, targets), "between and outside %s" % (shape,))


def test_eleven_scanlines_and_many_targets(rs):
    """More than one XCD round with surplus blocks (V = 11), and more targets than one launch carries (T = 300)."""
    S, V, U = 3, 11, 300
    depth, valid = cr.planted(S, V, U)
    loo = wr.leave_one_out(S)
    both_forms(rs, depth, valid, 1.0, *loo, 0, 1, wr.planted_warp(S, V, U, 0, *loo), "V = 11")
    S, V, U, radius = cr.SHAPES[1]
    depth, valid = cr.planted(S, V, U)
    targets = tuple(-2.0 + k * 0.07 for k in range(300))
    exclude = tuple(k % (S + 1) - 1 for k in range(300))
    both_forms(rs, depth, valid, 1.0, targets, exclude, 3, 1, wr.planted_warp(S, V, U, 3, targets, exclude), "T = 300")


# ---- 2: the other cases --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("slope,nearer,radius,masked", [(0.5, 1, 0, True), (-1.0, 1, 0, True), (1.0, -1, 0, True), (1.0, 1, 1, True),
                                                        (1.0, 1, 0, False), (0.5, -1, 2, False)])
def test_slope_order_radius_and_no_validity_plane(rs, slope, nearer, radius, masked):
    S, V, U, _ = cr.SHAPES[0]
    depth, valid = cr.planted(S, V, U, slope=abs(slope))
    loo = wr.leave_one_out(S)
    want = wr.planted_warp(S, V, U, radius, *loo, nearer=nearer, slope=slope, masked=masked)
    assert (want["count"] >= 2).mean() > 0.5
    both_forms(rs, depth, valid if masked else None, slope, *loo, radius, nearer, want, "slope %g nearer %d radius %d" % (slope, nearer, radius))


def test_every_pixel_invalid_and_t_is_one(rs):
    S, V, U, radius = cr.SHAPES[0]
    depth, valid = cr.planted(S, V, U)
    for d, v in ((depth, np.zeros((S, V, U), np.uint8)), (np.full((S, V, U), np.nan, F), None)):
        rc, got = run_entry(rs, d, v, 1.0, [4.0, 0.5], None)
        assert rc == 0
        assert not got["hit"].any() and not got["depth"].any() and not got["count"].any() and not got["row_hits"].any()
        assert (got["src_view"] == -1).all() and (got["src_col"] == -1).all()
    want = wr.planted_warp(S, V, U, radius, (4.0,), (4,))    # T = 1
    both_forms(rs, depth, valid, 1.0, (4.0,), (4,), radius, 1, want, "T = 1")


def test_the_tie_field(rs):
    """Whole regions of equal disparity: the distance-then-view order decides more than half of the hit pixels
    (tests/test_view_warp_cpu.py recounts the share)."""
    depth = wr.tie_field()
    S = depth.shape[0]
    c = S // 2
    targets, exclude = (float(c), c + 0.5, 0.0, float(S)), (c, -1, 0, -1)
    both_forms(rs, depth, None, 1.0, targets, exclude, 0, 1, wr.warp(depth, None, 1.0, targets, exclude), "tie field")
    both_forms(rs, depth, None, 1.0, targets, exclude, 0, -1, wr.warp(depth, None, 1.0, targets, exclude, 0, -1), "tie field, nearer -1")


def test_signed_zeros_and_rounding_ties(rs):
    """+-0.0 meet in one column (equal depths: the nearer view, then the smaller, wins, and the plane shows the winner's own
    bits); disparities at k + 0.5, whose offsets land on rounding ties, which roundf takes away from zero."""
    zeros = np.zeros((5, 2, 70), F)
    zeros[1::2] = -0.0
    zeros[:, :, 3::5] = -0.0
    zeros[2, :, 10::7] = 1.0
    for nearer in (1, -1):
        want = wr.warp(zeros, None, 1.0, (2.0, 1.5, 0.0), (2, -1, -1), 0, nearer)
        both_forms(rs, zeros, None, 1.0, (2.0, 1.5, 0.0), (2, -1, -1), 0, nearer, want, "signed zeros, nearer %d" % nearer)
        assert (wr.bits(want["depth"]) == 0x80000000).any() and (wr.bits(want["depth"][want["hit"] != 0]) == 0).any()
    half = np.full((9, 2, 70), 0.5, F)
    half[:, :, 1::3] = -0.5
    half[:, :, 2::7] = 1.5
    half[4, :, 10::7] = 2.5
    loo = wr.leave_one_out(9)
    both_forms(rs, half, None, 1.0, *loo, 0, 1, wr.warp(half, None, 1.0, *loo), "d = k + 0.5")
    both_forms(rs, half, None, 1.0, (3.5, 4.25), None, 0, 1, wr.warp(half, None, 1.0, (3.5, 4.25)), "d = k + 0.5, targets between views")


def test_infinities_huge_values_and_nans(rs):
    """+-inf, +-1e30 and NaN as disparities, and a slope of 1e30: all of them are skipped (not ok, or out of field with no
    conversion of the offset), and nothing is written out of place."""
    S, V, U, radius = cr.SHAPES[0]
    depth, valid = cr.planted(S, V, U)
    wild = depth.copy()
    wild[::2, :, ::7] = np.inf
    wild[1::2, :, 3::11] = -np.inf
    wild[:, :, 5::13] = 1e30
    wild[:, :, 6::17] = -1e30
    wild[:, :, 9::23] = np.nan
    loo = wr.leave_one_out(S)
    want = wr.warp(wild, valid, 1.0, *loo)
    assert np.isfinite(want["depth"]).all() and (np.abs(want["depth"]) < 1e29).all() and (want["hit"] != 0).mean() > 0.5
    both_forms(rs, wild, valid, 1.0, *loo, 0, 1, want, "wild values")
    zeroed = wild.copy()
    zeroed[:, :, 4::9] = 0.0
    for slope in (1e30, -1e30):
        want = wr.warp(wild, valid, slope, *loo)
        assert not want["hit"].any()      # every offset is out of range: nothing arrives anywhere
        both_forms(rs, wild, valid, slope, *loo, 0, 1, want, "slope %g" % slope)
        want = wr.warp(zeroed, valid, slope, *loo)
        assert (want["hit"] != 0).any() and not want["depth"].any()   # (a zero offset stays in field: 0 * 1e30)
        both_forms(rs, zeroed, valid, slope, *loo, 0, 1, want, "slope %g, zeros" % slope)
    tiny = wr.warp(wild, None, 2e-38, (4.0, 8.5), None)     # huge values come into field (2e-38 is a normal float)
    assert (np.abs(tiny["depth"]) >= 1e29).any()
    both_forms(rs, wild, None, 2e-38, (4.0, 8.5), None, 0, 1, tiny, "wild values, tiny slope")


def test_each_output_alone_and_all_together(rs):
    """Only the planes asked for are written; each alone holds what it holds among all; with the counts asked for and not,
    the other planes hold the same bits."""
    S, V, U, radius = cr.SHAPES[1]
    depth, valid = cr.planted(S, V, U)
    loo = wr.leave_one_out(S)
    want = wr.planted_warp(S, V, U, radius, *loo)
    names = wr.PLANES + ("row_hits",)
    rc, got = run_entry(rs, depth, valid, 1.0, *loo)
    assert rc == 0
    wr.assert_equal(got, want, "all", names=names)
    for k in names:
        for host in (False, True):
            rc, got = run_entry(rs, depth, valid, 1.0, *loo, want=(k,), host=host)
            assert rc == 0 and list(got) == [k]
            wr.assert_equal(got, want, "%s alone, host=%s" % (k, host), names=(k,))
    without = tuple(k for k in names if k != "count")
    rc, got = run_entry(rs, depth, valid, 1.0, *loo, want=without)
    assert rc == 0
    wr.assert_equal(got, want, "without the counts", names=without)
    got = rs.view_warp(rs.default_context(0), _dev(depth), _dev(valid), 1.0, *loo, depth=False, src=False)
    assert got[1:] == (None,) * 8
    wr.assert_equal(dict(hit=got.hit.cpu().numpy()), want, "hit alone", names=("hit",))


def test_the_width_cap(rs):
    """U = the cap with S = 2, V = 1 runs and matches (96 KiB of LDS with the counts); cap + 1 is refused."""
    from remotesensingproject_amd import _lib
    rng = np.random.RandomState(5)
    depth = rng.uniform(-3.0, 3.0, (2, 1, CAP)).astype(F)
    depth[:, :, ::2] = 1.0
    targets, exclude = (0.0, 1.0, 0.5, 3.0), (0, 1, -1, -1)
    want = wr.warp(depth, None, 1.0, targets, exclude)
    assert (want["count"] >= 2).any() and (want["hit"] == 0).any()
    both_forms(rs, depth, None, 1.0, targets, exclude, 0, 1, want, "U = cap")
    rc, got = run_entry(rs, np.zeros((2, 1, CAP + 1), F), None, 1.0, targets, exclude)
    assert rc == -2 and b"z-buffer" in _lib.lib().rslf_last_error() and (got["hit"] == 77).all()


@pytest.mark.parametrize("channels", [1, 3])
def test_colour_and_err(rs, channels):
    """colour and err on a uint8 volume of (9, 12, 150) built with Volume.from_epis; the yardstick normalises as K0 does,
    F(x) * F(1 / 255).  Device and host forms, all planes together, and the radiance planes alone."""
    V, S, U = 12, 9, 150
    rng = np.random.RandomState(40 + channels)
    raw = rng.randint(0, 256, (V, S, U, channels)).astype(np.uint8)
    vol = rs.Volume.from_epis(list(raw[..., 0] if channels == 1 else raw), ctx=rs.default_context(0))
    depth, valid = cr.planted(S, V, U)
    loo = wr.leave_one_out(S)
    want = wr.warp(depth, valid, 1.0, *loo, volume=wr.normalised(raw), want_err=True)
    assert (want["err"] > 0).mean() > 0.5 and (want["colour"] > 0).any()
    got = rs.view_warp(rs.default_context(0), _dev(depth), _dev(valid), 1.0, *loo, volume=vol, count=True, err=True, rows=True)
    wr.assert_equal(_host(got), want, "view_warp with a volume")
    for host in (False, True):
        rc, got = run_entry(rs, depth, valid, 1.0, *loo, want=wr.NAMES, host=host, volume=vol)
        assert rc == 0
        wr.assert_equal(got, want, "all nine, host=%s" % host)
        for k in ("colour", "err", "row_err"):
            rc, got = run_entry(rs, depth, valid, 1.0, *loo, want=(k,), host=host, volume=vol)
            assert rc == 0 and list(got) == [k]
            wr.assert_equal(got, want, "%s alone, host=%s" % (k, host), names=(k,))
    # colour needs no view among the targets
    targets = (4.5, -1.0)
    got = rs.view_warp(rs.default_context(0), _dev(depth), _dev(valid), 1.0, targets, volume=vol)
    wr.assert_equal(_host(got), wr.warp(depth, valid, 1.0, targets, volume=wr.normalised(raw)), "colour between views",
                    names=("hit", "depth", "src_view", "src_col", "colour"))


def test_the_error_returns(rs):
    """RSLF_ERR_INVALID_ARG (-1), the argument named, nothing launched (the sentinel planes stay), and the context usable
    afterwards; RSLF_ERR_UNSUPPORTED (-2) for the width cap and the grid limit."""
    import torch
    from remotesensingproject_amd import _lib
    L, ctx = _lib.lib(), rs.default_context(0)
    S, V, U, radius = cr.SHAPES[1]
    depth, valid = cr.planted(S, V, U)
    err = lambda: L.rslf_last_error()
    rc, _ = run_entry(rs, depth, valid, 1.0, [0.0], want=())
    assert rc == -1 and b"NULL" in err()
    for bad in (float("nan"), float("inf"), -float("inf"), 65537.0):
        for host in (False, True):
            rc, got = run_entry(rs, depth, valid, 1.0, [1.0, bad], host=host)
            assert rc == -1 and b"targets[1]" in err() and (got["hit"] == 77).all()
    rc, got = run_entry(rs, depth, valid, 1.0, [0.0], nearer=0)
    assert rc == -1 and b"nearer" in err() and (got["depth"].view(np.uint32) == np.float32(77).view(np.uint32)).all()
    vol = rs.Volume.from_epis(list(np.zeros((V, S, U), np.uint8)), ctx=ctx)
    other = rs.Volume.from_epis(list(np.zeros((V, S + 1, U), np.uint8)), ctx=ctx)
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
    t1, none = (C.c_float * 1)(0.0), _lib.RslfViewWarpOut()
    alias = _lib.RslfViewWarpOut(hit=v.data_ptr())
    assert L.rslf_view_warp(ctx._h, d.data_ptr(), v.data_ptr(), S, V, U, 1.0, None, t1, None, 1, 0, 1, C.byref(alias)) == -1
    assert b"input plane" in err()
    alias = _lib.RslfViewWarpOut(depth=d.data_ptr())
    assert L.rslf_view_warp(ctx._h, d.data_ptr(), v.data_ptr(), S, V, U, 1.0, None, t1, None, 1, 0, 1, C.byref(alias)) == -1
    assert L.rslf_view_warp(ctx._h, d.data_ptr(), v.data_ptr(), S, V, U, 1.0, None, t1, None, 1, 0, 1, C.byref(none)) == -1
    assert L.rslf_view_warp(ctx._h, d.data_ptr(), v.data_ptr(), S, V, U, 1.0, None, t1, None, 1, 0, 1, None) == -1
    torch.cuda.synchronize()
    assert np.array_equal(v.cpu().numpy(), valid) and cr.bits(d.cpu().numpy()).tolist() == cr.bits(depth).tolist()
    out = torch.zeros((1, V, U), dtype=torch.uint8, device="cuda")
    o = _lib.RslfViewWarpOut(hit=out.data_ptr())
    assert L.rslf_view_warp(ctx._h, None, v.data_ptr(), S, V, U, 1.0, None, t1, None, 1, 0, 1, C.byref(o)) == -1
    assert L.rslf_view_warp(ctx._h, d.data_ptr(), None, S, V, U, 1.0, None, None, None, 1, 0, 1, C.byref(o)) == -1 and b"targets" in err()
    for T in (0, -2):
        assert L.rslf_view_warp(ctx._h, d.data_ptr(), None, S, V, U, 1.0, None, t1, None, T, 0, 1, C.byref(o)) == -1 and b"T=" in err()
    for shape in ((0, V, U), (S, 0, U), (S, V, -1)):
        assert L.rslf_view_warp(ctx._h, d.data_ptr(), None, *shape, 1.0, None, t1, None, 1, 0, 1, C.byref(o)) == -1
    # past the limits: refused on the numbers alone, before a plane or a target is touched
    assert L.rslf_view_warp(ctx._h, d.data_ptr(), None, S, V, CAP + 1, 1.0, None, t1, None, 1, 0, 1, C.byref(o)) == -2 and b"z-buffer" in err()
    assert L.rslf_view_warp(ctx._h, d.data_ptr(), None, 65537, V, U, 1.0, None, t1, None, 1, 0, 1, C.byref(o)) == -2 and b"views" in err()
    for V_big, T_big in ((1 << 28, 8), ((1 << 31) - 1, 1), (8, 1 << 28)):
        assert L.rslf_view_warp(ctx._h, d.data_ptr(), None, S, V_big, U, 1.0, None, t1, None, T_big, 0, 1, C.byref(o)) == -2
        assert b"grid" in err()
    with pytest.raises(ValueError, match="contiguous float32 CUDA"):
        rs.view_warp(ctx, d.double(), None, 1.0, [0.0])
    with pytest.raises(ValueError, match="uint8 CUDA tensor of depth_s_v_u's shape"):
        rs.view_warp(ctx, d, v[:, :1], 1.0, [0.0])
    with pytest.raises(ValueError, match="pass volume"):
        rs.view_warp(ctx, d, v, 1.0, [0.0], err=True)
    # the context is usable
    loo = wr.leave_one_out(S)
    got = rs.view_warp(ctx, d, v, 1.0, *loo, count=True, rows=True)
    wr.assert_equal(_host(got), wr.planted_warp(S, V, U, 0, *loo), "after the refusals")


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
    wr.assert_equal(dict(err=pred.err.cpu().numpy(), hit=pred.hit.cpu().numpy(), row_err=pred.row_err.cpu().numpy(),
                         row_hits=pred.row_hits.cpu().numpy()), want, label, names=("err", "hit", "row_err", "row_hits"))
    hits = want["row_hits"].astype(np.int64).sum(axis=1)
    assert np.array_equal(pred.coverage, hits / float(want["hit"].shape[1] * want["hit"].shape[2])), label
    some = hits > 0
    assert np.allclose(pred.mean_abs_error[some], want["row_err"].sum(axis=1)[some] / hits[some], rtol=1e-9, atol=0), label
    assert np.isnan(pred.mean_abs_error[~some]).all(), label


@pytest.mark.parametrize("subgrid", [False, True], ids=["grid", "subgrid"])
def test_depth2d_computer_getters(rs, subgrid):
    """Depth2DComputer(...).run() on a synthetic field: get_warped_views and get_view_prediction equal the yardstick on the
    object's own downloaded planes, default mask and volume; the sweep's planes are what they were before the calls."""
    import torch
    vol, D, lo, hi = _field(), 17, -2.0, 2.0
    comp = rs.Depth2DComputer(rs.Volume.from_dense(vol, 1.0, rs.default_context(0)), lo, hi, D, subgrid=subgrid)
    comp.run()
    before = comp.results()
    S = vol.shape[1]
    depth, mask = before["depth"], comp.get_valid_depths_mask_s_v_u().cpu().numpy()
    slab = _slab(comp.m_epis.describe())
    targets = (4.0, 3.5, -0.5, 0.0)
    got = _host(comp.get_warped_views(targets, exclude=(4, -1, -1, -1), count=True))
    want = wr.warp(depth, mask, 1.0, targets, (4, -1, -1, -1), volume=slab)
    wr.assert_equal(got, want, "get_warped_views", names=wr.PLANES + ("colour",))
    assert (want["hit"] != 0).any() and (want["count"] >= 2).any()   # not an idle z-buffer: the sweep's views do meet
    own = (np.arange(depth.size).reshape(depth.shape) % 5 != 0).astype(np.uint8) * 255
    got = _host(comp.get_warped_views([2.0], mask=torch.from_numpy(own).cuda(), radius=2, nearer=-1, colour=False))
    wr.assert_equal(got, wr.warp(depth, own, 1.0, [2.0], None, 2, -1), "get_warped_views(mask, radius, nearer)", names=wr.PLANES[:4])
    assert "colour" not in got
    loo = wr.leave_one_out(S)
    pred = comp.get_view_prediction()
    want = wr.warp(depth, mask, 1.0, *loo, volume=slab, want_err=True)
    _check_prediction(pred, want, "get_view_prediction()")
    print("subgrid", subgrid, "mean abs error", pred.mean_abs_error, "coverage", pred.coverage)
    pred = comp.get_view_prediction(targets=[1, 7], radius=3)
    _check_prediction(pred, wr.warp(depth, mask, 1.0, (1.0, 7.0), (1, 7), 3, volume=slab, want_err=True), "get_view_prediction(targets, radius)")
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
    fused = kept.plane(0, "fused_map").cpu().numpy(), kept.plane(0, "fused_valid").cpu().numpy()
    slab = _slab(kept.volume_desc(0))
    targets = (3.0, 2.5, float(S))
    got = _host(kept.get_warped_views(targets, exclude=(3, -1, -1), count=True))
    want = wr.warp(*fused, 1.0, targets, (3, -1, -1), volume=slab)
    wr.assert_equal(got, want, "fused result", names=wr.PLANES + ("colour",))
    assert (want["count"] >= 2).any()
    _check_prediction(kept.get_view_prediction(), wr.warp(*fused, 1.0, *loo, volume=slab, want_err=True), "fused prediction")
    level = kept.n_levels - 1
    slope = F(kept.dims[level][1] / kept.dims[0][1])
    planes = kept.plane(level, "depth").cpu().numpy(), kept.plane(level, "valid").cpu().numpy()
    slab = _slab(kept.volume_desc(level))
    got = _host(kept.get_warped_views(targets, level=level, fused_result=False, radius=2, exclude=(3, -1, -1)))
    want = wr.warp(*planes, slope, targets, (3, -1, -1), 2, volume=slab)
    wr.assert_equal(got, want, "level %d, slope %g" % (level, slope), names=wr.PLANES[:4] + ("colour",))
    _check_prediction(kept.get_view_prediction(level=level, fused_result=False, nearer=-1),
                      wr.warp(*planes, slope, *loo, 0, -1, volume=slab, want_err=True), "level prediction")
    with pytest.raises(ValueError, match="finest size"):
        kept.get_warped_views([0.0], level=1)
    with pytest.raises(ValueError, match="level 9"):
        kept.get_view_prediction(level=9, fused_result=False)
    assert cr.bits(fused[0]).tolist() == cr.bits(kept.plane(0, "fused_map").cpu().numpy()).tolist()
    kept.close()
    bare = rs.fine_to_coarse_run_host(list(vol[..., 0]), -2.0, 2.0, 17, keep=True, keep_volumes=False)
    got = _host(bare.get_warped_views(targets, exclude=(3, -1, -1)))
    wr.assert_equal(got, wr.warp(*fused, 1.0, targets, (3, -1, -1)), "without volumes", names=wr.PLANES[:4])
    with pytest.raises(ValueError, match="keep_volumes"):
        bare.get_view_prediction()
    with pytest.raises(ValueError, match="keep_volumes"):
        bare.get_warped_views([0.0], colour=True)
    from remotesensingproject_amd import _lib
    err = np.zeros((1,) + bare.dims[0], F)
    o = _lib.RslfViewWarpOut(err=err.ctypes.data)
    assert _lib.lib().rslf_f2c_run_view_warp_host(bare._h, bare.ctx._h, 0, 1, (C.c_float * 1)(0.0), None, 1, 0, 1, C.byref(o)) == -1
    assert b"keep_volumes" in _lib.lib().rslf_last_error()
    bare.close()
