"""The cross-view consistency check on the device (rslf_view_consistency, k12_view_consistency) against
tests/consistency_ref.py, the numpy yardstick written from the rule: every plane, every pixel, bit for bit -- fused included,
whose additions run in ascending view order on both sides.  tests/test_consistency_cpu.py shows, on the yardstick alone, that
every planted field makes the check work: none of these tests passes on an idle kernel."""
import ctypes as C

import numpy as np
import pytest

import consistency_ref as cr

pytestmark = pytest.mark.gpu
F = np.float32
IDS = ["S%d_V%d_U%d_r%d" % sh for sh in cr.SHAPES]
DTYPES = dict(seen=np.int32, agree=np.int32, above=np.int32, below=np.int32, fused=F, valid=np.uint8)


@pytest.fixture(scope="module")
def rs():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from remotesensingproject_amd import depth
    return depth


def _host(out):
    return {k: t.cpu().numpy() for k, t in zip(cr.NAMES, out) if t is not None}


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()   # (a copy: the planted planes are read-only)


def run_entry(rs, depth, valid, slope, tol, radius, min_agree, want=cr.NAMES, host=False):
    """rslf_view_consistency (or its host form) with exactly the planes of `want`; every plane starts from a sentinel, and the
    ones not asked for are handed over as NULL -> (status, dict of the planes asked for)."""
    import torch
    from remotesensingproject_amd import _lib
    L, ctx = _lib.lib(), rs.default_context(0)
    S, V, U = depth.shape
    depth, valid = np.ascontiguousarray(depth, F), None if valid is None else np.ascontiguousarray(valid, np.uint8)
    outs = {k: np.full((S, V, U), 77, DTYPES[k]) for k in want}
    if host:
        keep = dict(outs)
        ptr = lambda a: None if a is None else a.ctypes.data
        entry, d_in, v_in = L.rslf_view_consistency_host, depth, valid
    else:
        keep = {k: _dev(a) for k, a in outs.items()}
        ptr = lambda t: None if t is None else t.data_ptr()
        entry, d_in, v_in = L.rslf_view_consistency, _dev(depth), _dev(valid)
    counts = _lib.RslfViewCounts(*(ptr(keep.get(k)) for k in cr.NAMES[:4]))
    ctx.use_current_stream()
    rc = entry(ctx._h, ptr(d_in), ptr(v_in), S, V, U, float(slope), float(tol), int(radius), int(min_agree), C.byref(counts),
               ptr(keep.get("fused")), ptr(keep.get("valid")))
    torch.cuda.synchronize()
    return rc, {k: (a if host else a.cpu().numpy()) for k, a in keep.items()}


# ---- 1: the planted fields ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", cr.SHAPES, ids=IDS)
def test_planted_fields(rs, shape):
    """U below a wave, U above 256 and no multiple of it, one view, nine and seventeen views (a batch of eight and a remainder),
    one scanline, a radius inside the view range and one its edges cut -- through view_consistency, and through the host form."""
    S, V, U, radius = shape
    depth, valid = cr.planted(S, V, U)
    want = cr.planted_reference(S, V, U, radius, min_agree=2)
    got = rs.view_consistency(rs.default_context(0), _dev(depth), _dev(valid), 1.0, cr.TOL, radius, 2)
    cr.assert_equal_bitwise(_host(got), want, "view_consistency %s" % (shape,))
    rc, got = run_entry(rs, depth, valid, 1.0, cr.TOL, radius, 2, host=True)
    assert rc == 0
    cr.assert_equal_bitwise(got, want, "host form %s" % (shape,))


@pytest.mark.parametrize("order", [1, 2])
def test_the_grid_orders_give_the_same_planes(rs, hooks, order):
    """rslf_ctx_set_debug("consistency_order"): placement only."""
    hooks(consistency_order=order)
    for S, V, U, radius in cr.SHAPES[:2] + [(3, 11, 300, 0)]:   # (11 scanlines: more than one XCD round, and surplus blocks)
        depth, valid = cr.planted(S, V, U)
        got = rs.view_consistency(rs.default_context(0), _dev(depth), _dev(valid), 1.0, cr.TOL, radius, 1)
        cr.assert_equal_bitwise(_host(got), cr.planted_reference(S, V, U, radius, min_agree=1), "order %d %s" % (order, (S, V, U)))


def test_eleven_scanlines_in_the_default_order(rs):
    S, V, U = 3, 11, 300
    depth, valid = cr.planted(S, V, U)
    got = rs.view_consistency(rs.default_context(0), _dev(depth), _dev(valid), 1.0, cr.TOL, 0, 1)
    cr.assert_equal_bitwise(_host(got), cr.planted_reference(S, V, U, 0, min_agree=1), "V = 11")


# ---- 2: the other cases --------------------------------------------------------------------------------------------------------

def test_without_the_validity_plane(rs):
    S, V, U, radius = cr.SHAPES[0]
    depth, _ = cr.planted(S, V, U)
    got = rs.view_consistency(rs.default_context(0), _dev(depth), None, 1.0, cr.TOL, radius, 1)
    cr.assert_equal_bitwise(_host(got), cr.planted_reference(S, V, U, radius, min_agree=1, masked=False), "valid NULL")


def test_each_output_alone_and_all_together(rs):
    """Only the planes asked for are written; each alone holds what it holds among all six."""
    S, V, U, radius = cr.SHAPES[1]
    depth, valid = cr.planted(S, V, U)
    want = cr.planted_reference(S, V, U, radius, min_agree=1)
    rc, got = run_entry(rs, depth, valid, 1.0, cr.TOL, radius, 1)
    assert rc == 0
    cr.assert_equal_bitwise(got, want, "all six")
    for k in cr.NAMES:
        for host in (False, True):
            rc, got = run_entry(rs, depth, valid, 1.0, cr.TOL, radius, 1, want=(k,), host=host)
            assert rc == 0 and list(got) == [k]
            cr.assert_equal_bitwise(got, want, "%s alone, host=%s" % (k, host), names=(k,))
    got = rs.view_consistency(rs.default_context(0), _dev(depth), _dev(valid), 1.0, cr.TOL, radius, 1, counts=False, fused=False)
    assert got[:5] == (None,) * 5
    cr.assert_equal_bitwise(dict(valid=got.valid.cpu().numpy()), want, "valid alone", names=("valid",))
    got = rs.view_consistency(rs.default_context(0), _dev(depth), _dev(valid), 1.0, cr.TOL, radius, 1, counts=False)
    assert got[:4] == (None,) * 4
    cr.assert_equal_bitwise(_host(got), want, "fused and valid", names=("fused", "valid"))


@pytest.mark.parametrize("slope,tol", [(0.5, cr.TOL), (1.0, 0.0), (0.5, 0.0), (-1.0, cr.TOL)])
def test_slope_and_tolerance(rs, slope, tol):
    """slope 0.5 (a pyramid level), tol 0 (only equal values agree: the jitter leaves few) and a mirrored field."""
    S, V, U, radius = cr.SHAPES[0]
    depth, valid = cr.planted(S, V, U, slope=abs(slope))
    want = cr.planted_reference(S, V, U, radius, min_agree=1, slope=abs(slope), tol=tol) if slope > 0 else \
        cr.consistency(depth, valid, slope, tol, radius, 1)
    got = rs.view_consistency(rs.default_context(0), _dev(depth), _dev(valid), slope, tol, radius, 1)
    cr.assert_equal_bitwise(_host(got), want, "slope %g tol %g" % (slope, tol))
    if tol == 0.0 and slope == 1.0:   # exact agreement happens: a constant plane agrees everywhere in field
        flat = np.full((5, 2, 70), 0.75, F)
        got = _host(rs.view_consistency(rs.default_context(0), _dev(flat), None, 1.0, 0.0))
        cr.assert_equal_bitwise(got, cr.consistency(flat, None, 1.0, 0.0), "constant plane, tol 0")
        assert (got["agree"] == got["seen"]).all() and got["agree"].max() == 4 and (got["fused"] == F(0.75)).all()


def test_negative_disparities_and_rounding_ties(rs):
    """The planted field negated (targets to the other side), and a plane of d = 0.5: every odd view distance lands on a tie,
    which roundf takes away from zero -- +-0.5 to +-1 --, on the device as in the yardstick."""
    S, V, U, radius = cr.SHAPES[0]
    depth, valid = cr.planted(S, V, U)
    neg = -depth
    got = rs.view_consistency(rs.default_context(0), _dev(neg), _dev(valid), 1.0, cr.TOL, radius, 1)
    cr.assert_equal_bitwise(_host(got), cr.consistency(neg, valid, 1.0, cr.TOL, radius, 1), "negated field")
    half = np.full((9, 2, 70), 0.5, F)
    half[:, :, 1::3] = -0.5
    half[4, :, 10::7] = 3.0   # markers: a tie taken the wrong way reads a neighbour of another class
    got = _host(rs.view_consistency(rs.default_context(0), _dev(half), None, 1.0, cr.TOL, 0, 0))
    want = cr.consistency(half, None, 1.0, cr.TOL, 0, 0)
    cr.assert_equal_bitwise(got, want, "d = +-0.5")
    assert (want["above"] > 0).any() and (want["below"] > 0).any() and (want["agree"] > 0).any()


def test_infinities_huge_values_and_nans(rs):
    """+-inf, +-1e30 and NaN as targets (nothing: not ok; 1e30 is ok and every other view is out of field) and as neighbours
    (seen only; 1e30: above), no conversion of an offset out of range."""
    S, V, U, radius = cr.SHAPES[0]
    depth, valid = cr.planted(S, V, U)
    wild = depth.copy()
    wild[::2, :, ::7] = np.inf
    wild[1::2, :, 3::11] = -np.inf
    wild[:, :, 5::13] = 1e30
    wild[:, :, 6::17] = -1e30
    wild[:, :, 9::23] = np.nan
    wild[3, :, 100:140] = 3e38    # neighbours whose difference overflows (under the tiny slope below, where they are in
    wild[4, :, 100:140] = -3e38   # field for each other): +-inf, classified above / below, never a NaN
    want = cr.consistency(wild, valid, 1.0, cr.TOL, radius, 1)
    got = rs.view_consistency(rs.default_context(0), _dev(wild), _dev(valid), 1.0, cr.TOL, radius, 1)
    cr.assert_equal_bitwise(_host(got), want, "wild values")
    ok_huge = (wild == F(1e30)) & (valid != 0)
    assert ok_huge.any() and not want["seen"][ok_huge].any() and (want["valid"][ok_huge] == 0).all()
    assert np.isfinite(want["fused"]).all()
    tiny = cr.consistency(wild, None, 2e-38, cr.TOL, radius, 0)    # huge values come into field (2e-38 is a normal float)
    got = rs.view_consistency(rs.default_context(0), _dev(wild), None, 2e-38, cr.TOL, radius, 0)
    cr.assert_equal_bitwise(_host(got), tiny, "wild values, tiny slope")
    assert tiny["below"][3, :, 110:130].all() and tiny["above"][4, :, 110:130].all()


def test_every_pixel_invalid(rs):
    """The workgroup-uniform early exit: nothing is ok anywhere, and every plane asked for is still written."""
    S, V, U, radius = cr.SHAPES[0]
    depth, _ = cr.planted(S, V, U)
    for d, v in ((depth, np.zeros((S, V, U), np.uint8)), (np.full((S, V, U), np.nan, F), None)):
        rc, got = run_entry(rs, d, v, 1.0, cr.TOL, radius, 0)
        assert rc == 0
        for k in cr.NAMES:
            assert not got[k].any(), k
    # ... and one segment of one row alone (columns 256 .. 299 of view 2, scanline 1)
    valid = np.full((S, V, U), 255, np.uint8)
    valid[2, 1, 256:] = 0
    got = rs.view_consistency(rs.default_context(0), _dev(depth), _dev(valid), 1.0, cr.TOL, radius, 0)
    cr.assert_equal_bitwise(_host(got), cr.consistency(depth, valid, 1.0, cr.TOL, radius, 0), "one dead segment")


@pytest.mark.parametrize("min_agree", [0, 1, 9])
def test_min_agree(rs, min_agree):
    S, V, U, radius = cr.SHAPES[0]
    depth, valid = cr.planted(S, V, U)
    want = cr.planted_reference(S, V, U, radius, min_agree=min_agree)
    got = rs.view_consistency(rs.default_context(0), _dev(depth), _dev(valid), 1.0, cr.TOL, radius, min_agree)
    cr.assert_equal_bitwise(_host(got), want, "min_agree %d" % min_agree)
    n = int((want["valid"] == 255).sum())
    assert (n == 0) == (min_agree == S)


def test_the_error_returns(rs):
    """RSLF_ERR_INVALID_ARG (-1): every output NULL, a tolerance that is negative or not finite, a negative min_agree, an
    output that is an input -- valid_out may not alias valid --, a NULL depth plane, no shape.  RSLF_ERR_UNSUPPORTED (-2): past
    the grid's limits.  Nothing is launched: the sentinel planes stay."""
    import torch
    from remotesensingproject_amd import _lib
    L, ctx = _lib.lib(), rs.default_context(0)
    S, V, U, radius = cr.SHAPES[1]
    depth, valid = cr.planted(S, V, U)
    rc, _ = run_entry(rs, depth, valid, 1.0, cr.TOL, 0, 0, want=())
    assert rc == -1 and b"NULL" in L.rslf_last_error()
    for bad in (-0.5, float("nan"), float("inf")):
        for host in (False, True):
            rc, got = run_entry(rs, depth, valid, 1.0, bad, 0, 0, host=host)
            assert rc == -1 and b"tol" in L.rslf_last_error() and (got["seen"] == 77).all()
    rc, got = run_entry(rs, depth, valid, 1.0, cr.TOL, 0, -1)
    assert rc == -1 and b"min_agree" in L.rslf_last_error() and (got["valid"] == 77).all()
    d, v = _dev(depth), _dev(valid)
    none = _lib.RslfViewCounts()
    assert L.rslf_view_consistency(ctx._h, d.data_ptr(), v.data_ptr(), S, V, U, 1.0, 0.1, 0, 0, C.byref(none), None, v.data_ptr()) == -1
    assert b"input plane" in L.rslf_last_error()
    assert L.rslf_view_consistency(ctx._h, d.data_ptr(), v.data_ptr(), S, V, U, 1.0, 0.1, 0, 0, None, d.data_ptr(), None) == -1
    assert L.rslf_view_consistency(ctx._h, d.data_ptr(), v.data_ptr(), S, V, U, 1.0, 0.1, 0, 0, None, None, None) == -1
    torch.cuda.synchronize()
    assert np.array_equal(v.cpu().numpy(), valid) and cr.bits(d.cpu().numpy()).tolist() == cr.bits(depth).tolist()
    out = torch.zeros((S, V, U), dtype=torch.uint8, device="cuda")
    assert L.rslf_view_consistency(ctx._h, None, v.data_ptr(), S, V, U, 1.0, 0.1, 0, 0, None, None, out.data_ptr()) == -1
    for shape in ((0, V, U), (S, 0, U), (S, V, -1)):
        assert L.rslf_view_consistency(ctx._h, d.data_ptr(), None, *shape, 1.0, 0.1, 0, 0, None, None, out.data_ptr()) == -1
    # past the grid: refused on the numbers alone, before a plane is touched
    for shape in ((1 << 20, 1 << 10, 1 << 12), (1, 1, (1 << 30) + 1), (1 << 30, 8, 1)):
        assert L.rslf_view_consistency(ctx._h, d.data_ptr(), None, *shape, 1.0, 0.1, 0, 0, None, None, out.data_ptr()) == -2
        assert b"grid" in L.rslf_last_error()
    with pytest.raises(ValueError, match="contiguous float32 CUDA"):
        rs.view_consistency(ctx, d.double(), None, 1.0, 0.1)
    with pytest.raises(ValueError, match="uint8 CUDA tensor of depth_s_v_u's shape"):
        rs.view_consistency(ctx, d, v[:, :1], 1.0, 0.1)


# ---- 3: the objects ----------------------------------------------------------------------------------------------------------

def _field(S=9, V=12, U=150, seed=11):
    from remotesensingproject_amd.synth import make_lightfield
    return make_lightfield(U, V, S, 1, seed=seed, dmin=-2.0, dmax=2.0, band=4)[0]


@pytest.mark.parametrize("subgrid", [False, True], ids=["grid", "subgrid"])
def test_depth2d_computer_getter(rs, subgrid):
    """Depth2DComputer(...).run() on a synthetic field: the getter equals the yardstick on the object's own downloaded planes
    -- default tolerance (one grid step) and mask, then a radius, a min_agree and a mask of the caller's --, and every plane of
    the sweep is what it was before the calls."""
    import torch
    vol, D, lo, hi = _field(), 17, -2.0, 2.0
    comp = rs.Depth2DComputer(rs.Volume.from_dense(vol, 1.0, rs.default_context(0)), lo, hi, D, subgrid=subgrid)
    comp.run()
    before = comp.results()
    depth, mask = before["depth"], comp.get_valid_depths_mask_s_v_u().cpu().numpy()
    step = (hi - lo) / (D - 1)
    got = _host(comp.get_consistency())
    want = cr.consistency(depth, mask, 1.0, step, 0, 0)
    cr.assert_equal_bitwise(got, want, "get_consistency()")
    print("subgrid", subgrid, cr.shares(depth, mask, want))
    assert (want["agree"] > 0).any() and (want["seen"] > 0).any()   # not an idle check: the sweep's views do meet
    own = (np.arange(depth.size).reshape(depth.shape) % 5 != 0).astype(np.uint8) * 255
    got = _host(comp.get_consistency(tol=0.3, radius=2, min_agree=3, mask=torch.from_numpy(own).cuda()))
    cr.assert_equal_bitwise(got, cr.consistency(depth, own, 1.0, 0.3, 2, 3), "get_consistency(tol, radius, min_agree, mask)")
    only = comp.get_consistent_depths_mask_s_v_u(min_agree=2).cpu().numpy()
    assert np.array_equal(only, cr.consistency(depth, mask, 1.0, step, 0, 2)["valid"]) and (only == 255).any()
    after = comp.results()
    for k in before:
        assert cr.bits(before[k]).tolist() == cr.bits(after[k]).tolist(), k


def test_kept_fine_to_coarse_getter(rs):
    """A kept fine-to-coarse run: the fused result and every level, each with the slope factor its sweep ran with
    (U_level / U_0), against the yardstick on the run's own planes; the run's planes are unchanged."""
    vol = _field(S=7, V=40, U=96, seed=5)
    kept = rs.fine_to_coarse_run_host(list(vol[..., 0]), -2.0, 2.0, 17, keep=True)
    assert kept.n_levels >= 2
    names = [(l, k) for l in range(kept.n_levels) for k in ("depth", "valid")] + [(0, "fused_map"), (0, "fused_valid")]
    before = {n: kept.plane(*n).cpu().numpy() for n in names}
    step = 4.0 / 16
    got = _host(kept.get_consistency())
    want = cr.consistency(before[(0, "fused_map")], before[(0, "fused_valid")], 1.0, step, 0, 0)
    cr.assert_equal_bitwise(got, want, "fused result")
    assert (want["agree"] > 0).any()
    for l in range(kept.n_levels):
        slope = F(kept.dims[l][1] / kept.dims[0][1])
        got = _host(kept.get_consistency(level=l, fused_result=False, tol=0.2, radius=2, min_agree=1))
        want = cr.consistency(before[(l, "depth")], before[(l, "valid")], slope, 0.2, 2, 1)
        cr.assert_equal_bitwise(got, want, "level %d, slope %g" % (l, slope))
        assert (want["agree"] > 0).any()
    with pytest.raises(ValueError, match="finest size"):
        kept.get_consistency(level=1)
    with pytest.raises(ValueError, match="level 9"):
        kept.get_consistency(level=9, fused_result=False)
    from remotesensingproject_amd import _lib
    assert _lib.lib().rslf_f2c_run_consistency(kept._h, kept.ctx._h, 1, 1, 0.1, 0, 0, None, None, None) == -1
    for n in names:
        assert cr.bits(before[n]).tolist() == cr.bits(kept.plane(*n).cpu().numpy()).tolist(), n
    kept.close()
