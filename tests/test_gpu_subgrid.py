"""Sub-grid disparities in the pile step on the device (k9_subgrid_refine; rslf_subgrid_refine and the *_sub entries) against
tests/subgrid_ref.py -- oracle_np.scan_pixel's rows through the rule, oracle_np.selective_median on the refined plane.
Every comparison is bit for bit.

Base field of the rslf_subgrid_refine cases: V = 7 scanlines, S = 9 views of uniform noise with columns 40-51 dark (the
shadow cut leaves them without a disparity: idx = -1), hypotheses in [-2, 5] so that the outer ones run off the row.  The
arg-max and score planes come from the device's own scan (whichever kernel the case selects); the reference asserts that
the arg max is the row's."""
import ctypes as C

import numpy as np
import pytest

import subgrid_ref as sr

pytestmark = pytest.mark.gpu

V, S, S_HAT = 7, 9, 4
DMIN, DMAX, FILL = -2.0, 5.0, -7.0
GENERIC, REG, STREAM = 0, 1, 2   # RSLF_SCAN_*
_cache = {}


@pytest.fixture(scope="module")
def rs():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from remotesensingproject_amd import depth
    return depth


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, want, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
    g = got.view(np.uint32) if got.dtype == np.float32 else got
    w = want.view(np.uint32) if want.dtype == np.float32 else want
    bad = np.argwhere(g != w)
    assert bad.size == 0, "%s: %d of %d values differ, first at %s: got %r want %r" % (
        label, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def field(C_, U, offset=0.0):
    key = ("field", C_, U, offset)
    if key not in _cache:
        vol = np.random.default_rng(900 + 10 * C_ + U).uniform(0.0, 1.0, size=(V, S, U, C_)).astype(np.float32)
        vol[:, :, 40:52] = 0.01
        _cache[key] = (vol - np.float32(offset)).astype(np.float32)
    return _cache[key]


def ranges(U):
    """Seeded per-pixel [lo, hi] inside [-2, 5], lo == hi on every 7th pixel."""
    rng = np.random.default_rng(1234 + U)
    lo = rng.uniform(DMIN, 1.0, size=(V, U)).astype(np.float32)
    hi = np.minimum((lo + rng.uniform(0.5, 4.0, size=(V, U)).astype(np.float32)).astype(np.float32), np.float32(DMAX))
    flat = (np.arange(V * U).reshape(V, U) % 7) == 0
    hi[flat] = lo[flat]
    return lo, hi


def oracle_params(interp=0, median=5):
    from oracle import oracle_np as onp
    p = onp.default_params()
    p["interpolation"] = interp
    p["median_filter_size"] = median
    return p


def device_scan(rs, vol_np, D, lo, hi, params):
    """Edge confidence and scan on the device: the volume, the planes (torch) and the scan's stats."""
    import torch
    dev = rs.Volume.from_dense(vol_np, 1.0, rs.default_context(0))
    n, C_ = (dev.V, dev.U), dev.C
    pl = dict(Ce=torch.zeros(n, dtype=torch.float32, device="cuda"), Cd=torch.zeros(n, dtype=torch.float32, device="cuda"),
              depth=torch.zeros(n, dtype=torch.float32, device="cuda"), rbar=torch.zeros(n + (C_,), dtype=torch.float32, device="cuda"),
              idx=torch.full(n, -5, dtype=torch.int32, device="cuda"), score=torch.full(n, FILL, dtype=torch.float32, device="cuda"))
    pl["mask"] = rs.compute_1D_edge_confidence_pile(dev, S_HAT, pl["Ce"], params)
    st = rs.compute_1D_depth_epi(dev, lo, hi, D, S_HAT, pl["Ce"], pl["mask"], pl["Cd"], pl["depth"], pl["rbar"], params,
                                 idx_v_u=pl["idx"], score_v_u=pl["score"], want_stats=True)
    return dev, pl, st


def filled(torch, shape):
    return torch.full(shape, FILL, dtype=torch.float32, device="cuda")


# name -> (C, U, D, interpolation, offset, per-pixel ranges, hooks, the scan kernel expected)
CASES = {
    "u70": (1, 70, 9, 0, 0.0, False, {}, REG),                 # one partial workgroup
    "u300": (1, 300, 9, 0, 0.0, False, {}, REG),               # two workgroups, the last partial
    "d2": (1, 70, 2, 0, 0.0, False, {}, REG),                  # no interior
    "d3": (1, 70, 3, 0, 0.0, False, {}, REG),
    "rgb": (3, 70, 9, 0, 0.0, False, {}, REG),
    "ranges": (1, 70, 9, 0, 0.0, True, {}, REG),
    "rgb_ranges": (3, 70, 9, 0, 0.0, True, {}, REG),
    "nearest": (1, 70, 9, 1, 0.0, False, {}, GENERIC),
    "negative": (1, 70, 9, 0, 0.3, False, {}, GENERIC),         # radiances below zero: the scan takes the generic kernel
    "generic": (1, 70, 9, 0, 0.0, False, dict(force_scan="generic"), GENERIC),
    "stream": (1, 70, 9, 0, 0.0, False, dict(force_scan="stream"), STREAM),
    "rgb_generic": (3, 70, 9, 0, 0.0, False, dict(force_scan="generic"), GENERIC),
    "rgb_stream": (3, 70, 9, 0, 0.0, False, dict(force_scan="stream"), STREAM),
}


@pytest.mark.parametrize("name", list(CASES))
def test_refine_against_the_reference(rs, hooks, name):
    """rslf_subgrid_refine on the planes of the device's own scan: disp, left and right against subgrid_ref at every pixel
    with idx >= 0, the caller's fill elsewhere; the same planes without the score plane; disp against rslf_depth_epi_peaks';
    left / right against the columns idx -+ 1 of rslf_depth_epi_scores; in place on the depth plane."""
    import torch
    C_, U, D, interp, offset, planes, hook, kernel = CASES[name]
    hooks(**hook)
    vol = field(C_, U, offset)
    params = rs.Depth1DParameters(par_interpolation_class=interp)
    lo_np, hi_np = ranges(U) if planes else (np.float32(DMIN), np.float32(DMAX))
    lo, hi = (torch.from_numpy(lo_np).cuda(), torch.from_numpy(hi_np).cuda()) if planes else (DMIN, DMAX)
    dev, pl, st = device_scan(rs, vol, D, lo, hi, params)
    assert st.scan_kernel == kernel, st.scan_kernel
    hooks(force_scan=0)
    out = rs.subgrid_refine(dev, lo, hi, D, S_HAT, pl["idx"], pl["score"], params,
                            disp=filled(torch, (V, U)), left=filled(torch, (V, U)), right=filled(torch, (V, U)))
    own = rs.subgrid_refine(dev, lo, hi, D, S_HAT, pl["idx"], None, params,
                            disp=filled(torch, (V, U)), left=filled(torch, (V, U)), right=filled(torch, (V, U)))
    in_place = pl["depth"].clone()
    rs.subgrid_refine(dev, lo, hi, D, S_HAT, pl["idx"], pl["score"], params, disp=in_place, neighbours=False)
    final_mask = pl["mask"]
    pk = rs.compute_1D_depth_peaks(dev, lo, hi, D, S_HAT, params, final_mask)
    rows = rs.compute_1D_depth_scores(dev, lo, hi, D, S_HAT, params, final_mask)
    torch.cuda.synchronize()
    idx = pl["idx"].cpu().numpy()
    has = idx >= 0
    assert has.sum() >= 300 and (~has).sum() >= 20 and np.array_equal(has, final_mask.cpu().numpy() != 0)
    assert offset != 0.0 or (idx[:, 40:52] == -1).all()   # (moved below zero the dark columns are no shadow)
    key = ("ref", C_, U, D, interp, offset, planes)
    if key not in _cache:
        _cache[key] = (idx.copy(),) + sr.refine(vol, idx, lo_np, hi_np, D, S_HAT, oracle_params(interp), fill=np.float32(FILL), scan_plane=True)
    ref_idx, disp, left, right = _cache[key]
    assert_same(idx, ref_idx, name + ": every scan kernel gives the same arg max")
    for n, g, w in (("disp", out.disp, disp), ("left", out.left, left), ("right", out.right, right)):
        assert_same(g.cpu().numpy(), w, "%s: %s" % (name, n))
    for n, g, w in zip(("disp", "left", "right"), own, out):
        assert_same(g.cpu().numpy(), w.cpu().numpy(), "%s: %s without the score plane" % (name, n))
    # in place: the refined value where the scan gave a disparity, the plane's own (the zeros it came in with) elsewhere
    depth = pl["depth"].cpu().numpy()
    assert_same(in_place.cpu().numpy(), np.where(has, disp, depth).astype(np.float32), name + ": in place")
    # the peaks' disp from whole rows, and the rows' own columns
    assert_same(pk.idx.cpu().numpy(), idx, name + ": peaks idx")
    assert_same(pk.disp.cpu().numpy()[has], disp[has], name + ": rslf_depth_epi_peaks' disp")
    rows = rows.cpu().numpy()
    vv, uu = np.nonzero(has)
    ii = idx[vv, uu]
    assert_same(out.left.cpu().numpy()[vv, uu], np.where(ii > 0, rows[vv, uu, np.maximum(ii - 1, 0)], np.float32(0)).astype(np.float32),
                name + ": left against the score rows")
    assert_same(out.right.cpu().numpy()[vv, uu], np.where(ii < D - 1, rows[vv, uu, np.minimum(ii + 1, D - 1)], np.float32(0)).astype(np.float32),
                name + ": right against the score rows")
    # the grid value: what the scan wrote; D = 2 has no interior, so nothing moves; D = 9 moves most pixels
    grid = np.array([sr.grid_value(i, D, l, h) for i, l, h in zip(ii, np.broadcast_to(lo_np, (V, U))[vv, uu], np.broadcast_to(hi_np, (V, U))[vv, uu])], np.float32)
    assert_same(depth[vv, uu], grid, name + ": the scan's grid values")
    moved = int((bits(disp[vv, uu]) != bits(grid)).sum())
    ends = int(((ii == 0) | (ii == D - 1)).sum())
    print("%s: %d pixels, %d at an end of the grid, %d moved off it" % (name, len(ii), ends, moved))
    if D == 2:
        assert moved == 0 and ends == len(ii)
    else:
        assert moved >= 50 and (D == 3 or ends >= 10)
    if planes:
        flat = (lo_np == hi_np) & has
        assert flat.sum() >= 30 and np.array_equal(bits(disp[flat]), bits(lo_np[flat]))


@pytest.mark.parametrize("C_", [1, 3])
def test_winners_forced_to_both_ends(rs, C_):
    """An arg-max plane made by hand: 0 and D - 1 in turn, every interior index, -1 and indices outside the grid.  No score
    plane, so the kernel scores the winner itself.  Pixels with idx < 0 or >= D keep the caller's fill."""
    import torch
    U, D = 70, 9
    vol = field(C_, U)
    dev = rs.Volume.from_dense(vol, 1.0, rs.default_context(0))
    idx = (np.arange(V * U).reshape(V, U) % (D + 3)).astype(np.int32)          # 0 .. D + 2
    idx[idx == D] = -1
    idx[idx == D + 1] = D
    idx[idx == D + 2] = 2 ** 30
    idx[0, ::2], idx[0, 1::2] = 0, D - 1
    idx[1, :] = -1
    out = rs.subgrid_refine(dev, DMIN, DMAX, D, S_HAT, torch.from_numpy(idx).cuda(), None, None,
                            disp=filled(torch, (V, U)), left=filled(torch, (V, U)), right=filled(torch, (V, U)))
    torch.cuda.synchronize()
    inside = np.where((idx >= 0) & (idx < D), idx, -1).astype(np.int32)
    assert (inside == 0).sum() >= 60 and (inside == D - 1).sum() >= 60 and (inside < 0).sum() >= 150
    disp, left, right = sr.refine(vol, inside, DMIN, DMAX, D, S_HAT, oracle_params(), fill=np.float32(FILL))
    assert_same(out.disp.cpu().numpy(), disp, "forced ends: disp")
    assert_same(out.left.cpu().numpy(), left, "forced ends: left")
    assert_same(out.right.cpu().numpy(), right, "forced ends: right")
    first, last = inside == 0, inside == D - 1
    assert (left[first] == 0).all() and (right[last] == 0).all()
    assert np.array_equal(bits(disp[first]), bits(np.full(first.sum(), DMIN, np.float32)))
    assert np.array_equal(bits(disp[last]), bits(np.full(last.sum(), sr.grid_value(D - 1, D, DMIN, DMAX), np.float32)))


def test_errors_and_an_open_sweep(rs):
    """NULL planes, dim_d < 2, one range plane, a bad s_hat, subgrid = 2: a status and a message, nothing launched.  Inside an
    open sweep the refinement is legal: it uses no context list."""
    import torch
    from remotesensingproject_amd import _lib
    L, vp = _lib.lib(), C.c_void_p
    U, D = 70, 9
    ctx, p = rs.default_context(0), rs.Depth1DParameters().to_c()
    dev = rs.Volume.from_dense(field(1, U), 1.0, ctx)
    idx = torch.full((V, U), 3, dtype=torch.int32, device="cuda")
    disp = filled(torch, (V, U))
    ctx.use_current_stream()

    def call(**kw):
        a = dict(lo=None, hi=None, D=D, s_hat=S_HAT, idx=idx.data_ptr(), disp=disp.data_ptr())
        a.update(kw)
        return L.rslf_subgrid_refine(ctx._h, dev._h, vp(a["lo"]), vp(a["hi"]), DMIN, DMAX, a["D"], a["s_hat"], C.byref(p), vp(a["idx"]),
                                     None, vp(a["disp"]), None, None)

    for kw in (dict(idx=None), dict(disp=None), dict(D=1), dict(lo=disp.data_ptr()), dict(hi=disp.data_ptr()), dict(s_hat=S), dict(s_hat=-1)):
        assert call(**kw) == -1 and L.rslf_last_error(), kw
    torch.cuda.synchronize()
    assert (disp == FILL).all().item()
    planes = [torch.zeros((V, U), dtype=torch.float32, device="cuda") for _ in range(4)]
    mask = torch.zeros((V, U), dtype=torch.uint8, device="cuda")
    rbar = torch.zeros((V, U, 1), dtype=torch.float32, device="cuda")
    rc = L.rslf_depth1d_pile_run_sub(ctx._h, dev._h, DMIN, DMAX, D, S_HAT, C.byref(p), vp(planes[0].data_ptr()), vp(mask.data_ptr()),
                                     vp(planes[1].data_ptr()), vp(planes[2].data_ptr()), vp(rbar.data_ptr()), None, None, None, None, 2)
    assert rc == -1 and b"subgrid" in L.rslf_last_error()
    cm = torch.zeros((S, V, U), dtype=torch.uint8, device="cuda")
    assert L.rslf_sweep_begin(ctx._h, dev._h, vp(cm.data_ptr()), None, D, 0, V) == 0
    try:
        assert call() == 0, L.rslf_last_error()
    finally:
        assert L.rslf_sweep_end(ctx._h, 0, D, None) == 0
    torch.cuda.synchronize()
    want = sr.refine(field(1, U), np.full((V, U), 3, np.int32), DMIN, DMAX, D, S_HAT, oracle_params())[0]
    assert_same(disp.cpu().numpy(), want, "inside an open sweep")
    with pytest.raises(ValueError):
        rs.subgrid_refine(dev, DMIN, DMAX, D, S_HAT, idx[:3])
    with pytest.raises(ValueError):
        rs.MultiDevice([0]).depth1d_pile([field(1, U)[v, :, :, 0] for v in range(V)], DMIN, DMAX, D, subgrid=True)


# ---- the pile step ---------------------------------------------------------------------------------------------------

PILE = ("Ce", "mask", "Cd", "depth", "rbar", "idx", "score", "raw")
REF_OF = dict(Ce="Ce", mask="Ce_mask", Cd="Cd", rbar="rbar", idx="idx", score="score")


def pile_field(C_):
    """The planted line of disparity 0.37 (tests/subgrid_ref.py): every confident pixel moves off the grid.  Three channels:
    the same texture at three gains."""
    one = sr.planted_field(0.37)
    return one if C_ == 1 else np.concatenate([one, one * np.float32(0.8), one * np.float32(0.6)], axis=3).astype(np.float32)


def pile_reference(C_, median):
    key = ("pile", C_, median)
    if key not in _cache:
        _cache[key] = sr.pile_run(pile_field(C_), np.float32(-1), np.float32(1), 9, -1, oracle_params(median=median))
    return _cache[key]


def pile_planes(torch, U, C_):
    f32 = lambda *s: torch.full(s, FILL, dtype=torch.float32, device="cuda")
    return dict(Ce=f32(V, U), mask=torch.full((V, U), 7, dtype=torch.uint8, device="cuda"), Cd=f32(V, U), depth=f32(V, U),
                rbar=f32(V, U, C_), idx=torch.full((V, U), -5, dtype=torch.int32, device="cuda"), score=f32(V, U), raw=f32(V, U))


def run_pile(rs, name, dev, pl, params, *extra, skip=()):
    from remotesensingproject_amd import _lib
    L, p = _lib.lib(), params.to_c()
    dev.ctx.use_current_stream()
    args = [C.c_void_p(None if n in skip else pl[n].data_ptr()) for n in PILE]
    rc = getattr(L, name)(dev.ctx._h, dev._h, -1.0, 1.0, 9, -1, C.byref(p), *args, None, *extra)
    assert rc == 0, L.rslf_last_error()
    import torch
    torch.cuda.synchronize()
    return {n: pl[n].cpu().numpy() for n in PILE}


def assert_sub_planes(got, ref, label, raw=True):
    """subgrid = 1 against the reference: the refined and filtered plane, the refined raw plane, the six others the grid run's."""
    assert_same(got["depth"], ref["depth_sub"], label + ": depth")
    if raw:
        assert_same(got["raw"], ref["depth_raw_sub"], label + ": depth_raw")
    for n, r in REF_OF.items():
        assert_same(got[n], ref[r], "%s: %s" % (label, n))


@pytest.mark.parametrize("median", [5, 13])
@pytest.mark.parametrize("C_", [1, 3])
def test_pile_run_sub(rs, C_, median):
    """rslf_depth1d_pile_run_sub: with 0 all eight planes of rslf_depth1d_pile_run, with 1 the reference's refined and filtered
    planes and the six other planes unchanged; the same with the context's own arg-max and score planes (NULL passed).
    Median sizes 5 (the register sort) and 13 (the radix select) on non-grid floats."""
    import torch
    vol = pile_field(C_)
    U = vol.shape[2]
    dev = rs.Volume.from_dense(vol, 1.0, rs.default_context(0))
    params = rs.Depth1DParameters(par_median_filter_size=median)
    ref = pile_reference(C_, median)
    base = run_pile(rs, "rslf_depth1d_pile_run", dev, pile_planes(torch, U, C_), params)
    off = run_pile(rs, "rslf_depth1d_pile_run_sub", dev, pile_planes(torch, U, C_), params, 0)
    for n in PILE:
        assert_same(off[n], base[n], "subgrid = 0: %s" % n)
    assert_same(base["depth"], ref["depth"], "the grid run: depth")
    assert_same(base["raw"], ref["depth_raw"], "the grid run: depth_raw")
    on = run_pile(rs, "rslf_depth1d_pile_run_sub", dev, pile_planes(torch, U, C_), params, 1)
    assert_sub_planes(on, ref, "subgrid = 1, C = %d, median %d" % (C_, median))
    has = ref["idx"] >= 0
    assert has.sum() >= 400 and (bits(on["raw"][has]) != bits(base["raw"][has])).sum() >= 0.9 * has.sum()
    assert (bits(on["depth"]) != bits(base["depth"])).sum() >= 0.9 * (ref["Ce_mask"] != 0).sum()
    bare = run_pile(rs, "rslf_depth1d_pile_run_sub", dev, pile_planes(torch, U, C_), params, 1, skip=("idx", "score", "raw"))
    assert_same(bare["depth"], ref["depth_sub"], "the context's own planes: depth")
    assert (bare["idx"] == -5).all() and (bare["raw"] == FILL).all()


def test_host_form_with_padded_rows(rs):
    """rslf_depth1d_pile_run_host_sub on a volume uploaded from padded rows (windows of wider, poisoned parents, handed on where
    they lie by depth.host_rows): host planes, subgrid 1 and 0."""
    from remotesensingproject_amd import _lib
    from test_gpu_host_strides import assert_in_place, windows
    L = _lib.lib()
    vol = pile_field(1)
    U = vol.shape[2]
    views = windows([vol[v, :, :, 0] for v in range(V)], "right1")
    assert_in_place(rs, views)
    dev = rs.Volume.from_epis(views, 1.0, rs.default_context(0))
    ref = pile_reference(1, 5)
    p = rs.Depth1DParameters().to_c()
    for sub in (1, 0):
        h = dict(Ce=np.full((V, U), FILL, np.float32), mask=np.full((V, U), 7, np.uint8), Cd=np.full((V, U), FILL, np.float32),
                 depth=np.full((V, U), FILL, np.float32), rbar=np.full((V, U, 1), FILL, np.float32), idx=np.full((V, U), -5, np.int32),
                 score=np.full((V, U), FILL, np.float32), raw=np.full((V, U), FILL, np.float32))
        st = _lib.RslfStats()
        rc = L.rslf_depth1d_pile_run_host_sub(dev.ctx._h, dev._h, -1.0, 1.0, 9, -1, C.byref(p), *[C.c_void_p(h[n].ctypes.data) for n in PILE],
                                              C.byref(st), sub)
        assert rc == 0, L.rslf_last_error()
        assert st.pixels_scanned >= int((ref["idx"] >= 0).sum()) >= 400
        if sub:
            assert_sub_planes(h, ref, "host form, subgrid = 1")
        else:
            assert_same(h["depth"], ref["depth"], "host form, subgrid = 0: depth")
            assert_same(h["raw"], ref["depth_raw"], "host form, subgrid = 0: depth_raw")


def test_scan_forms_and_python_classes(rs):
    """rslf_depth1d_run_sub and rslf_depth_epi_scan_sub (no median: the refined raw plane), rslf_depth_epi_pile_sub through
    compute_1D_depth_epi_pile, and the classes' subgrid keyword, whose getters then show refined planes."""
    import torch
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    vol = pile_field(1)
    U = vol.shape[2]
    ref = pile_reference(1, 5)
    dev = rs.Volume.from_dense(vol, 1.0, rs.default_context(0))
    params = rs.Depth1DParameters()
    p = params.to_c()
    dev.ctx.use_current_stream()
    for sub, want in ((1, ref["depth_raw_sub"]), (0, ref["depth_raw"])):
        pl = pile_planes(torch, U, 1)
        args = [C.c_void_p(pl[n].data_ptr()) for n in PILE[:-1]]
        rc = L.rslf_depth1d_run_sub(dev.ctx._h, dev._h, -1.0, 1.0, 9, -1, C.byref(p), *args, None, sub)
        assert rc == 0, L.rslf_last_error()
        torch.cuda.synchronize()
        assert_same(pl["depth"].cpu().numpy(), want, "rslf_depth1d_run_sub, subgrid = %d" % sub)
        for n, r in REF_OF.items():
            assert_same(pl[n].cpu().numpy(), ref[r], "rslf_depth1d_run_sub, subgrid = %d: %s" % (sub, n))
    # the scan and the pile entry on planes the caller prepared: edge confidence first, zeros elsewhere; no idx / score planes
    for fn, want in ((rs.compute_1D_depth_epi, ref["depth_raw_sub"]), (rs.compute_1D_depth_epi_pile, ref["depth_sub"])):
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
        Ce, Cd, depth, rbar = z(V, U), z(V, U), z(V, U), z(V, U, 1)
        mask = rs.compute_1D_edge_confidence_pile(dev, S_HAT, Ce, params)
        fn(dev, -1.0, 1.0, 9, S_HAT, Ce, mask, Cd, depth, rbar, params, subgrid=True)
        torch.cuda.synchronize()
        assert_same(depth.cpu().numpy(), want, fn.__name__ + ", subgrid")
        assert_same(mask.cpu().numpy(), ref["Ce_mask"], fn.__name__ + ": mask")
        assert_same(rbar.cpu().numpy(), ref["rbar"], fn.__name__ + ": rbar")
    # the classes
    comp = rs.Depth1DComputer_pile(vol, -1.0, 1.0, 9, -1, 1.0, subgrid=True)
    comp.run()
    res = comp.results()
    assert_same(res["depth"], ref["depth_sub"], "Depth1DComputer_pile: depth")
    assert_same(res["depth_raw"], ref["depth_raw_sub"], "Depth1DComputer_pile: depth_raw")
    assert_same(res["depth_idx"], ref["idx"], "Depth1DComputer_pile: idx")
    assert comp.stats.pixels_scanned >= int((ref["idx"] >= 0).sum())
    plain = rs.Depth1DComputer_pile(vol, -1.0, 1.0, 9, -1, 1.0)
    plain.run()
    assert_same(plain.results()["depth"], ref["depth"], "Depth1DComputer_pile, default: depth")
    dm, dm0 = comp.get_disparity_map().cpu().numpy(), plain.get_disparity_map().cpu().numpy()
    assert dm.shape == (V, U, 3) and dm.dtype == np.uint8 and (dm != dm0).any()
    assert tuple(comp.get_coloured_epi(3).shape) == (S, U, 3)
    one = rs.Depth1DComputer(vol[3, :, :, 0], -1.0, 1.0, 9, -1, 1.0, subgrid=True)
    one.run()
    assert_same(one.results()["depth"], ref["depth_raw_sub"][3], "Depth1DComputer: depth")
    assert_same(one.results()["depth_idx"], ref["idx"][3], "Depth1DComputer: idx")
