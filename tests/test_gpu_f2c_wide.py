"""Fine-to-coarse against the oracle on wide, odd and tiny shapes.

Every K5 launch runs one thread per column or value in 256-wide blocks; the suite's other fine-to-coarse cases are at most
128 columns wide, so a second x block, the row index of k5_gauss_rows' 1-D grid, the carry of k5_nearest_valid between
64-column chunks and the grid-stride tail of rslf_device_max_f32 would go wrong unseen.  Each primitive is compared
directly (the entry points tests/test_gpu_f2c.py uses), then the whole pyramid at skysat_lr's and mansion_lr's widths --
levels (44, 960) -> (22, 480) -> (11, 240), and (46, 1146) -> (23, 573) -> (12, 286) where the last width rounds half to
even -- and with max_pyr_depth and accept_all_last_scale=False, through the Python level loop (FineToCoarse) and the
native one (both of its C-ABI entries).  Everything bit-exact; C_d within 1e-5."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_sweep2d import _check

pytestmark = pytest.mark.gpu

MAX_STRIDE = 2048 * 256   # rslf_device_max_f32: values one pass of its grid covers


@pytest.fixture
def lib():
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd import depth as rs
    ctx = rs.default_context()
    ctx.use_current_stream()
    return ctx, _lib.lib()


# ---- the pyramid's downsampling ------------------------------------------------------------------------------------

DOWN_SHAPES = [(2, 2, 2, 1), (3, 1, 5, 3), (7, 2, 4, 1), (5, 3, 7, 3),    # BORDER_REFLECT folds more than once
               (6, 3, 257, 1), (4, 2, 1146, 3), (5, 2, 2049, 1),           # more than one x block per row
               (1311, 51, 3, 1)]                                           # V * S = 66 861 rows of the 1-D grid


@pytest.mark.parametrize("is_u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("V,S,U,C_", DOWN_SHAPES)
def test_downsample_wide_odd_and_tiny(oracle_mod, V, S, U, C_, is_u8):
    import torch
    from remotesensingproject_amd import depth as rs
    rng = np.random.default_rng(V * 1000 + U * 10 + C_)
    if is_u8:
        raw = rng.integers(0, 256, size=(V, S, U, C_)).astype(np.float32)
        raw[:, :, ::5] = 255.0   # saturated columns and odd sums: the area step's ties
        want = oracle_mod.downsample_epis_u8(raw)
    else:
        raw = rng.uniform(0, 250, size=(V, S, U, C_)).astype(np.float32)
        want = oracle_mod.downsample_epis(raw)
    got = rs.downsample_EPIs(torch.from_numpy(raw).cuda(), is_u8=is_u8).cpu().numpy()
    assert got.shape == want.shape == (int(np.rint(V / 2)), S, int(np.rint(U / 2)), C_)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (bad.size, np.unravel_index(bad[0], want.shape))


# ---- bound tightening ----------------------------------------------------------------------------------------------

def _row_patterns(U, rng):
    """Masks of one finer-level row each: the cases of k5_nearest_valid's ballots and carries."""
    pats = []
    for cols in ([], [0], [U - 1], [63], [64], [127], [128], [63, 64, 127, 128], [0, U - 1]):
        m = np.zeros(U, np.uint8)
        m[[c for c in cols if c < U]] = 255
        pats.append(m)
    edges = np.zeros(U, np.uint8)
    edges[(np.arange(U) % 64 == 0) | (np.arange(U) % 64 == 63)] = 255   # every chunk's first and last column
    pats.append(edges)
    pats.append(np.full(U, 255, np.uint8))                                # dense
    pats.append((rng.uniform(size=U) < 0.02).astype(np.uint8) * 255)      # 2 % random
    return pats


@pytest.mark.parametrize("U_up", [2, 3, 63, 64, 65, 129, 1146])
def test_tighten_bounds_row_patterns(oracle_mod, lib, U_up):
    import torch
    ctx, L = lib
    rng = np.random.default_rng(U_up)
    pats = _row_patterns(U_up, rng)
    S, V_up = 2, 2 * len(pats) + 1                                       # odd: the last coarser row has one finer row
    mask = np.stack([np.stack([pats[(v + 5 * s) % len(pats)] for v in range(V_up)]) for s in range(S)])
    dep = rng.uniform(-2, 2, size=(S, V_up, U_up)).astype(np.float32)
    V_dn, U_dn = int(np.rint(V_up / 2)), int(np.rint(U_up / 2))
    lo = np.full((S, V_dn, U_dn), -3, np.float32)
    hi = np.full((S, V_dn, U_dn), 3, np.float32)
    wlo, whi = oracle_mod.f2c_tighten_bounds(dep, mask, lo, hi)
    tlo, thi = torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()
    tdep, tmsk = torch.from_numpy(dep).cuda(), torch.from_numpy(mask).cuda()
    assert L.rslf_f2c_tighten_bounds(ctx._h, C.c_void_p(tdep.data_ptr()), C.c_void_p(tmsk.data_ptr()), S, V_up, U_up,
                                     C.c_void_p(tlo.data_ptr()), C.c_void_p(thi.data_ptr()), V_dn, U_dn) == 0
    assert np.array_equal(tlo.cpu().numpy(), wlo) and np.array_equal(thi.cpu().numpy(), whi)
    if U_up >= 63:   # the patterns leave some ranges alone and tighten others
        assert (wlo != lo).any() and (wlo == lo).any()


# ---- fusion --------------------------------------------------------------------------------------------------------

FUSE_CHAINS = {
    "skysat": ((540, 960), (270, 480), (135, 240)),
    "mansion": ((720, 1146), (360, 573), (180, 286), (90, 143)),
    "tiny": ((11, 11), (6, 6), (3, 3)),
}


@pytest.mark.parametrize("chain", list(FUSE_CHAINS))
def test_fuse_level_chains(oracle_mod, lib, chain):
    import torch
    ctx, L = lib
    dims = FUSE_CHAINS[chain]
    S, P = 2, len(dims)
    rng = np.random.default_rng(P * 100 + dims[0][1])
    d = [rng.uniform(-2, 2, size=(S,) + x).astype(np.float32) for x in dims]
    m = [(rng.uniform(size=(S,) + x) < 0.6).astype(np.uint8) * 255 for x in dims]
    m[0][:, :, -40:] = 0                                    # a band the finer levels leave to the coarser ones
    td = [torch.from_numpy(x).cuda() for x in d]
    tm = [torch.from_numpy(x).cuda() for x in m]
    dp = (C.c_void_p * P)(*[t.data_ptr() for t in td])
    mp = (C.c_void_p * P)(*[t.data_ptr() for t in tm])
    Vp = (C.c_int * P)(*[x[0] for x in dims])
    Up = (C.c_int * P)(*[x[1] for x in dims])
    om = torch.empty((S,) + dims[0], dtype=torch.float32, device="cuda")
    ov = torch.empty((S,) + dims[0], dtype=torch.uint8, device="cuda")
    assert L.rslf_f2c_fuse(ctx._h, dp, mp, Vp, Up, P, S, C.c_void_p(om.data_ptr()), C.c_void_p(ov.data_ptr())) == 0
    gm, gv = om.cpu().numpy(), ov.cpu().numpy()
    for s in range(S):
        wm, wv = oracle_mod.f2c_fuse([x[s] for x in d], [x[s] for x in m])
        bad = np.flatnonzero(gm[s].reshape(-1) != wm.reshape(-1))
        assert bad.size == 0, (chain, s, bad.size, np.unravel_index(bad[0], wm.shape))
        assert np.array_equal(gv[s], wv), (chain, s)


# ---- the per-level maximum -----------------------------------------------------------------------------------------

MAX_CASES = [(n, where, neg) for n in (1, 255, 257, MAX_STRIDE, MAX_STRIDE + 1, 3_000_000)
             for where in ("first", "last", "tail") for neg in (False, True)]


@pytest.mark.parametrize("n,where,neg", MAX_CASES)
def test_device_max(lib, n, where, neg):
    """rslf_device_max_f32 against np.max: the maximum first, last, or in the grid-stride loop's tail (past the first
    2048 x 256 values; below that, the middle of the last block)."""
    import torch
    ctx, L = lib
    rng = np.random.default_rng(n + (7 if neg else 0))
    x = (rng.uniform(-100.0, -1.0, size=n) if neg else rng.uniform(-5.0, 5.0, size=n)).astype(np.float32)
    peak = np.float32(-0.5) if neg else np.float32(6.0)
    i = {"first": 0, "last": n - 1,
         "tail": MAX_STRIDE + (n - MAX_STRIDE) * 2 // 3 if n > MAX_STRIDE else max(0, n - 1 - (n % 256) // 2)}[where]
    x[i] = peak
    t = torch.from_numpy(x).cuda()
    mx = C.c_float()
    assert L.rslf_device_max_f32(ctx._h, C.c_void_p(t.data_ptr()), n, C.byref(mx)) == 0
    assert np.float32(mx.value) == x.max() == peak


# ---- the pyramid end to end ----------------------------------------------------------------------------------------

# name: channels, uchar, scanlines, views, row length, hypotheses, dmin, dmax, the pyramid's (V, U)
PYRAMIDS = {
    "skysat": (1, False, 44, 33, 960, 48, -1.0, 4.0, [(44, 960), (22, 480), (11, 240)]),
    "mansion": (3, True, 46, 17, 1146, 32, 0.0, 4.0, [(46, 1146), (23, 573), (12, 286)]),
}
# (max_pyr_depth, accept_all_last_scale) beside the defaults (-1, True)
OPTIONS = {"default": (-1, True), "depth1": (1, True), "depth2": (2, True), "strict_last": (-1, False)}


def pyramid_input(name):
    """A light field whose texture alternates, in 96-column stretches of each scanline, between random values and a
    triangle wave: the wave is too smooth for the finest level's edge test (slope k per column: 60 k^2 per channel against
    0.02) and steep enough once a level has halved it, so the coarser levels decide a real share of the fused map."""
    from remotesensingproject_amd.synth import make_lightfield
    C_, u8, V, S, U, D, dmin, dmax, _ = PYRAMIDS[name]
    vol, deltas = make_lightfield(U, V, S, C_, seed=U, dmin=dmin, dmax=dmax, band=4)
    k = 0.012 if C_ == 1 else 0.008
    # texture coordinate of every sample, along the EPI lines make_lightfield draws: x = u - (s_hat - s) * delta
    x = (np.arange(U)[None, None, :] - (S // 2 - np.arange(S))[None, :, None] * deltas[:, None, None]).astype(np.float64)
    wave = 0.3 + k * np.abs(np.mod(x, 100.0) - 50.0)
    smooth = np.mod(np.floor(x / 96.0), 2) == 1
    vol = np.where(smooth[..., None], wave[..., None], vol)
    rng = np.random.default_rng(U)
    vol = (vol + rng.normal(0.0, 0.004, size=vol.shape)).clip(0.0, 1.0).astype(np.float32)
    if u8:
        return np.round(vol * np.float32(255.0)).astype(np.uint8)
    return (vol * np.float32(200.0) + np.float32(3.0)).astype(np.float32)


@pytest.fixture(scope="module")
def pyramids(oracle_mod):
    """The oracle's FineToCoarse of each (volume, options), computed once."""
    cache = {}

    def get(name, opt):
        if (name, opt) not in cache:
            C_, u8, V, S, U, D, dmin, dmax, _ = PYRAMIDS[name]
            raw = pyramid_input(name)
            depth, accept = OPTIONS[opt]
            cache[(name, opt)] = (raw, oracle_mod.fine_to_coarse_run(raw.astype(np.float32), dmin, dmax, D, max_pyr_depth=depth,
                                                                     accept_all_last_scale=accept, is_u8=u8))
        return cache[(name, opt)]
    return get


RUNS_F2C = [("skysat", o) for o in OPTIONS] + [("mansion", "default")]


def check_coarse_levels_decide(pyramids, oracle_mod, name, opt):
    """What the case is here for, read from the oracle: the fused output depends on every level, not on the finest alone.
    A fault of a coarser level -- its size, bounds, slope factor or validity -- must show in many fused pixels."""
    raw, ref = pyramids(name, opt)
    S = raw.shape[1]
    invalid0 = float((ref["levels"][0].edge_confidence <= np.float32(0.02)).mean())
    assert invalid0 > 0.2, (name, "share of the finest level's pixels left to coarser levels", invalid0)
    if len(ref["dims"]) > 1:   # fusing the finest level alone gives another map
        alone = np.stack([oracle_mod.f2c_fuse([ref["levels"][0].depth[s]], [ref["valids"][0][s]])[0] for s in range(S)])
        n = int((alone != ref["fused_map"]).sum())
        assert n >= 10000, (name, opt, "fused pixels the coarser levels decide", n)
    if opt != "default":       # and each option gives another output than the default
        _, dflt = pyramids(name, "default")
        n = int(((ref["fused_map"] != dflt["fused_map"]) | (ref["fused_valid"] != dflt["fused_valid"])).sum())
        assert n >= 1000, (name, opt, "fused pixels that differ from the default pyramid's", n)


@pytest.mark.parametrize("name,opt", RUNS_F2C)
def test_fine_to_coarse_wide(pyramids, oracle_mod, name, opt):
    from remotesensingproject_amd import depth as rs
    C_, u8, V, S, U, D, dmin, dmax, dims = PYRAMIDS[name]
    depth, accept = OPTIONS[opt]
    raw, ref = pyramids(name, opt)
    check_coarse_levels_decide(pyramids, oracle_mod, name, opt)
    assert ref["dims"] == (dims[:depth] if depth > 0 else dims)
    if name == "skysat" and opt == "default":
        assert V * S * U * C_ > MAX_STRIDE   # the finest level's maximum runs the grid-stride loop
    f = rs.FineToCoarse(raw, dmin, dmax, D, max_pyr_depth=depth, accept_all_last_scale=accept)
    assert [(c.m_epis.V, c.m_epis.U) for c in f.m_computers] == ref["dims"]
    f.run()
    for p, (comp, lv) in enumerate(zip(f.m_computers, ref["levels"])):
        assert comp.m_parameters.par_slope_factor == float(ref["params"][p].slope_factor), p
        _check(comp.results(), lv, "%s %s level %d" % (name, opt, p))
        assert np.array_equal(comp.get_valid_depths_mask_s_v_u().cpu().numpy(), ref["valids"][p]), p
    if not accept:   # the last level's validity is its edge test, not "everything"
        assert not ref["valids"][-1].all()
    out_map, out_valid = f.get_results()
    assert np.array_equal(out_map.cpu().numpy(), ref["fused_map"])
    assert np.array_equal(out_valid.cpu().numpy(), ref["fused_valid"])


@pytest.mark.parametrize("name,opt", RUNS_F2C)
def test_native_fine_to_coarse_wide(pyramids, oracle_mod, name, opt):
    """The native level loop behind the C ABI, through both of its entries on one device: the multi-device one
    (rslf_multi_fine_to_coarse_run_host) and the one-context one (rslf_fine_to_coarse_run_host).  Only the fused output
    comes back, so the scene must make every level count in it (check_coarse_levels_decide)."""
    from remotesensingproject_amd import depth as rs
    from tests.util import native_fine_to_coarse
    C_, u8, V, S, U, D, dmin, dmax, dims = PYRAMIDS[name]
    depth, accept = OPTIONS[opt]
    raw, ref = pyramids(name, opt)
    check_coarse_levels_decide(pyramids, oracle_mod, name, opt)
    epis = [np.ascontiguousarray(raw[v, :, :, 0] if C_ == 1 else raw[v]) for v in range(V)]
    md = rs.MultiDevice([0])
    try:
        multi = md.fine_to_coarse(epis, dmin, dmax, D, max_pyr_depth=depth, accept_all_last_scale=accept)
    finally:
        md.close()
    one = native_fine_to_coarse(epis, dmin, dmax, D, max_pyr_depth=depth, accept_all_last_scale=accept)[:3]
    for entry, (out_map, out_valid, n_levels) in (("multi", multi), ("one context", one)):
        assert n_levels == len(ref["dims"]), entry
        assert np.array_equal(out_map, ref["fused_map"]), entry
        assert np.array_equal(out_valid, ref["fused_valid"]), entry
