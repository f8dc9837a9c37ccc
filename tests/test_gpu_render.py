"""The renderers (K6: rslf_render_fit / rslf_render_planes / rslf_render_epi_lines and the getters of depth.py built on
them) against tests/render_ref.py, the numpy restatement of the reference's getters.

Every picture is compared byte for byte and every fitted (min, max) with == on the doubles (so -0.0 equals 0.0): each
operation is an IEEE float operation in a fixed order, or an integer count, so there is no tolerance to choose.
The one place where order could matter is the MEANSTD fit's double sums; its planes are therefore drawn as multiples of
2^-8 with magnitude below 8 and at most 2^20 pixels: every partial sum (< 2^23, 8 fractional bits) and every partial sum
of squares (< 2^26, 16 fractional bits) then fits a double's 53 bits exactly in any order of addition, and byte
equality is a fair demand of any correct summation.

No test provokes a fault and none reads the reference tree."""
import numpy as np
import pytest
import torch

import render_ref as rr

pytestmark = pytest.mark.gpu

GREY = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
MODES = (rr.MINMAX, rr.QUANTILE, rr.MEANSTD)


def random_table(seed=7):
    return np.random.default_rng(seed).integers(0, 256, size=(256, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def rs():
    from remotesensingproject_amd import depth
    return depth


@pytest.fixture(scope="module")
def ctx(rs):
    return rs.default_context(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def embedded(a, pad, fill):
    """`a` [rows, cols] as a slice of a device buffer whose rows are `pad` elements longer (row_stride > cols)."""
    buf = np.full((a.shape[0], a.shape[1] + pad), fill, a.dtype)
    buf[:, :a.shape[1]] = a
    return dev(buf)[:, :a.shape[1]]


def dyadic(rng, shape):
    """Multiples of 2^-8 with magnitude below 8, a large share of exact zeros and few distinct values among the rest."""
    x = rng.integers(-2047, 2048, size=shape).astype(np.float32) / np.float32(256.0)
    x[rng.random(shape) < 0.3] = 0.0
    few = rng.integers(-16, 17, size=shape).astype(np.float32) / np.float32(8.0)
    return np.where(rng.random(shape) < 0.5, few, x).astype(np.float32)


def check_fit(rs, ctx, plane, valid, modes=MODES):
    for mode in modes:
        want = rr.fit(plane, mode, valid)
        for pad in (0, 3, 4):   # contiguous; a stride that breaks the 16-byte rows; one that keeps them
            p = embedded(plane, pad, np.float32(1.0e6)) if pad else dev(plane)
            v = None if valid is None else (embedded(valid, pad, np.uint8(255)) if pad else dev(valid))
            got = rs.render_fit(ctx, p, v, mode)
            print("fit mode %d shape %s pad %d valid %s: got %r want %r" % (mode, plane.shape, pad, valid is not None, got, want))
            assert got == want, (mode, plane.shape, pad, got, want)
            assert rs.render_fit(ctx, p, v, mode) == got   # determinism


@pytest.fixture(scope="module")
def run2d(rs):
    """A Depth2DComputer run on a synthetic field whose hypotheses are multiples of 1/8 (dmin -1, dmax 2.875, 32 of them):
    its disparity planes carry few distinct values and many exact zeros, and qualify for the exact MEANSTD comparison."""
    from remotesensingproject_amd.synth import make_lightfield
    vol, _ = make_lightfield(96, 12, 9, 1, seed=3, dmin=-1.0, dmax=2.0, band=3)
    comp = rs.Depth2DComputer(vol, -1.0, 2.875, 32, epi_scale_factor=1.0)
    comp.run()
    return comp


# ---- fit ------------------------------------------------------------------------------------------------------------------

def test_fit_on_result_planes(rs, ctx, run2d):
    depth = host(run2d.m_best_depth_s_v_u)
    mask = host(run2d.m_edge_confidence_mask_s_v_u)
    assert np.array_equal(depth * 256, np.rint(depth * 256)) and np.abs(depth).max() < 8   # dyadic: MEANSTD is exact
    print("result planes: %.3f exact zeros, %d distinct values" % ((depth == 0).mean(), np.unique(depth).size))
    S, V, U = depth.shape
    check_fit(rs, ctx, depth[S // 2], None)
    check_fit(rs, ctx, depth[S // 2], mask[S // 2])
    check_fit(rs, ctx, depth.reshape(S * V, U), mask.reshape(S * V, U))
    # row v of the [S][V][U] stack as an S x U plane, in place through its row stride
    for v in (0, V // 2):
        for valid in (None, run2d.m_edge_confidence_mask_s_v_u[:, v, :]):
            for mode in MODES:
                got = rs.render_fit(ctx, run2d.m_best_depth_s_v_u[:, v, :], valid, mode)
                want = rr.fit(depth[:, v, :], mode, None if valid is None else mask[:, v, :])
                assert got == want, (v, mode, got, want)


def test_fit_on_random_normal_planes(rs, ctx):
    rng = np.random.default_rng(11)
    for shape in ((37, 53), (64, 256)):
        plane = rng.normal(-0.5, 2.0, size=shape).astype(np.float32)
        valid = (rng.random(shape) < 0.7).astype(np.uint8) * 255
        check_fit(rs, ctx, plane, None, (rr.MINMAX, rr.QUANTILE))   # MEANSTD: see the module docstring
        check_fit(rs, ctx, plane, valid, (rr.MINMAX, rr.QUANTILE))


@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (7, 7), (5, 10), (3, 17), (64, 4097)])
def test_fit_sizes(rs, ctx, shape):
    rng = np.random.default_rng(shape[0] * 10007 + shape[1])
    plane = dyadic(rng, shape)
    valid = (rng.random(shape) < 0.6).astype(np.uint8) * 255
    assert plane.size <= 1 << 20
    check_fit(rs, ctx, plane, None)
    check_fit(rs, ctx, plane, valid)


def test_fit_negative_zero_and_one_value(rs, ctx):
    check_fit(rs, ctx, np.full((9, 12), -2.625, np.float32), None)
    check_fit(rs, ctx, np.full((9, 12), -2.625, np.float32), np.zeros((9, 12), np.uint8))   # every pixel counts as 0
    plane = np.zeros((8, 8), np.float32)
    plane[::2] = -0.0
    plane[0, 0], plane[7, 7] = -1.0, 1.0
    check_fit(rs, ctx, plane, None)


def test_fit_with_a_nan_returns(rs, ctx):
    """cv::sort and minMaxLoc are undefined on a NaN; here the calls come back, with unspecified numbers."""
    plane = np.ones((16, 16), np.float32)
    plane[3, 5] = np.nan
    for mode in MODES:
        got = rs.render_fit(ctx, dev(plane), None, mode)
        assert len(got) == 2


# ---- plane render ---------------------------------------------------------------------------------------------------------

def half_planes(rng, n, rows, cols):
    """Integers (levels land on exact halves for every odd one at scale 0.5) with some non-integers, zeros and values
    beyond both ends among them."""
    x = rng.integers(-140, 460, size=(n, rows, cols)).astype(np.float32)
    frac = rng.random((n, rows, cols)) < 0.2
    x[frac] += rng.random(int(frac.sum())).astype(np.float32)
    x[rng.random((n, rows, cols)) < 0.1] = 0.0
    return x


@pytest.mark.parametrize("cols", [1, 3, 4, 5, 1919, 1920])
def test_render_planes_formulas_and_masks(rs, ctx, cols):
    rng = np.random.default_rng(100 + cols)
    n, rows = 3, 5
    planes = half_planes(rng, n, rows, cols)
    valid = (rng.random((n, rows, cols)) < 0.6).astype(np.uint8) * 255
    vmin, vmax = -100.0, 410.0   # scale exactly 0.5; level(0) = 50, so the two mask modes differ
    d_planes, d_valid = dev(planes), dev(valid)
    for lut in (GREY, random_table()):
        for formula in (rr.SHIFT, rr.AFFINE):
            for v, mode in ((None, rr.BLACK), (valid, rr.BLACK), (valid, rr.ZERO_VALUE)):
                got = host(rs.render_planes(ctx, d_planes, vmin, vmax, formula, lut, None if v is None else d_valid, mode))
                want = np.stack([rr.render(planes[k], vmin, vmax, formula, lut, None if v is None else v[k], mode) for k in range(n)])
                assert got.shape == (n, rows, cols, 3) and got.dtype == np.uint8
                assert np.array_equal(got, want), (cols, formula, mode, v is None, int((got != want).sum()))
    lv = rr.levels(planes, vmin, vmax, rr.AFFINE)
    if cols >= 1919:
        assert (lv == 50).any() and (lv == 0).any() and (lv == 255).any()
    black = host(rs.render_planes(ctx, d_planes, vmin, vmax, rr.AFFINE, GREY, d_valid, rr.BLACK))
    zero = host(rs.render_planes(ctx, d_planes, vmin, vmax, rr.AFFINE, GREY, d_valid, rr.ZERO_VALUE))
    assert (black[valid == 0] == 0).all() and (zero[valid == 0] == 50).all()
    # a general range and a constant plane (max == min renders lut[0])
    lo, hi = rr.fit(planes[0], rr.MINMAX)
    for formula in (rr.SHIFT, rr.AFFINE):
        got = host(rs.render_planes(ctx, d_planes, lo, hi, formula, random_table(3)))
        want = np.stack([rr.render(planes[k], lo, hi, formula, random_table(3)) for k in range(n)])
        assert np.array_equal(got, want)
        flat = host(rs.render_planes(ctx, dev(np.full((1, rows, cols), 3.5, np.float32)), 3.5, 3.5, formula, random_table(3)))
        assert (flat == random_table(3)[0]).all()
    # strided planes: rows and planes cut out of a larger stack
    big = half_planes(rng, n, rows + 2, cols + 4)
    got = host(rs.render_planes(ctx, dev(big)[:, 1:rows + 1, :cols], vmin, vmax, rr.SHIFT, GREY))
    want = np.stack([rr.render(big[k, 1:rows + 1, :cols], vmin, vmax, rr.SHIFT, GREY) for k in range(n)])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("cols", [1, 3, 4, 5, 1919, 1920])
def test_render_planes_shadow_cut(rs, ctx, channels, cols):
    rng = np.random.default_rng(200 + cols + channels)
    V, S = 5, 4
    seed = np.array([0.05] if channels == 1 else [0.03, 0.04, 0.0], np.float32)
    n0 = rr.norms(seed[None, :])[0]
    rad = (rng.random((V, S, cols, channels)) * (0.1 if channels == 1 else 0.06)).astype(np.float32)   # norms on both sides of n0
    rad[rng.random((V, S, cols)) < 0.3] = seed                                                     # ... and exactly on it
    vol = rs.Volume.from_dense(rad, 1.0, ctx)   # factor 1: the slab holds these values
    planes = half_planes(rng, S, V, cols)
    valid = (rng.random((S, V, cols)) < 0.7).astype(np.uint8) * 255
    d_planes, d_valid = dev(planes), dev(valid)
    lut = random_table(5)
    levels = (n0, np.nextafter(n0, np.float32(np.inf)), np.nextafter(n0, np.float32(-np.inf)))   # within one ulp on each side
    cut = set()
    for level in levels:
        below = rr.norms(rad) < level
        cut.add(int(below.sum()))
        # VIEW: planes 1 .. 2 are views 1 .. 2, rows are scanlines
        got = host(rs.render_planes(ctx, d_planes[1:3], -100.0, 410.0, rr.AFFINE, lut, d_valid[1:3], rr.BLACK, vol, rs.SLICE_VIEW, 1, float(level)))
        want = np.stack([rr.render(planes[s], -100.0, 410.0, rr.AFFINE, lut, valid[s], rr.BLACK, rad[:, s], level) for s in (1, 2)])
        assert np.array_equal(got, want), (channels, cols, float(level))
        # EPI: the one plane is scanline 3, its rows are views
        epi, epi_valid = np.ascontiguousarray(planes[:, 3, :]), np.ascontiguousarray(valid[:, 3, :])
        got = host(rs.render_planes(ctx, d_planes[:, 3, :].unsqueeze(0), -100.0, 410.0, rr.SHIFT, lut, d_valid[:, 3, :].unsqueeze(0),
                                    rr.ZERO_VALUE, vol, rs.SLICE_EPI, 3, float(level)))[0]
        want = rr.render(epi, -100.0, 410.0, rr.SHIFT, lut, epi_valid, rr.ZERO_VALUE, rad[3], level)
        assert np.array_equal(got, want), (channels, cols, float(level))
    assert len(cut) >= 2 and 0 < min(cut) and max(cut) < rad[..., 0].size   # the levels do straddle the radiances
    # without the volume nothing is cut
    got = host(rs.render_planes(ctx, d_planes, -100.0, 410.0, rr.AFFINE, lut))
    assert np.array_equal(got, np.stack([rr.render(planes[s], -100.0, 410.0, rr.AFFINE, lut) for s in range(S)]))
    with pytest.raises(Exception):   # the planes must lie in the volume
        rs.render_planes(ctx, d_planes, 0.0, 1.0, rr.AFFINE, lut, None, rr.BLACK, vol, rs.SLICE_VIEW, 1, 0.1)


def test_render_planes_is_deterministic(rs, ctx):
    rng = np.random.default_rng(9)
    planes = dev(half_planes(rng, 4, 33, 260))
    a = host(rs.render_planes(ctx, planes, -100.0, 410.0, rr.AFFINE, random_table()))
    b = host(rs.render_planes(ctx, planes, -100.0, 410.0, rr.AFFINE, random_table()))
    assert np.array_equal(a, b)


# ---- EPI lines ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("U", [1, 63, 64, 65, 1920])
def test_epi_lines_on_hand_made_rows(rs, ctx, U):
    rng = np.random.default_rng(300 + U)
    V, S = 4, 5
    few = np.array([-2.0, -1.0, -0.5, -0.0, 0.0, 0.25, 0.5, 1.0, 1.5, 3.0], np.float32)   # many equal depths, both slopes, halves
    depth = few[rng.integers(0, few.size, size=(V, U))]
    depth[1] = np.abs(depth[1])            # a scanline of positive slopes only
    depth[2] = 1.0                         # a scanline of one depth: every target is a tie (and max == min)
    mask = (rng.random((V, U)) < 0.5).astype(np.uint8) * 255
    mask[3] = 255
    d_depth, d_mask = dev(depth), dev(mask)
    lut = random_table(8)
    for s_hat in (0, S // 2, S - 1):
        want = np.stack([rr.epi_lines(depth[v], mask[v], S, s_hat, lut) for v in range(V)])
        together = host(rs.render_epi_lines(ctx, d_depth, d_mask, S, s_hat, 0, V, lut))
        assert together.shape == (V, S, U, 3)
        assert np.array_equal(together, want), (U, s_hat, int((together != want).sum()))
        for v in range(V):   # several scanlines in one call equal the same scanlines one by one
            one = host(rs.render_epi_lines(ctx, d_depth, d_mask, S, s_hat, v, 1, lut))
            assert np.array_equal(one[0], together[v]), (U, s_hat, v)
        again = host(rs.render_epi_lines(ctx, d_depth, d_mask, S, s_hat, 0, V, lut))
        assert np.array_equal(again, together)
    # a NaN depth paints nothing, and the call returns
    depth[0, 0] = np.nan
    out = host(rs.render_epi_lines(ctx, dev(depth), d_mask, S, S // 2, 0, 1, lut))
    assert out.shape == (1, S, U, 3)


def test_epi_lines_widest_row(rs, ctx):
    """The z-buffer is one 64-bit key per column in LDS: rows up to 8000 columns fit, wider ones are refused, not truncated."""
    rng = np.random.default_rng(77)
    U, S = 8000, 3
    depth = rng.integers(-24, 25, size=(1, U)).astype(np.float32) / np.float32(8.0)
    mask = (rng.random((1, U)) < 0.5).astype(np.uint8) * 255
    lut = random_table(10)
    got = host(rs.render_epi_lines(ctx, dev(depth), dev(mask), S, 1, 0, 1, lut))
    assert np.array_equal(got[0], rr.epi_lines(depth[0], mask[0], S, 1, lut))
    with pytest.raises(Exception, match="z-buffer"):
        rs.render_epi_lines(ctx, dev(np.zeros((1, U + 1), np.float32)), dev(np.zeros((1, U + 1), np.uint8)), S, 1, 0, 1, lut)


# ---- getters end to end -----------------------------------------------------------------------------------------------------

def field(U, V, S, C, seed, dtype=np.float32, dark=True):
    """A synthetic light field as a list of V EPIs; its first columns are darkened into shadow (norm below the level)."""
    from remotesensingproject_amd.synth import make_lightfield
    vol, _ = make_lightfield(U, V, S, C, seed=seed, dmin=-1.0, dmax=2.0, band=4)
    if dark:
        vol[:, :, :U // 8] *= np.float32(0.04)
    if dtype == np.uint8:
        vol = np.rint(vol * 255).astype(np.uint8)
    elif dtype == np.uint16:
        vol = np.rint(vol * 65535).astype(np.uint16)
    return [vol[v] if C > 1 else vol[v, ..., 0] for v in range(V)]


@pytest.mark.parametrize("channels", [1, 3])
def test_pile_getters(rs, channels):
    epis = field(96, 6, 9, channels, seed=21)
    comp = rs.Depth1DComputer_pile(epis, -1.0, 2.875, 32)
    comp.run()
    depth, mask = host(comp.m_best_depth_v_u), host(comp.m_edge_confidence_mask_v_u)
    assert 0 < (mask != 0).sum() < mask.size
    lut = random_table(1)
    assert np.array_equal(host(comp.get_disparity_map(lut)), rr.disparity_map(depth, mask, lut))
    assert np.array_equal(host(comp.get_coloured_epi(-1, lut)), rr.pile_coloured_epi(depth, mask, 9, comp.get_s_hat(), lut))
    assert np.array_equal(host(comp.get_coloured_epi(4, lut)), rr.pile_coloured_epi(depth, mask, 9, comp.get_s_hat(), lut, 4))
    several = host(comp.get_coloured_epi(range(1, 5), lut))
    assert several.shape == (4, 9, 96, 3)
    for i, v in enumerate(range(1, 5)):
        assert np.array_equal(several[i], rr.pile_coloured_epi(depth, mask, 9, comp.get_s_hat(), lut, v))
    assert comp.get_coloured_epi(2).shape == (9, 96, 3)   # the default table
    with pytest.raises(ValueError):
        comp.get_coloured_epi(6, lut)


@pytest.mark.parametrize("channels", [1, 3])
def test_single_epi_getter(rs, channels):
    epi = field(96, 3, 9, channels, seed=22)[1]
    comp = rs.Depth1DComputer(epi, -1.0, 2.875, 32)
    comp.run()
    depth, mask = host(comp.m_best_depth_u)[0], host(comp.m_edge_confidence_mask_u)[0]
    assert (mask != 0).any()
    lut = random_table(2)
    assert np.array_equal(host(comp.get_coloured_epi(lut)), rr.epi_lines(depth, mask, 9, comp.m_s_hat, lut, lowest_column=1))


@pytest.mark.parametrize("channels", [1, 3])
def test_depth2d_getters(rs, channels):
    epis = field(96, 12, 9, channels, seed=23)
    comp = rs.Depth2DComputer(epis, -1.0, 2.875, 32)
    comp.run()
    depth, mask = host(comp.m_best_depth_s_v_u), host(comp.m_edge_confidence_mask_s_v_u)
    lut = random_table(3)
    for a_s in (-1, 0, 8):
        s = 4 if a_s < 0 else a_s
        assert np.array_equal(host(comp.get_disparity_map(a_s, lut)), rr.disparity_map(depth[s], mask[s], lut)), a_s
    for a_v in (-1, 0, 11):
        assert np.array_equal(host(comp.get_coloured_epi(a_v, lut)), rr.depth2d_coloured_epi(depth, mask, lut, a_v)), a_v
    with pytest.raises(ValueError):
        comp.get_disparity_map(9, lut)
    with pytest.raises(ValueError):
        comp.get_coloured_epi(12, lut)


def test_depth2d_getters_under_the_disparity_confidence_switch(rs):
    """With par_use_disp_confidence_score (the reference's _USE_DISP_CONFIDENCE_SCORE build, dc.hpp:832-834, :875-878) the
    getters paint under C_d > (float)par_disp_score_threshold instead of the edge mask."""
    par = rs.Depth1DParameters(par_use_disp_confidence_score=True)
    comp = rs.Depth2DComputer(field(96, 12, 9, 1, seed=27), -1.0, 2.875, 32, parameters=par)
    comp.run()
    depth, conf = host(comp.m_best_depth_s_v_u), host(comp.m_disp_confidence_s_v_u)
    mask = (conf > np.float32(par.par_disp_score_threshold)).astype(np.uint8) * 255
    assert 0 < (mask != 0).sum() < mask.size
    lut = random_table(9)
    assert np.array_equal(host(comp.get_disparity_map(-1, lut)), rr.disparity_map(depth[4], mask[4], lut))
    assert np.array_equal(host(comp.get_coloured_epi(-1, lut)), rr.depth2d_coloured_epi(depth, mask, lut))


def f2c_radiances(rs, epis, ftc):
    """The normalised EPIs [V_p, S, U_p, C] of every level, as the levels' volumes hold them: the raw pyramid
    (rs.f2c_pyramid, the constructor's own) times float(1 / scale), the upload's one multiplication."""
    ctx = ftc.m_computers[0].m_epis.ctx
    out = []
    for (_, _, _, scale, raw), comp in zip(rs.f2c_pyramid(*rs.f2c_input(epis, ctx), -1.0, ftc.m_parameters, -1, ctx), ftc.m_computers):
        assert float(np.float32(scale)) == float(np.float32(comp.m_epis.scale_used))
        out.append(host(raw) * np.float32(1.0 / np.float64(np.float32(scale))))
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.uint8, np.uint16])
@pytest.mark.parametrize("channels", [1, 3])
def test_fine_to_coarse_getters(rs, channels, dtype):
    epis = field(64, 48, 5, channels, seed=24, dtype=dtype)
    ftc = rs.FineToCoarse(epis, -1.0, 2.875, 32)
    ftc.run()
    comps = ftc.m_computers
    assert len(comps) == 3   # 48 x 64, 24 x 32, 12 x 16
    depths = [host(c.m_best_depth_s_v_u) for c in comps]
    valids = [host(c.get_valid_depths_mask_s_v_u()) for c in comps]
    out_map, out_valid = (host(t) for t in ftc.get_results())
    rad = f2c_radiances(rs, epis, ftc)
    level = np.float32(ftc.m_parameters.par_shadow_level)
    assert (rr.norms(rad[0]) < level).any() and (rr.norms(rad[0]) >= level).any()
    lut = random_table(4)
    # level 0 runs the scalar range, whose hypotheses are multiples of 1/8: the planes the pyramid getters fit on qualify for
    # the exact MEANSTD comparison (module docstring).  The FUSED planes do not (the levels below carry per-pixel ranges
    # cut in 31 parts), so get_coloured_depth_maps is compared with saturate only here, and without it below on one level.
    assert np.array_equal(depths[0] * 256, np.rint(depths[0] * 256)) and np.abs(depths[0]).max() < 8
    got = host(ftc.get_coloured_depth_maps(lut))
    want = rr.f2c_coloured_depth_maps(out_map, out_valid, lut, True, rad[0], level)
    assert got.shape == (5, 48, 64, 3) and np.array_equal(got, want), int((got != want).sum())
    for saturate in (True, False):
        for s in (-1, 0, 4):
            got = [host(t) for t in ftc.get_coloured_depth_pyr(s, lut, saturate)]
            want = rr.f2c_coloured_depth_pyr(depths, valids, lut, s, saturate)
            assert [g.shape for g in got] == [(48, 64, 3), (24, 32, 3), (12, 16, 3)]
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (saturate, s)
        for v in (-1, 0, 45):
            got = [host(t) for t in ftc.get_coloured_epi_pyr(v, lut, saturate)]
            want = rr.f2c_coloured_epi_pyr(depths, valids, lut, v, saturate, rad, level)
            assert [g.shape for g in got] == [(5, 64, 3), (5, 32, 3), (5, 16, 3)]
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (saturate, v)
    # v = V_0 - 1 with V_p = V_0 / 2: 23.5 rounds up to V_p -- the reference reads out of bounds, here the call raises
    with pytest.raises(ValueError):
        ftc.get_coloured_epi_pyr(47, lut)
    with pytest.raises(ValueError):
        rr.f2c_coloured_epi_pyr(depths, valids, lut, 47)
    # without the shadow cut
    ftc.m_parameters.par_cut_shadows = False
    got = host(ftc.get_coloured_depth_maps(lut))
    assert np.array_equal(got, rr.f2c_coloured_depth_maps(out_map, out_valid, lut))
    got = [host(t) for t in ftc.get_coloured_epi_pyr(-1, lut)]
    assert all(np.array_equal(g, w) for g, w in zip(got, rr.f2c_coloured_epi_pyr(depths, valids, lut)))


def test_fine_to_coarse_depth_maps_without_saturation(rs):
    """get_coloured_depth_maps(saturate=False) on a one-level pyramid: the fused planes are then level 0's, multiples of
    1/8, so the MEANSTD fit's sums are exact in any order (module docstring)."""
    epis = field(64, 48, 5, 3, seed=26)
    ftc = rs.FineToCoarse(epis, -1.0, 2.875, 32, max_pyr_depth=1)
    ftc.run()
    out_map, out_valid = (host(t) for t in ftc.get_results())
    assert np.array_equal(out_map * 256, np.rint(out_map * 256)) and np.abs(out_map).max() < 8
    rad = f2c_radiances(rs, epis, ftc)
    lut = random_table(6)
    for saturate in (False, True):
        got = host(ftc.get_coloured_depth_maps(lut, saturate))
        want = rr.f2c_coloured_depth_maps(out_map, out_valid, lut, saturate, rad[0], np.float32(ftc.m_parameters.par_shadow_level))
        assert np.array_equal(got, want), (saturate, int((got != want).sum()))


def test_one_view_has_no_centre_plane(rs):
    """(int)std::round(S / 2.0) is S itself for S = 1: the reference indexes past its last plane, here the getters raise
    (before they touch a plane: the object need not have run)."""
    epis = field(32, 24, 1, 1, seed=25, dark=False)
    ftc = rs.FineToCoarse(epis, -1.0, 2.875, 8, max_pyr_depth=1)
    with pytest.raises(ValueError):
        ftc.get_coloured_depth_maps(GREY)
    with pytest.raises(ValueError):
        ftc.get_coloured_depth_pyr(-1, GREY)
    with pytest.raises(ValueError):
        rr.centre_index(1)
