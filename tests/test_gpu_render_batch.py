"""The batched renderers (rslf_render_fit_many, rslf_render_planes_each, Depth2DComputer.get_disparity_maps /
get_coloured_epis) against tests/render_ref.py and against the single-plane entries called plane by plane.

As in tests/test_gpu_render.py every comparison is exact: pictures byte for byte, (min, max) with == on the doubles.
The MEANSTD fit's double sums are the one place where order could matter, so the planes are `dyadic` (multiples of
2^-8, magnitude below 8, at most 2^20 pixels per plane): every partial sum is then exact in any order.

No test provokes a fault and none reads the reference tree."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_ref as rr

pytestmark = pytest.mark.gpu

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


def dyadic(rng, shape):
    """Multiples of 2^-8 with magnitude below 8, a large share of exact zeros and few distinct values among the rest."""
    x = rng.integers(-2047, 2048, size=shape).astype(np.float32) / np.float32(256.0)
    x[rng.random(shape) < 0.3] = 0.0
    few = rng.integers(-16, 17, size=shape).astype(np.float32) / np.float32(8.0)
    return np.where(rng.random(shape) < 0.5, few, x).astype(np.float32)


def embedded3(a, pad, fill):
    """`a` [n, rows, cols] as a slice of a device buffer whose rows are `pad` elements longer."""
    buf = np.full(a.shape[:2] + (a.shape[2] + pad,), fill, a.dtype)
    buf[..., :a.shape[2]] = a
    return dev(buf)[..., :a.shape[2]]


def stack(S, V, U, seed):
    """[S, V, U] dyadic planes with a range of their own each; view 1 is constant, view 2 all zero, view 3 has a single
    outlier: the constant and zero planes keep both ranks of the select on one prefix while their neighbours split."""
    rng = np.random.default_rng(seed)
    x = dyadic(rng, (S, V, U))
    for s in range(S):   # scaled down (back onto the multiples of 2^-8) and shifted: |x| < 8 / 2 + 1.5
        x[s] = np.rint(x[s] * np.float32(2.0 ** (7 - s % 3))) / np.float32(256.0) + np.float32(s % 4 - 1.5)
    if S > 3:
        x[1] = np.float32(-2.625)
        x[2] = np.float32(0.0)
        x[3] = np.float32(0.25)
        x[3, V // 2, U // 3] = np.float32(7.5)
    valid = (rng.random((S, V, U)) < 0.6).astype(np.uint8) * 255
    assert np.array_equal(x * 256, np.rint(x * 256)) and np.abs(x).max() < 8 and V * U <= 1 << 20 and S * U <= 1 << 20
    return x, valid


def check_fit_many(rs, ctx, planes, valid, d_planes, d_valid, what):
    """render_fit_many == rr.fit per plane == render_fit plane by plane, all modes, with and without validity, twice."""
    n = planes.shape[0]
    for mode in MODES:
        for v, d_v in ((None, None), (valid, d_valid)):
            got = rs.render_fit_many(ctx, d_planes, d_v, mode)
            want = [rr.fit(planes[k], mode, None if v is None else v[k]) for k in range(n)]
            single = [rs.render_fit(ctx, d_planes[k], None if d_v is None else d_v[k], mode) for k in range(min(n, 8))]
            bad = [k for k in range(n) if got[k] != want[k]]
            print("%s mode %d valid %s: %d planes, %d differ%s" % (what, mode, v is not None, n, len(bad),
                                                                 "" if not bad else " (first: plane %d got %r want %r)" % (bad[0], got[bad[0]], want[bad[0]])))
            assert got == want, (what, mode, v is not None, bad[:5])
            assert got[:len(single)] == single, (what, mode)
            assert rs.render_fit_many(ctx, d_planes, d_v, mode) == got   # determinism: the same doubles


@pytest.mark.parametrize("U", [52, 53])   # the 16-byte path and the scalar path
def test_fit_many_views_and_epi_slices_in_place(rs, ctx, U):
    S, V = 5, 7
    x, valid = stack(S, V, U, 1000 + U)
    d_x, d_valid = dev(x), dev(valid)
    assert len({rr.fit(x[s], rr.MINMAX) for s in range(S)}) == S
    check_fit_many(rs, ctx, x, valid, d_x, d_valid, "views U=%d" % U)   # plane_stride = V * U
    # every EPI slice: rows = S, plane_stride = U, row_stride = V * U
    xe, ve = np.ascontiguousarray(x.transpose(1, 0, 2)), np.ascontiguousarray(valid.transpose(1, 0, 2))
    d_e, d_ve = d_x.permute(1, 0, 2), d_valid.permute(1, 0, 2)
    assert d_e.data_ptr() == d_x.data_ptr() and d_e.stride() == (U, V * U, 1)
    check_fit_many(rs, ctx, xe, ve, d_e, d_ve, "EPI slices U=%d" % U)


def test_fit_many_in_a_padded_buffer(rs, ctx):
    """cols = 52 would take the 16-byte path, the row stride 55 breaks its alignment; 56 keeps it."""
    x, valid = stack(5, 7, 52, 1100)
    for pad in (3, 4):
        check_fit_many(rs, ctx, x, valid, embedded3(x, pad, np.float32(1.0e6)), embedded3(valid, pad, np.uint8(255)), "pad %d" % pad)


def test_fit_many_with_several_workgroups_per_plane(rs, ctx):
    """[3, 64, 4097]: 262 208 pixels per plane -- more than one sum block and workgroup per plane, a ragged last quad."""
    x, valid = stack(3, 64, 4097, 1200)
    check_fit_many(rs, ctx, x, valid, dev(x), dev(valid), "3 x 64 x 4097")


def test_fit_many_with_many_small_planes(rs, ctx):
    """[300, 3, 5]: planes of fewer pixels than a workgroup has threads, and more planes than the cap leaves one
    workgroup each."""
    x, valid = stack(300, 3, 5, 1300)
    check_fit_many(rs, ctx, x, valid, dev(x), dev(valid), "300 x 3 x 5")


def test_fit_many_of_one_plane_is_the_single_call(rs, ctx):
    x, valid = stack(1, 37, 53, 1400)
    d_x, d_valid = dev(x), dev(valid)
    for mode in MODES:
        for d_v in (None, d_valid):
            assert rs.render_fit_many(ctx, d_x, d_v, mode) == [rs.render_fit(ctx, d_x[0], None if d_v is None else d_v[0], mode)]
    check_fit_many(rs, ctx, x, valid, d_x, d_valid, "one plane")


def half_planes(rng, n, rows, cols):
    x = rng.integers(-140, 460, size=(n, rows, cols)).astype(np.float32)
    frac = rng.random((n, rows, cols)) < 0.2
    x[frac] += rng.random(int(frac.sum())).astype(np.float32)
    x[rng.random((n, rows, cols)) < 0.1] = 0.0
    return x


@pytest.mark.parametrize("cols", [5, 52, 260])
def test_render_planes_each(rs, ctx, cols):
    rng = np.random.default_rng(2000 + cols)
    n, rows = 6, 9
    planes = half_planes(rng, n, rows, cols) * np.float32(0.5) ** np.arange(n, dtype=np.float32)[:, None, None]
    valid = (rng.random((n, rows, cols)) < 0.6).astype(np.uint8) * 255
    d_planes, d_valid = dev(planes), dev(valid)
    mm = [rr.fit(planes[k], rr.MINMAX) for k in range(n)]
    mm[1] = (-100.0, 410.0)
    mm[2] = (3.5, 3.5)   # max == min renders lut[0]
    assert len(set(mm)) == n
    lut = random_table(cols)
    for formula in (rr.SHIFT, rr.AFFINE):
        for v, mode in ((None, rr.BLACK), (valid, rr.BLACK), (valid, rr.ZERO_VALUE)):
            got = host(rs.render_planes_each(ctx, d_planes, mm, formula, lut, None if v is None else d_valid, mode))
            want = np.stack([rr.render(planes[k], mm[k][0], mm[k][1], formula, lut, None if v is None else v[k], mode) for k in range(n)])
            assert got.shape == (n, rows, cols, 3) and got.dtype == np.uint8
            assert np.array_equal(got, want), (cols, formula, mode, v is None, int((got != want).sum()))
            # ... and equals the single-range entry plane by plane
            for k in (0, n - 1):
                one = host(rs.render_planes(ctx, d_planes[k:k + 1], mm[k][0], mm[k][1], formula, lut, None if v is None else d_valid[k:k + 1], mode))
                assert np.array_equal(one[0], got[k])
    # the planes of an [S][V][U] stack read as EPI slices, in place
    got = host(rs.render_planes_each(ctx, d_planes.permute(1, 0, 2), [(-100.0, 410.0 + r) for r in range(rows)], rr.AFFINE, lut))
    want = np.stack([rr.render(planes[:, r, :], -100.0, 410.0 + r, rr.AFFINE, lut) for r in range(rows)])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("channels", [1, 3])
def test_render_planes_each_epi_batch_with_shadow_cut(rs, ctx, channels):
    """RSLF_SLICE_EPI with several planes: plane k is scanline index + k of the volume, and equals the single-plane call."""
    rng = np.random.default_rng(2100 + channels)
    V, S, U = 6, 4, 52
    seed = np.array([0.05] if channels == 1 else [0.03, 0.04, 0.0], np.float32)
    level = float(rr.norms(seed[None, :])[0])
    rad = (rng.random((V, S, U, channels)) * (0.1 if channels == 1 else 0.06)).astype(np.float32)
    rad[rng.random((V, S, U)) < 0.3] = seed   # norms on both sides of the level and exactly on it
    vol = rs.Volume.from_dense(rad, 1.0, ctx)
    planes = half_planes(rng, S, V, U)
    valid = (rng.random((S, V, U)) < 0.7).astype(np.uint8) * 255
    d_planes, d_valid = dev(planes), dev(valid)
    lut = random_table(12)
    first, n = 1, 4   # scanlines 1 .. 4
    mm = [(-100.0 - v, 410.0 + 2 * v) for v in range(first, first + n)]
    d_e, d_ve = d_planes.permute(1, 0, 2)[first:first + n], d_valid.permute(1, 0, 2)[first:first + n]
    got = host(rs.render_planes_each(ctx, d_e, mm, rr.SHIFT, lut, d_ve, rr.ZERO_VALUE, vol, rs.SLICE_EPI, first, level))
    for k in range(n):
        v = first + k
        want = rr.render(planes[:, v, :], mm[k][0], mm[k][1], rr.SHIFT, lut, valid[:, v, :], rr.ZERO_VALUE, rad[v], level)
        assert np.array_equal(got[k], want), (channels, v)
        one = host(rs.render_planes(ctx, d_planes[:, v, :].unsqueeze(0), mm[k][0], mm[k][1], rr.SHIFT, lut, d_valid[:, v, :].unsqueeze(0),
                                    rr.ZERO_VALUE, vol, rs.SLICE_EPI, v, level))
        assert np.array_equal(got[k], one[0]), (channels, v)
    assert 0 < (rr.norms(rad) < np.float32(level)).sum() < rad[..., 0].size
    # views with the cut, each over its own range
    mm = [(-100.0 - s, 410.0 + s) for s in range(1, 3)]
    got = host(rs.render_planes_each(ctx, d_planes[1:3], mm, rr.AFFINE, lut, d_valid[1:3], rr.BLACK, vol, rs.SLICE_VIEW, 1, level))
    want = np.stack([rr.render(planes[s], mm[s - 1][0], mm[s - 1][1], rr.AFFINE, lut, valid[s], rr.BLACK, rad[:, s], level) for s in (1, 2)])
    assert np.array_equal(got, want)
    with pytest.raises(Exception):   # the scanlines must lie in the volume
        rs.render_planes_each(ctx, d_planes.permute(1, 0, 2)[3:6], [(0.0, 1.0)] * 3, rr.SHIFT, lut, None, rr.BLACK, vol, rs.SLICE_EPI, 4, level)
    with pytest.raises(Exception):   # the single-range entry keeps its one-plane rule
        rs.render_planes(ctx, d_e, 0.0, 1.0, rr.SHIFT, lut, None, rr.BLACK, vol, rs.SLICE_EPI, first, level)


@pytest.fixture(scope="module")
def run2d(rs):
    from remotesensingproject_amd.synth import make_lightfield
    vol, _ = make_lightfield(96, 12, 9, 1, seed=3, dmin=-1.0, dmax=2.0, band=3)
    comp = rs.Depth2DComputer(vol, -1.0, 2.875, 32, epi_scale_factor=1.0)
    comp.run()
    return comp


def test_depth2d_batch_getters(rs, run2d):
    depth, mask = host(run2d.m_best_depth_s_v_u), host(run2d.m_edge_confidence_mask_s_v_u)
    S, V, U = depth.shape
    assert (S, V, U) == (9, 12, 96) and (mask != 0).any()
    lut = random_table(31)
    maps = host(run2d.get_disparity_maps(lut))
    assert maps.shape == (S, V, U, 3)
    assert np.array_equal(maps, np.stack([rr.disparity_map(depth[s], mask[s], lut) for s in range(S)]))
    assert np.array_equal(maps, np.stack([host(run2d.get_disparity_map(s, lut)) for s in range(S)]))
    epis = host(run2d.get_coloured_epis(lut))
    assert epis.shape == (V, S, U, 3)
    assert np.array_equal(epis, np.stack([rr.depth2d_coloured_epi(depth, mask, lut, v) for v in range(V)]))
    assert np.array_equal(epis, np.stack([host(run2d.get_coloured_epi(v, lut)) for v in range(V)]))
    assert run2d.get_disparity_maps().shape == (S, V, U, 3)   # the default table


def test_depth2d_batch_getters_under_the_disparity_confidence_switch(rs):
    """With par_use_disp_confidence_score the getters paint under C_d > (float)par_disp_score_threshold, a mask that is
    made for the call (and, on this darkened field, neither empty nor full); the EPI slices read it through the strides
    of the disparities."""
    from remotesensingproject_amd.synth import make_lightfield
    vol, _ = make_lightfield(96, 12, 9, 1, seed=27, dmin=-1.0, dmax=2.0, band=4)
    vol[:, :, :12] *= np.float32(0.04)
    par = rs.Depth1DParameters(par_use_disp_confidence_score=True)
    comp = rs.Depth2DComputer([vol[v, ..., 0] for v in range(12)], -1.0, 2.875, 32, parameters=par)
    comp.run()
    depth, conf = host(comp.m_best_depth_s_v_u), host(comp.m_disp_confidence_s_v_u)
    mask = (conf > np.float32(par.par_disp_score_threshold)).astype(np.uint8) * 255
    assert 0 < (mask != 0).sum() < mask.size
    lut = random_table(32)
    assert np.array_equal(host(comp.get_disparity_maps(lut)), np.stack([rr.disparity_map(depth[s], mask[s], lut) for s in range(9)]))
    assert np.array_equal(host(comp.get_coloured_epis(lut)), np.stack([rr.depth2d_coloured_epi(depth, mask, lut, v) for v in range(12)]))


def test_bad_arguments_are_refused(rs, ctx):
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    x = dev(np.zeros((2, 4, 8), np.float32))
    out = torch.empty((2, 4, 8, 3), dtype=torch.uint8, device="cuda")
    mm = (C.c_double * 4)(0.0, 1.0, 0.0, 1.0)
    lut = random_table()
    p_lut = lut.ctypes.data_as(C.c_void_p)
    fit = lambda n, row_stride, mode=0, planes=x.data_ptr(), res=mm: L.rslf_render_fit_many(ctx._h, planes, n, 32, 4, 8, row_stride, None, mode, res)
    assert fit(2, 8) == 0
    assert fit(0, 8) == -1 and fit(65536, 8) == -1 and fit(-1, 8) == -1      # 1 <= n_planes <= 65535
    assert fit(2, 7) == -1                                                     # row_stride < cols
    assert fit(2, 8, 3) == -1 and fit(2, 8, planes=None) == -1 and fit(2, 8, res=None) == -1
    assert L.rslf_render_fit_many(None, x.data_ptr(), 2, 32, 4, 8, 8, None, 0, mm) == -1
    each = lambda n, row_stride, table=p_lut, ranges=mm: L.rslf_render_planes_each(
        ctx._h, x.data_ptr(), n, 32, 4, 8, row_stride, ranges, 0, table, None, 0, None, 0, 0, 0.0, out.data_ptr())
    assert each(2, 8) == 0
    assert each(0, 8) == -1 and each(65536, 8) == -1 and each(2, 7) == -1
    assert each(2, 8, table=None) == -1 and each(2, 8, ranges=None) == -1      # a null table, null ranges
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        rs.render_planes_each(ctx, x, [(0.0, 1.0)], rr.SHIFT, lut)             # one range per plane
