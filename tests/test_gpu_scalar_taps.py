"""The register scan's scalar-tap form (k2_reg.hpp, scan_reg_body_scalar; k2_taps.hpp, row_exact_entry): hypotheses whose every
view offset is row-exact take tap offsets and weights as scalars from a table the context makes once per hypothesis grid and row
geometry.  Every case is held bit for bit to the oracle, and every output plane with the form (scalar_taps=1, the default) to
the same run without it (scalar_taps=0: the tap-table and per-lane forms).  320-pixel rows, 101 views (reach 27 at |D| = 0.5:
tiles 1 to 3 are interior, 0 and 4 border), row tiles forced.  Grids: -0.5..0.5 with 17 hypotheses (all row-exact), with 18
(nearly none: the other forms run), -1..1 with 7 (exact and non-exact runs alternate inside one wave's range), and 330-pixel
rows (a ragged last tile).  Variants: holes inside interior tiles, slope 0.5, s_hat 30, one and two passes (the TRIM
epilogue), hypothesis groups, a padded view count, and the table's cache: other grids and another row width on one context."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V = 3
PLANES = ("edge_confidence", "edge_mask", "disp_confidence", "depth", "rbar", "depth_idx", "score", "depth_raw", "scan_mask")
G17 = (-0.5, 0.5, 17)
G18 = (-0.5, 0.5, 18)
G7 = (-1.0, 1.0, 7)


@pytest.fixture(scope="module")
def rs():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from remotesensingproject_amd import depth
    return depth


@functools.lru_cache(maxsize=None)
def field(U, S):
    rng = np.random.default_rng(5200 + U + 7 * S)
    vol = rng.uniform(0.0, 1.0, size=(V, S, U, 1)).astype(np.float32)
    vol.setflags(write=False)
    return vol


def masks(U, holes):
    """Every pixel confident; the scan mask full, or with holes inside interior tiles: a pixel of row 1 (its later tiles start
    at 129, 193, ...) and three pixels in the middle of row 2's third tile."""
    Ce = np.ones((V, U), np.float32)
    cm = np.full((V, U), 255, np.uint8)
    mask = np.full((V, U), 255, np.uint8)
    if holes:
        mask[1, 70] = 0
        mask[2, 160:163] = 0
    return Ce, cm, mask


@functools.lru_cache(maxsize=None)
def reference(oracle_mod, U, S, grid, slope, max_iter, holes, s_hat):
    dmin, dmax, D = grid
    op = oracle_mod.default_params()
    op.slope_factor = slope
    op.mean_shift_max_iter = max_iter
    Ce, cm, mask = masks(U, holes)
    full = lambda x: np.full((V, U), x, np.float32)
    return oracle_mod.depth_epi_pile(field(U, S), full(dmin), full(dmax), D, s_hat, Ce, cm, params=op, mask_vu=mask)


def run_gpu(rs, U, S, grid, slope, max_iter, holes, s_hat, expect_exact=None):
    import torch
    dmin, dmax, D = grid
    P = rs.Depth1DParameters(par_slope_factor=slope, par_mean_shift_max_iter=max_iter)
    Ce, cm, mask = masks(U, holes)
    t = lambda a: torch.from_numpy(a.copy()).cuda()
    tCe, tcm, tmask = t(Ce), t(cm), t(mask)
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    tCd, tdepth, trbar, tidx, tsc, traw = z(V, U), z(V, U), z(V, U, 1), z(V, U, dtype=torch.int32), z(V, U), z(V, U)
    st = rs.compute_1D_depth_epi_pile(rs.Volume.from_dense(field(U, S)), dmin, dmax, D, s_hat, tCe, tcm, tCd, tdepth, trbar, P, tmask,
                                      idx_v_u=tidx, score_v_u=tsc, depth_raw_v_u=traw, want_stats=True)
    torch.cuda.synchronize()
    assert st.scan_kernel == 1 and st.s_pad == 104, (st.scan_kernel, st.s_pad)   # the row kernel that has the form
    # ... and the form itself: the launch was handed the table, with the row-exact hypotheses the CPU test counts for this
    # grid (tests/test_row_exact_cpu.py) -- a quiet fall-back to the other forms would pass every comparison below
    if expect_exact is not None:
        assert rs.default_context(0).last_scan_row_exact() == expect_exact, (rs.default_context(0).last_scan_row_exact(), expect_exact)
    assert st.pixels_scanned == int(np.count_nonzero(mask))
    out = dict(edge_confidence=tCe, edge_mask=tcm, disp_confidence=tCd, depth=tdepth, rbar=trbar, depth_idx=tidx, score=tsc,
               depth_raw=traw, scan_mask=tmask)
    return {k: a.cpu().numpy() for k, a in out.items()}


def against_oracle(g, ref, what):
    for name in ("edge_confidence", "edge_mask", "depth", "rbar", "depth_idx", "score", "depth_raw"):
        want = getattr(ref, name)
        assert np.array_equal(g[name], want), "%s: %s differs from the oracle at %s" % (what, name, np.argwhere(g[name] != want)[:3].tolist())
    # C_d goes through a double on both sides (core.hpp:641): the suite's bar for it
    assert np.abs(g["disp_confidence"].astype(np.float64) - ref.disp_confidence).max() <= 1e-5


def check(rs, oracle_mod, hooks, grid, U=320, S=101, slope=1.0, max_iter=10.0, holes=False, groups=0, s_hat=None):
    s_hat = S // 2 if s_hat is None else s_hat
    ref = reference(oracle_mod, U, S, grid, slope, max_iter, holes, s_hat)
    got = {}
    for on in (1, 0):
        hooks(scalar_taps=on, force_groups=groups, force_packed=0)   # row tiles: the only launch form with the table
        # the row-exact hypotheses of the three grids at slope 1 and 0.5, any s_hat, S = 101 or 99 (all / D in {-0.5, 0.5} / D in {-1, 0, 1})
        exact = {G17: 17, G18: 2, G7: 3}[grid]
        got[on] = run_gpu(rs, U, S, grid, slope, max_iter, holes, s_hat, expect_exact=(True, exact) if on else (False, 0))
    for name in PLANES:
        a, b = got[1][name], got[0][name]
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%s differs between scalar_taps=1 and 0" % name
    for on in (1, 0):
        against_oracle(got[on], ref, "scalar_taps=%d" % on)
    assert (ref.depth_idx >= 0).sum() > 0.9 * np.count_nonzero(masks(U, holes)[2])


@pytest.mark.parametrize("grid", [G17, G18, G7], ids=["all_exact", "nearly_none_exact", "alternating"])
def test_grids(rs, oracle_mod, hooks, grid):
    check(rs, oracle_mod, hooks, grid)


def test_ragged_last_tile(rs, oracle_mod, hooks):
    """330 pixels: the sixth tile has 10 lanes, the idle ones shadow its last pixel."""
    check(rs, oracle_mod, hooks, G17, U=330)


@pytest.mark.parametrize("grid", [G17, G7], ids=["all_exact", "alternating"])
def test_masks_with_holes(rs, oracle_mod, hooks, grid):
    """Tiles that are not runs of consecutive pixels: the scalar-tap form serves them too (the tap table does not)."""
    check(rs, oracle_mod, hooks, grid, holes=True)


def test_slope_half(rs, oracle_mod, hooks):
    check(rs, oracle_mod, hooks, G17, slope=0.5)


@pytest.mark.parametrize("grid", [G17, G7], ids=["all_exact", "alternating"])
def test_off_centre_view(rs, oracle_mod, hooks, grid):
    """s_hat = 30: offsets up to 70 |D| on one side, so more tiles are border."""
    check(rs, oracle_mod, hooks, grid, s_hat=30)


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("max_iter", [1.0, 2.0])
def test_passes_and_groups(rs, oracle_mod, hooks, max_iter, groups):
    """One pass (the K-only last pass alone) and two (one full pass, then the TRIM epilogue's); one and two hypothesis groups."""
    check(rs, oracle_mod, hooks, G17, U=330, max_iter=max_iter, groups=groups)


def test_padded_view_count(rs, oracle_mod, hooks):
    """99 views still select the 104-slot kernel: five padding slots, which repeat the last view with zero weights and are never summed."""
    check(rs, oracle_mod, hooks, G7, S=99)
    check(rs, oracle_mod, hooks, G17, S=99, holes=True)


def test_the_cached_table_follows_the_grid_and_the_row_width(rs, oracle_mod, hooks):
    """Consecutive launches on one context: another grid, the first grid again, then the same grid on wider rows (the key
    includes U), another s_hat and another slope.  A stale table shows as a mismatch with the oracle."""
    hooks(scalar_taps=1, force_groups=0, force_packed=0)
    seq = [dict(grid=G17), dict(grid=G7), dict(grid=G17), dict(grid=G17, U=330), dict(grid=G17), dict(grid=G17, s_hat=30),
           dict(grid=G17, slope=0.5), dict(grid=G17)]
    for i, kw in enumerate(seq):
        U, slope, s_hat = kw.get("U", 320), kw.get("slope", 1.0), kw.get("s_hat", 50)
        g = run_gpu(rs, U, 101, kw["grid"], slope, 10.0, False, s_hat, expect_exact=(True, {G17: 17, G7: 3}[kw["grid"]]))
        against_oracle(g, reference(oracle_mod, U, 101, kw["grid"], slope, 10.0, False, s_hat), "launch %d %r" % (i, kw))
