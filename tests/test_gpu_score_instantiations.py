"""Every compiled score-row kernel (k2_score_rows_reg<SPAD, C> per slot count, k2_score_rows_generic<C>; k2_scores.hpp)
against oracle_np.scan_pixel: every scanned pixel's whole score row bit for bit, the caller's fill everywhere else.

tests/test_gpu_scores.py checks what the score rows are on nine volumes; this is the table of what the library compiles,
at shapes under which the sink's own code runs.  tests/test_score_coverage_cpu.py reads the compiled cells from the headers
and fails when a cell has no row here, and holds every row's volume to the conditions named below.  The tables are plain
data, importable without torch or a GPU.

Part A, ROWS_A -- one row per compiled (channels, slots), "exact" (S = slots) and "padded" (S = slots - 3, padded slots live).
Volume: one scanline of 300 pixels, uniform noise, columns 40-51 and 250-261 dark; the mask is the oracle's edge mask at
s_hat, 256-276 pixels: tiles of 64 + 64 + 64 + 64 + a ragged one, pixels on both sides of column 256 (k_score_lists goes
round its loop twice, the second dark band straddles the chunks), 24 hypotheses in [-40 / m, 100 / m] with
m = max(s_hat, S - 1 - s_hat): the lines reach 40 to 100 pixels, so every row has (tile, hypothesis) pairs of the interior form
and of the border form.  "planes": the padded volume with per-pixel [dmin, dmax] inside that range, dmin == dmax on every
7th pixel (the third body of score_reg_rows).  "unmasked": no mask, every pixel -- tiles of consecutive pixels are the only
ones that take taps from the table, so the kernels with score_rows_tap_table have these.  "s_hat": s_hat = 0 on the exact
volume, S - 1 on the padded one, mask and range taken at that s_hat: the kernels whose trimmed last pass only the score form
runs, <104, 1> and one RGB kernel.

Part B, ROWS_B -- hypothesis counts at which a wave parks more than one run of kScoreRun = 16 and flushes from a run start
other than its first hypothesis: force_groups = 1 at D = 70 (waves of 18, 18, 18, 16) and D = 133 (34, 34, 34, 31),
force_groups = 2 at D = 133 (slices of 17, the last 14).  <104, 1> masked and unmasked, <16, 1>, <24, 3> and the generic form.
The D = 133 volumes of 101 views have two scanlines and also go through rslf_depth_epi_peaks, in one pass and in two.

Part C, ROWS_C -- 513 pixels by two scanlines (three chunks of k_score_lists, the last of one pixel): the edge mask with
columns 0-255 of scanline 0 and 256-511 of scanline 1 cut away (an empty chunk before and after a full one), no mask, and a
window of one scanline; the 16-slot and the generic kernel."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

from tests import peaks_ref as pr
from tests.test_gpu_scores import assert_rows_equal

pytestmark = pytest.mark.gpu

REG, GENERIC = 1, 0   # RSLF_SCAN_REG, RSLF_SCAN_GENERIC
FILL = -7.0
FILL_I, FILL_F = -77, -7.0
SCORE_RUN = 16        # kScoreRun (rslf_plan.hpp); tests/test_score_coverage_cpu.py compares it with the header's

# (channels, slots) of every k2_score_rows_reg the library compiles (RSLF_SPAD_LIST_*; the coverage test reads the headers)
REGISTER = [(1, n) for n in (8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 104, 112, 120, 128, 144, 160, 176, 192)] + \
           [(3, n) for n in (8, 16, 24, 32, 40, 48)]
# ... those with score_rows_tap_table: the unmasked rows
TAP_TABLE = [(1, 104)]
# ... those with off-centre rows: score_rows_trim without scan_reg_trim (the trimmed last pass runs in the score form only),
# the tap table's kernel, one RGB kernel
OFF_CENTRE = [(1, 48), (1, 80), (1, 88), (1, 104), (1, 120), (1, 128), (1, 144), (3, 24)]

Row = namedtuple("Row", "id part kind C S slots s_hat U V D mask planes hooks kernel")


def padded_views(C_, slots):
    """slots - 3, or slots - 1 where slots - 3 views would select the next smaller kernel."""
    below = max([n for c, n in REGISTER if c == C_ and n < slots], default=0)
    return slots - 3 if slots - 3 > below else slots - 1


def _rows_a():
    out = []

    def add(kind, C_, S, slots, s_hat, mask="edge", planes=False):
        tail = "-at%d" % s_hat if kind == "s_hat" else ""
        out.append(Row("c%d-n%d-s%d-%s%s" % (C_, slots, S, kind, tail), "A", kind, C_, S, slots, s_hat, 300, 1, 24, mask, planes, {}, REG))

    for C_, slots in REGISTER:
        S = padded_views(C_, slots)
        add("exact", C_, slots, slots, slots // 2)
        add("padded", C_, S, slots, S // 2)
        add("planes", C_, S, slots, S // 2, planes=True)
        if (C_, slots) in TAP_TABLE:
            add("unmasked", C_, slots, slots, slots // 2, mask="none")
            add("unmasked", C_, S, slots, S // 2, mask="none")
        if (C_, slots) in OFF_CENTRE:
            add("s_hat", C_, slots, slots, 0)        # exact: every offset of one sign
            add("s_hat", C_, S, slots, S - 1)        # padded: the padded slots beside s_hat
    return out


# (force_groups, hypotheses): the per-wave shares are derived in tests/test_score_coverage_cpu.py
LONG_SHAPES = [(1, 70), (1, 133), (2, 133)]
# (name, channels, views, slots, mask, further hooks, form)
LONG_KERNELS = [
    ("c1-n104-s101", 1, 101, 104, "edge", {}, REG),
    ("c1-n104-s101-unmasked", 1, 101, 104, "none", {}, REG),    # the tap table's LDS beside the parking block
    ("c1-n16-s13", 1, 13, 16, "edge", {}, REG),                 # 7 waves per SIMD
    ("c3-n24-s21", 3, 21, 24, "edge", {}, REG),
    ("generic-c1-s13", 1, 13, 0, "edge", dict(force_scan=1), GENERIC),
]


def _rows_b():
    out = []
    for name, C_, S, slots, mask, more, kernel in LONG_KERNELS:
        for groups, D in LONG_SHAPES:
            V = 2 if (S, D) == (101, 133) else 1   # (two scanlines: the peaks of these rows are also taken in two passes)
            out.append(Row("%s-d%d-g%d" % (name, D, groups), "B", "long", C_, S, slots, S // 2, 300, V, D, mask, False,
                           dict(more, force_groups=groups), kernel))
    return out


WIDE_KERNELS = [("c1-n16-s13", 16, {}, REG), ("generic-c1-s13", 0, dict(force_scan=1), GENERIC)]


def _rows_c():
    return [Row("%s-u513-%s" % (name, mask), "C", "wide", 1, 13, slots, 6, 513, 2, 24, mask, False, h, kernel)
            for name, slots, h, kernel in WIDE_KERNELS for mask in ("cut", "none")]


ROWS_A, ROWS_B, ROWS_C = _rows_a(), _rows_b(), _rows_c()
PEAK_ROWS = [r for r in ROWS_B if (r.S, r.D) == (101, 133)]
_cache = {}


# ---- volumes, masks, ranges and the reference: plain numpy, shared with the coverage test -------------------------------

def volume(row):
    """[V, S, U, C]: uniform noise, two dark bands.  One volume per (channels, views, U, V), whatever s_hat or D."""
    key = ("vol", row.C, row.S, row.U, row.V)
    if key not in _cache:
        vol = np.random.default_rng(7000 + 10 * row.S + row.C).uniform(0.0, 1.0, size=(row.V, row.S, row.U, row.C)).astype(np.float32)
        vol[:, :, 40:52] = 0.01
        vol[:, :, 250:262] = 0.01
        _cache[key] = np.ascontiguousarray(vol)
    return _cache[key]


def scalar_range(row):
    m = max(row.s_hat, row.S - 1 - row.s_hat)
    return float(np.float32(-40.0 / m)), float(np.float32(100.0 / m))


def scanned(oracle_mod, row):
    """[V, U] u8: the pixels the call scans -- the oracle's edge mask at s_hat ("edge"), that mask with columns 0-255 of
    scanline 0 and 256-511 of scanline 1 cut away ("cut"), every pixel ("none": the call passes no mask)."""
    key = ("mask", row.C, row.S, row.U, row.V, row.s_hat, row.mask)
    if key not in _cache:
        if row.mask == "none":
            mask = np.full((row.V, row.U), 255, np.uint8)
        else:
            mask = np.ascontiguousarray(oracle_mod.edge_confidence_pile(volume(row), row.s_hat)[1]).copy()
            if row.mask == "cut":
                mask[0, 0:256] = 0
                mask[1, 256:512] = 0
        _cache[key] = mask
    return _cache[key]


def ranges(row):
    """Per-pixel [dmin, dmax] inside the row's scalar range, dmin == dmax on every 7th pixel."""
    key = ("ranges", row.C, row.S, row.U, row.V, row.s_hat)
    if key not in _cache:
        dmin, dmax = (np.float32(x) for x in scalar_range(row))
        rng = np.random.default_rng(1000 + 10 * row.S + row.C)
        width = np.float32(dmax - dmin)
        lo = (dmin + np.float32(0.3) * width * rng.uniform(0.0, 1.0, size=(row.V, row.U)).astype(np.float32)).astype(np.float32)
        hi = (dmax - np.float32(0.3) * width * rng.uniform(0.0, 1.0, size=(row.V, row.U)).astype(np.float32)).astype(np.float32)
        lo, hi = np.clip(lo, dmin, dmax), np.clip(hi, dmin, dmax)
        flat = (np.arange(row.V * row.U).reshape(row.V, row.U) % 7) == 0
        hi[flat] = lo[flat]
        assert (lo >= dmin).all() and (hi <= dmax).all() and (hi >= lo).all() and (hi == lo).sum() >= row.V * row.U // 7
        _cache[key] = (lo, hi)
    return _cache[key]


def reference(oracle_mod, row, fill=FILL):
    """[V, U, D]: oracle_np.scan_pixel's score row at every scanned pixel, `fill` elsewhere.  A pixel's row is computed once
    per (volume, s_hat, D, range form) and shared by the rows that differ in mask, hooks or window only."""
    from oracle import oracle_np as onp
    pixels = _cache.setdefault(("pixels", row.C, row.S, row.U, row.V, row.s_hat, row.D, row.planes), {})
    key = ("ref", row.C, row.S, row.U, row.V, row.s_hat, row.D, row.planes, row.mask, fill)
    if key not in _cache:
        vol, mask = volume(row), scanned(oracle_mod, row)
        if row.planes:
            lo, hi = ranges(row)
        else:
            lo, hi = (np.full((row.V, row.U), x, np.float32) for x in scalar_range(row))
        p = onp.default_params()
        want = np.full((row.V, row.U, row.D), fill, np.float32)
        for v, u in zip(*np.nonzero(mask)):
            if (v, u) not in pixels:
                pixels[(v, u)] = onp.scan_pixel(vol[v], int(u), lo[v, u], hi[v, u], row.D, row.s_hat, p)[1]
            want[v, u] = pixels[(v, u)]
        _cache[key] = want
    return _cache[key]


# ---- the device side ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rs():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from remotesensingproject_amd import depth
    return depth


def device_volume(rs, row):
    return rs.Volume.from_dense(volume(row), 1.0, rs.default_context(0))   # (factor 1: the values as they are)


def device_mask(oracle_mod, row):
    import torch
    return None if row.mask == "none" else torch.from_numpy(scanned(oracle_mod, row)).cuda()


def device_range(row):
    import torch
    return tuple(torch.from_numpy(a).cuda() for a in ranges(row)) if row.planes else scalar_range(row)


def scores(rs, oracle_mod, row, v_first=0, n_rows=None, out=None):
    """compute_1D_depth_scores into a tensor that holds FILL: (rows on the host, stats)."""
    import torch
    rows = row.V - v_first if n_rows is None else n_rows
    if out is None:
        out = torch.full((rows, row.U, row.D), FILL, dtype=torch.float32, device="cuda")
    lo, hi = device_range(row)
    got, st = rs.compute_1D_depth_scores(device_volume(rs, row), lo, hi, row.D, row.s_hat, None, device_mask(oracle_mod, row), v_first,
                                         n_rows, out, want_stats=True)
    torch.cuda.synchronize()
    return got.cpu().numpy(), st


def check_row(rs, oracle_mod, hooks, row):
    mask = scanned(oracle_mod, row)
    n = int((mask != 0).sum())
    assert n >= 100 * row.V, (row.id, n)
    want = reference(oracle_mod, row)
    assert (want[mask == 0] == FILL).all() and (want[mask != 0] >= 0).all()
    if row.hooks:
        hooks(**row.hooks)
    got, st = scores(rs, oracle_mod, row)
    # the form and the instantiation that ran: a fall-back to the generic form fails here
    assert (st.scan_kernel, st.s_pad) == (row.kernel, row.slots), (row.id, st.scan_kernel, st.s_pad)
    assert st.pixels_scanned == n and st.units == n * row.D, (row.id, st.pixels_scanned, n)
    assert_rows_equal(got, want, mask, row.id)


@pytest.mark.parametrize("row", ROWS_A, ids=[r.id for r in ROWS_A])
def test_score_instantiation_against_the_oracle(rs, oracle_mod, hooks, row):
    """Part A: every compiled register score kernel, exact and padded; planes; unmasked; off centre."""
    check_row(rs, oracle_mod, hooks, row)


@pytest.mark.parametrize("row", ROWS_B, ids=[r.id for r in ROWS_B])
def test_long_runs_against_the_oracle(rs, oracle_mod, hooks, row):
    """Part B: waves that park a full run of kScoreRun hypotheses, flush, and park the next."""
    check_row(rs, oracle_mod, hooks, row)


@pytest.mark.parametrize("row", ROWS_C, ids=[r.id for r in ROWS_C])
def test_wide_rows_against_the_oracle(rs, oracle_mod, hooks, row):
    """Part C: three chunks of k_score_lists, an empty chunk before a full one (scanline 0) and after one (scanline 1)."""
    mask = scanned(oracle_mod, row)
    if row.mask == "cut":
        assert not mask[0, :256].any() and not mask[1, 256:512].any() and all(int((m != 0).sum()) >= 100 for m in mask)
    check_row(rs, oracle_mod, hooks, row)


@pytest.mark.parametrize("row", ROWS_C, ids=[r.id for r in ROWS_C])
def test_wide_window_of_one_scanline(rs, oracle_mod, hooks, row):
    """Part C: v_first = 1, n_rows = 1 of the wide volume -> [1, U, D]; the guard region behind it keeps its fill."""
    import torch
    mask = scanned(oracle_mod, row)
    n = int((mask[1] != 0).sum())
    assert n >= 100
    if row.hooks:
        hooks(**row.hooks)
    guard = 4096
    buf = torch.full((row.U * row.D + guard,), FILL, dtype=torch.float32, device="cuda")
    got, st = scores(rs, oracle_mod, row, 1, 1, buf[:row.U * row.D].view(1, row.U, row.D))
    assert (st.scan_kernel, st.s_pad, st.pixels_scanned) == (row.kernel, row.slots, n), row.id
    assert_rows_equal(got, reference(oracle_mod, row)[1:2], mask[1:2], row.id + " window")
    assert (buf[row.U * row.D:] == FILL).all().item()


# ---- the peaks of the long rows -----------------------------------------------------------------------------------------

NAMES = ("idx", "score", "disp", "runner_idx", "runner_score")


def _is_idx(name):
    return name.endswith("idx")


def reference_planes(oracle_mod, row, fill_i=FILL_I, fill_f=FILL_F):
    """tests/peaks_ref.py on the oracle's row of every scanned pixel; the fill elsewhere."""
    key = ("peaks", row.C, row.S, row.U, row.V, row.s_hat, row.D, row.mask, fill_i, fill_f)
    if key not in _cache:
        rows, mask = reference(oracle_mod, row), scanned(oracle_mod, row)
        lo, hi = (np.float32(x) for x in scalar_range(row))
        want = {n: np.full((row.V, row.U), fill_i if _is_idx(n) else fill_f, np.int32 if _is_idx(n) else np.float32) for n in NAMES}
        for v, u in zip(*np.nonzero(mask)):
            for n, x in zip(NAMES, pr.peaks_ref(rows[v, u], lo, hi)):
                want[n][v, u] = x
        _cache[key] = want
    return _cache[key]


def assert_planes_equal(got, want, label):
    for n in NAMES:
        g, w = got[n], want[n]
        assert g.shape == w.shape and g.dtype == w.dtype, (label, n, g.shape, w.shape, g.dtype)
        bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
        assert bad.size == 0, "%s: plane %s differs at %d of %d pixels, first (row, u) = %s: got %r want %r" % (
            label, n, len(bad), g.size, tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])


@pytest.mark.parametrize("row", PEAK_ROWS, ids=[r.id for r in PEAK_ROWS])
def test_long_run_peaks(rs, oracle_mod, hooks, row):
    """The D = 133 rows of 101 views through rslf_depth_epi_peaks and its host form: the five planes of peaks_ref bit for bit,
    in one pass and, through a staging buffer of one scanline, in two."""
    import torch
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    kib = 156
    assert row.V == 2 and row.U * row.D * 4 <= kib * 1024 < 2 * row.U * row.D * 4   # one scanline of rows, not two
    mask = scanned(oracle_mod, row)
    n = int((mask != 0).sum())
    want = reference_planes(oracle_mod, row)
    want_host = {k: np.where(mask != 0, want[k], -1 if _is_idx(k) else 0).astype(want[k].dtype) for k in NAMES}
    lo, hi = scalar_range(row)
    vol, dmask = device_volume(rs, row), device_mask(oracle_mod, row)
    ctx, p = rs.default_context(0), rs.Depth1DParameters().to_c()
    for staging in (0, kib):
        hooks(staging_kib=staging, **row.hooks)
        out = rs.Peaks(*(torch.full((row.V, row.U), FILL_I if _is_idx(k) else FILL_F, dtype=torch.int32 if _is_idx(k) else torch.float32,
                                    device="cuda") for k in NAMES))
        got, st = rs.compute_1D_depth_peaks(vol, lo, hi, row.D, row.s_hat, None, dmask, out=out, want_stats=True)
        torch.cuda.synchronize()
        assert (st.scan_kernel, st.s_pad, st.pixels_scanned) == (row.kernel, row.slots, n), (row.id, staging)
        assert_planes_equal({k: t.cpu().numpy() for k, t in zip(NAMES, got)}, want, "%s staging_kib=%d" % (row.id, staging))
        # the host form: -1 / 0 at the pixels that are not scanned
        arrs = [np.full((row.V, row.U), FILL_I if _is_idx(k) else FILL_F, np.int32 if _is_idx(k) else np.float32) for k in NAMES]
        c_out, stats = _lib.RslfPeaks(*(a.ctypes.data for a in arrs)), _lib.RslfStats()
        ctx.use_current_stream()
        rc = L.rslf_depth_epi_peaks_host(ctx._h, vol._h, C.c_void_p(None), C.c_void_p(None), lo, hi, row.D, row.s_hat, C.byref(p),
                                         C.c_void_p(None if row.mask == "none" else mask.ctypes.data), 0, row.V, C.byref(c_out),
                                         C.byref(stats))
        assert rc == 0, L.rslf_last_error()
        assert (stats.scan_kernel, stats.s_pad, stats.pixels_scanned) == (row.kernel, row.slots, n), (row.id, staging)
        assert_planes_equal(dict(zip(NAMES, arrs)), want_host, "%s host form, staging_kib=%d" % (row.id, staging))
