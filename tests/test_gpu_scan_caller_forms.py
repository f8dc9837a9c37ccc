"""The table of tests/test_gpu_scan_instantiations.py, one dimension wider: the two other ways the scan is called.

The rows there all make one call: Depth1DComputer_pile with a scalar [dmin, dmax] and the centre view.  The kernels compile
other code for the calls the rest of the project makes:

`planes` rows -- per-pixel [dmin, dmax] planes (every fine-to-coarse level below the finest, compute_1D_depth_epi_pile, the
sweep entry points), s_hat = S // 2, through compute_1D_depth_epi_pile against oracle.edge_confidence_pile +
oracle.depth_epi_pile.  scan_reg_rows (k2_reg.hpp) sends a launch with planes to scan_reg_body<SPAD, C, BORDER=true,
UNIFORM_D=false, PK, 0, BestT, false, TRIM>, a body no scalar launch of the row kernel reaches, with its own registers and,
on the trimmed slot counts, the split last pass and LastPassRbar: every (channels, views, slots) of REGISTER in form `row`
and `groups`.  scan_stream_rows (k2_stream.hpp) sends them to scan_stream_body<C, true, false, NRES>: every STREAM_PREFIXES
row in `row_share0` and `row_share2` (63-entry tiles whose lane 63 must not be lent out).  The generic kernel: both volumes.
No packed or pixel-per-wave rows: k2_scan_reg_packed and the PACKED k2_scan_stream call the <BORDER=true, UNIFORM_D=false>
body whatever the range is, and k2_scan_reg_px / k2_scan_stream_px pick between their two LANE_D bodies from the reach of
the pixel's own [dmin, dmax], scalar or not -- planes select no instantiation there that the scalar rows do not run.  None
for the on-chip kernel: the plan never gives it planes (tests/test_gpu_chip.py pins that).

`s_hat` rows -- the scalar range with an off-centre s_hat (every sweep visit after the first), Depth1DComputer_pile.  What
depends on it: the interior / border split per hypothesis (max_ds = max(s_hat, S - 1 - s_hat)), the view offsets in otab, the
tap table of <104, 1> (every offset has one sign at s_hat = 0), the on-chip kernel's table, the padded slots beside
s_hat = S - 1.  Every REGISTER volume in form `row`, padded ones at s_hat = S - 1 and exact ones at 0; the kernels with the
tap table also in `groups`; every STREAM_PREFIXES row in `row_share0` and `row_share2`, every on-chip rung's exact volume
and the ragged tail with one workgroup per tile, s_hat alternating between 0 and S - 1; both generic volumes.

volume(C, S, s_hat) follows the other table's: 2 or 3 scanlines, 37 hypotheses, a row length that is no multiple of 64, the
dark band, and the tie scanline -- whose one non-constant view is s_hat.  (Radiances start at 0.1, so the band is the only
gap in the pixel lists: the tiles beside it hold consecutive pixels, which the tap table and the shared taps need.)  The range is sized from max(s_hat, S - 1 - s_hat):
the extreme hypotheses reach ~U/4 pixels from the pixel.  The planes lie inside that range and differ per pixel; a few per
cent of the pixels have dmax == dmin, so all their hypotheses are equal and index 0 must win; the MASKED volumes pass a scan
mask with holes.  tests/test_scan_coverage_cpu.py holds every volume to four conditions on the CPU: ties reach the arg max,
at least 100 pixels get a disparity, an s_hat row has a tile and a hypothesis that a centred classification gets wrong, and
the <104, 1> s_hat rows take taps from the table.  Plain data, importable without torch or a GPU."""
from collections import namedtuple

import numpy as np
import pytest

from tests import test_gpu_scan_instantiations as T
from tests.util import assert_pile_parity

pytestmark = pytest.mark.gpu

D = 37

# (channels, views) of the `planes` volumes that also pass a scan mask with holes: the trimmed kernels with the table's slot
# count, a 5-wave LDS-best one, RGB, and both streaming channel counts (a hole makes a 63-entry tile not consecutive)
MASKED = [(1, 101), (1, 104), (1, 48), (3, 45), (1, 200), (3, 57)]

# (channels, slots) of the register kernels whose s_hat rows also run in form `groups` (the tap table: scan_reg_tap_table)
TAP_TABLE = [(1, 104)]

Case = namedtuple("Case", "id kind family C S s_hat form hooks kernel slots")


def _ends(i, S):
    return 0 if i % 2 == 0 else S - 1


def _cases():
    out = []

    def add(kind, family, C, S, s_hat, form, hooks, kernel, slots):
        tail = "" if kind == "planes" else "-at%d" % s_hat
        name = "%s-%s-c%d-s%d-%s%s" % (kind, family, C, S, form, tail)
        out.append(Case(name, kind, family, C, S, s_hat, form, hooks, kernel, slots))

    for C, S, slots in T.REGISTER:
        for form in ("row", "groups"):
            add("planes", "reg", C, S, S // 2, form, T.REG_FORMS[form][0], T.REG_FORMS[form][1], slots)
    for C, S, nres, nres_px in T.STREAM_PREFIXES:
        for form in ("row_share0", "row_share2"):
            add("planes", "stream", C, S, S // 2, form, T.STREAM_FORMS[form][0], T.STREAM_FORMS[form][1], 0)
    for C, S in T.GENERIC_VOLUMES:
        add("planes", "generic", C, S, S // 2, "plain", dict(force_scan="generic"), T.GENERIC, 0)

    for C, S, slots in T.REGISTER:
        s_hat = 0 if S == slots else S - 1           # exact: every offset one sign; padded: the padded slots beside s_hat
        forms = ("row", "groups") if (C, slots) in TAP_TABLE else ("row",)
        for form in forms:
            add("s_hat", "reg", C, S, s_hat, form, T.REG_FORMS[form][0], T.REG_FORMS[form][1], slots)
    for i, (C, S, nres, nres_px) in enumerate(T.STREAM_PREFIXES):
        for j, form in enumerate(("row_share0", "row_share2")):
            add("s_hat", "stream", C, S, _ends(i + j, S), form, T.STREAM_FORMS[form][0], T.STREAM_FORMS[form][1], 0)
    chip = [S for S, rung, groups in T.CHIP_RUNGS if groups == 0 and (S == rung or S > rung)]   # exact volumes, the ragged tail
    for i, S in enumerate(chip):
        add("s_hat", "chip", 3, S, _ends(i, S), "single", dict(stream_groups=1), T.CHIP, 0)
    for i, (C, S) in enumerate(T.GENERIC_VOLUMES):
        add("s_hat", "generic", C, S, _ends(i, S), "plain", dict(force_scan="generic"), T.GENERIC, 0)
    return out


CASES = _cases()


def volume(C, S, s_hat):
    """The volume of every row with C channels, S views and centre view s_hat: (vol [V, S, U, C], dmin, dmax, D)."""
    U = 200 + (37 * S + 11 * C + 5 * s_hat) % 79     # (from ~200 pixels on a centred classification differs on some tile)
    if U % 64 == 0:
        U += 1
    V = 2 if S >= 100 else 3
    max_ds = max(s_hat, S - 1 - s_hat)
    reach = U / (4.0 * max_ds)                       # the extreme hypotheses' lines reach ~U/4 pixels from the pixel
    dmin = float(np.float32(-reach))
    dmax = float(np.float32(0.75 * reach))
    rng = np.random.default_rng(9000 + 1000 * s_hat + 10 * S + C)
    vol = rng.uniform(0.1, 1.0, size=(V, S, U, C)).astype(np.float32)   # (no pixel but the band's under the shadow level)
    vol[:, :, U // 3: U // 3 + 5] *= np.float32(0.05)   # a dark band: the shadow cut leaves a gap in the pixel lists, the
                                                         # tiles beside it hold consecutive pixels (tap table, shared taps)
    vol[1] = np.float32(0.5)                             # ties: every view but s_hat constant, so every line that stays
    vol[1, s_hat] = vol[0, s_hat]                        # inside the EPI reads the same samples
    return np.ascontiguousarray(vol), dmin, dmax, D


def planes(C, S):
    """The per-pixel range of the `planes` rows of volume(C, S, S // 2): (dmin [V, U], dmax [V, U], scan mask [V, U] or None)."""
    vol, dmin, dmax, _ = volume(C, S, S // 2)
    V, U = vol.shape[0], vol.shape[2]
    rng = np.random.default_rng(11000 + 10 * S + C)
    width = np.float32(dmax) - np.float32(dmin)
    lo = (np.float32(dmin) + np.float32(0.3) * width * rng.uniform(0.0, 1.0, size=(V, U)).astype(np.float32)).astype(np.float32)
    hi = (np.float32(dmax) - np.float32(0.3) * width * rng.uniform(0.0, 1.0, size=(V, U)).astype(np.float32)).astype(np.float32)
    lo = np.clip(lo, np.float32(dmin), np.float32(dmax))
    hi = np.clip(hi, np.float32(dmin), np.float32(dmax))
    flat = rng.uniform(size=(V, U)) < 0.04                # dmax == dmin: 37 equal hypotheses, index 0 must win
    hi[flat] = lo[flat]
    mask = None
    if (C, S) in MASKED:
        mask = np.where(rng.uniform(size=(V, U)) < 0.9, 255, 0).astype(np.uint8)
        mask[0, 70] = 0                                   # the tiles after it are consecutive but unaligned
        mask[V - 1, 100:103] = 0                          # a hole inside a tile
    return lo, hi, mask


def reference(oracle_mod, kind, C, S, s_hat):
    """The oracle's run of one volume in one caller form (oracle.PileResult; scan_mask: the mask after the scan, or None)."""
    vol, dmin, dmax, _ = volume(C, S, s_hat)
    if kind == "s_hat":
        return oracle_mod.depth1d_pile_run(vol, dmin, dmax, D, s_hat)
    lo, hi, mask = planes(C, S)
    Ce, cm = oracle_mod.edge_confidence_pile(vol, s_hat)
    return oracle_mod.depth_epi_pile(vol, lo, hi, D, s_hat, Ce, cm, mask_vu=mask)


@pytest.fixture(scope="module")
def rs():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from remotesensingproject_amd import depth
    return depth


@pytest.fixture(scope="module")
def oracle_for(oracle_mod):
    """The oracle's run of each (caller form, volume), computed once and compared with every launch form of it."""
    cache = {}

    def get(kind, C, S, s_hat):
        key = (kind, C, S, s_hat)
        if key not in cache:
            cache[key] = reference(oracle_mod, *key)
        return cache[key]
    return get


def run_planes(rs, case):
    """compute_1D_edge_confidence_pile + compute_1D_depth_epi_pile with per-pixel planes: (stats, every output plane)."""
    import torch
    vol, _, _, _ = volume(case.C, case.S, case.s_hat)
    lo, hi, mask = planes(case.C, case.S)
    V, U = lo.shape
    t = lambda a: torch.from_numpy(a.copy()).cuda()
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    v = rs.Volume.from_dense(vol)                    # (already in [0, 1): no rescale)
    tCe = z(V, U)
    tcm = rs.compute_1D_edge_confidence_pile(v, case.s_hat, tCe)
    tmask = None if mask is None else t(mask)
    tCd, tdepth, trbar, tidx, tsc, traw = z(V, U), z(V, U), z(V, U, case.C), z(V, U, dtype=torch.int32), z(V, U), z(V, U)
    st = rs.compute_1D_depth_epi_pile(v, t(lo), t(hi), D, case.s_hat, tCe, tcm, tCd, tdepth, trbar, None, tmask, idx_v_u=tidx,
                                      score_v_u=tsc, depth_raw_v_u=traw, want_stats=True)
    torch.cuda.synchronize()
    out = dict(edge_confidence=tCe, edge_mask=tcm, disp_confidence=tCd, depth=tdepth, rbar=trbar, depth_idx=tidx, score=tsc,
               depth_raw=traw)
    if tmask is not None:
        out["scan_mask"] = tmask
    return st, {k: a.cpu().numpy() for k, a in out.items()}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_scan_caller_form_against_the_oracle(rs, oracle_for, hooks, case):
    ref = oracle_for(case.kind, case.C, case.S, case.s_hat)
    if case.hooks:
        hooks(**case.hooks)
    if case.kind == "planes":
        st, got = run_planes(rs, case)
    else:
        vol, dmin, dmax, _ = volume(case.C, case.S, case.s_hat)
        comp = rs.Depth1DComputer_pile(vol, dmin, dmax, D, case.s_hat, 1.0)   # (already in [0, 1): no rescale)
        comp.run()
        st, got = comp.stats, comp.results()
    assert (st.scan_kernel, st.s_pad) == (case.kernel, case.slots), case.id
    assert_pile_parity(got, ref, label=case.id)
    if ref.scan_mask is not None:
        assert np.array_equal(got["scan_mask"], ref.scan_mask), "%s scan_mask: the mask after the scan differs" % case.id
