"""The table of tests/test_gpu_score_instantiations.py cannot fall behind the build, and its volumes reach what they name.

The compiled score-row kernels are read from the headers the library is built from -- RSLF_SPAD_LIST_*, with
score_rows_trim, score_rows_tap_table and scan_reg_trim of each cell from the constexpr functions themselves -- by a small
host program (tests/cpp/score_facts.cpp), which also answers, through the real plan::choose_score_kernel and
plan::score_plan, which kernel each row of the table selects and in how many hypothesis groups it runs.  Every
(channels, slots, exact | padded) cell must have a row, and a planes row; every tap-table cell its unmasked rows; every cell
whose trimmed last pass the scan never runs its off-centre rows.

The volumes are held to the conditions the table's docstring states: at least 100 scanned pixels with pixels on both sides of
column 256 (k_score_lists' second chunk), (tile, hypothesis) pairs of the interior and of the border form by the float32
rule of score_reg_rows over the row's real tiles, a positive share of gather batches from the tap table on the unmasked
rows, and, for the long rows, the per-wave shares a restatement of scan_chunk gives -- with a misplaced run or a rotated
store group visible in the reference tensor.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from tests import taps_ref
from tests import test_gpu_score_instantiations as T
from tests.test_scan_coverage_cpu import row_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remotesensingproject_amd", "csrc")
ALL_ROWS = T.ROWS_A + T.ROWS_B + T.ROWS_C
WAVES = 4   # kScanWaves; score_facts prints the header's


def _hipcc():
    from remotesensingproject_amd import build
    return build._hipcc()


def score_facts(tmp_path, defines=()):
    """Build tests/cpp/score_facts.cpp with extra -D flags and ask it about every row of the table.  (Its main runs on the host
    and calls no HIP function; k2_scores.hpp's one non-template kernel is compiled for gfx950 beside it.)"""
    exe = str(tmp_path / "score_facts")
    subprocess.run([_hipcc(), "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Werror", "-I", CSRC] + ["-D" + d for d in defines] +
                   [os.path.join(ROOT, "tests", "cpp", "score_facts.cpp"), "-o", exe], check=True)
    kernels = sorted({(r.S, r.C, int(r.hooks.get("force_scan", 0))) for r in ALL_ROWS})
    plans = sorted({(r.kernel, r.slots, r.C, r.V, r.U, r.D, int(r.hooks.get("force_groups", 0))) for r in ALL_ROWS} |
                   {(r.kernel, r.slots, r.C, 1, r.U, r.D, int(r.hooks.get("force_groups", 0))) for r in T.ROWS_C})
    text = "".join("kernel %d %d %d\n" % k for k in kernels) + "".join("plan %d %d %d %d %d %d %d\n" % p for p in plans)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    f = dict(cells={}, kernel={}, plan={})
    for line in out.splitlines():
        w = line.split()
        if w[0] == "cell":
            f["cells"][(int(w[1]), int(w[2]))] = dict(trim=bool(int(w[4])), taps=bool(int(w[6])), scan_trim=bool(int(w[8])), waves=int(w[10]))
        elif w[0] == "run":
            f.update(run=int(w[1]), waves=int(w[3]))
        elif w[0] == "kernel":
            f["kernel"][(int(w[1]), int(w[2]), int(w[3]))] = (int(w[5]), int(w[7]))
        elif w[0] == "plan":
            f["plan"][tuple(int(x) for x in w[1:8])] = (int(w[9]), int(w[11]))
    return f


@pytest.fixture(scope="module")
def facts(tmp_path_factory):
    return score_facts(tmp_path_factory.mktemp("score_facts"))


def groups_of(f, row, n_rows=None):
    groups, tile_w = f["plan"][(row.kernel, row.slots, row.C, row.V if n_rows is None else n_rows, row.U, row.D, int(row.hooks.get("force_groups", 0)))]
    assert tile_w == 64
    return groups


def compiled_cells(f):
    """Every cell the build has: ("reg", C, slots, exact | padded), a planes row of each instantiation, the unmasked rows of
    those with the tap table, the off-centre rows of those whose trimmed last pass only the score form runs."""
    cells = set()
    for (C, slots), c in f["cells"].items():
        for at in ("exact", "padded"):
            cells.add(("reg", C, slots, at))
            if c["taps"]:
                cells.add(("unmasked", C, slots, at))
            if c["trim"] and not c["scan_trim"]:
                cells.add(("s_hat", C, slots, at))
        cells.add(("planes", C, slots, "padded"))
    return cells


def covered_cells(f):
    """The cells the rows of part A select through plan::choose_score_kernel, and the rows that do not select what they say."""
    cells, wrong = set(), []
    slots_of = {C: sorted(n for c, n in f["cells"] if c == C) for C in (1, 3)}
    for r in T.ROWS_A:
        kind, spad = f["kernel"][(r.S, r.C, int(r.hooks.get("force_scan", 0)))]
        if (kind, spad) != (r.kernel, r.slots):
            wrong.append("%s: the plan picks form %d with %d slots, the table says form %d with %d" % (r.id, kind, spad, r.kernel, r.slots))
            continue
        below = [n for n in slots_of[r.C] if n < spad]
        at = "exact" if r.S == spad else "padded" if r.S > (max(below) if below else 0) else None
        if at == "padded" and r.S not in (spad - 3, spad - 1):
            wrong.append("%s: a padded row has slots - 3 views, or slots - 1" % r.id)
            continue
        centre = r.S // 2
        if r.kind in ("exact", "padded"):
            if (r.kind, r.s_hat, r.mask, r.planes) != (at, centre, "edge", False):
                wrong.append("%s: an %s row runs masked, at the centre view, with the scalar range" % (r.id, at))
                continue
            cells.add(("reg", r.C, spad, at))
        elif r.kind == "planes":
            if (r.s_hat, r.mask, r.planes) != (centre, "edge", True):
                wrong.append("%s: a planes row runs masked, at the centre view, with [dmin, dmax] planes" % r.id)
                continue
            cells.add(("planes", r.C, spad, at))
        elif r.kind == "unmasked":
            if (r.s_hat, r.mask, r.planes) != (centre, "none", False):
                wrong.append("%s: an unmasked row passes no mask" % r.id)
                continue
            cells.add(("unmasked", r.C, spad, at))
        elif r.kind == "s_hat":
            # (off centre: exact volumes at s_hat = 0, every offset of one sign; padded ones at S - 1, beside the padded slots)
            if (r.s_hat, r.mask, r.planes) != (0 if at == "exact" else r.S - 1, "edge", False):
                wrong.append("%s: an %s volume runs at s_hat %d" % (r.id, at, 0 if at == "exact" else r.S - 1))
                continue
            cells.add(("s_hat", r.C, spad, at))
        else:
            wrong.append("%s: unknown kind" % r.id)
    return cells, wrong


def missing_cells(f):
    return sorted(compiled_cells(f) - covered_cells(f)[0], key=str)


def test_every_compiled_score_cell_has_a_row(facts):
    f = facts
    assert f["run"] == T.SCORE_RUN and f["waves"] == WAVES and 64 % f["run"] == 0
    assert len(f["cells"]) >= 26 and len(compiled_cells(f)) >= 3 * len(f["cells"])
    wrong = covered_cells(f)[1]
    assert not wrong, wrong
    missing = missing_cells(f)
    assert not missing, "compiled score-row cells no row of tests/test_gpu_score_instantiations.py selects: %s" % missing
    # the table's own lists say what the headers say
    assert sorted(T.REGISTER) == sorted(f["cells"])
    assert sorted(T.TAP_TABLE) == sorted(k for k, c in f["cells"].items() if c["taps"])
    assert {k for k, c in f["cells"].items() if c["trim"] and not c["scan_trim"]} <= set(T.OFF_CENTRE)
    assert any(C == 3 for C, _ in T.OFF_CENTRE) and set(T.TAP_TABLE) <= set(T.OFF_CENTRE)
    # parts B and C run the kernels they name
    for r in T.ROWS_B + T.ROWS_C:
        assert f["kernel"][(r.S, r.C, int(r.hooks.get("force_scan", 0)))] == (r.kernel, r.slots), r.id
    print("%d instantiations; rows: %s" % (len(f["cells"]), {k: sum(r.kind == k for r in ALL_ROWS) for k in
                                                            ("exact", "padded", "planes", "unmasked", "s_hat", "long", "wide")}))


def test_a_new_instantiation_without_a_row_is_named(tmp_path):
    """The check is live: a slot count added to the build, and no row for it, fails it by name."""
    f = score_facts(tmp_path, ["RSLF_SPAD_LIST_1CH(X)=X(8) X(16) X(24) X(32) X(40) X(48) X(56) X(64) X(72) X(80) X(88) X(96) X(104) X(112) "
                               "X(120) X(128) X(136) X(144) X(160) X(176) X(192)"])
    assert (1, 136) in f["cells"]
    missing = missing_cells(f)
    for cell in (("reg", 1, 136, "exact"), ("reg", 1, 136, "padded"), ("planes", 1, 136, "padded")):
        assert cell in missing, missing
    c = f["cells"][(1, 136)]
    assert (("s_hat", 1, 136, "exact") in missing) == (c["trim"] and not c["scan_trim"])
    # and the rows for 144 slots at 141 views still select 144: nothing else goes missing
    assert {m[1:3] for m in missing} == {(1, 136)}, missing


# ---- the volumes ------------------------------------------------------------------------------------------------------

def tiles_of(oracle_mod, row, v=None):
    """The row's real tiles: k_score_lists' ascending pixel lists cut into 64 entries (scan_tile_span, tile_w = 64)."""
    mask = T.scanned(oracle_mod, row)
    return [t for vv in (range(row.V) if v is None else [v]) for t in row_tiles(np.flatnonzero(mask[vv]), 64) if mask[vv].any()]


def class_counts(row, tiles):
    """(interior, border) (tile, hypothesis) pairs by score_reg_rows' rule, float32 as in tests/taps_ref.py."""
    f32 = np.float32
    dmin, dmax = T.scalar_range(row)
    Dd = np.abs(taps_ref.hypotheses(dmin, dmax, row.D))
    reach = (((f32(max(row.s_hat, row.S - 1 - row.s_hat)) * Dd).astype(f32) * f32(1.0)).astype(f32) + f32(2)).astype(f32)
    inner = 0
    for u0, u1, _ in tiles:
        inner += int((((f32(u0) - reach).astype(f32) >= 0) & ((f32(u1) + reach).astype(f32) <= f32(row.U - 1))).sum())
    return inner, len(tiles) * row.D - inner


def test_every_row_scans_enough_pixels_in_both_chunks_and_both_forms(oracle_mod):
    """At least 100 scanned pixels a scanline, pixels on both sides of column 256, more than one tile of 64, and
    both hypothesis classes (parts A and B; the generic form classifies nothing, its rows are counted all the same)."""
    bad = []
    for r in ALL_ROWS:
        mask = T.scanned(oracle_mod, r)
        for v in range(r.V):
            n, left, right = int((mask[v] != 0).sum()), int((mask[v, :256] != 0).sum()), int((mask[v, 256:] != 0).sum())
            if n < 100:
                bad.append("%s: %d pixels in scanline %d" % (r.id, n, v))
            if r.part != "C" and (left == 0 or right == 0 or n <= 64):
                bad.append("%s: %d + %d pixels beside column 256" % (r.id, left, right))
        if r.part == "C" and r.mask == "cut":
            sides = [(int((m[:256] != 0).sum()), int((m[256:512] != 0).sum()), int((m[512:] != 0).sum())) for m in mask]
            if not (sides[0][0] == 0 and sides[0][1] > 0 and sides[1][0] > 0 and sides[1][1] == 0):
                bad.append("%s: chunks %s" % (r.id, sides))
        if r.part != "C":
            inner, border = class_counts(r, tiles_of(oracle_mod, r))
            if inner <= 0 or border <= 0:
                bad.append("%s: %d interior and %d border (tile, hypothesis) pairs" % (r.id, inner, border))
    assert not bad, bad
    assert all(r.U == 513 and r.V == 2 for r in T.ROWS_C) and {r.mask for r in T.ROWS_C} == {"cut", "none"}


def test_the_unmasked_rows_take_taps_from_the_table(facts):
    """Every unmasked row of a tap-table kernel: a positive share of all gather batches takes the interior form's taps from
    the table (tests/taps_ref.py over the row's tiles of consecutive pixels)."""
    rows = [r for r in T.ROWS_A + T.ROWS_B if r.mask == "none"]
    assert {r.kind for r in rows} == {"unmasked", "long"} and {(r.C, r.slots) for r in rows} == {k for k, c in facts["cells"].items() if c["taps"]}
    for r in rows:
        dmin, dmax = T.scalar_range(r)
        share = taps_ref.batch_shares(r.U, r.S, r.D, dmin, dmax, s_hat=r.s_hat)[0]
        print("%s: interior-form share of batches from the table %.3f" % (r.id, share))
        assert share > 0.0, r.id


# ---- the long rows ----------------------------------------------------------------------------------------------------

def wave_shares(D, groups):
    """scan_chunk (k2_scan.hpp): [d0, d1) of every wave of every group, contiguous slices of ceil(D / (4 * groups))."""
    slices = WAVES * groups
    chunk = (D + slices - 1) // slices
    out = []
    for s in range(slices):
        d0 = min(s * chunk, D)
        out.append((d0, min(d0 + chunk, D)))
    return out


def runs_of(d0, d1):
    """ScoreRows: a wave's hypotheses in runs of kScoreRun from d0, each flushed on its own."""
    return [(a, min(a + T.SCORE_RUN, d1)) for a in range(d0, d1, T.SCORE_RUN)]


def test_the_long_shapes_fill_more_than_one_run(facts):
    """The per-wave shares of part B's shapes: the sizes the table names, a wave with two or more runs, a wave of exactly
    kScoreRun (both flush conditions at once) -- in the groups plan::score_plan settles on under the row's hook
    (tests/cpp/test_plan_scores.cpp pins those).  Part A's rows, for contrast, never fill a run."""
    want = {(1, 70): [18, 18, 18, 16], (1, 133): [34, 34, 34, 31], (2, 133): [17] * 7 + [14]}
    assert sorted(want) == sorted(T.LONG_SHAPES)
    full = False
    for r in T.ROWS_B:
        force = r.hooks["force_groups"]
        groups = groups_of(facts, r)
        assert groups == force, (r.id, groups)
        shares = wave_shares(r.D, groups)
        sizes = [b - a for a, b in shares]
        assert sizes == want[(force, r.D)] and sum(sizes) == r.D, (r.id, sizes)
        runs = [[b - a for a, b in runs_of(*s)] for s in shares]
        assert any(len(x) >= 2 for x in runs), (r.id, runs)
        assert all(n == T.SCORE_RUN for x in runs for n in x[:-1])
        full |= T.SCORE_RUN in sizes
    assert full
    for force, D in T.LONG_SHAPES:
        print("force_groups=%d D=%d: runs per wave %s" % (force, D, [[b - a for a, b in runs_of(*s)] for s in wave_shares(D, force)]))
    for r in T.ROWS_A:
        assert max(b - a for a, b in wave_shares(r.D, groups_of(facts, r))) < T.SCORE_RUN, r.id


def second_run_shifted(ref, shares):
    """Every wave's second run holds the scores of the hypotheses one below (a run of one, too: its neighbour's score)."""
    out = ref.copy()
    for d0, d1 in shares:
        runs = runs_of(d0, d1)
        if len(runs) >= 2:
            a, b = runs[1]
            out[..., a:b] = ref[..., a - 1:b - 1]
    return out


def first_runs_swapped(ref, shares):
    out = ref.copy()
    for d0, d1 in shares:
        runs = runs_of(d0, d1)
        if len(runs) >= 2:
            (a0, _), (a1, b1) = runs[0], runs[1]
            n = b1 - a1
            out[..., a0:a0 + n], out[..., a1:a1 + n] = ref[..., a1:a1 + n], ref[..., a0:a0 + n]
    return out


def store_groups_rotated(ref, mask):
    """Within every tile, the pixels one store instruction covers (64 / kScoreRun consecutive list entries) rotated by one."""
    out = ref.copy()
    per = 64 // T.SCORE_RUN
    for v in range(mask.shape[0]):
        us = np.flatnonzero(mask[v])
        for t0 in range(0, len(us), 64):
            tile = us[t0:t0 + 64]
            for g0 in range(0, len(tile), per):
                g = tile[g0:g0 + per]
                out[v, g] = ref[v, np.roll(g, 1)]
    return out


@pytest.mark.parametrize("name", [k[0] for k in T.LONG_KERNELS])
def test_a_misplaced_run_is_visible_in_every_long_volume(oracle_mod, name):
    """A flush that lands one hypothesis off, two runs written at each other's place, or a store group's pixels in another
    order: each must change the reference tensor at 100 or more scanned pixels, or a comparison with it proves little."""
    for r in [r for r in T.ROWS_B if r.id.startswith(name + "-d")]:
        ref, mask = T.reference(oracle_mod, r), T.scanned(oracle_mod, r)
        shares = wave_shares(r.D, r.hooks["force_groups"])
        for what, changed in (("second run shifted", second_run_shifted(ref, shares)), ("runs 0 and 1 swapped", first_runs_swapped(ref, shares)),
                              ("store group rotated", store_groups_rotated(ref, mask))):
            differ = int(((changed.view(np.uint32) != ref.view(np.uint32)).any(axis=-1) & (mask != 0)).sum())
            print("%s, %s: %d of %d scanned pixels differ" % (r.id, what, differ, int((mask != 0).sum())))
            assert differ >= 100, (r.id, what, differ)
