"""The tables of tests/test_gpu_scan_instantiations.py and tests/test_gpu_scan_caller_forms.py cannot fall behind the build.

The compiled scan instantiations are read from the headers the library is built from -- RSLF_SPAD_LIST_*,
RSLF_CHIP_LADDER_* with kChipTopS / kChipMaxS / RSLF_CHIP_FIRST_S, and the resident prefixes stream_resident_for and
stream_px_resident_for can return (RSLF_STREAM_NRES_*) -- by a small host program (tests/cpp/scan_facts.cpp), which also
maps each row of the table to what it selects through the real plan::pick_spad, plan::chip_rung_for and plan::chip_takes.
Every (instantiation, launch form) cell must be selected by some row, and every row must select what it says.  A cell comes
in three caller forms: the scalar range at the centre view (the first table; the cell as it is), per-pixel [dmin, dmax]
planes ("planes", ...) and the scalar range at an off-centre view ("s_hat", ...), the two of the second table.

The tables' volumes must also make ties reach the arg max: an oracle built with the first-maximum test flipped (the last
maximum wins) must give other indices than the oracle on every one of them.  The second table's volumes are held to three
more conditions: enough pixels get a disparity, an off-centre row has a tile and a hypothesis that a classification with a
centred reach gets wrong, and the off-centre rows of the kernels with the tap table take taps from it.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import taps_ref
from tests import test_gpu_scan_caller_forms as F
from tests import test_gpu_scan_instantiations as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remotesensingproject_amd", "csrc")


def _hipcc():
    from remotesensingproject_amd import build
    return build._hipcc()


def scan_facts(tmp_path, defines=()):
    """Build tests/cpp/scan_facts.cpp (host code only) with extra -D flags and ask it about every volume of the table."""
    exe = str(tmp_path / "scan_facts")
    subprocess.run([_hipcc(), "-std=c++17", "--cuda-host-only", "-Wall", "-Werror", "-I", CSRC] + ["-D" + d for d in defines] +
                   [os.path.join(ROOT, "tests", "cpp", "scan_facts.cpp"), "-o", exe], check=True)
    queries = sorted({(c.S, c.C) for c in T.CASES + F.CASES})
    out = subprocess.run([exe], input="".join("%d %d\n" % q for q in queries), capture_output=True, text=True, check=True).stdout
    f = dict(spads={1: [], 3: []}, taps={1: [], 3: []}, rungs=[], ladder=[], nres={}, case={})
    for line in out.splitlines():
        w = line.split()
        if w[0] == "spad":
            f["spads"][int(w[1])].append(int(w[2]))
            if int(w[7]):                                             # scan_reg_tap_table
                f["taps"][int(w[1])].append(int(w[2]))
        elif w[0] == "rung":
            f["rungs"].append((w[1], int(w[4])))                      # (translation unit's list, views)
        elif w[0] == "ladder":
            f["ladder"].append(int(w[2]))
        elif w[0] == "chip":
            f.update(top=int(w[2]), max=int(w[4]), first=int(w[6]), min=int(w[8]), padmax=int(w[10]))
        elif w[0] == "nres":
            f["nres"].setdefault((int(w[1]), w[2]), set()).add(int(w[3]))
        elif w[0] == "case":
            f["case"][(int(w[1]), int(w[2]))] = dict(spad=int(w[4]), rung=int(w[6]), chip=bool(int(w[8])), nres=int(w[10]),
                                                     nres_px=int(w[12]))
    return f


def compiled_cells(f):
    """Every (instantiation, form) cell the build has; and, for the forms in which planes or an off-centre s_hat reach code of
    their own (tests/test_gpu_scan_caller_forms.py), that cell once more as ("planes", ...) and ("s_hat", ...)."""
    cells = set()
    for C, spads in f["spads"].items():
        for spad in spads:
            for form in T.REG_FORMS:
                for at in ("padded", "exact"):
                    cells.add(("reg", C, spad, form, at))
                    cells.update(caller_form_cells(f, ("reg", C, spad, form, at)))
    for (C, kind), prefixes in f["nres"].items():
        for n in prefixes:
            for form in T.STREAM_FORMS:
                if (form == "px") == (kind == "px"):
                    cells.add(("stream", C, n, form))
                    cells.update(caller_form_cells(f, ("stream", C, n, form)))
    for i in range(len(f["ladder"])):   # one workgroup per tile; and hypothesis groups once per translation unit's list
        cells.add(("chip", f["ladder"][i], "exact"))
        cells.add(("chip", f["ladder"][i], "padded"))
        cells.update(caller_form_cells(f, ("chip", f["ladder"][i], "exact")))
    if f["max"] > f["top"]:
        cells.add(("chip", f["top"], "ragged"))
        cells.update(caller_form_cells(f, ("chip", f["top"], "ragged")))
    for unit in sorted({u for u, _ in f["rungs"]}):
        cells.add(("chip-groups", unit))
    for C in (1, 3):
        cells.add(("generic", C))
        cells.update(caller_form_cells(f, ("generic", C)))
    return cells


def caller_form_cells(f, cell):
    """The `planes` and `s_hat` cells that go with a cell of the first table (the second table's docstring says why these)."""
    if cell[0] == "reg":
        C, spad, form = cell[1], cell[2], cell[3]
        kinds = [k for k, ok in (("planes", form in ("row", "groups")),
                                 ("s_hat", form == "row" or (form == "groups" and spad in f["taps"][C]))) if ok]
    elif cell[0] == "stream":
        kinds = ["planes", "s_hat"] if cell[3] in ("row_share0", "row_share2") else []
    elif cell[0] == "chip":
        kinds = ["s_hat"] if cell[2] in ("exact", "ragged") else []
    else:
        kinds = ["planes", "s_hat"]
    return [(k,) + tuple(cell) for k in kinds]


def covered_cells(f):
    """The cells the rows of the table select, through the plan's own functions, and the rows that do not select what they
    say (which cover nothing)."""
    cells, wrong = set(), []
    unit_of = {views: unit for unit, views in f["rungs"]}
    for c in T.CASES:
        q = f["case"][(c.S, c.C)]
        if c.family == "reg":
            spad = q["spad"]
            if spad != c.slots:
                wrong.append("%s: the plan picks %d slots, the table says %d" % (c.id, spad, c.slots))
                continue
            below = [n for n in f["spads"][c.C] if n < spad]
            if c.S == spad:
                cells.add(("reg", c.C, spad, c.form, "exact"))
            elif c.S > (max(below) if below else 0):
                cells.add(("reg", c.C, spad, c.form, "padded"))
        elif c.family == "stream":
            row = [r for r in T.STREAM_PREFIXES if (r[0], r[1]) == (c.C, c.S)][0]
            n = q["nres_px"] if c.form == "px" else q["nres"]
            if n != (row[3] if c.form == "px" else row[2]):
                wrong.append("%s: resident prefix %d, the table says %d" % (c.id, n, row[3] if c.form == "px" else row[2]))
                continue
            cells.add(("stream", c.C, n, c.form))
        elif c.family == "chip":
            row = [r for r in T.CHIP_RUNGS if r[0] == c.S and (r[2] > 0) == (c.form == "groups")][0]
            if not q["chip"] or q["rung"] < 0 or f["ladder"][q["rung"]] != row[1]:
                wrong.append("%s: the on-chip kernel takes %d views: %s, on rung %d; the table says the %d-view rung" % (
                    c.id, c.S, q["chip"], q["rung"], row[1]))
                continue
            views = f["ladder"][q["rung"]]
            below = f["ladder"][q["rung"] - 1] if q["rung"] > 0 else f["min"] - 1
            if c.form == "groups":
                cells.add(("chip-groups", unit_of[views]))
            elif c.S > f["top"]:
                cells.add(("chip", views, "ragged"))
            elif c.S == views:
                cells.add(("chip", views, "exact"))
            elif below < c.S and views - c.S <= f["padmax"]:
                cells.add(("chip", views, "padded"))
        else:
            cells.add(("generic", c.C))
    for c in F.CASES:
        q = f["case"][(c.S, c.C)]
        centre = c.S // 2
        if (c.kind == "planes") != (c.s_hat == centre) or (c.kind == "s_hat" and c.s_hat not in (0, c.S - 1)):
            wrong.append("%s: s_hat %d of %d views is not what a %s row runs at" % (c.id, c.s_hat, c.S, c.kind))
            continue
        if c.family == "reg":
            spad = q["spad"]
            if spad != c.slots:
                wrong.append("%s: the plan picks %d slots, the table says %d" % (c.id, spad, c.slots))
                continue
            below = [n for n in f["spads"][c.C] if n < spad]
            at = "exact" if c.S == spad else "padded" if c.S > (max(below) if below else 0) else None
            # (off centre: exact volumes at s_hat = 0, every offset of one sign; padded ones at S - 1, beside the padded slots)
            if c.kind == "s_hat" and at and c.s_hat != (0 if at == "exact" else c.S - 1):
                wrong.append("%s: an %s volume runs at s_hat %d" % (c.id, at, 0 if at == "exact" else c.S - 1))
                continue
            if at:
                cells.add((c.kind, "reg", c.C, spad, c.form, at))
        elif c.family == "stream":
            row = [r for r in T.STREAM_PREFIXES if (r[0], r[1]) == (c.C, c.S)][0]
            if q["nres"] != row[2]:
                wrong.append("%s: resident prefix %d, the table says %d" % (c.id, q["nres"], row[2]))
                continue
            cells.add((c.kind, "stream", c.C, q["nres"], c.form))
        elif c.family == "chip":
            if not q["chip"] or q["rung"] < 0:
                wrong.append("%s: the on-chip kernel does not take %d views" % (c.id, c.S))
                continue
            views = f["ladder"][q["rung"]]
            if c.S > f["top"]:
                cells.add((c.kind, "chip", views, "ragged"))
            elif c.S == views:
                cells.add((c.kind, "chip", views, "exact"))
        else:
            cells.add((c.kind, "generic", c.C))
    return cells, wrong


def missing_cells(f):
    return sorted(compiled_cells(f) - covered_cells(f)[0], key=str)


def test_every_compiled_scan_cell_has_a_row(tmp_path):
    f = scan_facts(tmp_path)
    # the build as the table's comments describe it (a change here is a change to read the table against)
    assert f["top"] == f["ladder"][-1] and f["min"] >= f["first"] and sorted(f["ladder"]) == f["ladder"]
    assert len(compiled_cells(f)) > 200
    wrong = covered_cells(f)[1]
    assert not wrong, wrong
    missing = missing_cells(f)
    assert not missing, ("compiled scan cells no row of tests/test_gpu_scan_instantiations.py (or, of a \"planes\" / \"s_hat\" cell, "
                         "of tests/test_gpu_scan_caller_forms.py) selects: %s" % missing)
    # both ends of the views among the off-centre rows of the kernels whose rows alternate
    for family in ("stream", "chip", "generic"):
        ends = {c.s_hat == 0 for c in F.CASES if c.kind == "s_hat" and c.family == family}
        assert ends == {True, False}, family


@pytest.mark.parametrize("define,cell", [
    ("RSLF_SPAD_LIST_1CH(X)=X(8) X(16) X(24) X(32) X(40) X(48) X(56) X(64) X(72) X(80) X(88) X(96) X(104) X(112) X(120) X(128) "
     "X(136) X(144) X(160) X(176) X(192)", ("reg", 1, 136, "row", "padded")),
    ("RSLF_STREAM_NRES_1CH=160", ("stream", 1, 160, "row_share0")),
])
def test_a_new_instantiation_without_a_row_is_named(tmp_path, define, cell):
    """The check is live: a slot count or resident prefix added to the build, and no row for it, fails it by name."""
    f = scan_facts(tmp_path, [define])
    missing = missing_cells(f)
    assert cell in missing, missing
    more = caller_form_cells(f, cell)
    assert {m[0] for m in more} == {"planes", "s_hat"} and all(m in missing for m in more), (more, missing)


def test_a_new_chip_rung_without_a_row_is_named(tmp_path):
    f = scan_facts(tmp_path, ["RSLF_CHIP_LADDER_A(X)=X(84, 32) X(84, 36) X(84, 40) X(84, 50)",
                              "RSLF_CHIP_LADDER_B(X)=X(84, 0) X(84, 8) X(84, 16) X(84, 24)",
                              "RSLF_CHIP_LADDER_C(X)=X(60, 0) X(68, 0) X(76, 0)"])
    assert 187 in f["ladder"]
    missing = missing_cells(f)
    assert ("chip", 187, "exact") in missing and ("chip", 187, "padded") in missing, missing
    assert ("s_hat", "chip", 187, "exact") in missing, missing


def test_every_table_volume_has_ties_that_reach_the_arg_max(tmp_path, oracle_mod, monkeypatch):
    """A scan that settled ties on the last maximum -- in any merge: lanes, waves, groups, records -- must fail some row of
    every volume.  The oracle with its minMaxLoc test flipped stands in for such a scan."""
    odir = os.path.join(ROOT, "oracle")
    src = open(os.path.join(odir, "rslf_oracle.c")).read()
    first_max = "if (w->score[d] > bestv) {"
    assert src.count(first_max) == 1, "the oracle's first-maximum test has moved: update this check"
    for name in ("rslf_oracle.h", "Makefile"):
        shutil.copy(os.path.join(odir, name), tmp_path / name)
    (tmp_path / "rslf_oracle.c").write_text(src.replace(first_max, "if (w->score[d] >= bestv) {"))
    subprocess.run(["make", "-C", str(tmp_path)], check=True, capture_output=True)
    volumes = sorted({(c.C, c.S) for c in T.CASES})
    first = {}
    for C, S in volumes:
        vol, dmin, dmax, D = T.volume(C, S)
        first[(C, S)] = oracle_mod.depth1d_pile_run(vol, dmin, dmax, D).depth_idx
    threads = oracle_mod.num_threads()
    monkeypatch.setattr(oracle_mod, "_SO", str(tmp_path / "librslf_oracle.so"))
    monkeypatch.setattr(oracle_mod, "_lib", None)
    oracle_mod.set_num_threads(threads)
    no_tie = []
    for C, S in volumes:
        vol, dmin, dmax, D = T.volume(C, S)
        last = oracle_mod.depth1d_pile_run(vol, dmin, dmax, D).depth_idx
        if np.array_equal(last, first[(C, S)]):
            no_tie.append((C, S))
    assert not no_tie, "volumes (channels, views) on which no tie reaches the arg max: %s" % no_tie


# ---- the volumes of tests/test_gpu_scan_caller_forms.py ---------------------------------------------------------------------

VOLUMES = sorted({(c.kind, c.C, c.S, c.s_hat) for c in F.CASES})


@pytest.fixture(scope="module")
def caller_form_runs(oracle_mod):
    """The oracle's run of every volume of the second table, once."""
    return {key: F.reference(oracle_mod, *key) for key in VOLUMES}


def test_every_caller_form_volume_has_ties_that_reach_the_arg_max(tmp_path, oracle_mod, monkeypatch, caller_form_runs):
    """As above, for the second table: on at least 25 pixels of every volume the last maximum is another index than the first."""
    odir = os.path.join(ROOT, "oracle")
    src = open(os.path.join(odir, "rslf_oracle.c")).read()
    first_max = "if (w->score[d] > bestv) {"
    assert src.count(first_max) == 1, "the oracle's first-maximum test has moved: update this check"
    for name in ("rslf_oracle.h", "Makefile"):
        shutil.copy(os.path.join(odir, name), tmp_path / name)
    (tmp_path / "rslf_oracle.c").write_text(src.replace(first_max, "if (w->score[d] >= bestv) {"))
    subprocess.run(["make", "-C", str(tmp_path)], check=True, capture_output=True)
    threads = oracle_mod.num_threads()
    monkeypatch.setattr(oracle_mod, "_SO", str(tmp_path / "librslf_oracle.so"))
    monkeypatch.setattr(oracle_mod, "_lib", None)
    oracle_mod.set_num_threads(threads)
    few = {}
    for key in VOLUMES:
        last = F.reference(oracle_mod, *key).depth_idx
        differ = int(np.count_nonzero(last != caller_form_runs[key].depth_idx))
        if differ < 25:
            few[key] = differ
    assert not few, "volumes (kind, channels, views, s_hat) on which fewer than 25 ties reach the arg max: %s" % few


def test_every_caller_form_volume_scans_enough_pixels(caller_form_runs):
    few = {key: int(np.count_nonzero(r.depth_idx >= 0)) for key, r in caller_form_runs.items() if np.count_nonzero(r.depth_idx >= 0) < 100}
    assert not few, "volumes (kind, channels, views, s_hat) on which fewer than 100 pixels get a disparity: %s" % few


def row_tiles(us, width):
    """scan_tile_span (k2_scan.hpp): a scanline's pixel list cut into tiles of 64 entries, or of 63 with the last one taking up
    to 64.  (first pixel, last pixel, consecutive with lane 63 free) each."""
    n = len(us)
    if width == 64:
        cuts = [(e, min(e + 64, n)) for e in range(0, n, 64)]
    else:
        T_ = max(1, (n + 61) // 63)
        cuts = [(63 * j, n if j == T_ - 1 else 63 * j + 63) for j in range(T_) if 63 * j < n]
    return [(int(us[a]), int(us[b - 1]), bool(us[b - 1] - us[a] == b - a - 1 and (width == 64 or b - a < 64))) for a, b in cuts]


def pixel_lists(oracle_mod, C, S, s_hat):
    """The scanlines' pixel lists of a Depth1DComputer_pile run: the pixels of the edge mask (K1 writes them; the shadow cut
    happens inside the scan)."""
    vol = F.volume(C, S, s_hat)[0]
    cm = oracle_mod.edge_confidence_pile(vol, s_hat)[1]
    return [np.flatnonzero(row) for row in cm]


def test_a_centred_classification_is_wrong_on_every_off_centre_row(oracle_mod, caller_form_runs):
    """An s_hat row tests the interior / border split only if the split with a centred reach, (S // 2) * |D[d]| * slope + 2,
    differs from the one with max_ds = max(s_hat, S - 1 - s_hat): on some tile that holds scanned pixels some hypothesis is
    interior by the first and border by the second.  float32 as in tests/taps_ref.py.  (The generic kernel makes no such split;
    the on-chip kernel makes it on tiles of consecutive pixels only.)"""
    f32 = np.float32
    none = []
    for c in F.CASES:
        if c.kind != "s_hat" or c.family == "generic":
            continue
        vol, dmin, dmax, D = F.volume(c.C, c.S, c.s_hat)
        U = vol.shape[2]
        scanned = caller_form_runs[(c.kind, c.C, c.S, c.s_hat)].depth_idx >= 0
        Dd = np.abs(taps_ref.hypotheses(dmin, dmax, D))
        reach = lambda ds: (((f32(ds) * Dd).astype(f32) * f32(1.0)).astype(f32) + f32(2)).astype(f32)
        true, centred = reach(max(c.s_hat, c.S - 1 - c.s_hat)), reach(c.S // 2)
        interior = lambda r, u0, u1: ((f32(u0) - r).astype(f32) >= 0) & ((f32(u1) + r).astype(f32) <= f32(U - 1))
        width = 63 if c.form == "row_share2" or c.family == "chip" else 64
        found = False
        for v, us in enumerate(pixel_lists(oracle_mod, c.C, c.S, c.s_hat)):
            for u0, u1, dense in row_tiles(us, width) if len(us) else []:
                if not scanned[v, u0:u1 + 1].any() or (c.family == "chip" and not dense):
                    continue
                found |= bool((interior(centred, u0, u1) & ~interior(true, u0, u1)).any())
        if not found:
            none.append(c.id)
    assert not none, "off-centre rows on which a centred classification is right everywhere: %s" % none


def test_the_off_centre_tap_table_rows_take_taps_from_the_table(tmp_path, oracle_mod):
    """The s_hat rows of the kernels with the tap table run the table form off centre: a positive share of their gather
    batches, counted over the volume's real tiles (the dark band leaves gaps), takes the interior form's taps from it."""
    taps = scan_facts(tmp_path)["taps"]
    rows = [c for c in F.CASES if c.kind == "s_hat" and c.family == "reg" and c.slots in taps[c.C]]
    assert {c.form for c in rows} == {"row", "groups"} and {c.s_hat == 0 for c in rows} == {True, False}
    for c in rows:
        vol, dmin, dmax, D = F.volume(c.C, c.S, c.s_hat)
        tiles = [t for us in pixel_lists(oracle_mod, c.C, c.S, c.s_hat) if len(us) for t in row_tiles(us, 64)]
        share, _ = taps_ref.batch_shares(vol.shape[2], c.S, D, dmin, dmax, s_hat=c.s_hat, tiles=tiles)
        print("%s: interior-form share of batches from the table %.3f" % (c.id, share))
        assert share > 0.0, c.id
