"""The sub-grid pile step without a GPU: the reference (tests/subgrid_ref.py) on the rows worked by hand, through the
three-score form of the rule; the shared header function (k8_peak_rule.hpp's peak_disp, the text both kernels compile) in
tests/cpp/test_plan_subgrid.cpp, a stand-alone program built with g++ under AddressSanitizer + UBSan and run directly; and
the planted-line field through the oracle's pile step, refined and then filtered."""
import os
import subprocess

import numpy as np
import pytest

import peaks_ref as pr
import subgrid_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remotesensingproject_amd", "csrc")
HAND = pr.hand_rows()


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("row", HAND, ids=[r[0] for r in HAND])
def test_hand_worked_rows_through_three_scores(row):
    name, s, lo, hi, i1, s1, disp = row[:7]
    D = len(s)
    a = s[i1 - 1] if i1 > 0 else np.float32(0)
    c = s[i1 + 1] if i1 < D - 1 else np.float32(0)
    got = sr.disp3(a, s[i1], c, i1, D, lo, hi)
    assert bits(got) == bits(disp), (name, got, disp)
    # at an end of the grid the neighbours are not read
    if i1 in (0, D - 1):
        assert bits(sr.disp3(np.float32(np.nan), s1, np.float32(np.nan), i1, D, lo, hi)) == bits(sr.grid_value(i1, D, lo, hi))


def test_shared_rule_under_sanitizers(tmp_path):
    rows = tmp_path / "hand_rows.txt"
    with open(rows, "w") as f:
        for name, s, lo, hi, i1, s1, disp, i2, s2 in HAND:
            f.write("%s %d %08x %08x %d %08x" % (name, len(s), bits(lo), bits(hi), i1, bits(disp)))
            f.write("".join(" %08x" % b for b in bits(s)) + "\n")
    exe = tmp_path / "test_plan_subgrid"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_plan_subgrid.cpp"), "-o", str(exe)],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), str(rows)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plan subgrid tests ok" in r.stdout and "%d hand-worked rows" % len(HAND) in r.stdout


def test_rule_is_stated_once():
    """Both kernels call peak_disp; the header that states it compiles without HIP."""
    rule = open(os.path.join(CSRC, "k8_peak_rule.hpp")).read()
    assert "hip/hip_runtime" not in rule and rule.count("den2 == 0.0f") == 1 and "peak_disp(i1, D, lo, hi, a, s1, c)" in rule
    k9 = open(os.path.join(CSRC, "k9_subgrid.hpp")).read()
    assert '#include "k8_peak_rule.hpp"' in k9 and "peak_disp(" in k9 and "den2" not in k9 and "scan_generic_body<" not in k9


def test_multi_device_forms_refuse_the_mode():
    from remotesensingproject_amd import depth as rs
    from remotesensingproject_amd import sharding
    with pytest.raises(ValueError, match="subgrid"):
        sharding.run_sharded(lambda shard: {}, 8, 8, 1, subgrid=True)
    with pytest.raises(ValueError, match="subgrid"):
        rs.require_no_subgrid(True, "MultiDevice.depth1d_pile")
    rs.require_no_subgrid(False, "MultiDevice.depth1d_pile")


# planted d -> (median error of the grid's filtered depth, of the refined and filtered depth, its max), as measured on the
# oracle (4 decimals)
TABLE = {0.37: (0.1200, 0.0006, 0.0021), -0.6: (0.1000, 0.0016, 0.0090), 0.1: (0.1000, 0.0015, 0.0098), 0.25: (0.0, 0.0015, 0.0040)}


@pytest.mark.parametrize("d_true", sorted(TABLE))
def test_planted_field(d_true):
    """oracle_np.depth1d_pile_run (default parameters) on V = 7 scanlines of the planted line, 9 hypotheses in [-1, 1], over
    the confident pixels of columns 16..79: off the grid the refined and filtered plane's median error is below a tenth of
    the grid's (measured ratio >= 60); every confident pixel's refined disparity differs from its grid value."""
    vol = sr.planted_field(d_true)
    out = sr.pile_run(vol, np.float32(-1), np.float32(1), 9)
    cols = slice(16, 80)
    m = out["Ce_mask"][:, cols] != 0
    assert m.sum() >= 300 and (out["idx"][:, cols][m] >= 0).all()
    grid = np.abs(out["depth"][:, cols][m].astype(np.float64) - d_true)
    sub = np.abs(out["depth_sub"][:, cols][m].astype(np.float64) - d_true)
    print("d_true %g: %d pixels, median grid %.4f, refined %.4f (max %.4f)" % (d_true, m.sum(), np.median(grid), np.median(sub), sub.max()))
    want = TABLE[d_true]
    assert abs(np.median(grid) - want[0]) < 5e-5 and abs(np.median(sub) - want[1]) < 5e-5 and abs(sub.max() - want[2]) < 5e-5
    if d_true != 0.25:
        assert np.median(sub) < 0.1 * np.median(grid)
        assert np.median(grid) / np.median(sub) >= 60
    grid_values = np.array([[sr.grid_value(max(i, 0), 9, -1, 1) for i in r] for r in out["idx"]], np.float32)
    assert (out["depth_raw_sub"][:, cols][m] != grid_values[:, cols][m]).all()
    assert np.array_equal(out["depth_raw"][:, cols][m], grid_values[:, cols][m])
    # pixels without a disparity keep the raw plane's zeros
    none = out["idx"] < 0
    assert (out["depth_raw_sub"][none] == 0).all()
