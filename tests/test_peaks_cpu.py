"""The score-row peaks without a GPU: the numpy restatement (tests/peaks_ref.py) on rows worked by hand and on the planted
line; the shared header rule (k8_peak_rule.hpp, the text the kernel compiles) and the plan functions
(rslf_plan_peaks.hpp) in tests/cpp/test_plan_peaks.cpp, a stand-alone program built with g++ under AddressSanitizer +
UBSan and run directly, on the same hand-worked rows."""
import os
import subprocess

import numpy as np
import pytest

import peaks_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remotesensingproject_amd", "csrc")
HAND = pr.hand_rows()


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("row", HAND, ids=[r[0] for r in HAND])
def test_hand_worked_rows(row):
    name, s, lo, hi, i1, s1, disp, i2, s2 = row
    got = pr.peaks_ref(s, lo, hi)
    assert (got[0], got[3]) == (i1, i2), (name, got)
    assert bits(got[1]) == bits(s1) and bits(got[2]) == bits(disp) and bits(got[4]) == bits(s2), (name, got)


def test_hand_worked_rows_cover_the_rule():
    """Winner at 0, at D-1 and inside; den2 == 0; delta = +0.5 (c == s1) and a negative delta; no runner-up on a monotone
    row, an all-equal row and D = 2; a runner-up tied with the winner; plateaus; lo == hi."""
    seen = {n: pr.branches(s) for n, s, *_ in HAND}
    assert "first" in seen["winner_first"] and "no_runner" in seen["winner_first"]
    assert "last" in seen["winner_last"] and "no_runner" in seen["winner_last"]
    assert {"interior", "fitted"} <= seen["interior"] and {"interior", "fitted", "runner"} <= seen["runner"]
    assert {"interior", "den2_zero"} <= seen["den2_zero"]
    assert {"interior", "clamp"} <= seen["delta_plus_half"] and {"interior", "clamp", "runner"} <= seen["plateaus"]
    assert {"first", "no_runner"} <= seen["all_equal"] and {"first", "no_runner"} <= seen["two_equal"]
    assert {"last", "no_runner"} <= seen["two_rising"] and "tied_runner" in seen["tied_runner"]
    by = {r[0]: r for r in HAND}
    assert by["delta_negative"][6] < 2.0 and by["flat_range"][2] == by["flat_range"][3] and len(by["two_equal"][1]) == 2
    # den2 is zero because the sum rounds, not because the points are equal
    s = by["den2_zero"][1]
    assert s[0] < s[1] and np.float32(s[0] + s[2]) == np.float32(s[1] + s[1])


def test_peak_rule_and_plan_unit_tests_under_sanitizers(tmp_path):
    rows = tmp_path / "hand_rows.txt"
    with open(rows, "w") as f:
        for name, s, lo, hi, i1, s1, disp, i2, s2 in HAND:
            f.write("%s %d %08x %08x %d %08x %08x %d %08x" % (name, len(s), bits(lo), bits(hi), i1, bits(s1), bits(disp), i2, bits(s2)))
            f.write("".join(" %08x" % b for b in bits(s)) + "\n")
    exe = tmp_path / "test_plan_peaks"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_plan_peaks.cpp"), "-o", str(exe)],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), str(rows)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plan peaks tests ok" in r.stdout and "%d hand-worked rows" % len(HAND) in r.stdout


def test_peak_headers_are_host_compilable():
    """k8_peak_rule.hpp is compiled by g++ alone, like k2_taps.hpp; rslf_plan_peaks.hpp is host-only like rslf_plan.hpp."""
    rule = open(os.path.join(CSRC, "k8_peak_rule.hpp")).read()
    assert "hip/hip_runtime" not in rule and "__global__" not in rule and "peak_row" in rule
    plan = open(os.path.join(CSRC, "rslf_plan_peaks.hpp")).read()
    assert "hip/hip_runtime" not in plan and "__device__" not in plan and "__global__" not in plan
    kernel = open(os.path.join(CSRC, "k8_peaks.hpp")).read()
    assert '#include "k8_peak_rule.hpp"' in kernel and "scan.offer(" in kernel and "scan.finish(" in kernel


def planted_errors(d_true, disp_of_row):
    """(|disp - d_true|, |grid value - d_true|) at pixels 16..79 of the planted line, the rows from oracle_np.scan_pixel."""
    from oracle import oracle_np as onp
    epi = pr.planted_epi(d_true)[:, :, None]
    p = onp.default_params()
    sub, grid = [], []
    for u in range(16, 80):
        Dv, score = onp.scan_pixel(epi, u, np.float32(-1), np.float32(1), 9, 4, p)[:2]
        i1, disp = disp_of_row(u, score)
        sub.append(abs(np.float64(disp) - d_true))
        grid.append(abs(np.float64(Dv[i1]) - d_true))
    return np.array(sub), np.array(grid)


@pytest.mark.parametrize("d_true", [0.37, -0.6, 0.1, 0.25])
def test_planted_line_on_the_reference(d_true):
    """A line of disparity d_true through a smooth texture, 9 views, 9 hypotheses in [-1, 1] (step 0.25): off the grid the
    sub-grid disparity's median error is at most a quarter of the grid arg max's (measured: 0.006, 0.023, 0.020 of it); on
    the grid it stays within half a step (measured max 0.037)."""
    def ref(u, score):
        r = pr.peaks_ref(score, -1.0, 1.0)
        return r[0], r[2]
    sub, grid = planted_errors(d_true, ref)
    print("d_true %g: median |disp - d| %.5f, median |grid - d| %.5f, max |disp - d| %.5f" % (d_true, np.median(sub), np.median(grid), sub.max()))
    if d_true == 0.25:
        assert sub.max() <= 0.125
    else:
        assert np.median(sub) <= 0.25 * np.median(grid)
