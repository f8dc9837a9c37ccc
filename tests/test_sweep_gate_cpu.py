"""The sweep gate without a GPU (rslf_sweep_propagation_ratio, the *_pr entries): the numpy yardstick against the one it
extends, the conditions that make its fields and ratios working ones -- recounted, so that no GPU test passes on an idle
gate --, a one-scanline field followed by hand, the plan and rule header under sanitizers, the exports and the refusals."""
import os
import subprocess

import numpy as np
import pytest

import sweep_gate_ref as sgr
import sweep_peaks_ref as spr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remotesensingproject_amd", "csrc")
F = np.float32
OLD = ("depth", "disp_confidence", "edge_confidence", "edge_mask", "rbar", "scan_mask", "line_confidence")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def _differ(a, b):
    return int((_bits(a) != _bits(b)).sum())


def _all_equal(x, y, label):
    for k in OLD:
        assert _differ(x[0][k], y[0][k]) == 0, (label, k)
    for k in sgr.PLANES:
        assert _differ(x[1][k], y[1][k]) == 0, (label, "peak " + k)


@pytest.mark.parametrize("kw", [dict(), dict(mode=2), dict(subgrid=True)], ids=["plain", "line2", "subgrid"])
def test_ratio_off_is_the_peaks_reference(oracle_mod, kw):
    """With the ratio off sweep_gate_ref.sweep is sweep_peaks_ref.sweep on every plane, and withholds nothing."""
    vol, D, lo, hi, p = sgr.field(oracle_mod, "planted")
    V, S, U, _ = vol.shape
    lo_p, hi_p = np.full((S, V, U), lo, F), np.full((S, V, U), hi, F)
    ours = sgr.sweep(oracle_mod, vol, lo_p, hi_p, D, p, ratio=0.0, **kw)
    theirs = spr.sweep(oracle_mod, vol, lo_p, hi_p, D, p, **kw)
    _all_equal(ours, theirs, "ratio off")
    assert ours[3] == [0] * S
    for (sa, ma), (sb, mb) in zip(ours[2], theirs[2]):
        assert sa == sb and (ma == mb).all()


@pytest.mark.parametrize("name", ["planted", "A"])
def test_ratio_one_withholds_nothing(oracle_mod, name):
    """r = 1: a runner-up as high as its winner is not above it -- the gate's line runs and the planes are the ungated ones."""
    one = sgr.reference(oracle_mod, name, 1.0)
    off = sgr.reference(oracle_mod, name, 0.0)
    _all_equal(one, off, "r = 1")
    assert sum(one[3]) == 0 and one[4] == off[4]


@pytest.mark.parametrize("case", list(sgr.SWEEP_CASES))
def test_the_fields_and_ratios_are_working_ones(oracle_mod, case):
    """On the reference alone, for every sweep the GPU tests run: the first visit withholds between 5 % and 25 % of its
    sources; a later visit scans more pixels than the ungated sweep's; at least one depth, one peak value and one scan_mask byte
    differ from the ungated reference; and no reference value sits within 1e-4 of a threshold the sweep compares it with."""
    name, ratio, kw, gated = sgr.case_reference(oracle_mod, case)
    off = sgr.case_reference(oracle_mod, case, gated=False)[3]
    withheld, scanned, sources = gated[3], gated[4], gated[5]
    print(case, "ratio", ratio, "withheld", withheld, "of sources", sources, "scanned", scanned, "ungated", off[4])
    assert 0.05 <= withheld[0] / sources[0] <= 0.25, (withheld[0], sources[0])
    assert scanned[0] == off[4][0] and any(g > o for g, o in zip(scanned[1:], off[4][1:]))
    assert _differ(gated[0]["depth"], off[0]["depth"]) >= 1
    assert sum(_differ(gated[1][k], off[1][k]) for k in sgr.PLANES) >= 1
    assert _differ(gated[0]["scan_mask"], off[0]["scan_mask"]) >= 1
    assert sum(off[3]) == 0
    p = sgr.field(oracle_mod, name)[4]
    assert sgr.threshold_margin(gated[0], kw, p) > 1e-4 and sgr.threshold_margin(off[0], kw, p) > 1e-4
    if kw.get("ranges") == "mixed":   # a flat band (lo == hi) has no runner-up: a pixel scanned there is never withheld
        flat = np.arange(gated[1]["idx"].shape[2]) % 4 == 1   # (one painted from another band carries that source's peaks)
        lone = (gated[1]["idx"] >= 0) & (gated[1]["runner_idx"] == -1)
        assert lone[..., flat].sum() > 100
        assert not sgr.ambiguous(gated[1], ratio)[lone].any()


def test_the_sums_the_issue_quotes(oracle_mod):
    """Recounted, not trusted: the per-visit counts of the planted field and of case A at 0.7."""
    g = sgr.case_reference(oracle_mod, "planted_C1")[3]
    assert g[3] == [33, 17, 2, 16, 15] and g[4] == [379, 39, 33, 22, 21]
    a = sgr.case_reference(oracle_mod, "A")[3]
    assert a[3] == [347, 185, 128, 83, 61] and a[4] == [2816, 497, 320, 225, 171]


# ---- one scanline by hand --------------------------------------------------------------------------------------------------

def hand_field(U=48, S=5, split=16, seed=3):
    """One scanline, five views, a scene of disparity +1: left of column `split` (of the centre view) the texture repeats every
    4 columns, right of it it is noise.  Hypotheses -4 .. 4 in steps of 1: on the repeating part, hypothesis -3 (index 1) and +1
    (index 5) read the same samples -- two peaks of EXACTLY the same height, the wrong one first."""
    rng = np.random.RandomState(seed)
    x = np.arange(U + 40)
    pat = np.array([0.2, 0.9, 0.4, 0.7], F)
    scene = np.where(x < split + 20, pat[x % 4], rng.uniform(0.2, 0.9, U + 40)).astype(F)
    vol = np.empty((1, S, U, 1), F)
    for s in range(S):
        sh = s - S // 2
        vol[0, s, :, 0] = scene[20 + sh:20 + sh + U]
    return vol


def test_one_scanline_by_hand(oracle_mod):
    """Pixel u = 4 of the centre view lies in the repeating texture.  Its two peaks are equal: idx 1 (disparity -3, wrong) wins
    by coming first, idx 5 (+1, the scene's) is the runner-up with the same score.
      ungated: the pixel is a source in the first visit, claims itself and keeps -3;
      r = 1:   runner_score > 1 * score is false: the same;
      r = 0.7: withheld in the first visit -- counted, no claim on itself, still in the running mask after that visit.  A later
               visit's unambiguous source of disparity +1, one view further and one column along the line, paints it: it ends
               with +1, that source's peaks, and out of the mask."""
    vol = hand_field()
    S, V, U, D, c, u = 5, 1, 48, 9, 2, 4
    lo, hi = np.full((S, V, U), -4.0, F), np.full((S, V, U), 4.0, F)
    p = oracle_mod.default_params()
    off = sgr.sweep(oracle_mod, vol, lo, hi, D, p, ratio=0.0)
    one = sgr.sweep(oracle_mod, vol, lo, hi, D, p, ratio=1.0)
    gat = sgr.sweep(oracle_mod, vol, lo, hi, D, p, ratio=0.7)
    _all_equal(one, off, "r = 1 by hand")
    pk = off[1]
    assert pk["idx"][c, 0, u] == 1 and pk["runner_idx"][c, 0, u] == 5
    assert _bits(pk["score"][c, 0, u:u + 1])[0] == _bits(pk["runner_score"][c, 0, u:u + 1])[0]      # equal height, bit for bit
    assert off[0]["depth"][c, 0, u] == F(-3.0) and off[0]["scan_mask"][c, 0, u] == 0                 # the wrong winner, kept
    # gated: the first visit reads the centre view's peaks as its scan left them -- the ungated sweep's, where that view is
    # never painted again -- and counts every source among the ambiguous ones (the gate is the edge mask here)
    first = sgr.ambiguous({k: pk[k][c] for k in sgr.PLANES}, 0.7)
    assert first[0, u] and gat[3][0] == int((first & (off[0]["edge_mask"][c] != 0)).sum())
    # ... and the end: painted by an unambiguous source of another view on the line of disparity +1
    g, gp = gat[0], gat[1]
    assert g["scan_mask"][c, 0, u] == 0 and g["depth"][c, 0, u] == F(1.0)
    assert gp["idx"][c, 0, u] == 5
    sources = []
    for s1 in range(S):
        u1 = u - (s1 - c)                       # u = u1 + round(1.0 * (s1 - c) * slope), slope 1
        if s1 != c and 0 <= u1 < U and all(_bits(gp[k][s1, 0, u1:u1 + 1])[0] == _bits(gp[k][c, 0, u:u + 1])[0] for k in sgr.PLANES):
            sources.append((s1, u1))
    assert sources, "no pixel on the line carries the painted pixel's peaks"
    s1, u1 = sources[0]
    assert not sgr.ambiguous({k: gp[k][s1, 0, u1:u1 + 1] for k in sgr.PLANES}, 0.7)[0]
    # the visits after the first scanned what the withheld sources left unpainted
    assert gat[4][0] == off[4][0] and sum(gat[4][1:]) > sum(off[4][1:])


# ---- the header, the exports, the refusals ----------------------------------------------------------------------------------

def test_plan_and_rule_under_sanitizers(tmp_path):
    exe = tmp_path / "test_plan_sweep_gate"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_plan_sweep_gate.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sweep gate plan tests ok" in r.stdout


def test_the_library_exports_the_entries():
    """The entries resolve in the built library, with the binding's argument lists; the ABI version stays."""
    from remotesensingproject_amd import _lib
    names = ("rslf_sweep_propagation_ratio", "rslf_sweep_withheld", "rslf_depth_epi_2d_pr", "rslf_depth2d_run_pr",
             "rslf_depth2d_run_host_pr", "rslf_f2c_run_host_pr", "rslf_f2c_run_propagation_ratio", "rslf_f2c_run_withheld")
    for name in names:
        assert name in _lib.SYMBOLS
    L = _lib.lib()
    for name in names:
        assert getattr(L, name) is not None
    for stem in ("rslf_depth_epi_2d", "rslf_depth2d_run", "rslf_depth2d_run_host", "rslf_f2c_run_host"):
        assert len(getattr(L, stem + "_pr").argtypes) == len(getattr(L, stem + "_pk").argtypes) + 1
    assert _lib.ABI_VERSION == 6 and L.rslf_abi_version() == 6


def test_the_other_forms_refuse_the_option():
    """Checked before anything touches a device: the multi-device and sharded forms, the Python level loop, the pyramid
    without keep or without peaks, and ratios that are none."""
    from remotesensingproject_amd import depth as rs
    from remotesensingproject_amd import sharding
    epis = [np.zeros((3, 16), F)] * 12
    nothing = object.__new__(rs.MultiDevice)
    with pytest.raises(ValueError, match="propagation_ratio is not built here"):
        rs.MultiDevice.depth2d(nothing, epis, -1.0, 1.0, 9, propagation_ratio=0.7)
    with pytest.raises(ValueError, match="propagation_ratio is not built here"):
        rs.MultiDevice.fine_to_coarse(nothing, epis, -1.0, 1.0, 9, propagation_ratio=0.7)
    with pytest.raises(ValueError, match="ShardedDepth2D: propagation_ratio"):
        sharding.ShardedDepth2D(None, None, -1.0, 1.0, 9, propagation_ratio=0.7)
    with pytest.raises(ValueError, match="ShardedFineToCoarse: propagation_ratio"):
        sharding.ShardedFineToCoarse(epis, -1.0, 1.0, 9, 0, 2, propagation_ratio=0.7)
    with pytest.raises(ValueError, match="FineToCoarse: propagation_ratio"):
        rs.FineToCoarse(epis, -1.0, 1.0, 9, propagation_ratio=0.7)
    with pytest.raises(ValueError, match="keep=True"):
        rs.fine_to_coarse_run_host(epis, -1.0, 1.0, 9, propagation_ratio=0.7)
    with pytest.raises(ValueError, match="peaks=True"):
        rs.fine_to_coarse_run_host(epis, -1.0, 1.0, 9, keep=True, propagation_ratio=0.7)
    for bad in (1.5, -0.2, float("nan")):
        with pytest.raises(ValueError, match=r"not in \(0, 1\]"):
            rs.fine_to_coarse_run_host(epis, -1.0, 1.0, 9, keep=True, peaks=True, propagation_ratio=bad)
        with pytest.raises(ValueError, match=r"not in \(0, 1\]"):
            rs.Depth2DComputer(None, -1.0, 1.0, 9, peaks=True, propagation_ratio=bad)
        with pytest.raises(ValueError, match=r"not in \(0, 1\]"):
            rs.compute_2D_depth_epi(None, -1.0, 1.0, 9, None, None, None, None, None, peaks=rs.Peaks(1, 1, None, 1, 1), propagation_ratio=bad)
    with pytest.raises(ValueError, match="peaks=True"):
        rs.Depth2DComputer(None, -1.0, 1.0, 9, propagation_ratio=0.7)
    with pytest.raises(ValueError, match="all four planes"):
        rs.compute_2D_depth_epi(None, -1.0, 1.0, 9, None, None, None, None, None, propagation_ratio=0.7)
    with pytest.raises(ValueError, match="all four planes"):
        rs.compute_2D_depth_epi(None, -1.0, 1.0, 9, None, None, None, None, None, peaks=rs.Peaks(1, 1, None, None, 1), propagation_ratio=0.7)
    # off is off: None, 0 and False ask for nothing
    for off in (None, 0, 0.0, False):
        rs.require_no_propagation_ratio(off, "anything")
