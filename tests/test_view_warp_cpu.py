"""The view warp without a GPU (rslf_view_warp): the two forms of the yardstick against each other, the conditions that make the
planted fields working ones -- recounted on the yardstick alone, so that no GPU test passes on an idle z-buffer --, the plan
and the rule header under sanitizers, the exports, and the forms that have no getter."""
import os
import subprocess

import numpy as np
import pytest

import consistency_ref as cr
import view_warp_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remotesensingproject_amd", "csrc")
F = np.float32
WORKING = [sh for sh in cr.SHAPES if sh[0] >= 5]
IDS = ["S%d_V%d_U%d_r%d" % sh for sh in WORKING]


def test_the_two_reference_forms_agree():
    """The lexsort form against the plain triple loop on (5, 2, 41): every integral target leave-one-out, a target between
    two views, two outside the range; then a radius, slope -0.5 and the opposite depth order; then the radiances."""
    S, V, U = 5, 2, 41
    depth, valid = cr.planted(S, V, U)
    targets = (0.0, 1.0, 2.0, 3.0, 4.0, 2.5, -1.0, 5.0)
    exclude = (0, 1, 2, 3, 4, -1, -1, -1)
    a, b = wr.warp(depth, valid, 1.0, targets, exclude), wr.warp_loops(depth, valid, 1.0, targets, exclude)
    wr.assert_equal(a, b, "slope 1")
    assert (a["hit"] != 0).any() and (a["count"] >= 2).any() and (a["hit"] == 0).any()
    a, b = wr.warp(depth, None, -0.5, targets, exclude, 2, -1), wr.warp_loops(depth, None, -0.5, targets, exclude, 2, -1)
    wr.assert_equal(a, b, "slope -0.5, radius 2, nearer -1, no validity plane")
    vol = wr.normalised(np.random.RandomState(3).randint(0, 256, (V, S, U, 3)).astype(np.uint8))
    loo = wr.leave_one_out(S)
    a, b = wr.warp(depth, valid, 1.0, *loo, volume=vol, want_err=True), wr.warp_loops(depth, valid, 1.0, *loo, volume=vol, want_err=True)
    wr.assert_equal(a, b, "radiances")
    assert (a["err"] > 0).any() and (a["row_err"] > 0).all() and a["row_hits"].sum() == (a["hit"] != 0).sum()


def test_the_winner_by_hand():
    """Three views, six columns, slope 1, target view 1 excluded.  View 0 sends (u, d) to u - d, view 2 to u + d.

        view 0:  0    0    1    1    2x   0         (2x: invalid)
        view 2:  0    1    0    NaN  0    -2
    """
    nan = np.nan
    depth = np.array([[[0, 0, 1, 1, 2, 0]], [[9, 9, 9, 9, 9, 9]], [[0, 1, 0, nan, 0, -2]]], F)
    valid = np.full((3, 1, 6), 255, np.uint8)
    valid[0, 0, 4] = 0
    out = wr.warp(depth, valid, 1.0, [1.0], [1])
    # column 1 receives view 0's pixels 1 (d = 0) and 2 (d = 1): the greater z wins; column 2 three pixels, two of them with z = 1
    assert out["src_view"][0, 0].tolist() == [0, 0, 0, 2, 2, 0]
    assert out["src_col"][0, 0].tolist() == [0, 2, 3, 5, 4, 5]
    assert out["count"][0, 0].tolist() == [2, 2, 3, 1, 1, 1]
    assert out["depth"][0, 0].tolist() == [0, 1, 1, -2, 0, 0]
    # equal z at equal distance: the smaller view (column 0: view 0's and view 2's zero); the other order keeps the smallest z
    far = wr.warp(depth, valid, 1.0, [1.0], [1], nearer=-1)
    assert far["src_view"][0, 0].tolist() == [0, 0, 2, 2, 2, 0] and far["depth"][0, 0, 1] == 0
    # one view, and that one excluded: nobody is left
    none = wr.warp(depth[:1], valid[:1], 1.0, [0.0], [0])
    assert not none["hit"].any() and (none["src_view"] == -1).all() and (none["src_col"] == -1).all() and not none["depth"].any()


@pytest.mark.parametrize("shape", WORKING, ids=IDS)
def test_the_planted_fields_are_working_ones(shape):
    """A recount, and a condition: with the shape's own radius and the centre view as target, excluded, at least 90 % of the
    target pixels receive two or more candidates -- the z-buffer decides -- and at least 90 % are hit.  Target 0 leaves holes."""
    S, V, U, radius = shape
    c = S // 2
    out = wr.planted_warp(S, V, U, radius, (float(c),), (c,))
    several, hit = float((out["count"] >= 2).mean()), float((out["hit"] != 0).mean())
    print(shape, "two or more candidates %.3f, hit %.3f" % (several, hit))
    assert several >= 0.90 and hit >= 0.90
    assert ((out["hit"] != 0) == (out["count"] > 0)).all() and ((out["src_view"] >= 0) == (out["hit"] != 0)).all()
    assert not (out["src_view"] == c).any()
    edge = wr.planted_warp(S, V, U, radius, (0.0,), (0,))
    print(shape, "target 0: two or more %.3f, hit %.3f" % (float((edge["count"] >= 2).mean()), float((edge["hit"] != 0).mean())))
    # (the 37-column field is the exception: sixteen other views reach every one of its columns)
    assert 0 < (edge["hit"] != 0).sum() and ((edge["hit"] != 0).sum() < edge["hit"].size or U < 300)


def test_the_tie_field_is_decided_by_distance_then_view():
    """On the field without jitter more than half of the hit pixels of the centre target have a runner-up of equal disparity."""
    depth = wr.tie_field()
    S = depth.shape[0]
    c = S // 2
    share = wr.tied_share(depth, None, 1.0, float(c), c)
    print("tied share %.3f" % share)
    assert share > 0.5
    out = wr.warp(depth, None, 1.0, [float(c)], [c])
    won = out["src_view"][out["hit"] != 0]
    assert set(np.unique(won)) <= {c - 1, c + 1} and (won == c - 1).sum() > (won == c + 1).sum()   # the nearest views, the smaller first
    half = wr.warp(depth, None, 1.0, [c + 0.5], None)    # distance tie between c and c + 1: the smaller view
    won = half["src_view"][half["hit"] != 0]
    assert (won == c).sum() > (won == c + 1).sum() and set(np.unique(won)) <= {c, c + 1}


def test_plan_and_rule_under_sanitizers(tmp_path):
    exe = tmp_path / "test_plan_warp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_plan_warp.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "warp plan tests ok" in r.stdout


def test_the_library_exports_the_entries():
    """The entries resolve in the built library, with the binding's argument lists; the ABI version stays."""
    import ctypes as C
    from remotesensingproject_amd import _lib
    names = ("rslf_view_warp", "rslf_view_warp_host", "rslf_f2c_run_view_warp", "rslf_f2c_run_view_warp_host")
    for name in names:
        assert name in _lib.SYMBOLS
    L = _lib.lib()
    for name in names:
        assert getattr(L, name) is not None
    assert len(L.rslf_view_warp.argtypes) == len(L.rslf_view_warp_host.argtypes) == 14
    assert len(L.rslf_f2c_run_view_warp.argtypes) == len(L.rslf_f2c_run_view_warp_host.argtypes) == 10
    assert C.sizeof(_lib.RslfViewWarpOut) == 9 * C.sizeof(C.c_void_p)
    assert _lib.ABI_VERSION == 6 and L.rslf_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "rslf_hip.h")).read()
    for name in names:
        assert "int %s(" % name in header
    # refused before a device is touched: no context
    assert L.rslf_view_warp(None, None, None, 1, 1, 1, 1.0, None, None, None, 1, 0, 1, None) == -1
    assert L.rslf_f2c_run_view_warp(None, None, 0, 0, None, None, 1, 0, 1, None) == -1


def test_the_unit_is_registered():
    from remotesensingproject_amd import build
    assert "rslf_warp.hip" in build.UNITS and "k14_view_warp.hpp" in build.UNITS["rslf_warp.hip"]


def test_the_forms_without_a_getter_say_so():
    """Checked before anything touches a device: the multi-device and sharded forms and the Python level loop have no warp
    getter; bad targets, a nearer of 0 and a volume that is missing are refused by name."""
    from remotesensingproject_amd import depth as rs
    from remotesensingproject_amd import sharding
    for cls in (rs.MultiDevice, rs.FineToCoarse, sharding.ShardedDepth2D, sharding.ShardedFineToCoarse):
        with pytest.raises(ValueError, match="get_warped_views is not built here"):
            cls.get_warped_views(object.__new__(cls), [0])
        with pytest.raises(ValueError, match="get_view_prediction is not built here"):
            cls.get_view_prediction(object.__new__(cls))
    for bad in (float("nan"), float("inf"), -float("inf"), 65537.0, 1e30):
        with pytest.raises(ValueError, match="not a finite position"):
            rs.view_warp(None, None, None, 1.0, [0.0, bad])
    with pytest.raises(ValueError, match="no targets"):
        rs.view_warp(None, None, None, 1.0, [])
    with pytest.raises(ValueError, match="nearer"):
        rs.view_warp(None, None, None, 1.0, [0.0], nearer=0)
    with pytest.raises(ValueError, match="exclude has 1 entries for 2 targets"):
        rs.view_warp(None, None, None, 1.0, [0.0, 1.0], exclude=[0])
    assert rs.Warp._fields == wr.NAMES
    assert rs.ViewPrediction._fields[:4] == ("err", "hit", "mean_abs_error", "coverage")
