"""The novel view without a GPU (rslf_novel_view): the two forms of the yardstick's fill against each other, a row worked by
hand, the sign and the sub-pixel taps on a synthetic light field with truth planes, the conditions that make the hole fields
working ones -- recounted on the yardstick alone, so that no GPU test passes on an idle fill stage --, the plan and the rule
header under sanitizers, the exports, and the forms that have no getter."""
import os
import subprocess

import numpy as np
import pytest

import consistency_ref as cr
import novel_view_ref as nr
import view_warp_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remotesensingproject_amd", "csrc")
F = np.float32


def test_the_two_reference_forms_agree():
    """The running-maxima form of stage B against the loop over runs: random hit rows of every density, rows with no hit and
    with every hit, U = 1, both depth orders, max_gap 0 / 1 / 3; then whole calls on a hole field and a planted one."""
    rng = np.random.RandomState(1)
    for U in (1, 2, 7, 64):
        for density in (0.0, 0.1, 0.5, 0.9, 1.0):
            hit = rng.uniform(size=(6, U)) < density
            dw = np.where(hit, rng.randint(-2, 3, (6, U)).astype(F), F(0)).astype(F)
            dw[hit & (rng.uniform(size=(6, U)) < 0.2)] = F(-0.0)
            for nearer in (1, -1):
                for max_gap in (0, 1, 3):
                    a, b = nr.fill_vectorised(hit, dw, max_gap, nearer), nr.fill_loops(hit, dw, max_gap, nearer)
                    assert np.array_equal(a[0], b[0]) and np.array_equal(cr.bits(a[1]), cr.bits(b[1])), (U, density, nearer, max_gap)
    depth, valid = nr.hole_field(9, 2, 160)
    for kw in (dict(max_gap=0), dict(max_gap=3, nearer=-1), dict(max_gap=2, radius=2, sources=2, tol=0.05)):
        a = nr.novel(depth, valid, 1.0, (0.0, 4.0, 4.5), (0, 4, -1), **kw)
        b = nr.novel(depth, valid, 1.0, (0.0, 4.0, 4.5), (0, 4, -1), fill_form=nr.fill_loops, **kw)
        nr.assert_equal(a, b, str(kw))
    depth, valid = cr.planted(5, 1, 513)
    nr.assert_equal(nr.novel(depth, valid, -0.5, (0.0, 6.5), None, max_gap=3), nr.novel(depth, valid, -0.5, (0.0, 6.5), None, max_gap=3,
                                                                                       fill_form=nr.fill_loops), "planted")


def test_a_row_by_hand():
    """Three views, ten columns, slope 1, target view 1 excluded; view 2 is invalid everywhere, view 0 sends (u, d) to u - d:

        u      0   1   2   3   4   5   6   7   8   9
        d      x   x   2   x   2   0   0   x   x   x         (x: invalid)
        lands          0       2   5   6

    Column 1 is a crack between two foreground pixels (equal z: the left bound); 3 and 4 are a disocclusion between z = 2
    and z = 0 (the farther: the right bound); 7 .. 9 are a run at the row's end (its only bound).  With max_gap 2 the run of
    three stays a hole, the others are filled.  With the opposite depth order the disocclusion takes its left bound."""
    depth = np.zeros((3, 1, 10), F)
    depth[0, 0, [2, 4]] = 2.0
    valid = np.zeros((3, 1, 10), np.uint8)
    valid[0, 0, [2, 4, 5, 6]] = 255
    vol = np.random.RandomState(2).uniform(0.2, 1.0, (1, 3, 10, 1)).astype(F)
    for form in (nr.fill_vectorised, nr.fill_loops):
        out = nr.novel(depth, valid, 1.0, [1.0], [1], tol=0.1, volume=vol, want_err=True, fill_form=form)
        assert out["fill"][0, 0].tolist() == [1, 2, 1, 3, 3, 1, 1, 2, 2, 2]
        assert out["depth"][0, 0].tolist() == [2, 2, 2, 0, 0, 0, 0, 0, 0, 0]
        # view 0 is asked at x + d: columns 0 and 2 find their own sources, 5 and 6 theirs; the filled ones find invalid pixels
        # (1, 3, 7 .. 9) or a disparity that disagrees (4: view 0 holds 2 at column 4)
        assert out["n_src"][0, 0].tolist() == [1, 0, 1, 0, 0, 1, 1, 0, 0, 0]
        assert out["row_cov"][0, 0] == 4
        # one agreeing view of weight 1 / 2: fl(fl(g * E) / g) = E; where nobody agreed: the first view in field, view 0 at x + d
        src = [2, 3, 4, 3, 4, 5, 6, 7, 8, 9]
        assert out["colour"][0, 0, :, 0].tolist() == vol[0, 0, src, 0].tolist()
        e = np.abs(vol[0, 0, src, 0] - vol[0, 1, :, 0])
        assert out["err"][0, 0].tolist() == e.tolist() and out["row_err"][0, 0] == e[[0, 2, 5, 6]].astype(np.float64).sum()
        gap = nr.novel(depth, valid, 1.0, [1.0], [1], max_gap=2, tol=0.1, fill_form=form)
        assert gap["fill"][0, 0].tolist() == [1, 2, 1, 3, 3, 1, 1, 0, 0, 0] and gap["n_src"][0, 0].tolist() == [1, 0, 1, 0, 0, 1, 1, 0, 0, 0]
        gap = nr.novel(depth, valid, 1.0, [1.0], [1], max_gap=1, tol=0.1, fill_form=form)
        assert gap["fill"][0, 0].tolist() == [1, 2, 1, 0, 0, 1, 1, 0, 0, 0]
        far = nr.novel(depth, valid, 1.0, [1.0], [1], nearer=-1, tol=0.1, fill_form=form)
        assert far["fill"][0, 0].tolist() == [1, 2, 1, 2, 2, 1, 1, 2, 2, 2] and far["depth"][0, 0].tolist() == [2, 2, 2, 2, 2, 0, 0, 0, 0, 0]
    # a run at the row's START takes its right bound; no hit at all: no bound, all holes
    valid[0, 0, 2] = 0
    out = nr.novel(depth, valid, 1.0, [1.0], [1])
    assert out["fill"][0, 0].tolist() == [3, 3, 1, 3, 3, 1, 1, 2, 2, 2] and out["depth"][0, 0, :2].tolist() == [2, 2]
    none = nr.novel(depth, np.zeros_like(valid), 1.0, [1.0], [1])
    assert not none["fill"].any() and not none["depth"].any() and not none["n_src"].any()


@pytest.mark.parametrize("sources,radius", [(1, 0), (4, 1), (4, 0)])
def test_sign_and_sub_pixel_taps_on_truth_planes(sources, radius):
    """synth.make_lightfield(U=96, V=4, S=7) with one integral disparity per row (-2, -1, 0, 1) and the truth as planes: view
    s shows the texture at u - (c - s) * delta, so a point of view s lies in view t at u + (s - t) * delta -- the rule's
    column with slope 1 and d = delta -- and every backward tap falls on a pixel (w = 0).  With tol = 0, leave-one-out, every
    view: err == 0 EXACTLY at every pixel with n_src > 0, and coverage 1 on the columns at least 3 * max|delta| from the border.

    Exactly zero needs a blend that is exact: every view shows the same radiance E, and fl(fl(sum g E) / fl(sum g)) == E when
    every weight is 1 / 2 (one source, whose nearest view is at distance 1; or radius 1, where only such views are asked:
    E / 2 + E / 2 = E, sum g = 1).  With sources 4 and no radius the weights 1 / 3 and 1 / 4 round: three products, three sums
    and a division, each within 2^-24 relative, of values below 1 -- err <= 8 * 2^-24 there, and coverage is still 1."""
    from remotesensingproject_amd.synth import make_lightfield
    U, V, S = 96, 4, 7
    vol, delta = make_lightfield(U, V, S, 1, seed=3, dmin=-2.0, dmax=1.0, band=1)
    assert delta.tolist() == [-2.0, -1.0, 0.0, 1.0]
    depth = np.broadcast_to(delta[None, :, None], (S, V, U)).astype(F)
    loo = wr.leave_one_out(S)
    out = nr.novel(depth, None, 1.0, *loo, radius=radius, sources=sources, tol=0.0, volume=vol, want_err=True)
    got = out["n_src"] > 0
    worst = float(out["err"][got].max())
    print("sources %d radius %d: max err %.3g, coverage %.4f" % (sources, radius, worst, got.mean()))
    assert worst == 0.0 if (sources == 1 or radius == 1) else worst <= 8 * 2.0 ** -24
    margin = int(3 * np.abs(delta).max())
    assert got[:, :, margin:U - margin].all()
    assert (out["fill"][:, :, margin:U - margin] == nr.HIT).all()
    # the other sign does not explain the light field
    wrong = nr.novel(-depth, None, 1.0, *loo, radius=radius, sources=sources, tol=0.0, volume=vol, want_err=True)
    assert float(wrong["err"][:, [0, 1, 3]][wrong["n_src"][:, [0, 1, 3]] > 0].mean()) > 0.1
    # half a pixel: the truth halved with slope 2 is the same line; delta = 1 seen from t = 2.5 taps between two pixels
    half = nr.novel((depth * F(0.5)).astype(F), None, 2.0, [2.5], None, sources=1, tol=0.0, volume=vol)
    row = half["colour"][0, 3, margin:U - margin, 0]     # view 2 at x + 0.5: the mean of two neighbours
    x = np.arange(margin, U - margin)
    sample = ((F(0.5) * vol[3, 2, x, 0]).astype(F) + (F(0.5) * vol[3, 2, x + 1, 0]).astype(F)).astype(F)
    g = F(1) / F(1.5)                                   # one source at distance 1 / 2
    assert row.tolist() == ((g * sample).astype(F) / g).astype(F).tolist()
    assert np.abs(row - sample).max() <= 2.0 ** -23


def test_the_hole_fields_are_working_ones():
    """The issue's bars, recounted on hole_field(9, 2, 160): target 0, exclude 0, radius 1, sources 4, tol 0.1."""
    S, V, U = 9, 2, 160
    depth, valid = nr.field("hole", S, V, U)
    a = nr.field_novel("hole", S, V, U, (0.0,), (0,), 1, max_gap=0)
    fill, n_src = a["fill"], a["n_src"]
    filled = (fill == nr.LEFT) | (fill == nr.RIGHT)
    shares = dict(left=(fill == nr.LEFT).mean(), right=(fill == nr.RIGHT).mean(), holes=(fill == nr.HOLE).mean(),
                  filled_blended=(filled & (n_src > 0)).mean(), filled_unblended=(filled & (n_src == 0)).mean())
    print("max_gap 0:", {k: round(float(x), 3) for k, x in shares.items()})
    assert shares["left"] >= 0.05 and shares["right"] >= 0.05 and shares["holes"] == 0
    assert shares["filled_blended"] >= 0.05 and shares["filled_unblended"] >= 0.02
    b = nr.field_novel("hole", S, V, U, (0.0,), (0,), 1, max_gap=3)
    holes, filled3 = float((b["fill"] == nr.HOLE).mean()), float(((b["fill"] == nr.LEFT) | (b["fill"] == nr.RIGHT)).mean())
    print("max_gap 3: holes %.3f filled %.3f filled and unblended %.3f" % (
        holes, filled3, float((((b["fill"] == nr.LEFT) | (b["fill"] == nr.RIGHT)) & (b["n_src"] == 0)).mean())))
    assert holes >= 0.03 and filled3 >= 0.10
    c = S // 2
    centre = nr.field_novel("hole", S, V, U, (float(c),), (c,), 0)
    print("centre view, radius 0: n_src >= 2 on %.3f" % float((centre["n_src"] >= 2).mean()))
    assert (centre["n_src"] >= 2).mean() >= 0.80
    # among the runs with two bounds of different z both sides are taken
    w = wr.warp(depth, valid, 1.0, (0.0,), (0,), 1)
    hit, dw = w["hit"][0] != 0, w["depth"][0]
    taken = set()
    for v in range(V):
        for x in range(1, U - 1):
            if not hit[v, x] and hit[v, x - 1]:
                end = x
                while end < U and not hit[v, end]:
                    end += 1
                if end < U and dw[v, x - 1] != dw[v, end]:
                    taken.add(int(fill[0, v, x]))
    assert taken == {nr.LEFT, nr.RIGHT}


def test_plan_and_rule_under_sanitizers(tmp_path):
    exe = tmp_path / "test_plan_novel"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_plan_novel.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "novel plan tests ok" in r.stdout


def test_the_library_exports_the_entries():
    """The entries resolve in the built library, with the binding's argument lists; the ABI version stays."""
    import ctypes as C
    from remotesensingproject_amd import _lib
    names = ("rslf_novel_view", "rslf_novel_view_host", "rslf_f2c_run_novel_view", "rslf_f2c_run_novel_view_host")
    for name in names:
        assert name in _lib.SYMBOLS
    L = _lib.lib()
    for name in names:
        assert getattr(L, name) is not None
    assert len(L.rslf_novel_view.argtypes) == len(L.rslf_novel_view_host.argtypes) == 13
    assert len(L.rslf_f2c_run_novel_view.argtypes) == len(L.rslf_f2c_run_novel_view_host.argtypes) == 9
    assert C.sizeof(_lib.RslfNovelViewOut) == 7 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.RslfNovelViewParams) == 4 * C.sizeof(C.c_int) + C.sizeof(C.c_float)
    assert _lib.ABI_VERSION == 6 and L.rslf_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "rslf_hip.h")).read()
    for name in names:
        assert "int %s(" % name in header
    # refused before a device is touched: no context
    assert L.rslf_novel_view(None, None, None, 1, 1, 1, 1.0, None, None, None, 1, None, None) == -1
    assert L.rslf_novel_view_host(None, None, None, 1, 1, 1, 1.0, None, None, None, 1, None, None) == -1
    assert L.rslf_f2c_run_novel_view(None, None, 0, 0, None, None, 1, None, None) == -1
    assert L.rslf_f2c_run_novel_view_host(None, None, 0, 0, None, None, 1, None, None) == -1


def test_the_unit_is_registered():
    from remotesensingproject_amd import build
    assert "rslf_novel.hip" in build.UNITS
    for h in ("k15_novel_view.hpp", "k15_novel_rule.hpp", "rslf_plan_novel.hpp"):
        assert h in build.UNITS["rslf_novel.hip"] and os.path.exists(os.path.join(CSRC, h))
    rule = open(os.path.join(CSRC, "k15_novel_rule.hpp")).read()
    assert '#include "k14_warp_rule.hpp"' in rule and "hip/" not in rule


def test_the_forms_without_a_getter_say_so():
    """Checked before anything touches a device: the multi-device and sharded forms and the Python level loop have no novel
    view; bad targets, a nearer of 0, sources below 1 and a tolerance that is none are refused by name."""
    from remotesensingproject_amd import depth as rs
    from remotesensingproject_amd import sharding
    for cls in (rs.MultiDevice, rs.FineToCoarse, sharding.ShardedDepth2D, sharding.ShardedFineToCoarse):
        with pytest.raises(ValueError, match="get_novel_views is not built here"):
            cls.get_novel_views(object.__new__(cls), [0])
        with pytest.raises(ValueError, match="get_novel_view_prediction is not built here"):
            cls.get_novel_view_prediction(object.__new__(cls))
    for bad in (float("nan"), float("inf"), 65537.0):
        with pytest.raises(ValueError, match="not a finite position"):
            rs.novel_view(None, None, None, None, 1.0, [0.0, bad])
    with pytest.raises(ValueError, match="no targets"):
        rs.novel_view(None, None, None, None, 1.0, [])
    with pytest.raises(ValueError, match="nearer"):
        rs.novel_view(None, None, None, None, 1.0, [0.0], nearer=0)
    with pytest.raises(ValueError, match="sources 0"):
        rs.novel_view(None, None, None, None, 1.0, [0.0], sources=0)
    for bad in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="not a tolerance"):
            rs.novel_view(None, None, None, None, 1.0, [0.0], tol=bad)
    with pytest.raises(ValueError, match="exclude has 1 entries for 2 targets"):
        rs.novel_view(None, None, None, None, 1.0, [0.0, 1.0], exclude=[0])
    assert rs.NovelView._fields == nr.NAMES
    assert rs.NovelViewPrediction._fields[:5] == ("err", "fill", "n_src", "mean_abs_error", "coverage")
    for cls in (rs.Depth2DComputer, rs.KeptFineToCoarse):
        assert callable(cls.get_novel_views) and callable(cls.get_novel_view_prediction)
