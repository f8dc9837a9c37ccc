"""The cross-view consistency check without a GPU (rslf_view_consistency): the conditions that make the planted fields working
ones -- recounted on the yardstick alone, so that no GPU test passes on an idle check --, one scanline counted by hand, the
rule header as a stand-alone program against the yardstick bit for bit, the plan and the rule under sanitizers, the exports
and the forms that have no getter."""
import os
import subprocess

import numpy as np
import pytest

import consistency_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remotesensingproject_amd", "csrc")
F = np.float32
IDS = ["S%d_V%d_U%d_r%d" % sh for sh in cr.SHAPES]


@pytest.mark.parametrize("shape", cr.SHAPES, ids=IDS)
def test_the_planted_fields_are_working_ones(shape):
    """On the yardstick alone, for every planted field with S > 1: at least 20 % of the ok pixels have an agreeing view, at
    least 10 % one above and 10 % one below, at least 1 % a target out of field (seen below the field's maximum), and the
    fused value differs from the pixel's own on at least 20 %.  With one view every count is 0."""
    S, V, U, radius = shape
    depth, valid = cr.planted(S, V, U)
    out = cr.planted_reference(S, V, U, radius)
    sh = cr.shares(depth, valid, out)
    print(shape, " ".join("%s %.3f" % kv for kv in sh.items()))
    ok = cr.ok_mask(depth, valid)
    assert 0.80 < ok.mean() < 0.95 and (valid == 0).sum() > 0
    assert depth.size < 1000 or np.isnan(depth).sum() > 0   # (1 % of the 140 pixels of the smallest field may be none)
    for k in cr.NAMES:   # a pixel that is not ok: all 0
        assert not out[k][~ok].any(), k
    if S == 1:
        for k in ("seen", "agree", "above", "below"):
            assert not out[k].any(), k
        assert cr.bits(out["fused"][ok]).tolist() == cr.bits(depth[ok]).tolist() and (out["valid"][ok] == 255).all()
        return
    assert sh["agree"] >= 0.20 and sh["above"] >= 0.10 and sh["below"] >= 0.10 and sh["partly_out"] >= 0.01 and sh["fused"] >= 0.20, sh
    assert (out["seen"] >= out["agree"] + out["above"] + out["below"]).all()
    n_views = (min(S - 1, 2 * radius) if radius > 0 else S - 1)
    assert out["seen"].max() == n_views


def test_min_agree_only_moves_the_valid_plane():
    S, V, U, radius = cr.SHAPES[0]
    base = cr.planted_reference(S, V, U, radius)
    depth, valid = cr.planted(S, V, U)
    ok = cr.ok_mask(depth, valid)
    for m in (0, 1, S):
        out = cr.planted_reference(S, V, U, radius, min_agree=m)
        cr.assert_equal_bitwise(out, base, "min_agree=%d" % m, names=cr.NAMES[:5])
        assert ((out["valid"] == 255) == (ok & (base["agree"] >= m))).all()
    assert (cr.planted_reference(S, V, U, radius, min_agree=0)["valid"] == np.where(ok, 255, 0)).all()
    assert 0 < (cr.planted_reference(S, V, U, radius, min_agree=1)["valid"] == 255).sum() < ok.sum()
    assert not cr.planted_reference(S, V, U, radius, min_agree=S)["valid"].any()   # S - 1 other views at the most


def test_one_scanline_by_hand():
    """Three views, six columns, slope 1, tol 0.125: the pixel (s, u) of disparity d looks at column u + round(d * (s - t)) of view t.

        view 0:  1    1    1    1    1    1
        view 1:  1    1x   1    NaN  2    1        (1x: invalid)
        view 2:  1    1    1.1  0    1    1
    """
    nan = np.nan
    depth = np.array([[[1, 1, 1, 1, 1, 1]], [[1, 1, 1, nan, 2, 1]], [[1, 1, 1.1, 0, 1, 1]]], F)
    valid = np.full((3, 1, 6), 255, np.uint8)
    valid[1, 0, 1] = 0
    out = cr.consistency(depth, valid, 1.0, 0.125, 0, 1)

    def px(s, u):
        return tuple(int(out[k][s, 0, u]) for k in ("seen", "agree", "above", "below")) + (out["fused"][s, 0, u], int(out["valid"][s, 0, u]))

    assert px(1, 2) == (2, 2, 0, 0, F(1), 255)                  # view 0 at column 3 and view 2 at column 1 hold 1
    assert px(0, 5) == (2, 0, 1, 1, F(1), 0)                    # view 1 at column 4 holds 2 (above), view 2 at column 3 holds 0 (below)
    assert px(0, 4) == (2, 1, 0, 0, (F(1) + F(1.1)) / F(2), 255)   # view 1 at column 3 is a NaN: seen only; view 2 at column 2 agrees
    assert px(0, 2) == (2, 1, 0, 0, F(1), 255)                  # view 1 at column 1 is invalid: seen only
    assert px(0, 0) == (0, 0, 0, 0, F(1), 0)                    # both targets left of the field; nobody agrees: not valid at min_agree 1
    assert px(1, 3) == (0, 0, 0, 0, F(0), 0) and px(1, 1) == (0, 0, 0, 0, F(0), 0)   # a NaN and an invalid pixel: nothing
    assert px(1, 4) == (1, 0, 0, 1, F(2), 0)                    # d = 2: view 0 at column 6 is out, view 2 at column 2 holds 1.1 (below)
    # the radius: from view 0 with radius 1, view 2 is not asked
    near = cr.consistency(depth, valid, 1.0, 0.125, 1, 0)
    assert (int(near["seen"][0, 0, 5]), int(near["above"][0, 0, 5]), int(near["below"][0, 0, 5])) == (1, 1, 0)
    # ties round away from zero: d = 0.5 one view apart lands one column along, to either side
    half = np.full((3, 1, 6), 0.5, F)
    half[0, 0, 3] = 9.0
    half[2, 0, 1] = -9.0
    tie = cr.consistency(half, None, 1.0, 0.125, 0, 0)
    assert (int(tie["above"][1, 0, 2]), int(tie["below"][1, 0, 2]), int(tie["agree"][1, 0, 2])) == (1, 1, 0)   # columns 3 and 1, not 2
    assert int(tie["agree"][1, 0, 3]) == 2


def _run_rule_program(exe, tmp_path, depth, valid, slope, tol, radius, min_agree):
    S, V, U = depth.shape
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.ascontiguousarray(depth, F).tobytes())
        if valid is not None:
            f.write(np.ascontiguousarray(valid, np.uint8).tobytes())
    subprocess.run([str(exe), str(src), str(dst), str(S), str(V), str(U), repr(float(slope)), repr(float(tol)), str(radius), str(min_agree),
                    "1" if valid is not None else "0"], check=True)
    raw = open(dst, "rb").read()
    n = S * V * U
    assert len(raw) == n * 21
    out = {k: np.frombuffer(raw, np.int32, n, i * 4 * n).reshape(S, V, U) for i, k in enumerate(cr.NAMES[:4])}
    out["fused"] = np.frombuffer(raw, F, n, 16 * n).reshape(S, V, U)
    out["valid"] = np.frombuffer(raw, np.uint8, n, 20 * n).reshape(S, V, U)
    return out


def test_the_rule_header_equals_the_yardstick(tmp_path):
    """csrc/k12_consistency_rule.hpp through g++ (no fused multiply-add), pixel by pixel, against the numpy yardstick on
    every planted field: all six planes, every pixel, bit for bit -- also without the validity plane, with slope 0.5 and tol 0,
    and on a field of infinities, huge values and NaNs."""
    exe = tmp_path / "consistency_rule_main"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "consistency_rule_main.cpp"), "-o", str(exe)], check=True)
    for S, V, U, radius in cr.SHAPES:
        depth, valid = cr.planted(S, V, U)
        got = _run_rule_program(exe, tmp_path, depth, valid, 1.0, cr.TOL, radius, 2)
        cr.assert_equal_bitwise(got, cr.planted_reference(S, V, U, radius, min_agree=2), "planted %s" % ((S, V, U, radius),))
    S, V, U, radius = cr.SHAPES[0]
    depth, valid = cr.planted(S, V, U)
    got = _run_rule_program(exe, tmp_path, depth, None, 0.5, 0.0, 3, 1)
    cr.assert_equal_bitwise(got, cr.consistency(depth, None, 0.5, 0.0, 3, 1), "no validity plane, slope 0.5, tol 0")
    wild = depth.copy()
    wild[::2, :, ::7] = np.inf
    wild[1::2, :, 3::11] = -np.inf
    wild[:, :, 5::13] = 1e30
    wild[:, :, 6::17] = -1e30
    wild[:, :, 8::19] = -wild[:, :, 8::19]
    got = _run_rule_program(exe, tmp_path, wild, valid, 1.0, cr.TOL, 0, 1)
    cr.assert_equal_bitwise(got, cr.consistency(wild, valid, 1.0, cr.TOL, 0, 1), "infinities and huge values")


def test_plan_and_rule_under_sanitizers(tmp_path):
    exe = tmp_path / "test_plan_consistency"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_plan_consistency.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "consistency plan tests ok" in r.stdout


def test_the_library_exports_the_entries():
    """The entries resolve in the built library, with the binding's argument lists; the ABI version stays."""
    import ctypes as C
    from remotesensingproject_amd import _lib
    names = ("rslf_view_consistency", "rslf_view_consistency_host", "rslf_f2c_run_consistency")
    for name in names:
        assert name in _lib.SYMBOLS
    L = _lib.lib()
    for name in names:
        assert getattr(L, name) is not None
    assert len(L.rslf_view_consistency.argtypes) == len(L.rslf_view_consistency_host.argtypes) == 13
    assert len(L.rslf_f2c_run_consistency.argtypes) == 10
    assert C.sizeof(_lib.RslfViewCounts) == 4 * C.sizeof(C.c_void_p)
    assert _lib.ABI_VERSION == 6 and L.rslf_abi_version() == 6
    # refused before a device is touched: no context
    assert L.rslf_view_consistency(None, None, None, 1, 1, 1, 1.0, 0.1, 0, 0, None, None, None) == -1
    assert L.rslf_f2c_run_consistency(None, None, 0, 0, 0.1, 0, 0, None, None, None) == -1


def test_the_hook_is_a_default():
    from remotesensingproject_amd import depth as rs
    assert rs.Context._DEBUG_DEFAULTS["consistency_order"] == 0


def test_the_forms_without_a_getter_say_so():
    """Checked before anything touches a device: the multi-device and sharded forms and the Python level loop have no
    consistency getter; bad tolerances and counts are refused by name."""
    from remotesensingproject_amd import depth as rs
    from remotesensingproject_amd import sharding
    for cls in (rs.MultiDevice, rs.FineToCoarse, sharding.ShardedDepth2D, sharding.ShardedFineToCoarse):
        with pytest.raises(ValueError, match="get_consistency is not built here"):
            cls.get_consistency(object.__new__(cls))
    for bad in (-0.1, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="not a finite tolerance"):
            rs.view_consistency(None, None, None, 1.0, bad)
    with pytest.raises(ValueError, match="min_agree"):
        rs.view_consistency(None, None, None, 1.0, 0.1, min_agree=-1)
    with pytest.raises(ValueError, match="no grid step"):
        rs.grid_step(0.0, 1.0, 1, "x")
    assert rs.grid_step(-1.0, 3.0, 9, "x") == 0.5
    assert rs.Consistency._fields == cr.NAMES
