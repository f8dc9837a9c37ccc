"""The renderers without a GPU: known answers, worked by hand here, for the numpy restatement of the reference's picture
getters (tests/render_ref.py, the yardstick of tests/test_gpu_render.py), and the renderers' host-side rules
(rslf_plan.hpp: radix select, index rules, level rounding) under AddressSanitizer + UBSan."""
import os
import subprocess

import numpy as np
import pytest

import render_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remotesensingproject_amd", "csrc")
GREY = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)   # level i -> (i, i, i)


def test_plan_render_unit_tests_under_sanitizers(tmp_path):
    exe = tmp_path / "test_plan_render"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_plan_render.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "render plan tests ok" in r.stdout


def test_quantile_fit_known_answers():
    # 4 x 5: N = 20, floor(0.4) = 0 and floor(19.6) = 19 -- the smallest and the largest element
    img = np.array([[7, 3, 19, 0, 11], [5, 13, 1, 17, 9], [2, 18, 6, 14, 10], [16, 4, 12, 8, -15]], np.float32)
    assert rr.fit(img, rr.QUANTILE) == (-15.0, 19.0)
    # N = 50: floor(1.0) = 1 and floor(49.0) = 49 -- the second smallest and the largest
    img = np.arange(50, dtype=np.float32)[::-1].reshape(5, 10) * 2 - 30   # -30, -28, ..., 68
    assert rr.fit(img, rr.QUANTILE) == (-28.0, 68.0)
    # a masked pixel counts as 0: {0, 0, 5, 6} for N = 4 -> indices 0 and 3
    assert rr.fit(np.array([[3, -9], [5, 6]], np.float32), rr.QUANTILE, np.array([[0, 0], [255, 1]], np.uint8)) == (0.0, 6.0)


def test_minmax_and_meanstd_fit_known_answers():
    img = np.array([[1, 3], [1, 3]], np.float32)   # mean 2, std 1
    assert rr.fit(img, rr.MINMAX) == (1.0, 3.0)
    assert rr.fit(img, rr.MEANSTD) == (1.0, 3.0)   # mean + 12 std = 14 is capped by the true max
    img = np.array([[0] * 199 + [100]], np.float32)   # mean 0.5, E[x^2] = 50, std = sqrt(49.75)
    lo, hi = rr.fit(img, rr.MEANSTD)
    assert lo == 0.0 and hi == 0.5 + 12 * np.sqrt(49.75) and hi < 100.0


def test_levels_round_to_nearest_even_both_ways():
    # SHIFT over [0, 510]: scale 0.5 exactly, so x = 1, 3, 5 give 0.5, 1.5, 2.5 -> 0, 2, 2
    x = np.array([[0, 1, 3, 5, 509, 510]], np.float32)
    assert rr.levels(x, 0.0, 510.0, rr.SHIFT).tolist() == [[0, 0, 2, 2, 254, 255]]
    # AFFINE over [2, 512]: alpha 0.5, beta -1: x = 3, 5, 7 give 0.5, 1.5, 2.5
    x = np.array([[2, 3, 5, 7, 512, 1000, -8]], np.float32)
    assert rr.levels(x, 2.0, 512.0, rr.AFFINE).tolist() == [[0, 0, 2, 2, 255, 255, 0]]


def test_constant_plane_renders_the_first_table_entry():
    lut = GREY.copy()
    lut[0] = (9, 8, 7)
    img = np.full((2, 3), 4.25, np.float32)
    for formula in (rr.SHIFT, rr.AFFINE):   # 255 / 0 = inf; 0 * inf (or inf - inf) = NaN -> INT_MIN -> 0
        assert (rr.levels(img, 4.25, 4.25, formula) == 0).all()
    out = rr.disparity_map(img, np.full((2, 3), 255, np.uint8), lut)
    assert out.shape == (2, 3, 3) and (out == np.array([9, 8, 7], np.uint8)).all()


def test_mask_modes_differ_where_level_of_zero_is_not_zero():
    img = np.array([[-1.0, 1.0, 0.5]], np.float32)
    valid = np.array([[255, 255, 0]], np.uint8)
    # over [-1, 1] AFFINE: alpha 127.5, beta 127.5 -> level(0) = rint(127.5) = 128
    black = rr.render(img, -1.0, 1.0, rr.AFFINE, GREY, valid, rr.BLACK)
    zero = rr.render(img, -1.0, 1.0, rr.AFFINE, GREY, valid, rr.ZERO_VALUE)
    assert black[0, :, 0].tolist() == [0, 255, 0] and zero[0, :, 0].tolist() == [0, 255, 128]


def test_shadow_cut_uses_the_reference_norms():
    img = np.zeros((1, 3), np.float32)
    lut = np.full((256, 3), 200, np.uint8)
    thr = np.float32(0.05 * 1.73205080757)
    rad1 = np.array([[[0.04], [0.05], [0.06]]], np.float32)   # norm = |x| * sqrt(3): 0.05 sits on the level, not below it
    assert rr.render(img, 0.0, 1.0, rr.SHIFT, lut, radiance=rad1, shadow_level=thr)[0, :, 0].tolist() == [0, 200, 200]
    rad3 = np.array([[[0.03, 0.04, 0.0], [0.06, 0.06, 0.02], [0.0, 0.0, 0.0]]], np.float32)   # norms 0.05, 0.087.., 0
    assert rr.render(img, 0.0, 1.0, rr.SHIFT, lut, radiance=rad3, shadow_level=thr)[0, :, 0].tolist() == [0, 200, 0]


def test_z_buffer_row_with_a_tie_and_lines_leaving_on_both_sides():
    """U = 6, S = 3, s_hat = 1.  Three sources: u = 0 and u = 1 with depth 1 (equal depths), u = 4 with depth 2; the rest
    unmasked.  Row s = 0 (s_hat - s = 1): targets u + d -> 1, 2 and 6 (off the right end).  Row s = 1: every source
    paints itself.  Row s = 2 (s_hat - s = -1): targets -1 (off the left end), 0 and 2.
    The scanline's depths are (1, 1, 0, -2, 2, 0): min -2 and max 2 over ALL of them, masked or not, so depth 1 ->
    rint(3 * 63.75) = 191 and depth 2 -> 255."""
    depth = np.array([1, 1, 0, -2, 2, 0], np.float32)
    mask = np.array([255, 255, 0, 0, 255, 0], np.uint8)
    out = rr.epi_lines(depth, mask, 3, 1, GREY)[..., 0]
    assert out.tolist() == [[0, 191, 191, 0, 0, 0], [191, 191, 0, 0, 255, 0], [191, 0, 255, 0, 0, 0]]
    # the single-EPI class never paints column 0
    out = rr.epi_lines(depth, mask, 3, 1, GREY, lowest_column=1)[..., 0]
    assert out.tolist() == [[0, 191, 191, 0, 0, 0], [0, 191, 0, 0, 255, 0], [0, 0, 255, 0, 0, 0]]
    # two sources on one target: u = 0 (depth 1) and u = 1 (depth 0.4, round(0.4) = 0) both reach column 1 of row s = 0;
    # the greater depth keeps it whatever the order of the sources.  (Of EQUAL depths the first u keeps the target --
    # the strict `<` -- but equal depths have equal colours, so the picture cannot tell.)
    depth = np.array([1.0, 0.4, 1.0, 0.0], np.float32)
    mask = np.array([255, 255, 255, 0], np.uint8)
    out = rr.epi_lines(depth, mask, 2, 1, GREY)
    assert out[0, 1, 0] == 255 and out[0, 3, 0] == 255 and out[1, 1, 0] == 102
    # std::round sends halves away from zero on both sides: depth 0.5 reaches u + 1 in row 0 and u - 1 in row 2
    depth = np.array([0.5, 0.0, 0.5], np.float32)
    mask = np.array([255, 0, 255], np.uint8)
    out = rr.epi_lines(depth, mask, 3, 1, GREY)[..., 0]
    assert out.tolist() == [[0, 255, 0], [255, 0, 255], [0, 255, 0]]


def test_index_rules_of_the_restatement():
    assert rr.cround(0.5) == 1 and rr.cround(1.5) == 2 and rr.cround(2.5) == 3 and rr.cround(-0.5) == -1 and round(2.5) == 2
    assert rr.centre_index(2) == 1 and rr.centre_index(5) == 3 and rr.centre_index(101) == 51
    with pytest.raises(ValueError):
        rr.centre_index(1)
    assert rr.scaled_row(12, 12, 24) == 6 and rr.scaled_row(22, 12, 24) == 11
    with pytest.raises(ValueError):
        rr.scaled_row(23, 12, 24)
    assert rr.scaled_row(0, 1, 1) == 0
    with pytest.raises(ValueError):   # V_0 = 1: the default scanline is round(0.5) = 1
        rr.scaled_row(rr.cround(1 / 2.0), 1, 1)


def test_restatement_does_not_import_the_library():
    src = open(os.path.join(ROOT, "tests", "render_ref.py")).read()
    assert "remotesensingproject_amd" not in src.split('"""', 2)[2] and "import torch" not in src and "oracle" not in src


def test_render_symbols_are_declared_bound_and_guarded():
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    names = ["rslf_render_fit", "rslf_render_planes", "rslf_render_epi_lines", "rslf_render_centre_index", "rslf_render_scaled_row"]
    hdr = open(os.path.join(ROOT, "include", "rslf_hip.h")).read()
    src = open(os.path.join(CSRC, "rslf_render.hip")).read()
    for n in names:
        assert n in _lib.SYMBOLS and hasattr(L, n) and ("int %s(" % n) in hdr and ('extern "C" int %s(' % n) in src
    assert L.rslf_abi_version() == 6
    # the index rules need no device: they refuse where the reference's index runs off the end, and say why
    import ctypes as C
    out = C.c_int(-7)
    assert L.rslf_render_centre_index(5, C.byref(out)) == 0 and out.value == 3
    assert L.rslf_render_centre_index(1, C.byref(out)) == -1 and b"round" in L.rslf_last_error()
    assert L.rslf_render_scaled_row(12, 12, 24, C.byref(out)) == 0 and out.value == 6
    assert L.rslf_render_scaled_row(23, 12, 24, C.byref(out)) == -1
    # NULL handles are rejected, not dereferenced
    lo, hi = C.c_double(), C.c_double()
    assert L.rslf_render_fit(None, None, 1, 1, 1, None, 0, C.byref(lo), C.byref(hi)) == -1
    assert L.rslf_render_planes(None, None, 1, 0, 1, 1, 1, 0.0, 1.0, 0, None, None, 0, None, 0, 0, 0.0, None) == -1
    assert L.rslf_render_epi_lines(None, None, None, 1, 1, 1, 0, 0, 1, None, None) == -1


def test_colormap_jet_is_a_table():
    from remotesensingproject_amd import depth as rs
    t = rs.colormap_jet()
    assert t.shape == (256, 3) and t.dtype == np.uint8
    assert "unpinned" in rs.colormap_jet.__doc__
    assert t[0, 0] > 0 and t[0, 2] == 0 and t[255, 2] > 0 and t[255, 0] == 0   # blue end to red end, BGR
