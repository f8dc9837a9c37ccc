"""CV_16U light fields without a GPU: the wrapper's cv::Mat constructors take CV_16U Mats (compiled against the
declaration-only OpenCV mock with CV_16U defined, as every OpenCV defines it), and the numpy restatement of the 16U
pyramid (tests/test_gpu_u16.py) agrees with exact arithmetic."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_u16 import GAUSS7, _reflect, blur_u16_np, halve_u16_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("unit", ["opencv_block.cpp", "opencv_block_u16.cpp"])
def test_opencv_blocks_compile_with_cv_16u(unit):
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-DCV_16U=2", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "tests", "cpp", "opencv_mock"), os.path.join(ROOT, "tests", "cpp", unit)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_wrapper_without_cv_16u_still_refuses_other_depths():
    """Without CV_16U the 16U branch is compiled out; the message names what is accepted."""
    with open(os.path.join(ROOT, "include", "rslf_hip.hpp")) as f:
        src = f.read()
    assert "#ifdef CV_16U" in src
    assert "EPIs must be CV_8U, CV_16U or CV_32F" in src and "EPIs must be CV_8U or CV_32F" in src


def _exact_blur(x: np.ndarray) -> np.ndarray:
    """The 7x7 blur in exact arithmetic: the taps are k/64 with small k, ushort inputs, so every product and sum is a
    dyadic rational that float64 holds exactly."""
    x = x.astype(np.float64)
    g = GAUSS7.astype(np.float64)
    V, S, U, C_ = x.shape
    u, y = np.arange(U), np.arange(V)
    t = sum(g[j] * x[:, :, _reflect(u + j - 3, U), :] for j in range(7))
    return sum(g[j] * t[_reflect(y + j - 3, V)] for j in range(7))


def test_restatement_agrees_with_exact_arithmetic():
    rng = np.random.default_rng(7)
    for V, U, C_ in ((23, 35, 1), (22, 30, 3), (16, 13, 1)):
        x = rng.integers(0, 4096, size=(V, 2, U, C_)).astype(np.float32)
        exact = _exact_blur(x)
        assert np.array_equal(exact, np.round(exact * 4096) / 4096)   # dyadic, 12 fractional bits: held exactly
        got = blur_u16_np(x)
        # away from a half-integer the float32 sums round to the exact value's nearest integer
        frac = exact - np.floor(exact)
        clear = np.abs(frac - 0.5) > 1e-3
        assert clear.mean() > 0.9
        assert np.array_equal(got[clear], np.rint(exact[clear]).astype(np.int64))
        # the halving on the rounded levels: integer (sum + 2) >> 2 where the 2x2 block is whole
        h = halve_u16_np(got)
        V2, U2 = h.shape[0], h.shape[2]
        for yy in range(min(V2, V // 2)):
            for xx in range(min(U2, U // 2)):
                blk = got[2 * yy:2 * yy + 2, :, 2 * xx:2 * xx + 2, :].sum(axis=(0, 2))
                assert np.array_equal(h[yy, :, xx, :], (blk + 2) // 4)


def test_restatement_impulse_ties_round_to_even():
    """An impulse of 512: blurred values 512 * k_i * k_j / 1024 -- 0.5 at the corners (-> 0), 3.5 (-> 4), 4.5 (-> 4),
    1.75 (-> 2), ...: exact in float32, the ties rounded to even as cvRound does."""
    x = np.zeros((15, 1, 15, 1), np.float32)
    x[7, 0, 7, 0] = 512
    b = blur_u16_np(x)[:, 0, :, 0]
    exact = _exact_blur(x)[:, 0, :, 0]
    assert exact[4, 4] == 0.5 and b[4, 4] == 0
    assert exact[4, 6] == 3.5 and b[4, 6] == 4
    assert exact[4, 7] == 4.5 and b[4, 7] == 4
    assert exact[4, 5] == 1.75 and b[4, 5] == 2
    assert np.array_equal(b, np.rint(exact).astype(np.int64))   # exact in float32, so every value is the exact one


def test_restatement_odd_border_and_saturation():
    # a 3 x 3 level halves to cvRound(1.5) = 2 x 2: the last row / column average what exists
    b = np.arange(9, dtype=np.int64).reshape(3, 1, 3, 1) * 7
    h = halve_u16_np(b)
    assert h.shape == (2, 1, 2, 1)
    assert h[0, 0, 0, 0] == (0 + 7 + 21 + 28 + 2) >> 2
    assert h[0, 0, 1, 0] == np.rint(np.float32(14 + 35) / np.float32(2))
    assert h[1, 0, 1, 0] == 56
    # full-scale values stay within ushort
    x = np.full((12, 1, 12, 1), 65535, np.float32)
    assert blur_u16_np(x).max() == 65535 and halve_u16_np(blur_u16_np(x)).max() == 65535
