"""The view warp through the C++11 host wrapper (include/rslf_hip.hpp): tests/cpp/test_host_view_warp.cpp, compiled with g++
against librslf_hip.so and run once on the GPU on a synthetic field -- rslfx::Depth2DComputer::get_warped_view /
get_view_prediction and the getters of a kept rslfx::FineToCoarse.  The program itself checks the refusals, an object built on
a MultiContext and that its planes stay as they were; here the planes the getters returned are held to the yardstick
tests/view_warp_ref.py applied to the planes the program wrote beside them, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import view_warp_ref as wr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, S, U, D = 40, 7, 96, 17
F = np.float32
WARP = dict(hit=("u8", np.uint8), depth=("f32", F), src_view=("i32", np.int32), src_col=("i32", np.int32), count=("i32", np.int32),
            colour=("f32", F))
PRED = dict(err=("f32", F), hit=("u8", np.uint8), row_err=("f64", np.float64), row_hits=("i32", np.int32))


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd.synth import make_lightfield
    _lib.lib()   # the library the package runs (built first if it is missing)
    so = _lib.library_path()
    tmp = tmp_path_factory.mktemp("host_view_warp")
    raw = make_lightfield(U, V, S, 1, seed=5, dmin=-2.0, dmax=2.0, band=4)[0]
    assert raw.shape == (V, S, U, 1) and raw.dtype == F
    raw.tofile(tmp / "input.f32")
    exe = str(tmp / "test_host_view_warp")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_host_view_warp.cpp"), "-o", exe,
                    "-L", os.path.dirname(so), "-lrslf_hip", "-Wl,-rpath," + os.path.dirname(so)], check=True)
    r = subprocess.run([exe, str(tmp)], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    return tmp, raw   # (epi_scale_factor 1: the slab holds the field's own values)


def _warp(out, stem, shape, colour=True):
    got = {}
    for k, (ext, dt) in WARP.items():
        a = np.fromfile(out / ("%s_%s.%s" % (stem, k, ext)), dt)
        if k == "colour":
            assert colour or a.size == 0
            if colour:
                got[k] = a.reshape(shape + (1,))
        else:
            got[k] = a.reshape(shape)
    return got


def _pred(out, stem, T, Vp, Up, want, label):
    got = {k: np.fromfile(out / ("%s_%s.%s" % (stem, k, ext)), dt).reshape((T, Vp) if k.startswith("row_") else (T, Vp, Up))
           for k, (ext, dt) in PRED.items()}
    wr.assert_equal(got, want, label, names=tuple(PRED))
    hits = want["row_hits"].astype(np.int64).sum(axis=1)
    assert hits.all()
    mae, cov = np.fromfile(out / (stem + "_mean_abs_error.f64")), np.fromfile(out / (stem + "_coverage.f64"))
    assert np.allclose(mae, want["row_err"].sum(axis=1) / hits, rtol=1e-9, atol=0) and np.array_equal(cov, hits / float(Vp * Up)), label


def test_depth2d_computer(out):
    out, raw = out
    shape = (S, V, U)
    depth, mask = np.fromfile(out / "sweep_depth.f32", F).reshape(shape), np.fromfile(out / "sweep_mask.u8", np.uint8).reshape(shape)
    own = np.fromfile(out / "sweep_own_mask.u8", np.uint8).reshape(shape)
    want = wr.warp(depth, mask, 1.0, [3.0], [3], volume=raw)
    wr.assert_equal(_warp(out, "sweep_centre", (1, V, U)), want, "Depth2DComputer::get_warped_view(3, 3)", names=tuple(WARP))
    assert (want["count"] >= 2).any()
    wr.assert_equal(_warp(out, "sweep_between", (1, V, U), colour=False), wr.warp(depth, own, 1.0, [2.5], None, 2, -1),
                    "Depth2DComputer::get_warped_view(2.5, -1, 2, -1, mask, false)", names=tuple(WARP)[:5])
    loo = wr.leave_one_out(S)
    _pred(out, "sweep_all", S, V, U, wr.warp(depth, mask, 1.0, *loo, volume=raw, want_err=True), "Depth2DComputer::get_view_prediction()")
    _pred(out, "sweep_picked", 2, V, U, wr.warp(depth, own, 1.0, (1.0, 5.0), (1, 5), 3, volume=raw, want_err=True),
          "Depth2DComputer::get_view_prediction({1, 5}, 3, 1, mask)")


def test_kept_fine_to_coarse(out):
    out, raw = out
    shape = (S, V, U)
    fmap, fvalid = np.fromfile(out / "f2c_fused_map.f32", F).reshape(shape), np.fromfile(out / "f2c_fused_valid.u8", np.uint8).reshape(shape)
    want = wr.warp(fmap, fvalid, 1.0, [3.0], [3], volume=raw)
    wr.assert_equal(_warp(out, "f2c_fused", (1, V, U)), want, "FineToCoarse::get_warped_view(3, 0, true, 3)", names=tuple(WARP))
    assert (want["count"] >= 2).any()
    loo = wr.leave_one_out(S)
    _pred(out, "f2c_pred", S, V, U, wr.warp(fmap, fvalid, 1.0, *loo, volume=raw, want_err=True), "FineToCoarse::get_view_prediction()")
    # level 1: the geometry against the yardstick with the slope U_1 / U_0 (its colour comes from the level's own volume, which
    # tests/test_gpu_view_warp.py reads back)
    shape1 = (S, V // 2, U // 2)
    d1, v1 = np.fromfile(out / "f2c_depth1.f32", F).reshape(shape1), np.fromfile(out / "f2c_valid1.u8", np.uint8).reshape(shape1)
    got = _warp(out, "f2c_level1", (1,) + shape1[1:])
    wr.assert_equal(got, wr.warp(d1, v1, F(0.5), [3.5], None, 2), "FineToCoarse::get_warped_view(3.5, 1, false, -1, 2)", names=tuple(WARP)[:5])
    assert got["colour"].any() and not got["colour"][got["hit"] == 0].any()
