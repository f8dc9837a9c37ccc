"""rslfx::Depth2DComputer::set_subgrid and rslfx::FineToCoarse::set_subgrid of the C++11 host wrapper (include/rslf_hip.hpp):
tests/cpp/test_host_sweep_subgrid.cpp, compiled with g++ against librslf_hip.so and run once on the GPU, runs both classes
with the mode off and on -- the pyramid also as a kept run -- and writes the planes out; here they are compared with the
Python objects' planes, bit for bit.  The program itself checks that objects built on a MultiContext throw
std::invalid_argument with the mode on."""
import os
import subprocess

import numpy as np
import pytest

import f2c_keep_ref as kr
import sweep_subgrid_ref as ssr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _same(got, want, label):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    g = got.view(np.uint32) if got.dtype == F else got
    w = want.view(np.uint32) if want.dtype == F else want
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert bad.size == 0, (label, bad.size, np.unravel_index(bad[0], want.shape))


def test_cpp_setters_equal_the_python_objects(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd import depth as rs
    _lib.lib()
    so = _lib.library_path()
    P = ssr.PLANTED
    V, S, U, D = P["V"], P["S"], P["U"], P["D"]
    sweep = ssr.planted_field(0.37)
    sweep.tofile(tmp_path / "sweep.f32")
    pyramid = kr.make_field("A").astype(F)
    Vp, Sp, Up = pyramid.shape[:3]
    assert (Vp, Sp, Up, pyramid.shape[3]) == (44, 5, 64, 1) and sweep.shape == (6, 5, 80, 1)
    pyramid.tofile(tmp_path / "pyramid.f32")
    exe = str(tmp_path / "test_host_sweep_subgrid")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_host_sweep_subgrid.cpp"), "-o", exe,
                    "-L", os.path.dirname(so), "-lrslf_hip", "-Wl,-rpath," + os.path.dirname(so)], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr   # includes: the mode changes the planes, the MultiContext forms throw

    rd = lambda name, dt, shape: np.fromfile(tmp_path / name, dt).reshape(shape)
    for name, subgrid in (("sweep_depth_grid.f32", False), ("sweep_depth_sub.f32", True)):
        comp = rs.Depth2DComputer(sweep, P["lo"], P["hi"], D, epi_scale_factor=1.0, subgrid=subgrid)
        comp.run()
        res = comp.results()
        _same(rd(name, F, (S, V, U)), res["depth"], name)
    _same(rd("sweep_Ce.f32", F, (S, V, U)), res["edge_confidence"], "C_e")
    _same(rd("sweep_mask.u8", np.uint8, (S, V, U)), res["edge_mask"], "mask")
    _same(rd("sweep_Cd.f32", F, (S, V, U)), res["disp_confidence"], "C_d")
    _same(rd("sweep_rbar.f32", F, (S, V, U, 1)), res["rbar"], "rbar")

    epis = list(pyramid[..., 0])
    out = rs.fine_to_coarse_run_host(epis, -1.0, 1.0, D, want_levels=True, subgrid=True)
    _same(rd("f2c_map.f32", F, (Sp, Vp, Up)), out["out_map"], "fused map")
    _same(rd("f2c_valid.u8", np.uint8, (Sp, Vp, Up)), out["out_valid"], "fused validity")
    for l, lv in enumerate(out["levels"]):
        _same(rd("f2c_depth_%d.f32" % l, F, lv["depth"].shape), lv["depth"], "level %d" % l)
    grid = rs.fine_to_coarse_run_host(epis, -1.0, 1.0, D)
    _same(rd("f2c_map_grid.f32", F, (Sp, Vp, Up)), grid["out_map"], "the grid pyramid")
