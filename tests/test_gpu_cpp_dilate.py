"""The dilation along u through the C++11 host wrapper (include/rslf_hip.hpp): tests/cpp/test_host_dilate.cpp, compiled with
g++ against librslf_hip.so and run once on the GPU.  The Python classes compute the planes of a pile run and of a sweep with
u_dilation = 2 and write them to a temporary directory; the program runs rslfx::Depth1DComputer_pile and
rslfx::Depth2DComputer after set_u_dilation(2, RSLF_DILATE_CUBIC) and holds every plane to those bytes, checks the undilated
getters, and the two forms that throw (an object built on a MultiContext, FineToCoarse)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, S, U, D = 5, 7, 80, 12
F = np.float32


def test_the_cpp_classes_in_the_dilated_frame(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd import depth as rs
    from remotesensingproject_amd.synth import make_lightfield
    _lib.lib()   # the library the package runs (built first if it is missing)
    so = _lib.library_path()
    raw = make_lightfield(U, V, S, 1, seed=42, dmin=-1.0, dmax=1.0, band=2)[0]
    assert raw.shape == (V, S, U, 1) and raw.dtype == F
    raw.tofile(tmp_path / "input.f32")
    pile = rs.Depth1DComputer_pile(raw, -1.0, 1.0, D, epi_scale_factor=1.0, u_dilation=2)
    pile.run()
    r = pile.results()
    for k, ext in (("depth", "f32"), ("edge_mask", "u8"), ("edge_confidence", "f32"), ("depth_idx", "i32"), ("score", "f32"), ("rbar", "f32")):
        r[k].tofile(tmp_path / ("pile_%s.%s" % (k, ext)))
    sweep = rs.Depth2DComputer(raw, -1.0, 1.0, D, epi_scale_factor=1.0, u_dilation=2)
    sweep.run()
    r = sweep.results()
    for k, ext in (("depth", "f32"), ("edge_mask", "u8"), ("edge_confidence", "f32"), ("rbar", "f32")):
        r[k].tofile(tmp_path / ("sweep_%s.%s" % (k, ext)))
    sweep.get_valid_depths_mask_s_v_u().cpu().numpy().tofile(tmp_path / "sweep_valid.u8")
    agree = sweep.get_consistency().agree.cpu().numpy()
    assert agree.dtype == np.int32 and agree.shape == (S, V, 2 * (U - 1) + 1) and agree.any()
    agree.tofile(tmp_path / "sweep_agree.i32")
    exe = str(tmp_path / "test_host_dilate")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_host_dilate.cpp"), "-o", exe,
                    "-L", os.path.dirname(so), "-lrslf_hip", "-Wl,-rpath," + os.path.dirname(so)], check=True)
    run = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "host dilate: ok" in run.stdout
