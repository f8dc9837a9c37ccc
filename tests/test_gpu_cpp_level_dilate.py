"""The level dilation of the pyramid through the C++11 host wrapper (include/rslf_hip.hpp): tests/cpp/test_host_level_dilate.cpp,
compiled with g++ against librslf_hip.so and run once on the GPU.  fine_to_coarse_run_host(..., keep=True, level_dilation=2)
-- rslf_f2c_run_host_dl -- computes the planes of case A's three-level pyramid and writes them to a temporary directory; the
program runs rslfx::FineToCoarse<1> after set_level_dilation(2, RSLF_DILATE_CUBIC) -- kept, with its levels out, and plain --
and holds every plane to those bytes, and checks that it throws on a MultiContext and that set_u_dilation still throws."""
import os
import subprocess

import numpy as np
import pytest

import f2c_keep_ref as kr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_the_cpp_pyramid_with_the_level_dilation(tmp_path):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd import depth as rs
    _lib.lib()   # the library the package runs (built first if it is missing)
    so = _lib.library_path()
    raw = kr.make_field("A")[..., 0]
    V, S, U = raw.shape
    assert (V, S, U) == (44, 5, 64) and raw.dtype == F
    raw.tofile(tmp_path / "input.f32")
    run = rs.fine_to_coarse_run_host([raw[v] for v in range(V)], -1.0, 1.0, 9, keep=True, level_dilation=2,
                                     level_dilation_kind=rs.DILATE_CUBIC)
    assert run.n_levels == 3 and run.dims == [(44, 64), (22, 32), (11, 16)] and run.level_dilation == (2, rs.DILATE_CUBIC)
    for l in range(3):
        for name, ext in (("depth", "f32"), ("valid", "u8"), ("Cd", "f32")):
            run.plane(l, name).cpu().numpy().tofile(tmp_path / ("%s_%d.%s" % (name, l, ext)))
    run.plane(0, "fused_map").cpu().numpy().tofile(tmp_path / "fused_map.f32")
    fused_valid = run.plane(0, "fused_valid").cpu().numpy()
    assert fused_valid.any()
    fused_valid.tofile(tmp_path / "fused_valid.u8")
    exe = str(tmp_path / "test_host_level_dilate")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_host_level_dilate.cpp"), "-o", exe,
                    "-L", os.path.dirname(so), "-lrslf_hip", "-Wl,-rpath," + os.path.dirname(so)], check=True)
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    print(out.stdout + out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "host level dilate: ok" in out.stdout
