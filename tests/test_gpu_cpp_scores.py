"""rslfx::Depth1DComputer_pile::get_scores of the C++11 host wrapper (include/rslf_hip.hpp): tests/cpp/test_host_scores.cpp,
compiled with g++ against librslf_hip.so and run once on the GPU, writes the getter's rows for the RGB 17-view case of
tests/test_gpu_scores.py; here they are compared with the Python getter's tensor.  The program itself checks that the
object built on a MultiContext throws std::invalid_argument."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, S, U, D, C_ = 3, 17, 150, 24, 3


def test_cpp_getter_equals_the_python_getter(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd import depth as rs
    _lib.lib()
    so = _lib.library_path()
    vol = np.random.default_rng(0).uniform(0.0, 1.0, size=(V, S, U, C_)).astype(np.float32)
    vol[:, :, 40:52] = 0.01
    vol.tofile(tmp_path / "volume.f32")
    exe = str(tmp_path / "test_host_scores")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_host_scores.cpp"), "-o", exe,
                    "-L", os.path.dirname(so), "-lrslf_hip", "-Wl,-rpath," + os.path.dirname(so)], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr   # includes: the refusals, the MultiContext form throws

    comp = rs.Depth1DComputer_pile(vol, -2.0, 5.0, D, -1, 1.0)
    comp.run()
    want = comp.get_scores().cpu().numpy()
    res = comp.results()
    mask = np.fromfile(tmp_path / "mask.u8", np.uint8).reshape(V, U)
    assert np.array_equal(mask, res["edge_mask"]) and (mask != 0).sum() >= 100
    assert np.array_equal(np.fromfile(tmp_path / "idx.i32", np.int32).reshape(V, U), res["depth_idx"])
    got = np.fromfile(tmp_path / "scores.f32", np.float32).reshape(V, U, D)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got[mask == 0] == 0).all() and (got[mask != 0].max(axis=1) > 0).all()
    assert np.array_equal(np.argmax(got[mask != 0], axis=1), res["depth_idx"][mask != 0])
    row1 = np.fromfile(tmp_path / "scores_row1.f32", np.float32).reshape(1, U, D)
    assert np.array_equal(row1.view(np.uint32), want[1:2].view(np.uint32))
