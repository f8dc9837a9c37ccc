"""rslfx::Depth1DComputer_pile::set_subgrid of the C++11 host wrapper (include/rslf_hip.hpp): tests/cpp/test_host_subgrid.cpp,
compiled with g++ against librslf_hip.so and run once on the GPU, compares the members with the C-ABI host entry
(rslf_depth1d_pile_run_host_sub, mode on and off) and writes them out for the planted-line field of tests/subgrid_ref.py;
here they are compared with the Python class's planes.  The program itself checks that the object built on a MultiContext
throws std::invalid_argument with the mode on."""
import os
import subprocess

import numpy as np
import pytest

import subgrid_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, S, U, D = 7, 9, 96, 9


def test_cpp_mode_equals_the_c_abi_and_the_python_class(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd import depth as rs
    _lib.lib()
    so = _lib.library_path()
    vol = sr.planted_field(0.37)
    assert vol.shape == (V, S, U, 1)
    vol.tofile(tmp_path / "volume.f32")
    exe = str(tmp_path / "test_host_subgrid")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_host_subgrid.cpp"), "-o", exe,
                    "-L", os.path.dirname(so), "-lrslf_hip", "-Wl,-rpath," + os.path.dirname(so)], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr   # includes: the C-ABI comparison, the MultiContext form throws

    for name, subgrid in (("depth_sub", True), ("depth_grid", False)):
        comp = rs.Depth1DComputer_pile(vol, -1.0, 1.0, D, -1, 1.0, subgrid=subgrid)
        comp.run()
        res = comp.results()
        got = np.fromfile(tmp_path / (name + ".f32"), np.float32).reshape(V, U)
        assert np.array_equal(got.view(np.uint32), res["depth"].view(np.uint32)), name
        assert np.array_equal(np.fromfile(tmp_path / "idx.i32", np.int32).reshape(V, U), res["depth_idx"])
        assert np.array_equal(np.fromfile(tmp_path / "mask.u8", np.uint8).reshape(V, U), res["edge_mask"])
    assert (res["depth_idx"] >= 0).sum() >= 400
