"""The cross-view consistency check through the C++11 host wrapper (include/rslf_hip.hpp):
tests/cpp/test_host_consistency.cpp, compiled with g++ against librslf_hip.so and run once on the GPU on a synthetic field --
rslfx::Depth2DComputer::get_consistency and the getter of a kept rslfx::FineToCoarse.  The program itself checks the refusals,
an object built on a MultiContext and that its planes stay as they were; here the planes the getters returned are held to the
yardstick tests/consistency_ref.py applied to the planes the program wrote beside them, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import consistency_ref as cr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, S, U, D = 40, 7, 96, 17
F = np.float32
EXT = dict(seen=("i32", np.int32), agree=("i32", np.int32), above=("i32", np.int32), below=("i32", np.int32), fused=("f32", F),
           valid=("u8", np.uint8))


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd.synth import make_lightfield
    _lib.lib()   # the library the package runs (built first if it is missing)
    so = _lib.library_path()
    tmp = tmp_path_factory.mktemp("host_consistency")
    raw = make_lightfield(U, V, S, 1, seed=5, dmin=-2.0, dmax=2.0, band=4)[0]
    assert raw.shape == (V, S, U, 1) and raw.dtype == F
    raw.tofile(tmp / "input.f32")
    exe = str(tmp / "test_host_consistency")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_host_consistency.cpp"), "-o", exe,
                    "-L", os.path.dirname(so), "-lrslf_hip", "-Wl,-rpath," + os.path.dirname(so)], check=True)
    r = subprocess.run([exe, str(tmp)], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    return tmp


def _planes(out, stem, shape):
    return {k: np.fromfile(out / ("%s_%s.%s" % (stem, k, ext)), dt).reshape(shape) for k, (ext, dt) in EXT.items()}


def test_depth2d_computer(out):
    shape = (S, V, U)
    depth, mask = np.fromfile(out / "sweep_depth.f32", F).reshape(shape), np.fromfile(out / "sweep_mask.u8", np.uint8).reshape(shape)
    own = np.fromfile(out / "sweep_own_mask.u8", np.uint8).reshape(shape)
    want = cr.consistency(depth, mask, 1.0, 4.0 / (D - 1), 0, 0)
    cr.assert_equal_bitwise(_planes(out, "sweep_plain", shape), want, "Depth2DComputer::get_consistency()")
    assert (want["agree"] > 0).any()
    cr.assert_equal_bitwise(_planes(out, "sweep_picked", shape), cr.consistency(depth, own, 1.0, F(0.3), 2, 3),
                            "Depth2DComputer::get_consistency(tol, radius, min_agree, mask)")


def test_kept_fine_to_coarse(out):
    shape = (S, V, U)
    fmap, fvalid = np.fromfile(out / "f2c_fused_map.f32", F).reshape(shape), np.fromfile(out / "f2c_fused_valid.u8", np.uint8).reshape(shape)
    want = cr.consistency(fmap, fvalid, 1.0, 4.0 / (D - 1), 0, 0)
    cr.assert_equal_bitwise(_planes(out, "f2c_fused", shape), want, "FineToCoarse::get_consistency()")
    assert (want["agree"] > 0).any()
    shape1 = (S, V // 2, U // 2)
    d1, v1 = np.fromfile(out / "f2c_depth1.f32", F).reshape(shape1), np.fromfile(out / "f2c_valid1.u8", np.uint8).reshape(shape1)
    cr.assert_equal_bitwise(_planes(out, "f2c_level1", shape1), cr.consistency(d1, v1, F(0.5), F(0.2), 2, 1),
                            "FineToCoarse::get_consistency(1, false, ...): slope U_1 / U_0")
