"""A kept fine-to-coarse run's validity by cross-view consistency through the C++11 host wrapper (include/rslf_hip.hpp):
tests/cpp/test_host_f2c_consistency.cpp, compiled with g++ against librslf_hip.so and run once on the GPU on the synthetic field
of tests/test_gpu_cpp_consistency.py -- rslfx::FineToCoarse::set_consistency_gate, get_inconsistent and get_gate_counts.  The
program itself checks the refusals, an object built on a MultiContext and that the gate off changes nothing; here the planes
it wrote are held to the yardstick (tests/f2c_consistency_ref.gate_level on the ungated validity, oracle.f2c_fuse on the
gated one), bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import f2c_consistency_ref as fc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, S, U, D = 40, 7, 96, 17
F = np.float32


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd.synth import make_lightfield
    _lib.lib()   # the library the package runs (built first if it is missing)
    so = _lib.library_path()
    tmp = tmp_path_factory.mktemp("host_f2c_consistency")
    raw = make_lightfield(U, V, S, 1, seed=5, dmin=-2.0, dmax=2.0, band=4)[0]
    assert raw.shape == (V, S, U, 1) and raw.dtype == F
    raw.tofile(tmp / "input.f32")
    exe = str(tmp / "test_host_f2c_consistency")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_host_f2c_consistency.cpp"), "-o", exe,
                    "-L", os.path.dirname(so), "-lrslf_hip", "-Wl,-rpath," + os.path.dirname(so)], check=True)
    r = subprocess.run([exe, str(tmp)], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    return tmp


@pytest.mark.parametrize("stem,min_agree,tol,radius", [("gate_default", 2, 4.0 / (D - 1), 0), ("gate_picked", 3, F(0.3), 2)])
def test_gated_run(out, oracle_mod, stem, min_agree, tol, radius):
    shape0, shape1 = (S, V, U), (S, V // 2, U // 2)
    load = lambda name, dt, shape: np.fromfile(out / ("%s_%s" % (stem, name)), dt).reshape(shape)
    depth0, valid0 = load("depth0.f32", F, shape0), load("valid0.u8", np.uint8, shape0)
    depth1, valid1 = load("depth1.f32", F, shape1), load("valid1.u8", np.uint8, shape1)
    ungated = np.fromfile(out / "off_valid0.u8", np.uint8).reshape(shape0)
    want, agree, seen, drop, naive = fc.gate_level(depth0, ungated, 1.0, tol, radius, min_agree)
    n = int(drop.sum())
    print(stem, "dropped", n, "of", int((ungated != 0).sum()), "valid; agree >= min_agree would drop", int(naive.sum()))
    assert 0 < n < int(naive.sum())
    assert np.array_equal(valid0, want)
    assert np.array_equal(load("agree0.i32", np.int32, shape0), agree) and np.array_equal(load("seen0.i32", np.int32, shape0), seen)
    assert int(np.fromfile(out / (stem + "_dropped0.u64"), np.uint64)[0]) == n
    assert (valid1 == 255).all()   # accepted whole: untouched
    # the fusion was fed the gated plane
    fmap, fvalid = load("fused_map.f32", F, shape0), load("fused_valid.u8", np.uint8, shape0)
    for s in range(S):
        m, v = oracle_mod.f2c_fuse([depth0[s], depth1[s]], [valid0[s], valid1[s]])
        assert np.array_equal(fmap[s].view(np.uint32), m.view(np.uint32)) and np.array_equal(fvalid[s], v), s
    off = np.fromfile(out / "off_fused_map.f32", F).reshape(shape0)
    assert (fmap.view(np.uint32) != off.view(np.uint32)).sum() > 0
