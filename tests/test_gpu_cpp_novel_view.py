"""The novel view through the C++11 host wrapper (include/rslf_hip.hpp): tests/cpp/test_host_novel_view.cpp, compiled with g++
against librslf_hip.so and run once on the GPU on a synthetic field -- rslfx::Depth2DComputer::get_novel_view and the getter of
a kept rslfx::FineToCoarse.  The program itself checks the refusals, an object built on a MultiContext and that its planes stay
as they were; here the planes the getters returned are held to the yardstick tests/novel_view_ref.py applied to the planes the
program wrote beside them, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import novel_view_ref as nr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, S, U, D = 40, 7, 96, 17
F = np.float32
STEP = 4.0 / (D - 1)
PLANES = dict(colour=("f32", F), depth=("f32", F), fill=("u8", np.uint8), n_src=("i32", np.int32))


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd.synth import make_lightfield
    _lib.lib()   # the library the package runs (built first if it is missing)
    so = _lib.library_path()
    tmp = tmp_path_factory.mktemp("host_novel_view")
    raw = make_lightfield(U, V, S, 1, seed=5, dmin=-2.0, dmax=2.0, band=4)[0]
    assert raw.shape == (V, S, U, 1) and raw.dtype == F
    raw.tofile(tmp / "input.f32")
    exe = str(tmp / "test_host_novel_view")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_host_novel_view.cpp"), "-o", exe,
                    "-L", os.path.dirname(so), "-lrslf_hip", "-Wl,-rpath," + os.path.dirname(so)], check=True)
    r = subprocess.run([exe, str(tmp)], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    return tmp, raw   # (epi_scale_factor 1: the slab holds the field's own values)


def _novel(out, stem, shape, colour=True):
    got = {}
    for k, (ext, dt) in PLANES.items():
        a = np.fromfile(out / ("%s_%s.%s" % (stem, k, ext)), dt)
        if k == "colour":
            assert colour or a.size == 0
            if colour:
                got[k] = a.reshape(shape + (1,))
        else:
            got[k] = a.reshape(shape)
    return got


def test_depth2d_computer(out):
    out, raw = out
    shape = (S, V, U)
    depth, mask = np.fromfile(out / "sweep_depth.f32", F).reshape(shape), np.fromfile(out / "sweep_mask.u8", np.uint8).reshape(shape)
    own = np.fromfile(out / "sweep_own_mask.u8", np.uint8).reshape(shape)
    want = nr.novel(depth, mask, 1.0, [3.0], [3], tol=STEP, volume=raw)
    nr.assert_equal(_novel(out, "sweep_centre", (1, V, U)), want, "Depth2DComputer::get_novel_view(3, 3)", names=tuple(PLANES))
    assert (want["n_src"] >= 2).any()
    nr.assert_equal(_novel(out, "sweep_between", (1, V, U), colour=False), nr.novel(depth, own, 1.0, [2.5], None, 2, -1, 2, 2, 0.5),
                    "Depth2DComputer::get_novel_view(2.5, -1, {2, -1, 2, 2, 0.5}, mask, false)", names=tuple(PLANES)[1:])


def test_kept_fine_to_coarse(out):
    out, raw = out
    shape = (S, V, U)
    fmap, fvalid = np.fromfile(out / "f2c_fused_map.f32", F).reshape(shape), np.fromfile(out / "f2c_fused_valid.u8", np.uint8).reshape(shape)
    want = nr.novel(fmap, fvalid, 1.0, [3.0], [3], tol=STEP, volume=raw)
    nr.assert_equal(_novel(out, "f2c_fused", (1, V, U)), want, "FineToCoarse::get_novel_view(3, 0, true, 3)", names=tuple(PLANES))
    assert (want["n_src"] >= 2).any()
    # level 1: the geometry against the yardstick with the slope U_1 / U_0 (its colour comes from the level's own volume, which
    # tests/test_gpu_novel_view.py reads back)
    shape1 = (S, V // 2, U // 2)
    d1, v1 = np.fromfile(out / "f2c_depth1.f32", F).reshape(shape1), np.fromfile(out / "f2c_valid1.u8", np.uint8).reshape(shape1)
    got = _novel(out, "f2c_level1", (1,) + shape1[1:])
    nr.assert_equal(got, nr.novel(d1, v1, F(0.5), [3.5], None, 2, 1, 3, 2, 0.3), "FineToCoarse::get_novel_view(3.5, 1, false, -1, {2, 1, 3, 2, 0.3})",
                    names=tuple(PLANES)[1:])
    assert got["colour"].any() and not got["colour"][got["fill"] == 0].any()
