"""The picture getters of the C++11 host wrapper (include/rslf_hip.hpp): tests/cpp/test_host_getters.cpp, compiled with
g++ against librslf_hip.so and run once on the GPU, writes every picture together with the result planes it rendered
from; here each picture is rebuilt from those planes with tests/render_ref.py and compared byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import render_ref as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    from remotesensingproject_amd import _lib
    _lib.lib()   # the library the package runs (built first if it is missing)
    so = _lib.library_path()
    tmp = tmp_path_factory.mktemp("host_getters")
    exe = str(tmp / "test_host_getters")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_host_getters.cpp"), "-o", exe,
                    "-L", os.path.dirname(so), "-lrslf_hip", "-Wl,-rpath," + os.path.dirname(so)], check=True)
    r = subprocess.run([exe, str(tmp)], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr   # includes: refusals, the MultiContext objects through the Context& forms

    def read(name, dtype, *shape):
        a = np.fromfile(tmp / name, dtype)
        return a.reshape(shape) if shape else a
    return read


def test_pile_getters(out):
    V, S, U = 7, 13, 150
    lut = out("lut.u8", np.uint8, 256, 3)
    depth, mask = out("pile_depth.f32", np.float32, V, U), out("pile_mask.u8", np.uint8, V, U)
    s_hat = int(out("pile_s_hat.i32", np.int32)[0])
    assert 0 < (mask != 0).sum() < mask.size
    assert np.array_equal(out("pile_epi_default.u8", np.uint8, S, U, 3), rr.pile_coloured_epi(depth, mask, S, s_hat, lut))
    assert np.array_equal(out("pile_epi_5.u8", np.uint8, S, U, 3), rr.pile_coloured_epi(depth, mask, S, s_hat, lut, 5))
    assert np.array_equal(out("pile_map.u8", np.uint8, V, U, 3), rr.disparity_map(depth, mask, lut))


def test_depth2d_getters(out):
    V, S, U = 44, 5, 64
    lut = out("lut.u8", np.uint8, 256, 3)
    depth, mask = out("d2_depth.f32", np.float32, S, V, U), out("d2_mask.u8", np.uint8, S, V, U)
    assert 0 < (mask != 0).sum() < mask.size
    assert np.array_equal(out("d2_epi_default.u8", np.uint8, S, U, 3), rr.depth2d_coloured_epi(depth, mask, lut))
    assert np.array_equal(out("d2_epi_43.u8", np.uint8, S, U, 3), rr.depth2d_coloured_epi(depth, mask, lut, 43))
    assert np.array_equal(out("d2_map_default.u8", np.uint8, V, U, 3), rr.disparity_map(depth[S // 2], mask[S // 2], lut))
    assert np.array_equal(out("d2_map_0.u8", np.uint8, V, U, 3), rr.disparity_map(depth[0], mask[0], lut))
    want = np.stack([rr.disparity_map(depth[s], mask[s], lut) for s in range(S)])
    assert np.array_equal(out("d2_maps.u8", np.uint8, S, V, U, 3), want)
    want = np.stack([rr.depth2d_coloured_epi(depth, mask, lut, v) for v in range(V)])
    assert np.array_equal(out("d2_epis.u8", np.uint8, V, S, U, 3), want)
    # The batch does hold planes with ranges of their own: on this field every view spans (0, 1), but the scanlines of the
    # upper half (disparity 0 throughout) span (0, 0) and those of the shifted lower half (0, 1).
    assert len({rr.fit(np.ascontiguousarray(depth[:, v, :]), rr.MINMAX) for v in range(V)}) > 1


def test_depth2d_getters_under_the_disparity_confidence_switch(out):
    V, S, U = 44, 5, 64
    lut = out("lut.u8", np.uint8, 256, 3)
    depth, conf = out("d2s_depth.f32", np.float32, S, V, U), out("d2s_conf.f32", np.float32, S, V, U)
    mask = (conf > out("d2s_threshold.f32", np.float32)[0]).astype(np.uint8) * 255
    assert 0 < (mask != 0).sum() < mask.size
    want = np.stack([rr.disparity_map(depth[s], mask[s], lut) for s in range(S)])
    assert np.array_equal(out("d2s_maps.u8", np.uint8, S, V, U, 3), want)


def test_fine_to_coarse_getter_with_and_without_the_shadow_cut(out):
    V, S, U = 44, 5, 64
    lut = out("lut.u8", np.uint8, 256, 3)
    raw = out("sweep_input.f32", np.float32, V, S, U, 1)
    rad = raw * np.float32(1.0 / np.float64(raw.max()))   # the constructor's copy: times float(1 / max over all EPIs)
    level = out("shadow_level.f32", np.float32)[0]
    dark = rr.norms(rad) < level
    assert 0 < dark.sum() < dark.size
    fused, valid = out("f2c_map.f32", np.float32, S, V, U), out("f2c_valid.u8", np.uint8, S, V, U)
    got = out("f2c_maps_cut.u8", np.uint8, S, V, U, 3)
    assert np.array_equal(got, rr.f2c_coloured_depth_maps(fused, valid, lut, True, rad, level))
    assert not np.array_equal(got, rr.f2c_coloured_depth_maps(fused, valid, lut))   # the cut does show
    fused, valid = out("f2c_plain_map.f32", np.float32, S, V, U), out("f2c_plain_valid.u8", np.uint8, S, V, U)
    assert np.array_equal(out("f2c_maps_plain.u8", np.uint8, S, V, U, 3), rr.f2c_coloured_depth_maps(fused, valid, lut))
