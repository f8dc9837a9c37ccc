"""FineToCoarse of the C++11 host wrapper (include/rslf_hip.hpp) with set_peaks and set_uniqueness_ratio:
tests/cpp/test_host_f2c_peaks.cpp, compiled with g++ against librslf_hip.so and run once on the GPU on case A of
tests/f2c_line_conf_ref.py at the ratio 0.7.  The program itself holds every plane of the object to what the C entry
rslf_f2c_run_host_pk gives and checks the setters' throws; here what it wrote is held to the yardstick tests/f2c_peaks_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import f2c_keep_ref as kr
import f2c_peaks_ref as pf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, S, U = 44, 5, 64


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    from remotesensingproject_amd import _lib
    _lib.lib()   # the library the package runs (built first if it is missing)
    so = _lib.library_path()
    tmp = tmp_path_factory.mktemp("host_f2c_peaks")
    field = kr.make_field("A")
    assert field.shape == (V, S, U, 1) and field.dtype == np.float32
    field.tofile(tmp / "input.f32")
    exe = str(tmp / "test_host_f2c_peaks")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_host_f2c_peaks.cpp"), "-o", exe,
                    "-L", os.path.dirname(so), "-lrslf_hip", "-Wl,-rpath," + os.path.dirname(so)], check=True)
    r = subprocess.run([exe, str(tmp)], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    # includes: the setters' throws, every plane equal to the C entry's, the ratio switched off again
    assert r.returncode == 0, r.stdout + r.stderr
    return lambda name, dtype: np.fromfile(tmp / name, dtype).reshape(S, V, U)


def test_the_wrapper_gives_the_yardsticks_planes(out, oracle_mod):
    ref = pf.reference(oracle_mod, "A", ratio=0.7)
    for name, dtype, want in (("fused_map.f32", np.uint32, ref["fused_map"].view(np.uint32)), ("fused_level.u8", np.uint8, ref["fused_level"]),
                              ("fused_idx.i32", np.int32, ref["fused_pk"]["idx"]), ("valid0.u8", np.uint8, ref["levels"][0]["valid"])):
        got = out(name, dtype)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
    assert [int((out("fused_level.u8", np.uint8) == p).sum()) for p in range(3)] == [12324, 1096, 660]
