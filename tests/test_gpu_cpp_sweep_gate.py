"""The sweep gate through the C++11 host wrapper (include/rslf_hip.hpp): tests/cpp/test_host_sweep_gate.cpp, compiled with g++
against librslf_hip.so and run once on the GPU on case A at the ratio 0.7 -- rslfx::Depth2DComputer on the case's level 0 and a
kept rslfx::FineToCoarse on its raw field.  The program itself checks the setters' refusals, r = 1, the ratio switched off
again and every plane against the C entries; here what it wrote is held to the yardstick tests/sweep_gate_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import f2c_keep_ref as kr
import sweep_gate_ref as sgr
from util import TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, S, U = 44, 5, 64
F = np.float32


@pytest.fixture(scope="module")
def out(tmp_path_factory, oracle_mod):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from remotesensingproject_amd import _lib
    _lib.lib()   # the library the package runs (built first if it is missing)
    so = _lib.library_path()
    tmp = tmp_path_factory.mktemp("host_sweep_gate")
    raw = kr.make_field("A")
    level0 = sgr.field(oracle_mod, "A")[0]
    assert raw.shape == (V, S, U, 1) and raw.dtype == F and level0.shape == raw.shape and level0.dtype == F
    raw.tofile(tmp / "input.f32")
    np.ascontiguousarray(level0).tofile(tmp / "level0.f32")
    exe = str(tmp / "test_host_sweep_gate")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_host_sweep_gate.cpp"), "-o", exe,
                    "-L", os.path.dirname(so), "-lrslf_hip", "-Wl,-rpath," + os.path.dirname(so)], check=True)
    r = subprocess.run([exe, str(tmp)], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    return tmp


def _bits_equal(got, want, label):
    g = got.view(np.uint32) if got.dtype == F else got
    w = np.ascontiguousarray(want)
    w = w.view(np.uint32) if w.dtype == F else w
    assert g.shape == w.shape and np.array_equal(g, w), (label, int((g != w).sum()))


def test_the_classes_give_the_yardsticks_planes(out, oracle_mod):
    ref = sgr.case_reference(oracle_mod, "A")[3]
    rd = lambda name, dt: np.fromfile(out / name, dt).reshape(S, V, U)
    _bits_equal(rd("gate_depth.f32", F), ref[0]["depth"], "depth")
    assert np.abs(rd("gate_Cd.f32", F).astype(np.float64) - ref[0]["disp_confidence"]).max() <= TOL
    _bits_equal(rd("gate_idx.i32", np.int32), ref[1]["idx"], "idx")
    _bits_equal(rd("gate_score.f32", F), ref[1]["score"], "score")
    _bits_equal(rd("gate_runner_idx.i32", np.int32), ref[1]["runner_idx"], "runner_idx")
    _bits_equal(rd("gate_runner_score.f32", F), ref[1]["runner_score"], "runner_score")
    pyr = sgr.f2c_reference(oracle_mod, "A", sgr.RATIOS["A"])
    _bits_equal(rd("f2c_fused_map.f32", F), pyr["fused_map"], "fused map")
    _bits_equal(rd("f2c_depth0.f32", F), pyr["levels"][0]["depth"], "level 0 depth")
    counts = [int(x) for x in (out / "counts.txt").read_text().split()]
    assert counts == [sum(ref[3])] + [lv["withheld"] for lv in pyr["levels"]]
