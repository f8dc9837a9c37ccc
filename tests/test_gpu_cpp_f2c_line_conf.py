"""rslfx::FineToCoarse with the line confidence (include/rslf_hip.hpp), compiled with g++ against librslf_hip.so and run on
the GPU: case A in mode 2 against the numpy yardstick (tests/f2c_line_conf_ref.py), get_coloured_depth_pyr against the
Python getter byte for byte, and set_line_confidence_mode on a MultiContext."""
import os
import subprocess

import numpy as np
import pytest

import f2c_line_conf_ref as fr

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(src, exe):
    from remotesensingproject_amd import _lib
    _lib.lib()
    so = _lib.library_path()
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                    "-L", os.path.dirname(so), "-lrslf_hip", "-Wl,-rpath," + os.path.dirname(so)], check=True)


def test_cpp_fine_to_coarse_in_mode_2(tmp_path, oracle_mod):
    from remotesensingproject_amd import depth as rs
    exe = str(tmp_path / "test_host_f2c_line_conf")
    _compile(os.path.join(ROOT, "tests", "cpp", "test_host_f2c_line_conf.cpp"), exe)
    C_, dt, V, U, S, D, accept, thrs = fr.CASES["A"]
    thr = thrs[0]
    ref = fr.reference(oracle_mod, "A", 2, thr)
    field = fr.make_field("A")
    field.tofile(tmp_path / "input.f32")
    r = subprocess.run([exe, str(tmp_path), str(V), str(S), str(U), str(D), "%.9g" % F(thr)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rd = lambda name, t: np.fromfile(tmp_path / name, t)
    dims = [tuple(map(int, line.split())) for line in open(tmp_path / "f2c_dims.txt")]
    assert dims == ref["dims"]
    lut = rd("f2c_lut.u8", np.uint8).reshape(256, 3)
    f2c = rs.FineToCoarse(list(field[..., 0]), -1.0, 1.0, D, parameters=rs.Depth1DParameters(par_line_score_threshold=thr),
                          line_confidence_mode=2)
    f2c.run()
    pyr = f2c.get_coloured_depth_pyr(-1, lut)
    for l, (Vp, Up) in enumerate(dims):
        lv = ref["levels"][l]
        assert np.array_equal(rd("f2c_l%d_Cl.f32" % l, F).view(np.uint32).reshape(S, Vp, Up), lv["line_confidence"].view(np.uint32)), l
        assert np.array_equal(rd("f2c_l%d_valid.u8" % l, np.uint8).reshape(S, Vp, Up), lv["valid"]), l
        assert np.array_equal(rd("f2c_l%d_depth.f32" % l, F).view(np.uint32).reshape(S, Vp, Up), lv["depth"].view(np.uint32)), l
        assert np.array_equal(rd("f2c_l%d_pyr.u8" % l, np.uint8).reshape(Vp, Up, 3), pyr[l].cpu().numpy()), l
    assert np.array_equal(rd("f2c_map.f32", F).view(np.uint32).reshape(S, V, U), ref["fused_map"].view(np.uint32))
    assert np.array_equal(rd("f2c_valid.u8", np.uint8).reshape(S, V, U), ref["fused_valid"])


def test_cpp_multi_context_refuses_the_mode(tmp_path):
    src = tmp_path / "multi.cpp"
    src.write_text(r'''
#include <cstdio>
#include <vector>
#include "rslf_hip.hpp"
int main()
{
    std::vector<float> flat(40 * 3 * 40, 0.5f);
    std::vector<const void*> ptrs(40);
    for (int v = 0; v < 40; v++)
        ptrs[v] = flat.data() + (size_t)v * 3 * 40;
    rslfx::MultiContext multi(std::vector<int>(1, 0));
    rslfx::FineToCoarse<1> f2c(multi, ptrs.data(), false, 40, 3, 40, 0, -1.0f, 1.0f, 8);
    try {
        f2c.set_line_confidence_mode(RSLF_LINE_CONF_AS_BUILT);
    } catch (const rslfx::Error& e) {
        std::printf("refused: %s\n", e.what());
        return 0;
    }
    return 1;
}
''')
    exe = str(tmp_path / "multi")
    _compile(str(src), exe)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "refused" in r.stdout, r.stdout + r.stderr
