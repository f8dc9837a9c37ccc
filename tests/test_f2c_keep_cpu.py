"""The kept fine-to-coarse run without a GPU: the validity rule and the sizing functions under ASan / UBSan, the yardstick
(tests/f2c_keep_ref.py) against tests/f2c_line_conf_ref.py where both speak, the conditions under which the cases can tell
validity by C_d from validity by C_e, and the new entry points in header and library with NULL handles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import f2c_keep_ref as kr
import f2c_line_conf_ref as fr
from util import TOL

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rslf_f2c_run_host", "rslf_f2c_run_destroy", "rslf_f2c_run_describe", "rslf_f2c_run_copy", "rslf_f2c_run_volume",
           "rslf_f2c_run_render_depth_maps", "rslf_f2c_run_render_depth_maps_host", "rslf_f2c_run_render_depth_pyr",
           "rslf_f2c_run_render_depth_pyr_host", "rslf_f2c_run_render_epi_pyr", "rslf_f2c_run_render_epi_pyr_host"]
PLANES = ("edge_confidence", "edge_mask", "disp_confidence", "depth", "rbar", "scan_mask", "line_confidence", "valid", "dmin", "dmax")
DISP_CASES = [("A", 0.2), ("B", 1.0)]   # (case, disp_score_threshold) of the REFERENCE-rule tests


def test_validity_rule_and_sizes_under_sanitizers(tmp_path):
    exe = tmp_path / "test_plan_f2c_keep"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-Werror", "-I", os.path.join(ROOT, "remotesensingproject_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_plan_f2c_keep.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "kept fine-to-coarse plan tests ok" in r.stdout


# ---- the yardstick itself ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rule", [kr.COMPAT, kr.REFERENCE])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_without_use_disp_the_yardstick_is_the_line_confidence_yardstick(oracle_mod, mode, rule):
    """use_disp_confidence_score = 0: both rules are the table of f2c_line_conf_ref, plane for plane."""
    thr = fr.CASES["A"][7][1] if mode == 2 else 0.02
    got, want = kr.reference(oracle_mod, "A", mode, thr, rule=rule), fr.reference(oracle_mod, "A", mode, thr)
    assert got["dims"] == want["dims"] and got["pixels_scanned"] == want["pixels_scanned"]
    for l, (a, b) in enumerate(zip(got["levels"], want["levels"])):
        for k in PLANES:
            assert np.array_equal(a[k], b[k], equal_nan=True), (l, k)
    assert np.array_equal(got["fused_map"], want["fused_map"]) and np.array_equal(got["fused_valid"], want["fused_valid"])
    # the volumes are the normalised levels: the first is the field over its own max
    field = fr.make_field("A")
    assert np.array_equal(got["volumes"][0], oracle_mod.normalize_f32(field, -1.0)[0]) and got["scales"][0] == float(field.max())
    assert [v.shape for v in got["volumes"]] == [(V, field.shape[1], U, field.shape[3]) for V, U in got["dims"]]


def test_the_compat_rule_with_use_disp_is_the_line_confidence_yardstick(oracle_mod):
    got, want = kr.reference(oracle_mod, "A", 0, use_disp=True), fr.reference(oracle_mod, "A", 0, use_disp=True)
    for l, (a, b) in enumerate(zip(got["levels"], want["levels"])):
        for k in PLANES:
            assert np.array_equal(a[k], b[k], equal_nan=True), (l, k)
    assert np.array_equal(got["fused_map"], want["fused_map"]) and np.array_equal(got["fused_valid"], want["fused_valid"])


@pytest.mark.parametrize("name,thr", DISP_CASES, ids=["%s_%g" % c for c in DISP_CASES])
def test_the_cases_can_tell_validity_by_disp_confidence_from_the_edge_reading(oracle_mod, name, thr):
    """Conditions on the yardstick alone, under use_disp_confidence_score with disp_score_threshold = thr: a share of level
    0's pixels strictly between 0.05 and 0.95 is valid by C_d; the fused map moves in at least 100 values against the C_e
    reading (the COMPAT rule); on case A the next level's tightened ranges move too; and no finite C_d lies within 2 TOL of
    the threshold, so the documented C_d tolerance cannot flip a validity byte."""
    ref = kr.reference(oracle_mod, name, 0, use_disp=True, disp_thr=thr, rule=kr.REFERENCE)
    by_edge = kr.reference(oracle_mod, name, 0, use_disp=True, disp_thr=thr, rule=kr.COMPAT)
    share = float((ref["levels"][0]["valid"] != 0).mean())
    moved = int((ref["fused_map"].view(np.uint32) != by_edge["fused_map"].view(np.uint32)).sum())
    moved_dmin = int((ref["levels"][1]["dmin"] != by_edge["levels"][1]["dmin"]).sum())
    nearest = min(float(np.abs(lv["disp_confidence"][np.isfinite(lv["disp_confidence"])] - F(thr)).min()) for lv in ref["levels"])
    print("%s @ %g: level-0 validity share %.3f, fused values moved %d, level-1 dmin moved %d, nearest C_d to the threshold %.3g"
          % (name, thr, share, moved, moved_dmin, nearest))
    assert 0.05 < share < 0.95, share
    assert moved >= 100, moved
    if name == "A":
        assert moved_dmin > 0
    assert nearest > 2 * TOL, nearest
    assert np.array_equal(ref["levels"][0]["valid"], np.where(ref["levels"][0]["disp_confidence"] > F(thr), 255, 0))
    last = ref["levels"][-1]
    assert (last["valid"] == 255).all()   # accept_all comes before C_d in the chain


def test_without_accept_all_the_fused_validity_moves_too(oracle_mod):
    ref = kr.reference(oracle_mod, "A_noacc", 0, use_disp=True, disp_thr=0.2, rule=kr.REFERENCE)
    by_edge = kr.reference(oracle_mod, "A_noacc", 0, use_disp=True, disp_thr=0.2, rule=kr.COMPAT)
    moved = int((ref["fused_valid"] != by_edge["fused_valid"]).sum())
    nearest = min(float(np.abs(lv["disp_confidence"][np.isfinite(lv["disp_confidence"])] - F(0.2)).min()) for lv in ref["levels"])
    print("A_noacc @ 0.2: fused validity values moved %d, nearest C_d to the threshold %.3g" % (moved, nearest))
    assert moved > 0 and nearest > 2 * TOL
    assert not (ref["levels"][-1]["valid"] == 255).all()


def test_the_darkened_fields_have_shadow_at_every_level(oracle_mod):
    """0 < dark < all at every level of the picture tests' fields: the shadow cut has something to cut and something to leave."""
    import render_ref as rr
    level = F(oracle_mod.default_params().shadow_level)
    for name in ("A", "B"):
        for l, vol in enumerate(kr.reference(oracle_mod, name, 0, dark=True)["volumes"]):
            dark = int((rr.norms(vol) < level).sum())
            assert 0 < dark < vol[..., 0].size, (name, l, dark)


# ---- header, library, NULL handles --------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "rslf_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"^\s*int\s+(rslf_\w+)\s*\(", hdr, flags=re.M))
    assert set(ENTRIES) <= declared, sorted(set(ENTRIES) - declared)
    for macro, value in (("RSLF_ELEM_F32", 0), ("RSLF_ELEM_U8", 1), ("RSLF_ELEM_U16", 2), ("RSLF_F2C_VALID_COMPAT", 0),
                         ("RSLF_F2C_VALID_REFERENCE", 1), ("RSLF_F2C_PLANE_DEPTH", 0), ("RSLF_F2C_PLANE_VALID", 1), ("RSLF_F2C_PLANE_CE", 2),
                         ("RSLF_F2C_PLANE_CD", 3), ("RSLF_F2C_PLANE_CL", 4), ("RSLF_F2C_PLANE_FUSED_MAP", 5),
                         ("RSLF_F2C_PLANE_FUSED_VALID", 6), ("RSLF_F2C_MAX_LEVELS", 32)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), hdr), macro
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.SYMBOLS
        getattr(L, name)   # AttributeError: not exported
    assert L.rslf_abi_version() == 6   # new entry points only: the ABI version stays


def test_the_run_description_has_the_layout_of_the_header(tmp_path):
    from remotesensingproject_amd import _lib
    fields = [f for f, _ in _lib.RslfF2cRunDesc._fields_]
    body = ['#include <stdio.h>', '#include <stddef.h>', '#include "rslf_hip.h"', 'int main(void){',
            'printf("%zu\\n", sizeof(rslf_f2c_run_desc));'] + ['printf("%%zu\\n", offsetof(rslf_f2c_run_desc, %s));' % f for f in fields]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(body + ["return 0;}"]))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert out == [C.sizeof(_lib.RslfF2cRunDesc)] + [getattr(_lib.RslfF2cRunDesc, f).offset for f in fields]


def test_null_handles_are_refused_and_say_so():
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    INVALID = -1
    p, st, run = _lib.default_params(), _lib.RslfStats(), C.c_void_p(1234)
    ptrs = (C.c_void_p * 1)(None)
    buf = (C.c_uint8 * 16)()
    outs = (C.c_void_p * 1)(C.addressof(buf))
    desc, vol = _lib.RslfF2cRunDesc(), C.c_void_p(5)
    calls = {
        "rslf_f2c_run_host": lambda: L.rslf_f2c_run_host(None, ptrs, 0, 44, 5, 64, 1, 0, -1.0, 1.0, 9, -1.0, C.byref(p), -1, 1, 0, 0, 1,
                                                         C.byref(run), C.byref(st)),
        "rslf_f2c_run_describe": lambda: L.rslf_f2c_run_describe(None, C.byref(desc)),
        "rslf_f2c_run_copy": lambda: L.rslf_f2c_run_copy(None, 0, 0, buf, 1, None),
        "rslf_f2c_run_volume": lambda: L.rslf_f2c_run_volume(None, 0, C.byref(vol)),
        "rslf_f2c_run_render_depth_maps": lambda: L.rslf_f2c_run_render_depth_maps(None, None, 1, buf, buf),
        "rslf_f2c_run_render_depth_maps_host": lambda: L.rslf_f2c_run_render_depth_maps_host(None, None, 1, buf, buf),
        "rslf_f2c_run_render_depth_pyr": lambda: L.rslf_f2c_run_render_depth_pyr(None, None, -1, 1, buf, outs),
        "rslf_f2c_run_render_depth_pyr_host": lambda: L.rslf_f2c_run_render_depth_pyr_host(None, None, -1, 1, buf, outs),
        "rslf_f2c_run_render_epi_pyr": lambda: L.rslf_f2c_run_render_epi_pyr(None, None, -1, 1, buf, outs),
        "rslf_f2c_run_render_epi_pyr_host": lambda: L.rslf_f2c_run_render_epi_pyr_host(None, None, -1, 1, buf, outs),
    }
    assert set(calls) | {"rslf_f2c_run_destroy"} == set(ENTRIES)
    for name, call in calls.items():
        L.rslf_volume_describe(None, None)   # leaves another text behind
        before = L.rslf_last_error()
        assert call() == INVALID, name
        assert L.rslf_last_error() and L.rslf_last_error() != before, name
    assert run.value is None      # a failed run hands nothing out
    assert vol.value is None
    assert L.rslf_f2c_run_host(None, ptrs, 0, 44, 5, 64, 1, 0, -1.0, 1.0, 9, -1.0, C.byref(p), -1, 1, 0, 0, 1, None, None) == INVALID
    assert L.rslf_f2c_run_destroy(None) == 0


def test_the_python_form_refuses_what_a_kept_run_does_not_take():
    from remotesensingproject_amd import depth as rs
    field = [np.zeros((3, 40), F)] * 40
    with pytest.raises(ValueError, match="keep=True"):
        rs.fine_to_coarse_run_host(field, -1.0, 1.0, 8, validity_rule=rs.F2C_VALID_REFERENCE, ctx=object())
    with pytest.raises(ValueError, match="KeptFineToCoarse.plane"):
        rs.fine_to_coarse_run_host(field, -1.0, 1.0, 8, keep=True, want_levels=True, ctx=object())
