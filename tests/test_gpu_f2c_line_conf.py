"""Fine-to-coarse with the line confidence C_l on the GPU against the numpy yardstick tests/f2c_line_conf_ref.py: the class
path (rs.FineToCoarse(..., line_confidence_mode=m)) level by level, mode 1 against the default build, the native level loop
(rslf_fine_to_coarse_run_host_lc / _u16_lc) against the class path, the precedence of C_d, the pyramid getter and the error
cases.  Everything is bit-exact but C_d (a double sum whose order is free), held to 1e-5 as include/rslf_hip.h states."""
import ctypes as C

import numpy as np
import pytest

import f2c_line_conf_ref as fr
import render_ref as rr

pytestmark = pytest.mark.gpu
F = np.float32
EXACT = ("edge_mask", "scan_mask", "edge_confidence", "depth", "rbar", "line_confidence")
RUNS = [(name, 1, 0.02) for name in fr.CASES] + [(name, 2, thr) for name, case in fr.CASES.items() for thr in case[7]]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, label):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (label, bad.size, np.unravel_index(bad[0], want.shape))


def _epis(field):
    """[V,S,U,C] -> the list of V EPIs the classes take ([S,U] with one channel)."""
    return list(field[..., 0]) if field.shape[3] == 1 else list(field)


def _params(thr, use_disp=False):
    from remotesensingproject_amd import depth as rs
    return rs.Depth1DParameters(par_line_score_threshold=thr, par_use_disp_confidence_score=use_disp)


def _class_run(name, mode, thr=0.02, use_disp=False, field=None):
    from remotesensingproject_amd import depth as rs
    D, accept = fr.CASES[name][5], fr.CASES[name][6]
    f2c = rs.FineToCoarse(_epis(fr.make_field(name) if field is None else field), -1.0, 1.0, D, parameters=_params(thr, use_disp),
                          accept_all_last_scale=accept, line_confidence_mode=mode)
    f2c.run()
    return f2c


def _check_against(f2c, ref, label):
    assert [(c.m_epis.V, c.m_epis.U) for c in f2c.m_computers] == ref["dims"], label
    for l, (comp, lv) in enumerate(zip(f2c.m_computers, ref["levels"])):
        got = comp.results()
        for k in EXACT:
            _same(got[k], lv[k], (label, l, k))
        err = float(np.abs(got["disp_confidence"] - lv["disp_confidence"]).max())
        assert err <= 1e-5, (label, l, "disp_confidence", err)
        _same(comp.get_valid_depths_mask_s_v_u().cpu().numpy(), lv["valid"], (label, l, "valid"))
        if l > 0:
            _same(comp.m_dmin_s_v_u.cpu().numpy(), lv["dmin"], (label, l, "dmin"))
            _same(comp.m_dmax_s_v_u.cpu().numpy(), lv["dmax"], (label, l, "dmax"))
    out_map, out_valid = f2c.get_results()
    _same(out_map.cpu().numpy(), ref["fused_map"], (label, "fused map"))
    _same(out_valid.cpu().numpy(), ref["fused_valid"], (label, "fused validity"))
    assert sum(c.stats.pixels_scanned for c in f2c.m_computers) == ref["pixels_scanned"], label


# ---- 1: the class path against the yardstick ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,mode,thr", RUNS, ids=["%s_mode%d_%g" % r for r in RUNS])
def test_class_path_matches_the_yardstick(oracle_mod, name, mode, thr):
    _check_against(_class_run(name, mode, thr), fr.reference(oracle_mod, name, mode, thr), "%s mode %d thr %g" % (name, mode, thr))


# ---- 2: mode 1 is mode 0 plus planes -----------------------------------------------------------------------------------

def test_mode_1_is_the_default_build_plus_planes():
    import torch
    a, b = _class_run("A", None), _class_run("A", 1)
    for l, (ca, cb) in enumerate(zip(a.m_computers, b.m_computers)):
        for k in ("m_edge_confidence_s_v_u", "m_edge_confidence_mask_s_v_u", "m_disp_confidence_s_v_u", "m_best_depth_s_v_u",
                  "m_rbar_s_v_u", "m_scan_mask_s_v_u"):
            assert torch.equal(getattr(ca, k), getattr(cb, k)), (l, k)
        assert torch.equal(ca.get_valid_depths_mask_s_v_u(), cb.get_valid_depths_mask_s_v_u()), l
        if l > 0:
            assert torch.equal(ca.m_dmin_s_v_u, cb.m_dmin_s_v_u) and torch.equal(ca.m_dmax_s_v_u, cb.m_dmax_s_v_u), l
        assert ca.stats.pixels_scanned == cb.stats.pixels_scanned
        assert ca.m_line_confidence_s_v_u is None and bool((cb.m_line_confidence_s_v_u > 0).any())
    for x, y in zip(a.get_results(), b.get_results()):
        assert torch.equal(x, y)


# ---- 3: the native level loop against the class path -------------------------------------------------------------------

@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", ["A", "B"])
def test_native_loop_equals_the_class_path(name, mode):
    from remotesensingproject_amd import depth as rs
    C_, dt, V, U, S, D, accept, thrs = fr.CASES[name]
    thr = thrs[0]
    f2c = _class_run(name, mode, thr)
    out = rs.fine_to_coarse_run_host(_epis(fr.make_field(name)), -1.0, 1.0, D, parameters=_params(thr), accept_all_last_scale=accept,
                                     line_mode=mode, want_levels=True)
    assert out["n_levels"] == len(f2c.m_computers) == len(out["levels"])
    for l, (comp, lv) in enumerate(zip(f2c.m_computers, out["levels"])):
        assert np.array_equal(_bits(lv["depth"]), _bits(comp.m_best_depth_s_v_u.cpu().numpy())), l
        assert np.array_equal(lv["valid"], comp.get_valid_depths_mask_s_v_u().cpu().numpy()), l
        assert np.array_equal(_bits(lv["line_confidence"]), _bits(comp.m_line_confidence_s_v_u.cpu().numpy())), l
        assert np.array_equal(_bits(lv["edge_confidence"]), _bits(comp.m_edge_confidence_s_v_u.cpu().numpy())), l
    out_map, out_valid = f2c.get_results()
    assert np.array_equal(_bits(out["out_map"]), _bits(out_map.cpu().numpy())) and np.array_equal(out["out_valid"], out_valid.cpu().numpy())
    assert out["stats"].pixels_scanned == sum(c.stats.pixels_scanned for c in f2c.m_computers)


def _plain_entry(epis, D, accept, u16=False):
    """rslf_fine_to_coarse_run_host / _u16, the entries that were there before."""
    from remotesensingproject_amd import _lib, depth as rs
    keep, ptrs, dt, V, S, U, C_ = rs.host_epis(epis)
    ctx = rs.default_context()
    ctx.use_current_stream()
    out_map, out_valid = np.empty((S, V, U), F), np.empty((S, V, U), np.uint8)
    p, st, nl = rs.Depth1DParameters().to_c(), _lib.RslfStats(), C.c_int()
    rest = (V, S, U, C_, 0, -1.0, 1.0, D, -1.0, C.byref(p), -1, 1 if accept else 0, out_map.ctypes.data_as(C.c_void_p),
            out_valid.ctypes.data_as(C.c_void_p), C.byref(nl), C.byref(st))
    L = _lib.lib()
    if u16:
        assert L.rslf_fine_to_coarse_run_host_u16(ctx._h, ptrs, *rest) == 0
    else:
        assert L.rslf_fine_to_coarse_run_host(ctx._h, ptrs, 1 if dt == np.uint8 else 0, *rest) == 0
    return out_map, out_valid, nl.value, st.pixels_scanned


@pytest.mark.parametrize("name", ["A", "B"])
def test_mode_0_through_the_lc_entry_is_the_plain_entry(name):
    from remotesensingproject_amd import depth as rs
    D, accept = fr.CASES[name][5], fr.CASES[name][6]
    epis = _epis(fr.make_field(name))
    want = _plain_entry(epis, D, accept)
    out = rs.fine_to_coarse_run_host(epis, -1.0, 1.0, D, accept_all_last_scale=accept, line_mode=0)
    assert np.array_equal(_bits(out["out_map"]), _bits(want[0])) and np.array_equal(out["out_valid"], want[1])
    assert (out["n_levels"], out["stats"].pixels_scanned) == want[2:]


# ---- 4: CV_16U ---------------------------------------------------------------------------------------------------------

def _u16_field():
    from remotesensingproject_amd.synth import make_lightfield
    C_, dt, V, U, S, D, _, _ = fr.CASES["A"]
    vol, _ = make_lightfield(U, V, S, C_, seed=2, dmin=-1.0, dmax=1.0, band=8)
    return np.ascontiguousarray(np.rint(vol * 65535.0).astype(np.uint16))


def test_u16_mode_1_is_the_plain_u16_entry_and_mode_2_is_the_class_path():
    from remotesensingproject_amd import depth as rs
    D, accept, thr = fr.CASES["A"][5], fr.CASES["A"][6], fr.CASES["A"][7][0]
    field = _u16_field()
    epis = _epis(field)
    want = _plain_entry(epis, D, accept, u16=True)
    got = rs.fine_to_coarse_run_host(epis, -1.0, 1.0, D, accept_all_last_scale=accept, line_mode=1, want_levels=True)
    assert np.array_equal(_bits(got["out_map"]), _bits(want[0])) and np.array_equal(got["out_valid"], want[1])
    assert bool((got["levels"][0]["line_confidence"] > 0).any())
    f2c = _class_run("A", 2, thr, field=field)
    got2 = rs.fine_to_coarse_run_host(epis, -1.0, 1.0, D, parameters=_params(thr), accept_all_last_scale=accept, line_mode=2,
                                      want_levels=True)
    for l, (comp, lv) in enumerate(zip(f2c.m_computers, got2["levels"])):
        assert np.array_equal(_bits(lv["line_confidence"]), _bits(comp.m_line_confidence_s_v_u.cpu().numpy())), l
        assert np.array_equal(lv["valid"], comp.get_valid_depths_mask_s_v_u().cpu().numpy()), l
    assert not np.array_equal(got2["levels"][0]["valid"], got["levels"][0]["valid"])   # the validity moved with the mode


# ---- 5: precedence -----------------------------------------------------------------------------------------------------

def test_the_disp_confidence_comes_first(oracle_mod):
    thr = fr.CASES["A"][7][0]
    ref = fr.reference(oracle_mod, "A", 2, thr, use_disp=True)
    f2c = _class_run("A", 2, thr, use_disp=True)
    _check_against(f2c, ref, "A mode 2 with use_disp_confidence_score")
    ref0 = fr.reference(oracle_mod, "A", 0, use_disp=True)
    for comp, lv in zip(f2c.m_computers, ref0["levels"]):
        assert np.array_equal(comp.get_valid_depths_mask_s_v_u().cpu().numpy(), lv["valid"])
    from remotesensingproject_amd import depth as rs
    out = rs.fine_to_coarse_run_host(_epis(fr.make_field("A")), -1.0, 1.0, fr.CASES["A"][5], parameters=_params(thr, True), line_mode=2)
    assert np.array_equal(_bits(out["out_map"]), _bits(ref["fused_map"])) and np.array_equal(out["out_valid"], ref["fused_valid"])


# ---- 6: the getters ----------------------------------------------------------------------------------------------------

def test_pyramid_getter_paints_under_the_line_confidence_in_mode_2(oracle_mod):
    from remotesensingproject_amd import depth as rs
    thr = fr.CASES["A"][7][0]
    ref = fr.reference(oracle_mod, "A", 2, thr)
    f2c = _class_run("A", 2, thr)
    lut = rs.colormap_jet()
    assert lut.any(axis=1).all()   # no black entry: black is the mask's alone
    depths, valids = [lv["depth"] for lv in ref["levels"]], [lv["valid"] for lv in ref["levels"]]
    by_edge = np.where(ref["levels"][0]["edge_confidence"] > F(0.02), 255, 0).astype(np.uint8)
    assert not np.array_equal(valids[0], by_edge)
    for s in (-1, 0):
        got = [t.cpu().numpy() for t in f2c.get_coloured_depth_pyr(s, lut)]
        want = rr.f2c_coloured_depth_pyr(depths, valids, lut, s)
        view = rr.centre_index(depths[0].shape[0]) if s == -1 else s
        for l, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (s, l)
            assert np.array_equal(g.any(axis=2), valids[l][view] != 0), (s, l)


# ---- 8: errors ---------------------------------------------------------------------------------------------------------

def test_error_cases():
    from remotesensingproject_amd import _lib, depth as rs
    L = _lib.lib()
    INVALID = -1
    C_, dt, V, U, S, D, accept, _ = fr.CASES["A"]
    keep, ptrs, _, V, S, U, C_ = rs.host_epis(_epis(fr.make_field("A")))
    ctx = rs.default_context()
    ctx.use_current_stream()
    out_map, out_valid = np.full((S, V, U), -7.0, F), np.full((S, V, U), 7, np.uint8)
    p = rs.Depth1DParameters().to_c()
    run = lambda mode, lo: L.rslf_fine_to_coarse_run_host_lc(ctx._h, ptrs, 0, V, S, U, C_, 0, -1.0, 1.0, D, -1.0, C.byref(p), -1, 1,
                                                             out_map.ctypes.data_as(C.c_void_p), out_valid.ctypes.data_as(C.c_void_p),
                                                             None, None, mode, lo)
    assert run(3, None) == INVALID and b"mode" in L.rslf_last_error()
    assert run(-1, None) == INVALID
    short = _lib.RslfF2cLevelsOut(2, None, None, None, None)   # the pyramid has three levels
    assert run(1, C.byref(short)) == INVALID and b"capacity" in L.rslf_last_error()
    u16 = np.zeros((V, S, U), np.uint16)
    keep16, ptrs16, _, _, _, _, _ = rs.host_epis(list(u16))
    assert L.rslf_fine_to_coarse_run_host_u16_lc(ctx._h, ptrs16, V, S, U, 1, 0, -1.0, 1.0, D, -1.0, C.byref(p), -1, 1,
                                                 out_map.ctypes.data_as(C.c_void_p), out_valid.ctypes.data_as(C.c_void_p), None, None,
                                                 3, None) == INVALID
    ctx.synchronize()
    assert (out_map == F(-7.0)).all() and (out_valid == 7).all()   # nothing ran
    with pytest.raises(ValueError):
        rs.FineToCoarse(_epis(fr.make_field("A")), -1.0, 1.0, D, line_confidence_mode=3)
    # a NULL member and NULL entries of the level outputs are "not wanted"
    some = _lib.RslfF2cLevelsOut(3, None, None, (C.c_void_p * 3)(None, None, None), None)
    assert run(1, C.byref(some)) == 0
