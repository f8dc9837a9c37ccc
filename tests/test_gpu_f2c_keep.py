"""The kept fine-to-coarse run (rslf_f2c_run_host and what follows it in include/rslf_hip.h) on the GPU against the numpy
yardstick tests/f2c_keep_ref.py: every kept plane under both validity rules, the kept volumes, the three coloured getters
against tests/render_ref.py, and the object's lifetime.  Everything is bit-exact but C_d (a double sum whose order is free),
held to util.TOL as include/rslf_hip.h states."""
import ctypes as C

import numpy as np
import pytest

import f2c_keep_ref as kr
import f2c_line_conf_ref as fr
from util import TOL

pytestmark = pytest.mark.gpu
F = np.float32
INVALID = -1
# yardstick plane -> the kept plane's name
KEPT = dict(depth="depth", valid="valid", edge_confidence="Ce", line_confidence="Cl")
COMPAT_RUNS = [(name, mode) for name in ("A", "B", "C", "U16") for mode in (0, 1, 2)]
REFERENCE_RUNS = [("A", 0.2), ("A_noacc", 0.2), ("B", 1.0)]


@pytest.fixture(scope="module")
def rs():
    from remotesensingproject_amd import depth
    return depth


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, label):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (label, bad.size, np.unravel_index(bad[0], want.shape))


def _epis(field):
    """[V,S,U,C] -> the list of V EPIs the entries take ([S,U] with one channel)."""
    return list(field[..., 0]) if field.shape[3] == 1 else list(field)


def _thr(name, mode):
    return fr.CASES["A" if name == "U16" else name][7][0] if mode == 2 else 0.02


def _params(rs, thr=0.02, use_disp=False, disp_thr=0.01, cut_shadows=True):
    return rs.Depth1DParameters(par_line_score_threshold=thr, par_use_disp_confidence_score=use_disp, par_disp_score_threshold=disp_thr,
                                par_cut_shadows=cut_shadows)


def _keep(rs, name, mode=0, thr=0.02, use_disp=False, disp_thr=0.01, rule=kr.COMPAT, keep_volumes=True, dark=False, ctx=None,
          epi_scale_factor=-1.0, cut_shadows=True, field=None):
    _, _, _, _, _, D, accept = kr.case_of(name)
    field = kr.make_field(name, dark) if field is None else field
    return rs.fine_to_coarse_run_host(_epis(field), -1.0, 1.0, D, epi_scale_factor, _params(rs, thr, use_disp, disp_thr, cut_shadows),
                                      accept_all_last_scale=accept, ctx=ctx, line_mode=mode, keep=True, validity_rule=rule,
                                      keep_volumes=keep_volumes)


def _planes(kept):
    """Every plane the run holds, on the host."""
    names = ["depth", "valid", "Ce", "Cd"] + (["Cl"] if kept.line_mode != 0 else [])
    out = dict(levels=[{k: kept.plane(l, k).cpu().numpy() for k in names} for l in range(kept.n_levels)])
    out["fused_map"], out["fused_valid"] = [t.cpu().numpy() for t in kept.get_results()]
    return out


def _check_against(kept, ref, label):
    assert kept.dims == ref["dims"], label
    got = _planes(kept)
    for l, lv in enumerate(ref["levels"]):
        for k, name in KEPT.items():
            if name in got["levels"][l]:
                _same(got["levels"][l][name], lv[k], (label, l, k))
        err = float(np.abs(got["levels"][l]["Cd"] - lv["disp_confidence"]).max())
        print("%s level %d: max |C_d - yardstick| %.3g" % (label, l, err))
        assert err <= TOL, (label, l, "disp_confidence", err)
    _same(got["fused_map"], ref["fused_map"], (label, "fused map"))
    _same(got["fused_valid"], ref["fused_valid"], (label, "fused validity"))
    assert kept.stats.pixels_scanned == ref["pixels_scanned"], label
    return got


def _read_device(ptr, nbytes):
    """Device memory at a raw address -> host bytes, through the HIP runtime the library itself is bound to."""
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.hipMemcpy.restype = C.c_int
    out = np.empty(nbytes, np.uint8)
    assert L.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), nbytes, 2) == 0   # hipMemcpyDeviceToHost
    return out


def _kept_volume(kept, level):
    """Level `level`'s kept volume read back through rslf_volume_describe's pointer and pitch -> [V,S,U,C], and its padding."""
    d = kept.volume_desc(level)
    assert d.bytes == d.V * d.S * d.C * d.pitch * 4 and d.pitch % 64 == 0 and d.pitch > d.U
    slab = _read_device(d.d_base, d.bytes).view(F).reshape(d.V, d.S, d.pitch, d.C)
    return slab[:, :, :d.U], slab[:, :, d.U:], d


# ---- 1: the COMPAT rule: the yardstick, and the entry that was there before ----------------------------------------------

@pytest.mark.parametrize("name,mode", COMPAT_RUNS, ids=["%s_mode%d" % r for r in COMPAT_RUNS])
def test_compat_run_matches_the_yardstick_and_the_levels_out_entry(rs, oracle_mod, name, mode):
    thr = _thr(name, mode)
    kept = _keep(rs, name, mode, thr)
    ref = kr.reference(oracle_mod, name, mode, thr)
    got = _check_against(kept, ref, "%s mode %d" % (name, mode))
    d = kept.describe()
    assert (d.n_levels, d.S, d.C, d.line_mode, d.validity_rule, d.keep_volumes) == (len(ref["dims"]), kept.S, kr.case_of(name)[0], mode, 0, 1)
    assert d.elem == {"f32": 0, "u8": 1, "u16": 2}[kr.case_of(name)[1]]
    assert kept.scales == [float(F(s)) for s in ref["scales"]]
    assert d.planes_held == (0b1101111 if mode == 0 else 0b1111111)
    # the same input through rslf_fine_to_coarse_run_host_lc / _u16_lc with levels_out
    _, _, _, _, _, D, accept = kr.case_of(name)
    out = rs.fine_to_coarse_run_host(_epis(kr.make_field(name)), -1.0, 1.0, D, parameters=_params(rs, thr), accept_all_last_scale=accept,
                                     line_mode=mode, want_levels=True)
    assert out["n_levels"] == kept.n_levels
    for l, lv in enumerate(out["levels"]):
        for k, kn in (("depth", "depth"), ("valid", "valid"), ("edge_confidence", "Ce"), ("line_confidence", "Cl")):
            if lv[k] is not None:
                _same(got["levels"][l][kn], lv[k], (name, mode, l, k, "levels_out"))
    _same(got["fused_map"], out["out_map"], "out_map")
    _same(got["fused_valid"], out["out_valid"], "out_valid")
    for f in ("pixels_scanned", "units", "scan_kernel", "s_pad"):
        assert getattr(kept.stats, f) == getattr(out["stats"], f), f
    kept.close()


# ---- 2: the REFERENCE rule: validity by C_d ------------------------------------------------------------------------------

@pytest.mark.parametrize("name,disp_thr", REFERENCE_RUNS, ids=["%s_%g" % r for r in REFERENCE_RUNS])
def test_reference_rule_reads_the_validity_from_the_disp_confidence(rs, oracle_mod, name, disp_thr):
    kept = _keep(rs, name, 0, use_disp=True, disp_thr=disp_thr, rule=kr.REFERENCE)
    ref = kr.reference(oracle_mod, name, 0, use_disp=True, disp_thr=disp_thr, rule=kr.REFERENCE)
    got = _check_against(kept, ref, "%s REFERENCE @ %g" % (name, disp_thr))
    assert kept.validity_rule == 1
    # ... and the COMPAT rule on the same parameters is the edge reading, which the yardstick tells apart
    compat = _keep(rs, name, 0, use_disp=True, disp_thr=disp_thr, rule=kr.COMPAT)
    by_edge = _check_against(compat, kr.reference(oracle_mod, name, 0, use_disp=True, disp_thr=disp_thr, rule=kr.COMPAT), "%s COMPAT" % name)
    assert not np.array_equal(got["levels"][0]["valid"], by_edge["levels"][0]["valid"])
    assert not np.array_equal(_bits(got["fused_map"]), _bits(by_edge["fused_map"]))
    kept.close(); compat.close()


def test_reference_rule_without_use_disp_is_the_compat_rule(rs):
    a, b = _keep(rs, "A", 2, _thr("A", 2), rule=kr.REFERENCE), _keep(rs, "A", 2, _thr("A", 2), rule=kr.COMPAT)
    pa, pb = _planes(a), _planes(b)
    for l in range(a.n_levels):
        for k in pa["levels"][l]:
            _same(pa["levels"][l][k], pb["levels"][l][k], (l, k))
    _same(pa["fused_map"], pb["fused_map"], "fused map")
    _same(pa["fused_valid"], pb["fused_valid"], "fused validity")


# ---- 3: the kept volumes -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,factor", [("A", -1.0), ("A", 250.0), ("B", -1.0), ("U16", -1.0)],
                         ids=["f32_own_max", "f32_given_factor", "u8", "u16"])
def test_kept_volumes_are_the_normalised_levels(rs, oracle_mod, name, factor):
    kept = _keep(rs, name, 0, epi_scale_factor=factor)
    ref = kr.reference(oracle_mod, name, 0, epi_scale_factor=factor)
    assert kept.scales == [float(F(s)) for s in ref["scales"]]
    total = 0
    for l, want in enumerate(ref["volumes"]):
        vol, pad, d = _kept_volume(kept, l)
        _same(vol, want, (name, factor, "volume", l))
        assert not pad.any(), (name, l, "padding")
        assert (d.V, d.S, d.U, d.C) == (want.shape[0], want.shape[1], want.shape[2], want.shape[3])
        n = d.S * d.V * d.U
        total += d.bytes + n * 13
    assert kept.describe().device_bytes == total + kept.S * kept.dims[0][0] * kept.dims[0][1] * 5
    if factor > 0:   # the given factor reached every level, and the run is the yardstick's
        assert kept.scales == [250.0] * kept.n_levels
        _check_against(kept, ref, "A with a given factor")
    kept.close()


def test_a_run_without_volumes_holds_none(rs):
    from remotesensingproject_amd import _lib
    kept = _keep(rs, "A", 1, keep_volumes=False)
    d = kept.describe()
    assert d.keep_volumes == 0 and d.device_bytes == sum(kept.S * v * u * 17 for v, u in kept.dims) + kept.S * kept.dims[0][0] * kept.dims[0][1] * 5
    vol = C.c_void_p(7)
    assert _lib.lib().rslf_f2c_run_volume(kept._h, 0, C.byref(vol)) == INVALID and vol.value is None
    assert b"keep_volumes" in _lib.lib().rslf_last_error()
    kept.close()


# ---- 4: the pictures -----------------------------------------------------------------------------------------------------

def _lut(rs):
    lut = rs.colormap_jet()
    assert lut.any(axis=1).all()   # no black entry: black is the masks' and the shadow cut's alone
    return lut


def _want_pictures(got, ref, lut, level, saturate, s, v, shadows=True):
    """render_ref on the planes copied from the handle; the radiance is the yardstick's normalised levels."""
    depths, valids = [lv["depth"] for lv in got["levels"]], [lv["valid"] for lv in got["levels"]]
    return kr.pictures(depths, valids, got["fused_map"], got["fused_valid"], lut, ref["volumes"] if shadows else None, level, saturate, s, v)


@pytest.mark.parametrize("name", ["A", "B"])
def test_getters_match_render_ref_in_every_variant(rs, oracle_mod, name):
    lut = _lut(rs)
    kept = _keep(rs, name, 0, dark=True)
    ref = kr.reference(oracle_mod, name, 0, dark=True)
    got = _check_against(kept, ref, "%s darkened" % name)
    level = float(F(oracle_mod.default_params().shadow_level))
    import render_ref as rr
    for l, vol in enumerate(ref["volumes"]):   # the darkened rectangle is in shadow at every level, and nothing else is
        dark = int((rr.norms(vol) < F(level)).sum())
        assert 0 < dark < vol[..., 0].size, (l, dark)
        _same(_kept_volume(kept, l)[0], vol, ("darkened volume", l))
    for saturate in (True, False):
        maps = kept.get_coloured_depth_maps(lut, saturate).cpu().numpy()
        want = _want_pictures(got, ref, lut, level, saturate, -1, -1)
        assert np.array_equal(maps, want["maps"]), ("maps", saturate)
        no_cut = _want_pictures(got, ref, lut, level, saturate, -1, -1, shadows=False)
        assert not np.array_equal(maps, no_cut["maps"])               # the shadow cut changed the picture
        for s in (-1, 0):
            pyr = [t.cpu().numpy() for t in kept.get_coloured_depth_pyr(s, lut, saturate)]
            want = _want_pictures(got, ref, lut, level, saturate, s, -1)
            assert len(pyr) == kept.n_levels
            for l, (g, w) in enumerate(zip(pyr, want["depth_pyr"])):
                assert np.array_equal(g, w), ("depth_pyr", saturate, s, l)
        for v in (-1, 5):
            pyr = [t.cpu().numpy() for t in kept.get_coloured_epi_pyr(v, lut, saturate)]
            want = _want_pictures(got, ref, lut, level, saturate, -1, v)
            no_cut = _want_pictures(got, ref, lut, level, saturate, -1, v, shadows=False)
            for l, (g, w) in enumerate(zip(pyr, want["epi_pyr"])):
                assert np.array_equal(g, w), ("epi_pyr", saturate, v, l)
            if v == -1:   # scanline 22 crosses the darkened rectangle: the cut changed the finest picture (scanline 5 lies above it)
                assert not np.array_equal(pyr[0], no_cut["epi_pyr"][0])
    kept.close()


def test_host_forms_give_the_device_pictures(rs):
    from remotesensingproject_amd import _lib
    L, lut = _lib.lib(), _lut(rs)
    kept = _keep(rs, "B", 0, dark=True)
    table = lut.ctypes.data_as(C.c_void_p)
    S, dims = kept.S, kept.dims
    kept.ctx.use_current_stream()
    maps = np.zeros((S,) + dims[0] + (3,), np.uint8)
    assert L.rslf_f2c_run_render_depth_maps_host(kept._h, kept.ctx._h, 0, table, maps.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(maps, kept.get_coloured_depth_maps(lut, False).cpu().numpy())
    for entry, shapes, arg, getter in (("rslf_f2c_run_render_depth_pyr_host", [d + (3,) for d in dims], 0, kept.get_coloured_depth_pyr),
                                       ("rslf_f2c_run_render_epi_pyr_host", [(S, u, 3) for _, u in dims], 5, kept.get_coloured_epi_pyr)):
        outs = [np.zeros(sh, np.uint8) for sh in shapes]
        ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
        assert getattr(L, entry)(kept._h, kept.ctx._h, arg, 1, table, ptrs) == 0, entry
        for l, (o, t) in enumerate(zip(outs, getter(arg, lut, True))):
            assert o.any() and np.array_equal(o, t.cpu().numpy()), (entry, l)
    kept.close()


def test_the_three_refusals(rs):
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd.synth import make_lightfield
    L, lut = _lib.lib(), _lut(rs)
    # S = 1: (int)std::round(1 / 2.0) = 1 is past the last view
    one_view, _ = make_lightfield(64, 44, 1, 1, seed=2, dmin=-1.0, dmax=1.0, band=8)
    kept = _keep(rs, "A", 0, field=np.ascontiguousarray(one_view))
    assert kept.S == 1
    with pytest.raises(ValueError, match="round"):
        kept.get_coloured_depth_maps(lut)
    with pytest.raises(ValueError, match="round"):
        kept.get_coloured_depth_pyr(-1, lut)
    assert len(kept.get_coloured_depth_pyr(0, lut)) == kept.n_levels     # the view named outright is fine
    with pytest.raises(ValueError):
        kept.get_coloured_depth_pyr(1, lut)
    kept.close()
    # v = V_0 - 1 with V_1 = V_0 / 2: round(43 * 22 / 44) = 22 is past level 1's last row
    kept = _keep(rs, "A", 0)
    assert kept.dims[0][0] == 44 and kept.dims[1][0] == 22
    outs = [np.full((kept.S, u, 3), 9, np.uint8) for _, u in kept.dims]
    ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
    assert L.rslf_f2c_run_render_epi_pyr_host(kept._h, kept.ctx._h, 43, 1, lut.ctypes.data_as(C.c_void_p), ptrs) == INVALID
    assert b"scanline 43" in L.rslf_last_error()
    assert all((o == 9).all() for o in outs)                              # refused before anything was written
    with pytest.raises(ValueError, match="scanline"):
        kept.get_coloured_epi_pyr(43, lut)
    with pytest.raises(ValueError):
        kept.get_coloured_epi_pyr(44, lut)
    kept.close()
    # cut_shadows without kept volumes: the two getters that cut say why; the one that does not cut works
    kept = _keep(rs, "A", 0, keep_volumes=False)
    for call in (lambda: kept.get_coloured_depth_maps(lut), lambda: kept.get_coloured_epi_pyr(-1, lut)):
        with pytest.raises(ValueError, match="keep_volumes"):
            call()
    assert len(kept.get_coloured_depth_pyr(-1, lut)) == kept.n_levels
    kept.close()
    # ... and without cut_shadows no volume is needed
    kept = _keep(rs, "A", 0, keep_volumes=False, cut_shadows=False)
    assert kept.get_coloured_depth_maps(lut).any() and len(kept.get_coloured_epi_pyr(-1, lut)) == kept.n_levels
    with pytest.raises(_lib.RslfError):
        kept.plane(0, "Cl")                                               # a plane that was not kept
    assert L.rslf_f2c_run_copy(kept._h, 1, 5, C.c_void_p(kept.plane(0, "depth").data_ptr()), 0, kept.ctx._h) == INVALID   # fused: level 0
    assert L.rslf_f2c_run_copy(kept._h, kept.n_levels, 0, C.c_void_p(kept.plane(0, "depth").data_ptr()), 0, kept.ctx._h) == INVALID
    kept.close()


# ---- 5: lifetime -----------------------------------------------------------------------------------------------------------

def _equal_planes(a, b, label):
    for l, (x, y) in enumerate(zip(a["levels"], b["levels"])):
        for k in x:
            _same(x[k], y[k], (label, l, k))
    _same(a["fused_map"], b["fused_map"], (label, "fused map"))
    _same(a["fused_valid"], b["fused_valid"], (label, "fused validity"))


def test_two_handles_of_different_shapes_and_a_later_run_leave_a_handle_unchanged(rs, oracle_mod):
    """Two runs alive at once; the second, larger one regrows the context's grow-only scratch and a third reuses it: the first
    run's planes and pictures are what they were."""
    lut = _lut(rs)
    ctx = rs.Context(0)
    a = _keep(rs, "A", 1, dark=True, ctx=ctx)
    before, maps = _planes(a), a.get_coloured_depth_maps(lut).cpu().numpy()
    c = _keep(rs, "C", 1, ctx=ctx)
    again = _keep(rs, "A", 1, dark=True, ctx=ctx)
    assert a.dims != c.dims
    _check_against(c, kr.reference(oracle_mod, "C", 1), "C beside A")
    _equal_planes(_planes(a), before, "A after C")
    _equal_planes(_planes(again), before, "A again")
    assert np.array_equal(a.get_coloured_depth_maps(lut).cpu().numpy(), maps)
    host = np.empty((a.S,) + a.dims[0], F)       # a host pointer, no context: the copy waits
    from remotesensingproject_amd import _lib
    assert _lib.lib().rslf_f2c_run_copy(a._h, 0, 0, host.ctypes.data_as(C.c_void_p), 1, None) == 0
    _same(host, before["levels"][0]["depth"], "host copy")
    for k in (a, c, again):
        k.close()
    ctx.close()


def test_a_handle_outlives_its_context(rs):
    lut = _lut(rs)
    ctx = rs.Context(0)
    kept = _keep(rs, "B", 0, dark=True, ctx=ctx)
    before = _planes(kept)
    pics = (kept.get_coloured_depth_maps(lut).cpu().numpy(), [t.cpu().numpy() for t in kept.get_coloured_depth_pyr(-1, lut)],
            [t.cpu().numpy() for t in kept.get_coloured_epi_pyr(-1, lut)])
    ctx.close()
    kept.ctx = rs.Context(0)                       # a fresh context of the same device
    _equal_planes(_planes(kept), before, "after the context")
    assert np.array_equal(kept.get_coloured_depth_maps(lut).cpu().numpy(), pics[0])
    for got, want in ((kept.get_coloured_depth_pyr(-1, lut), pics[1]), (kept.get_coloured_epi_pyr(-1, lut), pics[2])):
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    _kept_volume(kept, 0)
    kept.close()
    kept.ctx.close()


def test_a_failing_run_hands_nothing_out_and_the_next_one_succeeds(rs, oracle_mod):
    """The "sweep" site fails the first level on the host before its sweep is queued: the entry reports a status, *run is
    NULL, and the same call then succeeds with the yardstick's result."""
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    keep_alive, ptrs, dt, V, S, U, C_, stride = rs.host_epis(_epis(kr.make_field("A")), stride=True)
    ctx = rs.default_context()
    ctx.use_current_stream()
    p, st = rs.Depth1DParameters().to_c(), _lib.RslfStats()
    run = C.c_void_p(99)
    call = lambda: L.rslf_f2c_run_host(ctx._h, ptrs, 0, V, S, U, C_, stride, -1.0, 1.0, 9, -1.0, C.byref(p), -1, 1, 0, 0, 1, C.byref(run), C.byref(st))
    assert L.rslf_debug_inject(b"sweep", 1) == 0
    try:
        assert call() == -6 and run.value is None
        assert b"injected" in L.rslf_last_error()
    finally:
        assert L.rslf_debug_inject(b"sweep", 0) == 0
    # bad arguments leave NULL behind too
    run = C.c_void_p(99)
    assert L.rslf_f2c_run_host(ctx._h, ptrs, 3, V, S, U, C_, stride, -1.0, 1.0, 9, -1.0, C.byref(p), -1, 1, 0, 0, 1, C.byref(run), None) == INVALID
    assert run.value is None and b"element type" in L.rslf_last_error()
    run = C.c_void_p(99)
    assert L.rslf_f2c_run_host(ctx._h, ptrs, 0, V, S, U, C_, stride, -1.0, 1.0, 9, -1.0, C.byref(p), -1, 1, 0, 2, 1, C.byref(run), None) == INVALID
    assert run.value is None and b"validity rule" in L.rslf_last_error()
    run = C.c_void_p(99)
    assert call() == 0 and run.value
    kept = rs.KeptFineToCoarse(run, ctx, st)
    _check_against(kept, kr.reference(oracle_mod, "A", 0), "after a failed run")
    kept.close()
