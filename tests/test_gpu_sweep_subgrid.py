"""Sub-grid disparities in the 2-D sweep and the fine-to-coarse pyramid on the device (rslf_sweep_subgrid, the *_sub entries,
k9_subgrid_refine and its list form) against tests/sweep_subgrid_ref.py -- the oracle's sweep loop restated in numpy with
subgrid_ref.refine between a visit's scan and its selective median.  Every plane is compared bit for bit: disparities, C_d,
C_e, the edge masks, r-bar, the running masks and, where kept, C_l.

The planted field: 6 scanlines of peaks_ref's planted line, 5 views, 80 columns, 9 hypotheses in [-2, 2]."""
import ctypes as C

import numpy as np
import pytest

import f2c_keep_ref as kr
import line_conf_ref as lcr
import subgrid_ref as sr
import sweep_subgrid_ref as ssr

pytestmark = pytest.mark.gpu
F = np.float32
P = ssr.PLANTED
V, S, U, D, LO, HI = P["V"], P["S"], P["U"], P["D"], P["lo"], P["hi"]
ORDER = lcr.sweep_order(S)   # core.hpp:981-990: the centre view, then outwards
PLANES = ("depth", "disp_confidence", "edge_confidence", "edge_mask", "rbar", "scan_mask")
INVALID = -1
vp = C.c_void_p


@pytest.fixture(scope="module")
def rs():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from remotesensingproject_amd import depth
    return depth


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def _same(got, want, label):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (label, g.shape, w.shape, g.dtype, w.dtype)
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    if bad.size:
        at = np.unravel_index(bad[0], w.shape)
        raise AssertionError("%s: %d of %d values differ, first at %s: got %r want %r" % (
            label, bad.size, w.size, at, np.asarray(got)[at], np.asarray(want)[at]))


def _check(got, ref, label, line=False):
    for k in PLANES + (("line_confidence",) if line else ()):
        _same(got[k], ref[k], "%s: %s" % (label, k))


def _params(rs, mode=0, thr=0.02, use_disp=False, disp_thr=0.01, slope=1.0):
    return rs.Depth1DParameters(par_line_confidence_mode=mode, par_line_score_threshold=thr, par_use_disp_confidence_score=use_disp,
                                par_disp_score_threshold=disp_thr, par_slope_factor=slope)


class Sweep:
    """A volume on the device and a set of zeroed result planes; `call` runs a C entry on them."""

    def __init__(self, rs, vol_np, line=True, fill=0.0):
        import torch
        self.rs, self.torch = rs, torch
        self.vol = rs.Volume.from_dense(vol_np, 1.0, rs.default_context(0))
        self.ctx = self.vol.ctx
        n, C_ = (self.vol.S, self.vol.V, self.vol.U), self.vol.C
        f32 = lambda *s: torch.full(s, fill, dtype=torch.float32, device="cuda")
        self.t = dict(edge_confidence=f32(*n), edge_mask=torch.zeros(n, dtype=torch.uint8, device="cuda"), disp_confidence=f32(*n),
                      depth=f32(*n), rbar=f32(*n, C_), scan_mask=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                      line_confidence=f32(*n) if line else None)
        self.stats = None

    def ptr(self, k):
        return vp(None if self.t[k] is None else self.t[k].data_ptr())

    def run(self, name, par, *tail, lo=LO, hi=HI, dim_d=D):
        """rslf_depth2d_run / _lc / _sub: (ctx, vol, dmin, dmax, D, p, planes..., scan mask, stats, *tail)."""
        from remotesensingproject_amd import _lib
        L, p, st = _lib.lib(), par.to_c(), _lib.RslfStats()
        self.ctx.use_current_stream()
        rc = getattr(L, name)(self.ctx._h, self.vol._h, lo, hi, dim_d, C.byref(p), self.ptr("edge_confidence"), self.ptr("edge_mask"),
                              self.ptr("disp_confidence"), self.ptr("depth"), self.ptr("rbar"), self.ptr("scan_mask"), C.byref(st), *tail)
        self.stats = st
        return rc

    def planes(self):
        self.torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in self.t.items() if t is not None}


def run_sub(rs, vol_np, par, subgrid=1):
    sw = Sweep(rs, vol_np)
    mode = int(par.par_line_confidence_mode)
    from remotesensingproject_amd import _lib
    assert sw.run("rslf_depth2d_run_sub", par, mode, sw.ptr("line_confidence") if mode else None, subgrid) == 0, _lib.lib().rslf_last_error()
    return sw.planes(), sw.stats


# ---- 1: the planted line ---------------------------------------------------------------------------------------------------

CASE1 = [(0.37, 1), (1.3, 1), (0.37, 3)]


@pytest.mark.parametrize("d_true,C_", CASE1, ids=["d%g_C%d" % c for c in CASE1])
def test_planted_line(rs, oracle_mod, d_true, C_):
    """Through rslf_depth2d_run_sub and Depth2DComputer(subgrid=True): the reference's planes; they differ from the mode-off
    run's; a visit after the first refined at least one pixel (the list form ran on a non-empty list)."""
    ref, scanned, refined = ssr.planted_reference(oracle_mod, d_true, True, C=C_)
    grid = ssr.planted_reference(oracle_mod, d_true, False, C=C_)[0]
    assert sum(refined[1:]) >= 1, refined
    vol = ssr.planted_field(d_true, C_)
    got, st = run_sub(rs, vol, _params(rs))
    _check(got, ref, "rslf_depth2d_run_sub d=%g C=%d" % (d_true, C_))
    assert st.pixels_scanned == sum(scanned) and st.units == sum(scanned) * D
    off, st0 = run_sub(rs, vol, _params(rs), subgrid=0)
    _check(off, grid, "subgrid = 0 against the grid reference")
    assert not np.array_equal(_bits(got["depth"]), _bits(off["depth"]))
    m = ref["edge_mask"] != 0
    assert (got["depth"][m] != off["depth"][m]).mean() > 0.9
    comp = rs.Depth2DComputer(vol, LO, HI, D, epi_scale_factor=1.0, subgrid=True)
    comp.run()
    _check(comp.results(), ref, "Depth2DComputer(subgrid=True)")
    assert comp.stats.pixels_scanned == sum(scanned)
    # the getters show the refined plane
    import render_ref as rr
    lut = rs.colormap_jet()
    assert np.array_equal(comp.get_disparity_map(-1, lut).cpu().numpy(), rr.disparity_map(ref["depth"][S // 2], ref["edge_mask"][S // 2], lut))


# ---- 2 and 3: long lists, both forms, the fallbacks --------------------------------------------------------------------------

def _long_params(rs):
    return _params(rs, use_disp=True, disp_thr=1.0)


def test_long_lists(rs, oracle_mod):
    """use_disp_confidence_score with a threshold above every C_d: nothing is painted, each of the five visits scans 367-380
    pixels -- more than one workgroup of list entries, a partial last one, entries on every scanline."""
    ref, scanned, refined = ssr.planted_reference(oracle_mod, 0.37, True, use_disp=True, disp_thr=1.0)
    assert all(367 <= n <= 380 for n in scanned) and refined == scanned
    assert (np.stack([ref["edge_mask"][s].any(axis=1) for s in range(S)])).all()   # entries on every scanline of every view
    got, st = run_sub(rs, ssr.planted_field(0.37), _long_params(rs))
    _check(got, ref, "long lists")
    assert st.pixels_scanned == sum(scanned)


HOOKS = [dict(subgrid_list=0), dict(force_packed=0), dict(subgrid_list=0, force_packed=0)]


FORM_CASES = [c + (False,) for c in CASE1] + [(0.37, 1, True)]   # every field of case 1, and case 2's long lists


@pytest.mark.parametrize("hook", HOOKS, ids=["_".join("%s%d" % kv for kv in h.items()) for h in HOOKS])
@pytest.mark.parametrize("d_true,C_,long_lists", FORM_CASES, ids=["d%g_C%d%s" % (d, c, "_long" if l else "") for d, c, l in FORM_CASES])
def test_both_forms_and_the_fallbacks(rs, oracle_mod, hooks, d_true, C_, long_lists, hook):
    """"subgrid_list" = 0 (every visit the dense form) and "force_packed" = 0 (no packed list: the dense form) give the
    default's planes, plane by plane -- and so the reference's -- on every field of case 1 and on case 2."""
    par = _long_params(rs) if long_lists else _params(rs)
    ref = ssr.planted_reference(oracle_mod, d_true, True, C=C_, **(dict(use_disp=True, disp_thr=1.0) if long_lists else {}))[0]
    vol = ssr.planted_field(d_true, C_)
    default, _ = run_sub(rs, vol, par)
    hooks(**hook)
    got, _ = run_sub(rs, vol, par)
    label = "d=%g C=%d%s under %s" % (d_true, C_, " long" if long_lists else "", hook)
    for k in PLANES:
        _same(got[k], default[k], "%s: %s" % (label, k))
    _check(got, ref, label)


# ---- 4: per-pixel ranges -----------------------------------------------------------------------------------------------------

def _ranges():
    """Seeded per-pixel [lo, hi] inside [-2, 2] over [S, V, U], lo == hi on every 7th pixel."""
    rng = np.random.default_rng(77)
    lo = rng.uniform(LO, 0.0, size=(S, V, U)).astype(F)
    hi = np.minimum((lo + rng.uniform(0.5, 2.5, size=(S, V, U)).astype(F)).astype(F), F(HI))
    flat = (np.arange(S * V * U).reshape(S, V, U) % 7) == 0
    hi[flat] = lo[flat]
    return lo, hi


RANGE_CASES = [(9, 1.0), (2, 1.0), (3, 0.5)]
_range_cache = {}


@pytest.mark.parametrize("dim_d,slope", RANGE_CASES, ids=["D%d_slope%g" % c for c in RANGE_CASES])
def test_per_pixel_ranges(rs, oracle_mod, dim_d, slope):
    """rslf_depth_epi_2d_sub (compute_2D_depth_epi(subgrid=True)) with range planes, lo == hi on every 7th pixel; D = 2 (no
    interior hypothesis: every refined value is its grid value) and D = 3; slope_factor = 0.5."""
    import torch
    lo, hi = _ranges()
    vol = ssr.planted_field(0.37)
    if (dim_d, slope) not in _range_cache:
        p = oracle_mod.default_params()
        p.slope_factor = slope
        _range_cache[(dim_d, slope)] = ssr.sweep(oracle_mod, vol, lo, hi, dim_d, p, subgrid=True)
    ref, scanned, refined = _range_cache[(dim_d, slope)]
    assert sum(refined) >= 300
    sw = Sweep(rs, vol, line=False)
    par = _params(rs, slope=slope)
    sw.t["edge_mask"] = rs.compute_2D_edge_confidence(sw.vol, sw.t["edge_confidence"], par)
    dev = lambda a: torch.from_numpy(a).cuda()
    st = rs.compute_2D_depth_epi(sw.vol, dev(lo), dev(hi), dim_d, sw.t["edge_confidence"], sw.t["edge_mask"], sw.t["disp_confidence"],
                                 sw.t["depth"], sw.t["rbar"], par, scan_mask_s_v_u=sw.t["scan_mask"], want_stats=True, subgrid=True)
    got = sw.planes()
    _check(got, ref, "ranges D=%d slope=%g" % (dim_d, slope))
    assert st.pixels_scanned == sum(scanned)
    flat = (lo == hi) & (ref["edge_mask"] != 0) & (ref["scan_mask"] == 0)
    assert flat.sum() >= 20


# ---- 5: line confidence ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("d_true,C_", CASE1, ids=["d%g_C%d" % c for c in CASE1])
def test_line_confidence(rs, oracle_mod, d_true, C_, mode):
    """Modes 1 and 2 with the sub-grid mode on every field of case 1: one arg-max plane serves K7 and K9 (with three channels
    k7_line_confidence<3> and k9_subgrid_refine<3, ...>); C_l is the reference's too."""
    thr = 0.02
    ref = ssr.planted_reference(oracle_mod, d_true, True, C=C_, mode=mode, thr=thr)[0]
    assert (ref["line_confidence"] > 0).any()
    vol = ssr.planted_field(d_true, C_)
    label = "d=%g C=%d line mode %d" % (d_true, C_, mode)
    got, _ = run_sub(rs, vol, _params(rs, mode=mode, thr=thr))
    _check(got, ref, label, line=True)
    comp = rs.Depth2DComputer(vol, LO, HI, D, epi_scale_factor=1.0, parameters=_params(rs, mode=mode, thr=thr), subgrid=True)
    comp.run()
    _check(comp.results(), ref, "Depth2DComputer, " + label, line=True)


# ---- 6: the visit API ----------------------------------------------------------------------------------------------------------

def _visits(L, sw, p, subgrid, first_call=None):
    """begin -> [rslf_sweep_subgrid] -> visits -> end on a Sweep's planes (edge confidence computed, the rest zero)."""
    ctx, vol, t = sw.ctx, sw.vol, sw.t
    assert L.rslf_sweep_begin(ctx._h, vol._h, sw.ptr("edge_mask"), sw.ptr("scan_mask"), D, 0, V) == 0, L.rslf_last_error()
    if subgrid is not None:
        assert L.rslf_sweep_subgrid(ctx._h, vol._h, subgrid) == 0, L.rslf_last_error()
    for s_hat in ORDER:
        assert L.rslf_sweep_visit_scan(ctx._h, vol._h, None, None, LO, HI, D, s_hat, sw.ptr("edge_confidence"), sw.ptr("edge_mask"),
                                       sw.ptr("disp_confidence"), sw.ptr("depth"), sw.ptr("rbar"), C.byref(p)) == 0, L.rslf_last_error()
        if first_call is not None:
            first_call()
            first_call = None
        assert L.rslf_sweep_visit_finish(ctx._h, vol._h, s_hat, sw.ptr("edge_mask"), sw.ptr("disp_confidence"), sw.ptr("depth"),
                                         sw.ptr("rbar"), C.byref(p)) == 0, L.rslf_last_error()
    assert L.rslf_sweep_end(ctx._h, 1, D, None) == 0


def _prepared(rs, vol_np, par):
    sw = Sweep(rs, vol_np, line=False)
    sw.t["edge_mask"] = rs.compute_2D_edge_confidence(sw.vol, sw.t["edge_confidence"], par)
    return sw


def test_visit_api(rs, oracle_mod):
    """begin -> rslf_sweep_subgrid -> visits -> end equals the one-call entry; the calls outside the window and on = 2 give a
    status and a message and launch nothing; the mode does not outlive rslf_sweep_end."""
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    par = _params(rs)
    p = par.to_c()
    vol = ssr.planted_field(0.37)
    ref = ssr.planted_reference(oracle_mod, 0.37, True)[0]
    grid = ssr.planted_reference(oracle_mod, 0.37, False)[0]

    sw = _prepared(rs, vol, par)
    ctx, dev = sw.ctx, sw.vol
    ctx.use_current_stream()
    # before begin: refused
    assert L.rslf_sweep_subgrid(ctx._h, dev._h, 1) == INVALID and b"rslf_sweep_begin" in L.rslf_last_error()
    assert L.rslf_sweep_subgrid(None, dev._h, 1) == INVALID and L.rslf_sweep_subgrid(ctx._h, None, 1) == INVALID
    # on = 2, on = -1: refused inside the window, and the sweep stays out of the mode
    assert L.rslf_sweep_begin(ctx._h, dev._h, sw.ptr("edge_mask"), sw.ptr("scan_mask"), D, 0, V) == 0
    assert L.rslf_sweep_subgrid(ctx._h, dev._h, 2) == INVALID and b"on=2" in L.rslf_last_error()
    assert L.rslf_sweep_subgrid(ctx._h, dev._h, -1) == INVALID
    assert L.rslf_sweep_subgrid(ctx._h, dev._h, 1) == 0 and L.rslf_sweep_subgrid(ctx._h, dev._h, 0) == 0   # on, then off again
    assert L.rslf_sweep_end(ctx._h, 0, D, None) == 0
    sw.torch.cuda.synchronize()
    for k in ("depth", "disp_confidence", "rbar"):
        assert not sw.t[k].any().item(), k   # nothing was launched on the planes

    # the mode on, through the visits; after the first visit's scan the call is refused and changes nothing
    def late():
        assert L.rslf_sweep_subgrid(ctx._h, dev._h, 0) == INVALID and b"first visit" in L.rslf_last_error()

    _visits(L, sw, p, 1, first_call=late)
    _check(sw.planes(), ref, "the visit API, mode on")
    assert L.rslf_sweep_subgrid(ctx._h, dev._h, 1) == INVALID   # the sweep is closed

    # the mode did not outlive rslf_sweep_end: the next sweep on the same context gives the grid planes, through the visits
    # and through the one-call entry
    sw2 = _prepared(rs, vol, par)
    assert sw2.ctx is ctx
    _visits(L, sw2, p, None)
    _check(sw2.planes(), grid, "a sweep after a sub-grid sweep, same context")
    sw3 = Sweep(rs, vol, line=False)
    assert sw3.run("rslf_depth2d_run", par) == 0
    _check(sw3.planes(), grid, "rslf_depth2d_run after a sub-grid sweep")
    # a sweep left open in the mode by an error path: begin starts the next one out of it
    assert L.rslf_sweep_begin(ctx._h, dev._h, sw.ptr("edge_mask"), sw.ptr("scan_mask"), D, 0, V) == 0
    assert L.rslf_sweep_subgrid(ctx._h, dev._h, 1) == 0
    sw4 = _prepared(rs, vol, par)
    _visits(L, sw4, p, None)
    _check(sw4.planes(), grid, "begin over an open sub-grid sweep")
    # the one-call entries refuse a bad flag before anything is queued
    sw5 = Sweep(rs, vol, line=False, fill=-7.0)
    assert sw5.run("rslf_depth2d_run_sub", par, 0, None, 2) == INVALID and b"subgrid" in L.rslf_last_error()
    assert L.rslf_depth2d_run_host_sub(ctx._h, dev._h, LO, HI, D, C.byref(p), None, None, None, None, None, None, 0, None, 3) == INVALID
    assert (sw5.planes()["depth"] == -7.0).all()


# ---- 7: mode off ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
def test_mode_off_is_the_namesake(rs, mode):
    """rslf_depth2d_run_sub, rslf_depth_epi_2d_sub and rslf_depth2d_run_host_sub with 0: the _lc entry's planes, bit for bit."""
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    vol = ssr.planted_field(0.37)
    par = _params(rs, mode=mode)
    p = par.to_c()
    a, b = Sweep(rs, vol), Sweep(rs, vol)
    cl = lambda sw: sw.ptr("line_confidence") if mode else None
    assert a.run("rslf_depth2d_run_lc", par, mode, cl(a)) == 0 and b.run("rslf_depth2d_run_sub", par, mode, cl(b), 0) == 0
    pa, pb = a.planes(), b.planes()
    for k in pa:
        _same(pb[k], pa[k], "rslf_depth2d_run_sub(0): %s" % k)
    assert a.stats.pixels_scanned == b.stats.pixels_scanned
    # the sweep alone, on prepared planes
    out = []
    for name, tail in (("rslf_depth_epi_2d_lc", ()), ("rslf_depth_epi_2d_sub", (0,))):
        sw = _prepared(rs, vol, par)
        if mode:
            sw.t["line_confidence"] = sw.torch.zeros_like(sw.t["depth"])
        sw.ctx.use_current_stream()
        rc = getattr(L, name)(sw.ctx._h, sw.vol._h, None, None, LO, HI, D, sw.ptr("edge_confidence"), sw.ptr("edge_mask"),
                              sw.ptr("disp_confidence"), sw.ptr("depth"), sw.ptr("rbar"), C.byref(p), sw.ptr("scan_mask"), None, mode,
                              sw.ptr("line_confidence") if mode else None, *tail)
        assert rc == 0, L.rslf_last_error()
        out.append(sw.planes())
    for k in out[0]:
        _same(out[1][k], out[0][k], "rslf_depth_epi_2d_sub(0): %s" % k)
        _same(out[0][k], pa[k], "the sweep alone: %s" % k)
    # host planes out
    host = []
    for name, tail in (("rslf_depth2d_run_host_lc", ()), ("rslf_depth2d_run_host_sub", (0,))):
        h = dict(edge_confidence=np.empty((S, V, U), F), edge_mask=np.empty((S, V, U), np.uint8), disp_confidence=np.empty((S, V, U), F),
                 depth=np.empty((S, V, U), F), rbar=np.empty((S, V, U, 1), F), line_confidence=np.zeros((S, V, U), F))
        hp = [h[k].ctypes.data_as(vp) for k in ("edge_confidence", "edge_mask", "disp_confidence", "depth", "rbar")]
        rc = getattr(L, name)(a.ctx._h, a.vol._h, LO, HI, D, C.byref(p), *hp, None, mode,
                              h["line_confidence"].ctypes.data_as(vp) if mode else None, *tail)
        assert rc == 0, L.rslf_last_error()
        host.append(h)
    for k in host[0]:
        _same(host[1][k], host[0][k], "rslf_depth2d_run_host_sub(0): %s" % k)
        if k != "line_confidence" or mode:
            _same(host[0][k], pa[k], "host planes: %s" % k)


def _f2c_args(rs, field, dim_d, par, accept, line_mode, levels=None):
    """The argument tuples of the host pyramid entries for a raw field [V,S,U,C]."""
    from remotesensingproject_amd import _lib
    epis = list(field[..., 0]) if field.shape[3] == 1 else list(field)
    keep, ptrs, dt, V_, S_, U_, C_, stride = rs.host_epis(epis, stride=True)
    out_map, out_valid = np.empty((S_, V_, U_), F), np.empty((S_, V_, U_), np.uint8)
    p, st, nl = par.to_c(), _lib.RslfStats(), C.c_int()
    rest = (V_, S_, U_, C_, stride, -1.0, 1.0, dim_d, -1.0, C.byref(p), -1, 1 if accept else 0, out_map.ctypes.data_as(vp),
            out_valid.ctypes.data_as(vp), C.byref(nl), C.byref(st), line_mode, None)
    return dict(keep=(keep, p, st, nl), ptrs=ptrs, dt=dt, rest=rest, out_map=out_map, out_valid=out_valid, stats=st)


def test_mode_off_pyramid_entries_are_the_namesakes(rs):
    """rslf_fine_to_coarse_run_host_sub and rslf_f2c_run_host_sub with 0 against rslf_fine_to_coarse_run_host_lc and
    rslf_f2c_run_host: the fused planes and every kept plane, bit for bit; rslf_f2c_run_subgrid reads 0."""
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    ctx = rs.default_context(0)
    ctx.use_current_stream()
    field = kr.make_field("B")
    _, _, _, _, _, dim_d, accept = kr.case_of("B")
    par = _params(rs)
    a = _f2c_args(rs, field, dim_d, par, accept, 0)
    assert L.rslf_fine_to_coarse_run_host_lc(ctx._h, a["ptrs"], 1, *a["rest"]) == 0, L.rslf_last_error()
    b = _f2c_args(rs, field, dim_d, par, accept, 0)
    assert L.rslf_fine_to_coarse_run_host_sub(ctx._h, b["ptrs"], 1, *b["rest"], 0) == 0, L.rslf_last_error()   # RSLF_ELEM_U8 = 1
    _same(b["out_map"], a["out_map"], "rslf_fine_to_coarse_run_host_sub(0): fused map")
    _same(b["out_valid"], a["out_valid"], "rslf_fine_to_coarse_run_host_sub(0): fused validity")
    assert a["stats"].pixels_scanned == b["stats"].pixels_scanned
    assert L.rslf_fine_to_coarse_run_host_sub(ctx._h, b["ptrs"], 1, *b["rest"], 2) == INVALID and b"subgrid" in L.rslf_last_error()
    assert L.rslf_fine_to_coarse_run_host_sub(ctx._h, b["ptrs"], 7, *b["rest"], 0) == INVALID
    epis = list(field)
    kept = rs.fine_to_coarse_run_host(epis, -1.0, 1.0, dim_d, parameters=par, accept_all_last_scale=accept, keep=True)
    assert kept.subgrid is False and L.rslf_f2c_run_subgrid(None) == 0
    h, st, p = vp(), _lib.RslfStats(), par.to_c()
    keep_alive, ptrs, dt, V_, S_, U_, C_, stride = rs.host_epis(epis, stride=True)
    rc = L.rslf_f2c_run_host_sub(ctx._h, ptrs, 1, V_, S_, U_, C_, stride, -1.0, 1.0, dim_d, -1.0, C.byref(p), -1, 1 if accept else 0, 0, 0, 1,
                                 C.byref(h), C.byref(st), 0)
    assert rc == 0, L.rslf_last_error()
    other = rs.KeptFineToCoarse(h, ctx, st)
    assert other.subgrid is False and other.dims == kept.dims
    for l in range(kept.n_levels):
        for k in ("depth", "valid", "Ce", "Cd"):
            _same(other.plane(l, k).cpu().numpy(), kept.plane(l, k).cpu().numpy(), "rslf_f2c_run_host_sub(0): level %d %s" % (l, k))
    _same(other.get_results()[0].cpu().numpy(), a["out_map"], "the kept run's fused map")
    kept.close()
    other.close()


# ---- 8: the pyramid ------------------------------------------------------------------------------------------------------------

def _epis(field):
    return list(field[..., 0]) if field.shape[3] == 1 else list(field)


def _check_levels(levels, ref, label):
    for l, (lv, rv) in enumerate(zip(levels, ref["levels"])):
        _same(lv["depth"], rv["depth"], "%s: level %d depth" % (label, l))
        _same(lv["valid"], rv["valid"], "%s: level %d validity" % (label, l))
        _same(lv["edge_confidence"], rv["edge_confidence"], "%s: level %d C_e" % (label, l))


@pytest.mark.parametrize("name", ["A", "B", "U16"])
def test_pyramid(rs, oracle_mod, name):
    """Every level's planes through levels_out, the fused map and validity, against the reference's pyramid on the sub-grid
    sweep: rslf_fine_to_coarse_run_host_sub; a kept run (rslf_f2c_run_subgrid == 1) and its coloured depth maps against
    render_ref on the reference's planes; FineToCoarse(subgrid=True), the Python level loop.  Some level's dmin / dmax plane
    holds an off-grid value: the tightening consumed refined disparities."""
    C_, elem, V_, U_, S_, dim_d, accept = kr.case_of(name)
    field = kr.make_field(name)
    ref = ssr.f2c_reference(oracle_mod, name, True)
    grid_ref = kr.reference(oracle_mod, name)
    assert not np.array_equal(_bits(ref["fused_map"]), _bits(grid_ref["fused_map"]))
    assert all(sum(lv["refined"][1:]) >= 1 for lv in ref["levels"])
    grid_values = np.array([sr.grid_value(i, dim_d, -1.0, 1.0) for i in range(dim_d)], F)
    off_grid = sum(int((~np.isin(lv[k], grid_values)).sum()) for lv in ref["levels"][1:] for k in ("dmin", "dmax"))
    flat = sum(int((lv["dmin"] == lv["dmax"]).sum()) for lv in ref["levels"][1:])
    assert off_grid >= 100 and flat >= 100, (off_grid, flat)
    par = _params(rs)

    out = rs.fine_to_coarse_run_host(_epis(field), -1.0, 1.0, dim_d, parameters=par, accept_all_last_scale=accept, want_levels=True,
                                     subgrid=True)
    assert out["n_levels"] == len(ref["dims"]) == 3
    _check_levels(out["levels"], ref, "%s rslf_fine_to_coarse_run_host_sub" % name)
    _same(out["out_map"], ref["fused_map"], "fused map")
    _same(out["out_valid"], ref["fused_valid"], "fused validity")
    assert out["stats"].pixels_scanned == ref["pixels_scanned"]
    if name == "U16":
        return   # one u16 run: the entry has no u16 twin, the element type goes in `elem`

    kept = rs.fine_to_coarse_run_host(_epis(field), -1.0, 1.0, dim_d, parameters=par, accept_all_last_scale=accept, keep=True, subgrid=True)
    assert kept.subgrid is True and kept.dims == ref["dims"]
    for l, rv in enumerate(ref["levels"]):
        for k, rk in (("depth", "depth"), ("valid", "valid"), ("Ce", "edge_confidence"), ("Cd", "disp_confidence")):
            _same(kept.plane(l, k).cpu().numpy(), rv[rk], "kept run: level %d %s" % (l, k))
    fm, fv = [t.cpu().numpy() for t in kept.get_results()]
    _same(fm, ref["fused_map"], "kept run: fused map")
    _same(fv, ref["fused_valid"], "kept run: fused validity")
    lut = rs.colormap_jet()
    level = float(F(oracle_mod.default_params().shadow_level))
    for saturate in (True, False):
        want = kr.pictures([lv["depth"] for lv in ref["levels"]], [lv["valid"] for lv in ref["levels"]], ref["fused_map"], ref["fused_valid"],
                           lut, ref["volumes"], level, saturate)
        assert np.array_equal(kept.get_coloured_depth_maps(lut, saturate).cpu().numpy(), want["maps"]), ("maps", saturate)
    kept.close()

    loop = rs.FineToCoarse(_epis(field), -1.0, 1.0, dim_d, parameters=par, accept_all_last_scale=accept, subgrid=True)
    loop.run()
    assert len(loop.m_computers) == 3 and all(c.m_subgrid for c in loop.m_computers)
    for l, (comp, rv) in enumerate(zip(loop.m_computers, ref["levels"])):
        got = comp.results()
        for k in PLANES:
            _same(got[k], rv[k], "FineToCoarse(subgrid=True): level %d %s" % (l, k))
        _same(comp.get_valid_depths_mask_s_v_u().cpu().numpy(), rv["valid"], "level %d validity" % l)
        if l > 0:   # the ranges the level was swept in: tightened from refined disparities
            _same(comp.m_dmin_s_v_u.cpu().numpy(), rv["dmin"], "level %d dmin" % l)
            _same(comp.m_dmax_s_v_u.cpu().numpy(), rv["dmax"], "level %d dmax" % l)
    fm, fv = [t.cpu().numpy() for t in loop.get_results()]
    _same(fm, ref["fused_map"], "FineToCoarse(subgrid=True): fused map")
    _same(fv, ref["fused_valid"], "FineToCoarse(subgrid=True): fused validity")
    assert np.array_equal(loop.get_coloured_depth_maps(lut).cpu().numpy(), kr.pictures(
        [lv["depth"] for lv in ref["levels"]], [lv["valid"] for lv in ref["levels"]], ref["fused_map"], ref["fused_valid"], lut,
        ref["volumes"], level, True)["maps"])


# ---- 9: refusals ---------------------------------------------------------------------------------------------------------------

def test_multi_device_forms_refuse_the_mode(rs):
    """Every multi-device form raises before a device is touched (MultiDevice([0]) itself needs one)."""
    from remotesensingproject_amd import sharding
    vol = ssr.planted_field(0.37)
    epis = list(vol[..., 0])
    md = rs.MultiDevice([0])
    with pytest.raises(ValueError, match="subgrid"):
        md.depth2d(epis, LO, HI, D, subgrid=True)
    with pytest.raises(ValueError, match="subgrid"):
        md.fine_to_coarse(_epis(kr.make_field("A")), -1.0, 1.0, D, subgrid=True)
    md.close()
    dev = rs.Volume.from_dense(vol, 1.0, rs.default_context(0))
    with pytest.raises(ValueError, match="subgrid"):
        sharding.ShardedDepth2D(dev, sharding.make_shard(V, 0, 1), LO, HI, D, subgrid=True)
    with pytest.raises(ValueError, match="subgrid"):
        sharding.ShardedFineToCoarse(_epis(kr.make_field("A")), -1.0, 1.0, D, 0, 1, subgrid=True)
