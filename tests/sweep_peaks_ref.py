"""The yardstick of the 2-D sweep's peaks mode (include/rslf_hip.h, rslf_sweep_peaks and the *_pk entries below it): numpy,
written from that text and composed of public pieces.  Never the HIP path against itself.

`sweep` restates the loop of tests/sweep_subgrid_ref.sweep -- per-pixel ranges, the three line modes, gating by C_d, the
sub-grid step -- and adds the mode: for every pixel a visit scanned and accepted (the visit's idx >= 0), oracle_np.scan_pixel's
score row goes through peaks_ref.peaks_ref, the rule's restatement, and its idx, score, runner_idx and runner_score land in
four planes [S, V, U]; the apply step copies the source's four values with the disparity, C_d and C_l.  Every other pixel
keeps what the planes held at the start (`fill`: -1 / 0, what the *_run entries put there, or the caller's planes).  The mode
changes no other plane: `sweep` returns them all, and tests/test_sweep_peaks_cpu.py holds them to sweep_subgrid_ref's.

Also: the pixels every visit scanned and accepted, as masks -- what the GPU tests check the winner and the centre view on."""
import numpy as np

import line_conf_ref as lcr
import peaks_ref as pr
import subgrid_ref as sr
import sweep_subgrid_ref as ssr
from oracle import oracle_np as onp

F = np.float32
PLANES = ("idx", "score", "runner_idx", "runner_score")


def empty_planes(S, V, U):
    """What the *_run entries fill before the first visit: no index, and 0."""
    return dict(idx=np.full((S, V, U), -1, np.int32), score=np.zeros((S, V, U), F),
                runner_idx=np.full((S, V, U), -1, np.int32), runner_score=np.zeros((S, V, U), F))


def row_peaks(vol_v, u, lo, hi, D, s_hat, pd):
    """(idx, score, runner_idx, runner_score) of pixel u of EPI vol_v [S, U, C]: oracle_np.scan_pixel's row through the rule."""
    row = onp.scan_pixel(vol_v, int(u), lo, hi, D, s_hat, pd)[1]
    i1, s1, _, i2, s2 = pr.peaks_ref(row, lo, hi)
    return i1, s1, i2, s2


def sweep(oracle, vol, dmin_svu, dmax_svu, D, p, mode=0, line_score_threshold=0.02, propagation_epsilon=0.1, subgrid=False,
          fill=None, v_lo=0, v_hi=None):
    """compute_2D_edge_confidence + compute_2D_depth_epi in the peaks mode on a normalised volume [V,S,U,C] with per-pixel
    ranges [S,V,U].  Returns (planes, peak planes, accepted): `planes` as sweep_subgrid_ref.sweep's, the four peak planes as
    a dict, and per visit (in sweep order) the pair (s_hat, mask [V, U] of the pixels the visit scanned and accepted).
    v_lo, v_hi: the active scanlines of rslf_sweep_begin (the others are never scanned and never painted)."""
    vol = np.ascontiguousarray(vol, F)
    V, S, U, C = vol.shape
    v_hi = V if v_hi is None else v_hi
    pd = ssr.params_dict(p)
    Ce = np.zeros((S, V, U), F); cm = np.zeros((S, V, U), np.uint8)
    for s in range(S):
        Ce[s], cm[s] = oracle.edge_confidence_pile(vol, s, p)
    Cd = np.zeros((S, V, U), F); depth = np.zeros((S, V, U), F); rbar = np.zeros((S, V, U, C), F)
    Cl = np.zeros((S, V, U), F)
    K = np.zeros((V, S, U), F)
    mask = cm.copy()
    mask[:, :v_lo] = 0
    mask[:, v_hi:] = 0
    pk = empty_planes(S, V, U) if fill is None else {k: fill[k].copy() for k in PLANES}
    slope = F(p.slope_factor)
    thr_line = F(line_score_threshold); thr_disp = F(p.disp_score_threshold)
    eps = F(propagation_epsilon)
    accepted = []
    for s_hat in lcr.sweep_order(S):
        idx = np.full((V, U), -1, np.int32)
        for v in range(V):
            r = oracle.depth_epi(vol[v], dmin_svu[s_hat, v], dmax_svu[s_hat, v], D, s_hat, Ce[s_hat, v], cm[s_hat, v], p,
                                 mask_u=mask[s_hat, v], want_K=True)
            mask[s_hat, v] = cm[s_hat, v] & mask[s_hat, v]
            Ce[s_hat, v], cm[s_hat, v] = r["Ce"], r["Ce_mask"]
            sel = r["idx"] >= 0
            Cd[s_hat, v][sel] = r["Cd"][sel]
            depth[s_hat, v][sel] = r["depth"][sel]
            rbar[s_hat, v][sel] = r["rbar"][sel]
            K[v][:, sel] = r["K"][:, sel]
            idx[v] = r["idx"]
        got = idx >= 0
        if subgrid:
            disp = sr.refine(vol, idx, dmin_svu[s_hat], dmax_svu[s_hat], D, s_hat, pd)[0]
            depth[s_hat][got] = disp[got]
        # the step this file adds: the peaks of the pixels this visit scanned and accepted
        for v, u in zip(*np.nonzero(got)):
            i1, s1, i2, s2 = row_peaks(vol[v], u, dmin_svu[s_hat, v, u], dmax_svu[s_hat, v, u], D, s_hat, pd)
            pk["idx"][s_hat, v, u], pk["score"][s_hat, v, u] = i1, s1
            pk["runner_idx"][s_hat, v, u], pk["runner_score"][s_hat, v, u] = i2, s2
        accepted.append((s_hat, got.copy()))
        filtered = oracle.selective_median(depth[s_hat], vol, s_hat, cm[s_hat], p.median_filter_size, F(p.median_filter_epsilon))
        if mode != 0:
            lcr.line_confidence_visit(Ce, K, filtered, cm[s_hat], s_hat, Cl[s_hat])
        if p.use_disp_confidence_score:                                   # core.hpp:1097-1103
            src = Cd[s_hat] > thr_disp
        elif mode == 2:
            src = Cl[s_hat] > thr_line
        else:
            src = cm[s_hat] != 0
        for v, u in zip(*np.nonzero(src)):                                # row-major, as the loops of :1088-1129 run
            cur = filtered[v, u]
            cd_u, cl_u = Cd[s_hat, v, u], Cl[s_hat, v, u]
            pk_u = tuple(pk[k][s_hat, v, u] for k in PLANES)
            for s in range(S):
                off = F(F(cur * F(s_hat - s)) * slope)                    # :1109
                if not np.isfinite(off):
                    continue
                ri = u + int(np.sign(off) * np.floor(np.abs(np.float64(off)) + 0.5))   # std::round, the sum in double
                if -1 < ri < U and mask[s, v, ri]:
                    if lcr._norm((vol[v, s, ri] - rbar[s_hat, v, u])[None])[0] < eps:
                        depth[s, v, ri] = cur
                        mask[s, v, ri] = 0
                        Cd[s, v, ri] = cd_u
                        if mode != 0:
                            Cl[s, v, ri] = cl_u                           # :1122-1124
                        for k, val in zip(PLANES, pk_u):                  # the source's peaks travel with the disparity
                            pk[k][s, v, ri] = val
    planes = dict(edge_confidence=Ce, edge_mask=cm, disp_confidence=Cd, depth=depth, rbar=rbar, scan_mask=mask,
                  line_confidence=Cl)
    return planes, pk, accepted


_cache = {}


def planted_reference(oracle, d_true, C=1, mode=0, subgrid=False, use_disp=False, disp_thr=None, thr=0.02, D=None, slope=None,
                      interp=None, ranges=None):
    """`sweep` on sweep_subgrid_ref's planted field, computed once per session and shared (callers must not write into it).
    D: hypotheses (default the field's 9); slope: slope_factor; interp: the interpolation mode; ranges: None for the field's
    scalar range, or a name of RANGES -- per-pixel planes."""
    key = (float(d_true), C, mode, bool(subgrid), bool(use_disp), disp_thr, float(thr), D, slope, interp, ranges)
    if key not in _cache:
        p = oracle.default_params()
        p.use_disp_confidence_score = int(use_disp)
        if disp_thr is not None:
            p.disp_score_threshold = disp_thr
        if slope is not None:
            p.slope_factor = slope
        if interp is not None:
            p.interpolation = interp
        vol = ssr.planted_field(d_true, C)
        lo, hi = range_planes(ranges)
        _cache[key] = sweep(oracle, vol, lo, hi, D or ssr.PLANTED["D"], p, mode, thr, subgrid=subgrid)
    return _cache[key]


def range_planes(name):
    """The [S, V, U] range planes of the planted field: None -> the field's scalar range everywhere; "mixed" -> columns in
    four bands: the whole range, lo == hi (a constant row: every hypothesis is the same disparity), a range whose winner sits
    at its first hypothesis (it ends at the planted disparity's far side) and one whose winner sits at its last."""
    S, V, U = ssr.PLANTED["S"], ssr.PLANTED["V"], ssr.PLANTED["U"]
    lo = np.full((S, V, U), ssr.PLANTED["lo"], F); hi = np.full((S, V, U), ssr.PLANTED["hi"], F)
    if name is None:
        return lo, hi
    assert name == "mixed"
    u = np.arange(U)
    flat, first, last = (u % 4 == 1), (u % 4 == 2), (u % 4 == 3)
    lo[..., flat] = F(0.4); hi[..., flat] = F(0.4)
    lo[..., first] = F(0.5); hi[..., first] = F(2.0)     # the planted 0.37 lies below the range: the first hypothesis is nearest
    lo[..., last] = F(-2.0); hi[..., last] = F(0.25)     # ... above it: the last
    return lo, hi
