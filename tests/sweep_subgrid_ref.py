"""The yardstick of the sub-grid 2-D sweep and pyramid (include/rslf_hip.h, rslf_sweep_subgrid and the *_sub entries below
it): numpy, written from that text and composed of public pieces.  Never the HIP path against itself.

`sweep` restates the loop of tests/f2c_line_conf_ref.sweep -- per-pixel ranges, the three line modes, gating by C_d -- with
one step more per visit: for the pixels the visit's depth_epi gave an idx >= 0, subgrid_ref.refine (oracle_np.scan_pixel's
row through the rule) replaces the raw disparity before selective_median.  Everything downstream then reads refined floats:
the median, the propagation's columns u + round(d * (s_hat - s) * slope), the line confidence's positions.  rbar, the K
columns, C_d, C_e and the masks stay what the scan wrote.  With the mode on the sweep is a different computation -- which
pixels later visits still scan changes -- so it reports the pixels every visit scanned and refined.

`fine_to_coarse` is f2c_line_conf_ref.fine_to_coarse on that sweep: tighten_bounds, the validity rules and the fusion are the
oracle's, and receive off-grid disparities.  Also the planted-line field the CPU and GPU tests share."""
import numpy as np

import f2c_keep_ref as fkr
import f2c_line_conf_ref as flr
import line_conf_ref as lcr
import peaks_ref as pr
import subgrid_ref as sr

F = np.float32


def params_dict(p):
    """The oracle's parameter structure as the dict oracle_np.scan_pixel reads."""
    return dict(kernel_bandwidth=F(p.kernel_bandwidth), slope_factor=F(p.slope_factor), interpolation=int(p.interpolation),
                mean_shift_max_iter=F(p.mean_shift_max_iter), raw_score_threshold=F(p.raw_score_threshold))


def sweep(oracle, vol, dmin_svu, dmax_svu, D, p, mode=0, line_score_threshold=0.02, propagation_epsilon=0.1, subgrid=False):
    """compute_2D_edge_confidence + compute_2D_depth_epi on a normalised volume [V,S,U,C] with per-pixel ranges [S,V,U].
    Returns (planes, pixels scanned per visit, pixels refined per visit), the visits in sweep order."""
    vol = np.ascontiguousarray(vol, F)
    V, S, U, C = vol.shape
    pd = params_dict(p)
    Ce = np.zeros((S, V, U), F); cm = np.zeros((S, V, U), np.uint8)
    for s in range(S):
        Ce[s], cm[s] = oracle.edge_confidence_pile(vol, s, p)
    Cd = np.zeros((S, V, U), F); depth = np.zeros((S, V, U), F); rbar = np.zeros((S, V, U, C), F)
    Cl = np.zeros((S, V, U), F)
    K = np.zeros((V, S, U), F)
    mask = cm.copy()
    slope = F(p.slope_factor)
    thr_line = F(line_score_threshold); thr_disp = F(p.disp_score_threshold)
    eps = F(propagation_epsilon)
    scanned, refined = [], []
    for s_hat in lcr.sweep_order(S):
        scanned.append(int(((cm[s_hat] != 0) & (mask[s_hat] != 0)).sum()))
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
        if subgrid:   # the step this file adds: the pixels this visit scanned and accepted, moved off the grid
            got = idx >= 0
            disp = sr.refine(vol, idx, dmin_svu[s_hat], dmax_svu[s_hat], D, s_hat, pd)[0]
            depth[s_hat][got] = disp[got]
            refined.append(int(got.sum()))
        else:
            refined.append(0)
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
    return dict(edge_confidence=Ce, edge_mask=cm, disp_confidence=Cd, depth=depth, rbar=rbar, scan_mask=mask,
                line_confidence=Cl), scanned, refined


def fine_to_coarse(oracle, raw_vsuc, dmin, dmax, D, params=None, mode=0, line_score_threshold=0.02, max_pyr_depth=-1,
                   accept_all_last_scale=True, elem="f32", min_spatial_dim=10, subgrid=False):
    """f2c_line_conf_ref.fine_to_coarse with every level swept by `sweep` above, on f2c_keep_ref.pyramid's levels.  elem:
    "f32", "u8" or "u16" -- the arithmetic the pyramid keeps.  Every level also reports its visits' counts."""
    vols, scales, pars = fkr.pyramid(oracle, raw_vsuc, params, max_pyr_depth, elem, -1.0, min_spatial_dim)
    S = vols[0].shape[1]
    levels, total = [], 0
    for l, (vol, p) in enumerate(zip(vols, pars)):
        Vp, Up = vol.shape[0], vol.shape[2]
        lo = np.full((S, Vp, Up), dmin, F); hi = np.full((S, Vp, Up), dmax, F)
        if l > 0:
            lo, hi = oracle.f2c_tighten_bounds(levels[-1]["depth"], levels[-1]["valid"], lo, hi)             # f2c.hpp:176-294
        r, scanned, refined = sweep(oracle, vol, lo, hi, D, p, mode, line_score_threshold, subgrid=subgrid)
        total += sum(scanned)
        r["valid"] = flr.validity(r, p, mode, line_score_threshold, accept_all_last_scale and l == len(vols) - 1)
        r["dmin"], r["dmax"] = lo, hi
        r["scanned"], r["refined"] = scanned, refined
        levels.append(r)
    fused = np.zeros((S,) + levels[0]["depth"].shape[1:], F)
    fvalid = np.zeros(fused.shape, np.uint8)
    for s in range(S):                                                                                       # fine_to_coarse_core.cpp:84
        fused[s], fvalid[s] = oracle.f2c_fuse([lv["depth"][s] for lv in levels], [lv["valid"][s] for lv in levels])
    return dict(levels=levels, dims=[(v.shape[0], v.shape[2]) for v in vols], volumes=vols, scales=scales, fused_map=fused,
                fused_valid=fvalid, pixels_scanned=total)


# ---- the planted field ---------------------------------------------------------------------------------------------------
PLANTED = dict(V=6, U=80, S=5, D=9, lo=-2.0, hi=2.0)
PLANTED_D = (0.37, -0.61, 1.3)


def planted_field(d_true, C=1):
    """6 scanlines of peaks_ref's planted line of disparity d_true, scanline v shifted by v pixels, 5 views, 80 columns:
    [V, S, U, C] float32.  C = 3: the same texture at three gains, as tests/test_gpu_subgrid.py's pile field."""
    V, U, S = PLANTED["V"], PLANTED["U"], PLANTED["S"]
    wide = pr.planted_epi(d_true, S=S, U=U + 8, s_hat=S // 2)
    one = np.stack([wide[:, v:v + U] for v in range(V)]).astype(F)
    if C == 1:
        return one[..., None]
    return np.ascontiguousarray(np.stack([one, one * F(0.8), one * F(0.6)], axis=-1).astype(F))


def planted_error(planes, d_true):
    """Median |disparity - d_true| over all valid pixels (edge mask set) of all views."""
    m = planes["edge_mask"] != 0
    return float(np.median(np.abs(planes["depth"][m].astype(np.float64) - d_true)))


_cache = {}


def planted_reference(oracle, d_true, subgrid, C=1, mode=0, use_disp=False, disp_thr=None, thr=0.02):
    """`sweep` on the planted field with default parameters, computed once per session and shared (callers must not write
    into it).  Returns (planes, scanned per visit, refined per visit)."""
    key = (float(d_true), bool(subgrid), C, mode, bool(use_disp), disp_thr, float(thr))
    if key not in _cache:
        p = oracle.default_params()
        p.use_disp_confidence_score = int(use_disp)
        if disp_thr is not None:
            p.disp_score_threshold = disp_thr
        vol = planted_field(d_true, C)
        S, V, U = PLANTED["S"], PLANTED["V"], PLANTED["U"]
        lo = np.full((S, V, U), PLANTED["lo"], F); hi = np.full((S, V, U), PLANTED["hi"], F)
        _cache[key] = sweep(oracle, vol, lo, hi, PLANTED["D"], p, mode, thr, subgrid=subgrid)
    return _cache[key]


def f2c_reference(oracle, name, subgrid, mode=0, thr=0.02):
    """`fine_to_coarse` on a case of f2c_keep_ref (f2c_line_conf_ref's "A", "B", ...; "U16"), range [-1, 1], computed once per
    session and shared."""
    key = ("f2c", name, bool(subgrid), mode, float(thr))
    if key not in _cache:
        C, elem, V, U, S, D, accept = fkr.case_of(name)
        _cache[key] = fine_to_coarse(oracle, fkr.make_field(name).astype(F), -1.0, 1.0, D, oracle.default_params(), mode, thr,
                                     accept_all_last_scale=accept, elem=elem, subgrid=subgrid)
    return _cache[key]
