"""The yardstick of the 2-D sweep's gate by peak ratio (include/rslf_hip.h, rslf_sweep_propagation_ratio and the *_pr entries
below it): numpy, written from that text and composed of public pieces.  Never the HIP path against itself.

`sweep` restates the loop of tests/sweep_peaks_ref.sweep with ONE line more -- `src &= ~ambiguous(pk[s_hat], r)` -- and counts:
per visit the sources that line withheld (pixels that pass the gate of core.hpp:1097-1103 and fail the predicate) and the
pixels the visit's scan was entered with.  The predicate is f2c_peaks_ref.ambiguous, the one of the pyramid's validity by
uniqueness: idx >= 0 and runner_idx >= 0 and runner_score > r * score, the product one float32 multiply.  With the ratio off
(0) the loop is sweep_peaks_ref's; tests/test_sweep_gate_cpu.py holds every plane to it.

`fine_to_coarse` is f2c_peaks_ref.fine_to_coarse with every level swept by that `sweep`: f2c_keep_ref.pyramid's levels and
validity, the uniqueness predicate, oracle.f2c_tighten_bounds / f2c_fuse and f2c_peaks_ref.origin_walk.

Also the fields and ratios the CPU and GPU tests share, each computed once per session."""
import numpy as np

import f2c_keep_ref as kr
import f2c_peaks_ref as fpr
import line_conf_ref as lcr
import subgrid_ref as sr
import sweep_peaks_ref as spr
import sweep_subgrid_ref as ssr

F = np.float32
PLANES = spr.PLANES


def ambiguous(pk_vu, r):
    """The predicate on a dict of peak planes (any shape)."""
    return fpr.ambiguous(pk_vu, r)


def sweep(oracle, vol, dmin_svu, dmax_svu, D, p, mode=0, line_score_threshold=0.02, propagation_epsilon=0.1, subgrid=False,
          fill=None, ratio=0.0):
    """sweep_peaks_ref.sweep gated by `ratio` (0: off).  Returns (planes, peak planes, accepted, withheld, scanned, sources): the
    first three as sweep_peaks_ref.sweep's; the others per visit, in sweep order -- the sources the ratio withheld, the pixels
    of the visited view that were in its edge mask and its running mask when the visit began, and the pixels that passed the
    gate of core.hpp:1097-1103 (withheld ones included)."""
    vol = np.ascontiguousarray(vol, F)
    V, S, U, C = vol.shape
    pd = ssr.params_dict(p)
    Ce = np.zeros((S, V, U), F); cm = np.zeros((S, V, U), np.uint8)
    for s in range(S):
        Ce[s], cm[s] = oracle.edge_confidence_pile(vol, s, p)
    Cd = np.zeros((S, V, U), F); depth = np.zeros((S, V, U), F); rbar = np.zeros((S, V, U, C), F)
    Cl = np.zeros((S, V, U), F)
    K = np.zeros((V, S, U), F)
    mask = cm.copy()
    pk = spr.empty_planes(S, V, U) if fill is None else {k: fill[k].copy() for k in PLANES}
    slope = F(p.slope_factor)
    thr_line = F(line_score_threshold); thr_disp = F(p.disp_score_threshold)
    eps = F(propagation_epsilon)
    accepted, withheld, scanned, sources = [], [], [], []
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
        got = idx >= 0
        if subgrid:
            disp = sr.refine(vol, idx, dmin_svu[s_hat], dmax_svu[s_hat], D, s_hat, pd)[0]
            depth[s_hat][got] = disp[got]
        for v, u in zip(*np.nonzero(got)):
            i1, s1, i2, s2 = spr.row_peaks(vol[v], u, dmin_svu[s_hat, v, u], dmax_svu[s_hat, v, u], D, s_hat, pd)
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
        sources.append(int(src.sum()))
        # the line this file adds: an ambiguous pixel is no source -- it makes no claim, not even the one on itself
        if ratio > 0:
            amb = ambiguous({k: pk[k][s_hat] for k in PLANES}, ratio)
            withheld.append(int((src & amb).sum()))
            src = src & ~amb
        else:
            withheld.append(0)
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
                        for k, val in zip(PLANES, pk_u):
                            pk[k][s, v, ri] = val
    planes = dict(edge_confidence=Ce, edge_mask=cm, disp_confidence=Cd, depth=depth, rbar=rbar, scan_mask=mask,
                  line_confidence=Cl)
    return planes, pk, accepted, withheld, scanned, sources


def fine_to_coarse(oracle, raw_vsuc, dmin, dmax, D, params=None, mode=0, line_score_threshold=0.02, max_pyr_depth=-1,
                   accept_all_last_scale=True, elem="f32", rule=kr.COMPAT, epi_scale_factor=-1.0, subgrid=False, ratio=0.0,
                   propagation_ratio=0.0):
    """f2c_peaks_ref.fine_to_coarse with every level's sweep gated by propagation_ratio; `ratio` stays the uniqueness ratio of
    the validity.  Every level also reports `withheld`, its sweep's sum."""
    vols, scales, pars = kr.pyramid(oracle, raw_vsuc, params, max_pyr_depth, elem, epi_scale_factor)
    S = vols[0].shape[1]
    levels = []
    for l, (vol, p) in enumerate(zip(vols, pars)):
        Vp, Up = vol.shape[0], vol.shape[2]
        lo = np.full((S, Vp, Up), dmin, F); hi = np.full((S, Vp, Up), dmax, F)
        if l > 0:
            lo, hi = oracle.f2c_tighten_bounds(levels[-1]["depth"], levels[-1]["valid"], lo, hi)
        r, pk, _, withheld, _, _ = sweep(oracle, vol, lo, hi, D, p, mode, line_score_threshold, subgrid=subgrid, ratio=propagation_ratio)
        accept_all = accept_all_last_scale and l == len(vols) - 1
        valid = kr.validity(r, p, mode, line_score_threshold, accept_all, rule)
        r["dropped"] = 0
        if ratio > 0 and not accept_all:
            drop = (valid != 0) & fpr.ambiguous(pk, ratio)
            valid = np.where(drop, 0, valid).astype(np.uint8)
            r["dropped"] = int(drop.sum())
        r["valid"], r["dmin"], r["dmax"], r["pk"], r["withheld"] = valid, lo, hi, pk, int(sum(withheld))
        levels.append(r)
    fused = np.zeros((S,) + levels[0]["depth"].shape[1:], F)
    fvalid = np.zeros(fused.shape, np.uint8)
    for s in range(S):
        fused[s], fvalid[s] = oracle.f2c_fuse([lv["depth"][s] for lv in levels], [lv["valid"][s] for lv in levels])
    fused_pk, fused_level = fpr.origin_walk([lv["valid"] for lv in levels], [lv["pk"] for lv in levels])
    return dict(levels=levels, dims=[(v.shape[0], v.shape[2]) for v in vols], volumes=vols, scales=scales, fused_map=fused,
                fused_valid=fvalid, fused_pk=fused_pk, fused_level=fused_level)


# ---- the fields and their working ratios (tests/test_sweep_gate_cpu.py recounts what makes them working ones) -------------
# name -> (ratio, what the field is)
RATIOS = {"planted": 0.7, "A": 0.7, "B": 0.4, "C": 0.8}
WIDE = dict(S=3, V=5, U=520, D=9, lo=-4.0, hi=4.0, d_true=3.3, ratio=0.9)   # claims cross the 256-column segments


def field(oracle, name, C=1):
    """(normalised volume [V,S,U,C], D, lo, hi, parameters) of a sweep field: "planted" (sweep_subgrid_ref.planted_field(0.37)),
    "A" / "B" / "C" (level 0 of that case of f2c_keep_ref.pyramid, range [-1, 1]) or "wide" (peaks_ref's planted line, 520
    columns, a disparity range whose claims cross the 256-column segments)."""
    if name == "planted":
        return ssr.planted_field(0.37, C), ssr.PLANTED["D"], ssr.PLANTED["lo"], ssr.PLANTED["hi"], oracle.default_params()
    if name == "wide":
        import peaks_ref as pr
        w = WIDE
        wide = pr.planted_epi(w["d_true"], S=w["S"], U=w["U"] + 8, s_hat=w["S"] // 2)
        vol = np.stack([wide[:, v:v + w["U"]] for v in range(w["V"])]).astype(F)[..., None]
        return np.ascontiguousarray(vol), w["D"], w["lo"], w["hi"], oracle.default_params()
    _, elem, _, _, _, D, _ = kr.case_of(name)
    vols, _, pars = kr.pyramid(oracle, kr.make_field(name).astype(F), oracle.default_params(), -1, elem)
    return vols[0], D, -1.0, 1.0, pars[0]


def ratio_of(name):
    return WIDE["ratio"] if name == "wide" else RATIOS[name]


_cache = {}


def reference(oracle, name, ratio, C=1, mode=0, thr=0.02, subgrid=False, use_disp=False, disp_thr=None, median=None, ranges=None):
    """`sweep` on a field of `field`, computed once per session and shared (callers must not write into it).  median: the
    median window (default the parameters'); ranges: None or "mixed" (sweep_peaks_ref.range_planes; the planted field)."""
    key = (name, float(ratio), C, mode, float(thr) if mode == 2 else 0.0, bool(subgrid), bool(use_disp), disp_thr, median, ranges)
    if key not in _cache:
        vol, D, lo, hi, p = field(oracle, name, C)
        p = type(p).from_buffer_copy(p)
        p.use_disp_confidence_score = int(use_disp)
        if disp_thr is not None:
            p.disp_score_threshold = disp_thr
        if median is not None:
            p.median_filter_size = median
        V, S, U, _ = vol.shape
        if ranges is None:
            lo_p, hi_p = np.full((S, V, U), lo, F), np.full((S, V, U), hi, F)
        else:
            assert name == "planted"
            lo_p, hi_p = spr.range_planes(ranges)
        _cache[key] = sweep(oracle, vol, lo_p, hi_p, D, p, mode, thr, subgrid=subgrid, ratio=ratio)
    return _cache[key]


def f2c_reference(oracle, name, propagation_ratio, ratio=0.0):
    """`fine_to_coarse` on a case of f2c_keep_ref, range [-1, 1], once per session and shared."""
    key = ("f2c", name, float(propagation_ratio), float(ratio))
    if key not in _cache:
        C, elem, V, U, S, D, accept = kr.case_of(name)
        _cache[key] = fine_to_coarse(oracle, kr.make_field(name).astype(F), -1.0, 1.0, D, oracle.default_params(), 0, 0.02,
                                     accept_all_last_scale=accept, elem=elem, ratio=ratio, propagation_ratio=propagation_ratio)
    return _cache[key]


# ---- the sweeps the CPU test recounts and the GPU test runs: id -> (field, keywords of `reference`) -----------------------
LINE2_THR = 0.06
SWEEP_CASES = {
    "planted_C1": ("planted", dict(C=1)),
    "planted_C3": ("planted", dict(C=3)),
    "planted_mixed": ("planted", dict(ranges="mixed")),
    "A": ("A", dict()),
    "A_line1": ("A", dict(mode=1)),
    "A_line2": ("A", dict(mode=2, thr=LINE2_THR)),
    "A_disp": ("A", dict(use_disp=True)),
    "A_sub": ("A", dict(subgrid=True)),
    "A_med0": ("A", dict(median=0)),
    "A_med11": ("A", dict(median=11)),
    "B": ("B", dict()),
    "C": ("C", dict()),
    "wide": ("wide", dict()),
}


def case_reference(oracle, case, gated=True):
    """(field name, ratio, keywords, reference) of a case of SWEEP_CASES, gated by the field's working ratio or not."""
    name, kw = SWEEP_CASES[case]
    ratio = ratio_of(name)
    return name, ratio, kw, reference(oracle, name, ratio if gated else 0.0, **kw)


def threshold_margin(planes, kw, p):
    """How far the nearest reference value lies from the threshold a case gates or validates by (C_d with use_disp, C_l in line
    mode 2); inf for a case that compares against none."""
    if kw.get("use_disp"):
        return float(np.abs(planes["disp_confidence"].astype(np.float64) - float(F(p.disp_score_threshold))).min())
    if kw.get("mode") == 2:
        return float(np.abs(planes["line_confidence"].astype(np.float64) - float(F(kw["thr"]))).min())
    return float("inf")
