"""The yardstick of a kept fine-to-coarse run's validity by cross-view consistency (include/rslf_hip.h, rslf_f2c_run_host_cs):
numpy, written from that text and composed of public pieces.  Never the HIP path against itself.

  * f2c_peaks_ref's level loop: f2c_keep_ref.pyramid's levels, each swept by sweep_peaks_ref.sweep (by sweep_gate_ref.sweep
    with a propagation ratio), f2c_keep_ref.validity, then f2c_peaks_ref.ambiguous with a uniqueness ratio;
  * consistency_ref.consistency(depth, valid, slope, tol, radius, 0) on the level's disparities and THAT validity, with the
    level's slope factor: its `seen` and `agree` planes;
  * the gate agree >= minimum(seen, min_agree) on the pixels that are valid, not on a level accepted whole;
  * oracle.f2c_tighten_bounds and oracle.f2c_fuse, fed the gated validity, and f2c_peaks_ref.origin_walk.

Every level also reports `inconsistent` (pixels the gate made invalid), `cs_agree` / `cs_seen` (the gate's counts; None where
the gate did not run), `pre_gate_valid` and `naive_drop` (what `agree >= min_agree` alone would have dropped).
"""
import numpy as np

import consistency_ref as cr
import f2c_keep_ref as kr
import f2c_peaks_ref as pf
import sweep_gate_ref as sgr
import sweep_peaks_ref as spr

F = np.float32
TOL = 0.25          # one step of the cases' hypothesis grid: (1 - -1) / (9 - 1); case C's is 2 / 39
MIN_AGREE = 2


def gate(seen, agree, min_agree):
    """consistency_gate: at least min_agree of the views that see the pixel agree, or all of them where fewer see it."""
    return agree >= np.minimum(seen, min_agree)


def gate_level(depth, valid, slope, tol, radius, min_agree):
    """One level's gate -> (gated validity, cs_agree, cs_seen, dropped mask, what agree >= min_agree alone would drop)."""
    c = cr.consistency(depth, valid, slope, tol, radius, 0)
    live = valid != 0
    drop = live & ~gate(c["seen"], c["agree"], min_agree)
    naive = live & (c["agree"] < min_agree)
    return np.where(drop, 0, valid).astype(np.uint8), c["agree"], c["seen"], drop, naive


def fine_to_coarse(oracle, raw_vsuc, dmin, dmax, D, params=None, mode=0, line_score_threshold=0.02, max_pyr_depth=-1,
                   accept_all_last_scale=True, elem="f32", rule=kr.COMPAT, epi_scale_factor=-1.0, subgrid=False, ratio=0.0,
                   propagation_ratio=0.0, min_agree=0, tol=TOL, radius=0):
    """f2c_peaks_ref.fine_to_coarse (sweep_gate_ref.fine_to_coarse with a propagation ratio) with the consistency gate after
    the uniqueness predicate.  min_agree = 0: those functions, plane for plane."""
    vols, scales, pars = kr.pyramid(oracle, raw_vsuc, params, max_pyr_depth, elem, epi_scale_factor)
    S = vols[0].shape[1]
    levels = []
    for l, (vol, p) in enumerate(zip(vols, pars)):
        Vp, Up = vol.shape[0], vol.shape[2]
        lo = np.full((S, Vp, Up), dmin, F); hi = np.full((S, Vp, Up), dmax, F)
        if l > 0:
            lo, hi = oracle.f2c_tighten_bounds(levels[-1]["depth"], levels[-1]["valid"], lo, hi)
        withheld = 0
        if propagation_ratio > 0:
            r, pk, _, w, _, _ = sgr.sweep(oracle, vol, lo, hi, D, p, mode, line_score_threshold, subgrid=subgrid, ratio=propagation_ratio)
            withheld = int(sum(w))
        else:
            r, pk, _ = spr.sweep(oracle, vol, lo, hi, D, p, mode, line_score_threshold, subgrid=subgrid)
        accept_all = accept_all_last_scale and l == len(vols) - 1
        valid = kr.validity(r, p, mode, line_score_threshold, accept_all, rule)
        r["dropped"] = 0
        if ratio > 0 and not accept_all:
            drop = (valid != 0) & pf.ambiguous(pk, ratio)
            valid = np.where(drop, 0, valid).astype(np.uint8)
            r["dropped"] = int(drop.sum())
        r["pre_gate_valid"], r["inconsistent"], r["cs_agree"], r["cs_seen"], r["naive_drop"] = valid, 0, None, None, 0
        if min_agree > 0 and not accept_all:
            valid, r["cs_agree"], r["cs_seen"], drop, naive = gate_level(r["depth"], valid, p.slope_factor, tol, radius, min_agree)
            r["inconsistent"], r["naive_drop"] = int(drop.sum()), int(naive.sum())
            r["kept_by_border_rule"] = int((naive & ~drop).sum())
        r["valid"], r["dmin"], r["dmax"], r["pk"], r["withheld"] = valid, lo, hi, pk, withheld
        levels.append(r)
    fused = np.zeros((S,) + levels[0]["depth"].shape[1:], F)
    fvalid = np.zeros(fused.shape, np.uint8)
    for s in range(S):
        fused[s], fvalid[s] = oracle.f2c_fuse([lv["depth"][s] for lv in levels], [lv["valid"][s] for lv in levels])
    fused_pk, fused_level = pf.origin_walk([lv["valid"] for lv in levels], [lv["pk"] for lv in levels])
    return dict(levels=levels, dims=[(v.shape[0], v.shape[2]) for v in vols], volumes=vols, scales=scales, fused_map=fused,
                fused_valid=fvalid, fused_pk=fused_pk, fused_level=fused_level)


def grid_step(name):
    """One step of a case's hypothesis grid as the float32 the library is handed."""
    D = kr.case_of(name)[5]
    return float(F((1.0 - -1.0) / (D - 1)))


_cache = {}


def reference(oracle, name, min_agree=0, radius=0, mode=0, thr=0.02, subgrid=False, ratio=0.0, propagation_ratio=0.0, tol=None):
    """fine_to_coarse on a case of f2c_line_conf_ref.CASES, range [-1, 1], tol one grid step unless given; computed once per
    session and shared (callers must not write into it)."""
    tol = grid_step(name) if tol is None else float(tol)
    key = (name, int(min_agree), int(radius) if min_agree else 0, mode, float(thr) if mode == 2 else 0.0, bool(subgrid), float(ratio),
           float(propagation_ratio), tol if min_agree else 0.0)
    if key not in _cache:
        C, elem, V, U, S, D, accept = kr.case_of(name)
        _cache[key] = fine_to_coarse(oracle, kr.make_field(name).astype(F), -1.0, 1.0, D, oracle.default_params(), mode, thr,
                                     accept_all_last_scale=accept, elem=elem, subgrid=subgrid, ratio=ratio,
                                     propagation_ratio=propagation_ratio, min_agree=min_agree, tol=tol, radius=radius)
    return _cache[key]
