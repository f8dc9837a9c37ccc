"""The yardstick of a kept fine-to-coarse run's peak planes and of its validity by uniqueness (include/rslf_hip.h,
rslf_f2c_run_host_pk): numpy, written from that text and composed of public pieces.  Never the HIP path against itself.

  * f2c_keep_ref.pyramid's levels, each swept by sweep_peaks_ref.sweep (which changes no plane of the sweeps the other
    references run, tests/test_sweep_peaks_cpu.py);
  * f2c_keep_ref.validity, then the uniqueness predicate: a pixel is invalid if idx >= 0 and runner_idx >= 0 and
    runner_score > r * score, the product one float32 multiply; the level accepted whole is not touched;
  * oracle.f2c_tighten_bounds and oracle.f2c_fuse, fed those validity planes;
  * the origin walk: for every pixel of the finest plane the first level down the fusion's nearest-pixel mask chain whose
    validity is set -- from level p, pixel (y, x), to level p + 1, pixel (min(floor(y * (1 / (R_p / R_{p+1}))), R_{p+1} - 1),
    the same in x), in double -- and that pixel's four peak values; 255 and -1 / 0 where no level is valid.
"""
import numpy as np

import f2c_keep_ref as kr
import sweep_peaks_ref as spr

F = np.float32
PLANES = spr.PLANES
OLD_PLANES = ("depth", "edge_confidence", "disp_confidence", "line_confidence", "valid", "dmin", "dmax")


def ambiguous(pk, r):
    """The uniqueness predicate on a dict of peak planes."""
    bound = (F(r) * pk["score"]).astype(F)                      # one binary32 multiply per pixel
    return (pk["idx"] >= 0) & (pk["runner_idx"] >= 0) & (pk["runner_score"] > bound)


def walk_index(n_fine, n_coarse):
    """Where each index of a side of n_fine pixels looks on the side of n_coarse pixels one level down."""
    scale = 1.0 / (float(n_fine) / n_coarse)
    return np.minimum(np.floor(np.arange(n_fine) * scale).astype(np.int64), n_coarse - 1)


def origin_walk(valids, pks):
    """valids[p] [S,V_p,U_p] uint8, pks[p] dicts of the four planes, finest first -> (fused peak planes, fused_level)."""
    P = len(valids)
    S, V0, U0 = valids[0].shape
    level = np.full((S, V0, U0), 255, np.uint8)
    out = spr.empty_planes(S, V0, U0)
    y0, x0 = np.meshgrid(np.arange(V0), np.arange(U0), indexing="ij")
    for s in range(S):
        y, x = y0.copy(), x0.copy()
        undecided = np.ones((V0, U0), bool)
        for p in range(P):
            hit = undecided & (valids[p][s][y, x] != 0)
            level[s][hit] = p
            for k in PLANES:
                out[k][s][hit] = pks[p][k][s][y[hit], x[hit]]
            undecided &= ~hit
            if p + 1 < P:
                y = walk_index(valids[p].shape[1], valids[p + 1].shape[1])[y]
                x = walk_index(valids[p].shape[2], valids[p + 1].shape[2])[x]
    return out, level


def fine_to_coarse(oracle, raw_vsuc, dmin, dmax, D, params=None, mode=0, line_score_threshold=0.02, max_pyr_depth=-1,
                   accept_all_last_scale=True, elem="f32", rule=kr.COMPAT, epi_scale_factor=-1.0, subgrid=False, ratio=0.0):
    """f2c_keep_ref.fine_to_coarse with every level swept in the peaks mode and, with ratio > 0, the validity by
    uniqueness.  Returns its dict plus per level `pk` (the four planes) and `dropped` (pixels the predicate made invalid), and
    fused_pk, fused_level."""
    vols, scales, pars = kr.pyramid(oracle, raw_vsuc, params, max_pyr_depth, elem, epi_scale_factor)
    S = vols[0].shape[1]
    levels = []
    for l, (vol, p) in enumerate(zip(vols, pars)):
        Vp, Up = vol.shape[0], vol.shape[2]
        lo = np.full((S, Vp, Up), dmin, F); hi = np.full((S, Vp, Up), dmax, F)
        if l > 0:
            lo, hi = oracle.f2c_tighten_bounds(levels[-1]["depth"], levels[-1]["valid"], lo, hi)
        r, pk, _ = spr.sweep(oracle, vol, lo, hi, D, p, mode, line_score_threshold, subgrid=subgrid)
        accept_all = accept_all_last_scale and l == len(vols) - 1
        valid = kr.validity(r, p, mode, line_score_threshold, accept_all, rule)
        r["dropped"] = 0
        if ratio > 0 and not accept_all:
            drop = (valid != 0) & ambiguous(pk, ratio)
            valid = np.where(drop, 0, valid).astype(np.uint8)
            r["dropped"] = int(drop.sum())
        r["valid"], r["dmin"], r["dmax"], r["pk"] = valid, lo, hi, pk
        levels.append(r)
    fused = np.zeros((S,) + levels[0]["depth"].shape[1:], F)
    fvalid = np.zeros(fused.shape, np.uint8)
    for s in range(S):
        fused[s], fvalid[s] = oracle.f2c_fuse([lv["depth"][s] for lv in levels], [lv["valid"][s] for lv in levels])
    fused_pk, fused_level = origin_walk([lv["valid"] for lv in levels], [lv["pk"] for lv in levels])
    return dict(levels=levels, dims=[(v.shape[0], v.shape[2]) for v in vols], volumes=vols, scales=scales, fused_map=fused,
                fused_valid=fvalid, fused_pk=fused_pk, fused_level=fused_level)


# The ratio at which case B (RGB u8) shows the rule: at 0.7 no fused value of B changes; chosen on this reference, going down
# from 0.7 in steps of 0.1 until at least 100 fused values change (tests/test_f2c_peaks_cpu.py recounts it).
# (0.7: 0 fused values change, 0.6: 1, 0.5: 23, 0.4: 250.)
RATIO_A = 0.7
RATIO_B = 0.4

_cache = {}


def reference(oracle, name, mode=0, thr=0.02, subgrid=False, ratio=0.0):
    """fine_to_coarse on a case of f2c_line_conf_ref.CASES, computed once per session and shared (callers must not write
    into it)."""
    key = (name, mode, float(thr) if mode == 2 else 0.0, bool(subgrid), float(ratio))
    if key not in _cache:
        C, elem, V, U, S, D, accept = kr.case_of(name)
        _cache[key] = fine_to_coarse(oracle, kr.make_field(name).astype(F), -1.0, 1.0, D, oracle.default_params(), mode, thr,
                                     accept_all_last_scale=accept, elem=elem, subgrid=subgrid, ratio=ratio)
    return _cache[key]
