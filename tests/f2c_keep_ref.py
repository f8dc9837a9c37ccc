"""The yardstick of the kept fine-to-coarse run (tests only; numpy, composed from tests/f2c_line_conf_ref.py and the CPU
oracle).  Never the HIP path against itself.

It is f2c_line_conf_ref.fine_to_coarse with three additions:
  * the validity rule.  COMPAT is f2c_line_conf_ref.validity; REFERENCE is the whole chain of get_valid_depths_mask_s_v_u
    (dc.hpp:893-915): accept_all -> everything; else use_disp_confidence_score -> C_d > (float)disp_score_threshold (:902);
    else mode 2 -> C_l > (float)line_score_threshold (:904); else C_e > (float)edge_score_threshold (:906);
  * every level's normalised volume and epi_scale_factor come back too (what a kept run holds with keep_volumes);
  * the element type: "f32" (every level by its own max, or by a given factor), "u8" (1/255, uchar pyramid), "u16" (the f32
    rule on ushort levels, ushort pyramid -- tests/test_gpu_u16.py's numpy restatement of the halving).
The pictures of a run are tests/render_ref.py's, fed these planes (pictures()).
"""
import numpy as np

import f2c_line_conf_ref as fr
import render_ref as rr

F = np.float32
COMPAT, REFERENCE = 0, 1


def validity(planes, p, mode, line_score_threshold, accept_all, rule):
    """get_valid_depths_mask_s_v_u (dc.hpp:893-915) under a validity rule."""
    if rule == REFERENCE and not accept_all and p.use_disp_confidence_score:
        return np.where(planes["disp_confidence"] > F(p.disp_score_threshold), 255, 0).astype(np.uint8)   # :902
    return fr.validity(planes, p, mode, line_score_threshold, accept_all)


def _normalise(oracle, cur, elem, epi_scale_factor):
    """Depth2DComputer's constructor on a raw level (dc.hpp:671-705) -> (normalised volume, the factor used)."""
    if elem == "u8":
        return oracle.normalize_u8(cur.astype(np.uint8)), 255.0
    return oracle.normalize_f32(cur, float(epi_scale_factor))


def _downsample(oracle, cur, elem):
    if elem == "u8":
        return oracle.downsample_epis_u8(cur)
    if elem == "u16":
        from test_gpu_u16 import downsample_u16_np
        return downsample_u16_np(cur)
    return oracle.downsample_epis(cur)


def pyramid(oracle, raw_vsuc, params=None, max_pyr_depth=-1, elem="f32", epi_scale_factor=-1.0, min_spatial_dim=10):
    """FineToCoarse's constructor (f2c.hpp:103-159) on a RAW float32 volume [V,S,U,C]: per level, finest first, the normalised
    volume its Depth2DComputer holds, the epi_scale_factor it used and its parameters -> (volumes, scales, parameters)."""
    base = params or oracle.default_params()
    cur = np.ascontiguousarray(raw_vsuc, F)
    U0 = cur.shape[2]
    if max_pyr_depth < 1:
        max_pyr_depth = 1 << 30
    vols, scales, pars = [], [], []
    while cur.shape[0] > min_spatial_dim and cur.shape[2] > min_spatial_dim and len(vols) < max_pyr_depth:   # f2c.hpp:130
        p = type(base).from_buffer_copy(base)
        p.slope_factor = F((0.0 + cur.shape[2]) / U0)                                                        # f2c.hpp:139
        vol, scale = _normalise(oracle, cur, elem, epi_scale_factor)
        vols.append(vol); scales.append(float(scale)); pars.append(p)
        cur = _downsample(oracle, cur, elem)                                                                 # f2c.hpp:145-147
    return vols, scales, pars


def fine_to_coarse(oracle, raw_vsuc, dmin, dmax, D, params=None, mode=0, line_score_threshold=0.02, max_pyr_depth=-1,
                   accept_all_last_scale=True, elem="f32", rule=COMPAT, epi_scale_factor=-1.0, min_spatial_dim=10):
    """FineToCoarse constructor + run() + get_results() on a RAW float32 volume [V,S,U,C] (uchar / ushort levels with elem
    "u8" / "u16").  Returns dict(levels=[planes + valid, dmin, dmax], dims, volumes, scales, fused_map, fused_valid,
    pixels_scanned)."""
    vols, scales, pars = pyramid(oracle, raw_vsuc, params, max_pyr_depth, elem, epi_scale_factor, min_spatial_dim)
    S = vols[0].shape[1]
    levels, total = [], 0
    for l, (vol, p) in enumerate(zip(vols, pars)):
        Vp, Up = vol.shape[0], vol.shape[2]
        lo = np.full((S, Vp, Up), dmin, F); hi = np.full((S, Vp, Up), dmax, F)
        if l > 0:
            lo, hi = oracle.f2c_tighten_bounds(levels[-1]["depth"], levels[-1]["valid"], lo, hi)             # f2c.hpp:176-294
        r, n = fr.sweep(oracle, vol, lo, hi, D, p, mode, line_score_threshold)
        total += n
        r["valid"] = validity(r, p, mode, line_score_threshold, accept_all_last_scale and l == len(vols) - 1, rule)
        r["dmin"], r["dmax"] = lo, hi
        levels.append(r)
    fused = np.zeros((S,) + levels[0]["depth"].shape[1:], F)
    fvalid = np.zeros(fused.shape, np.uint8)
    for s in range(S):                                                                                       # fine_to_coarse_core.cpp:84
        fused[s], fvalid[s] = oracle.f2c_fuse([lv["depth"][s] for lv in levels], [lv["valid"][s] for lv in levels])
    return dict(levels=levels, dims=[(v.shape[0], v.shape[2]) for v in vols], volumes=vols, scales=scales, fused_map=fused,
                fused_valid=fvalid, pixels_scanned=total)


# ---- the cases: those of f2c_line_conf_ref, the u16 field built like make_field, and their darkened forms --------------

DARK = (slice(8, 30), slice(12, 44))   # scanlines and columns of the darkened rectangle (cases of 44 x 64)


def make_field(name, dark=False):
    """The raw light field [V,S,U,C] of a case of f2c_line_conf_ref.CASES, or "U16": case A's scene as `round(vol * 65535)`
    uint16.  dark: the rectangle DARK of every view is scaled by 0.04, below the getters' shadow level after normalisation
    (the synthetic scene itself has no radiance below 0.2)."""
    if name == "U16":
        from remotesensingproject_amd.synth import make_lightfield
        C, _, V, U, S, _, _, _ = fr.CASES["A"]
        vol, _ = make_lightfield(U, V, S, C, seed=2, dmin=-1.0, dmax=1.0, band=8)
        field = np.ascontiguousarray(np.rint(vol * 65535.0).astype(np.uint16))
    else:
        field = fr.make_field(name)
    if dark:
        cut = field.astype(np.float64)
        cut[DARK[0], :, DARK[1]] *= 0.04
        field = np.ascontiguousarray(np.rint(cut).astype(field.dtype) if field.dtype != F else cut.astype(F))
    return field


def case_of(name):
    """(C, elem, V, U, S, D, accept_all_last_scale) of a case name."""
    C, dt, V, U, S, D, accept, _ = fr.CASES["A" if name == "U16" else name]
    return C, ("u16" if name == "U16" else dt), V, U, S, D, accept


_cache = {}


def reference(oracle, name, mode=0, thr=0.02, use_disp=False, disp_thr=0.01, rule=COMPAT, dark=False, epi_scale_factor=-1.0):
    """fine_to_coarse on a case, computed once per session and shared (callers must not write into it)."""
    key = (name, mode, float(thr) if mode == 2 else 0.0, bool(use_disp), float(disp_thr) if use_disp else 0.0, rule, dark,
           float(epi_scale_factor))
    if key not in _cache:
        C, elem, V, U, S, D, accept = case_of(name)
        p = oracle.default_params()
        p.use_disp_confidence_score = int(use_disp)
        p.disp_score_threshold = F(disp_thr)
        _cache[key] = fine_to_coarse(oracle, make_field(name, dark).astype(F), -1.0, 1.0, D, p, mode, thr, accept_all_last_scale=accept,
                                     elem=elem, rule=rule, epi_scale_factor=epi_scale_factor)
    return _cache[key]


def pictures(depths, valids, fused_map, fused_valid, lut, volumes=None, shadow_level=0.0, saturate=True, s=-1, v=-1):
    """The three getters of rslf::FineToCoarse from a run's planes (render_ref): dict(maps [S,V,U,3], depth_pyr, epi_pyr).
    volumes: per level the normalised EPIs [V_p,S,U_p,C] with par_cut_shadows, else None."""
    return dict(maps=rr.f2c_coloured_depth_maps(fused_map, fused_valid, lut, saturate, None if volumes is None else volumes[0], shadow_level),
                depth_pyr=rr.f2c_coloured_depth_pyr(depths, valids, lut, s, saturate),
                epi_pyr=rr.f2c_coloured_epi_pyr(depths, valids, lut, v, saturate, volumes, shadow_level))
