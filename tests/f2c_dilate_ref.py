"""The yardstick of the level dilation (include/rslf_hip.h, rslf_f2c_run_host_dl; tests only): numpy, composed of public
pieces.  Never the HIP path against itself.

It is f2c_keep_ref.fine_to_coarse with the level's SWEEP moved into a frame dilated along u by f.  Per level:
  * dilate_ref.dilate(vol, f, kind) on the level's normalised volume (the clamp range is that volume's min and max);
  * the level's ranges [S,V,U] -> [S,V,U'] by the union rule (dilate_ranges): column i f takes column i's range, the columns
    between i and i + 1 take min(dmin[i], dmin[i + 1]) and max(dmax[i], dmax[i + 1]); of equal values the left one's bits,
    and a NaN loses to a number (fminf / fmaxf with what C leaves open stated);
  * f2c_line_conf_ref.sweep with slope_factor = F(F(p.slope_factor) * F(f));
  * every returned plane cut to [:, :, ::f];
  * validity, oracle.f2c_tighten_bounds and oracle.f2c_fuse as before, on the level's own grid.
The dilation never enters the level chain: f2c_keep_ref.pyramid is untouched, and `volumes` are the undilated levels.

With subgrid / peaks the sweep is sweep_peaks_ref.sweep (which is sweep_subgrid_ref's loop plus the peak planes) fed the
same dilated volume, ranges and slope; uniqueness (f2c_peaks_ref.ambiguous), the consistency gate
(f2c_consistency_ref.gate_level, at the level's OWN slope) and the origin walk then run on the cut planes.

Also the field of the issue: small_slope_pyramid_field, a small-slope texture coherent across scanlines."""
import numpy as np

import dilate_ref as dlr
import f2c_keep_ref as kr
import f2c_line_conf_ref as fr

F = np.float32
LINEAR, CUBIC, LANCZOS3 = dlr.LINEAR, dlr.CUBIC, dlr.LANCZOS3


def ranges_min(a, b):
    """fminf with the left operand on ties (so -0.0 / +0.0 keep the left one's sign) and a NaN losing to a number."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return np.where((a <= b) | np.isnan(b), a, b).astype(F)


def ranges_max(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return np.where((a >= b) | np.isnan(b), a, b).astype(F)


def dilate_ranges(dmin, dmax, f):
    """[..., U] float32 -> [..., f (U - 1) + 1]: the union rule."""
    dmin, dmax = np.asarray(dmin, F), np.asarray(dmax, F)
    U = dmin.shape[-1]
    lo = np.zeros(dmin.shape[:-1] + (dlr.dilated_width(U, f),), F)
    hi = np.zeros_like(lo)
    lo[..., ::f], hi[..., ::f] = dmin, dmax
    for p in range(1, f):
        lo[..., p::f] = ranges_min(dmin[..., :-1], dmin[..., 1:])
        hi[..., p::f] = ranges_max(dmax[..., :-1], dmax[..., 1:])
    return lo, hi


def dilated_params(p, f):
    """A copy of the level's parameters for the dilated frame: one binary32 product."""
    q = type(p).from_buffer_copy(p)
    q.slope_factor = F(F(p.slope_factor) * F(f))
    return q


def _cut(planes, f):
    return {k: (np.ascontiguousarray(v[:, :, ::f]) if isinstance(v, np.ndarray) else v) for k, v in planes.items()}


def level_sweep(oracle, vol, lo, hi, D, p, f, kind, subgrid=False, peaks=False, line_score_threshold=0.02):
    """One level's sweep in the frame dilated by f -> (planes cut to the level's grid, peak planes cut or None, pixels the
    sweep scanned in the dilated frame or None where the peaks' loop ran, which does not count them)."""
    if f == 1:
        vol_d, lo_d, hi_d, q = vol, lo, hi, p
    else:
        vol_d = dlr.dilate(vol, f, kind)
        lo_d, hi_d = dilate_ranges(lo, hi, f)
        q = dilated_params(p, f)
    if subgrid or peaks:
        import sweep_peaks_ref as spr
        r, pk, _ = spr.sweep(oracle, vol_d, lo_d, hi_d, D, q, 0, line_score_threshold, subgrid=subgrid)
        return _cut(r, f), (_cut(pk, f) if peaks else None), None
    r, n = fr.sweep(oracle, vol_d, lo_d, hi_d, D, q, 0, line_score_threshold)
    return _cut(r, f), None, n


def fine_to_coarse(oracle, raw_vsuc, dmin, dmax, D, f=1, kind=CUBIC, params=None, max_pyr_depth=-1, accept_all_last_scale=True,
                   elem="f32", rule=kr.COMPAT, epi_scale_factor=-1.0, subgrid=False, peaks=False, ratio=0.0, min_agree=0, tol=0.0,
                   radius=0):
    """f2c_keep_ref.fine_to_coarse (mode 0) with every level's sweep dilated by f.  Returns its dict; with peaks also per
    level `pk` and fused_pk / fused_level; with min_agree per level `inconsistent`."""
    vols, scales, pars = kr.pyramid(oracle, raw_vsuc, params, max_pyr_depth, elem, epi_scale_factor)
    S = vols[0].shape[1]
    levels, total = [], 0
    for l, (vol, p) in enumerate(zip(vols, pars)):
        Vp, Up = vol.shape[0], vol.shape[2]
        lo = np.full((S, Vp, Up), dmin, F); hi = np.full((S, Vp, Up), dmax, F)
        if l > 0:
            lo, hi = oracle.f2c_tighten_bounds(levels[-1]["depth"], levels[-1]["valid"], lo, hi)
        r, pk, n = level_sweep(oracle, vol, lo, hi, D, p, f, kind, subgrid, peaks)
        total = None if (n is None or total is None) else total + n
        accept_all = accept_all_last_scale and l == len(vols) - 1
        valid = kr.validity(r, p, 0, 0.02, accept_all, rule)
        if peaks and ratio > 0 and not accept_all:
            import f2c_peaks_ref as pf
            valid = np.where((valid != 0) & pf.ambiguous(pk, ratio), 0, valid).astype(np.uint8)
        r["inconsistent"] = 0
        if min_agree > 0 and not accept_all:
            import f2c_consistency_ref as fcr
            valid, _, _, drop, _ = fcr.gate_level(r["depth"], valid, p.slope_factor, tol, radius, min_agree)   # the level's own slope
            r["inconsistent"] = int(drop.sum())
        r["valid"], r["dmin"], r["dmax"], r["pk"] = valid, lo, hi, pk
        levels.append(r)
    fused = np.zeros((S,) + levels[0]["depth"].shape[1:], F)
    fvalid = np.zeros(fused.shape, np.uint8)
    for s in range(S):
        fused[s], fvalid[s] = oracle.f2c_fuse([lv["depth"][s] for lv in levels], [lv["valid"][s] for lv in levels])
    out = dict(levels=levels, dims=[(v.shape[0], v.shape[2]) for v in vols], volumes=vols, scales=scales, fused_map=fused,
               fused_valid=fvalid, pixels_scanned=total)
    if peaks:
        import f2c_peaks_ref as pf
        out["fused_pk"], out["fused_level"] = pf.origin_walk([lv["valid"] for lv in levels], [lv["pk"] for lv in levels])
    return out


_cache = {}


def reference(oracle, name, f, kind, **kw):
    """fine_to_coarse on a case of f2c_line_conf_ref.CASES, range [-1, 1]; computed once per session and shared (callers must
    not write into it).  kw: subgrid, peaks, ratio, min_agree, tol, radius, and derivative (a weight: the raw one-channel field
    goes in as derivative_ref.augment's three channels)."""
    key = (name, int(f), int(kind)) + tuple(sorted(kw.items()))
    if key not in _cache:
        C, elem, V, U, S, D, accept = kr.case_of(name)
        field = kr.make_field(name).astype(F)
        kw = dict(kw)
        weight = kw.pop("derivative", 0.0)
        if weight:
            import derivative_ref as dref
            field = dref.augment(field, weight, elem)
        _cache[key] = fine_to_coarse(oracle, field, -1.0, 1.0, D, f, kind, oracle.default_params(), accept_all_last_scale=accept,
                                     elem=elem, **kw)
    return _cache[key]


# ---- the field of the issue: a small-slope texture coherent across scanlines, two pyramid levels ----------------------

FIELD_V, FIELD_S, FIELD_U = 24, 9, 96
FIELD_D, FIELD_DMIN, FIELD_DMAX = 241, -0.6, 0.6
FIELD_MARGIN = 12


def small_slope_pyramid_field(seed, V=FIELD_V, S=FIELD_S, U=FIELD_U):
    """(vol [V,S,U,1] float32 in [0, 1], delta [V]).  One texture for the whole field, 24 sinusoids whose frequency along v is
    small, so it survives the pyramid's 7 x 7 Gaussian; scanline v has the slope delta_v = linspace(-0.45, 0.45, V)[v]."""
    rng = np.random.default_rng(seed)
    fx = rng.uniform(0.02, 0.40, 24)
    fy = rng.uniform(-0.03, 0.03, 24)
    a = rng.uniform(0.2, 1.0, 24) / np.sqrt(24) * 0.6
    ph = rng.uniform(0, 2 * np.pi, 24)
    delta = np.linspace(-0.45, 0.45, V)
    u = np.arange(U, dtype=np.float64)
    vol = np.zeros((V, S, U, 1), F)
    for v in range(V):
        for s in range(S):
            x = u - (S // 2 - s) * delta[v]
            t = np.sum(a[:, None] * np.sin(2 * np.pi * (fx[:, None] * x[None, :] + fy[:, None] * v) + ph[:, None]), 0)
            vol[v, s, :, 0] = np.clip(0.5 + 0.35 * t / 0.36, 0.0, 1.0).astype(F)
    return vol, delta


def field_errors(fused_map, level0_depth, level0_valid, delta, U=FIELD_U):
    """(fused MAE, level-0 MAE) against the truth over columns 12 .. U - 13: the first over all views and scanlines, the
    second over level 0's valid pixels."""
    cols = slice(FIELD_MARGIN, U - FIELD_MARGIN)
    truth = delta[None, :, None]
    fused = float(np.abs(fused_map[:, :, cols].astype(np.float64) - truth).mean())
    sel = level0_valid[:, :, cols] != 0
    err0 = np.abs(level0_depth[:, :, cols].astype(np.float64) - truth)
    return fused, float(err0[sel].mean())
