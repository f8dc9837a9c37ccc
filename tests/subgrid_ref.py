"""numpy restatement of the sub-grid pile step (include/rslf_hip.h, rslf_subgrid_refine and the *_sub entries), written from
the rule's text and composed of the oracle's public functions: a pixel's scores are oracle_np.scan_pixel's row, the rule is
peaks_ref's, the filter oracle_np.selective_median.  Also the planted-line field the CPU and GPU tests share."""
import numpy as np

import peaks_ref as pr
from oracle import oracle_np as onp

F = np.float32


def disp3(a, s1, c, idx, D, lo, hi):
    """The rule in its three-score form: the winner idx scored s1, its neighbours a (idx - 1) and c (idx + 1); a and c are not
    read at the ends of the grid.  Every operation one binary32 operation."""
    lo, hi = F(lo), F(hi)
    rng = F(hi - lo)
    denom = F(D - 1)
    Dd = F(lo + F(F(F(idx) * rng) / denom))
    if idx == 0 or idx == D - 1:
        delta = F(0)
    else:
        a, s1, c = F(a), F(s1), F(c)
        num = F(a - c)
        den = F(F(a + c) - F(s1 + s1))
        den2 = F(den + den)
        delta = F(0) if den2 == 0 else F(num / den2)
        delta = min(max(delta, F(-0.5)), F(0.5))
    return F(Dd + F(delta * F(rng / denom)))


def grid_value(idx, D, lo, hi):
    lo, hi = F(lo), F(hi)
    return F(lo + F(F(F(idx) * F(hi - lo)) / F(D - 1)))


def refine(vol, idx, lo, hi, D, s_hat, p, fill=F(0), scan_plane=False):
    """(disp, left, right) planes [V, U] of a volume [V, S, U, C] and an arg-max plane idx: at every pixel with idx >= 0 the
    row of oracle_np.scan_pixel through the rule; `fill` elsewhere.  lo / hi: scalars or [V, U] planes.  Where idx is the row's
    arg max disp is also checked against peaks_ref's; scan_plane: idx is a scan's plane, so it must be the arg max everywhere."""
    V, S, U, C = vol.shape
    lo, hi = np.broadcast_to(F(lo), (V, U)), np.broadcast_to(F(hi), (V, U))
    disp, left, right = (np.full((V, U), fill, F) for _ in range(3))
    for v, u in zip(*np.nonzero(idx >= 0)):
        row = onp.scan_pixel(vol[v], int(u), lo[v, u], hi[v, u], D, s_hat, p)[1]
        i = int(idx[v, u])
        a = row[i - 1] if i > 0 else F(0)
        c = row[i + 1] if i < D - 1 else F(0)
        disp[v, u] = disp3(a, row[i], c, i, D, lo[v, u], hi[v, u])
        left[v, u], right[v, u] = a, c
        whole = pr.peaks_ref(row, lo[v, u], hi[v, u])
        assert whole[0] == i or not scan_plane, "pixel (%d, %d): the plane holds %d, the row's arg max is %d" % (v, u, i, whole[0])
        if whole[0] == i:
            assert whole[2].view(np.uint32) == disp[v, u].view(np.uint32)
    return disp, left, right


def pile_run(vol, dmin, dmax, D, s_hat=-1, p=None):
    """oracle_np.depth1d_pile_run, then the sub-grid step: out["depth_raw_sub"] is the raw plane with every assigned disparity
    refined, out["depth_sub"] its selective median.  Every other plane is the grid run's."""
    p = p or onp.default_params()
    out = onp.depth1d_pile_run(vol, dmin, dmax, D, s_hat, p)
    S = vol.shape[1]
    if s_hat < 0 or s_hat > S - 1:
        s_hat = int(np.floor((0.0 + S) / 2))
    disp = refine(vol, out["idx"], dmin, dmax, D, s_hat, p)[0]
    out["depth_raw_sub"] = np.where(out["idx"] >= 0, disp, out["depth_raw"]).astype(F)
    out["depth_sub"] = onp.selective_median(out["depth_raw_sub"], vol, s_hat, out["Ce_mask"], p["median_filter_size"],
                                            p["median_filter_epsilon"])
    return out


def planted_field(d_true, V=7, U=96):
    """V scanlines of the planted line of disparity d_true, scanline v shifted by v pixels: [V, 9, U, 1] float32."""
    wide = pr.planted_epi(d_true, S=9, U=U + 8, s_hat=4)
    return np.stack([wide[:, v:v + U] for v in range(V)])[..., None].astype(F)
