"""numpy float32 restatement of the register scan's tap table (csrc/k2_taps.hpp, k2_reg.hpp): which gather batches of a frame
whose every pixel is scanned take their taps from the table, in the interior form and in the border form."""
from __future__ import annotations

import numpy as np

f32 = np.float32
BATCH = 8


def hypotheses(dmin: float, dmax: float, D: int) -> np.ndarray:
    """k2_scan.hpp, hypothesis(): dmin + (d * (dmax - dmin)) / (D - 1), one binary32 operation each."""
    d = np.arange(D, dtype=f32)
    rng = f32(f32(dmax) - f32(dmin))
    return (f32(dmin) + ((d * rng).astype(f32) / f32(D - 1)).astype(f32)).astype(f32)


def fast_entries(off: np.ndarray, u_first: int, u_last: int, U: int) -> np.ndarray:
    """tap_entry(...).fast for an array of view offsets and one tile [u_first, u_last] of a U-pixel row."""
    x0 = (off + f32(u_first)).astype(f32)
    x1 = (off + f32(u_last)).astype(f32)
    binade = ((x0.view(np.uint32) ^ x1.view(np.uint32)) >> 23) == 0
    exact = (x1 - f32(u_last)).astype(f32) == off
    return (x0 > 0) & (x1 <= f32(U - 1)) & (binade | exact)


def batch_shares(U: int, S: int, D: int, dmin: float, dmax: float, slope: float = 1.0, s_hat: int | None = None, tiles=None):
    """(interior-form, border-form) share of all gather batches that take the table: rows whose every pixel is scanned (tiles
    of 64 consecutive pixels, the last one shorter), scan_reg_rows' interior rule per (tile, hypothesis), whole batches of
    eight samples only (the batch that reaches past S takes the per-lane form).  `tiles`: a frame's real tiles instead, as
    (first pixel, last pixel, consecutive) each; a tile with a gap takes no taps from the table."""
    s_hat = S // 2 if s_hat is None else s_hat
    Dd = hypotheses(dmin, dmax, D)
    ds = (s_hat - np.arange(S)).astype(f32)
    off = ((ds[None, :] * Dd[:, None]).astype(f32) * f32(slope)).astype(f32)          # [D][S]
    reach = (((f32(max(s_hat, S - 1 - s_hat)) * np.abs(Dd)).astype(f32) * f32(abs(slope))).astype(f32) + f32(2)).astype(f32)
    whole = S // BATCH
    total = fast_in = fast_border = 0
    if tiles is None:
        tiles = [(u0, min(u0 + 63, U - 1), True) for u0 in range(0, U, 64)]
    for u0, u1, consecutive in tiles:
        interior = ((f32(u0) - reach).astype(f32) >= 0) & ((f32(u1) + reach).astype(f32) <= f32(U - 1))
        ok = fast_entries(off, u0, u1, U)[:, :whole * BATCH].reshape(D, whole, BATCH).all(axis=2)
        total += D * ((S + BATCH - 1) // BATCH)
        if not consecutive:
            continue
        fast_in += int((ok & interior[:, None]).sum())
        fast_border += int((ok & ~interior[:, None]).sum())
    return fast_in / total, fast_border / total
