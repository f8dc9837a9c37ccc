"""The derivative channels (K17) on a field built for them: what the pyramid does with the option off and at a few weights,
and what the kernel costs.

    python tools/probe_derivative_channels.py [--weights 0.5,1,2,4] [--size 256] [--views 9] [--dim-d 33] [--reps 5] [--rounds 3]
                                              [--configs c2,c3] [--tree DIR]

--tree DIR: import the package from another checkout (another build of the library) instead of this one.

The field: one channel, V = U = --size, S = --views.  The scanlines come in bands of V / 8 rows; each band has its own
disparity (eight distinct values across [-1, 1]) and every band has the SAME mean (0.5): within a band every scanline is white
noise of its own, uniform in 0.5 +- 0.2 -- fine texture that the 7 x 7 Gaussian and the halving erase, so that a level or two
down the intensity is flat.  View s of scanline v is the texture sampled at u - (s_hat - s) * delta(v), by a float64 lerp.  The
truth of every pixel is its band's disparity.

Per run (off, then each weight), from a kept run (fine_to_coarse_run_host(keep=True)):
  every level's share of valid pixels; the fused map's share of valid pixels and its mean absolute error against the truth
  over them, and over every pixel; get_view_prediction of the fused planes (mean over the views of mean_abs_error, and the
  coverage -- with the option on the level-0 volume holds three channels, the features count in that error, so it is shown
  beside the off run's, not compared with it); the pyramid's wall time (median of --reps calls, host EPIs in).
K17 itself, at the (V, S, U) of the bench configs: the dense form on buffers allocated beforehand, an event pair around the one
launch, against a device-to-device copy that moves as many bytes (4 x the source: once in, three channels out -- a buffer of
8 n bytes copied once), alternating round by round; and the volume form's host time, which holds its allocation and the wait
for the range.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time


def make_field(np, size: int, views: int, seed: int = 7):
    """-> (epis: list of V arrays [S, U] float32, truth [V] float64)."""
    rng = np.random.default_rng(seed)
    V = U = size
    bands = 8
    deltas = np.linspace(-0.9, 0.9, bands)[rng.permutation(bands)]
    s_hat = views // 2
    x = np.arange(U, dtype=np.float64)
    epis, truth = [], np.empty(V)
    for v in range(V):
        d = deltas[min(v * bands // V, bands - 1)]
        truth[v] = d
        tex = 0.5 + rng.uniform(-0.2, 0.2, U + 64)          # (32 columns of margin at each end)
        epi = np.empty((views, U), np.float32)
        for s in range(views):
            pos = x - (s_hat - s) * d + 32.0
            i = np.floor(pos).astype(np.int64)
            f = pos - i
            epi[s] = ((1.0 - f) * tex[i] + f * tex[i + 1]).astype(np.float32)
        epis.append(epi)
    return epis, truth


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", default="0.5,1,2,4")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--views", type=int, default=9)
    ap.add_argument("--dim-d", type=int, default=33)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)

    import numpy as np
    import torch
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd import depth as rs
    from remotesensingproject_amd.synth import CONFIGS

    torch.cuda.set_device(0)
    ctx = rs.default_context(0)
    L = _lib.lib()
    out = dict(size=args.size, views=args.views, dim_d=args.dim_d, reps=args.reps, rounds=args.rounds, pyramid={}, k17={})

    # ---- the pyramid, off and at the weights -------------------------------------------------------------------------
    epis, truth = make_field(np, args.size, args.views)
    truth_svu = np.broadcast_to(truth[None, :, None], (args.views, args.size, args.size))
    dmin, dmax = -1.0, 1.0
    for w in [0.0] + [float(t) for t in args.weights.split(",") if t]:
        def call():
            return rs.fine_to_coarse_run_host(epis, dmin, dmax, args.dim_d, keep=True, ctx=ctx, derivative_channels=w)
        run = call()
        shares = [round(float((run.plane(l, "valid") != 0).float().mean()), 4) for l in range(run.n_levels)]
        fmap, fvalid = run.plane(0, "fused_map").cpu().numpy(), run.plane(0, "fused_valid").cpu().numpy() != 0
        err = np.abs(fmap.astype(np.float64) - truth_svu)
        pred = run.get_view_prediction()
        mae_views = np.asarray(pred.mean_abs_error, np.float64)
        row = dict(C=run.C, levels=run.dims, valid_share=shares, fused_valid_share=round(float(fvalid.mean()), 4),
                   fused_mae_valid=round(float(err[fvalid].mean()), 5) if fvalid.any() else None,
                   fused_mae_all=round(float(err.mean()), 5),
                   view_prediction_mae=round(float(np.nanmean(mae_views)), 6),
                   view_prediction_coverage=round(float(np.mean(np.asarray(pred.coverage, np.float64))), 4))
        run.close()
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call().close()
            times.append((time.perf_counter() - t0) * 1e3)
        row["pyramid_ms"] = dict(median=round(statistics.median(times), 3), spread=[round(min(times), 3), round(max(times), 3)])
        out["pyramid"]["off" if w == 0.0 else "w%g" % w] = row
        print("# %s: %s" % ("off" if w == 0.0 else "w=%g" % w, row), flush=True)

    # ---- K17 against a copy of the same bytes --------------------------------------------------------------------------
    def pair():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    for name in [c for c in args.configs.split(",") if c]:
        cfg = CONFIGS[name]
        U, V, S = cfg["U"], cfg["V"], cfg["S"]
        n = V * S * U
        x = torch.rand((V, S, U), device="cuda")
        y = torch.empty((V, S, U, 3), device="cuda")
        a, b = torch.empty(2 * n, device="cuda"), torch.empty(2 * n, device="cuda")      # 8 n bytes read, 8 n written
        a.fill_(1.0)
        ctx.use_current_stream()

        def copy_ms() -> float:
            e0, e1 = pair()
            e0.record()
            b.copy_(a)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        def k17_ms(elem: int) -> float:
            e0, e1 = pair()
            e0.record()
            rc = L.rslf_derivative_channels_dense(ctx._h, x.data_ptr(), elem, V, S, U, 1.0, 1.0, y.data_ptr())
            e1.record()
            e1.synchronize()
            assert rc == 0, L.rslf_last_error()
            return e0.elapsed_time(e1)

        k17_ms(0), copy_ms()   # warm-up
        got = dict(copy=[], f32=[], integer=[])
        for _ in range(args.rounds):
            got["copy"].append(statistics.median(copy_ms() for _ in range(args.reps)))
            got["f32"].append(statistics.median(k17_ms(0) for _ in range(args.reps)))
            got["integer"].append(statistics.median(k17_ms(2) for _ in range(args.reps)))
        moved = 16 * n
        copy = statistics.median(got["copy"])
        row = dict(U=U, V=V, S=S, bytes_moved=moved, rows_16_byte_aligned=(U % 4 == 0),
                   copy=dict(ms=round(copy, 4), spread=[round(min(got["copy"]), 4), round(max(got["copy"]), 4)], gbps=round(moved / copy / 1e6, 1)))
        for k in ("f32", "integer"):
            ms = statistics.median(got[k])
            row[k] = dict(ms=round(ms, 4), spread=[round(min(got[k]), 4), round(max(got[k]), 4)], gbps=round(moved / ms / 1e6, 1),
                          ratio_to_copy=round(ms / copy, 3))
        vol = rs.Volume.from_dense(x, 1.0, ctx)
        vol.with_derivative_channels(1.0).close()
        host = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v3 = vol.with_derivative_channels(1.0)
            host.append((time.perf_counter() - t0) * 1e3)
            v3.close()
        row["volume_form_host_ms"] = round(statistics.median(host), 3)
        vol.close()
        out["k17"][name] = row
        print("# %s: %s" % (name, row), flush=True)
        del x, y, a, b
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
