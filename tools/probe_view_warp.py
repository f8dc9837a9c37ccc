"""The view warp (rslf_view_warp, K14) at the sweep shapes: every view leave-one-out in one call, timed by HIP events and
alternating, round by round, with a K12 launch (rslf_view_consistency) on the same planes -- and, unless --no-sweep, the 2-D
sweep of the same field and get_view_prediction on its planes with the default and the consistent mask.

    python tools/probe_view_warp.py [--config c2|c3] [--reps 3] [--rounds 3] [--radius 8] [--no-sweep]
    rocprofv3 --pmc FETCH_SIZE -d OUT --output-format csv -- python tools/probe_view_warp.py --config c3 --pmc-run [--radius R]

The synthetic fields of remotesensingproject_amd/synth.py, as bench.py --path sweep2d builds them.  The planes timed are the
`truth` planes of tools/probe_consistency.py: the scene's own disparity per scanline with 5 % of the pixels replaced by uniform
values of the hypothesis range and 10 % invalid -- no sweep needed, the same in every process.  Variants, each once per ROUND,
each figure the median of --reps launches after a warm-up, the summary the median over the rounds and the spread:

  warp/loo            hit, err, row_err, row_hits (what get_view_prediction asks for), T = S targets, every view
  warp/loo/radius     the same with --radius
  warp/geometry       hit, depth, src_view, src_col: no volume
  warp/geometry+count ... and the candidate counts (the COUNT instantiation: 12 bytes of LDS per column for 8)
  k12/all             rslf_view_consistency, every view, all six planes
  k12/radius          ... with --radius

algorithmic_bytes: plan::warp_bytes of the loo variant -- the S source rows of a scanline read once for all targets, two slab
rows per target row, the planes written once.  --pmc-run: nothing but --launches launches of warp/loo, for a counter pass of its
own: rocprofv3's per-dispatch FETCH_SIZE of k14_view_warp against the algorithmic bytes printed here.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=["c2", "c3"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sweep-reps", type=int, default=2)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--pmc-run", action="store_true")
    ap.add_argument("--launches", type=int, default=2)
    args = ap.parse_args()

    import numpy as np
    import torch
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd import depth as rs
    from remotesensingproject_amd.synth import CONFIGS, make_lightfield

    cfg = dict(CONFIGS[args.config])
    U, V, S, C_, D = cfg["U"], cfg["V"], cfg["S"], cfg["C"], cfg["D"]
    dmin, dmax = cfg["dmin"], cfg["dmax"]
    torch.cuda.set_device(0)
    ctx = rs.default_context(0)
    L = _lib.lib()
    n = S * V * U
    tol = rs.grid_step(dmin, dmax, D, "probe")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(f) -> float:
        ev[0].record()
        f()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1])

    def median_ms(f, reps) -> float:
        f()   # warm-up
        torch.cuda.synchronize()
        return statistics.median(timed(f) for _ in range(reps))

    host, delta = make_lightfield(U, V, S, C_, seed=cfg["seed"], dmin=dmin, dmax=dmax)
    vol = rs.Volume.from_dense(torch.from_numpy(host).cuda(), 1.0, ctx)
    del host
    rng = np.random.default_rng(12)
    truth = np.broadcast_to(np.asarray(delta, np.float32)[None, :, None], (S, V, U)).copy()
    wild = rng.random((S, V, U), dtype=np.float32) < 0.05
    truth[wild] = rng.uniform(dmin, dmax, int(wild.sum())).astype(np.float32)
    depth = torch.from_numpy(truth).cuda()
    mask = torch.from_numpy(np.where(rng.random((S, V, U), dtype=np.float32) < 0.10, 0, 255).astype(np.uint8)).cuda()
    del truth, wild

    T = S
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device="cuda")
    w = dict(hit=new((T, V, U), torch.uint8), depth=new((T, V, U), torch.float32), src_view=new((T, V, U), torch.int32),
             src_col=new((T, V, U), torch.int32), count=new((T, V, U), torch.int32), err=new((T, V, U), torch.float32),
             row_err=new((T, V), torch.float64), row_hits=new((T, V), torch.int32))
    sets = dict(loo=("hit", "err", "row_err", "row_hits"), geometry=("hit", "depth", "src_view", "src_col"),
                count=("hit", "depth", "src_view", "src_col", "count"))
    c_out = {k: _lib.RslfViewWarpOut(**{name: w[name].data_ptr() for name in names}) for k, names in sets.items()}
    targets = (C.c_float * T)(*[float(s) for s in range(S)])
    exclude = (C.c_int * T)(*range(S))
    k12 = dict(seen=new((S, V, U), torch.int32), agree=new((S, V, U), torch.int32), above=new((S, V, U), torch.int32),
               below=new((S, V, U), torch.int32), fused=new((S, V, U), torch.float32), valid=new((S, V, U), torch.uint8))
    counts = _lib.RslfViewCounts(*(k12[k].data_ptr() for k in ("seen", "agree", "above", "below")))
    ctx.use_current_stream()

    def warp(which, radius):
        _lib.check(L.rslf_view_warp(ctx._h, depth.data_ptr(), mask.data_ptr(), S, V, U, 1.0, vol._h if which == "loo" else None, targets,
                                    exclude, T, radius, 1, C.byref(c_out[which])), "rslf_view_warp")

    def consistency(radius):
        _lib.check(L.rslf_view_consistency(ctx._h, depth.data_ptr(), mask.data_ptr(), S, V, U, 1.0, tol, radius, 1, C.byref(counts),
                                           k12["fused"].data_ptr(), k12["valid"].data_ptr()), "rslf_view_consistency")

    cells = T * V * U
    out = dict(config=args.config, U=U, V=V, S=S, C=C_, D=D, T=T, lds_atomics=n * (S - 1),
               algorithmic_bytes=dict(loo=n * 5 + cells * (2 * 4 * C_ + 5) + T * V * 12, geometry=n * 5 + cells * 13,
                                      k12_all=n * 26))
    if args.pmc_run:
        for _ in range(args.launches):
            warp("loo", args.radius if args.radius > 0 else 0)
        torch.cuda.synchronize()
        out.update(radius=args.radius, launches=args.launches)
        print(json.dumps(out), flush=True)
        return

    variants = [("warp/loo", lambda: warp("loo", 0)), ("k12/all", lambda: consistency(0)),
                ("warp/loo/radius%d" % args.radius, lambda: warp("loo", args.radius)), ("k12/radius%d" % args.radius, lambda: consistency(args.radius)),
                ("warp/geometry", lambda: warp("geometry", 0)), ("warp/geometry+count", lambda: warp("count", 0))]
    got = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, f in variants:
            got[name].append(median_ms(f, args.reps))
    out["ms"] = {name: dict(median=round(statistics.median(ms), 4), spread=[round(min(ms), 4), round(max(ms), 4)]) for name, ms in got.items()}
    # what the warp found, so that a reader sees the z-buffer had work to do
    warp("count", 0)
    warp("loo", 0)
    torch.cuda.synchronize()
    hits = int(w["row_hits"].sum().item())
    out["truth"] = dict(coverage=round(hits / cells, 4), two_or_more=round(int((w["count"] >= 2).sum().item()) / cells, 4),
                        mean_candidates=round(float(w["count"].float().mean().item()), 2),
                        mean_abs_error=float(w["row_err"].sum().item()) / max(1, hits))

    if not args.no_sweep:
        comp = rs.Depth2DComputer(vol, dmin, dmax, D)
        out["sweep_ms"] = round(median_ms(lambda: comp.run(want_stats=False), args.sweep_reps), 3)
        for name, m in (("default_mask", None), ("consistent_mask", comp.get_consistent_depths_mask_s_v_u())):
            pred = comp.get_view_prediction(mask=m)
            out["prediction_" + name] = dict(mean_abs_error=round(float(np.nanmean(pred.mean_abs_error)), 6),
                                             coverage=round(float(pred.coverage.mean()), 4),
                                             worst_view=round(float(np.nanmax(pred.mean_abs_error)), 6))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
