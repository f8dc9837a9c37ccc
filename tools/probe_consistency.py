"""The cross-view consistency check (rslf_view_consistency, K12) at the sweep shapes: kernel time with every view and with a
radius, against a device copy of its algorithmic bytes and against the 2-D sweep whose planes it checks -- all in one process,
the variants alternating round by round.

    python tools/probe_consistency.py [--config c2|c3|mansion_lr] [--reps 5] [--rounds 3] [--radius 8] [--no-sweep]
    rocprofv3 --pmc FETCH_SIZE -d OUT --output-format csv -- python tools/probe_consistency.py --config c3 --pmc-run [--order N] [--radius R]

The synthetic fields of remotesensingproject_amd/synth.py, as bench.py --path sweep2d builds them.  Two plane sets are checked:

  sweep   the disparities and the validity mask of Depth2DComputer.run() on the field (skipped with --no-sweep); the sweep's
          time -- the median of --sweep-reps runs -- is taken here too: this pull request does not touch it
  truth   the scene's own disparity per scanline with 5 % of the pixels replaced by uniform values of the hypothesis range and
          10 % invalid: no sweep needed, the same in every process -- what the counter passes run on

HIP-event times on the current stream; every variant once per ROUND, --rounds rounds, each figure the median of --reps
launches after a warm-up; the summary holds the median over the rounds and the spread (min .. max).  Variants: the three grid
orders ("consistency_order" 0 / 1 / 2) with every view and all six outputs, order 0 with --radius, order 0 with the valid plane
alone, and the floors: a device copy of 5 B per cell plus a fill of the output bytes (21 B or 1 B per cell).

--pmc-run: nothing but --launches launches of the kernel on the truth planes (all six outputs), for a counter pass of its own:
rocprofv3's per-dispatch FETCH_SIZE / WRITE_SIZE of k12_view_consistency against `algorithmic_bytes` printed here.
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
    ap.add_argument("--config", default="c2", choices=["c2", "c3", "mansion_lr"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sweep-reps", type=int, default=2)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--pmc-run", action="store_true")
    ap.add_argument("--order", type=int, default=0)
    ap.add_argument("--launches", type=int, default=3)
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

    # the truth planes: made on the host from a seed, no device work
    if args.pmc_run or args.no_sweep:
        from remotesensingproject_amd.synth import band_disparities
        delta = band_disparities(V, dmin, dmax)
        host = None
    else:
        host, delta = make_lightfield(U, V, S, C_, seed=cfg["seed"], dmin=dmin, dmax=dmax)
    rng = np.random.default_rng(12)
    truth = np.broadcast_to(np.asarray(delta, np.float32)[None, :, None], (S, V, U)).copy()
    wild = rng.random((S, V, U), dtype=np.float32) < 0.05
    truth[wild] = rng.uniform(dmin, dmax, int(wild.sum())).astype(np.float32)
    planes = dict(truth=(torch.from_numpy(truth).cuda(), torch.from_numpy(np.where(rng.random((S, V, U), dtype=np.float32) < 0.10, 0, 255)
                                                                         .astype(np.uint8)).cuda()))
    del truth, wild

    outs = dict(seen=torch.empty((S, V, U), dtype=torch.int32, device="cuda"), agree=torch.empty((S, V, U), dtype=torch.int32, device="cuda"),
                above=torch.empty((S, V, U), dtype=torch.int32, device="cuda"), below=torch.empty((S, V, U), dtype=torch.int32, device="cuda"),
                fused=torch.empty((S, V, U), dtype=torch.float32, device="cuda"), valid=torch.empty((S, V, U), dtype=torch.uint8, device="cuda"))
    all_counts = _lib.RslfViewCounts(*(outs[k].data_ptr() for k in ("seen", "agree", "above", "below")))
    no_counts = _lib.RslfViewCounts()
    ctx.use_current_stream()

    def launch(which, radius, full):
        d, m = planes[which]
        _lib.check(L.rslf_view_consistency(ctx._h, d.data_ptr(), m.data_ptr(), S, V, U, 1.0, tol, radius, 1,
                                           C.byref(all_counts if full else no_counts), outs["fused"].data_ptr() if full else None,
                                           outs["valid"].data_ptr()), "rslf_view_consistency")

    out = dict(config=args.config, U=U, V=V, S=S, C=C_, D=D, tol=tol, cells=n, gathers=n * (S - 1),
               algorithmic_bytes=dict(all=n * 26, valid_only=n * 6))
    if args.pmc_run:
        ctx.set_debug(consistency_order=args.order)
        for _ in range(args.launches):
            launch("truth", args.radius if args.radius > 0 else 0, True)
        torch.cuda.synchronize()
        out.update(order=args.order, radius=args.radius, launches=args.launches)
        print(json.dumps(out), flush=True)
        return

    if host is not None:
        vol = rs.Volume.from_dense(torch.from_numpy(host).cuda(), 1.0, ctx)
        comp = rs.Depth2DComputer(vol, dmin, dmax, D)
        out["sweep_ms"] = round(median_ms(lambda: comp.run(want_stats=False), args.sweep_reps), 3)
        planes["sweep"] = (comp.get_depths_s_v_u(), comp.get_valid_depths_mask_s_v_u().contiguous())
        ctx.use_current_stream()

    # the floors: a copy of the 5 input bytes per cell and a fill of the other output bytes
    src5, dst5 = torch.empty(n * 5, dtype=torch.uint8, device="cuda"), torch.empty(n * 5, dtype=torch.uint8, device="cuda")
    rest16, rest1 = torch.empty(n * 4, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")

    def floor_all():
        dst5.copy_(src5)
        rest16.zero_()

    def floor_valid():
        dst5.copy_(src5)
        rest1.zero_()

    variants = []
    for which in planes:
        for order in (0, 1, 2):
            variants.append(("%s/all/order%d" % (which, order), order, lambda w=which: launch(w, 0, True)))
        variants.append(("%s/radius%d/order0" % (which, args.radius), 0, lambda w=which: launch(w, args.radius, True)))
        variants.append(("%s/all/valid_only" % which, 0, lambda w=which: launch(w, 0, False)))
        variants.append(("%s/radius%d/valid_only" % (which, args.radius), 0, lambda w=which: launch(w, args.radius, False)))
    variants += [("floor/copy5+fill16", 0, floor_all), ("floor/copy5+fill1", 0, floor_valid)]
    got = {name: [] for name, _, _ in variants}
    for _ in range(args.rounds):
        for name, order, f in variants:
            ctx.set_debug(consistency_order=order)
            got[name].append(median_ms(f, args.reps))
    ctx.reset_debug()
    out["ms"] = {name: dict(median=round(statistics.median(ms), 4), spread=[round(min(ms), 4), round(max(ms), 4)]) for name, ms in got.items()}
    # what the check found, so that a reader sees the planes were working ones
    for which in planes:
        launch(which, 0, True)
        torch.cuda.synchronize()
        ok = (planes[which][1] != 0) & torch.isfinite(planes[which][0])
        k = max(1, int(ok.sum().item()))
        out["shares_" + which] = dict(ok=round(k / n, 4), agree=round(int((outs["agree"][ok] > 0).sum().item()) / k, 4),
                                      above=round(int((outs["above"][ok] > 0).sum().item()) / k, 4),
                                      below=round(int((outs["below"][ok] > 0).sum().item()) / k, 4),
                                      mean_seen=round(float(outs["seen"][ok].float().mean().item()), 2))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
