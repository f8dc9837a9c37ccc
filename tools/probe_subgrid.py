"""The sub-grid refinement (rslf_subgrid_refine; k9_subgrid_refine) against what the same plane costs through the score rows,
same box.

    python tools/probe_subgrid.py [--config c3] [--alternations 3] [--reps 5] [--tree DIR]

The synthetic field of remotesensingproject_amd/synth.py, whole frame, every pixel confident (no mask).  HIP-event times on
the context's stream, each the median of --reps runs after one warm-up, the modes ALTERNATING --alternations times; the
figures of record are the medians over the alternations.  --tree DIR imports the package from another checkout (the parent
commit's, built there): the modes that build lacks are left out, so fresh processes of the two builds can alternate on one
box (measuring on the MI355X: never compare across boxes or across a long gap).

  frame    rslf_depth_epi_peaks over the whole field: the score rows through the staging buffer, then k8_score_peaks
  scan     the pile step's scan over the whole field (rslf_last_scan_kernel_ms)
           frame - scan is what the sub-grid plane costs through the rows: THE BAR for `refine`, taken on the parent's build
  refine   rslf_subgrid_refine alone on the scan's idx and score planes, disp only
  own      the same without the score plane (three hypotheses a pixel)
  pile0    rslf_depth1d_pile_run_sub(subgrid = 0) (the parent: rslf_depth1d_pile_run), the whole pile step
  pile1    rslf_depth1d_pile_run_sub(subgrid = 1)

Prints one JSON line per alternation and one summary line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))

    import torch
    from remotesensingproject_amd import depth as rs
    from remotesensingproject_amd.synth import CONFIGS, make_lightfield

    has_subgrid = hasattr(rs, "subgrid_refine")
    cfg = dict(CONFIGS[args.config])
    U, V, S, C, D = cfg["U"], cfg["V"], cfg["S"], cfg["C"], cfg["D"]
    torch.cuda.set_device(0)
    ctx = rs.default_context(0)
    host, _ = make_lightfield(U, V, S, C, seed=cfg["seed"], dmin=cfg["dmin"], dmax=cfg["dmax"])
    vol = rs.Volume.from_dense(torch.from_numpy(host).cuda(), 1.0, ctx)
    s_hat = S // 2
    params = rs.Depth1DParameters()
    dev = ctx.device
    dmin, dmax = cfg["dmin"], cfg["dmax"]
    frame = rs.Peaks(*(torch.empty((V, U), dtype=torch.int32 if n.endswith("idx") else torch.float32, device=dev) for n in rs.Peaks._fields))
    Ce = torch.empty((V, U), dtype=torch.float32, device=dev)
    mask = torch.empty((V, U), dtype=torch.uint8, device=dev)
    Cd, depth, score, disp, own = (torch.empty_like(Ce) for _ in range(5))
    idx = torch.empty((V, U), dtype=torch.int32, device=dev)
    rbar = torch.empty((V, U, C), dtype=torch.float32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(f):
        def run() -> float:
            ev[0].record()
            f()
            ev[1].record()
            ev[1].synchronize()
            return ev[0].elapsed_time(ev[1])
        return run

    def scan_ms() -> float:
        Ce.fill_(1.0)
        mask.fill_(255)   # every pixel confident
        rs.compute_1D_depth_epi(vol, dmin, dmax, D, s_hat, Ce, mask, Cd, depth, rbar, params, idx_v_u=idx, score_v_u=score)
        torch.cuda.synchronize()
        return ctx.last_scan_kernel_ms()

    piles = {sub: rs.Depth1DComputer_pile(vol, dmin, dmax, D, s_hat, 1.0, params, **(dict(subgrid=bool(sub)) if has_subgrid else {}))
             for sub in ((0, 1) if has_subgrid else (0,))}
    modes = [("frame", timed(lambda: rs.compute_1D_depth_peaks(vol, dmin, dmax, D, s_hat, params, None, 0, V, frame))), ("scan", scan_ms)]
    if has_subgrid:
        modes += [("refine", timed(lambda: rs.subgrid_refine(vol, dmin, dmax, D, s_hat, idx, score, params, disp=disp, neighbours=False))),
                  ("own", timed(lambda: rs.subgrid_refine(vol, dmin, dmax, D, s_hat, idx, None, params, disp=own, neighbours=False)))]
    modes += [("pile%d" % sub, timed(lambda c=comp: c.run(want_stats=False))) for sub, comp in piles.items()]

    scan_ms()   # (the planes `refine` reads)
    per = {name: [] for name, _ in modes}
    for a in range(args.alternations):
        line = {"alternation": a}
        for name, f in modes:
            f()   # warm-up
            ms = statistics.median(f() for _ in range(args.reps))
            per[name].append(ms)
            line[name + "_ms"] = round(ms, 4)
        print(json.dumps(line), flush=True)
    med = {name: statistics.median(v) for name, v in per.items()}
    out = dict(config=args.config, tree=os.path.abspath(args.tree), subgrid=has_subgrid, U=U, V=V, S=S, C=C, D=D, pixels=V * U,
               frame_ms=round(med["frame"], 4), scan_ms=round(med["scan"], 4), rows_cost_ms=round(med["frame"] - med["scan"], 4),
               pile0_ms=round(med["pile0"], 4))
    if has_subgrid:
        # the refinement and the rows agree on every pixel, with and without the score plane
        torch.cuda.synchronize()
        out.update(refine_ms=round(med["refine"], 4), own_ms=round(med["own"], 4), pile1_ms=round(med["pile1"], 4),
                   pile1_over_pile0=round(med["pile1"] / med["pile0"], 4), refine_over_rows_cost=round(med["refine"] / (med["frame"] - med["scan"]), 4),
                   refine_equals_peaks=bool((disp.view(torch.int32) == frame.disp.view(torch.int32)).all().item()),
                   own_equals_refine=bool((own.view(torch.int32) == disp.view(torch.int32)).all().item()))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
