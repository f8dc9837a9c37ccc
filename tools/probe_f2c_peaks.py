"""A kept fine-to-coarse run (fine_to_coarse_run_host(keep=True)) with its peak planes off, on, and on with the uniqueness
ratio: what the two options cost, and what the ratio does to the pyramid.

    python tools/probe_f2c_peaks.py [--config c2|c3|skysat_lr|mansion_lr] [--reps 5] [--ratio 0.7] [--tree DIR] [--limit SECONDS]

The synthetic fields of remotesensingproject_amd/synth.py, as bench.py --path f2c builds them.  Every step runs in a child
process of its own under `timeout` (--limit seconds each), one after the other; the first one that fails ends the probe.
Wall-clock times of the whole call (host upload, every level, the fusion; the call waits for the device), each the median of
--reps runs after one warm-up.  --tree DIR imports the package from another checkout (the parent commit's, built there):
the steps that build lacks are left out, so fresh processes of the two builds can alternate on one box.

  off     keep=True, both options off
  peaks   peaks=True
  ratio   peaks=True, uniqueness_ratio=--ratio; reports each level's share of valid pixels and of fused_level
  dense   as `ratio` under "peaks_list" = 0 (every visit the dense form of the peaks step)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time


def child(args) -> None:
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd import depth as rs
    from remotesensingproject_amd.synth import CONFIGS, make_lightfield

    cfg = dict(CONFIGS[args.config])
    U, V, S, C_, D = cfg["U"], cfg["V"], cfg["S"], cfg["C"], cfg["D"]
    torch.cuda.set_device(0)
    ctx = rs.default_context(0)
    host, _ = make_lightfield(U, V, S, C_, seed=cfg["seed"], dmin=cfg["dmin"], dmax=cfg["dmax"])
    raw = (host * 200.0 + 3.0).astype(np.float32)
    epis = list(raw[..., 0]) if C_ == 1 else list(raw)
    has_mode = "rslf_f2c_run_host_pk" in _lib.SYMBOLS
    if args.step != "off" and not has_mode:
        raise SystemExit("this build has no peak planes in the pyramid")
    opts = {}
    if args.step in ("peaks", "ratio", "dense"):
        opts["peaks"] = True
    if args.step in ("ratio", "dense"):
        opts["uniqueness_ratio"] = args.ratio
    if args.step == "dense":
        ctx.set_debug(peaks_list=0)
    last = {}

    def once() -> float:
        if "run" in last:
            last.pop("run").close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last["run"] = rs.fine_to_coarse_run_host(epis, cfg["dmin"], cfg["dmax"], D, ctx=ctx, keep=True, keep_volumes=False, **opts)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    once()   # warm-up
    times = [once() for _ in range(args.reps)]
    run = last["run"]
    out = dict(step=args.step, config=args.config, tree=os.path.abspath(args.tree), has_mode=has_mode, U=U, V=V, S=S, C=C_, D=D,
               ms=round(statistics.median(times), 3), ms_min=round(min(times), 3), ms_max=round(max(times), 3), dims=run.dims,
               scanned_pixels=int(run.stats.pixels_scanned))
    valid = [run.plane(l, "valid") for l in range(run.n_levels)]
    out["valid_share"] = [round(float((v != 0).float().mean().item()), 4) for v in valid]
    if opts:
        _, level = run.get_fused_peaks()
        out["fused_level_share"] = [round(float((level == l).float().mean().item()), 4) for l in range(run.n_levels)]
        out["undecided_share"] = round(float((level == 255).float().mean().item()), 4)
        pk = run.get_peaks(0)
        out["level0_with_peaks"] = round(float((pk.idx >= 0).float().mean().item()), 4)
        out["level0_with_runner_up"] = round(float((pk.runner_idx >= 0).float().mean().item()), 4)
    print(json.dumps(out), flush=True)


def main() -> None:
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=["c2", "c3", "skysat_lr", "mansion_lr"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ratio", type=float, default=0.7)
    ap.add_argument("--tree", default=here)
    ap.add_argument("--limit", type=int, default=240, help="seconds every step may take (its own timeout)")
    ap.add_argument("--steps", default="", help="comma-separated steps to run (default: all this build has)")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return child(args)
    tree_has_mode = "rslf_f2c_run_host_pk" in open(os.path.join(args.tree, "remotesensingproject_amd", "_lib.py")).read()
    steps = [s for s in args.steps.split(",") if s] or (["off"] + (["peaks", "ratio", "dense"] if tree_has_mode else []))
    got = {}
    for step in steps:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", step, "--config", args.config,
               "--reps", str(args.reps), "--ratio", str(args.ratio), "--tree", args.tree]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:   # a failure, a fault or the time limit: nothing more is started on the device
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("step %s ended with status %d: the probe stops here" % (step, r.returncode))
        got[step] = json.loads(r.stdout.strip().splitlines()[-1])
    summary = dict(config=args.config, tree=os.path.abspath(args.tree), **{k + "_ms": v["ms"] for k, v in got.items()})
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
