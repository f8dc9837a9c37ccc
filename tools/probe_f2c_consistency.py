"""A kept fine-to-coarse run (fine_to_coarse_run_host(keep=True)) with its validity by cross-view consistency off and on: what
the gate costs, what it does to the pyramid, and the gate launch beside a plain consistency launch on the same planes.

    python tools/probe_f2c_consistency.py [--config c2|c3|skysat_lr|mansion_lr] [--reps 5] [--rounds 3] [--min-agree 2]
                                          [--radius 0] [--tree DIR] [--limit SECONDS]

The synthetic fields of remotesensingproject_amd/synth.py, as bench.py --path f2c builds them.  Every step runs in a child
process of its own under `timeout` (--limit seconds each), one after the other, `off` and `gate` alternating for --rounds
rounds; the first one that fails ends the probe.  Wall-clock times of the whole call (host upload, every level, the fusion; the
call waits for the device), each the median of --reps runs after one warm-up.  --tree DIR imports the package from another
checkout (the parent commit's, built there): the steps that build lacks are left out, so fresh processes of the two builds can
alternate on one box.

  off      keep=True, the gate off; every level's share of valid pixels
  gate     consistency_min_agree=--min-agree, tol one grid step, --radius; every level's share of valid pixels, the dropped counts
  launch   on the planes of an ungated run, per level: the gate launch (rslf_f2c_consistency_mask: validity, agree, seen and the
           counter) beside rslf_view_consistency writing one plane (valid_out), device time by events, median of --reps * 4
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
    has_mode = "rslf_f2c_run_host_cs" in _lib.SYMBOLS
    if args.step != "off" and not has_mode:
        raise SystemExit("this build has no consistency gate in the pyramid")
    opts = dict(consistency_min_agree=args.min_agree, consistency_radius=args.radius) if args.step == "gate" else {}
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
    if args.step == "gate":
        out["gate"] = run.consistency_gate
        out["dropped"] = [run.inconsistent(l) for l in range(run.n_levels)]
    if args.step == "launch":
        tol = rs.grid_step(cfg["dmin"], cfg["dmax"], D, "probe")
        per_level = []
        for l in range(run.n_levels):
            depth, v = run.plane(l, "depth"), valid[l]
            slope = float(np.float32((0.0 + run.dims[l][1]) / run.dims[0][1]))
            counter = torch.zeros((1,), dtype=torch.int64, device="cuda")

            def timed(fn) -> float:
                fn()   # warm-up
                ms = []
                for _ in range(args.reps * 4):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                return round(statistics.median(ms), 4)

            gate_ms = timed(lambda: rs.f2c_consistency_mask(ctx, depth, v, slope, tol, args.radius, args.min_agree, dropped=counter))
            gate_alone_ms = timed(lambda: rs.f2c_consistency_mask(ctx, depth, v, slope, tol, args.radius, args.min_agree, counts=False))
            k12_ms = timed(lambda: rs.view_consistency(ctx, depth, v, slope, tol, args.radius, args.min_agree, counts=False, fused=False))
            per_level.append(dict(level=l, cells=int(depth.numel()), gate_ms=gate_ms, gate_valid_only_ms=gate_alone_ms, k12_valid_only_ms=k12_ms))
        out["launch"] = per_level
    print(json.dumps(out), flush=True)


def main() -> None:
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=["c2", "c3", "skysat_lr", "mansion_lr"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="how often `off` and `gate` alternate")
    ap.add_argument("--min-agree", type=int, default=2)
    ap.add_argument("--radius", type=int, default=0)
    ap.add_argument("--tree", default=here)
    ap.add_argument("--limit", type=int, default=240, help="seconds every step may take (its own timeout)")
    ap.add_argument("--steps", default="", help="comma-separated steps to run (default: all this build has, alternating)")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return child(args)
    tree_has_mode = "rslf_f2c_run_host_cs" in open(os.path.join(args.tree, "remotesensingproject_amd", "_lib.py")).read()
    steps = [s for s in args.steps.split(",") if s] or (["off", "gate"] * args.rounds + ["launch"] if tree_has_mode else ["off"] * args.rounds)
    got: dict[str, list] = {}
    for step in steps:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", step, "--config", args.config,
               "--reps", str(args.reps), "--min-agree", str(args.min_agree), "--radius", str(args.radius), "--tree", args.tree]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:   # a failure, a fault or the time limit: nothing more is started on the device
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("step %s ended with status %d: the probe stops here" % (step, r.returncode))
        got.setdefault(step, []).append(json.loads(r.stdout.strip().splitlines()[-1]))
    summary = dict(config=args.config, tree=os.path.abspath(args.tree), **{k + "_ms": [v["ms"] for v in vs] for k, vs in got.items()})
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
