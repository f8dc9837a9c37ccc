"""The 2-D sweep in the peaks mode without the propagation ratio, with r = 1 (the gate's code runs, nothing is withheld) and with
working ratios, alternating, visit by visit: what the sweep gate costs and what it makes the later visits scan.

    python tools/probe_sweep_gate.py [--config c2|c3|skysat_lr|mansion_lr] [--ratios 0.9,0.7] [--reps 5] [--rounds 3]
                                     [--tree DIR] [--f2c] [--limit SECONDS] [--hook peaks_list=0]

The synthetic fields of remotesensingproject_amd/synth.py, as bench.py --path sweep2d builds them.  Every step runs in a child
process of its own under `timeout` (--limit seconds each), one after the other; the first one that fails ends the probe.
HIP-event times on the current stream, each the median of --reps runs after one warm-up.  A ROUND is every step once, in the
order below; --rounds rounds follow one another, so the steps alternate on one box, and the summary holds every step's median
over the rounds next to its spread (min .. max): a difference between two steps inside the spreads is no difference.

  pk@DIR  with --tree DIR: the peaks-mode sweep of another checkout (the parent commit's, built there) -- it has no ratio
  pk      the peaks-mode sweep of this build, no ratio (k34_median_claim)
  r1      ... with propagation_ratio = 1 (k34_median_claim_gated: the four loads, the ballot; nothing withheld; same digest)
  r<x>    ... with a working ratio: the scanned pixels, the withheld sources, the time per scanned pixel-hypothesis unit
  visits  (once, after the rounds) per form one sweep through the visit API: per visit the pixels its scan takes, the sources
          the ratio withholds (counted on the host from the planes the visit's claims read; default parameters: the edge mask
          is the gate) and the visit's time
  --f2c   instead of the sweep: fine_to_coarse_run_host(keep=True, peaks=True) without and with the ratios; per level the
          withheld sources
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys


def child(args) -> None:
    sys.path.insert(0, os.path.abspath(args.tree))
    import ctypes as C

    import numpy as np
    import torch
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd import depth as rs
    from remotesensingproject_amd.sharding import sweep_order
    from remotesensingproject_amd.synth import CONFIGS, make_lightfield

    cfg = dict(CONFIGS[args.config])
    U, V, S, C_, D = cfg["U"], cfg["V"], cfg["S"], cfg["C"], cfg["D"]
    dmin, dmax = cfg["dmin"], cfg["dmax"]
    torch.cuda.set_device(0)
    ctx = rs.default_context(0)
    for h in filter(None, args.hook.split(",")):
        k, v = h.split("=")
        ctx.set_debug(**{k: int(v)})
    host, _ = make_lightfield(U, V, S, C_, seed=cfg["seed"], dmin=dmin, dmax=dmax)
    has_gate = "rslf_sweep_propagation_ratio" in _lib.SYMBOLS
    ratio = float(args.ratio)
    if ratio and not has_gate:
        raise SystemExit("this build has no sweep gate")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(f) -> float:
        ev[0].record()
        f()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1])

    def median_ms(f) -> float:
        f()   # warm-up
        torch.cuda.synchronize()
        return statistics.median(timed(f) for _ in range(args.reps))

    def digest(planes) -> str:
        h = hashlib.sha256()
        for t in planes:
            h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
        return h.hexdigest()[:16]

    out = dict(step=args.step, ratio=ratio, config=args.config, tree=os.path.abspath(args.tree), hook=args.hook, U=U, V=V, S=S, C=C_, D=D)
    gate = dict(propagation_ratio=ratio) if ratio else {}
    if args.step == "f2c":
        epis = list(host[..., 0]) if C_ == 1 else list(host)
        run = lambda: rs.fine_to_coarse_run_host(epis, dmin, dmax, D, 1.0, keep=True, peaks=True, keep_volumes=False, **gate)
        kept = run()
        out.update(levels=kept.n_levels, scanned_pixels=int(kept.stats.pixels_scanned),
                   withheld=[kept.withheld(l) for l in range(kept.n_levels)] if has_gate else None,
                   digest=digest(kept.get_results()))
        kept.close()
        out["ms"] = round(median_ms(lambda: run().close()), 4)
    elif args.step == "visits":
        vol = rs.Volume.from_dense(torch.from_numpy(host).cuda(), 1.0, ctx)
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
        L, p = _lib.lib(), rs.Depth1DParameters().to_c()
        ptr = lambda t: C.c_void_p(t.data_ptr())
        order = sweep_order(S)
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(order) + 1)]
        per_visit, counts, withheld = [], [], []
        for rep in range(args.reps + 1):
            Ce, Cd, depth, rbar, sm = z(S, V, U), z(S, V, U), z(S, V, U), z(S, V, U, C_), z(S, V, U, dt=torch.uint8)
            pk = rs.Peaks(torch.full((S, V, U), -1, dtype=torch.int32, device="cuda"), z(S, V, U), None,
                          torch.full((S, V, U), -1, dtype=torch.int32, device="cuda"), z(S, V, U))
            c_pk = _lib.RslfPeaks(*(None if t is None else t.data_ptr() for t in pk))
            cm = rs.compute_2D_edge_confidence(vol, Ce)
            ctx.use_current_stream()
            _lib.check(L.rslf_sweep_begin(ctx._h, vol._h, ptr(cm), ptr(sm), D, 0, V), "rslf_sweep_begin")
            _lib.check(L.rslf_sweep_peaks(ctx._h, vol._h, C.byref(c_pk)), "rslf_sweep_peaks")
            if ratio:
                _lib.check(L.rslf_sweep_propagation_ratio(ctx._h, vol._h, ratio), "rslf_sweep_propagation_ratio")
            evs[0].record()
            for i, s_hat in enumerate(order):
                if rep == 0:   # (host reads: the warm-up sweep alone counts)
                    counts.append(int(((cm[s_hat] != 0) & (sm[s_hat] != 0)).sum().item()))
                _lib.check(L.rslf_sweep_visit_scan(ctx._h, vol._h, None, None, dmin, dmax, D, s_hat, ptr(Ce), ptr(cm), ptr(Cd),
                                                   ptr(depth), ptr(rbar), C.byref(p)), "rslf_sweep_visit_scan")
                if rep == 0 and ratio:   # what the claims of this visit will read
                    amb = (pk.idx[s_hat] >= 0) & (pk.runner_idx[s_hat] >= 0) & (pk.runner_score[s_hat] > torch.tensor(ratio, dtype=torch.float32) * pk.score[s_hat])
                    withheld.append(int(((cm[s_hat] != 0) & amb).sum().item()))
                _lib.check(L.rslf_sweep_visit_finish(ctx._h, vol._h, s_hat, ptr(cm), ptr(Cd), ptr(depth), ptr(rbar), C.byref(p)),
                           "rslf_sweep_visit_finish")
                evs[i + 1].record()
            _lib.check(L.rslf_sweep_end(ctx._h, 1, D, None), "rslf_sweep_end")
            torch.cuda.synchronize()
            if rep == 0 and ratio:
                out["withheld_counter"] = ctx.get_withheld_sources()
            if rep > 0:
                per_visit.append([evs[i].elapsed_time(evs[i + 1]) for i in range(len(order))])
        med = [statistics.median(r[i] for r in per_visit) for i in range(len(order))]
        out.update(scanned_per_visit=counts, withheld_per_visit=withheld, visit_ms=[round(m, 4) for m in med])
    else:
        vol = rs.Volume.from_dense(torch.from_numpy(host).cuda(), 1.0, ctx)
        comp = rs.Depth2DComputer(vol, dmin, dmax, D, peaks=True, **gate)
        comp.run(want_stats=True)
        units = int(comp.stats.units)
        pk = comp.get_peaks_s_v_u()
        planes = [comp.m_best_depth_s_v_u, comp.m_disp_confidence_s_v_u, comp.m_edge_confidence_s_v_u, comp.m_edge_confidence_mask_s_v_u,
                  comp.m_rbar_s_v_u, comp.m_scan_mask_s_v_u, pk.idx, pk.score, pk.runner_idx, pk.runner_score]
        out.update(units=units, scanned_pixels=units // D, digest=digest(planes),
                   withheld=comp.get_withheld_sources() if has_gate else None)
        ms = median_ms(lambda: comp.run(want_stats=False))
        out.update(ms=round(ms, 4), ns_per_unit=round(ms * 1e6 / units, 4))
    print(json.dumps(out), flush=True)


def main() -> None:
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=["c2", "c3", "skysat_lr", "mansion_lr"])
    ap.add_argument("--ratios", default="0.9,0.7", help="working ratios, comma-separated")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tree", default="", help="another checkout, built: its peaks-mode sweep alternates with this build's")
    ap.add_argument("--f2c", action="store_true")
    ap.add_argument("--hook", default="", help="rslf_ctx_set_debug hooks for every step, e.g. peaks_list=0")
    ap.add_argument("--limit", type=int, default=240, help="seconds every step may take (its own timeout)")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    ap.add_argument("--ratio", default="0", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        args.tree = args.tree or here
        return child(args)
    ratios = [r for r in args.ratios.split(",") if r]
    kind = "f2c" if args.f2c else "sweep"
    steps = ([("pk@" + args.tree, args.tree, "0")] if args.tree else []) + [("pk", here, "0"), ("r1", here, "1")] + [("r" + r, here, r) for r in ratios]

    def run(name, tree, ratio, step):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", step, "--ratio", ratio,
               "--config", args.config, "--reps", str(args.reps), "--tree", tree, "--hook", args.hook]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:   # a failure, a fault or the time limit: nothing more is started on the device
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("step %s ended with status %d: the probe stops here" % (name, r.returncode))
        return json.loads(r.stdout.strip().splitlines()[-1])

    got = {name: [] for name, _, _ in steps}
    for _ in range(args.rounds):
        for name, tree, ratio in steps:
            got[name].append(run(name, tree, ratio, kind))
    summary = dict(config=args.config, kind=kind, hook=args.hook, rounds=args.rounds)
    for name, runs in got.items():
        ms = [r["ms"] for r in runs]
        summary[name] = dict(ms=round(statistics.median(ms), 4), spread=[min(ms), max(ms)], scanned_pixels=runs[0]["scanned_pixels"],
                             withheld=runs[0]["withheld"], digest=runs[0]["digest"])
        if "ns_per_unit" in runs[0]:
            summary[name]["ns_per_unit"] = round(statistics.median(r["ns_per_unit"] for r in runs), 4)
    summary["r1_is_pk"] = summary["r1"]["digest"] == summary["pk"]["digest"]
    if args.tree:
        summary["pk_is_the_other_trees"] = summary["pk"]["digest"] == summary["pk@" + args.tree]["digest"]
    print(json.dumps(summary), flush=True)
    if not args.f2c:
        for name, tree, ratio in steps[1 if args.tree else 0:]:
            if name != "r1":
                run(name, tree, ratio, "visits")
    if not summary["r1_is_pk"]:
        raise SystemExit("r = 1 and the sweep without a ratio gave different planes")


if __name__ == "__main__":
    main()
