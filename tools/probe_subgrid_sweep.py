"""The 2-D sweep and fine-to-coarse with the sub-grid mode off, on, and on with "subgrid_list" = 0 (every visit the dense form of
the refinement), and what the pile step pays per refined pixel: the cost bar of the mode.

    python tools/probe_subgrid_sweep.py [--config c2|c3|skysat_lr|mansion_lr] [--f2c] [--reps 5] [--tree DIR] [--limit SECONDS]

The synthetic fields of remotesensingproject_amd/synth.py, as bench.py --path sweep2d / f2c build them.  Every step runs in a
child process of its own under `timeout` (--limit seconds each), one after the other; the first one that fails ends the probe.
HIP-event times on the current stream, each the median of --reps runs after one warm-up.  --tree DIR imports the package from
another checkout (the parent commit's, built there): the steps that build lacks are left out, so fresh processes of the two
builds can alternate on one box.

  pile    Depth1DComputer_pile.run with subgrid 0 and 1 on the same volume, alternating; (pile1 - pile0) / confident pixels is
          the price per refined pixel of the dense kernel on a full plane: taken on the parent's build, it is THE BAR
  off     the sweep (Depth2DComputer.run) or the pyramid (FineToCoarse ctor + run + get_results), mode off
  on      ... mode on; reports stats.units / dim_d, the scanned pixels, and a digest of every result plane
  dense   ... mode on under "subgrid_list" = 0; its digest must equal `on`'s: the two forms give identical planes
  visits  (sweep only) one sweep per mode through the visit API, untimed: the pixels every visit scanned

The summary line holds added = on - off, the bar's verdict where a price is at hand (added < price x scanned pixels x 2) and
the measured ratio added / (price x scanned pixels).
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
    host, _ = make_lightfield(U, V, S, C_, seed=cfg["seed"], dmin=dmin, dmax=dmax)
    has_mode = "rslf_sweep_subgrid" in _lib.SYMBOLS
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

    out = dict(step=args.step, config=args.config, f2c=bool(args.f2c), tree=os.path.abspath(args.tree), has_mode=has_mode,
               U=U, V=V, S=S, C=C_, D=D)
    sub = dict(subgrid=True) if args.step in ("on", "dense") else {}
    if args.step in ("on", "dense", "visits") and not has_mode:
        raise SystemExit("this build has no sub-grid sweep")
    if args.step == "dense":
        ctx.set_debug(subgrid_list=0)

    if args.step == "pile":
        vol = rs.Volume.from_dense(torch.from_numpy(host).cuda(), 1.0, ctx)
        piles = {s: rs.Depth1DComputer_pile(vol, dmin, dmax, D, S // 2, 1.0, rs.Depth1DParameters(), subgrid=bool(s)) for s in (0, 1)}
        per = {0: [], 1: []}
        for _ in range(3):   # the two modes alternating
            for s, comp in piles.items():
                per[s].append(median_ms(lambda c=comp: c.run(want_stats=False)))
        piles[1].run(want_stats=True)
        pixels = int(piles[1].stats.pixels_scanned)
        p0, p1 = statistics.median(per[0]), statistics.median(per[1])
        out.update(pile0_ms=round(p0, 4), pile1_ms=round(p1, 4), confident_pixels=pixels, price_ns_per_pixel=round((p1 - p0) * 1e6 / pixels, 4))
    elif args.step == "visits":
        vol = rs.Volume.from_dense(torch.from_numpy(host).cuda(), 1.0, ctx)
        L, p = _lib.lib(), rs.Depth1DParameters().to_c()
        vp = C.c_void_p
        order = sweep_order(S)   # core.hpp:981-990: the centre view, then outwards, alternating
        for mode in (0, 1):
            z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
            Ce, Cd, depth, rbar, sm = z(S, V, U), z(S, V, U), z(S, V, U), z(S, V, U, C_), z(S, V, U, dt=torch.uint8)
            cm = rs.compute_2D_edge_confidence(vol, Ce)
            ctx.use_current_stream()
            ptr = lambda t: vp(t.data_ptr())
            _lib.check(L.rslf_sweep_begin(ctx._h, vol._h, ptr(cm), ptr(sm), D, 0, V), "rslf_sweep_begin")
            _lib.check(L.rslf_sweep_subgrid(ctx._h, vol._h, mode), "rslf_sweep_subgrid")
            counts = []
            for s_hat in order:
                counts.append(int(((cm[s_hat] != 0) & (sm[s_hat] != 0)).sum().item()))   # what this visit's scan takes
                _lib.check(L.rslf_sweep_visit_scan(ctx._h, vol._h, None, None, dmin, dmax, D, s_hat, ptr(Ce), ptr(cm), ptr(Cd), ptr(depth),
                                                   ptr(rbar), C.byref(p)), "rslf_sweep_visit_scan")
                _lib.check(L.rslf_sweep_visit_finish(ctx._h, vol._h, s_hat, ptr(cm), ptr(Cd), ptr(depth), ptr(rbar), C.byref(p)),
                           "rslf_sweep_visit_finish")
            st = _lib.RslfStats()
            _lib.check(L.rslf_sweep_end(ctx._h, 1, D, C.byref(st)), "rslf_sweep_end")
            assert sum(counts) == st.pixels_scanned, (sum(counts), st.pixels_scanned)
            out["scanned_per_visit_%s" % ("on" if mode else "off")] = counts
    elif args.f2c:
        raw = (host * 200.0 + 3.0).astype(np.float32)
        last = {}

        def once():
            f = rs.FineToCoarse(raw, dmin, dmax, D, **sub)
            f.run()
            last["f"], last["out"] = f, f.get_results()

        ms = median_ms(once)
        f = last["f"]
        out.update(ms=round(ms, 4), scanned_pixels=sum(int(c.stats.units) for c in f.m_computers) // D,
                   dims=[(c.m_epis.V, c.m_epis.U) for c in f.m_computers],
                   digest=digest(list(last["out"]) + [c.m_best_depth_s_v_u for c in f.m_computers]))
    else:
        vol = rs.Volume.from_dense(torch.from_numpy(host).cuda(), 1.0, ctx)
        comp = rs.Depth2DComputer(vol, dmin, dmax, D, **sub)
        comp.run(want_stats=True)
        units = int(comp.stats.units)
        ms = median_ms(lambda: comp.run(want_stats=False))
        out.update(ms=round(ms, 4), scanned_pixels=units // D,
                   digest=digest([comp.m_best_depth_s_v_u, comp.m_disp_confidence_s_v_u, comp.m_edge_confidence_s_v_u,
                                  comp.m_edge_confidence_mask_s_v_u, comp.m_rbar_s_v_u, comp.m_scan_mask_s_v_u]))
    print(json.dumps(out), flush=True)


def main() -> None:
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=["c2", "c3", "skysat_lr", "mansion_lr"])
    ap.add_argument("--f2c", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tree", default=here)
    ap.add_argument("--limit", type=int, default=240, help="seconds every step may take (its own timeout)")
    ap.add_argument("--steps", default="", help="comma-separated steps to run (default: all this build has)")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return child(args)
    tree_has_mode = "rslf_sweep_subgrid" in open(os.path.join(args.tree, "remotesensingproject_amd", "_lib.py")).read()
    steps = [s for s in args.steps.split(",") if s] or (["pile", "off"] + (["on", "dense"] + ([] if args.f2c else ["visits"]) if tree_has_mode else []))
    got = {}
    for step in steps:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", step, "--config", args.config,
               "--reps", str(args.reps), "--tree", args.tree] + (["--f2c"] if args.f2c else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:   # a failure, a fault or the time limit: nothing more is started on the device
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("step %s ended with status %d: the probe stops here" % (step, r.returncode))
        got[step] = json.loads(r.stdout.strip().splitlines()[-1])
    summary = dict(config=args.config, f2c=bool(args.f2c), tree=os.path.abspath(args.tree))
    if "off" in got:
        summary["off_ms"] = got["off"]["ms"]
    if "on" in got and "off" in got:
        added = got["on"]["ms"] - got["off"]["ms"]
        summary.update(on_ms=got["on"]["ms"], added_ms=round(added, 4), scanned_pixels=got["on"]["scanned_pixels"])
        if "pile" in got:
            allowance = got["pile"]["price_ns_per_pixel"] * got["on"]["scanned_pixels"] * 1e-6
            summary.update(price_ns_per_pixel=got["pile"]["price_ns_per_pixel"], price_x_pixels_ms=round(allowance, 4),
                           ratio=round(added / allowance, 4) if allowance > 0 else None, within_twice=bool(added < 2 * allowance))
    if "dense" in got and "on" in got:
        summary.update(dense_ms=got["dense"]["ms"], forms_identical=got["dense"]["digest"] == got["on"]["digest"])
        if not summary["forms_identical"]:
            print(json.dumps(summary), flush=True)
            raise SystemExit("the list form and the dense form gave different planes")
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
