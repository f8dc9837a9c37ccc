"""The 2-D sweep with the peaks mode off, on, and on with "peaks_list" = 0 (every visit the dense form), visit by visit, and what
the peaks cost through the score rows: the cost bar of the mode.

    python tools/probe_sweep_peaks.py [--config c2|c3|skysat_lr|mansion_lr] [--reps 5] [--tree DIR] [--limit SECONDS] [--steps a,b]

The synthetic fields of remotesensingproject_amd/synth.py, as bench.py --path sweep2d builds them.  Every step runs in a child
process of its own under `timeout` (--limit seconds each), one after the other; the first one that fails ends the probe.
HIP-event times on the current stream, each the median of --reps runs after one warm-up.  --tree DIR imports the package from
another checkout (the parent commit's, built there): the steps that build lacks are left out, so fresh processes of the two
builds can alternate on one box.

  price   whole-frame rslf_depth_epi_peaks (score rows through the staging buffer, then their peaks) and the scan
          (rslf_depth_epi_scan) on the centre view's edge mask, alternating; (peaks - scan) / pixels is what the peaks cost
          per pixel through the rows -- any build has both entries; taken on the parent's build it is THE BAR
  off     the sweep (Depth2DComputer.run), mode off
  on      ... mode on; reports stats.units / dim_d, the scanned pixels, and a digest of every result plane and the four peak planes
  dense   ... mode on under "peaks_list" = 0; its digest must equal `on`'s: the two forms give identical planes
  visits  one sweep per form through the visit API: the pixels every visit's scan takes, and every visit's time (scan, step and
          finish; HIP events around each visit, the median of --reps sweeps) -- the split between the first visit and the rest

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
    has_mode = "rslf_sweep_peaks" in _lib.SYMBOLS
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

    out = dict(step=args.step, config=args.config, tree=os.path.abspath(args.tree), has_mode=has_mode, U=U, V=V, S=S, C=C_, D=D)
    if args.step in ("on", "dense", "visits") and not has_mode:
        raise SystemExit("this build has no peaks mode in the sweep")
    vol = rs.Volume.from_dense(torch.from_numpy(host).cuda(), 1.0, ctx)
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")

    if args.step == "price":
        s_hat = S // 2
        par = rs.Depth1DParameters()
        Ce3 = z(S, V, U)
        cm = rs.compute_2D_edge_confidence(vol, Ce3)[s_hat].contiguous()
        Ce = Ce3[s_hat].contiguous()
        pixels = int((cm != 0).sum().item())
        Cd, depth, rbar = z(V, U), z(V, U), z(V, U, C_)
        peaks = rs.compute_1D_depth_peaks(vol, dmin, dmax, D, s_hat, par, cm)

        def scan():
            rs.compute_1D_depth_epi(vol, dmin, dmax, D, s_hat, Ce.clone(), cm.clone(), Cd, depth, rbar, par, cm)

        def rows_and_peaks():
            rs.compute_1D_depth_peaks(vol, dmin, dmax, D, s_hat, par, cm, out=peaks)

        per = {0: [], 1: []}
        for _ in range(3):   # the two alternating
            per[0].append(median_ms(scan))
            per[1].append(median_ms(rows_and_peaks))
        t0, t1 = statistics.median(per[0]), statistics.median(per[1])
        out.update(scan_ms=round(t0, 4), peaks_ms=round(t1, 4), pixels=pixels, price_ns_per_pixel=round((t1 - t0) * 1e6 / pixels, 4))
    elif args.step == "visits":
        L, p = _lib.lib(), rs.Depth1DParameters().to_c()
        vp = C.c_void_p
        ptr = lambda t: vp(t.data_ptr())
        order = sweep_order(S)   # core.hpp:981-990: the centre view, then outwards, alternating
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(order) + 1)]
        for form in ("off", "on", "dense"):
            ctx.set_debug(peaks_list=0 if form == "dense" else 1)
            per_visit, counts = [], []
            for rep in range(args.reps + 1):
                Ce, Cd, depth, rbar, sm = z(S, V, U), z(S, V, U), z(S, V, U), z(S, V, U, C_), z(S, V, U, dt=torch.uint8)
                pk = rs.Peaks(torch.full((S, V, U), -1, dtype=torch.int32, device="cuda"), z(S, V, U), None,
                              torch.full((S, V, U), -1, dtype=torch.int32, device="cuda"), z(S, V, U))
                c_pk = _lib.RslfPeaks(*(None if t is None else t.data_ptr() for t in pk))
                cm = rs.compute_2D_edge_confidence(vol, Ce)
                ctx.use_current_stream()
                _lib.check(L.rslf_sweep_begin(ctx._h, vol._h, ptr(cm), ptr(sm), D, 0, V), "rslf_sweep_begin")
                if form != "off":
                    _lib.check(L.rslf_sweep_peaks(ctx._h, vol._h, C.byref(c_pk)), "rslf_sweep_peaks")
                counts = []
                evs[0].record()
                for i, s_hat in enumerate(order):
                    if rep == 0:   # (a host read: the warm-up sweep alone counts)
                        counts.append(int(((cm[s_hat] != 0) & (sm[s_hat] != 0)).sum().item()))
                    _lib.check(L.rslf_sweep_visit_scan(ctx._h, vol._h, None, None, dmin, dmax, D, s_hat, ptr(Ce), ptr(cm), ptr(Cd),
                                                       ptr(depth), ptr(rbar), C.byref(p)), "rslf_sweep_visit_scan")
                    _lib.check(L.rslf_sweep_visit_finish(ctx._h, vol._h, s_hat, ptr(cm), ptr(Cd), ptr(depth), ptr(rbar), C.byref(p)),
                               "rslf_sweep_visit_finish")
                    evs[i + 1].record()
                _lib.check(L.rslf_sweep_end(ctx._h, 1, D, None), "rslf_sweep_end")
                torch.cuda.synchronize()
                if rep == 0:
                    out["scanned_per_visit"] = counts
                else:
                    per_visit.append([evs[i].elapsed_time(evs[i + 1]) for i in range(len(order))])
            med = [statistics.median(r[i] for r in per_visit) for i in range(len(order))]
            out["visit_ms_%s" % form] = [round(m, 4) for m in med]
            out["first_ms_%s" % form] = round(med[0], 4)
            out["rest_ms_%s" % form] = round(sum(med[1:]), 4)
    else:
        kw = dict(peaks=True) if args.step in ("on", "dense") else {}
        if args.step == "dense":
            ctx.set_debug(peaks_list=0)
        comp = rs.Depth2DComputer(vol, dmin, dmax, D, **kw)
        comp.run(want_stats=True)
        units = int(comp.stats.units)
        ms = median_ms(lambda: comp.run(want_stats=False))
        planes = [comp.m_best_depth_s_v_u, comp.m_disp_confidence_s_v_u, comp.m_edge_confidence_s_v_u,
                  comp.m_edge_confidence_mask_s_v_u, comp.m_rbar_s_v_u, comp.m_scan_mask_s_v_u]
        out.update(ms=round(ms, 4), scanned_pixels=units // D, digest=digest(planes))
        if kw:
            pk = comp.get_peaks_s_v_u()
            out.update(peaks_digest=digest([pk.idx, pk.score, pk.runner_idx, pk.runner_score]),
                       with_runner_up=int((pk.runner_idx >= 0).sum().item()), with_winner=int((pk.idx >= 0).sum().item()))
    print(json.dumps(out), flush=True)


def main() -> None:
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=["c2", "c3", "skysat_lr", "mansion_lr"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tree", default=here)
    ap.add_argument("--limit", type=int, default=240, help="seconds every step may take (its own timeout)")
    ap.add_argument("--steps", default="", help="comma-separated steps to run (default: all this build has)")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return child(args)
    tree_has_mode = "rslf_sweep_peaks" in open(os.path.join(args.tree, "remotesensingproject_amd", "_lib.py")).read()
    steps = [s for s in args.steps.split(",") if s] or (["price", "off"] + (["on", "dense", "visits"] if tree_has_mode else []))
    got = {}
    for step in steps:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", step, "--config", args.config,
               "--reps", str(args.reps), "--tree", args.tree]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:   # a failure, a fault or the time limit: nothing more is started on the device
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("step %s ended with status %d: the probe stops here" % (step, r.returncode))
        got[step] = json.loads(r.stdout.strip().splitlines()[-1])
    summary = dict(config=args.config, tree=os.path.abspath(args.tree))
    if "off" in got:
        summary["off_ms"] = got["off"]["ms"]
    if "on" in got and "off" in got:
        added = got["on"]["ms"] - got["off"]["ms"]
        summary.update(on_ms=got["on"]["ms"], added_ms=round(added, 4), scanned_pixels=got["on"]["scanned_pixels"])
        if "price" in got:
            allowance = got["price"]["price_ns_per_pixel"] * got["on"]["scanned_pixels"] * 1e-6
            summary.update(price_ns_per_pixel=got["price"]["price_ns_per_pixel"], price_x_pixels_ms=round(allowance, 4),
                           ratio=round(added / allowance, 4) if allowance > 0 else None, within_twice=bool(added < 2 * allowance))
    if "dense" in got and "on" in got:
        same = got["dense"]["digest"] == got["on"]["digest"] and got["dense"]["peaks_digest"] == got["on"]["peaks_digest"]
        summary.update(dense_ms=got["dense"]["ms"], forms_identical=same)
        if not same:
            print(json.dumps(summary), flush=True)
            raise SystemExit("the list form and the dense form gave different planes")
    if "off" in got and "on" in got:
        summary["other_planes_identical"] = got["off"]["digest"] == got["on"]["digest"]
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
