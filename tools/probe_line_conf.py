"""The 2-D sweep with and without the line confidence (K7), on the synthetic c2 / c3 fields of bench.py --path sweep2d.

    python tools/probe_line_conf.py --config c3 [--modes 0,1,2] [--reps 5] [--threshold T] [--k7-stats stats.csv]

One process, one volume, one Depth2DComputer per mode; the modes ALTERNATE (mode 0, 1, 2, 0, 1, 2, ...) so that clock and
box drift hit them alike, and each mode reports the median of --reps timed runs after one warm-up.  Mode 2 takes
par_line_score_threshold = the median of mode 1's C_l over the masked pixels and reports the share of the centre view's masked
pixels that pass the gate; --threshold gives it instead, so that a traced mode-2 run holds mode-2 sweeps only.

K7's algorithmic bytes per sweep (printed for the modes that run it): per masked pixel of a visit 4 S for its column and 4 for
the result, per scanned pixel 4 S for the column written, per scanline and visit the S rows of C_e once.  (A scanned pixel
reads its fresh column back instead of keeping it in registers: 4 S more per scanned pixel, reported beside the count.)  The tool also times
a plain device-to-device copy moving the bytes of ONE visit (torch's copy_ of a buffer of half that size: it reads and writes
it).  K7's own time comes from a kernel trace of this tool:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/probe_line_conf.py --config c3 --modes 1 --reps 1 --no-copy

and --k7-stats OUT/.../*_kernel_stats.csv turns the trace's k7_line_confidence row into time per visit and bytes per second.
Prints one JSON line per mode and one for the copy.

    python tools/probe_line_conf.py --f2c [--config skysat_lr] [--modes 0,1,2] [--reps 3] [--threshold T] [--k7-stats stats.csv]

is the same for fine-to-coarse: bench.py --path f2c's step (FineToCoarse constructor + run + get_results on the raw field, host
upload included) with line_confidence_mode = the mode, the modes alternating.  Mode 2 takes the median of mode 1's C_l over
the masked pixels of the finest level unless --threshold is given, and every mode reports each level's share of valid pixels.
--k7-stats here gives K7's share of the kernel time of the traced run (the trace's Percentage column).
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def k7_row(path: str):
    """(calls, total ns) of the k7_line_confidence rows of a rocprofv3 kernel_stats.csv."""
    calls, total = 0, 0.0
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "k7_line_confidence" in row.get("Name", ""):
                calls += int(row["Calls"])
                total += float(row["TotalDurationNs"])
    return calls, total


def kernel_share(path: str, needle: str):
    """(calls, total ns, share of all kernel time) of the rows of a rocprofv3 kernel_stats.csv whose name holds `needle`."""
    calls, total, everything = 0, 0.0, 0.0
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            everything += float(row["TotalDurationNs"])
            if needle in row.get("Name", ""):
                calls += int(row["Calls"])
                total += float(row["TotalDurationNs"])
    return calls, total, (total / everything if everything else 0.0)


def f2c(args) -> None:
    import numpy as np
    import torch
    from remotesensingproject_amd import depth as rs
    from remotesensingproject_amd.synth import CONFIGS, make_lightfield

    cfg = dict(CONFIGS[args.config])
    U, V, S, C, D = cfg["U"], cfg["V"], cfg["S"], cfg["C"], cfg["D"]
    modes = [int(m) for m in args.modes.split(",")]
    torch.cuda.set_device(0)
    host, _ = make_lightfield(U, V, S, C, seed=cfg["seed"], dmin=cfg["dmin"], dmax=cfg["dmax"])
    raw = (host * 200.0 + 3.0).astype(np.float32)

    def once(mode: int, thr: float):
        f = rs.FineToCoarse(raw, cfg["dmin"], cfg["dmax"], D, parameters=rs.Depth1DParameters(par_line_score_threshold=thr),
                            line_confidence_mode=mode)
        f.run()
        f.get_results()
        torch.cuda.synchronize()
        return f

    thr = 0.02
    if args.threshold is not None:
        thr = args.threshold
    elif 2 in modes:
        c0 = once(1, thr).m_computers[0]
        m = c0.m_edge_confidence_mask_s_v_u != 0
        thr = float(c0.m_line_confidence_s_v_u[m].median()) if bool(m.any()) else 0.02
        del c0
    last = {mode: once(mode, thr) for mode in modes}   # warm-up: scratch sized, clocks up
    times = {mode: [] for mode in modes}
    for _ in range(args.reps):
        for mode in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[mode] = once(mode, thr)
            times[mode].append((time.perf_counter() - t0) * 1e3)
    for mode in modes:
        comps = last[mode].m_computers
        line = {"path": "f2c", "config": args.config, "mode": mode, "ms_median": statistics.median(times[mode]),
                "ms_runs": [round(t, 3) for t in times[mode]], "levels": [(c.m_epis.V, c.m_epis.U) for c in comps],
                "pixels_scanned": [int(c.stats.pixels_scanned) for c in comps],
                "valid_share": [round(float((c.get_valid_depths_mask_s_v_u() != 0).float().mean()), 4) for c in comps]}
        if mode:
            # K7 per visit: 4 S + 4 bytes per masked pixel, 4 S per scanned pixel, the S rows of C_e once per scanline
            masked = [int((c.m_edge_confidence_mask_s_v_u != 0).sum()) for c in comps]
            line.update(k7_masked_pixels=masked, line_score_threshold=thr,
                        k7_algorithmic_bytes=sum(m * (4 * S + 4) + int(c.stats.pixels_scanned) * 4 * S + S * (c.m_epis.V * S * c.m_epis.U * 4)
                                                 for m, c in zip(masked, comps)))
            if args.k7_stats:
                calls, ns, share = kernel_share(args.k7_stats, "k7_line_confidence")
                line.update(k7_calls=calls, k7_ms_total=ns / 1e6, k7_share_of_kernel_time=share)
        print(json.dumps(line), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--f2c", action="store_true", help="fine-to-coarse (bench.py --path f2c's step) instead of one 2-D sweep")
    ap.add_argument("--config", default=None, help="c2 / c3 (the sweep; default c2), or with --f2c any config of synth.CONFIGS (default skysat_lr)")
    ap.add_argument("--modes", default="0,1,2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-copy", action="store_true")
    ap.add_argument("--threshold", type=float, default=None, help="par_line_score_threshold of the mode-2 runs (default: measured)")
    ap.add_argument("--k7-stats", default="", help="rocprofv3 kernel_stats.csv of a run of this tool with ONE timed mode-1 or mode-2 run")
    args = ap.parse_args()
    if args.f2c:
        args.config = args.config or "skysat_lr"
        return f2c(args)
    args.config = args.config or "c2"
    if args.config not in ("c2", "c3"):
        ap.error("the sweep form takes --config c2 or c3")
    import numpy as np
    import torch
    from remotesensingproject_amd import depth as rs
    from remotesensingproject_amd.synth import CONFIGS, make_lightfield

    cfg = dict(CONFIGS[args.config])
    U, V, S, C, D = cfg["U"], cfg["V"], cfg["S"], cfg["C"], cfg["D"]
    modes = [int(m) for m in args.modes.split(",")]
    torch.cuda.set_device(0)
    host, _ = make_lightfield(U, V, S, C, seed=cfg["seed"], dmin=cfg["dmin"], dmax=cfg["dmax"])
    ctx = rs.default_context(0)
    vol = rs.Volume.from_dense(torch.from_numpy(host).cuda(), 1.0, ctx)

    def computer(mode: int, thr: float = 0.02):
        par = rs.Depth1DParameters(par_line_confidence_mode=mode, par_line_score_threshold=thr)
        return rs.Depth2DComputer(vol, cfg["dmin"], cfg["dmax"], D, parameters=par)

    thr = 0.02
    if args.threshold is not None:
        thr = args.threshold
    elif 2 in modes:   # the threshold of the mode-2 runs: the median of mode 1's C_l over the masked pixels
        c1 = computer(1)
        c1.run(want_stats=False)
        torch.cuda.synchronize()
        m = c1.m_edge_confidence_mask_s_v_u != 0
        thr = float(c1.m_line_confidence_s_v_u[m].median()) if bool(m.any()) else 0.02
        del c1
    comps = {mode: computer(mode, thr) for mode in modes}
    for mode in modes:   # warm-up: scratch sized, clocks up
        comps[mode].run(want_stats=True)
    torch.cuda.synchronize()
    scanned = {mode: int(comps[mode].stats.pixels_scanned) for mode in modes}   # the timed runs ask for no stats
    times = {mode: [] for mode in modes}
    for _ in range(args.reps):
        for mode in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            comps[mode].run(want_stats=False)
            torch.cuda.synchronize()
            times[mode].append((time.perf_counter() - t0) * 1e3)
    visit_bytes = 0
    for mode in modes:
        comp = comps[mode]
        line = {"config": args.config, "mode": mode, "ms_median": statistics.median(times[mode]),
                "ms_runs": [round(t, 3) for t in times[mode]], "pixels_scanned": scanned[mode]}
        if mode:
            masked = int((comp.m_edge_confidence_mask_s_v_u != 0).sum())   # over all views = over all visits
            total = masked * (4 * S + 4) + scanned[mode] * 4 * S + S * (V * S * U * 4)
            visit_bytes = total // S
            # not in the algorithmic count: a scanned pixel's column is stored and read back (L1 / L2) instead of kept in registers
            line.update(k7_masked_pixels=masked, k7_algorithmic_bytes=total, k7_bytes_per_visit=visit_bytes,
                        k7_column_reread_bytes=scanned[mode] * 4 * S)
            if args.k7_stats:
                calls, ns = k7_row(args.k7_stats)
                if calls:
                    line.update(k7_calls=calls, k7_ms_total=ns / 1e6, k7_us_per_visit=ns / 1e3 / calls,
                                k7_gb_per_s=(total * calls / S) / ns)
        if mode == 2:
            c = S // 2
            mc = comp.m_edge_confidence_mask_s_v_u[c] != 0
            share = float((comp.m_line_confidence_s_v_u[c][mc] > float(np.float32(thr))).float().mean()) if bool(mc.any()) else 0.0
            line.update(line_score_threshold=thr, centre_view_pass_share=share)
        print(json.dumps(line), flush=True)
    if visit_bytes and not args.no_copy:
        src = torch.empty(visit_bytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        dst.copy_(src)
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ms = statistics.median(ts)
        print(json.dumps({"config": args.config, "copy_bytes_moved": 2 * (visit_bytes // 2), "copy_ms_median": ms,
                          "copy_gb_per_s": 2 * (visit_bytes // 2) / ms / 1e6, "copy_ms_runs": [round(t, 4) for t in ts]}), flush=True)


if __name__ == "__main__":
    main()
