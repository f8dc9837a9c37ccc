"""The three records of profiles/r11_f2c_keep.md, through the C-ABI on one GPU, at the shapes of
`bench.py --path f2c --config skysat_lr / mansion_lr`:

  1. run time   rslf_f2c_run_host (+ rslf_f2c_run_destroy) against rslf_fine_to_coarse_run_host, alternating in one
                process; with --parent LIB the plain entry is ALSO taken from another build of the library (the parent
                commit's, loaded beside this one), and the plain entry against itself gives the spread of the lease.
  2. getter     get_coloured_depth_maps with par_cut_shadows as the C++ class without keep_on_device does it (volume +
                upload of the field + rslf_render_planes_host of the fused planes) against
                rslf_f2c_run_render_depth_maps_host; the bytes that cross the link in each.
  3. memory     rslf_f2c_run_describe's device_bytes (plan::f2c_kept_bytes) beside the change of free device memory.

    python tools/f2c_keep_measure.py [--configs skysat_lr,mansion_lr] [--reps 5] [--parent ab/librslf_parent.so] [--rows N]

Prints one JSON line per config.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="skysat_lr,mansion_lr")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default="")
    ap.add_argument("--rows", type=int, default=0, help="override the number of scanlines (developer runs)")
    args = ap.parse_args()

    import torch
    from remotesensingproject_amd import _lib, depth as rs
    from remotesensingproject_amd.synth import CONFIGS, make_lightfield
    L = _lib.lib()
    torch.cuda.set_device(0)
    ctx = rs.default_context(0)
    parent = parent_ctx = None
    if args.parent:
        parent = C.CDLL(os.path.abspath(args.parent))
        parent.rslf_ctx_create.argtypes = L.rslf_ctx_create.argtypes
        parent.rslf_fine_to_coarse_run_host.argtypes = L.rslf_fine_to_coarse_run_host.argtypes
        parent_ctx = C.c_void_p()
        assert parent.rslf_ctx_create(0, C.byref(parent_ctx)) == 0

    for name in args.configs.split(","):
        cfg = dict(CONFIGS[name])
        if args.rows:
            cfg["V"] = args.rows
        U, V, S, C_, D = cfg["U"], cfg["V"], cfg["S"], cfg["C"], cfg["D"]
        host, _ = make_lightfield(U, V, S, C_, seed=cfg["seed"], dmin=cfg["dmin"], dmax=cfg["dmax"])
        raw = (host * 200.0 + 3.0).astype(np.float32)
        del host
        epis = list(raw[..., 0]) if C_ == 1 else list(raw)
        keep_alive, ptrs, dt, V, S, U, C_, stride = rs.host_epis(epis, stride=True)
        p = rs.Depth1DParameters().to_c()
        n = S * V * U
        out_map, out_valid = np.empty((S, V, U), np.float32), np.empty((S, V, U), np.uint8)
        st, nl = _lib.RslfStats(), C.c_int()

        def plain(lib=L, h=ctx._h):
            t0 = time.perf_counter()
            rc = lib.rslf_fine_to_coarse_run_host(h, ptrs, 0, V, S, U, C_, stride, cfg["dmin"], cfg["dmax"], D, -1.0, C.byref(p), -1, 1,
                                                  out_map.ctypes.data_as(C.c_void_p), out_valid.ctypes.data_as(C.c_void_p), C.byref(nl), C.byref(st))
            assert rc == 0, rc
            return (time.perf_counter() - t0) * 1e3

        def kept(volumes=True, destroy=True):
            run = C.c_void_p()
            t0 = time.perf_counter()
            rc = L.rslf_f2c_run_host(ctx._h, ptrs, 0, V, S, U, C_, stride, cfg["dmin"], cfg["dmax"], D, -1.0, C.byref(p), -1, 1, 0, 0,
                                     1 if volumes else 0, C.byref(run), C.byref(st))
            assert rc == 0, rc
            if destroy:
                L.rslf_f2c_run_destroy(run)
            return (time.perf_counter() - t0) * 1e3, run

        ctx.use_current_stream()
        plain(); kept()                                           # warm-up: scratch grown, code objects loaded
        if parent:
            plain(parent, parent_ctx)
        t = dict(plain_a=[], plain_b=[], kept=[], kept_no_volumes=[], parent=[])
        for _ in range(args.reps):                                # alternating in one command
            t["plain_a"].append(plain())
            t["kept"].append(kept()[0])
            t["plain_b"].append(plain())
            t["kept_no_volumes"].append(kept(volumes=False)[0])
            if parent:
                t["parent"].append(plain(parent, parent_ctx))
        med = {k: statistics.median(v) for k, v in t.items() if v}
        base = med["parent"] if parent else med["plain_a"]
        line = dict(config=name, shape=dict(U=U, V=V, S=S, C=C_, D=D), reps=args.reps, run_ms=t, run_ms_median=med,
                    kept_over_plain=med["kept"] / base, plain_spread=abs(med["plain_b"] - med["plain_a"]) / med["plain_a"],
                    baseline="parent build" if parent else "this build's rslf_fine_to_coarse_run_host")

        # 3. memory, and the run the getter renders from
        torch.cuda.synchronize()
        mem = {}
        for volumes in (False, True):
            free0 = torch.cuda.mem_get_info(0)[0]
            _, run = kept(volumes=volumes, destroy=False)
            free1 = torch.cuda.mem_get_info(0)[0]
            d = _lib.RslfF2cRunDesc()
            assert L.rslf_f2c_run_describe(run, C.byref(d)) == 0
            mem["with_volumes" if volumes else "without_volumes"] = dict(sized_bytes=int(d.device_bytes), free_memory_delta=int(free0 - free1))
            if not volumes:
                L.rslf_f2c_run_destroy(run)
        line["memory"] = mem
        line["levels"] = [(d.V[l], d.U[l]) for l in range(d.n_levels)]

        # 2. the getter: the class without keep_on_device against the kept run
        lut = rs.colormap_jet()
        table = lut.ctypes.data_as(C.c_void_p)
        pic_a, pic_b = np.empty((S, V, U, 3), np.uint8), np.empty((S, V, U, 3), np.uint8)
        mid = C.c_int()
        assert L.rslf_render_centre_index(S, C.byref(mid)) == 0
        assert L.rslf_f2c_run_copy(run, 0, 5, out_map.ctypes.data_as(C.c_void_p), 1, None) == 0
        assert L.rslf_f2c_run_copy(run, 0, 6, out_valid.ctypes.data_as(C.c_void_p), 1, None) == 0

        def getter_plain():
            t0 = time.perf_counter()
            vol, su = C.c_void_p(), C.c_float()
            assert L.rslf_volume_create(ctx._h, V, S, U, C_, C.byref(vol)) == 0
            assert L.rslf_volume_upload_epis_f32(vol, ptrs, stride, -1.0, C.byref(su)) == 0
            rc = L.rslf_render_planes_host(ctx._h, out_map.ctypes.data_as(C.c_void_p), S, V * U, V, U, U, out_valid.ctypes.data_as(C.c_void_p),
                                           rs.FIT_QUANTILE, mid.value, 0, rs.RENDER_AFFINE, table, rs.MASK_BLACK, vol, rs.SLICE_VIEW, 0,
                                           float(p.shadow_level), pic_a.ctypes.data_as(C.c_void_p), None)
            assert rc == 0, rc
            L.rslf_volume_destroy(vol)
            return (time.perf_counter() - t0) * 1e3

        def getter_kept():
            t0 = time.perf_counter()
            assert L.rslf_f2c_run_render_depth_maps_host(run, ctx._h, 1, table, pic_b.ctypes.data_as(C.c_void_p)) == 0
            return (time.perf_counter() - t0) * 1e3

        getter_plain(); getter_kept()
        g = dict(plain=[], kept=[])
        for _ in range(args.reps):
            g["plain"].append(getter_plain())
            g["kept"].append(getter_kept())
        L.rslf_f2c_run_destroy(run)
        line["getter_ms"] = g
        line["getter_ms_median"] = {k: statistics.median(v) for k, v in g.items()}
        line["getter_pictures_equal"] = bool(np.array_equal(pic_a, pic_b))
        line["getter_link_bytes"] = dict(plain=dict(up=int(raw.nbytes + n * 5 + 768), down=int(n * 3)), kept=dict(up=768, down=int(n * 3)))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
