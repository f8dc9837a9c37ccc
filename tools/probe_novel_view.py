"""The novel view (rslf_novel_view, K15) at the sweep shapes: every view leave-one-out in one call, timed by HIP events and
alternating, round by round, with a K14 launch (rslf_view_warp) on the same planes -- and, unless --no-sweep, the 2-D sweep of
the same field with get_novel_view_prediction beside get_view_prediction on its planes, default and consistent mask.

    python tools/probe_novel_view.py [--config c2|c3] [--reps 3] [--rounds 3] [--no-sweep] [--tree DIR]

--tree DIR: import the package from another checkout (another build of the library) instead of this one.

The synthetic fields of remotesensingproject_amd/synth.py, as bench.py --path sweep2d builds them.  The planes timed are the
`truth` planes of tools/probe_view_warp.py: the scene's own disparity per scanline with 5 % of the pixels replaced by uniform
values of the hypothesis range and 10 % invalid.  Variants, each once per ROUND, each figure the median of --reps launches after
a warm-up, the summary the median over the rounds and the spread:

  novel/r<R>/s<N>/g<G>   fill, n_src, err, row_err, row_cov (what get_novel_view_prediction asks for), T = S targets, every
                         view excluded from itself; radius R in {0, 8}, sources N in {1, 2, 4}, max_gap G in {0, 3}; tol one
                         step of the hypothesis grid
  novel/image            colour, depth, fill, n_src at radius 8, sources 4, max_gap 0: the finished images
  warp/r<R>              rslf_view_warp: hit, err, row_err, row_hits

Per variant also what the call found (coverage, mean n_src, filled share, mean abs error) and plan::novel_bytes' algorithmic
bytes with the measured mean number of views a pixel blends.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=["c2", "c3"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sweep-reps", type=int, default=2)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))

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
    cells = T * V * U
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device="cuda")
    w = dict(hit=new((T, V, U), torch.uint8), err=new((T, V, U), torch.float32), row_err=new((T, V), torch.float64),
             row_hits=new((T, V), torch.int32))
    nv = dict(colour=new((T, V, U, C_), torch.float32), depth=new((T, V, U), torch.float32), fill=new((T, V, U), torch.uint8),
              n_src=new((T, V, U), torch.int32), err=w["err"], row_err=w["row_err"], row_cov=new((T, V), torch.int32))
    warp_out = _lib.RslfViewWarpOut(**{k: t.data_ptr() for k, t in w.items()})
    loo_out = _lib.RslfNovelViewOut(**{k: nv[k].data_ptr() for k in ("fill", "n_src", "err", "row_err", "row_cov")})
    image_out = _lib.RslfNovelViewOut(**{k: nv[k].data_ptr() for k in ("colour", "depth", "fill", "n_src")})
    targets = (C.c_float * T)(*[float(s) for s in range(S)])
    exclude = (C.c_int * T)(*range(S))
    ctx.use_current_stream()

    def warp(radius):
        _lib.check(L.rslf_view_warp(ctx._h, depth.data_ptr(), mask.data_ptr(), S, V, U, 1.0, vol._h, targets, exclude, T, radius, 1,
                                    C.byref(warp_out)), "rslf_view_warp")

    def novel(radius, sources, max_gap, out=loo_out):
        par = _lib.RslfNovelViewParams(radius, 1, max_gap, sources, tol)
        _lib.check(L.rslf_novel_view(ctx._h, depth.data_ptr(), mask.data_ptr(), S, V, U, 1.0, vol._h, targets, exclude, T, C.byref(par),
                                     C.byref(out)), "rslf_novel_view")

    grid = [(r, s, g) for r in (0, 8) for s in (1, 2, 4) for g in (0, 3)]
    variants = []
    for r in (0, 8):
        variants.append(("warp/r%d" % r, lambda r=r: warp(r)))
        variants += [("novel/r%d/s%d/g%d" % (r, s, g), lambda r=r, s=s, g=g: novel(r, s, g)) for (rr, s, g) in grid if rr == r]
    variants.append(("novel/image", lambda: novel(8, 4, 0, image_out)))
    got = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, f in variants:
            got[name].append(median_ms(f, args.reps))
    out = dict(config=args.config, U=U, V=V, S=S, C=C_, D=D, T=T, tol=tol)
    out["ms"] = {name: dict(median=round(statistics.median(ms), 4), spread=[round(min(ms), 4), round(max(ms), 4)]) for name, ms in got.items()}

    # what the calls found, and the algorithmic bytes with the measured number of views blended per pixel
    found = {}
    for r, s, g in grid:
        novel(r, s, g)
        torch.cuda.synchronize()
        cov = int(nv["row_cov"].sum().item())
        filled = nv["fill"] >= 2
        views = float(nv["n_src"].sum().item()) / cells
        window = S if r <= 0 else min(S, 2 * r + 1)
        found["novel/r%d/s%d/g%d" % (r, s, g)] = dict(
            coverage=round(cov / cells, 4), mean_n_src=round(views, 3), filled=round(float(filled.sum().item()) / cells, 4),
            holes=round(float((nv["fill"] == 0).sum().item()) / cells, 4),
            unblended=round(float(((nv["fill"] != 0) & (nv["n_src"] == 0)).sum().item()) / cells, 4),
            mean_abs_error=float(nv["row_err"].sum().item()) / max(1, cov),
            algorithmic_bytes=int(window * V * U * 5 + cells * views * (8 * C_ + 5) + cells * 4 * C_ + cells * 9 + T * V * 12))
    for r in (0, 8):
        warp(r)
        torch.cuda.synchronize()
        hits = int(w["row_hits"].sum().item())
        found["warp/r%d" % r] = dict(coverage=round(hits / cells, 4), mean_abs_error=float(w["row_err"].sum().item()) / max(1, hits))
    out["truth"] = found

    if not args.no_sweep:
        comp = rs.Depth2DComputer(vol, dmin, dmax, D)
        out["sweep_ms"] = round(median_ms(lambda: comp.run(want_stats=False), args.sweep_reps), 3)
        for name, m in (("default_mask", None), ("consistent_mask", comp.get_consistent_depths_mask_s_v_u())):
            pred = comp.get_view_prediction(mask=m)
            res = dict(warp=dict(mean_abs_error=round(float(np.nanmean(pred.mean_abs_error)), 6), coverage=round(float(pred.coverage.mean()), 4)))
            for g in (0, 3):
                p = comp.get_novel_view_prediction(mask=m, max_gap=g)
                blended = p.n_src > 0
                hit, filled = blended & (p.fill == 1), blended & (p.fill >= 2)
                mean = lambda sel: round(float(p.err[sel].double().mean().item()), 6) if bool(sel.any().item()) else None
                res["novel_gap%d" % g] = dict(mean_abs_error=round(float(np.nanmean(p.mean_abs_error)), 6),
                                              coverage=round(float(p.coverage.mean()), 4), hit_pixels=mean(hit), filled_pixels=mean(filled),
                                              filled_share=round(float(filled.float().mean().item()), 5),
                                              unblended_pixels=mean((p.fill != 0) & ~blended),
                                              unblended_share=round(float(((p.fill != 0) & ~blended).float().mean().item()), 5))
            out["prediction_" + name] = res
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
