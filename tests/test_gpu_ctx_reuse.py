"""One long-lived context through every entry point that grows its scratch, against a fresh context per step.

A context's buffers only ever grow and are shared between entry points (rslf_internal.hpp: Scratch, SharedBuf), so what a
step computes must not depend on what the context ran before: shapes that regrow some buffers and leave others larger
than needed, the renderers on the buffers the fusion just used, the packed lists' row bases after the per-row buffers
have regrown, and the multi-device object's planes, pinned staging and arena regrown on a live object.  Every step runs
on the long-lived Context(0) and on a new Context(0); the two are compared plane by plane: C_d to 1e-5 (the bound
rslf_hip.h states for launch-shape differences), every other plane bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _field(V, S, U, C, seed, dtype=np.float32):
    """A seeded light field as the reference's Vec<Mat>: V separately allocated EPIs [S,U] / [S,U,3]."""
    from remotesensingproject_amd.synth import make_lightfield
    vol, _ = make_lightfield(U, V, S, C, seed=seed, dmin=-1.0, dmax=1.0, band=2)
    if dtype == np.uint8:
        vol = np.rint(vol * 255.0).astype(np.uint8)
    return [np.array(e[..., 0] if C == 1 else e) for e in vol]


def _pile(ctx, epis, D=12):
    from remotesensingproject_amd import depth as rs
    comp = rs.Depth1DComputer_pile(epis, -1.0, 1.0, D, epi_scale_factor=1.0, ctx=ctx)
    comp.run()
    return comp.results()


def _sweep(ctx, epis, mode, D=12):
    from remotesensingproject_amd import depth as rs
    comp = rs.Depth2DComputer(epis, -1.0, 1.0, D, epi_scale_factor=1.0, parameters=rs.Depth1DParameters(par_line_confidence_mode=mode),
                              ctx=ctx)
    comp.run()
    return comp.results()


def _f2c(ctx, epis, line_mode, D=12):
    from remotesensingproject_amd import depth as rs
    out = rs.fine_to_coarse_run_host(epis, -1.0, 1.0, D, ctx=ctx, line_mode=line_mode, want_levels=True)
    planes = dict(out_map=out["out_map"], out_valid=out["out_valid"], n_levels=np.array([out["n_levels"]]))
    for l, lv in enumerate(out["levels"]):
        for k, a in lv.items():
            if a is not None:
                planes["level%d_%s" % (l, k)] = a
    return planes


def _render(ctx, fused_map, fused_valid):
    import torch
    from remotesensingproject_amd import depth as rs
    planes = torch.from_numpy(np.nan_to_num(fused_map)).cuda()
    valid = torch.from_numpy(fused_valid).cuda()
    lo, hi = rs.render_fit(ctx, planes[planes.shape[0] // 2], valid[valid.shape[0] // 2], rs.FIT_QUANTILE)
    img = rs.render_planes(ctx, planes, lo, hi, rs.RENDER_AFFINE, rs.colormap_jet(), valid, rs.MASK_BLACK)
    torch.cuda.synchronize()
    return dict(fit=np.array([lo, hi]), picture=img.cpu().numpy())


@pytest.fixture(scope="module")
def steps():
    """Every step in order on one context, and on a context of its own: {name: (long-lived, fresh)}."""
    from remotesensingproject_amd import depth as rs
    long_lived = rs.Context(0)
    out = {}

    def both(name, fn, *args, **kw):
        fresh = rs.Context(0)
        out[name] = (fn(long_lived, *args, **kw), fn(fresh, *args, **kw))
        fresh.close()

    both("1_pile", _pile, _field(6, 9, 96, 1, seed=1))
    # two levels, 24 x 44 and 12 x 22: the pyramid, the tightening and the fusion on the shared buffers, the line-confidence
    # buffers, the sweep's scratch, rslf_device_max_f32
    both("2_f2c_u8_gate", _f2c, _field(24, 5, 44, 3, seed=2, dtype=np.uint8), rs.LINE_CONF_GATE)
    fused = out["2_f2c_u8_gate"][0]
    both("3_render", _render, fused["out_map"], fused["out_valid"])   # on the buffers the fusion just used
    # V*U grows (1056 -> 1500) while S*V*U shrinks (5280 -> 4500): the order tools/fuzz_sweep.py found, now for the [V][S][U]
    # K columns and the [V][U] arg-max plane as well
    both("4_sweep_line_conf", _sweep, _field(30, 3, 50, 1, seed=4), rs.LINE_CONF_AS_BUILT)
    epis5 = _field(40, 5, 64, 3, seed=5)
    both("5_pile", _pile, epis5)

    def packed(ctx, epis):   # the packed lists' row bases, after the per-row buffers have regrown
        ctx.set_debug(force_packed=1)
        try:
            return _pile(ctx, epis)
        finally:
            ctx.reset_debug()

    both("5_pile_packed", packed, epis5)
    both("6_f2c_f32", _f2c, _field(32, 4, 64, 1, seed=6), rs.LINE_CONF_OFF)   # every shared buffer regrows after the renderers
    long_lived.close()

    # one multi-device object: planes, pinned staging and the arena regrown on a live object, against single contexts
    m = rs.MultiDevice([0, 0])
    for name, V, S, U in (("7_multi_pile_V12", 12, 5, 64), ("7_multi_pile_V40", 40, 5, 64)):
        epis = _field(V, S, U, 1, seed=70 + V)
        fresh = rs.Context(0)
        out[name] = (m.depth1d_pile(epis, -1.0, 1.0, 12, epi_scale_factor=1.0), _pile(fresh, epis))
        fresh.close()
    for name, V, S, U in (("7_multi_sweep_12x3x40", 12, 3, 40), ("7_multi_sweep_20x3x56", 20, 3, 56)):
        epis = _field(V, S, U, 1, seed=70 + U)
        fresh = rs.Context(0)
        out[name] = (m.depth2d(epis, -1.0, 1.0, 12, epi_scale_factor=1.0), _sweep(fresh, epis, rs.LINE_CONF_OFF))
        fresh.close()
    m.close()
    return out


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("name", ["1_pile", "2_f2c_u8_gate", "3_render", "4_sweep_line_conf", "5_pile", "5_pile_packed", "6_f2c_f32",
                                  "7_multi_pile_V12", "7_multi_pile_V40", "7_multi_sweep_12x3x40", "7_multi_sweep_20x3x56"])
def test_step_does_not_depend_on_the_contexts_history(steps, name):
    got, want = steps[name]
    assert sorted(got) == sorted(want), name
    assert len(got) >= 2
    for k in sorted(got):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (name, k)
        if k == "disp_confidence":
            err = float(np.abs(got[k].astype(np.float64) - want[k].astype(np.float64)).max())
            print("%s %s: max |diff| %.3g" % (name, k, err))
            assert err <= 1e-5, (name, k, err)
        else:
            bad = np.flatnonzero(_bits(got[k]).reshape(-1) != _bits(want[k]).reshape(-1))
            assert bad.size == 0, (name, k, bad.size, np.unravel_index(bad[0], got[k].shape))


def test_the_steps_did_real_work(steps):
    """The comparisons above mean something: pixels were scanned, both pyramids have two levels, line confidence was
    computed, and the picture is not black."""
    assert (steps["1_pile"][0]["edge_mask"] > 0).any() and (steps["5_pile_packed"][0]["edge_mask"] > 0).any()
    f2c = steps["2_f2c_u8_gate"][0]
    assert f2c["n_levels"][0] == 2 and f2c["level0_depth"].shape == (5, 24, 44) and f2c["level1_depth"].shape == (5, 12, 22)
    assert (f2c["level0_line_confidence"] > 0).any() and (f2c["out_valid"] > 0).any()
    assert steps["6_f2c_f32"][0]["n_levels"][0] == 2
    assert steps["3_render"][0]["picture"].any()
    assert (steps["4_sweep_line_conf"][0]["line_confidence"] > 0).any()
    assert (steps["7_multi_sweep_20x3x56"][0]["edge_mask"] > 0).any()
