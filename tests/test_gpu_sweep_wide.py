"""The 2-D sweep against the oracle on rows as wide as bench.py's frames.

K4 keeps its claim bookkeeping per 256-column segment of a row: the `dirty` flags the claims set, the `remain` counts
k4_count_segments builds, the apply pass that visits flagged segments only, and the claim skip of k34_median_claim, which
derives the segments a workgroup can reach from its disparity range and the slope.  Rows of at most 300 columns hold two
segments and never see a claim land more than 256 columns from its source.  Here: rows on both sides of the segment
edges, c2's row, a far-reaching scene whose claims cross segments, skysat_lr's and mansion_lr's widths at their view and
hypothesis counts, and the two sweep parameters that are otherwise fixed (slope factor, propagation epsilon).  Planes
bit-exact, C_d within 1e-5 (tests/test_gpu_sweep2d.py).

Every case also checks, from the oracle's planes, that its scene does what it is here for: propagation painted pixels in
the far segments of views away from the centre, and, for the far-reaching scene, across more than 256 columns."""
import numpy as np
import pytest

from tests.test_gpu_sweep2d import _check

HOOKS = [{}, dict(claim_skip=0), dict(row_split=0), dict(px=0)]
HOOK_IDS = ["default", "no_claim_skip", "no_row_split", "no_px"]

FAR_DELTAS = (12, -12, 7, -7, 12, -3, 0, 9, -12, 4, -9, 12)   # both signs, |d| = 12 on several scanlines

# name: channels, views, row length, scanlines, hypotheses, dmin, dmax, per-scanline disparities (None: bands of 2),
#       slope factor, propagation epsilon
CASES = {
    **{"edge_u%d" % U: (1, S, U, 4, 24, -2.0, 2.0, None, 1.0, 0.1)
       for U, S in ((255, 9), (256, 13), (257, 17), (511, 9), (513, 13), (769, 17))},
    "c2_row": (1, 33, 512, 6, 128, -1.0, 2.96875, None, 1.0, 0.1),
    "far_reach": (1, 49, 777, 12, 48, -12.0, 12.0, FAR_DELTAS, 1.0, 0.1),
    "skysat_width": (1, 100, 960, 4, 120, -1.0, 4.0, (4, -1, 2.5, 1), 1.0, 0.1),
    "mansion_width": (3, 100, 1146, 4, 120, 0.0, 4.0, (4, 0, 2, 3.5), 1.0, 0.1),
    "slope_0.5": (1, 17, 600, 6, 32, -4.0, 4.0, (4, -4, 2, -3, 1, 3.5), 0.5, 0.1),
    "slope_1.5": (1, 17, 600, 6, 32, -4.0, 4.0, (4, -4, 2, -3, 1, 3.5), 1.5, 0.1),
    **{"eps_%g" % e: (1, 17, 520, 4, 16, -2.0, 2.0, (2, -2, 1, -1), 1.0, e) for e in (0.0, 0.02, 0.5, np.inf)},
}
# the claims' and the apply pass's shortcuts matter where segments are many and claims reach far: every hook there
HOOKED = ("far_reach", "skysat_width", "mansion_width")
RUNS = [(n, h) for n in CASES for h in (range(len(HOOKS)) if n in HOOKED else (0,))]


def scene(C, S, U, V, dmin, dmax, deltas, seed):
    """A clean light field with per-pixel noise, so that propagation fails for many pixels and the sparse visits have work."""
    from remotesensingproject_amd.synth import make_lightfield
    d = None if deltas is None else np.asarray(deltas, np.float32)
    vol, _ = make_lightfield(U, V, S, C, seed=seed, deltas=d, dmin=dmin, dmax=dmax, band=2)
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray((vol + rng.normal(0.0, 0.03, size=vol.shape)).clip(0.0, 1.0), np.float32)


@pytest.fixture(scope="module")
def sweeps(oracle_mod):
    """The oracle's sweep of each case, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            C, S, U, V, D, dmin, dmax, deltas, slope, eps = CASES[name]
            vol = scene(C, S, U, V, dmin, dmax, deltas, seed=U + 7 * S + C)
            p = oracle_mod.default_params()
            p.slope_factor = slope
            cache[name] = (vol, oracle_mod.depth2d_run(vol, dmin, dmax, D, params=p, propagation_epsilon=eps))
        return cache[name]
    return get


def painted_elsewhere(ref):
    """[S,V,U]: pixels another view's visit painted -- in the edge mask, out of the running mask, never scanned.  A scanned
    pixel's rbar is a kernel-weighted mean of radiances along its EPI line, and a scene value is 0 only where noise
    clipped it, so an all-zero rbar marks a pixel no scan reached (a rare exact-0 mean would only undercount)."""
    return (ref.edge_mask > 0) & (ref.scan_mask == 0) & (ref.rbar == 0).all(axis=-1)


def far_views(S):
    sc = S // 2
    return np.abs(np.arange(S) - sc) >= max(1, S // 4)


def long_claims(ref, slope):
    """Pixels painted from the centre view's visit across more than 256 columns: a pixel painted elsewhere whose value d
    puts its source at u = t - round(d * (s_c - s) * slope) in the centre view, where a confident pixel painted itself
    with the same d."""
    S, V, U = ref.depth.shape
    sc = S // 2
    n = 0
    painted = painted_elsewhere(ref)
    for s in range(S):
        v, t = np.nonzero(painted[s])
        d = ref.depth[s, v, t]
        off = (d * np.float32(sc - s)).astype(np.float32) * np.float32(slope)
        u = t - (np.sign(off) * np.floor(np.abs(off) + np.float32(0.5))).astype(np.int64)   # std::round
        ok = (np.abs(off) > 256) & (u >= 0) & (u < U)
        v, u, d = v[ok], u[ok], d[ok]
        n += int(((ref.edge_mask[sc, v, u] > 0) & (ref.scan_mask[sc, v, u] == 0) & (ref.depth[sc, v, u] == d)).sum())
    return n


def check_scene(name, ref):
    """What the case is here for, read from the oracle's planes: a scene that stops exercising its path fails."""
    C, S, U, V, D, dmin, dmax, deltas, slope, eps = CASES[name]
    painted = painted_elsewhere(ref)
    if eps == 0.0:   # nothing is within 0 of anything: no pixel is ever painted, every visit rescans what remains
        assert not ((ref.edge_mask > 0) & (ref.scan_mask == 0)).any(), name
        return
    first = min(512, 256 * ((U - 1) // 256))   # the last segment, or segment 2 and beyond on rows that have it
    n = int(painted[far_views(S)][:, :, first:].sum())
    assert n >= min(20, U - first), (name, "pixels painted at columns >= %d of views far from the centre" % first, n)
    if name == "far_reach":
        n = long_claims(ref, slope)
        assert n >= 20, ("claims across more than 256 columns", n)


@pytest.mark.gpu
@pytest.mark.parametrize("name,hook", RUNS, ids=["%s-%s" % (n, HOOK_IDS[h]) for n, h in RUNS])
def test_wide_sweep_matches_the_oracle(sweeps, hooks, name, hook):
    from remotesensingproject_amd import depth as rs
    C, S, U, V, D, dmin, dmax, deltas, slope, eps = CASES[name]
    vol, ref = sweeps(name)
    check_scene(name, ref)
    if HOOKS[hook]:
        hooks(**HOOKS[hook])
    p = rs.Depth1DParameters(par_slope_factor=slope, par_propagation_epsilon=float(eps))
    comp = rs.Depth2DComputer(vol, dmin, dmax, D, epi_scale_factor=1.0, parameters=p)
    comp.run()
    _check(comp.results(), ref, "%s %s" % (name, HOOKS[hook]))


def test_the_sweep_parameters_reach_the_result(sweeps):
    """The slope factors and the epsilons each give a different sweep: a case that ignored its parameter would be a copy of
    another.  Oracle planes only, so this runs without a GPU."""
    for group in (["slope_0.5", "slope_1.5"], ["eps_0", "eps_0.02", "eps_0.5", "eps_inf"]):
        refs = [sweeps(n)[1] for n in group]
        for i in range(len(refs)):
            for j in range(i + 1, len(refs)):
                assert not (np.array_equal(refs[i].scan_mask, refs[j].scan_mask) and np.array_equal(refs[i].depth, refs[j].depth)), \
                    (group[i], group[j])
    painted = [int(painted_elsewhere(sweeps(n)[1]).sum()) for n in ("eps_0", "eps_0.02", "eps_0.5", "eps_inf")]
    assert painted[0] == 0 < painted[1] < painted[2] < painted[3], painted
