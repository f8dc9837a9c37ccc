"""Every device entry point on a non-default stream, against the oracle ("Streams").

The rest of the suite runs with torch's current stream equal to the legacy null stream, where a launch, copy, memset or
wait on the wrong stream still gives the right answer.  Here every case runs twice on a Context made under a non-blocking
side stream -- in the scenarios late_inputs and busy_default of tests/stream_harness.py -- and is held to the yardstick its
family's own test file uses: oracle.* for pile, sweep, pyramid, downsample, tighten, fuse and median, the numpy rule files
of this directory for the rest.  Never a null-stream run of the library.  Comparisons are bit for bit; disp_confidence is
held to the 1e-5 include/rslf_hip.h states.

The three controls at the top commit a stream mistake on purpose and must see the wrong answer, or the module proves
nothing.  Shapes are each family's smallest from its own test file.  Outputs the library or a wrapper allocates are
overwritten after they are read, so that a later case that gets the same block back cannot find a right answer in it."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import stream_harness as sh
from tests.stream_harness import SCENARIOS, Late, assert_close, assert_same
from tests.util import assert_pile_parity

pytestmark = pytest.mark.gpu
F = np.float32
TOL_CD = 1e-5
_T0 = time.time()


class Env:
    def __init__(self, oracle_mod):
        import torch
        from remotesensingproject_amd import _lib
        from remotesensingproject_amd import depth as rs
        assert torch.cuda.is_available(), "gpu tests need a GPU"
        self.torch, self.rs, self.o, self.L, self._lib = torch, rs, oracle_mod, _lib.lib(), _lib
        self.h = sh.Harness(0)
        dirty_device_heap(self)               # what the module's context allocates first is not the zeros of fresh memory
        with torch.cuda.stream(self.h.side):
            self.ctx = rs.Context(0)          # made under the side stream, like every case's work
        self.refs = {}

    def ref(self, key, make):
        """One reference per case for both scenarios; shared and left unchanged."""
        if key not in self.refs:
            self.refs[key] = make()
        return self.refs[key]


@pytest.fixture(scope="module")
def env(oracle_mod):
    e = Env(oracle_mod)
    print("side-stream harness: delay of %d cycles = %.1f ms on the side stream, %.1f ms on the null stream"
          % (e.h.cycles, e.h.delay_ms["side"], e.h.delay_ms["null"]))
    yield e
    e.torch.cuda.synchronize()
    e.ctx.close()
    print("side-stream module: %.1f s wall" % (time.time() - _T0))


@pytest.fixture(params=SCENARIOS)
def kind(request):
    return request.param


def scrub(*objs):
    """Poison over device planes: 0 in masks, depth and confidence planes, -1 in index planes.  Before a call: what the
    call must overwrite.  After the results are read: what the next owner of the block must not find."""
    import torch
    for o in objs:
        if o is None or isinstance(o, (int, float, str, bytes, np.ndarray)):
            continue
        if isinstance(o, torch.Tensor):
            if o.is_cuda:
                o.fill_(sh.POISON_INDEX if o.dtype == torch.int32 else 0)
        elif isinstance(o, dict):
            scrub(*o.values())
        elif isinstance(o, (tuple, list)):
            scrub(*o)
        elif hasattr(o, "__dict__"):
            scrub(*[v for k, v in vars(o).items() if k.startswith("m_") and not k.startswith("m_epi") and k != "m_parameters"])


def armed(env, sc, *objs):
    """Poison the planes of `objs`, let the poison land, and start the delay again: the next library call is under test."""
    scrub(*objs)
    env.h.side.synchronize()
    sc.arm()


def dev(env, a):
    """A device input that is NOT under test (made and finished before the scenario starts)."""
    t = env.torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    env.torch.cuda.synchronize()
    return t


def host(t):
    return t.cpu().numpy()


def field(V, S, U, C_, seed, dmin=-1.0, dmax=1.0, band=2):
    from remotesensingproject_amd.synth import make_lightfield
    vol, _ = make_lightfield(U, V, S, C_, seed=seed, dmin=dmin, dmax=dmax, band=band)
    return vol


def epis_of(x):
    return [np.ascontiguousarray(x[v] if x.shape[3] == 3 else x[v, :, :, 0]) for v in range(x.shape[0])]


def ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def hptr(a):
    return C.c_void_p(0 if a is None else a.ctypes.data)


# ---- the controls ------------------------------------------------------------------------------------------------------

def test_control_a_copy_on_a_third_stream_sees_poison_in_late_inputs(env):
    """Torch only: in late_inputs the input is produced behind the delay, and a reader on a third non-blocking stream that
    does not wait reads the poison."""
    torch = env.torch
    real = np.arange(4096, dtype=F).reshape(64, 64) + F(1)
    late = Late(real, 0.5)
    third = torch.cuda.Stream(0)
    out = torch.zeros((64, 64), dtype=torch.float32, device="cuda")
    with env.h.scenario("late_inputs") as sc:
        x = sc.produce(late)
        with torch.cuda.stream(third):
            out.copy_(x, non_blocking=True)
    assert np.array_equal(host(late.t), real)                  # the producer did run ...
    assert np.array_equal(host(out), np.full((64, 64), 0.5, F))   # ... after the reader had read


def test_control_a_null_stream_write_is_not_visible_on_the_side_stream_in_busy_default(env):
    """Torch only: in busy_default a write queued on the null stream waits behind the delay, and a reader on the side
    stream reads what was there before."""
    torch = env.torch
    real = np.arange(4096, dtype=F).reshape(64, 64) + F(1)
    late = Late(real, 0.5)
    out = torch.zeros((64, 64), dtype=torch.float32, device="cuda")
    with env.h.scenario("busy_default"):
        with torch.cuda.stream(torch.cuda.default_stream(0)):
            late.produce()                                     # on the null stream: behind the delay
        out.copy_(late.t, non_blocking=True)                   # on the side stream: at once
    assert np.array_equal(host(late.t), real)
    assert np.array_equal(host(out), np.full((64, 64), 0.5, F))


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_control_the_library_on_the_wrong_stream_gives_a_wrong_answer(env, scenario):
    """A fresh context whose stream is set to NULL by rslf_ctx_set_stream itself, rslf_downsample_epis_f32 through the C ABI
    (pure arithmetic, no data-dependent addressing).  late_inputs: its kernels start at once on the null stream and read the
    poison the input still holds.  busy_default: they wait behind the delay, and the side stream reads the output's
    pre-fill.  Either way the result differs from the oracle's: the harness sees a launch on the wrong stream."""
    torch, rs, L = env.torch, env.rs, env.L
    V, S, U, C_ = 24, 5, 44, 1
    raw = (field(V, S, U, C_, seed=31) * F(200) + F(3)).astype(F)
    want = env.ref(("control_down",), lambda: env.o.downsample_epis(raw))
    late = Late(raw, 100.0)
    out = torch.zeros(want.shape, dtype=torch.float32, device="cuda")
    seen = torch.zeros(want.shape, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx = rs.Context(0)
    try:
        rs.check(L.rslf_ctx_set_stream(ctx._h, C.c_void_p(0)), "rslf_ctx_set_stream")   # deliberately not torch's current stream
        with env.h.scenario(scenario) as sc:
            x = sc.produce(late)
            rs.check(L.rslf_downsample_epis_f32(ctx._h, ptr(x), V, S, U, C_, ptr(out)), "rslf_downsample_epis_f32")
            seen.copy_(out, non_blocking=True)                 # what a consumer on the caller's stream gets
        got = host(seen)
        assert got.shape == want.shape
        assert not np.array_equal(got, want), "a launch on the null stream went unnoticed in %s" % scenario
        # the same call on the caller's stream is the oracle's: the difference above is the stream's alone
        late.reset(100.0)
        scrub(out, seen)
        with env.h.scenario(scenario) as sc:
            ctx.use_current_stream()
            x = sc.produce(late)
            rs.check(L.rslf_downsample_epis_f32(ctx._h, ptr(x), V, S, U, C_, ptr(out)), "rslf_downsample_epis_f32")
            seen.copy_(out, non_blocking=True)
        assert_same(host(seen), want, "downsample on the caller's stream")
    finally:
        torch.cuda.synchronize()
        ctx.close()


def dirty_device_heap(env, fill=0x55):
    """Blocks of the sizes a context's first calls ask for (64 B to 4 MiB), filled with a byte and freed through the HIP
    runtime the library is bound to: where the runtime hands a freed block out again, the scratch a fresh context
    allocates next holds that byte instead of the zeros of fresh device memory, and a set-up memset that did not run
    (or ran late, on another stream) shows.  0x55555555 is a valid value of every cell it can land in: a count that
    is never reached, a total, a float of 1.5e13; nothing is indexed by it."""
    L = env.L
    L.hipMalloc.argtypes, L.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
    L.hipMemset.argtypes, L.hipMemset.restype = [C.c_void_p, C.c_int, C.c_size_t], C.c_int
    L.hipFree.argtypes, L.hipFree.restype = [C.c_void_p], C.c_int
    blocks = []
    for k in range(17):
        for _ in range(3):
            p = C.c_void_p()
            assert L.hipMalloc(C.byref(p), 64 << k) == 0 and L.hipMemset(p, fill, 64 << k) == 0
            blocks.append(p)
    env.torch.cuda.synchronize()
    for p in blocks:
        assert L.hipFree(p) == 0


def test_context_created_while_the_null_stream_is_busy(env):
    """busy_default with the context itself made inside: its set-up writes (the pixel total, the min / max cell, the
    tickets of its first grouped scan) must not sit on the null stream, behind the delay, when the side stream uses them.
    The device heap is dirtied first, so that a write that has not happened yet leaves something other than zeros."""
    rs = env.rs
    vol = field(5, 9, 70, 1, seed=8)
    D = 64                                                     # >= 32 hypotheses: grouped launches, tickets
    ref = env.ref(("fresh_ctx",), lambda: env.o.depth1d_pile_run(vol, -1.0, 1.0, D))
    dirty_device_heap(env)
    with env.h.scenario("busy_default"):
        ctx = rs.Context(0)
        ctx.set_debug(force_groups=4)
        comp = rs.Depth1DComputer_pile(epis_of(vol), -1.0, 1.0, D, epi_scale_factor=1.0, ctx=ctx)
        scrub(comp)
        comp.run()
        got = comp.results()
    assert_pile_parity(got, ref, label="fresh context under a busy null stream")
    scrub(comp)
    env.torch.cuda.synchronize()
    ctx.close()


# ---- uploads and pack --------------------------------------------------------------------------------------------------

def _upload_ref(env, hs, C_, elem, rotated):
    def make():
        raw, factor = hs.raw_of(hs.field("A", C_), elem)
        norm, scale = hs.normalised(env.o, hs.restated(raw, rotated), elem, factor)
        ref = env.o.depth1d_pile_run(norm, -1.0, 2.0, 12)
        assert (ref.edge_mask != 0).mean() >= 0.5
        return norm, float(scale), ref
    return env.ref(("upload", C_, elem, rotated), make)


UPLOADS = [("epis", "f32", 1, None, 0), ("epis", "u8", 3, None, 0), ("epis", "u16", 1, None, 0), ("epis", "f32", 3, "right1", 0),
           ("epis", "u8", 1, "both16", 0), ("images", "u8", 1, None, 0), ("images", "f32", 1, "double", 0), ("tr", "f32", 1, None, 0),
           ("tr", "u16", 1, "right1", 0), ("epis", "f32", 1, None, 12), ("tr", "u8", 3, None, 12), ("images", "u16", 1, None, 12)]


@pytest.mark.parametrize("form,elem,C_,pad,rows_per_pass", UPLOADS,
                         ids=["%s_%s_C%d_%s_%s" % (f, e, c, p or "dense", "two_passes" if r else "one_pass") for f, e, c, p, r in UPLOADS])
def test_uploads(env, kind, form, elem, C_, pad, rows_per_pass):
    """Volume.from_epis / from_images (plain; transposed and rotated), dense and padded rows, one pass and -- with
    "staging_kib" -- two (12 scanlines, then 11): the staged copies, the pack kernels and the min / max fold all on the
    caller's stream, and the volume complete when the call returns.  Held through the pile run of the uploaded volume."""
    import tests.test_gpu_host_strides as hs
    rs, ctx = env.rs, env.ctx
    rotated = form == "tr"
    raw, factor = hs.raw_of(hs.field("A", C_), elem)
    norm, scale, ref = _upload_ref(env, hs, C_, elem, rotated)
    arrays = [np.ascontiguousarray(e) for e in hs.epis_of(raw)] if form == "epis" else hs.images_of(raw, rotated)
    if pad is not None:
        arrays = hs.windows(arrays, pad)
        hs.assert_in_place(rs, arrays)
    try:
        if rows_per_pass:
            V, S, U = raw.shape[:3]
            ctx.set_debug(staging_kib=hs.staging_kib_for(rows_per_pass, S * U * C_ * raw.dtype.itemsize))
        with env.h.scenario(kind) as sc:
            if form == "epis":
                vol = rs.Volume.from_epis(arrays, factor, ctx)
            else:
                vol = rs.Volume.from_images(arrays, factor, ctx, transpose=rotated, rotate_180=rotated)
            d = vol.describe()
            comp = rs.Depth1DComputer_pile(vol, -1.0, 2.0, 12)
            armed(env, sc, comp)
            comp.run()
            got = comp.results()
    finally:
        ctx.reset_debug()
    assert vol.scale_used == scale
    assert (d.min_value, d.max_value) == (float(norm.min()), float(norm.max()))
    assert_pile_parity(got, ref, label="upload %s %s C%d %s in %s" % (form, elem, C_, pad, kind))
    scrub(comp)


def test_from_dense_of_a_tensor_produced_late(env, kind):
    """rslf_volume_pack_device_f32 of a CUDA tensor whose values arrive on the side stream behind the delay, with a given
    factor; the slab's min / max are what the pack finds."""
    rs = env.rs
    vol = field(6, 9, 96, 3, seed=3)
    raw = (vol * F(173.0)).astype(F)

    def make():
        norm, scale = env.o.normalize_f32(raw, 173.0)
        return norm, float(scale), env.o.depth1d_pile_run(norm, -1.0, 1.0, 12)
    norm, scale, ref = env.ref(("from_dense",), make)
    late = Late(raw, 100.0)
    with env.h.scenario(kind) as sc:
        v = rs.Volume.from_dense(sc.produce(late), 173.0, env.ctx)
        d = v.describe()
        comp = rs.Depth1DComputer_pile(v, -1.0, 1.0, 12)
        armed(env, sc, comp)
        comp.run()
        got = comp.results()
    assert v.scale_used == scale and (d.min_value, d.max_value) == (float(norm.min()), float(norm.max()))
    assert_pile_parity(got, ref, label="from_dense late in " + kind)
    scrub(comp)


# ---- the pile step -------------------------------------------------------------------------------------------------------

PILE = [((6, 9, 96, 1), {}, 1), ((4, 7, 90, 3), {}, 1), ((6, 9, 96, 1), dict(force_scan="stream"), 2),
        ((4, 7, 90, 3), dict(force_scan="stream"), 2), ((6, 9, 96, 1), dict(force_scan="generic"), 0),
        ((6, 9, 96, 1), dict(force_packed=1), 1), ((4, 7, 90, 3), dict(force_packed=1), 1),
        ((6, 9, 96, 1), dict(force_groups=4, force_packed=1), 1)]


def _pile_ref(env, shape, D):
    V, S, U, C_ = shape
    vol = field(V, S, U, C_, seed=V + S)
    return vol, env.ref(("pile", shape, D), lambda: env.o.depth1d_pile_run(vol, -1.0, 1.0, D))


@pytest.mark.parametrize("shape,debug,kernel", PILE, ids=["%dx%dx%dx%d_%s" % (s + ("_".join("%s_%s" % kv for kv in d.items()) or "auto",))
                                                           for s, d, _ in PILE])
def test_depth1d_computer_pile(env, kind, shape, debug, kernel):
    """Depth1DComputer_pile from a CUDA tensor produced late (the pack), then run() (K1, the scan in every launch form, K3)
    with the delay armed again and every output plane poisoned."""
    rs, ctx = env.rs, env.ctx
    D = 36 if "force_groups" in debug else 12
    vol, ref = _pile_ref(env, shape, D)
    late = Late(vol, sh.POISON_RADIANCE)
    try:
        ctx.set_debug(**debug)
        with env.h.scenario(kind) as sc:
            comp = rs.Depth1DComputer_pile(sc.produce(late), -1.0, 1.0, D, epi_scale_factor=1.0, ctx=ctx)
            armed(env, sc, comp)
            comp.run()
            got = comp.results()
    finally:
        ctx.reset_debug()
    assert comp.stats.scan_kernel == kernel, comp.stats.scan_kernel
    assert_pile_parity(got, ref, label="pile %s %s in %s" % (shape, debug, kind))
    scrub(comp)


def test_pile_entries_in_the_sub_grid_mode(env, kind):
    """rslf_depth1d_pile_run_sub (Depth1DComputer_pile(subgrid=True)) and rslf_depth1d_run_sub (Depth1DComputer(subgrid=True)):
    the refinement queued between the scan and the median, against tests/subgrid_ref.py."""
    import subgrid_ref as sr
    rs, ctx = env.rs, env.ctx
    V, S, U, D = 6, 9, 96, 9
    vol = field(V, S, U, 1, seed=15)
    ref = env.ref(("pile_sub",), lambda: sr.pile_run(vol, F(-1), F(1), D))
    assert (ref["idx"] >= 0).sum() > 100
    with env.h.scenario(kind) as sc:
        comp = rs.Depth1DComputer_pile(epis_of(vol), -1.0, 1.0, D, epi_scale_factor=1.0, ctx=ctx, subgrid=True)
        armed(env, sc, comp)
        comp.run()
        got = comp.results()
        one = rs.Depth1DComputer(vol[3, :, :, 0], -1.0, 1.0, D, epi_scale_factor=1.0, ctx=ctx, subgrid=True)
        armed(env, sc, one)
        one.run()
        g1 = one.results()
        # the scan and the pile entry on planes the caller prepared (rslf_edge_confidence_pile, then rslf_depth_epi_scan_sub /
        # rslf_depth_epi_pile_sub): edge confidence first, zeros elsewhere
        torch = env.torch
        by_entry = {}
        for fn in (rs.compute_1D_depth_epi, rs.compute_1D_depth_epi_pile):
            z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
            Ce, Cd, depth, rbar = z(V, U), z(V, U), z(V, U), z(V, U, 1)
            env.h.side.synchronize()
            sc.arm()
            mask = rs.compute_1D_edge_confidence_pile(comp.m_epis, S // 2, Ce)
            fn(comp.m_epis, -1.0, 1.0, D, S // 2, Ce, mask, Cd, depth, rbar, subgrid=True)
            by_entry[fn.__name__] = (host(depth), host(mask), host(rbar))
            scrub(Ce, Cd, depth, rbar, mask)
    for name, want in (("compute_1D_depth_epi", ref["depth_raw_sub"]), ("compute_1D_depth_epi_pile", ref["depth_sub"])):
        assert_same(by_entry[name][0], want, "%s(subgrid) depth in %s" % (name, kind))
        assert_same(by_entry[name][1], ref["Ce_mask"], "%s(subgrid) mask in %s" % (name, kind))
        assert_same(by_entry[name][2], ref["rbar"], "%s(subgrid) rbar in %s" % (name, kind))
    for k, r in (("depth", "depth_sub"), ("depth_raw", "depth_raw_sub"), ("depth_idx", "idx"), ("edge_mask", "Ce_mask")):
        assert_same(got[k], ref[r], "Depth1DComputer_pile(subgrid) %s in %s" % (k, kind))
    assert_same(g1["depth"], ref["depth_raw_sub"][3], "Depth1DComputer(subgrid) depth in " + kind)
    assert_same(g1["depth_idx"], ref["idx"][3], "Depth1DComputer(subgrid) idx in " + kind)
    scrub(comp, one)


@pytest.mark.parametrize("C_,elem", [(1, "f32"), (3, "u8")])
def test_depth1d_computer_of_one_epi(env, kind, C_, elem):
    """Depth1DComputer (rslf_depth1d_run): one EPI from the host, its constructor's normalisation, edge confidence + scan."""
    rs = env.rs
    rng = np.random.default_rng(17)
    S, U, D = 11, 130, 14
    if elem == "u8":
        raw = rng.integers(0, 256, size=(S, U, C_), dtype=np.uint8)
        epi_n = env.o.normalize_u8(raw)
    else:
        raw = rng.uniform(5.0, 200.0, size=(S, U)).astype(F)
        epi_n, _ = env.o.normalize_f32(raw[..., None], -1.0)
    epi_n = np.ascontiguousarray(epi_n.reshape(S, U, C_))

    def make():
        Ce, cm = env.o.edge_confidence_pile(epi_n[None], S // 2)
        return env.o.depth_epi(epi_n, np.full(U, -1.0, F), np.full(U, 2.0, F), D, S // 2, Ce[0], cm[0])
    ref = env.ref(("one_epi", elem), make)
    with env.h.scenario(kind) as sc:
        one = rs.Depth1DComputer(raw, -1.0, 2.0, D, ctx=env.ctx)
        armed(env, sc, one)
        one.run()
        g = one.results()
    for k, r in (("edge_mask", "Ce_mask"), ("depth_idx", "idx"), ("edge_confidence", "Ce"), ("score", "score"), ("depth", "depth"),
                 ("rbar", "rbar")):
        assert_same(g[k], ref[r], "Depth1DComputer %s %s in %s" % (elem, k, kind))
    assert_close(g["disp_confidence"], ref["Cd"], TOL_CD, "Depth1DComputer C_d")
    scrub(one)


def test_depth_epi_pile_with_per_pixel_planes_produced_late(env, kind):
    """compute_1D_depth_epi_pile: the range planes, the edge confidence, its mask and the caller's scan mask all arrive on
    the side stream behind the delay (poison: dmin in both range planes, zero masks: a scan that read them finds nothing)."""
    torch, rs = env.torch, env.rs
    rng = np.random.default_rng(77)
    V, S, U, D = 6, 9, 96, 12
    vol = field(V, S, U, 1, seed=V + S)
    dmin = rng.uniform(-2.0, 0.0, size=(V, U)).astype(F)
    dmax = (dmin + rng.uniform(0.0, 3.0, size=(V, U))).astype(F)
    mask = (rng.uniform(size=(V, U)) < 0.6).astype(np.uint8) * 255
    mask[2] = 0

    def make():
        Ce, cm = env.o.edge_confidence_pile(vol, S // 2)
        return Ce, cm, env.o.depth_epi_pile(vol, dmin, dmax, D, S // 2, Ce.copy(), cm.copy(), mask_vu=mask.copy())
    Ce, cm, ref = env.ref(("pile_planes",), make)
    assert (ref.depth_idx >= 0).sum() > 50
    L_vol = Late(vol, sh.POISON_RADIANCE)
    L_in = [Late(dmin, -2.0), Late(dmax, -2.0), Late(Ce, 0.0), Late(cm, sh.POISON_MASK), Late(mask, sh.POISON_MASK)]
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device="cuda")
    tCd, tdepth, trbar, tsc, traw = z(V, U), z(V, U), z(V, U, 1), z(V, U), z(V, U)
    tidx = torch.full((V, U), 7, dtype=torch.int32, device="cuda")
    with env.h.scenario(kind) as sc:
        v = rs.Volume.from_dense(sc.produce(L_vol), 1.0, env.ctx)
        armed(env, sc)
        tlo, thi, tCe, tcm, tmask = sc.produce(*L_in)
        rs.compute_1D_depth_epi_pile(v, tlo, thi, D, S // 2, tCe, tcm, tCd, tdepth, trbar, None, tmask, idx_v_u=tidx, score_v_u=tsc,
                                     depth_raw_v_u=traw)
    for name, t, want in (("depth_idx", tidx, ref.depth_idx), ("score", tsc, ref.score), ("depth", tdepth, ref.depth),
                          ("depth_raw", traw, ref.depth_raw), ("rbar", trbar, ref.rbar), ("edge_mask", tcm, ref.edge_mask),
                          ("edge_confidence", tCe, ref.edge_confidence), ("scan_mask", tmask, ref.scan_mask)):
        assert_same(host(t), want, "per-pixel planes %s in %s" % (name, kind))
    assert_close(host(tCd), ref.disp_confidence, TOL_CD, "per-pixel planes C_d")


def _row_exact_inputs(env, grid):
    """The smallest shape of tests/test_gpu_scalar_taps.py that k2_scan_reg<104,1> takes with the row-exact table: 3 rows of
    320 pixels, 101 views, every pixel confident, scalar range."""
    import tests.test_gpu_scalar_taps as st
    U, S = 320, 101
    vol = st.field(U, S)
    Ce, cm, mask = st.masks(U, False)
    ref = env.ref(("row_exact", grid), lambda: st.reference(env.o, U, S, grid, 1.0, 10.0, False, S // 2))
    return vol, Ce, cm, mask, ref


def _row_exact_call(env, v, grid, lates, outs, want_stats):
    rs = env.rs
    tCe, tcm, tmask = (x.produce() for x in lates)
    P = rs.Depth1DParameters(par_slope_factor=1.0, par_mean_shift_max_iter=10.0)
    return rs.compute_1D_depth_epi_pile(v, grid[0], grid[1], grid[2], 50, tCe, tcm, outs["disp_confidence"], outs["depth"], outs["rbar"], P,
                                        tmask, idx_v_u=outs["depth_idx"], score_v_u=outs["score"], depth_raw_v_u=outs["depth_raw"],
                                        want_stats=want_stats)


def _row_exact_outs(env):
    torch = env.torch
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device="cuda")
    return dict(disp_confidence=z(3, 320), depth=z(3, 320), rbar=z(3, 320, 1), depth_idx=torch.full((3, 320), 7, dtype=torch.int32, device="cuda"),
                score=z(3, 320), depth_raw=z(3, 320))


def _row_exact_check(outs, ref, label):
    for k in ("depth", "rbar", "depth_idx", "score", "depth_raw"):
        assert_same(host(outs[k]), getattr(ref, k), "%s: %s" % (label, k))
    assert_close(host(outs["disp_confidence"]), ref.disp_confidence, TOL_CD, label + ": C_d")


def test_row_exact_table_is_filled_on_the_callers_stream(env, kind):
    """k2_fill_row_exact and the scan that reads its table (k2_scan_reg<104,1>, scalar taps): both on the side stream."""
    import tests.test_gpu_scalar_taps as st
    rs, ctx = env.rs, env.ctx
    grid = st.G7
    vol, Ce, cm, mask, ref = _row_exact_inputs(env, grid)
    L_vol, lates = Late(vol, sh.POISON_RADIANCE), [Late(Ce, 0.0), Late(cm, sh.POISON_MASK), Late(mask, sh.POISON_MASK)]
    outs = _row_exact_outs(env)
    try:
        ctx.set_debug(scalar_taps=1, force_groups=0, force_packed=0)
        with env.h.scenario(kind) as sc:
            v = rs.Volume.from_dense(sc.produce(L_vol), 1.0, ctx)
            armed(env, sc)
            stats = _row_exact_call(env, v, grid, lates, outs, True)
            attached = ctx.last_scan_row_exact()
    finally:
        ctx.reset_debug()
    assert (stats.scan_kernel, stats.s_pad) == (1, 104) and attached == (True, 3), (stats.scan_kernel, stats.s_pad, attached)
    _row_exact_check(outs, ref, "row-exact in " + kind)


def test_a_scan_on_another_stream_refills_the_row_exact_table(env):
    """RowExactKey::queued_on (rslf_internal.hpp): a table whose fill was queued on stream A is not trusted by a scan on
    stream B.  Call 0 fills the table for range R1 on A and is awaited.  Behind a delay on A, call 1 asks for R2 (same V, S,
    U, D): its refill is queued, not run.  The context then moves to B, where call 2 asks for R2 and is awaited while A still
    sleeps.  A library that trusted the table on B would read R1's entries -- in bounds, and wrong.  Both results must be
    the oracle's for R2.

    This case leans on queued_on alone.  It is not something INTEGRATION.md invites callers to do: one context is not to
    have work in flight on two streams, and only the table is protected here (call 2 has finished before call 1 starts)."""
    torch, rs = env.torch, env.rs
    R1, R2 = (-1.0, 1.0, 7), (-1.5, 1.5, 7)
    vol, Ce, cm, mask, ref1 = _row_exact_inputs(env, R1)
    ref2 = _row_exact_inputs(env, R2)[4]
    assert not np.array_equal(ref1.depth, ref2.depth)
    A, B = env.h.side, torch.cuda.Stream(0)
    lates = [[Late(Ce, 0.0), Late(cm, sh.POISON_MASK), Late(mask, sh.POISON_MASK)] for _ in range(3)]
    outs = [_row_exact_outs(env) for _ in range(3)]
    tvol = dev(env, vol)
    with env.h.on(A):
        ctx = rs.Context(0)
        ctx.set_debug(scalar_taps=1, force_groups=0, force_packed=0)
        v = rs.Volume.from_dense(tvol, 1.0, ctx)
        st0 = _row_exact_call(env, v, R1, lates[0], outs[0], True)          # call 0: R1, awaited (the stats wait)
        assert (st0.scan_kernel, st0.s_pad) == (1, 104) and ctx.last_scan_row_exact() == (True, 3)
        A.synchronize()
        env.h.delay(A)
        _row_exact_call(env, v, R2, lates[1], outs[1], False)               # call 1: R2, queued behind the delay
        with torch.cuda.stream(B):
            st2 = _row_exact_call(env, v, R2, lates[2], outs[2], True)      # call 2: R2 on B, awaited while A sleeps
            attached = ctx.last_scan_row_exact()
            B.synchronize()
            early = {k: host(t) for k, t in outs[2].items()}
        A.synchronize()
    assert (st2.scan_kernel, st2.s_pad) == (1, 104) and attached[0] and attached[1] >= 3, (st2.scan_kernel, attached)
    _row_exact_check(outs[0], ref1, "call 0 (R1 on A)")
    for k in ("depth", "rbar", "depth_idx", "score", "depth_raw"):
        assert_same(early[k], getattr(ref2, k), "call 2 (R2 on B, read while A slept): " + k)
    _row_exact_check(outs[1], ref2, "call 1 (R2 on A)")
    _row_exact_check(outs[2], ref2, "call 2 (R2 on B)")
    torch.cuda.synchronize()
    ctx.close()


def test_pile_run_host_with_poisoned_host_planes(env, kind):
    """rslf_depth1d_pile_run_host: device planes carved from the context's scratch, eight downloads and one wait.  A wait on
    another stream than the downloads' hands the host planes back with their poison."""
    rs, L = env.rs, env.L
    shape, D = (6, 9, 96, 1), 12
    V, S, U, C_ = shape
    vol, ref = _pile_ref(env, shape, D)
    out = dict(edge_confidence=sh.host_poison((V, U), F, 0.0), edge_mask=sh.host_poison((V, U), np.uint8, 0),
               disp_confidence=sh.host_poison((V, U), F, 0.0), depth=sh.host_poison((V, U), F, 0.0), rbar=sh.host_poison((V, U, C_), F, 0.0),
               depth_idx=sh.host_poison((V, U), np.int32, -1), score=sh.host_poison((V, U), F, 0.0), depth_raw=sh.host_poison((V, U), F, 0.0))
    p, st = rs.Depth1DParameters().to_c(), env._lib.RslfStats()
    with env.h.scenario(kind) as sc:
        v = rs.Volume.from_epis(epis_of(vol), 1.0, env.ctx)
        armed(env, sc)
        env.ctx.use_current_stream()
        rs.check(L.rslf_depth1d_pile_run_host(env.ctx._h, v._h, -1.0, 1.0, D, -1, C.byref(p), *[hptr(out[k]) for k in (
            "edge_confidence", "edge_mask", "disp_confidence", "depth", "rbar", "depth_idx", "score", "depth_raw")], C.byref(st)),
            "rslf_depth1d_pile_run_host")
        got = {k: a.copy() for k, a in out.items()}             # as they are when the call returns
    assert st.pixels_scanned == int((env.o.edge_confidence_pile(vol, S // 2)[1] > 0).sum())
    assert_pile_parity(got, ref, label="pile_run_host in " + kind)


# ---- the 2-D sweep ---------------------------------------------------------------------------------------------------------

SWEEP_SHAPES = [(12, 3, 40, 1), (10, 5, 64, 3)]
SWEEP_MODES = ["off", "line_as_built", "subgrid", "peaks", "peaks_ratio"]
SWEEP_D = 12
RATIO = 0.5   # the ratio at which both shapes withhold sources (the three-channel one withholds none at 0.9)


def _sweep_ref(env, shape, mode):
    import sweep_gate_ref as sgr
    V, S, U, C_ = shape
    vol = field(V, S, U, C_, seed=70 + U)

    def make():
        if mode == "off":
            r = env.o.depth2d_run(vol, -1.0, 1.0, SWEEP_D)
            return {k: getattr(r, k) for k in ("edge_confidence", "edge_mask", "disp_confidence", "depth", "rbar", "scan_mask")}, None, 0
        lo, hi = np.full((S, V, U), -1.0, F), np.full((S, V, U), 1.0, F)
        planes, pk, _, withheld, _, _ = sgr.sweep(env.o, vol, lo, hi, SWEEP_D, env.o.default_params(), mode=1 if mode == "line_as_built" else 0,
                                                  subgrid=mode == "subgrid", ratio=RATIO if mode == "peaks_ratio" else 0.0)
        return planes, pk, sum(withheld)
    return (vol,) + env.ref(("sweep", shape, mode), make)


def _sweep_check(got, planes, label, line=False):
    for k in ("edge_mask", "scan_mask", "edge_confidence", "depth", "rbar") + (("line_confidence",) if line else ()):
        assert_same(got[k], planes[k], "%s: %s" % (label, k))
    assert_close(got["disp_confidence"], planes["disp_confidence"], TOL_CD, label + ": C_d")


@pytest.mark.parametrize("mode", SWEEP_MODES)
@pytest.mark.parametrize("shape", SWEEP_SHAPES, ids=["%dx%dx%dx%d" % s for s in SWEEP_SHAPES])
def test_depth2d_computer(env, kind, shape, mode):
    """Depth2DComputer.run() (rslf_depth2d_run_pr): off, LINE_CONF_AS_BUILT, sub-grid, peaks, and peaks with a propagation
    ratio (rslf_sweep_withheld asserted too) -- every visit's scan, median, line confidence, peaks step and propagation, and
    the memsets that open the sweep, on the caller's stream."""
    rs = env.rs
    vol, planes, pk, withheld = _sweep_ref(env, shape, mode)
    par = rs.Depth1DParameters(par_line_confidence_mode=rs.LINE_CONF_AS_BUILT if mode == "line_as_built" else rs.LINE_CONF_OFF)
    peaks = mode in ("peaks", "peaks_ratio")
    late = Late(vol, sh.POISON_RADIANCE)
    n_withheld = None
    with env.h.scenario(kind) as sc:
        comp = rs.Depth2DComputer(sc.produce(late), -1.0, 1.0, SWEEP_D, epi_scale_factor=1.0, parameters=par, ctx=env.ctx,
                                  subgrid=mode == "subgrid", peaks=peaks, propagation_ratio=RATIO if mode == "peaks_ratio" else None)
        armed(env, sc, comp)
        comp.run(want_stats=False)
        if mode == "peaks_ratio":
            n_withheld = comp.get_withheld_sources()           # waits for the stream it was counted on
        got = comp.results()
        got_pk = {k: host(getattr(comp.get_peaks_s_v_u(), k)) for k in ("idx", "score", "runner_idx", "runner_score")} if peaks else None
    label = "sweep %s %s in %s" % (shape, mode, kind)
    _sweep_check(got, planes, label, line=mode == "line_as_built")
    if peaks:
        for k in got_pk:
            assert_same(got_pk[k], pk[k], "%s: peaks.%s" % (label, k))
    if mode == "peaks_ratio":
        assert n_withheld == withheld and withheld > 0, (n_withheld, withheld)
    scrub(comp, comp.m_peaks_s_v_u)


def test_sweep_through_the_visit_api(env, kind):
    """rslf_edge_confidence_2d, then rslf_sweep_begin ... visit_scan / visit_finish ... rslf_sweep_end on caller planes that
    start as poison-free zeros produced late."""
    import line_conf_ref as lcr
    torch, rs, L, ctx = env.torch, env.rs, env.L, env.ctx
    shape = SWEEP_SHAPES[0]
    V, S, U, C_ = shape
    vol, planes, _, _ = _sweep_ref(env, shape, "off")
    late = Late(vol, sh.POISON_RADIANCE)
    n = (S, V, U)
    t = dict(edge_confidence=torch.zeros(n, device="cuda"), disp_confidence=torch.zeros(n, device="cuda"), depth=torch.zeros(n, device="cuda"),
             rbar=torch.zeros(n + (C_,), device="cuda"), scan_mask=torch.zeros(n, dtype=torch.uint8, device="cuda"))
    p, st = rs.Depth1DParameters().to_c(), env._lib.RslfStats()
    with env.h.scenario(kind) as sc:
        v = rs.Volume.from_dense(sc.produce(late), 1.0, ctx)
        armed(env, sc)
        t["edge_mask"] = rs.compute_2D_edge_confidence(v, t["edge_confidence"])
        q = lambda k: ptr(t[k])
        rs.check(L.rslf_sweep_begin(ctx._h, v._h, q("edge_mask"), q("scan_mask"), SWEEP_D, 0, V), "rslf_sweep_begin")
        for s_hat in lcr.sweep_order(S):
            rs.check(L.rslf_sweep_visit_scan(ctx._h, v._h, None, None, -1.0, 1.0, SWEEP_D, s_hat, q("edge_confidence"), q("edge_mask"),
                                             q("disp_confidence"), q("depth"), q("rbar"), C.byref(p)), "rslf_sweep_visit_scan")
            rs.check(L.rslf_sweep_visit_finish(ctx._h, v._h, s_hat, q("edge_mask"), q("disp_confidence"), q("depth"), q("rbar"), C.byref(p)),
                     "rslf_sweep_visit_finish")
        rs.check(L.rslf_sweep_end(ctx._h, 1, SWEEP_D, C.byref(st)), "rslf_sweep_end")
    _sweep_check({k: host(x) for k, x in t.items()}, planes, "visit API in " + kind)
    assert st.pixels_scanned > 0
    scrub(t)


# ---- the pyramid -------------------------------------------------------------------------------------------------------------

def _f2c_raw(C_, elem, V=24, S=5, U=44, seed=2):
    vol = field(V, S, U, C_, seed=seed)
    if elem == "u8":
        return np.rint(vol * 255.0).astype(np.uint8)
    if elem == "u16":
        return np.rint(vol / vol.max() * 4095).astype(np.uint16)
    return (vol * F(200) + F(3)).astype(F)


def _f2c_oracle(env, C_, elem, mode=0, D=12):
    """oracle.fine_to_coarse_run for the default build, the numpy line-confidence pyramid for a line mode, the restated 16U
    pyramid of tests/test_gpu_u16.py for ushort fields."""
    import f2c_keep_ref as kr
    raw = _f2c_raw(C_, elem)

    def make():
        ref = kr.fine_to_coarse(env.o, raw.astype(F), -1.0, 1.0, D, mode=mode, elem=elem)
        assert len(ref["dims"]) == 2, ref["dims"]
        return ref
    return raw, env.ref(("f2c", C_, elem, mode, D), make)


def _run_host_f2c(env, epis, D, line_mode, P):
    """rslf_fine_to_coarse_run_host_sub through the C ABI with every host plane pre-filled with poison."""
    rs, L, ctx = env.rs, env.L, env.ctx
    keep, ptrs, dt, V, S, U, C_, stride = rs.host_epis(epis, stride=True)
    out_map, out_valid = sh.host_poison((S, V, U), F, 0.0), sh.host_poison((S, V, U), np.uint8, 0)
    Vp, Up, nl = (C.c_int * P)(), (C.c_int * P)(), C.c_int()
    rs.check(L.rslf_f2c_pyramid_dims(V, U, -1, Vp, Up, P, C.byref(nl)), "rslf_f2c_pyramid_dims")
    assert nl.value == P
    levels = []
    for l in range(P):
        s = (S, Vp[l], Up[l])
        levels.append(dict(depth=sh.host_poison(s, F, 0.0), valid=sh.host_poison(s, np.uint8, 0),
                           line_confidence=sh.host_poison(s, F, 0.0) if line_mode else None, edge_confidence=sh.host_poison(s, F, 0.0)))
    arr = lambda k: (C.c_void_p * P)(*[None if lv[k] is None else lv[k].ctypes.data for lv in levels])
    lo = env._lib.RslfF2cLevelsOut(P, arr("depth"), arr("valid"), arr("line_confidence"), arr("edge_confidence"))
    p, st = rs.Depth1DParameters().to_c(), env._lib.RslfStats()
    ctx.use_current_stream()
    rs.check(L.rslf_fine_to_coarse_run_host_sub(ctx._h, ptrs, rs._ELEM[np.dtype(dt)], V, S, U, C_, stride, -1.0, 1.0, D, -1.0, C.byref(p), -1, 1,
                                                hptr(out_map), hptr(out_valid), C.byref(nl), C.byref(st), int(line_mode), C.byref(lo), 0),
             "rslf_fine_to_coarse_run_host_sub")
    return out_map.copy(), out_valid.copy(), [{k: (None if a is None else a.copy()) for k, a in lv.items()} for lv in levels], st


F2C_HOST = [(3, "u8", 2), (1, "f32", 0), (1, "u16", 0)]


@pytest.mark.parametrize("C_,elem,mode", F2C_HOST, ids=["u8_rgb_line_gate", "f32_one_channel", "u16"])
def test_fine_to_coarse_run_host_with_levels(env, kind, C_, elem, mode):
    """fine_to_coarse_run_host(want_levels=True): 24 x 44 and 12 x 22, the raw upload, every level's scale (rslf_device_max_f32),
    downsample, sweep, validity, the tightening, the fusion, and the downloads of every level's planes and one wait."""
    raw, ref = _f2c_oracle(env, C_, elem, mode)
    with env.h.scenario(kind):
        om, ov, levels, st = _run_host_f2c(env, epis_of(raw), 12, mode, 2)
    label = "f2c host %s C%d mode %d in %s" % (elem, C_, mode, kind)
    assert_same(om, ref["fused_map"], label + ": fused map")
    assert_same(ov, ref["fused_valid"], label + ": fused validity")
    for l, lv in enumerate(levels):
        assert_same(lv["depth"], ref["levels"][l]["depth"], "%s: level %d depth" % (label, l))
        assert_same(lv["valid"], ref["levels"][l]["valid"], "%s: level %d valid" % (label, l))
        assert_same(lv["edge_confidence"], ref["levels"][l]["edge_confidence"], "%s: level %d C_e" % (label, l))
        if mode:
            assert_same(lv["line_confidence"], ref["levels"][l]["line_confidence"], "%s: level %d C_l" % (label, l))
    assert st.pixels_scanned > 0


@pytest.mark.parametrize("C_,elem", [(1, "f32"), (3, "u8")], ids=["f32", "u8_rgb"])
def test_fine_to_coarse_python_level_loop(env, kind, C_, elem):
    """FineToCoarse: f2c_input, rslf_device_max_f32, downsample_EPIs, from_dense, run() (f2c_ranges between the levels) and
    get_results() (f2c_fuse), each a call of its own on the caller's stream; the delay is armed again before run()."""
    rs = env.rs
    raw = _f2c_raw(C_, elem)
    ref = env.ref(("f2c_oracle", C_, elem), lambda: env.o.fine_to_coarse_run(raw.astype(F), -1.0, 1.0, 12, is_u8=elem == "u8"))
    with env.h.scenario(kind) as sc:
        f2c = rs.FineToCoarse(raw, -1.0, 1.0, 12, ctx=env.ctx)
        armed(env, sc, f2c)
        f2c.run()
        got = [c.results() for c in f2c.m_computers]
        valids = [host(c.get_valid_depths_mask_s_v_u()) for c in f2c.m_computers]
        armed(env, sc)
        out_map, out_valid = f2c.get_results()
        om, ov = host(out_map), host(out_valid)
    assert [(c.m_epis.V, c.m_epis.U) for c in f2c.m_computers] == ref["dims"] and len(ref["dims"]) == 2
    for p_, (g, lv) in enumerate(zip(got, ref["levels"])):
        for k in ("edge_mask", "edge_confidence", "depth", "scan_mask", "rbar"):
            assert_same(g[k], getattr(lv, k), "FineToCoarse %s level %d %s in %s" % (elem, p_, k, kind))
        assert_close(g["disp_confidence"], lv.disp_confidence, TOL_CD, "FineToCoarse level %d C_d" % p_)
        assert_same(valids[p_], ref["valids"][p_], "FineToCoarse level %d valid" % p_)
    assert_same(om, ref["fused_map"], "FineToCoarse fused map in " + kind)
    assert_same(ov, ref["fused_valid"], "FineToCoarse fused validity in " + kind)
    scrub(f2c, out_map, out_valid)


# ---- stand-alone helpers: the oracle's ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("elem,C_", [("f32", 1), ("u8", 3), ("u16", 1)])
def test_downsample_epis(env, kind, elem, C_):
    """downsample_EPIs f32 / u8 / u16 of a level produced late: two dependent launches through the shared scratch."""
    rs = env.rs
    V, S, U = 17, 3, 23
    rng = np.random.default_rng(V + U + C_)
    if elem == "f32":
        raw = rng.uniform(0, 250, size=(V, S, U, C_)).astype(F)
        want = env.ref(("down", elem), lambda: env.o.downsample_epis(raw))
        poison = 100.0
    elif elem == "u8":
        raw = rng.integers(0, 256, size=(V, S, U, C_)).astype(F)
        want = env.ref(("down", elem), lambda: env.o.downsample_epis_u8(raw))
        poison = sh.POISON_LEVEL_U8
    else:
        from tests.test_gpu_u16 import downsample_u16_np
        raw = rng.integers(0, 65536, size=(V, S, U, C_)).astype(F)
        want = env.ref(("down", elem), lambda: downsample_u16_np(raw))
        poison = sh.POISON_LEVEL_U16
    late = Late(raw, poison)
    with env.h.scenario(kind) as sc:
        out = rs.downsample_EPIs(sc.produce(late), env.ctx, dtype={"f32": np.float32, "u8": np.uint8, "u16": np.uint16}[elem])
        got = host(out)
    assert_same(got, want, "downsample %s in %s" % (elem, kind))
    scrub(out)


def test_device_max(env, kind):
    """rslf_device_max_f32: a launch, a download and a wait."""
    rs, L = env.rs, env.L
    rng = np.random.default_rng(5)
    a = rng.uniform(0, 250, size=(70001,)).astype(F)
    late = Late(a, 100.0)
    mx = C.c_float(-1.0)
    with env.h.scenario(kind) as sc:
        x = sc.produce(late)
        env.ctx.use_current_stream()
        rs.check(L.rslf_device_max_f32(env.ctx._h, ptr(x), a.size, C.byref(mx)), "rslf_device_max_f32")
    assert mx.value == float(a.max())


def test_f2c_ranges_and_fuse(env, kind):
    """f2c_ranges (rslf_f2c_tighten_bounds; the range planes are made by the wrapper under the caller's stream) and f2c_fuse
    over three levels, inputs produced late."""
    rs = env.rs
    rng = np.random.default_rng(4)
    S, Vu, Uu = 3, 16, 30
    dep = rng.uniform(-2, 2, size=(S, Vu, Uu)).astype(F)
    m = (rng.uniform(size=(S, Vu, Uu)) < 0.7).astype(np.uint8) * 255
    Vd, Ud = 8, 15
    wlo, whi = env.ref(("tighten",), lambda: env.o.f2c_tighten_bounds(dep, m, np.full((S, Vd, Ud), -3, F), np.full((S, Vd, Ud), 3, F)))
    lates = [Late(dep, sh.POISON_DEPTH), Late(m, sh.POISON_MASK)]
    with env.h.scenario(kind) as sc:
        tdep, tm = sc.produce(*lates)
        lo, hi = rs.f2c_ranges(env.ctx, tdep, tm, Vd, Ud, -3.0, 3.0)
        glo, ghi = host(lo), host(hi)
    assert_same(glo, wlo, "tightened dmin in " + kind)
    assert_same(ghi, whi, "tightened dmax in " + kind)
    scrub(lo, hi)

    dims = ((17, 23), (8, 12), (4, 6))
    d = [rng.uniform(-2, 2, size=(S,) + x).astype(F) for x in dims]
    v = [(rng.uniform(size=(S,) + x) > 0.5).astype(np.uint8) * 255 for x in dims]

    def make():
        pairs = [env.o.f2c_fuse([x[s] for x in d], [x[s] for x in v]) for s in range(S)]
        return np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
    wm, wv = env.ref(("fuse",), make)
    Ld, Lv = [Late(x, sh.POISON_DEPTH) for x in d], [Late(x, sh.POISON_MASK) for x in v]
    with env.h.scenario(kind) as sc:
        om, ov = rs.f2c_fuse(env.ctx, list(sc.produce(*Ld)), list(sc.produce(*Lv)))
        gm, gv = host(om), host(ov)
    assert_same(gm, wm, "fused map in " + kind)
    assert_same(gv, wv, "fused validity in " + kind)
    scrub(om, ov)


@pytest.mark.parametrize("size", [5, 15])
def test_selective_median(env, kind, size):
    """selective_median_filter at 5 and 15 (the two kernel forms) on planes produced late."""
    rs = env.rs
    rng = np.random.default_rng(size)
    V, S, U = 9, 3, 70
    vol = rng.uniform(0, 1, size=(V, S, U, 1)).astype(F)
    src = rng.uniform(-1, 1, size=(V, U)).astype(F)
    mask = (rng.uniform(size=(V, U)) < 0.8).astype(np.uint8) * 255
    want = env.ref(("median", size), lambda: env.o.selective_median(src, vol, 1, mask, size, F(0.1)))
    L_vol, lates = Late(vol, sh.POISON_RADIANCE), [Late(src, sh.POISON_DEPTH), Late(mask, sh.POISON_MASK)]
    with env.h.scenario(kind) as sc:
        v = rs.Volume.from_dense(sc.produce(L_vol), 1.0, env.ctx)
        armed(env, sc)
        tsrc, tmask = sc.produce(*lates)
        out = rs.selective_median_filter(tsrc, v, 1, size, tmask, 0.1)
        got = host(out)
    assert_same(got, want, "selective median %d in %s" % (size, kind))
    scrub(out)


# ---- score rows, peaks, sub-grid -------------------------------------------------------------------------------------------------

def fresh(env, sc, *lates):
    """Device inputs for the NEXT call of a case that makes several: the delay armed again, then the inputs produced."""
    env.h.side.synchronize()
    sc.arm()
    return sc.produce(*lates)


def test_score_rows_and_peaks(env, kind):
    """compute_1D_depth_scores, score_peaks on its rows, compute_1D_depth_peaks (the rows through the staging buffer), and the
    two host forms with poisoned host planes: tests/test_gpu_scores.py's smallest register case against oracle_np's rows and
    tests/peaks_ref.py."""
    import tests.test_gpu_peaks as tgp
    import tests.test_gpu_scores as tgs
    torch, rs, L, ctx = env.torch, env.rs, env.L, env.ctx
    i = 1
    C_, S, U, D, V = tgs.CASES[i][:5]
    s_hat = S // 2
    vol, mask = tgs.volume(i), tgs.edge_mask(env.o, i, s_hat)
    rows = tgs.reference(env.o, i, s_hat)                              # FILL at unmasked pixels
    want_pk = env.ref(("peaks", i), lambda: tgp.reference_planes(rows, mask, tgs.DMIN, tgs.DMAX))
    NAMES = tgp.NAMES
    L_vol, L_mask = Late(vol, sh.POISON_RADIANCE), [Late(mask, sh.POISON_MASK) for _ in range(3)]
    out_rows = torch.full((V, U, D), tgs.FILL, dtype=torch.float32, device="cuda")
    out_a, out_b = tgp.filled(rs, torch, V, U), tgp.filled(rs, torch, V, U)
    h_rows = sh.host_poison((V, U, D), F, tgs.FILL)
    h_pk = [sh.host_poison((V, U), np.int32 if n.endswith("idx") else F, tgp.FILL_I if n.endswith("idx") else tgp.FILL_F) for n in NAMES]
    p, st = rs.Depth1DParameters().to_c(), env._lib.RslfStats()
    with env.h.scenario(kind) as sc:
        v = rs.Volume.from_dense(sc.produce(L_vol), 1.0, ctx)
        rs.compute_1D_depth_scores(v, tgs.DMIN, tgs.DMAX, D, s_hat, None, fresh(env, sc, L_mask[0]), 0, None, out_rows)
        rs.score_peaks(out_rows, tgs.DMIN, tgs.DMAX, L_mask[0].t, 0, out_a, ctx)      # the rows' consumer, on the same stream
        got_rows, got_a = host(out_rows), {n: host(t) for n, t in zip(NAMES, out_a)}
        rs.compute_1D_depth_peaks(v, tgs.DMIN, tgs.DMAX, D, s_hat, None, fresh(env, sc, L_mask[1]), out=out_b)
        got_b = {n: host(t) for n, t in zip(NAMES, out_b)}
        fresh(env, sc)
        ctx.use_current_stream()
        rs.check(tgs._c_call(L, "rslf_depth_epi_scores_host", ctx, v, None, None, D, s_hat, p, mask.ctypes.data, 0, V, h_rows.ctypes.data, st),
                 "rslf_depth_epi_scores_host")
        got_h_rows = h_rows.copy()
        fresh(env, sc)
        rs.check(tgp._c_call(L, "rslf_depth_epi_peaks_host", ctx, v, None, None, D, s_hat, p, mask.ctypes.data, 0, V, tgp._c_peaks(h_pk), st),
                 "rslf_depth_epi_peaks_host")
        got_h_pk = {n: a.copy() for n, a in zip(NAMES, h_pk)}
    tgs.assert_rows_equal(got_rows, rows, mask, "score rows in " + kind)
    tgp.assert_planes_equal(got_a, want_pk, "score_peaks in " + kind)
    tgp.assert_planes_equal(got_b, want_pk, "compute_1D_depth_peaks in " + kind)
    tgs.assert_rows_equal(got_h_rows, tgs.reference(env.o, i, s_hat, fill=0.0), mask, "score rows, host form, in " + kind)
    want_host = {n: np.where(mask != 0, want_pk[n], -1 if n.endswith("idx") else 0).astype(want_pk[n].dtype) for n in NAMES}
    tgp.assert_planes_equal(got_h_pk, want_host, "peaks, host form, in " + kind)
    assert st.pixels_scanned == int((mask != 0).sum())


def test_subgrid_refine(env, kind):
    """subgrid_refine on an arg-max plane produced late (poison -1: a refinement that read it refines nothing)."""
    import subgrid_ref as sr
    from oracle import oracle_np as onp
    rs = env.rs
    V, S, U, D = 6, 9, 96, 9
    vol = field(V, S, U, 1, seed=15)
    run = env.ref(("pile_sub",), lambda: sr.pile_run(vol, F(-1), F(1), D))
    idx = np.ascontiguousarray(run["idx"])
    want = env.ref(("refine",), lambda: sr.refine(vol, idx, F(-1), F(1), D, S // 2, onp.default_params()))
    L_vol, L_idx = Late(vol, sh.POISON_RADIANCE), Late(idx, sh.POISON_INDEX)
    with env.h.scenario(kind) as sc:
        v = rs.Volume.from_dense(sc.produce(L_vol), 1.0, env.ctx)
        out = rs.subgrid_refine(v, -1.0, 1.0, D, S // 2, fresh(env, sc, L_idx))
        got = [host(t) for t in out]
    for name, g, w in zip(("disp", "left", "right"), got, want):
        assert_same(g, w, "subgrid_refine %s in %s" % (name, kind))
    assert (idx >= 0).sum() > 100
    scrub(list(out))


# ---- kept runs and their getters -------------------------------------------------------------------------------------------------

KEPT_D = 9
KEPT_TOL = float(F(2.0 / (KEPT_D - 1)))
KEPT = {"plain": dict(), "peaks_uniqueness": dict(peaks=True, uniqueness_ratio=0.7), "consistency_gate": dict(consistency_min_agree=2),
        "derivative_channels": dict(derivative_channels=4.0)}


def _kept_ref(env, variant):
    import derivative_ref as dr
    import f2c_consistency_ref as fcr
    raw = _f2c_raw(1, "f32")

    def make():
        x = raw
        if variant == "derivative_channels":
            x = dr.augment(raw[..., 0], 4.0)
        return fcr.fine_to_coarse(env.o, x.astype(F), -1.0, 1.0, KEPT_D, None, ratio=0.7 if variant == "peaks_uniqueness" else 0.0,
                                  min_agree=2 if variant == "consistency_gate" else 0, tol=KEPT_TOL)
    return raw, env.ref(("kept", variant), make)


@pytest.mark.parametrize("variant", list(KEPT))
def test_kept_run_planes(env, kind, variant):
    """fine_to_coarse_run_host(keep=True): plain, with peaks and validity by uniqueness, with the consistency gate, with
    derivative channels.  Every kept plane through rslf_f2c_run_copy on the caller's stream."""
    rs = env.rs
    raw, ref = _kept_ref(env, variant)
    with env.h.scenario(kind) as sc:
        kept = rs.fine_to_coarse_run_host(epis_of(raw), -1.0, 1.0, KEPT_D, ctx=env.ctx, keep=True, **KEPT[variant])
        fresh(env, sc)
        names = ["depth", "valid", "Ce", "Cd"] + (["pk_idx", "pk_score", "pk_runner_idx", "pk_runner_score"] if kept.peaks else [])
        planes = [{k: kept.plane(l, k) for k in names} for l in range(kept.n_levels)]
        fused = kept.get_results()
        gate = [kept.get_gate_counts(l) if ref["levels"][l]["cs_agree"] is not None else None for l in range(kept.n_levels)] \
            if variant == "consistency_gate" else []
        got = [{k: host(t) for k, t in lv.items()} for lv in planes]
        got_fused = [host(t) for t in fused]
        got_gate = [None if g is None else [host(t) for t in g] for g in gate]
    label = "kept %s in %s" % (variant, kind)
    assert kept.dims == ref["dims"] and kept.n_levels == 2, (kept.dims, ref["dims"])
    for l, lv in enumerate(ref["levels"]):
        for k, r in (("depth", "depth"), ("valid", "valid"), ("Ce", "edge_confidence")):
            assert_same(got[l][k], lv[r], "%s: level %d %s" % (label, l, k))
        assert_close(got[l]["Cd"], lv["disp_confidence"], TOL_CD, "%s: level %d C_d" % (label, l))
        if kept.peaks:
            for k in ("idx", "score", "runner_idx", "runner_score"):
                assert_same(got[l]["pk_" + k], lv["pk"][k], "%s: level %d peaks.%s" % (label, l, k))
        if variant == "consistency_gate" and lv["cs_agree"] is not None:
            assert_same(got_gate[l][0], lv["cs_agree"], "%s: level %d gate agree" % (label, l))
            assert_same(got_gate[l][1], lv["cs_seen"], "%s: level %d gate seen" % (label, l))
            assert kept.inconsistent(l) == lv["inconsistent"]
    assert_same(got_fused[0], ref["fused_map"], label + ": fused map")
    assert_same(got_fused[1], ref["fused_valid"], label + ": fused validity")
    if variant == "consistency_gate":
        assert sum(lv["inconsistent"] for lv in ref["levels"]) > 0
    scrub(planes, list(fused), gate)
    env.torch.cuda.synchronize()
    kept.close()


def test_kept_run_getters(env, kind):
    """On a kept run: rslf_f2c_run_copy in both forms (stream_ctx given and NULL), the three renderers on the device and on
    the host, rslf_f2c_run_consistency(_host), rslf_f2c_run_view_warp(_host), rslf_f2c_run_novel_view(_host).  The yardsticks
    read the planes of the numpy pyramid, never the library's."""
    import consistency_ref as cr
    import f2c_keep_ref as kr
    import novel_view_ref as nvr
    import view_warp_ref as vwr
    torch, rs, L, ctx = env.torch, env.rs, env.L, env.ctx
    raw, ref = _kept_ref(env, "plain")
    lut = rs.colormap_jet()
    table = lut.ctypes.data_as(C.c_void_p)
    level = float(F(env.o.default_params().shadow_level))
    depths, valids = [lv["depth"] for lv in ref["levels"]], [lv["valid"] for lv in ref["levels"]]
    S = raw.shape[1]
    targets, exclude = (0.0, 2.0, 3.5), (0, 2, -1)

    def make():
        pics = {sat: kr.pictures(depths, valids, ref["fused_map"], ref["fused_valid"], lut, ref["volumes"], level, sat, -1, -1) for sat in (True, False)}
        cons = cr.consistency(ref["fused_map"], ref["fused_valid"], 1.0, KEPT_TOL, 0, 1)
        warp = vwr.warp(ref["fused_map"], ref["fused_valid"], 1.0, targets, exclude, 0, 1, ref["volumes"][0])
        novel = nvr.novel(ref["fused_map"], ref["fused_valid"], 1.0, targets, exclude, 0, 1, 0, 4, np.inf, ref["volumes"][0])
        return pics, cons, warp, novel
    pics, cons, warp, novel = env.ref(("kept_getters",), make)
    V0, U0 = ref["dims"][0]
    c_t, c_ex = (C.c_float * 3)(*targets), (C.c_int * 3)(*exclude)
    with env.h.scenario(kind) as sc:
        kept = rs.fine_to_coarse_run_host(epis_of(raw), -1.0, 1.0, KEPT_D, ctx=ctx, keep=True)
        # -- rslf_f2c_run_copy: stream_ctx given (device and host destination), stream_ctx NULL (the null stream's form)
        fresh(env, sc)
        d_given = kept.plane(1, "depth")
        h_given = sh.host_poison((S,) + ref["dims"][1], F, 0.0)
        rs.check(L.rslf_f2c_run_copy(kept._h, 1, 0, hptr(h_given), 1, ctx._h), "rslf_f2c_run_copy")
        h_given = h_given.copy()
        h_null, d_null = sh.host_poison((S, V0, U0), F, 0.0), torch.zeros((S, V0, U0), dtype=torch.float32, device="cuda")
        rs.check(L.rslf_f2c_run_copy(kept._h, 0, 5, hptr(h_null), 1, None), "rslf_f2c_run_copy")      # fused map, to the host
        rs.check(L.rslf_f2c_run_copy(kept._h, 0, 5, ptr(d_null), 0, None), "rslf_f2c_run_copy")       # ... and to the device
        h_null, got_d_null, got_d_given = h_null.copy(), host(d_null), host(d_given)
        # -- the renderers, device then host
        fresh(env, sc)
        maps = {sat: kept.get_coloured_depth_maps(lut, sat) for sat in (True, False)}
        dpyr, epyr = kept.get_coloured_depth_pyr(-1, lut, True), kept.get_coloured_epi_pyr(-1, lut, True)
        got_maps, got_dpyr, got_epyr = {s_: host(t) for s_, t in maps.items()}, [host(t) for t in dpyr], [host(t) for t in epyr]
        fresh(env, sc)
        ctx.use_current_stream()
        h_maps = sh.host_poison((S, V0, U0, 3), np.uint8, 0)
        rs.check(L.rslf_f2c_run_render_depth_maps_host(kept._h, ctx._h, 1, table, hptr(h_maps)), "rslf_f2c_run_render_depth_maps_host")
        h_dpyr = [sh.host_poison(d + (3,), np.uint8, 0) for d in ref["dims"]]
        h_epyr = [sh.host_poison((S, u, 3), np.uint8, 0) for _, u in ref["dims"]]
        rs.check(L.rslf_f2c_run_render_depth_pyr_host(kept._h, ctx._h, -1, 1, table, (C.c_void_p * 2)(*[a.ctypes.data for a in h_dpyr])),
                 "rslf_f2c_run_render_depth_pyr_host")
        rs.check(L.rslf_f2c_run_render_epi_pyr_host(kept._h, ctx._h, -1, 1, table, (C.c_void_p * 2)(*[a.ctypes.data for a in h_epyr])),
                 "rslf_f2c_run_render_epi_pyr_host")
        h_maps, h_dpyr, h_epyr = h_maps.copy(), [a.copy() for a in h_dpyr], [a.copy() for a in h_epyr]
        # -- consistency, view warp, novel view: device forms
        fresh(env, sc)
        d_cons = kept.get_consistency(0, True, KEPT_TOL, 0, 1)
        d_warp = kept.get_warped_views(targets, exclude=exclude, count=True)
        d_novel = kept.get_novel_views(targets, exclude=exclude, tol=float("inf"))
        got_cons = {k: host(t) for k, t in d_cons._asdict().items()}
        got_warp = {k: host(t) for k, t in d_warp._asdict().items() if t is not None}
        got_novel = {k: host(t) for k, t in d_novel._asdict().items() if t is not None}
        # -- ... and the host forms
        fresh(env, sc)
        ctx.use_current_stream()
        n = (S, V0, U0)
        hc = {k: sh.host_poison(n, np.int32, -1) for k in ("seen", "agree", "above", "below")}
        hc["fused"], hc["valid"] = sh.host_poison(n, F, 0.0), sh.host_poison(n, np.uint8, 0)
        counts = env._lib.RslfViewCounts(*[hc[k].ctypes.data for k in ("seen", "agree", "above", "below")])
        rs.check(L.rslf_f2c_run_consistency_host(kept._h, ctx._h, 0, 1, KEPT_TOL, 0, 1, C.byref(counts), hptr(hc["fused"]), hptr(hc["valid"])),
                 "rslf_f2c_run_consistency_host")
        t3 = (3, V0, U0)
        hw = dict(hit=sh.host_poison(t3, np.uint8, 0), depth=sh.host_poison(t3, F, 0.0), src_view=sh.host_poison(t3, np.int32, -1),
                  src_col=sh.host_poison(t3, np.int32, -1), count=sh.host_poison(t3, np.int32, -1), colour=sh.host_poison(t3 + (1,), F, 0.0))
        w_out = env._lib.RslfViewWarpOut(*[hw[k].ctypes.data for k in ("hit", "depth", "src_view", "src_col", "count", "colour")], None, None, None)
        rs.check(L.rslf_f2c_run_view_warp_host(kept._h, ctx._h, 0, 1, c_t, c_ex, 3, 0, 1, C.byref(w_out)), "rslf_f2c_run_view_warp_host")
        hn = dict(colour=sh.host_poison(t3 + (1,), F, 0.0), depth=sh.host_poison(t3, F, 0.0), fill=sh.host_poison(t3, np.uint8, 0),
                  n_src=sh.host_poison(t3, np.int32, -1))
        n_par = env._lib.RslfNovelViewParams(0, 1, 0, 4, float("inf"))
        n_out = env._lib.RslfNovelViewOut(*[hn[k].ctypes.data for k in ("colour", "depth", "fill", "n_src")], None, None, None)
        rs.check(L.rslf_f2c_run_novel_view_host(kept._h, ctx._h, 0, 1, c_t, c_ex, 3, C.byref(n_par), C.byref(n_out)), "rslf_f2c_run_novel_view_host")
        hc, hw, hn = ({k: a.copy() for k, a in d.items()} for d in (hc, hw, hn))
    label = "kept getters in " + kind
    assert_same(got_d_given, ref["levels"][1]["depth"], label + ": copy with a context, device")
    assert_same(h_given, ref["levels"][1]["depth"], label + ": copy with a context, host")
    assert_same(h_null, ref["fused_map"], label + ": copy without a context, host")
    assert_same(got_d_null, ref["fused_map"], label + ": copy without a context, device")
    for sat in (True, False):
        assert_same(got_maps[sat], pics[sat]["maps"], "%s: depth maps, saturate=%s" % (label, sat))
    assert_same(h_maps, pics[True]["maps"], label + ": depth maps, host form")
    for l in range(2):
        assert_same(got_dpyr[l], pics[True]["depth_pyr"][l], "%s: depth pyramid %d" % (label, l))
        assert_same(got_epyr[l], pics[True]["epi_pyr"][l], "%s: EPI pyramid %d" % (label, l))
        assert_same(h_dpyr[l], pics[True]["depth_pyr"][l], "%s: depth pyramid %d, host form" % (label, l))
        assert_same(h_epyr[l], pics[True]["epi_pyr"][l], "%s: EPI pyramid %d, host form" % (label, l))
    cr.assert_equal_bitwise(got_cons, cons, label + ": consistency")
    cr.assert_equal_bitwise(hc, cons, label + ": consistency, host form")
    names_w = ("hit", "depth", "src_view", "src_col", "count", "colour")
    vwr.assert_equal(got_warp, warp, label + ": view warp", names_w)
    vwr.assert_equal(hw, warp, label + ": view warp, host form", names_w)
    names_n = ("colour", "depth", "fill", "n_src")
    nvr.assert_equal(got_novel, novel, label + ": novel view", names_n)
    nvr.assert_equal(hn, novel, label + ": novel view, host form", names_n)
    assert warp["hit"].any() and (novel["fill"] > 1).any() and (cons["agree"] > 0).any()
    scrub(d_given, d_null, list(maps.values()), dpyr, epyr, list(d_cons), list(d_warp), list(d_novel))
    torch.cuda.synchronize()
    kept.close()


# ---- stand-alone helpers: the numpy rule files ---------------------------------------------------------------------------------------

def test_line_confidence_pile(env, kind):
    """line_confidence_pile (K7) on caller planes produced late, against tests/line_conf_ref.py."""
    import line_conf_ref as lcr
    torch, rs = env.torch, env.rs
    rng = np.random.default_rng(23)
    S, V, U, s_hat = 5, 4, 70, 2
    Ce = rng.uniform(0, 1, size=(S, V, U)).astype(F)
    K = rng.uniform(0, 1, size=(V, S, U)).astype(F)
    K[:, :, ::9] = 0                                                  # columns nobody scanned: 0 / 0 -> 0
    depth = rng.uniform(-1.5, 1.5, size=(V, U)).astype(F)
    mask = (rng.uniform(size=(V, U)) < 0.8).astype(np.uint8) * 255

    def make():
        Cl = np.full((V, U), -3.0, F)
        lcr.line_confidence_visit(Ce, K, depth, mask, s_hat, Cl)
        return Cl
    want = env.ref(("line_conf",), make)
    lates = [Late(Ce, 0.0), Late(K, 0.0), Late(depth, sh.POISON_DEPTH), Late(mask, sh.POISON_MASK)]
    Cl = torch.full((V, U), -3.0, dtype=torch.float32, device="cuda")
    with env.h.scenario(kind) as sc:
        tCe, tK, tdepth, tmask = sc.produce(*lates)
        rs.line_confidence_pile(env.ctx, s_hat, tCe, tK, tdepth, tmask, Cl)
        got = host(Cl)
    assert_same(got, want, "line_confidence_pile in " + kind)
    assert (want[mask != 0] > 0).any() and (want[mask == 0] == -3.0).all()


def test_view_consistency_warp_and_novel_view(env, kind):
    """view_consistency, view_warp and novel_view, device forms on planes produced late and host forms with poisoned host
    planes, on the planted field of tests/consistency_ref.py (17 views: a batch of eight and a remainder) with a volume."""
    import consistency_ref as cr
    import novel_view_ref as nvr
    import view_warp_ref as vwr
    torch, rs, L, ctx = env.torch, env.rs, env.L, env.ctx
    S, V, U = 17, 2, 37
    depth, valid = cr.planted(S, V, U)
    depth, valid = np.array(depth), np.array(valid)
    rng = np.random.default_rng(41)
    vol = rng.uniform(0, 1, size=(V, S, U, 3)).astype(F)
    targets, exclude = (0.0, 8.0, 11.5), (0, 8, -1)

    def make():
        return (cr.consistency(depth, valid, 1.0, cr.TOL, 4, 2), vwr.warp(depth, valid, 1.0, targets, exclude, 0, 1, vol),
                nvr.novel(depth, valid, 1.0, targets, exclude, 0, 1, 3, 4, 0.1, vol))
    cons, warp, novel = env.ref(("views",), make)
    L_vol = Late(vol, sh.POISON_RADIANCE)
    lates = [[Late(depth, sh.POISON_DEPTH), Late(valid, sh.POISON_MASK)] for _ in range(3)]
    c_t, c_ex = (C.c_float * 3)(*targets), (C.c_int * 3)(*exclude)
    with env.h.scenario(kind) as sc:
        v = rs.Volume.from_dense(sc.produce(L_vol), 1.0, ctx)
        d_cons = rs.view_consistency(ctx, *fresh(env, sc, *lates[0]), 1.0, cr.TOL, 4, 2)
        got_cons = {k: host(t) for k, t in d_cons._asdict().items()}
        d_warp = rs.view_warp(ctx, *fresh(env, sc, *lates[1]), 1.0, targets, exclude, volume=v, count=True)
        got_warp = {k: host(t) for k, t in d_warp._asdict().items() if t is not None}
        d_novel = rs.novel_view(ctx, *fresh(env, sc, *lates[2]), v, 1.0, targets, exclude, max_gap=3, tol=0.1)
        got_novel = {k: host(t) for k, t in d_novel._asdict().items() if t is not None}
        # the host forms
        fresh(env, sc)
        ctx.use_current_stream()
        n, t3 = (S, V, U), (3, V, U)
        hc = {k: sh.host_poison(n, np.int32, -1) for k in ("seen", "agree", "above", "below")}
        hc["fused"], hc["valid"] = sh.host_poison(n, F, 0.0), sh.host_poison(n, np.uint8, 0)
        counts = env._lib.RslfViewCounts(*[hc[k].ctypes.data for k in ("seen", "agree", "above", "below")])
        rs.check(L.rslf_view_consistency_host(ctx._h, hptr(depth), hptr(valid), S, V, U, 1.0, cr.TOL, 4, 2, C.byref(counts), hptr(hc["fused"]),
                                              hptr(hc["valid"])), "rslf_view_consistency_host")
        fresh(env, sc)
        hw = dict(hit=sh.host_poison(t3, np.uint8, 0), depth=sh.host_poison(t3, F, 0.0), src_view=sh.host_poison(t3, np.int32, -1),
                  src_col=sh.host_poison(t3, np.int32, -1), count=sh.host_poison(t3, np.int32, -1), colour=sh.host_poison(t3 + (3,), F, 0.0))
        w_out = env._lib.RslfViewWarpOut(*[hw[k].ctypes.data for k in ("hit", "depth", "src_view", "src_col", "count", "colour")], None, None, None)
        rs.check(L.rslf_view_warp_host(ctx._h, hptr(depth), hptr(valid), S, V, U, 1.0, v._h, c_t, c_ex, 3, 0, 1, C.byref(w_out)), "rslf_view_warp_host")
        fresh(env, sc)
        hn = dict(colour=sh.host_poison(t3 + (3,), F, 0.0), depth=sh.host_poison(t3, F, 0.0), fill=sh.host_poison(t3, np.uint8, 0),
                  n_src=sh.host_poison(t3, np.int32, -1))
        n_par = env._lib.RslfNovelViewParams(0, 1, 3, 4, 0.1)
        n_out = env._lib.RslfNovelViewOut(*[hn[k].ctypes.data for k in ("colour", "depth", "fill", "n_src")], None, None, None)
        rs.check(L.rslf_novel_view_host(ctx._h, hptr(depth), hptr(valid), S, V, U, 1.0, v._h, c_t, c_ex, 3, C.byref(n_par), C.byref(n_out)),
                 "rslf_novel_view_host")
        hc, hw, hn = ({k: a.copy() for k, a in d.items()} for d in (hc, hw, hn))
    label = "in " + kind
    cr.assert_equal_bitwise(got_cons, cons, "view_consistency " + label)
    cr.assert_equal_bitwise(hc, cons, "view_consistency, host form, " + label)
    names_w = ("hit", "depth", "src_view", "src_col", "count", "colour")
    vwr.assert_equal(got_warp, warp, "view_warp " + label, names_w)
    vwr.assert_equal(hw, warp, "view_warp, host form, " + label, names_w)
    names_n = ("colour", "depth", "fill", "n_src")
    nvr.assert_equal(got_novel, novel, "novel_view " + label, names_n)
    nvr.assert_equal(hn, novel, "novel_view, host form, " + label, names_n)
    scrub(list(d_cons), list(d_warp), list(d_novel))


@pytest.mark.parametrize("dilate_kind", [0, 1, 2], ids=["linear", "cubic", "lanczos3"])
def test_dilated_u_and_undilate_u(env, kind, dilate_kind):
    """Volume.dilated_u (three kernels, factor 2) read back through the slab against tests/dilate_ref.py, and undilate_u on
    planes produced late."""
    import dilate_ref as dlr
    from tests.test_gpu_f2c_keep import _read_device
    torch, rs = env.torch, env.rs
    V, S, U, C_ = 3, 5, 70, 1
    vol = field(V, S, U, C_, seed=19)
    want = env.ref(("dilate", dilate_kind), lambda: dlr.dilate(vol, 2, dilate_kind))
    Ud = dlr.dilated_width(U, 2)
    rng = np.random.default_rng(3)
    planes = rng.uniform(-1, 1, size=(4, Ud)).astype(F)
    L_vol, L_planes = Late(vol, sh.POISON_RADIANCE), Late(planes, sh.POISON_DEPTH)
    with env.h.scenario(kind) as sc:
        v = rs.Volume.from_dense(sc.produce(L_vol), 1.0, env.ctx)
        fresh(env, sc)
        wide = v.dilated_u(2, dilate_kind)
        back = rs.undilate_u(env.ctx, sc.produce(L_planes), 2)
        env.h.side.synchronize()
        d = wide.describe()
        slab = _read_device(d.d_base, d.bytes).view(F).reshape(d.V, d.S, d.pitch, d.C)[:, :, :d.U]
        got_back = host(back)
    assert (d.V, d.S, d.U, d.C) == (V, S, Ud, C_)
    assert_same(np.ascontiguousarray(slab), want, "dilated_u kind %d in %s" % (dilate_kind, kind))
    assert_same(got_back, np.ascontiguousarray(planes[:, ::2]), "undilate_u in " + kind)
    scrub(back)


def test_derivative_channels(env, kind):
    """Volume.with_derivative_channels (read back through the slab) and derivative_channels on a dense level produced late
    (rslf_device_max_f32, then the kernel), against tests/derivative_ref.py."""
    import derivative_ref as dr
    from tests.test_gpu_f2c_keep import _read_device
    rs = env.rs
    V, S, U = 7, 5, 70
    vol = field(V, S, U, 1, seed=29)
    raw = (vol * F(200) + F(3)).astype(F)
    want_vol = env.ref(("deriv_vol",), lambda: dr.augment(vol[..., 0], 3.0))
    want_raw = env.ref(("deriv_raw",), lambda: dr.augment(raw[..., 0], 3.0))
    L_vol, L_raw = Late(vol, sh.POISON_RADIANCE), Late(raw, 100.0)
    with env.h.scenario(kind) as sc:
        v = rs.Volume.from_dense(sc.produce(L_vol), 1.0, env.ctx)
        fresh(env, sc)
        v3 = v.with_derivative_channels(3.0)
        out = rs.derivative_channels(env.ctx, sc.produce(L_raw), 3.0)
        got_raw = host(out)
        d = v3.describe()
        slab = _read_device(d.d_base, d.bytes).view(F).reshape(d.V, d.S, d.pitch, d.C)[:, :, :d.U]
    assert_same(np.ascontiguousarray(slab), want_vol, "with_derivative_channels in " + kind)
    assert_same(got_raw, want_raw, "derivative_channels in " + kind)
    scrub(out)


def test_renderers(env, kind):
    """render_fit (FIT_QUANTILE: nine dependent launches and a wait), render_fit_many, render_planes, render_planes_each,
    render_epi_lines and the host forms, each on planes produced late, against tests/render_ref.py."""
    import render_ref as rr
    torch, rs, L, ctx = env.torch, env.rs, env.L, env.ctx
    rng = np.random.default_rng(11)
    n, rows, cols, S = 3, 20, 70, 9
    planes = rng.uniform(-100, 410, size=(n, rows, cols)).astype(F)
    valid = (rng.uniform(size=(n, rows, cols)) < 0.8).astype(np.uint8) * 255
    depth = rng.uniform(-1.5, 1.5, size=(rows, cols)).astype(F)
    lut = rs.colormap_jet()
    table = lut.ctypes.data_as(C.c_void_p)

    def make():
        fits = [rr.fit(planes[k], rs.FIT_QUANTILE, valid[k]) for k in range(n)]
        mm = [rr.fit(planes[k], rs.FIT_MINMAX) for k in range(n)]
        return dict(fits=fits, mm=mm,
                    planes=np.stack([rr.render(planes[k], -100.0, 410.0, rr.AFFINE, lut, valid[k], rr.BLACK) for k in range(n)]),
                    each=np.stack([rr.render(planes[k], mm[k][0], mm[k][1], rr.SHIFT, lut, valid[k], rr.ZERO_VALUE) for k in range(n)]),
                    own=np.stack([rr.render(planes[k], fits[k][0], fits[k][1], rr.AFFINE, lut, valid[k], rr.BLACK) for k in range(n)]),
                    lines=np.stack([rr.epi_lines(depth[v], valid[0][v], S, S // 2, lut) for v in range(rows)]))
    want = env.ref(("render",), make)
    pairs = [[Late(planes, sh.POISON_DEPTH), Late(valid, sh.POISON_MASK)] for _ in range(4)]
    L_depth, L_mask = Late(depth, sh.POISON_DEPTH), Late(valid[0], sh.POISON_MASK)
    with env.h.scenario(kind) as sc:
        x, m = sc.produce(*pairs[0])
        fit1 = rs.render_fit(ctx, x[1], m[1], rs.FIT_QUANTILE)
        x, m = fresh(env, sc, *pairs[1])
        fits = rs.render_fit_many(ctx, x, m, rs.FIT_QUANTILE)
        x, m = fresh(env, sc, *pairs[2])
        pic = rs.render_planes(ctx, x, -100.0, 410.0, rs.RENDER_AFFINE, lut, m, rs.MASK_BLACK)
        got_pic = host(pic)
        x, m = fresh(env, sc, *pairs[3])
        each = rs.render_planes_each(ctx, x, want["mm"], rs.RENDER_SHIFT, lut, m, rs.MASK_ZERO_VALUE)
        got_each = host(each)
        td, tm = fresh(env, sc, L_depth, L_mask)
        lines = rs.render_epi_lines(ctx, td, tm, S, S // 2, 0, rows, lut)
        got_lines = host(lines)
        # the host forms
        fresh(env, sc)
        ctx.use_current_stream()
        h_pic, h_mm = sh.host_poison((n, rows, cols, 3), np.uint8, 0), sh.host_poison((n, 2), np.float64, 0.0)
        rs.check(L.rslf_render_planes_host(ctx._h, hptr(planes), n, rows * cols, rows, cols, cols, hptr(valid), rs.FIT_QUANTILE, -1, 1,
                                           rs.RENDER_AFFINE, table, rs.MASK_BLACK, None, rs.SLICE_VIEW, 0, 0.0, hptr(h_pic),
                                           h_mm.ctypes.data_as(C.POINTER(C.c_double))), "rslf_render_planes_host")
        fresh(env, sc)
        h_lines = sh.host_poison((rows, S, cols, 3), np.uint8, 0)
        rs.check(L.rslf_render_epi_lines_host(ctx._h, hptr(depth), hptr(valid[0]), rows, S, cols, S // 2, 0, rows, table, hptr(h_lines)),
                 "rslf_render_epi_lines_host")
        h_pic, h_mm, h_lines = h_pic.copy(), h_mm.copy(), h_lines.copy()
    assert fit1 == want["fits"][1], (fit1, want["fits"][1])
    assert fits == want["fits"], (fits, want["fits"])
    assert_same(got_pic, want["planes"], "render_planes in " + kind)
    assert_same(got_each, want["each"], "render_planes_each in " + kind)
    assert_same(got_lines, want["lines"], "render_epi_lines in " + kind)
    assert [tuple(r) for r in h_mm.tolist()] == want["fits"], (h_mm, want["fits"])
    assert_same(h_pic, want["own"], "rslf_render_planes_host in " + kind)
    assert_same(h_lines, want["lines"], "rslf_render_epi_lines_host in " + kind)
    scrub(pic, each, lines)


# ---- the default context, moved ----------------------------------------------------------------------------------------------

def test_the_default_context_follows_the_current_stream_there_and_back(env):
    """default_context() carries whatever the rest of the suite left in it.  After side.wait_stream(default) one pile step,
    one sweep and one pyramid run on it under the side stream (the null stream busy), then one of each back on the null
    stream after default.wait_stream(side): all six are the oracle's."""
    torch, rs = env.torch, env.rs
    ctx = rs.default_context(0)
    pile_vol, pile_ref = _pile_ref(env, (6, 9, 96, 1), 12)
    sweep_vol, sweep_planes, _, _ = _sweep_ref(env, SWEEP_SHAPES[0], "off")
    raw, f2c_ref = _f2c_oracle(env, 1, "f32", 0)

    def three(label):
        comp = rs.Depth1DComputer_pile(epis_of(pile_vol), -1.0, 1.0, 12, epi_scale_factor=1.0, ctx=ctx)
        comp.run()
        assert_pile_parity(comp.results(), pile_ref, label=label + " pile")
        sweep = rs.Depth2DComputer(epis_of(sweep_vol), -1.0, 1.0, SWEEP_D, epi_scale_factor=1.0, ctx=ctx)
        sweep.run()
        _sweep_check(sweep.results(), sweep_planes, label + " sweep")
        out = rs.fine_to_coarse_run_host(epis_of(raw), -1.0, 1.0, 12, ctx=ctx)
        assert_same(out["out_map"], f2c_ref["fused_map"], label + " pyramid map")
        assert_same(out["out_valid"], f2c_ref["fused_valid"], label + " pyramid validity")
        scrub(comp, sweep)

    side, null = env.h.side, torch.cuda.default_stream(0)
    side.wait_stream(null)
    with env.h.scenario("busy_default"):
        three("default context on the side stream")
    null.wait_stream(side)
    three("default context back on the null stream")
    torch.cuda.synchronize()
