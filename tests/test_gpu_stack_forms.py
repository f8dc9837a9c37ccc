"""The four forms of the three stack operations -- cross-view consistency (K12), the view warp (K14), the novel view (K15):
planes on the device, planes on the host, a kept fine-to-coarse run read in place, and the kept run with its outputs on the
host.  One table: what every form refuses, with which text and in which order, that a refused call leaves the caller's planes
alone, that the host forms refuse an open sweep while the device forms do not, and that all four forms of an operation
compute the same bits, which are the numpy yardsticks' (consistency_ref, view_warp_ref, novel_view_ref).  The numerics of
each operation are the business of its own test file; this one pins what the forms have in common."""
import ctypes as C

import numpy as np
import pytest

import consistency_ref as cr
import novel_view_ref as nr
import view_warp_ref as wr
from test_gpu_view_warp import _field, _slab

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 77
PLANE_FORMS, RUN_FORMS = ("device", "host"), ("run", "run_host")
HOST_OF = {"device": "host", "run": "run_host"}
TARGETS, EXCLUDE = (2.0, 0.0), (2, 0)   # two views, each left out of its own prediction: err and row_err can be asked for


def _warp_shape(k, T, V, U, Cn):
    return (T, V) if k.startswith("row_") else (T, V, U, Cn) if k == "colour" else (T, V, U)


class Op:
    """One operation: its planes, the word its "nothing to compute" refusal counts them with, its arguments, one bad argument
    and the text that names it, the C arguments after the forms' common head, and the yardstick."""

    def __init__(self, name, names, dtypes, word, args, bad, bad_text, takes_volume, tail, ref, assert_equal):
        self.name, self.names, self.dtypes, self.word, self.args = name, names, dtypes, word, args
        self.bad, self.bad_text, self.takes_volume, self.tail, self.ref, self.assert_equal = bad, bad_text, takes_volume, tail, ref, assert_equal

    def entry(self, L, form):
        stem = {"consistency": "consistency", "warp": "view_warp", "novel": "novel_view"}[self.name]
        if form in PLANE_FORMS:
            return getattr(L, "rslf_%s%s%s" % ("view_" if self.name == "consistency" else "", stem, "_host" if form == "host" else ""))
        return getattr(L, "rslf_f2c_run_%s%s" % (stem, "_host" if form == "run_host" else ""))

    def shape(self, k, S, V, U, Cn):
        return (S, V, U) if self.name == "consistency" else _warp_shape(k, len(TARGETS), V, U, Cn)


def _targets():
    return (C.c_float * len(TARGETS))(*TARGETS), (C.c_int * len(EXCLUDE))(*EXCLUDE), len(TARGETS)


def _consistency_tail(a, p):
    from remotesensingproject_amd import _lib
    counts = _lib.RslfViewCounts(*(p.get(k) for k in cr.NAMES[:4]))
    return [a["tol"], a["radius"], a["min_agree"], C.byref(counts), p.get("fused"), p.get("valid")]


def _warp_tail(a, p):
    from remotesensingproject_amd import _lib
    out = _lib.RslfViewWarpOut(*(p.get(k) for k in wr.NAMES))
    return [*_targets(), a["radius"], a["nearer"], C.byref(out)]


def _novel_tail(a, p):
    from remotesensingproject_amd import _lib
    out = _lib.RslfNovelViewOut(*(p.get(k) for k in nr.NAMES))
    par = _lib.RslfNovelViewParams(a["radius"], a["nearer"], a["max_gap"], a["sources"], a["tol"])
    return [*_targets(), C.byref(par), C.byref(out)]


OPS = [
    Op("consistency", cr.NAMES, dict(seen=np.int32, agree=np.int32, above=np.int32, below=np.int32, fused=F, valid=np.uint8), "six",
       dict(tol=cr.TOL, radius=0, min_agree=2), dict(tol=-1.0), "tol=", False, _consistency_tail,
       lambda d, v, slope, slab, a: cr.consistency(d, v, slope, a["tol"], a["radius"], a["min_agree"]), cr.assert_equal_bitwise),
    Op("warp", wr.NAMES, wr.DTYPES, "nine", dict(radius=0, nearer=1), dict(nearer=0), "nearer=0", True, _warp_tail,
       lambda d, v, slope, slab, a: wr.warp(d, v, slope, TARGETS, EXCLUDE, a["radius"], a["nearer"], volume=slab, want_err=True), wr.assert_equal),
    Op("novel", nr.NAMES, nr.DTYPES, "seven", dict(radius=0, nearer=1, max_gap=3, sources=4, tol=0.25), dict(sources=0), "sources=0", True,
       _novel_tail, lambda d, v, slope, slab, a: nr.novel(d, v, slope, TARGETS, EXCLUDE, a["radius"], a["nearer"], a["max_gap"], a["sources"],
                                                          a["tol"], volume=slab, want_err=True), nr.assert_equal),
]


class Env:
    """What the table's rows share, made once: a context, the two planted fields with a volume each, the kept run with and
    without its volumes, and a volume to open a sweep on."""

    def __init__(self, rs):
        import torch
        from remotesensingproject_amd import _lib
        self.rs, self.L, self.ctx = rs, _lib.lib(), rs.Context(0)
        self.fields = {}
        for U in (37, 40):   # the scalar stores and staged planes that start off a 16-byte boundary / the vector stores
            S, V = 5, 3
            depth, valid = cr.planted(S, V, U)
            raw = np.random.RandomState(U).randint(0, 256, (V, S, U)).astype(np.uint8)
            vol = rs.Volume.from_epis(list(raw), ctx=self.ctx)
            self.fields[U] = dict(depth=np.array(depth, F), valid=np.array(valid, np.uint8), vol=vol,   # (copies: planted's are read-only)
                                  slab=wr.normalised(raw[..., None]), dims=(S, V, U))
        lf = _field(S=7, V=40, U=96, seed=5)   # the field of test_gpu_view_warp.py's test_kept_fine_to_coarse_getters
        self.kept = rs.fine_to_coarse_run_host(list(lf[..., 0]), -2.0, 2.0, 17, keep=True)
        self.bare = rs.fine_to_coarse_run_host(list(lf[..., 0]), -2.0, 2.0, 17, keep=True, keep_volumes=False)
        assert self.kept.n_levels >= 2 and self.kept.keep_volumes and not self.bare.keep_volumes
        self.fused = dict(depth=self.kept.plane(0, "fused_map").cpu().numpy(), valid=self.kept.plane(0, "fused_valid").cpu().numpy(),
                          slab=_slab(self.kept.volume_desc(0)))
        self.sweep_dims = (4, 5, 32, 9)   # V, S, U, D
        V, S, U, _ = self.sweep_dims
        self.sweep_vol = rs.Volume.from_dense(np.random.RandomState(3).uniform(0.0, 1.0, (V, S, U)).astype(F), 1.0, self.ctx)
        self.sweep_mask = torch.zeros((S, V, U), dtype=torch.uint8, device="cuda")

    def open_sweep(self):
        V, _, _, D = self.sweep_dims
        assert self.L.rslf_sweep_begin(self.ctx._h, self.sweep_vol._h, C.c_void_p(self.sweep_mask.data_ptr()), None, D, 0, V) == 0

    def close_sweep(self):
        assert self.L.rslf_sweep_end(self.ctx._h, 0, self.sweep_dims[3], None) == 0

    def close(self):
        self.kept.close()
        self.bare.close()


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from remotesensingproject_amd import depth
    e = Env(depth)
    yield e
    e.close()


NO_RUN = object()


def call(env, op, form, want=None, args=None, field=37, run=None, level=0, fused=1):
    """One call of `op` in `form` with exactly the planes of `want` (default: all), each starting from the sentinel, the others
    NULL -> (status, rslf_last_error(), the planes as the call left them).  run: env.kept unless given; NO_RUN: a NULL run."""
    import torch
    want = op.names if want is None else want
    a = dict(op.args, **(args or {}))
    run = env.kept if run is None else run
    on_host = form in ("host", "run_host")
    if form in PLANE_FORMS:
        f = env.fields[field]
        S, V, U = f["dims"]
        Cn = 1
    else:
        dims = env.kept.dims[level if 0 <= level < env.kept.n_levels else 0]
        S, V, U, Cn = env.kept.S, *dims, env.kept.C
    planes = {k: np.full(op.shape(k, S, V, U, Cn), SENTINEL, op.dtypes[k]) for k in want}
    if not on_host:
        planes = {k: torch.from_numpy(p).cuda() for k, p in planes.items()}
    ptrs = {k: (p.ctypes.data if on_host else p.data_ptr()) for k, p in planes.items()}
    env.ctx.use_current_stream()
    if form in PLANE_FORMS:
        d_in, v_in = (f["depth"], f["valid"]) if on_host else (torch.from_numpy(f["depth"]).cuda(), torch.from_numpy(f["valid"]).cuda())
        in_ptr = (lambda x: x.ctypes.data) if on_host else (lambda x: x.data_ptr())
        head = [env.ctx._h, in_ptr(d_in), in_ptr(v_in), S, V, U, 1.0] + ([f["vol"]._h] if op.takes_volume else [])
    else:
        head = [None if run is NO_RUN else run._h, env.ctx._h, level, fused]
    rc = op.entry(env.L, form)(*head, *op.tail(a, ptrs))
    text = env.L.rslf_last_error().decode(errors="replace") if rc else ""
    torch.cuda.synchronize()
    return rc, text, {k: (p if on_host else p.cpu().numpy()) for k, p in planes.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def untouched(planes):
    return all((p == SENTINEL).all() for p in planes.values())


def same_bits(a, b):
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


def refused(env, op, form, text, **kw):
    rc, err, got = call(env, op, form, **kw)
    assert rc == -1 and text in err, (op.name, form, kw, rc, err)
    assert untouched(got), (op.name, form, kw, "a refused call wrote a plane")
    return err


@pytest.mark.parametrize("op", OPS, ids=[o.name for o in OPS])
def test_the_four_forms(env, op):
    # 1-4: what the kept-run forms refuse before they look at the operation's own arguments
    for form in RUN_FORMS:
        refused(env, op, form, "NULL argument", run=NO_RUN)
        for level in (-1, env.kept.n_levels):
            refused(env, op, form, "level", level=level, fused=0)
        refused(env, op, form, "finest size", level=1, fused=1)
        if op.takes_volume:
            refused(env, op, form, "without keep_volumes", run=env.bare, want=("colour",))
    # 6: nothing asked for, in the operation's own words
    for form in PLANE_FORMS + RUN_FORMS:
        refused(env, op, form, "all %s output planes are NULL" % op.word, want=())
    # 5 and 7: a sweep open on the context
    during = {}
    env.open_sweep()
    try:
        for form in HOST_OF.values():
            err = refused(env, op, form, op.bad_text, args=op.bad)   # both fail: the argument is named, so its check comes first
            assert "sweep" not in err, (op.name, form, err)
            refused(env, op, form, "a sweep is open")
        for form in HOST_OF:   # the device forms enqueue and return, sweep or no sweep
            rc, err, during[form] = call(env, op, form)
            assert rc == 0, (op.name, form, err)
    finally:
        env.close_sweep()
    for dev_form, host_form in HOST_OF.items():
        rc, err, got = call(env, op, host_form)
        assert rc == 0, (op.name, host_form, err)
        assert same_bits(got, during[dev_form]), (op.name, host_form, "differs from the device form")
    # 8: after the refusals every form once more, every plane asked for, against one another and against the yardstick
    for field in (37, 40):
        f = env.fields[field]
        ref = op.ref(f["depth"], f["valid"], 1.0, f["slab"], op.args)
        rc, err, dev = call(env, op, "device", field=field)
        assert rc == 0, (op.name, field, err)
        rc, err, host = call(env, op, "host", field=field)
        assert rc == 0, (op.name, field, err)
        assert same_bits(host, dev), (op.name, field, "host and device forms differ")
        op.assert_equal(dev, ref, "%s, U = %d" % (op.name, field))
    ref = op.ref(env.fused["depth"], env.fused["valid"], 1.0, env.fused["slab"], op.args)
    rc, err, dev = call(env, op, "run")
    assert rc == 0, (op.name, err)
    rc, err, host = call(env, op, "run_host")
    assert rc == 0, (op.name, err)
    assert same_bits(host, dev) and same_bits(dev, during["run"]), (op.name, "the kept-run forms differ")
    op.assert_equal(dev, ref, "%s, the kept run's fused planes" % op.name)
