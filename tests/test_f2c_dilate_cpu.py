"""The level dilation of the pyramid (K18) without a GPU: the union rule as a stand-alone program against numpy bit for
bit, the two kernels' plans replayed under sanitizers, the host entry on padded rows, the point of the feature -- the oracle's
pyramid with dilated sweeps on the small-slope field --, the exports, the Python signatures and the refusals that need no
device."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import dilate_ref as dlr
import f2c_dilate_ref as fdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remotesensingproject_amd", "csrc")
F = np.float32
GXX = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
       "-Wall", "-Wextra", "-Werror", "-I", CSRC]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
INVALID, UNSUPPORTED = -1, -2


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def range_planes(rng, rows, U):
    """dmin <= dmax planes with what the rule must get right: -0.0 beside +0.0 in both orders, equal neighbours, plateaus."""
    lo = np.round(rng.uniform(-1.0, 0.5, (rows, U)) * 8).astype(F) / F(8)
    hi = (lo + np.round(rng.uniform(0.0, 1.0, (rows, U)) * 8).astype(F) / F(8)).astype(F)
    for a in (lo, hi):
        a[:, ::5] = F(-0.0)
        a[:, 1::5] = F(0.0)
        if U > 8:
            a[:, 6] = F(0.0)
            a[:, 7] = F(-0.0)      # ... and +0.0 on the left of -0.0
            a[:, 3] = a[:, 2]      # equal neighbours
    return lo, hi


def test_the_yardstick_by_hand():
    lo, hi = fdr.dilate_ranges(np.array([[-1.0, 0.0, -0.5]], F), np.array([[0.0, 1.0, 0.5]], F), 3)
    assert lo.tolist() == [[-1.0, -1.0, -1.0, 0.0, -0.5, -0.5, -0.5]]
    assert hi.tolist() == [[0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5]]
    z = fdr.dilate_ranges(np.array([-0.0, 0.0, -0.0], F), np.array([0.0, -0.0, 0.0], F), 2)
    assert np.signbit(z[0]).tolist() == [True, True, False, False, True]      # the left neighbour's bits on ties
    assert np.signbit(z[1]).tolist() == [False, False, True, True, False]
    n = fdr.dilate_ranges(np.array([np.nan, 1.0, np.nan], F), np.array([np.nan, 2.0, np.nan], F), 2)
    assert n[0][1] == 1.0 and n[0][3] == 1.0 and n[1][1] == 2.0 and n[1][3] == 2.0   # a NaN loses to a number
    one = fdr.dilate_ranges(np.array([[3.0]], F), np.array([[4.0]], F), 8)
    assert one[0].tolist() == [[3.0]] and one[1].tolist() == [[4.0]]
    p = type("P", (C.Structure,), dict(_fields_=[("slope_factor", C.c_float)]))()
    p.slope_factor = 0.3
    assert fdr.dilated_params(p, 3).slope_factor == F(F(0.3) * F(3)) and p.slope_factor == F(0.3)


def test_the_rule_program_equals_the_numpy_union_rule(tmp_path):
    """csrc/k18_ranges_rule.hpp, compiled alone by g++ into a program with its own main, for U in {1, 2, 3, 63, 64, 65, 130},
    f in 1..8 and 1..5 rows, on planes with -0.0 and equal neighbours: f2c_dilate_ref.dilate_ranges bit for bit."""
    exe = tmp_path / "ranges_rule_main"
    subprocess.run(GXX + [os.path.join(ROOT, "tests", "cpp", "ranges_rule_main.cpp"), "-o", str(exe)], check=True)
    rng = np.random.default_rng(18)
    cases = []
    with open(tmp_path / "cases.bin", "wb") as fh:
        for U in (1, 2, 3, 63, 64, 65, 130):
            for f in range(1, 9):
                rows = 1 + (U + f) % 5
                lo, hi = range_planes(rng, rows, U)
                np.array([f, U, rows], np.int32).tofile(fh)
                lo.tofile(fh)
                hi.tofile(fh)
                cases.append((f, U, rows, lo, hi))
    assert {c[2] for c in cases} == {1, 2, 3, 4, 5}
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ranges rule: %d cases ok" % len(cases) in r.stdout
    got = np.fromfile(tmp_path / "out.bin", F)
    at = 0
    for f, U, rows, lo, hi in cases:
        n = rows * dlr.dilated_width(U, f)
        want_lo, want_hi = fdr.dilate_ranges(lo, hi, f)
        assert np.array_equal(_bits(got[at:at + n]), _bits(want_lo).reshape(-1)), (f, U, rows, "dmin")
        assert np.array_equal(_bits(got[at + n:at + 2 * n]), _bits(want_hi).reshape(-1)), (f, U, rows, "dmax")
        at += 2 * n
    assert at == got.size


def test_the_plans_under_sanitizers(tmp_path):
    exe = tmp_path / "test_plan_level_dilate"
    subprocess.run(GXX + [os.path.join(ROOT, "tests", "cpp", "test_plan_level_dilate.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "level dilate plan tests ok" in r.stdout


NAMES = ("rslf_planes_dilate_ranges_u", "rslf_planes_dilate_ranges_u_host", "rslf_planes_undilate_many_u",
         "rslf_fine_to_coarse_run_host_dl", "rslf_f2c_run_host_dl", "rslf_f2c_run_level_dilation")


def test_the_host_entry_equals_the_rule_on_padded_rows_and_refuses():
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(181)
    for U, f, rows in ((1, 3, 2), (2, 8, 1), (65, 2, 3), (130, 3, 2), (7, 1, 4)):
        lo, hi = range_planes(rng, rows, U)
        Ud = dlr.dilated_width(U, f)
        pad_in, pad_out = np.full((2, rows, U + 3), 77, F), np.full((2, rows, Ud + 5), 99, F)
        pad_in[0, :, :U], pad_in[1, :, :U] = lo, hi
        rc = L.rslf_planes_dilate_ranges_u_host(pad_in[0].ctypes.data, pad_in[1].ctypes.data, (U + 3) * 4, rows, U, f,
                                                pad_out[0].ctypes.data, pad_out[1].ctypes.data, (Ud + 5) * 4)
        assert rc == 0, L.rslf_last_error()
        want = fdr.dilate_ranges(lo, hi, f)
        for k in (0, 1):
            assert np.array_equal(_bits(pad_out[k, :, :Ud]), _bits(want[k])), (U, f, rows, k)
            assert (pad_out[k, :, Ud:] == 99).all()
        dense = np.empty((2, rows, Ud), F)
        assert L.rslf_planes_dilate_ranges_u_host(lo.ctypes.data, hi.ctypes.data, 0, rows, U, f, dense[0].ctypes.data, dense[1].ctypes.data, 0) == 0
        assert np.array_equal(_bits(dense[0]), _bits(want[0])) and np.array_equal(_bits(dense[1]), _bits(want[1]))
    a, b = np.zeros((2, 5), F), np.zeros((2, 5), F)
    x, y = np.zeros((2, 9), F), np.zeros((2, 9), F)
    A, B, X, Y = (t.ctypes.data for t in (a, b, x, y))
    bad = [(None, B, 0, 2, 5, 2, X, Y, 0), (A, None, 0, 2, 5, 2, X, Y, 0), (A, B, 0, 2, 5, 2, None, Y, 0), (A, B, 0, 2, 5, 2, X, None, 0),
           (A, B, 0, 2, 5, 2, A, Y, 0), (A, B, 0, 2, 5, 2, X, B, 0), (A, B, 0, 2, 5, 2, X, X, 0),
           (A, B, 0, 2, 5, 0, X, Y, 0), (A, B, 0, 2, 5, 9, X, Y, 0), (A, B, 0, 2, 0, 2, X, Y, 0),
           (A, B, 16, 2, 5, 2, X, Y, 0), (A, B, 0, 2, 5, 2, X, Y, 32), (A, B, 22, 2, 5, 2, X, Y, 0)]
    for args in bad:
        assert L.rslf_planes_dilate_ranges_u_host(*args) == INVALID, args
        assert L.rslf_last_error()
    # the device entries, refused before a device is touched
    assert L.rslf_planes_dilate_ranges_u(None, A, B, 2, 5, 2, X, Y) == INVALID
    ptr = (C.c_void_p * 1)(A)
    out = (C.c_void_p * 1)(X)
    four = (C.c_int * 1)(4)
    assert L.rslf_planes_undilate_many_u(None, ptr, out, four, 1, 2, 9, 2) == INVALID
    assert L.rslf_planes_undilate_many_u(None, None, None, None, 1, 2, 9, 2) == INVALID


def test_the_library_exports_the_entries_and_the_version_stays():
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "rslf_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and getattr(L, name) is not None and "int %s(" % name in header
    assert _lib.ABI_VERSION == 6 and L.rslf_abi_version() == 6
    f, k = C.c_int(-3), C.c_int(-3)
    assert L.rslf_f2c_run_level_dilation(None, C.byref(f), C.byref(k)) == 0 and (f.value, k.value) == (1, 1)
    assert L.rslf_f2c_run_level_dilation(None, None, None) == 0


def _refused(L, entry, args, status, words):
    rc = getattr(L, entry)(*args)
    assert rc == status, (entry, rc, L.rslf_last_error())
    msg = L.rslf_last_error().decode()
    for w in words:
        assert w in msg, (entry, msg)


def test_the_c_entries_refuse_by_name_before_a_device_is_touched():
    """No context is ever made here: the refusals come before the device is looked at."""
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd import depth as rs
    L = _lib.lib()
    epi = np.zeros((3, 12), F)
    ptrs = (C.c_void_p * 12)(*[epi.ctypes.data] * 12)
    p, st, nl, h = rs.Depth1DParameters().to_c(), _lib.RslfStats(), C.c_int(), C.c_void_p()
    ctx = C.c_void_p(8)   # never dereferenced by the refusals below
    m, v = np.zeros((3, 12, 12), F), np.zeros((3, 12, 12), np.uint8)

    def host(line_mode, dl, kind):
        return (ctx, ptrs, 0, 12, 3, 12, 1, 0, -1.0, 1.0, 9, -1.0, C.byref(p), -1, 1, m.ctypes.data, v.ctypes.data, C.byref(nl), C.byref(st),
                line_mode, None, 0, 0.0, dl, kind)

    def kept(line_mode, dl, kind):
        return (ctx, ptrs, 0, 12, 3, 12, 1, 0, -1.0, 1.0, 9, -1.0, C.byref(p), -1, 1, line_mode, 0, 0, C.byref(h), C.byref(st), 0, 0, 0.0, 0.0,
                0.0, 0, 0, 0.0, dl, kind)
    for entry, make in (("rslf_fine_to_coarse_run_host_dl", host), ("rslf_f2c_run_host_dl", kept)):
        for dl in (0, 9, -1):
            _refused(L, entry, make(0, dl, 1), INVALID, ["level_dilation=%d" % dl])
        for kind in (-1, 3):
            _refused(L, entry, make(0, 2, kind), INVALID, ["dilation_kind=%d" % kind])
        _refused(L, entry, make(0, 1, 7), INVALID, ["dilation_kind=7"])       # the kind is checked at factor 1 too
        for mode in (1, 2):
            _refused(L, entry, make(mode, 2, 1), UNSUPPORTED, ["level_dilation=2", "line confidence mode %d" % mode])
    assert not h.value


def test_the_units_are_registered_and_the_rule_has_no_hip():
    from remotesensingproject_amd import build
    for hdr in ("k18_level_dilate.hpp", "k18_ranges_rule.hpp", "rslf_plan_level_dilate.hpp"):
        assert hdr in build.UNITS["rslf_dilate.hip"] and os.path.exists(os.path.join(CSRC, hdr))
    rule = open(os.path.join(CSRC, "k18_ranges_rule.hpp")).read()
    plan = open(os.path.join(CSRC, "rslf_plan_level_dilate.hpp")).read()
    assert "hip/" not in rule and "hip/" not in plan and '#include "k18_ranges_rule.hpp"' in plan
    kern = open(os.path.join(CSRC, "k18_level_dilate.hpp")).read()
    assert "__shared__" not in kern and "asm" not in kern


def test_the_python_signatures_and_the_refusals():
    from remotesensingproject_amd import depth as rs
    from remotesensingproject_amd import sharding
    for fn in (rs.fine_to_coarse_run_host, rs.FineToCoarse.__init__):
        sig = inspect.signature(fn).parameters
        for name, default in (("level_dilation", 1), ("level_dilation_kind", rs.DILATE_CUBIC)):
            assert sig[name].default == default and sig[name].kind is inspect.Parameter.KEYWORD_ONLY, (fn, name)
        assert sig["u_dilation"].default == 1
    assert list(inspect.signature(rs.dilate_ranges_u).parameters) == ["ctx", "dmin", "dmax", "factor"]
    assert list(inspect.signature(rs.undilate_many_u).parameters) == ["ctx", "planes", "factor"]
    for fn in (rs.MultiDevice.fine_to_coarse, sharding.ShardedFineToCoarse.__init__):
        sig = inspect.signature(fn).parameters
        assert sig["level_dilation"].default == 1 and sig["level_dilation"].kind is inspect.Parameter.KEYWORD_ONLY
    # u_dilation is still refused on the pyramid forms, with the message it had
    for call in (lambda: rs.FineToCoarse(None, -1.0, 1.0, 8, u_dilation=2), lambda: rs.fine_to_coarse_run_host(None, -1.0, 1.0, 8, u_dilation=2)):
        with pytest.raises(ValueError, match="u_dilation=2 is not built here"):
            call()
    # factors and kinds that are none
    forms = (lambda **kw: rs.fine_to_coarse_run_host(None, -1.0, 1.0, 8, **kw), lambda **kw: rs.fine_to_coarse_run_host(None, -1.0, 1.0, 8, keep=True, **kw),
             lambda **kw: rs.FineToCoarse(None, -1.0, 1.0, 8, **kw))
    for form in forms:
        for bad in (0, 9, -2, 1.5, True, "2"):
            with pytest.raises(ValueError, match="level_dilation"):
                form(level_dilation=bad)
        for bad in (3, -1, None, True):
            with pytest.raises(ValueError, match="level_dilation_kind"):
                form(level_dilation=2, level_dilation_kind=bad)
    # a line mode together with the dilation: both named
    for mode in (rs.LINE_CONF_AS_BUILT, rs.LINE_CONF_GATE):
        with pytest.raises(ValueError, match="line confidence mode %d together with level_dilation=2" % mode):
            rs.fine_to_coarse_run_host(None, -1.0, 1.0, 8, line_mode=mode, level_dilation=2)
        with pytest.raises(ValueError, match="line confidence mode %d together with level_dilation=3" % mode):
            rs.FineToCoarse(None, -1.0, 1.0, 8, line_confidence_mode=mode, level_dilation=3)
    # the forms that have none refuse it by name
    md = object.__new__(rs.MultiDevice)
    with pytest.raises(ValueError, match="MultiDevice.fine_to_coarse: level_dilation=2 is not built here"):
        md.fine_to_coarse(None, -1.0, 1.0, 8, level_dilation=2)
    with pytest.raises(ValueError, match="ShardedFineToCoarse: level_dilation=4 is not built here"):
        sharding.ShardedFineToCoarse(None, -1.0, 1.0, 8, 0, 1, level_dilation=4)
    with pytest.raises(ValueError, match="float32 CUDA"):
        rs.dilate_ranges_u(None, np.zeros(3), np.zeros(3), 2)
    assert callable(getattr(rs.KeptFineToCoarse, "describe"))


# ---- the point of the feature --------------------------------------------------------------------------------------

def field_run(oracle_mod, vol, delta, f, kind):
    p = oracle_mod.default_params()
    r = fdr.fine_to_coarse(oracle_mod, vol, fdr.FIELD_DMIN, fdr.FIELD_DMAX, fdr.FIELD_D, f, kind, p, accept_all_last_scale=True)
    assert r["dims"] == [(24, 96), (12, 48)]
    return fdr.field_errors(r["fused_map"], r["levels"][0]["depth"], r["levels"][0]["valid"], delta)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_point_of_the_feature(oracle_mod, seed):
    """small_slope_pyramid_field (V = 24, S = 9, U = 96, two levels), 241 hypotheses in [-0.6, 0.6], default parameters, mode 0,
    accept_all_last_scale, through the oracle: relative to the undilated pyramid, the fused MAE over columns 12 .. 83 is
    <= 0.90 with Lanczos-3 x2, <= 1.00 with cubic x2 and within [0.95, 1.20] with linear x2; level 0's valid-pixel MAE is
    <= 0.85 with Lanczos-3 x2 and <= 0.93 with cubic x2."""
    vol, delta = fdr.small_slope_pyramid_field(seed)
    plain = field_run(oracle_mod, vol, delta, 1, fdr.CUBIC)
    ratios = {}
    for kind in dlr.KINDS:
        got = field_run(oracle_mod, vol, delta, 2, kind)
        ratios[dlr.NAMES[kind]] = (got[0] / plain[0], got[1] / plain[1])
    print("seed %d: plain fused MAE %.5f, level-0 MAE %.5f; (fused, level 0) ratios %s"
          % (seed, plain[0], plain[1], {k: (round(a, 4), round(b, 4)) for k, (a, b) in ratios.items()}))
    assert plain[0] > 0 and plain[1] > 0
    assert ratios["lanczos3"][0] <= 0.90 and ratios["lanczos3"][1] <= 0.85
    assert ratios["cubic"][0] <= 1.00 and ratios["cubic"][1] <= 0.93
    assert 0.95 <= ratios["linear"][0] <= 1.20
