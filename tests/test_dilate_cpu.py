"""The dilation along u without a GPU (K16, rslf_volume_dilate_u): the rule header as a stand-alone C++ program against the
numpy yardstick bit for bit, the plan functions under sanitizers, the point of the feature -- the oracle on dilated small-slope
fields --, the exports, the Python signatures and the refusals that need no device."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import dilate_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remotesensingproject_amd", "csrc")
F = np.float32
GXX = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
       "-Wall", "-Wextra", "-Werror", "-I", CSRC]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def step_field(rng, rows: int, U: int, C: int) -> np.ndarray:
    """[rows, U, C] float32 in [-0.5, 1]: plateaus of 2 .. 6 columns at the two ends of the range or somewhere between, so
    that the cubic and Lanczos sums overshoot next to the steps and the range clamp has work."""
    x = np.empty((rows, U, C), F)
    for r in range(rows):
        for c in range(C):
            u = 0
            while u < U:
                n = int(rng.integers(2, 7))
                k = rng.uniform()
                x[r, u:u + n, c] = -0.5 if k < 0.35 else (1.0 if k < 0.7 else rng.uniform(-0.5, 1.0))
                u += n
    x[0, 0, 0], x[-1, -1, -1] = -0.5, 1.0     # both ends of the range are present whatever U is
    return x


def test_the_rule_program_equals_the_numpy_yardstick(tmp_path):
    """csrc/k16_dilate_rule.hpp, compiled alone by g++ into a program with its own main, on C in {1, 3}, f in {1, 2, 3, 4, 8},
    the three kinds and U in {1, 2, 5, 64, 65}: outputs and unclamped sums equal dilate_ref's bit for bit.  The program
    itself checks phase 0, the identity at f = 1, min and max, and that the clamp acts on >= 1 % of the samples."""
    exe = tmp_path / "dilate_rule_main"
    subprocess.run(GXX + [os.path.join(ROOT, "tests", "cpp", "dilate_rule_main.cpp"), "-o", str(exe)], check=True)
    rng = np.random.default_rng(16)
    cases = []
    with open(tmp_path / "cases.bin", "wb") as fh:
        for C in (1, 3):
            for f in (1, 2, 3, 4, 8):
                for kind in dr.KINDS:
                    for U in (1, 2, 5, 64, 65):
                        rows = 2 if U == 1 else 3          # (U = 1, C = 1 still holds both ends of the range)
                        x = step_field(rng, rows, U, C)
                        np.array([C, f, kind, U, rows], np.int32).tofile(fh)
                        x.tofile(fh)
                        cases.append((C, f, kind, U, rows, x))
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       env=dict(os.environ, **SAN_ENV))
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dilate rule: %d cases ok" % len(cases) in r.stdout
    got = np.fromfile(tmp_path / "out.bin", F)
    at = 0
    for C, f, kind, U, rows, x in cases:
        n = rows * dr.dilated_width(U, f) * C
        y, raw = got[at:at + n], got[at + n:at + 2 * n]
        at += 2 * n
        want = dr.dilate(x, f, kind)
        want_raw = dr.dilate(x, f, kind, clamp=False)
        label = (C, f, dr.NAMES[kind], U)
        assert np.array_equal(y.view(np.uint32), want.reshape(-1).view(np.uint32)), label
        assert np.array_equal(raw.view(np.uint32), want_raw.reshape(-1).view(np.uint32)), label
        assert want.min() == x.min() and want.max() == x.max(), label
        assert np.array_equal(want[:, ::f].view(np.uint32), x.view(np.uint32)), label
    assert at == got.size


def test_plan_and_weights_under_sanitizers(tmp_path):
    exe = tmp_path / "test_plan_dilate"
    subprocess.run(GXX + [os.path.join(ROOT, "tests", "cpp", "test_plan_dilate.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dilate plan tests ok" in r.stdout


def test_the_yardstick_by_hand():
    """Linear x2 is the midpoint; cubic x2 is (-1, 9, 9, -1) / 16 with the ends repeated; the clamp holds the overshoot."""
    x = np.array([0.0, 0.0, 1.0, 1.0, 0.25], F).reshape(1, 5, 1)
    lin = dr.dilate(x, 2, dr.LINEAR)[0, :, 0]
    assert lin.tolist() == [0.0, 0.0, 0.0, 0.5, 1.0, 1.0, 1.0, 0.625, 0.25]
    raw = dr.dilate(x, 2, dr.CUBIC, clamp=False)[0, :, 0]
    assert raw[1] == F(-0.0625) and raw[3] == F(0.5) and raw[5] == F(1.109375)
    cub = dr.dilate(x, 2, dr.CUBIC)[0, :, 0]
    assert cub[1] == 0.0 and cub[5] == 1.0 and cub.min() == 0.0 and cub.max() == 1.0
    assert np.array_equal(dr.dilate(x, 1, dr.LANCZOS3), x)
    assert dr.dilate(np.ones((2, 1, 3), F), 8, dr.LANCZOS3).shape == (2, 1, 3)
    assert dr.slab(np.ones((1, 1, 22, 1), F), 3, dr.LINEAR).shape == (1, 1, 128, 1)      # U' = 64: the pitch must be 128


def field_runs(oracle_mod, seed: int) -> dict:
    """MAE of the plain run and of the three x2 dilations of the small-slope field, through the oracle."""
    vol, delta = dr.small_slope_field(seed)
    ref = oracle_mod.depth1d_pile_run(vol, dr.FIELD_DMIN, dr.FIELD_DMAX, dr.FIELD_D)
    out = dict(plain=dr.field_mae(ref.depth_raw, ref.edge_mask, delta))
    for kind in dr.KINDS:
        p = oracle_mod.default_params()
        p.slope_factor = 2.0
        d = oracle_mod.depth1d_pile_run(dr.dilate(vol, 2, kind), dr.FIELD_DMIN, dr.FIELD_DMAX, dr.FIELD_D, params=p)
        out[dr.NAMES[kind]] = dr.field_mae(d.depth_raw, d.edge_mask, delta, 2)
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_point_of_the_feature(oracle_mod, seed):
    """V = 12, S = 9, U = 96 band-limited scanlines at disparities linspace(-0.45, 0.45, 12), 241 hypotheses in [-0.6, 0.6]:
    the mean absolute error of depth_raw over the confident pixels of columns 12 .. 83, relative to the undilated run, is
    <= 0.80 with cubic x2, <= 0.65 with Lanczos-3 x2 and within [0.95, 1.05] with linear x2 (which does nothing, as it should:
    the scan's own lerp).  The reference alone, dilation in float64, gave 0.63-0.68, 0.42-0.53 and 0.98-1.001 over seeds 1..6."""
    m = field_runs(oracle_mod, seed)
    ratios = {k: m[k] / m["plain"] for k in ("linear", "cubic", "lanczos3")}
    print("seed %d: plain MAE %.5f; ratios %s" % (seed, m["plain"], {k: round(v, 4) for k, v in ratios.items()}))
    assert m["plain"] > 0
    assert ratios["cubic"] <= 0.80
    assert ratios["lanczos3"] <= 0.65
    assert 0.95 <= ratios["linear"] <= 1.05


NAMES = ("rslf_dilated_width", "rslf_volume_dilate_u", "rslf_planes_undilate_u", "rslf_planes_undilate_u_host")


def test_the_library_exports_the_entries():
    """The entries resolve in the built library; the ABI version stays 6; what needs no device is refused or answered."""
    import ctypes as C
    from remotesensingproject_amd import _lib
    for name in NAMES:
        assert name in _lib.SYMBOLS
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "rslf_hip.h")).read()
    for name in NAMES:
        assert getattr(L, name) is not None and "int %s(" % name in header
    assert _lib.ABI_VERSION == 6 and L.rslf_abi_version() == 6
    for k, name in enumerate(("RSLF_DILATE_LINEAR", "RSLF_DILATE_CUBIC", "RSLF_DILATE_LANCZOS3")):
        assert "#define %s" % name in header
    w = C.c_int(-7)
    for U, f in ((1, 1), (2, 4), (33, 2), (22, 3), (1920, 8)):
        assert L.rslf_dilated_width(U, f, C.byref(w)) == 0 and w.value == dr.dilated_width(U, f)
    for U, f in ((0, 2), (10, 0), (10, 9), (-1, 1)):
        assert L.rslf_dilated_width(U, f, C.byref(w)) == -1
    assert L.rslf_dilated_width(10, 2, None) == -1
    # refused before a device is touched
    out = C.c_void_p()
    assert L.rslf_volume_dilate_u(None, None, 2, 1, C.byref(out)) == -1 and not out.value
    assert L.rslf_volume_dilate_u(None, None, 2, 1, None) == -1
    assert L.rslf_planes_undilate_u(None, None, 4, 1, 5, 2, None) == -1
    # the host form is a strided copy: u8 and 4-byte planes, padded rows, and its refusals
    for dt in (np.uint8, np.float32, np.int32):
        a = (np.arange(3 * 16).reshape(3, 16) % 251).astype(dt)
        src = a[:, :13]                                   # rows 16 elements apart, 13 = 4 * 3 + 1 wide
        dst = np.full((3, 6), 99, dt)
        e = a.itemsize
        rc = L.rslf_planes_undilate_u_host(src.ctypes.data, 16 * e, e, 3, 13, 4, dst.ctypes.data, 6 * e)
        assert rc == 0 and np.array_equal(dst[:, :4], src[:, ::4]) and (dst[:, 4:] == 99).all()
        dense = np.ascontiguousarray(src)
        dst2 = np.empty((3, 4), dt)
        assert L.rslf_planes_undilate_u_host(dense.ctypes.data, 0, e, 3, 13, 4, dst2.ctypes.data, 0) == 0
        assert np.array_equal(dst2, src[:, ::4])
    a = np.zeros((2, 13), F)
    b = np.zeros((2, 4), F)
    bad = [(None, 0, 4, 2, 13, 4, b.ctypes.data, 0), (a.ctypes.data, 0, 4, 2, 13, 4, None, 0), (a.ctypes.data, 0, 2, 2, 13, 4, b.ctypes.data, 0),
           (a.ctypes.data, 0, 4, 2, 13, 0, b.ctypes.data, 0), (a.ctypes.data, 0, 4, 2, 13, 9, b.ctypes.data, 0),
           (a.ctypes.data, 0, 4, 2, 12, 4, b.ctypes.data, 0), (a.ctypes.data, 0, 4, 2, 0, 4, b.ctypes.data, 0),
           (a.ctypes.data, 0, 4, 2, 13, 4, a.ctypes.data, 0), (a.ctypes.data, 8, 4, 2, 13, 4, b.ctypes.data, 0),
           (a.ctypes.data, 0, 4, 2, 13, 4, b.ctypes.data, 8)]
    for args in bad:
        assert L.rslf_planes_undilate_u_host(*args) == -1, args
        assert L.rslf_last_error()


def test_the_unit_is_registered():
    from remotesensingproject_amd import build
    assert "rslf_dilate.hip" in build.UNITS
    for h in ("k16_dilate.hpp", "k16_dilate_rule.hpp", "rslf_plan_dilate.hpp"):
        assert h in build.UNITS["rslf_dilate.hip"] and os.path.exists(os.path.join(CSRC, h))
    rule = open(os.path.join(CSRC, "k16_dilate_rule.hpp")).read()
    plan = open(os.path.join(CSRC, "rslf_plan_dilate.hpp")).read()
    assert "hip/" not in rule and "hip/" not in plan and '#include "k16_dilate_rule.hpp"' in plan


def test_the_python_signatures_and_the_refusals():
    """The new arguments with their defaults; what is not built says so by the argument's name, before a device is touched."""
    from remotesensingproject_amd import depth as rs
    from remotesensingproject_amd import sharding
    assert (rs.DILATE_LINEAR, rs.DILATE_CUBIC, rs.DILATE_LANCZOS3) == (dr.LINEAR, dr.CUBIC, dr.LANCZOS3) == (0, 1, 2)
    for cls in (rs.Depth1DComputer_pile, rs.Depth1DComputer, rs.Depth2DComputer):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["u_dilation"].default == 1 and sig["dilation_kind"].default == rs.DILATE_CUBIC
        assert callable(cls.undilated)
    sig = inspect.signature(rs.Volume.dilated_u).parameters
    assert list(sig) == ["self", "factor", "kind"] and sig["kind"].default == rs.DILATE_CUBIC
    assert list(inspect.signature(rs.undilate_u).parameters) == ["ctx", "planes", "factor"]
    # the line confidence takes no slope factor
    p = rs.Depth1DParameters(par_line_confidence_mode=rs.LINE_CONF_GATE)
    with pytest.raises(ValueError, match="par_line_confidence_mode=2 together with u_dilation=2"):
        rs.Depth2DComputer(None, -1.0, 1.0, 8, parameters=p, u_dilation=2)
    # factors and kinds that are none
    for cls in (rs.Depth1DComputer_pile, rs.Depth1DComputer, rs.Depth2DComputer):
        for bad in (0, 9, -2, 1.5, True):
            with pytest.raises(ValueError, match="u_dilation"):
                cls(None, -1.0, 1.0, 8, u_dilation=bad)
        with pytest.raises(ValueError, match="dilation_kind"):
            cls(None, -1.0, 1.0, 8, u_dilation=2, dilation_kind=3)
    # the forms that have no dilation
    new = object.__new__
    md = new(rs.MultiDevice)
    calls = [lambda: md.depth1d_pile(None, -1.0, 1.0, 8, u_dilation=2), lambda: md.depth2d(None, -1.0, 1.0, 8, u_dilation=2),
             lambda: md.fine_to_coarse(None, -1.0, 1.0, 8, u_dilation=2), lambda: md.depth1d_pile_device_out(None, -1.0, 1.0, 8, u_dilation=2),
             lambda: rs.FineToCoarse(None, -1.0, 1.0, 8, u_dilation=2), lambda: rs.fine_to_coarse_run_host(None, -1.0, 1.0, 8, u_dilation=2),
             lambda: sharding.ShardedDepth2D(None, None, -1.0, 1.0, 8, u_dilation=2),
             lambda: sharding.ShardedFineToCoarse(None, -1.0, 1.0, 8, 0, 1, u_dilation=2)]
    for call in calls:
        with pytest.raises(ValueError, match="u_dilation=2 is not built here"):
            call()
    # the caller's parameter object is not modified
    q = rs.Depth1DParameters(par_slope_factor=0.3)
    d = rs._dilated_parameters(q, 3)
    assert q.par_slope_factor == 0.3 and d is not q and d.par_slope_factor == float(F(0.3) * F(3))
    assert d.to_c().slope_factor == F(0.3) * F(3)
    # undilate_u's refusals that need no device
    import torch
    with pytest.raises(ValueError, match="CUDA tensor"):
        rs.undilate_u(None, torch.zeros((2, 5)), 2)
    with pytest.raises(ValueError, match="u_dilation"):
        rs.undilate_u(None, torch.zeros((2, 5)), 0)
