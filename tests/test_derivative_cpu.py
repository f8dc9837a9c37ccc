"""The derivative channels without a GPU (K17, rslf_volume_derivative_channels): the rule header as a stand-alone C++ program
against the numpy yardstick bit for bit, the plan functions under sanitizers, the exports, the Python signatures and the
refusals that need no device."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import derivative_ref as dref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remotesensingproject_amd", "csrc")
F = np.float32
GXX = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
       "-Wall", "-Wextra", "-Werror", "-I", CSRC]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
ELEM_ID = {"f32": 0, "u8": 1, "u16": 2}


def rule_cases():
    """(elem, weight, x [V,S,U] float32) -- random fields of every element type at odd shapes, U = 1, V = 1, a weight that
    saturates, and for integer elements the odd differences at weight = 1 whose halves are ties."""
    rng = np.random.default_rng(17)
    cases = []
    for V, S, U in ((3, 2, 7), (1, 2, 5), (4, 1, 1), (1, 1, 1), (2, 3, 66), (5, 2, 2)):
        cases.append(("f32", 1.0, rng.uniform(-0.5, 1.0, (V, S, U)).astype(F)))
        cases.append(("f32", 40.0, rng.uniform(0.0, 1.0, (V, S, U)).astype(F)))        # most features reach hi
        cases.append(("f32", 0.37, -rng.uniform(0.5, 1.0, (V, S, U)).astype(F)))       # a negative field: hi = 0
        cases.append(("u8", 1.0, rng.integers(0, 256, (V, S, U)).astype(F)))
        cases.append(("u8", 7.5, rng.integers(0, 256, (V, S, U)).astype(F)))           # saturates at 255
        cases.append(("u16", 1.0, rng.integers(0, 65536, (V, S, U)).astype(F)))
        cases.append(("u16", 300.0, rng.integers(0, 65536, (V, S, U)).astype(F)))      # saturates at 65535
    # differences 1, 3, 5 along u at weight 1: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    ties = np.array([[[0, 9, 1, 9, 4, 9, 9, 14, 9]]], F)        # centred differences at u = 1, 3, 5: 1, 3, 5; at the ends 9 and 5
    cases.append(("u8", 1.0, ties))
    cases.append(("u16", 1.0, ties))
    cases.append(("u8", 1.0, np.ascontiguousarray(ties.transpose(2, 1, 0))))           # the same along v
    return cases


def test_the_ties_by_hand():
    """Integer elements round the halves to even; float elements keep them; both cap at hi; one column or one row: zero."""
    x = np.array([[[0, 9, 1, 9, 4, 9, 9, 14, 9]]], F)
    a = dref.augment(x, 1.0, "u8")
    assert a[0, 0, :, 0].tolist() == x[0, 0].tolist()
    assert a[0, 0, [1, 3, 5, 7], 1].tolist() == [0.0, 2.0, 2.0, 0.0]             # 0.5, 1.5, 2.5, 0
    assert a[0, 0, [0, 8], 1].tolist() == [4.0, 2.0]                               # the ends: |9 - 0| / 2 = 4.5 -> 4, |9 - 14| / 2 -> 2
    assert not a[..., 2].any()                                                     # V = 1
    f = dref.augment(x, 1.0, "f32")
    assert f[0, 0, [1, 3, 5], 1].tolist() == [0.5, 1.5, 2.5]
    assert dref.augment(x, 100.0, "u8")[..., 1].max() == 255 and dref.augment(x, 100.0, "f32")[..., 1].max() == 14.0
    assert not dref.augment(np.ones((3, 2, 1), F), 2.0)[..., 1].any()
    assert dref.augment(-np.ones((2, 1, 3), F) * np.arange(1, 4, dtype=F), 1.0)[..., 1:].max() == 0.0     # hi = max(m, 0) = 0
    assert dref.slab(np.ones((1, 1, 64), F), 1.0).shape == (1, 1, 128, 3)


def test_the_rule_program_equals_the_numpy_yardstick(tmp_path):
    """csrc/k17_derivative_rule.hpp, compiled alone by g++ with -ffp-contract=off into a program with its own main: its
    outputs equal derivative_ref's bytes for every case of rule_cases()."""
    exe = tmp_path / "derivative_rule_main"
    subprocess.run(GXX + [os.path.join(ROOT, "tests", "cpp", "derivative_rule_main.cpp"), "-o", str(exe)], check=True)
    cases = rule_cases()
    with open(tmp_path / "cases.bin", "wb") as fh:
        for elem, w, x in cases:
            np.array([ELEM_ID[elem], *x.shape], np.int32).tofile(fh)
            np.array([w, dref.cap_of(x, elem)], F).tofile(fh)
            x.tofile(fh)
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "derivative rule: %d cases ok" % len(cases) in r.stdout
    got = np.fromfile(tmp_path / "out.bin", F)
    at, saturated, ties = 0, 0, 0
    for elem, w, x in cases:
        want = dref.augment(x, w, elem)
        y = got[at:at + want.size]
        at += want.size
        assert np.array_equal(y.view(np.uint32), want.reshape(-1).view(np.uint32)), (elem, w, x.shape)
        assert np.array_equal(want[..., 0].view(np.uint32), x.view(np.uint32))
        if x.shape[2] == 1:
            assert not want[..., 1].any()
        if x.shape[0] == 1:
            assert not want[..., 2].any()
        hi = dref.cap_of(x, elem)
        saturated += int((want[..., 1:] == hi).sum()) if hi > 0 else 0
        if elem != "f32" and w == 1.0:
            u = np.arange(x.shape[2])
            d = np.abs(x[:, :, np.minimum(u + 1, x.shape[2] - 1)] - x[:, :, np.maximum(u - 1, 0)])
            ties += int((d % 2 == 1).sum())
    assert at == got.size and saturated > 100 and ties > 50


def test_the_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "test_plan_derivative"
    subprocess.run(GXX + [os.path.join(ROOT, "tests", "cpp", "test_plan_derivative.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "derivative plan tests ok" in r.stdout


NAMES = ("rslf_volume_derivative_channels", "rslf_derivative_channels_dense", "rslf_fine_to_coarse_run_host_dv", "rslf_f2c_run_host_dv")


def test_the_library_exports_the_entries():
    """The entries resolve in the built library; the ABI version stays 6; what needs no device is refused, *out left as the
    contract says."""
    import ctypes as C
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "rslf_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and getattr(L, name) is not None and "int %s(" % name in header
    assert _lib.ABI_VERSION == 6 and L.rslf_abi_version() == 6
    out = C.c_void_p(0x1234)
    assert L.rslf_volume_derivative_channels(None, None, 1.0, C.byref(out)) == -1 and not out.value       # NULL on failure
    assert L.rslf_volume_derivative_channels(None, None, 1.0, None) == -1
    assert "NULL" in L.rslf_last_error().decode()
    a = np.zeros(8, F)
    assert L.rslf_derivative_channels_dense(None, a.ctypes.data, 0, 1, 1, 2, 1.0, 1.0, a.ctypes.data) == -1
    n = C.c_int(-1)
    for w in (-1.0, float("nan"), float("inf")):   # refused by the level loop before a device is touched: the context is NULL
        assert L.rslf_fine_to_coarse_run_host_dv(None, None, 0, 4, 4, 4, 1, 0, -1.0, 1.0, 8, -1.0, None, -1, 1, None, None, C.byref(n),
                                                 None, 0, None, 0, w) == -1
    run = C.c_void_p(0x1234)
    assert L.rslf_f2c_run_host_dv(None, None, 0, 4, 4, 4, 1, 0, -1.0, 1.0, 8, -1.0, None, -1, 1, 0, 0, 0, C.byref(run), None, 0, 0, 0.0,
                                  0.0, 0.0, 0, 0, 1.0) == -1 and not run.value


def test_the_unit_is_registered():
    from remotesensingproject_amd import build
    assert "rslf_derivative.hip" in build.UNITS and "-ffp-contract=off" in build.HIPCC_FLAGS
    for h in ("k17_derivative.hpp", "k17_derivative_rule.hpp", "rslf_plan_derivative.hpp"):
        assert h in build.UNITS["rslf_derivative.hip"] and os.path.exists(os.path.join(CSRC, h))
    rule = open(os.path.join(CSRC, "k17_derivative_rule.hpp")).read()
    plan = open(os.path.join(CSRC, "rslf_plan_derivative.hpp")).read()
    assert "hip/" not in rule and "hip/" not in plan and '#include "k17_derivative_rule.hpp"' in plan


def test_the_python_signatures_and_the_refusals():
    """The new names with their defaults; what is not built says so by the argument's name, before a device is touched."""
    import torch
    from remotesensingproject_amd import depth as rs
    from remotesensingproject_amd import sharding
    assert list(inspect.signature(rs.Volume.with_derivative_channels).parameters) == ["self", "weight"]
    sig = inspect.signature(rs.derivative_channels).parameters
    assert list(sig) == ["ctx", "raw_vsuc", "weight", "dtype"]
    for fn in (rs.fine_to_coarse_run_host, rs.FineToCoarse.__init__, rs.MultiDevice.fine_to_coarse, sharding.ShardedFineToCoarse.__init__):
        params = inspect.signature(fn).parameters
        last = list(params.values())[-1]
        assert last.name == "derivative_channels" and last.default == 0.0 and last.kind is inspect.Parameter.KEYWORD_ONLY, fn
    # the forms that do not build it
    md = object.__new__(rs.MultiDevice)
    for w in (0.5, 2):
        for call in (lambda: md.fine_to_coarse(None, -1.0, 1.0, 8, derivative_channels=w),
                     lambda: sharding.ShardedFineToCoarse(None, -1.0, 1.0, 8, 0, 1, derivative_channels=w)):
            with pytest.raises(ValueError, match="derivative_channels=%r is not built here" % (w,)):
                call()
    # weights that are none
    for bad in (-1.0, float("nan"), float("inf"), True, "x", 1e39):
        with pytest.raises(ValueError, match="derivative_channels"):
            rs.fine_to_coarse_run_host(None, -1.0, 1.0, 8, derivative_channels=bad)
        with pytest.raises(ValueError, match="derivative_channels"):
            rs.FineToCoarse(None, -1.0, 1.0, 8, derivative_channels=bad)
        with pytest.raises(ValueError, match="derivative_channels"):
            rs.derivative_channels(None, torch.zeros((2, 2, 2)), bad)
    with pytest.raises(ValueError, match="finite weight > 0"):
        rs.derivative_channels(None, torch.zeros((2, 2, 2)), 0)
    with pytest.raises(ValueError, match="float32 CUDA tensor"):
        rs.derivative_channels(None, torch.zeros((2, 2, 2)), 1.0)
    vol = object.__new__(rs.Volume)
    for bad in (0, None, -2.0, float("nan")):
        with pytest.raises(ValueError, match="derivative_channels"):
            vol.with_derivative_channels(bad)
    vol._h = None   # (nothing to destroy)
    # an RGB field has no derivative channels: refused on the host, by the argument's name
    rgb = [np.zeros((3, 12, 3), F) for _ in range(12)]
    with pytest.raises(ValueError, match="derivative_channels=1.5 needs a one-channel field"):
        rs.fine_to_coarse_run_host(rgb, -1.0, 1.0, 8, ctx=object(), derivative_channels=1.5)
    assert rs._derivative_weight(None, "x") == 0.0 and rs._derivative_weight(0, "x") == 0.0 and rs._derivative_weight(2, "x") == 2.0
