"""The C-ABI library on a box without a GPU: it loads, exports every symbol the header
declares, its structs match the ctypes mirror, and it fails cleanly (no compute, no crash)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rslf_hip.h")


@pytest.fixture(scope="module")
def L():
    from remotesensingproject_amd import _lib
    return _lib.lib()


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rslf_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported(L):
    from remotesensingproject_amd import _lib
    names = declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(L, n), "librslf_hip.so does not export %s" % n
    assert sorted(_lib.SYMBOLS) == names, "binding and header disagree on the symbol list"


def test_abi_version_and_strings(L):
    from remotesensingproject_amd import _lib
    assert L.rslf_abi_version() == _lib.ABI_VERSION == 6
    assert L.rslf_status_string(0) == b"ok"
    assert b"invalid" in L.rslf_status_string(-1)


def test_default_params_match_reference_defaults(L, oracle_mod):
    """core.hpp:16-31, :74-99 -- and the oracle's mirror of the same defaults."""
    from remotesensingproject_amd import _lib
    from remotesensingproject_amd.depth import Depth1DParameters
    p = _lib.default_params()
    o = oracle_mod.default_params()
    assert p.edge_score_threshold == C.c_float(0.02).value
    assert p.raw_score_threshold == 0.0
    assert p.mean_shift_max_iter == 10.0
    assert p.edge_confidence_filter_size == 9 and p.median_filter_size == 5
    assert p.median_filter_epsilon == C.c_float(0.1).value
    assert p.slope_factor == 1.0 and p.cut_shadows == 1
    assert p.shadow_level == C.c_float(0.05 * 1.73205080757).value
    assert p.kernel_bandwidth == C.c_float(0.2).value
    assert p.interpolation == 0 == o.interpolation   # Interpolation1DLinear, core.hpp:76
    for f in ("edge_score_threshold", "raw_score_threshold", "mean_shift_max_iter", "edge_confidence_filter_size",
              "median_filter_size", "median_filter_epsilon", "slope_factor", "cut_shadows", "shadow_level", "kernel_bandwidth"):
        assert getattr(p, f) == getattr(o, f), f
    q = Depth1DParameters().to_c()
    for f, _ in _lib.RslfParams._fields_:
        assert getattr(p, f) == getattr(q, f), f


def test_struct_layout_matches_c(tmp_path):
    """sizeof/offsetof as gcc sees include/rslf_hip.h == the ctypes mirror."""
    from remotesensingproject_amd import _lib
    src = tmp_path / "layout.c"
    fields_p = [f for f, _ in _lib.RslfParams._fields_]
    fields_d = [f for f, _ in _lib.RslfVolumeDesc._fields_]
    fields_s = [f for f, _ in _lib.RslfStats._fields_]
    body = ['#include <stdio.h>', '#include <stddef.h>', '#include "rslf_hip.h"', 'int main(void){',
            'printf("%zu %zu %zu\\n", sizeof(rslf_params), sizeof(rslf_volume_desc), sizeof(rslf_stats));']
    for f in fields_p:
        body.append('printf("%%zu\\n", offsetof(rslf_params, %s));' % f)
    for f in fields_d:
        body.append('printf("%%zu\\n", offsetof(rslf_volume_desc, %s));' % f)
    for f in fields_s:
        body.append('printf("%%zu\\n", offsetof(rslf_stats, %s));' % f)
    body.append("return 0;}")
    src.write_text("\n".join(body))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    sizes = list(map(int, out[:3]))
    assert sizes == [C.sizeof(_lib.RslfParams), C.sizeof(_lib.RslfVolumeDesc), C.sizeof(_lib.RslfStats)]
    offs = list(map(int, out[3:]))
    want = [getattr(_lib.RslfParams, f).offset for f in fields_p] + \
           [getattr(_lib.RslfVolumeDesc, f).offset for f in fields_d] + \
           [getattr(_lib.RslfStats, f).offset for f in fields_s]
    assert offs == want


def test_header_is_plain_c(tmp_path):
    """The boundary must be consumable from C and from the reference's C++11."""
    for comp, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text('#include "rslf_hip.h"\nint main(void){ rslf_params p; (void)p; return 0; }\n')
        subprocess.run([comp, std, "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / ("inc_%s.o" % ext))], check=True)


def test_no_device_is_an_error_not_a_fallback(L):
    """On a box without a GPU the product must refuse, loudly -- never compute on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    rc = L.rslf_ctx_create(0, C.byref(h))
    assert rc in (-4, -3), rc
    assert not h.value
    assert L.rslf_last_error()
    # NULL handles are rejected, not dereferenced
    assert L.rslf_volume_create(None, 1, 1, 1, 1, C.byref(h)) == -1
    assert L.rslf_ctx_synchronize(None) == -1


def test_host_epi_lists_reach_the_library_checked_and_converted():
    """MultiDevice's four methods (depth1d_pile, depth2d, fine_to_coarse, depth1d_pile_device_out) hand their EPI lists to
    the library through depth.host_epis; MultiDevice() itself needs a device.  An EPI shorter than the first is refused
    before the library could read past its end; every EPI goes as the first one's element type, or as float32 where the
    method takes float32 only (depth1d_pile_device_out)."""
    import numpy as np
    from remotesensingproject_amd import depth as rs
    short = [np.zeros((5, 7), np.float32) for _ in range(4)]
    short[2] = np.zeros((5, 6), np.float32)
    with pytest.raises(ValueError):
        rs.host_epis(short)
    mixed = [np.full((5, 7), 3, np.uint16), np.full((5, 7), 2.0, np.float64), np.full((5, 7), 1, np.uint8)]
    keep, ptrs, dt, V, S, U, C_ = rs.host_epis(mixed)
    assert dt == np.uint16 and [a.dtype for a in keep] == [np.uint16] * 3
    assert (V, S, U, C_) == (3, 5, 7, 1) and [int(a[0, 0]) for a in keep] == [3, 2, 1]
    assert keep[0] is mixed[0] and list(ptrs) == [a.ctypes.data for a in keep]
    keep, _, dt, V, S, U, C_ = rs.host_epis(mixed, np.float32)
    assert dt == np.float32 and all(a.dtype == np.float32 for a in keep)
    assert rs.host_epis([np.zeros((2, 4, 3), np.uint8)] * 2)[3:] == (2, 2, 4, 3)


def test_host_rows_takes_padded_rows_in_place_and_copies_what_it_cannot():
    """depth.host_rows, the one place where a host array becomes (pointer, row_stride_bytes): dense arrays go as stride 0 (as
    they always did), a window of a wider parent goes up where it lies with the parent's stride, and whatever one stride
    cannot describe -- mixed strides, a channel slice, a reversed or transposed view, another dtype -- goes as a dense copy."""
    import numpy as np
    from remotesensingproject_amd import depth as rs
    for dt, C_ in ((np.float32, 1), (np.uint8, 3), (np.uint16, 1)):
        shape = (5, 20) if C_ == 1 else (5, 20, C_)
        parents = [np.arange(np.prod(shape), dtype=np.int64).reshape(shape).astype(dt) for _ in range(3)]
        row_bytes = 7 * C_ * np.dtype(dt).itemsize
        # dense in: stride 0, the arrays themselves
        dense = [np.ascontiguousarray(p[:, 3:10]) for p in parents]
        keep, ptrs, stride = rs.host_rows(dense, dt)
        assert stride == 0 and all(k is d for k, d in zip(keep, dense)) and list(ptrs) == [d.ctypes.data for d in dense]
        # a padded window: the same pointer, the parent's stride
        views = [p[:, 3:10] for p in parents]
        keep, ptrs, stride = rs.host_rows(views, dt)
        assert stride == parents[0].strides[0] != row_bytes
        assert list(ptrs) == [v.ctypes.data for v in views] and all(k is v for k, v in zip(keep, views))
        # host_epis hands the same on
        out = rs.host_epis(views, stride=True)
        assert out[2] == dt and out[3:] == (3, 5, 7, C_, parents[0].strides[0]) and list(out[1]) == list(ptrs)
        # ... and without the stride, to a caller that passes 0, dense copies
        out = rs.host_epis(views)
        assert len(out) == 7 and all(k.flags.c_contiguous and np.array_equal(k, v) for k, v in zip(out[0], views))
        assert list(out[1]) == [k.ctypes.data for k in out[0]] and rs.host_epis(dense, stride=True)[7] == 0
        # a window as wide as its parent is dense
        assert rs.host_rows([p[:, :] for p in parents], dt)[2] == 0
        # mixed strides (a clone among windows): everything dense, values kept
        mixed = [views[0], dense[1], views[2]]
        keep, ptrs, stride = rs.host_rows(mixed, dt)
        assert stride == 0 and all(k.flags.c_contiguous for k in keep) and keep[1] is dense[1]
        assert all(np.array_equal(k, m) for k, m in zip(keep, mixed)) and list(ptrs) == [k.ctypes.data for k in keep]
        wider = np.zeros((5, 31) + shape[2:], dt)
        assert rs.host_rows([views[0], wider[:, 3:10]], dt)[2] == 0
        # views one stride cannot describe, and another dtype
        for odd in ([v[:, ::-1] for v in views], [v[::-1] for v in views], [v[:, ::2] for v in views],
                    [v.astype(np.float64) for v in views]):
            keep, ptrs, stride = rs.host_rows(odd, dt)
            assert stride == 0 and all(k.flags.c_contiguous and k.dtype == dt for k in keep)
            assert all(np.array_equal(k, o) for k, o in zip(keep, odd))
    rgb = [np.arange(5 * 20 * 3, dtype=np.float32).reshape(5, 20, 3) for _ in range(2)]
    for sliced in ([p[:, 3:10, 1] for p in rgb], [p[:, 3:10, :1] for p in rgb], [p[:, 3:10, :2] for p in rgb]):   # channel slices
        keep, ptrs, stride = rs.host_rows(sliced, np.float32)
        assert stride == 0 and all(k.flags.c_contiguous for k in keep) and all(np.array_equal(k, s) for k, s in zip(keep, sliced))
    # one row: no stride to speak of; lists (not arrays) are converted
    assert rs.host_rows([p[:1, 3:10] for p in rgb], np.float32)[2] == 0
    assert rs.host_rows([[[1, 2], [3, 4]]], np.uint8)[2] == 0
    with pytest.raises(ValueError):
        rs.host_rows([rgb[0][:, 3:10], rgb[1][:, 3:9]], np.float32)


def test_product_does_not_import_the_oracle():
    """oracle/ is test infrastructure: nothing under the package or include/ may reference it."""
    bad = []
    for base in (os.path.join(ROOT, "remotesensingproject_amd"), os.path.join(ROOT, "include")):
        for dp, _, fs in os.walk(base):
            for f in fs:
                if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                    txt = open(os.path.join(dp, f), errors="replace").read()
                    if re.search(r"^\s*(import|from)\s+oracle\b", txt, flags=re.M) or "rslf_oracle" in txt or "liboracle" in txt:
                        bad.append(os.path.join(dp, f))
    assert not bad, bad


def test_opencv_block_compiles():
    """The cv::Mat constructors and getters of include/rslf_hip.hpp (north_star's literal 'cv::Mat in / cv::Mat out') are
    compiled -- syntax and types only -- against a declaration-only mock of the few cv::Mat members they touch: this image
    has no OpenCV, and without this the block had never met a compiler."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(root, "include"),
                        "-I", os.path.join(root, "tests", "cpp", "opencv_mock"), os.path.join(root, "tests", "cpp", "opencv_block.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
