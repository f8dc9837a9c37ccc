"""The batched renderers without a GPU: their host-side rules (rslf_plan_render.hpp: workgroups per plane and their cap,
scratch sizes, launches per fit, the 16-byte rule with the plane stride) under AddressSanitizer + UBSan, and the new
entries' place in the header, the binding and the library."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remotesensingproject_amd", "csrc")
NEW = ["rslf_render_fit_many", "rslf_render_planes_each", "rslf_render_planes_host", "rslf_render_epi_lines_host"]


def test_plan_render_batch_unit_tests_under_sanitizers(tmp_path):
    exe = tmp_path / "test_plan_render_batch"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_plan_render_batch.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "render batch plan tests ok" in r.stdout


def test_render_plan_header_is_host_only():
    txt = open(os.path.join(CSRC, "rslf_plan_render.hpp")).read()
    assert "hip/hip_runtime" not in txt and "__device__" not in txt and "__global__" not in txt


def test_a_fit_is_one_launch_sequence_one_copy_and_one_wait():
    """fit_many in rslf_render.hip, which every fit goes through: no launch, copy or wait sits in a loop over planes (the
    only loops over planes are host arithmetic), and the body holds one wait per branch."""
    src = open(os.path.join(CSRC, "rslf_render.hip")).read()
    body = src[src.index("int fit_many("):src.index("int check_fit_args(")]
    assert body.count("hipStreamSynchronize") == 2 and body.count("hipMemcpyAsync") == 2   # the QUANTILE branch, and the other
    assert body.count("hipLaunchKernelGGL") == 5   # init, count, narrow (in the loop over digits) | partial sums, reduction
    for loop in re.findall(r"for \(int k = [^{]*\{[^}]*\}", body):
        assert "hip" not in loop
    assert 'extern "C" int rslf_render_fit(' in src and src.count("fit_many(ctx") >= 4   # the single call is the batch of one


def test_new_symbols_are_declared_bound_and_guarded():
    from remotesensingproject_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "rslf_hip.h")).read()
    src = open(os.path.join(CSRC, "rslf_render.hip")).read()
    for n in NEW:
        assert n in _lib.SYMBOLS and hasattr(L, n) and ("int %s(" % n) in hdr and ('extern "C" int %s(' % n) in src
    # NULL handles and bad counts are rejected before anything is touched
    mm = (C.c_double * 2)()
    assert L.rslf_render_fit_many(None, None, 1, 0, 1, 1, 1, None, 0, mm) == -1
    assert L.rslf_render_planes_each(None, None, 1, 0, 1, 1, 1, mm, 0, None, None, 0, None, 0, 0, 0.0, None) == -1
    assert L.rslf_render_planes_host(None, None, 1, 0, 1, 1, 1, None, 0, -1, 0, 0, None, 0, None, 0, 0, 0.0, None, None) == -1
    assert L.rslf_render_epi_lines_host(None, None, None, 1, 1, 1, 0, 0, 1, None, None) == -1


def test_cpp_getters_compile_as_cxx11(tmp_path):
    """The getters of include/rslf_hip.hpp and the program that uses them, syntax and types only (the run is
    tests/test_gpu_cpp_getters.py)."""
    subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_host_getters.cpp")], check=True)
