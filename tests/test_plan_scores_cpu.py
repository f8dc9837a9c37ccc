"""Host-side planning of the score rows (rslf_plan.hpp, "score rows") on the CPU under AddressSanitizer + UBSan: a
stand-alone program with its own main, built with g++ and run directly, as tests/test_plan_cpu.py runs test_plan.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remotesensingproject_amd", "csrc")


def test_score_plan_unit_tests_under_sanitizers(tmp_path):
    exe = tmp_path / "test_plan_scores"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_plan_scores.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plan score tests ok" in r.stdout
