"""The output stage's layout (rslf_plan_stage.hpp: plan::stage_layout) without a GPU: the plan header under sanitizers, as a
stand-alone program, and that the library's build knows the host frame's headers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remotesensingproject_amd", "csrc")


def test_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "test_plan_stage"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                    "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_plan_stage.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stage plan tests ok" in r.stdout


def test_the_frame_is_registered():
    """Staleness and source_hash() see the frame: every unit that includes it lists it and what it includes."""
    from remotesensingproject_amd import build
    for unit in ("rslf_consistency.hip", "rslf_warp.hip", "rslf_novel.hip"):
        assert '#include "rslf_stack_op.hpp"' in open(os.path.join(CSRC, unit)).read()
        for header in ("rslf_stack_op.hpp", "rslf_plan_stage.hpp", "rslf_plan_warp.hpp", "k14_warp_rule.hpp"):
            assert header in build.UNITS[unit] and os.path.exists(os.path.join(CSRC, header)), (unit, header)
