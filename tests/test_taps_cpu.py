"""The tap table's arithmetic (remotesensingproject_amd/csrc/k2_taps.hpp) on the CPU, under AddressSanitizer + UBSan: wherever
tap_entry says an entry holds for a whole tile, its weight, tap and 1 - t are what every lane of scan_reg_body computes for
itself -- random and dyadic offsets, half-quantum ties in every binade, tiles on binade edges, ragged tiles, the row's ends
-- and the share of gather batches that take the table on the c3 and SkysatLR-like frames is the one DESIGN.md quotes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remotesensingproject_amd", "csrc")


def _run_tap_program(tmp_path):
    exe = tmp_path / "test_taps"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_taps.cpp"), "-o", str(exe)],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    print(r.stdout)
    return r


def test_tap_entry_matches_the_per_lane_arithmetic(tmp_path):
    """One run of the program.  Its own assertions (per-lane comparison; the c3 and SkysatLR-like shares, 0.833 / 0.546 with the
    padded batch counted and 0.769 / 0.504 for the whole batches the kernel serves), and every frame's kernel shares against
    tests/taps_ref.py, the numpy restatement the GPU tests take their shares from: the two are written independently."""
    from tests import taps_ref
    r = _run_tap_program(tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tap tests ok" in r.stdout
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("share ")]
    assert len(lines) >= 7
    for w in lines:
        U, S, D = int(w[3]), int(w[5]), int(w[7])
        dmin, dmax, slope = float(w[9]), float(w[11]), float(w[13])
        kern_in, kern_border = float(w[19]), float(w[20])
        ref_in, ref_border = taps_ref.batch_shares(U, S, D, dmin, dmax, slope)
        assert abs(ref_in - kern_in) < 1e-5 and abs(ref_border - kern_border) < 1e-5, (w[1], ref_in, kern_in, ref_border, kern_border)


def test_taps_header_needs_no_hip():
    """k2_taps.hpp is shared by the kernel and the host: g++ alone must compile it, so no HIP include."""
    txt = open(os.path.join(CSRC, "k2_taps.hpp")).read()
    assert "hip/hip_runtime" not in txt and "__global__" not in txt
