"""The row-exact table's arithmetic (remotesensingproject_amd/csrc/k2_taps.hpp, row_exact_entry) on the CPU, under
AddressSanitizer + UBSan: wherever an entry is flagged exact, its tap offset, weight and 1 - t are what every lane of
scan_reg_body computes for itself in EVERY pixel of the row whose sample lies inside it -- the bench grids, dyadic steps at the
edge where exactness is lost with the row's width, slopes 1 / 0.5 / 0.3, an off-centre s_hat, negative, positive and integer
offsets -- and the shares of row-exact hypotheses are the ones the scalar-tap form was designed on."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "remotesensingproject_amd", "csrc")


def _run(tmp_path):
    exe = tmp_path / "test_row_exact"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_row_exact.cpp"), "-o", str(exe)],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    print(r.stdout)
    return r


def test_row_exact_entry_matches_the_per_lane_arithmetic_in_every_pixel(tmp_path):
    r = _run(tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "row-exact tests ok" in r.stdout
    grids = {}
    for line in r.stdout.splitlines():
        m = re.match(r"grid (\S+) .* exact hypotheses (\d+) of (\d+), exact entries (\d+) \(t == 0: (\d+), off < 0: (\d+), off > 0: (\d+)\)", line)
        if m:
            grids[m.group(1)] = [int(x) for x in m.groups()[1:]]
    # the shares: c3, c2, c1 wholly exact; -1..1 with 7 hypotheses exactly D_d in {-1, 0, 1}; SkysatLR-like 2 of 120
    assert grids["c3"][:2] == [256, 256] and grids["c2"][:2] == [128, 128] and grids["c1"][:2] == [64, 64]
    assert grids["skysat_lr"][:2] == [2, 120]
    assert grids["minus1_1_D7"][:2] == [3, 7]
    which = sorted(float(l.split()[-1]) for l in r.stdout.splitlines() if l.startswith("exact-hypothesis minus1_1_D7 "))
    assert which == [-1.0, 0.0, 1.0], which
    # the GPU test's grids are what its docstring says: all exact / nearly none
    assert grids["gpu_D17"][:2] == [17, 17] and grids["gpu_U330"][:2] == [17, 17]
    assert grids["gpu_D18"][0] == 2   # (the GPU test asserts these counts on the device's table; the program holds its variants too)
    # the comparison saw negative, positive and integer offsets
    assert grids["c3"][3] > 0 and grids["c3"][4] > 0 and grids["c3"][5] > 0
    assert grids["integers"][1] == grids["integers"][0] and grids["integers"][3] == grids["integers"][2]
    # steps 2^-14 and 2^-16: all exact on a short row, lost on a long one
    assert grids["step_2^-14_U256"][0] == 33 and grids["step_2^-14_U4096"][0] < 33
    assert grids["step_2^-16_U4096"][0] <= grids["step_2^-14_U4096"][0]


def test_row_exact_header_needs_no_hip():
    txt = open(os.path.join(CSRC, "k2_taps.hpp")).read()
    assert "row_exact_entry" in txt and "hip/hip_runtime" not in txt and "__global__" not in txt
