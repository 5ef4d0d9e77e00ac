"""CPU: the FASTQ rule of seeq_amd/csrc/seeq_fastq.h -- which raw lines are sequence lines, their record numbers, the records a
buffer of so many raw lines counts -- compiled for the host by plain g++ (tests/fastq_host_driver.cpp) and compared with the
Python one-liners the GPU tests (tests/test_gpu_fastq.py) build their expectations from.  Once more as a stand-alone program
under -fsanitize=address,undefined."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "seeq_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "build")
SRC = os.path.join(ROOT, "tests", "fastq_host_driver.cpp")


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    deps = [SRC, os.path.join(CSRC, "seeq_fastq.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + ["-I" + CSRC, SRC, "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _check(out):
    rows = [ln.split() for ln in out.splitlines()]
    got_l = {int(r[1]): (int(r[2]), int(r[3])) for r in rows if r[0] == "L"}
    got_n = {int(r[1]): int(r[2]) for r in rows if r[0] == "N"}
    assert sorted(got_l) == list(range(1, 42)) and sorted(got_n) == list(range(14))
    for line in range(1, 42):
        is_seq = (line - 1) % 4 == 1
        assert got_l[line] == (int(is_seq), (line - 1) // 4 + 1 if is_seq else 0), line
    # the sequence lines, in order, are records 1, 2, 3, ...
    assert [got_l[line][1] for line in range(1, 42) if got_l[line][0]] == list(range(1, 11))
    for raw in range(14):
        lines = ["x"] * raw
        assert got_n[raw] == len(lines[1::4]), raw
    tile, wg, items = [int(x) for x in next(r for r in rows if r[0] == "T")[1:]]
    assert tile == wg * items and wg % 64 == 0


def test_fastq_rule_on_the_host():
    exe = _build("fastq_host_driver", [])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    _check(r.stdout)


def test_fastq_rule_under_sanitizers():
    exe = _build("fastq_host_driver_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    _check(r.stdout)
