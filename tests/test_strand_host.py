"""CPU: the both-strands rule of seeq_amd/csrc/seeq_strand.h -- the reverse complement of compiled key bytes, the co-rank that places
a record in the merged array, the winner of a line -- compiled for the host by plain g++ (tests/strand_host_driver.cpp) and compared
with device.revcomp_pattern, Python's sorted() and a per-line min().  Once more as a stand-alone program under
-fsanitize=address,undefined.  Then the entries on the real library: exports, the strand bit, and the argument checks, which run
before any device call and so fail the same way without a GPU."""
import ctypes as C
import errno
import os
import random
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "seeq_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "build")
SRC = os.path.join(ROOT, "tests", "strand_host_driver.cpp")
EXPRS = ["GATGTAGCGCGATTAGCCTG", "TG[AC]CANNGT", "GAATTC", "A[]CG[TU]N"]
SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025]
FIRST, BEST, ALL = 0, 1, 2


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    deps = [SRC, os.path.join(CSRC, "seeq_strand.h"), os.path.join(CSRC, "seeq_pattern.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + ["-I" + CSRC, SRC, "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


# ---- the reverse complement of key bytes ----
def _check_keys(out):
    from seeq_amd import device as dev
    rows = [ln.split() for ln in out.splitlines()]
    assert len(rows) == len(EXPRS) and all(r[0] == "K" for r in rows)
    for expr, (_, keys, rc, of_expr, twice) in zip(EXPRS, rows):
        assert rc == of_expr, (expr, dev.revcomp_pattern(expr))     # the key-level complement == the compiled revcomp_pattern(expr)
        assert twice == keys, expr                                  # applying it twice is the identity
        assert len(rc) == len(keys)
    by = dict(zip(EXPRS, rows))
    assert by["GAATTC"][1] == by["GAATTC"][2] == "040101080802"     # maps to itself
    assert by["TG[AC]CANNGT"][1] == "0804030201" + "1f1f" + "0408" and by["TG[AC]CANNGT"][2] == "0102" + "1f1f" + "0804" + "0c" + "0201"   # [AC] -> [GT], N stays N
    assert by["A[]CG[TU]N"][1] == "010204081f" and by["A[]CG[TU]N"][2] == "1f01020408"      # [] is no position, U is T


def _key_args():
    from seeq_amd import device as dev
    args = []
    for e in EXPRS:
        args += [e, dev.revcomp_pattern(e)]
    return args


def test_revcomp_pattern_expressions():
    from seeq_amd import device as dev
    assert dev.revcomp_pattern("GATGTAGCGCGATTAGCCTG") == "CAGGCTAATCGCGCTACATC"
    assert dev.revcomp_pattern("TG[AC]CANNGT") == "ACNNTG[TG]CA"
    assert dev.revcomp_pattern("GAATTC") == "GAATTC"
    assert dev.revcomp_pattern("A[]CG[TU]N") == "N[AA]CG[]T"
    assert dev.revcomp_pattern("acgU") == "Acgt"                       # case is preserved, U is read as T
    for e in EXPRS + ["ACGTTGCA", "[ACG][TN]A"]:
        assert dev.revcomp_pattern(dev.revcomp_pattern(e)).replace("U", "T") == e.replace("U", "T")
    for bad in ("AC[GT", "ACXT", "AC]T"):
        with pytest.raises(ValueError):
            dev.revcomp_pattern(bad)


def test_key_reverse_complement_on_the_host():
    exe = _build("strand_host_driver", [])
    r = subprocess.run([exe, "keys"] + _key_args(), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    _check_keys(r.stdout)
    tile, wg, items, minus = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()[1:]]
    assert tile == wg * items == 1024 and wg % 64 == 0 and minus == 0x80000000


# ---- the merge ----
def _strand_list(rng, n, mode, lo, hi, every_line=False):
    """n records (line, start, end, dist) in key order, lines in [lo, hi): SQ_ALL -- strictly increasing (line, end), starts that
    repeat; SQ_BEST / SQ_FIRST -- at most one record per line."""
    if n == 0:
        return []
    if mode == ALL and not every_line:
        keys = set()
        while len(keys) < n:
            keys.add((rng.randrange(lo, hi), rng.randrange(8, 40)))
        keys = sorted(keys)
    else:
        keys = [(ln, rng.randrange(8, 40)) for ln in sorted(rng.sample(range(lo, hi), n))]
    return [(ln, max(0, end - rng.randrange(6, 9)), end, rng.randrange(0, 4)) for ln, end in keys]


def _cases():
    rng = random.Random(20251018)
    cases = []
    for mode in (FIRST, BEST, ALL):
        for na in SIZES:
            for nb in SIZES:
                span = max(4, (na + nb) // 2)               # about half the lines are shared
                cases.append((mode, _strand_list(rng, na, mode, 1, 1 + max(span, na)), _strand_list(rng, nb, mode, 1, 1 + max(span, nb))))
                # all plus keys below all minus keys, and the reverse
                cases.append((mode, _strand_list(rng, na, mode, 1, 1 + 2 * na), _strand_list(rng, nb, mode, 1 + 2 * na, 1 + 2 * na + 2 * nb)))
                cases.append((mode, _strand_list(rng, na, mode, 1 + 2 * nb, 1 + 2 * nb + 2 * na), _strand_list(rng, nb, mode, 1, 1 + 2 * nb)))
            # identical key sets: every key ties (the distances too, or not)
            a = _strand_list(rng, na, mode, 1, 1 + 2 * na)
            cases.append((mode, a, list(a)))
            cases.append((mode, a, [(ln, s, e, rng.randrange(0, 4)) for ln, s, e, d in a]))
    return cases


def _expected(mode, a, b):
    """-> the merged records (line, start, end, dist, strand) in order: SQ_ALL all of them, else the winners."""
    both = [r + (0,) for r in a] + [r + (1,) for r in b]
    if mode == ALL:
        return sorted(both, key=lambda r: (r[0], r[2], r[4]))
    per_line = {}
    for r in both:
        per_line.setdefault(r[0], []).append(r)
    pick = (lambda r: (r[3], r[4])) if mode == BEST else (lambda r: (r[2], r[4]))
    return [min(per_line[ln], key=pick) for ln in sorted(per_line)]


def _check_merge(out, cases):
    lines = out.split("\n")
    at = 0
    for mode, a, b in cases:
        n = len(a) + len(b)
        assert lines[at] == "M %d" % n
        got = [tuple(int(x) for x in ln.split()) for ln in lines[at + 1:at + 1 + n]]
        at += 1 + n
        exp = _expected(mode, a, b)
        kept = [r for r in got if r[0] != 0]
        assert kept == exp, (mode, len(a), len(b))
        if mode == ALL:
            assert len(kept) == n
        else:
            # a loser keeps its place in (line, end, strand) order: with its line number back, the array is the SQ_ALL merge
            assert len(got) - len(kept) == n - len(exp)
            assert sorted(r[1:] for r in got) == sorted(r[1:] for r in _expected(ALL, a, b))
    assert lines[at:] in ([], [""])


def _merge_input(cases):
    rows = []
    for mode, a, b in cases:
        rows.append("C %d %d %d" % (mode, len(a), len(b)))
        rows += ["%d %d %d %d" % r for r in a + b]
    return "\n".join(rows) + "\n"


@pytest.fixture(scope="module")
def merge_cases():
    cases = _cases()
    assert any(len(a) == 1025 and len(b) == 1025 for _, a, b in cases) and any(not a and not b for _, a, b in cases)
    return cases, _merge_input(cases)


def test_merge_rule_on_the_host(merge_cases):
    cases, text = merge_cases
    exe = _build("strand_host_driver", [])
    r = subprocess.run([exe, "merge"], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    _check_merge(r.stdout, cases)


def test_strand_rule_under_sanitizers(merge_cases):
    cases, text = merge_cases
    exe = _build("strand_host_driver_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "keys"] + _key_args(), capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    _check_keys(r.stdout)
    r = subprocess.run([exe, "merge"], input=text, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    _check_merge(r.stdout, cases)


# ---- the entries on the real library, without a GPU ----
def test_strand_symbols_exported(capi):
    L = capi.lib()
    for name in ("seeqdevPatternRevComp", "seeqdevScanRunStrands", "seeqdevScanHostStrands"):
        assert name in capi.EXPORTS
        assert hasattr(L, name), name


def test_strand_bit_is_free(capi):
    from seeq_amd import device as dev
    import re
    src = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    minus = int(re.search(r"#define\s+SEEQDEV_HIT_MINUS\s+(0x[0-9A-Fa-f]+)u", src).group(1), 16)
    max_wlen = int(re.search(r"#define\s+SEEQDEV_MAX_WLEN\s+(\d+)", src).group(1))
    assert minus == capi.SEEQDEV_HIT_MINUS == 1 << 31
    assert max_wlen - 1 == 511 and all(d & minus == 0 for d in range(max_wlen))       # a distance is below the pattern's length
    assert re.search(r"#define\s+SEEQDEV_HIT_DIST\(", src) and re.search(r"#define\s+SEEQDEV_HIT_STRAND\(", src)
    assert C.sizeof(capi.seeqdev_hit_t) == 16
    assert dev.STRAND_DTYPE.names == ("line", "start", "end", "dist", "strand")


def _einval(call):
    C.set_errno(0)
    assert call() == -1
    assert C.get_errno() == errno.EINVAL


def test_strand_argument_checks_without_a_device(capi):
    # The checks come before the device is touched: of the stand-in context and pattern only the device numbers are read.
    L = capi.lib()
    ctx = C.addressof(C.create_string_buffer(8192))
    keep = [C.create_string_buffer(1024), C.create_string_buffer(b"\x01" * 1024, 1024)]
    pat, foreign = C.addressof(keep[0]), C.addressof(keep[1])          # device 0 like the context's; some other device
    text = b"ACGT\n"
    cnt = capi.seeqdev_counts_t()
    per = (C.c_uint64 * 2)()
    for run, tx in ((L.seeqdevScanHostStrands, text), (L.seeqdevScanRunStrands, C.cast(C.c_char_p(text), C.c_void_p))):
        _einval(lambda: run(ctx, pat, tx, len(text), capi.SEEQDEV_SINGLELINE, 2, C.byref(cnt), per))
        _einval(lambda: run(ctx, pat, tx, len(text), capi.SQ_STREAM, 2, C.byref(cnt), per))
        _einval(lambda: run(ctx, pat, tx, len(text), capi.SQ_STREAM | capi.SQ_ALL, 0, C.byref(cnt), None))
        _einval(lambda: run(None, pat, tx, len(text), 0, 2, C.byref(cnt), per))                    # NULL context
        _einval(lambda: run(ctx, None, tx, len(text), 0, 2, C.byref(cnt), per))                    # NULL pattern
        _einval(lambda: run(ctx, pat, tx, len(text), 0, 2, None, per))                             # NULL counts
        _einval(lambda: run(ctx, pat, None, 5, 0, 2, C.byref(cnt), per))                           # NULL text with bytes
        _einval(lambda: run(ctx, pat, tx, len(text), 0, -1, C.byref(cnt), per))                    # want outside 0 .. 2
        _einval(lambda: run(ctx, pat, tx, len(text), 0, 3, C.byref(cnt), per))
        _einval(lambda: run(ctx, foreign, tx, len(text), 0, 2, C.byref(cnt), per))                 # a pattern on another device
        _einval(lambda: run(ctx, pat, tx, len(text), capi.SEEQDEV_FASTQ | capi.SEEQDEV_FASTA, 2, C.byref(cnt), per))   # as every scan entry
    C.set_errno(0)
    assert L.seeqdevPatternRevComp(None) is None and C.get_errno() == errno.EINVAL
