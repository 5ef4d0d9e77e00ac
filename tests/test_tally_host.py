"""CPU: the tally rule of seeq_amd/csrc/seeq_tally.h -- a span's key, a key's bases, the digit a pass sorts by, the pass count, the run
heads -- compiled for the host by plain g++ (tests/tally_host_driver.cpp) and compared with a restatement in Python.  Once more as a
stand-alone program under -fsanitize=address,undefined.  Then the entries on the real library: exports, the entry's layout, the two
host functions, and the argument checks, which run before any device call and so fail the same way without a GPU."""
import collections
import ctypes as C
import errno
import os
import random
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "seeq_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "build")
SRC = os.path.join(ROOT, "tests", "tally_host_driver.cpp")
OK, LONG, FOREIGN, BAD = 0, 1, 2, 3
BASES = b"ACGTUacgtu"


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    deps = [SRC, os.path.join(CSRC, "seeq_tally.h"), os.path.join(CSRC, "seeq_strand.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + ["-I" + CSRC, SRC, "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


# ---- the rule, restated ----
def py_key(seq):
    """bytes -> (kind, key): the length is decided first, then the bytes."""
    if len(seq) > 31:
        return LONG, 0
    if any(c not in BASES for c in seq):
        return FOREIGN, 0
    key = 1
    for c in seq:
        key = (key << 2) | ((c >> 1) & 3)
    return OK, key


def py_decode(key):
    n = (key.bit_length() - 1) // 2
    return "".join("ACTG"[(key >> (2 * (n - 1 - i))) & 3] for i in range(n))


def py_order(seq):
    """What the table is ordered by: the length, then the bases with A < C < T < G."""
    return len(seq), seq.upper().replace(b"U", b"T").translate(bytes.maketrans(b"ACTG", b"0123"))


def _span_cases():
    """(text, nbytes, off, start, end, expected kind, expected key, expected len)"""
    rng = random.Random(20251020)
    seqs = []
    for n in range(0, 32):                                  # every length that has a key
        seqs += [bytes(rng.choice(b"ACGT") for _ in range(n)) for _ in range(3)]
    seqs += [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in (32, 40)]
    seqs += [bytes([c]) for c in BASES] + [BASES, BASES * 3, b"G" * 31, b"A" * 31, b"T" * 31, b"u" * 31]
    for n in (1, 12, 31, 32, 40):                           # N, newline, byte 0x80 at the first, a middle and the last position
        for bad in (b"N", b"\n", b"\x80", b"n", b"@", b"\x00"):
            for at in sorted({0, n // 2, n - 1}):
                s = bytearray(rng.choice(b"ACGT") for _ in range(n))
                s[at:at + 1] = bad
                seqs.append(bytes(s))
    cases = []
    for k, s in enumerate(seqs):
        head = bytes(rng.choice(b"ACGTN\n") for _ in range(k % 7))
        tail = b"" if k % 3 == 0 else bytes(rng.choice(b"ACGTN\n") for _ in range(1 + k % 5))      # every third span ends with the text
        text = head + s + tail
        off = rng.randrange(0, len(head) + 1)
        kind, key = py_key(s)
        cases.append((text, len(text), off, len(head) - off, len(head) - off + len(s), kind, key, len(s)))
    text = b"ACGTACGTACGTACGTACGT\n"
    n = len(text)
    cases += [(text, n, 0, 5, 4, BAD, 0, 0),                # end < start
              (text, n, 0, 0, n + 1, BAD, 0, 0),            # beyond the text
              (text, n - 4, 0, n - 8, n - 3, BAD, 0, 0),    # beyond the nbytes given, inside the buffer
              (text, n, n - 2, 0, 3, BAD, 0, 0),
              (text, n, n + 1, 0, 0, BAD, 0, 0),            # the line itself lies beyond the text
              (text, n, 2 ** 40, 0, 0, BAD, 0, 0),
              (text, n, 0, 0xFFFFFFF0, 0xFFFFFFFF, BAD, 0, 0),
              (text, n, n, 0, 0, OK, 1, 0),                 # the empty span at the very end
              (b"", 0, 0, 0, 0, OK, 1, 0),
              (text, n, 1, n - 1, n - 1, OK, 1, 0),
              (text, n - 1, 0, n - 5, n - 1, OK, py_key(b"ACGT")[1], 4)]
    return cases


def _span_input(cases):
    return "".join("S %s %d %d %d %d\n" % (c[0].hex() or "-", c[1], c[2], c[3], c[4]) for c in cases)


def _check_spans(out, cases):
    lines = out.split("\n")
    assert lines[len(cases):] in ([], [""])
    seen = collections.Counter()
    for row, (text, nbytes, off, start, end, kind, key, length) in zip(lines, cases):
        f = row.split()
        what = (text[off + start:off + end] if kind != BAD else None, row)
        assert (int(f[0]), int(f[1], 16), int(f[2])) == (kind, key, length if kind != BAD else 0), what
        seen[kind] += 1
        if kind == OK:
            s = text[off + start:off + end]
            assert f[3] == (py_decode(key) or "-") == (s.upper().replace(b"U", b"T").decode() or "-"), what
            assert int(f[4], 16) == key, what               # encode -> decode -> encode
            assert key >> 63 == 0 and key.bit_length() == 2 * len(s) + 1, what
    assert seen[OK] > 100 and seen[LONG] > 30 and seen[FOREIGN] > 40 and seen[BAD] == 7
    return seen


def test_the_restatement_itself():
    """The properties the issue states, on the Python side: the order of keys is the order of (length, bases with A < C < T < G); the
    extreme keys; a span that is both long and foreign is long."""
    rng = random.Random(5)
    seqs = {bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(0, 32))) for _ in range(3000)} | {b"", b"G" * 31, b"A" * 31}
    keyed = sorted(seqs, key=lambda s: py_key(s)[1])
    assert keyed == sorted(seqs, key=py_order)
    assert py_key(b"G" * 31) == (OK, (1 << 63) - 1) and py_key(b"A" * 31) == (OK, 1 << 62) and py_key(b"") == (OK, 1)
    assert py_key(b"acgu") == py_key(b"ACGT") == (OK, 0b1_00_01_11_10)
    assert py_key(b"N" * 40)[0] == LONG and py_key(b"N" * 31)[0] == FOREIGN
    assert all(py_decode(py_key(s)[1]) == s.decode() for s in seqs)


def test_span_rule_on_the_host():
    cases = _span_cases()
    exe = _build("tally_host_driver", [])
    r = subprocess.run([exe, "span"], input=_span_input(cases), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    _check_spans(r.stdout, cases)
    f = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()[1:]]
    tile, wg, items, radix, chunk, longest = f[:6]
    assert tile == wg * items == chunk == 1024 and wg % 64 == 0 and radix == wg == 256 and longest == 31
    assert f[6:] == [1, 256, 1, 1, 256, 1, 2, 512, 1, 5, 1280, 2]      # tiles, matrix entries, scan chunks of 1, 1024, 1025, 4100 spans
    hdr = open(os.path.join(CSRC, "seeq_tally.h")).read()
    assert int(re.search(r"#define\s+SEEQ_TALLY_TILE\s+(\d+)", hdr).group(1)) == tile


# ---- the sort as the host drives it, and the run heads ----
def _table_cases():
    rng = random.Random(99)
    mk = lambda n: py_key(bytes(rng.choice(b"ACGT") for _ in range(n)))[1]      # noqa: E731
    cases = [[], [0], [0, 0, 0], [1], [1, 1, 0, 1]]
    for longest, passes in ((3, 1), (4, 2), (12, 4), (31, 8)):
        pool = [mk(rng.randrange(0, longest + 1)) for _ in range(40)] + [mk(longest)]
        cases.append([rng.choice(pool + [0]) for _ in range(700)])
    cases.append([mk(31) for _ in range(300)])                                   # all distinct
    lo = py_key(b"ACGTACGTACGT")[1]
    cases.append([lo ^ rng.randrange(4) for _ in range(500)])                    # keys that differ in the lowest digit only
    cases.append([lo ^ (rng.randrange(2) << 23) for _ in range(500)])            # ... in the highest used digit only
    cases.append([(1 << 63) - 1, 1 << 62] * 100)
    return cases


def _table_expected(keys):
    longest = max([(k.bit_length() - 1) // 2 for k in keys if k], default=0)
    tab = sorted(collections.Counter(k for k in keys if k).items())
    return (2 * longest + 1 + 7) // 8, tab


def _check_table(out, cases):
    lines = out.split("\n")
    at = 0
    seen = set()
    for keys in cases:
        passes, tab = _table_expected(keys)
        assert lines[at] == "P %d" % passes and lines[at + 1] == "T %d" % len(tab), (lines[at:at + 2], passes, len(tab))
        got = [(int(a, 16), int(b)) for a, b in (ln.split() for ln in lines[at + 2:at + 2 + len(tab)])]
        assert got == tab
        assert sum(c for _, c in got) == sum(1 for k in keys if k)
        at += 2 + len(tab)
        seen.add(passes)
    assert lines[at:] in ([], [""])
    assert {1, 2, 4, 8} <= seen


def test_sort_and_run_heads_on_the_host():
    cases = _table_cases()
    exe = _build("tally_host_driver", [])
    text = "".join("N %d\n%s\n" % (len(k), " ".join("%x" % x for x in k)) for k in cases)
    r = subprocess.run([exe, "table"], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    _check_table(r.stdout, cases)


def test_tally_rule_under_sanitizers():
    exe = _build("tally_host_driver_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    cases = _span_cases()
    r = subprocess.run([exe, "span"], input=_span_input(cases), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    _check_spans(r.stdout, cases)
    tcases = _table_cases()
    text = "".join("N %d\n%s\n" % (len(k), " ".join("%x" % x for x in k)) for k in tcases)
    r = subprocess.run([exe, "table"], input=text, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    _check_table(r.stdout, tcases)


# ---- the entries on the real library, without a GPU ----
TALLY_SYMBOLS = ("seeqdevScanTally", "seeqdevScanTallyDevice", "seeqdevScanCopyTally", "seeqdevScanLastTallyMs", "seeqdevTallyKey",
                 "seeqdevTallyDecode")


def test_tally_symbols_exported(capi):
    L = capi.lib()
    for name in TALLY_SYMBOLS:
        assert name in capi.EXPORTS
        assert hasattr(L, name), name


def test_tally_entry_layout(capi):
    from seeq_amd import device as dev
    assert C.sizeof(capi.seeqdev_tally_t) == 16 and capi.seeqdev_tally_t.key.offset == 0 and capi.seeqdev_tally_t.count.offset == 8
    assert C.sizeof(capi.seeqdev_tally_counts_t) == 48
    assert dev.TALLY_DTYPE.names == ("key", "count") and dev.TALLY_DTYPE.itemsize == 16
    assert (capi.SEEQDEV_TALLY_INSERTS, capi.SEEQDEV_TALLY_HITS, capi.SEEQDEV_TALLY_MAX_LEN) == (0, 1, 31)
    hdr = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    for name, value in (("SEEQDEV_TALLY_INSERTS", 0), ("SEEQDEV_TALLY_HITS", 1), ("SEEQDEV_TALLY_MAX_LEN", 31)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == value


def _einval(call):
    C.set_errno(0)
    assert call() == -1
    assert C.get_errno() == errno.EINVAL


def test_tally_key_and_decode_on_the_library(capi):
    from seeq_amd import device as dev
    L = capi.lib()
    rng = random.Random(3)
    seqs = [bytes(rng.choice(BASES) for _ in range(n)) for n in range(0, 32) for _ in range(4)] + [b"G" * 31, b"A" * 31]
    for s in seqs:
        key = C.c_uint64(0)
        assert L.seeqdevTallyKey(s, len(s), C.byref(key)) == 0 and key.value == py_key(s)[1], s
        out = C.create_string_buffer(b"\xff" * 32, 32)
        assert L.seeqdevTallyDecode(key.value, out) == len(s)
        assert out.raw[:len(s) + 1] == s.upper().replace(b"U", b"T") + b"\0"
        assert dev.tally_key(s) == key.value and dev.tally_key(s.decode()) == key.value
        assert dev.tally_decode(key.value) == py_decode(key.value)
    assert dev.tally_key("G" * 31) == (1 << 63) - 1 and dev.tally_key("A" * 31) == 1 << 62 and dev.tally_key("") == 1
    key = C.c_uint64(7)
    for s in (b"A" * 32, b"A" * 40, b"ACGN", b"N", b"AC\nT", b"\x80CGT", b"ACG\x80", b"N" * 40):
        _einval(lambda: L.seeqdevTallyKey(s, len(s), C.byref(key)))
        with pytest.raises(ValueError):
            dev.tally_key(s)
    assert key.value == 7                                   # nothing is written on a refusal
    _einval(lambda: L.seeqdevTallyKey(b"ACGT", 4, None))
    _einval(lambda: L.seeqdevTallyKey(None, 4, C.byref(key)))
    out = C.create_string_buffer(32)
    for bad in (0, 1 << 63, (1 << 64) - 1, 2, 0b1000):      # no key, bit 63, a leading 1 at an odd bit
        _einval(lambda: L.seeqdevTallyDecode(bad, out))
        with pytest.raises(ValueError):
            dev.tally_decode(bad)
    _einval(lambda: L.seeqdevTallyDecode(1, None))


def test_tally_lookup_is_a_search_over_the_table():
    import numpy as np
    from seeq_amd import device as dev
    seqs = ["", "A", "G", "ACGT", "ACGTTGCAAGCT", "G" * 31]
    keys = np.array(sorted(dev.tally_key(s) for s in seqs), dtype=np.uint64)
    res = dict(keys=keys, counts=np.arange(10, 10 + len(keys), dtype=np.uint64))
    by = {int(k): int(c) for k, c in zip(res["keys"], res["counts"])}
    ask = ["G" * 31, "acgu", "ACGA", "", "T", "A" * 31, "C" * 30, "ACGTTGCAAGCT"]
    assert dev.tally_lookup(res, ask).tolist() == [by.get(dev.tally_key(s), 0) for s in ask]
    assert dev.tally_lookup(dict(keys=keys[:0], counts=keys[:0]), ask).tolist() == [0] * len(ask)
    assert dev.tally_lookup(res, []).tolist() == []
    with pytest.raises(ValueError):
        dev.tally_lookup(res, ["ACGN"])


def test_tally_argument_checks_without_a_device(capi):
    # The checks come before the device is touched: the stand-in context is all zeros -- no completed inserts call, nothing fetched.
    L = capi.lib()
    ctx = C.addressof(C.create_string_buffer(8192))
    text = C.cast(C.c_char_p(b"ACGT\n"), C.c_void_p)
    cnt = capi.seeqdev_tally_counts_t()
    ok = C.byref(cnt)
    for source in (capi.SEEQDEV_TALLY_INSERTS, capi.SEEQDEV_TALLY_HITS):
        _einval(lambda: L.seeqdevScanTally(None, source, text, 5, ok))                # NULL context
        _einval(lambda: L.seeqdevScanTally(ctx, source, text, 5, None))               # NULL counts
        _einval(lambda: L.seeqdevScanTally(ctx, source, None, 5, ok))                 # NULL text with bytes
        _einval(lambda: L.seeqdevScanTally(ctx, source, text, 5, ok))                 # no completed inserts call / nothing fetched
        _einval(lambda: L.seeqdevScanTally(ctx, source, None, 0, ok))                 # ... and no staged text / hits without text
    for source in (2, -1, 255):
        _einval(lambda: L.seeqdevScanTally(ctx, source, text, 5, ok))                 # an unknown source
    _einval(lambda: L.seeqdevScanCopyTally(None, None, 0, 0))
    _einval(lambda: L.seeqdevScanCopyTally(ctx, None, 0, 1))
    out = (capi.seeqdev_tally_t * 2)()
    _einval(lambda: L.seeqdevScanCopyTally(ctx, out, 0, 1))                           # a context without a table has no entry
    _einval(lambda: L.seeqdevScanCopyTally(ctx, out, 1, 0))
    assert L.seeqdevScanCopyTally(ctx, out, 0, 0) == 0
    assert L.seeqdevScanTallyDevice(None) is None and L.seeqdevScanTallyDevice(ctx) is None
    ms = C.c_float(1.0)
    _einval(lambda: L.seeqdevScanLastTallyMs(ctx, None))
    _einval(lambda: L.seeqdevScanLastTallyMs(None, C.byref(ms)))
    assert L.seeqdevScanLastTallyMs(ctx, C.byref(ms)) == 0 and ms.value == 0.0
