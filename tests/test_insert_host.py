"""CPU: the insert rule of seeq_amd/csrc/seeq_insert.h -- where a left record's walk over the right records starts and stops, which
right record is chosen, and which record an output byte of the insert text belongs to -- compiled for the host by plain g++
(tests/insert_host_driver.cpp) and compared with a brute-force join and a concatenation in Python.  Once more as a stand-alone program
under -fsanitize=address,undefined.  Then the entries on the real library: exports, the record's layout, and the argument checks, which
run before any device call and so fail the same way without a GPU."""
import ctypes as C
import errno
import os
import random
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "seeq_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "build")
SRC = os.path.join(ROOT, "tests", "insert_host_driver.cpp")
SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025]
WINDOWS = [(0, 0), (10, 14), (1, 0), (5, 5)]
FIRST, BEST = 0, 1


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    deps = [SRC, os.path.join(CSRC, "seeq_insert.h"), os.path.join(CSRC, "seeq_strand.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + ["-I" + CSRC, SRC, "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


# ---- the join ----
def _left_list(rng, n, lo, hi):
    """n records (line, start, end, dist), one per line, lines in [lo, hi)."""
    out = []
    for ln in sorted(rng.sample(range(lo, hi), n)):
        end = rng.randrange(8, 40)
        out.append((ln, max(0, end - rng.randrange(6, 9)), end, rng.randrange(0, 4)))
    return out


def _right_list(rng, lo, hi):
    """0 - 5 records on every line of [lo, hi): strictly increasing (line, end), starts that do not decrease and may repeat."""
    out = []
    for ln in range(lo, hi):
        prev = 0
        for end in sorted(rng.sample(range(7, 80), rng.randrange(0, 6))):
            start = max(prev, end - rng.randrange(6, 9))
            out.append((ln, start, end, rng.randrange(0, 4)))
            prev = start
    return out


def _cases():
    rng = random.Random(20251019)
    cases = []
    for mode in (FIRST, BEST):
        for lo, hi in WINDOWS:
            for nl in SIZES:
                span = max(4, nl + nl // 3)
                cases.append((mode, lo, hi, _left_list(rng, nl, 1, 1 + span), _right_list(rng, 1, 1 + span)))
            # right lists entirely below and entirely above the left lines, and none at all
            cases.append((mode, lo, hi, _left_list(rng, 65, 500, 700), _right_list(rng, 1, 400)))
            cases.append((mode, lo, hi, _left_list(rng, 65, 1, 200), _right_list(rng, 300, 700)))
            cases.append((mode, lo, hi, _left_list(rng, 65, 1, 200), []))
            # one line holding 3 000 right records among ordinary ones: a walk that crosses tiles of the right list
            long_line = [(50, 12 + i - 8 + (i % 3 == 0), 12 + i + 1, 1 + (i * 7) % 3 if i % 500 else 0) for i in range(8, 3008)]
            right = _right_list(rng, 1, 50) + long_line + _right_list(rng, 51, 100)
            left = _left_list(rng, 80, 1, 100)
            left = [r if r[0] != 50 else (50, 4, 15, 2) for r in left]
            if all(r[0] != 50 for r in left):
                left = sorted(left + [(50, 4, 15, 2)])
            cases.append((mode, lo, hi, left, right))
            # the sum L.end + min_len beyond 32 bits: nothing is admissible, whatever the window
            top = 0xFFFFFFF0
            cases.append((mode, 0x20, 0, [(3, top - 8, top, 1), (4, 2, 10, 0)],
                          [(3, top + 1, top + 9, 0), (3, top + 5, 0xFFFFFFFF, 1), (4, 0x30, 0x38, 0), (5, 1, 9, 0)]))
    return cases


def _expected(mode, lo, hi, left, right):
    """Per left record what k_insert_join stores: (line, start, end, ldist, rdist), or (0, has a right record, 0, 0, 0)."""
    by = {}
    for r in right:
        by.setdefault(r[0], []).append(r)
    out = []
    for ln, _, lend, ldist in left:
        adm = [r for r in by.get(ln, []) if r[1] >= lend + lo and (hi == 0 or r[1] <= lend + hi)]
        if adm:
            r = min(adm, key=(lambda r: (r[3], r[2])) if mode == BEST else (lambda r: r[2]))
            out.append((ln, lend, r[1], ldist, r[3]))
        else:
            out.append((0, 1 if ln in by else 0, 0, 0, 0))
    return out


def _join_input(cases):
    rows = []
    for mode, lo, hi, left, right in cases:
        rows.append("C %d %d %d %d %d" % (mode, lo, hi, len(left), len(right)))
        rows += ["%d %d %d %d" % r for r in left + right]
    return "\n".join(rows) + "\n"


def _check_join(out, cases):
    lines = out.split("\n")
    at = 0
    seen = dict(inserts=0, none=0)
    for mode, lo, hi, left, right in cases:
        assert lines[at] == "J %d" % len(left)
        got = [tuple(int(x) for x in ln.split()) for ln in lines[at + 1:at + 1 + len(left)]]
        at += 1 + len(left)
        exp = _expected(mode, lo, hi, left, right)
        assert got == exp, (mode, lo, hi, len(left), len(right), next((g, e) for g, e in zip(got, exp) if g != e))
        seen["inserts"] += sum(1 for r in exp if r[0])
        seen["none"] += sum(1 for r in exp if not r[0] and r[1])
    assert lines[at:] in ([], [""])
    assert seen["inserts"] > 1024 and seen["none"] > 1024


@pytest.fixture(scope="module")
def join_cases():
    cases = _cases()
    assert any(len(left) == 1025 for _, _, _, left, _ in cases) and any(not left for _, _, _, left, _ in cases)
    # the right lists are what the rule assumes: strictly increasing keys, starts that do not decrease within a line
    for _, _, _, left, right in cases:
        assert all((a[0], a[2]) < (b[0], b[2]) and (a[0] != b[0] or a[1] <= b[1]) for a, b in zip(right, right[1:]))
        assert all(a[0] < b[0] for a, b in zip(left, left[1:]))
    # the long line: under SQ_BEST its chosen record is not its first admissible one, and the saturating case has right records on its line
    mode, lo, hi, left, right = next(c for c in cases if c[0] == BEST and (c[1], c[2]) == (0, 0) and sum(1 for r in c[4] if r[0] == 50) == 3000)
    exp = dict((r[0], r) for r in _expected(mode, lo, hi, left, right))[50]
    first = min(r[2] for r in right if r[0] == 50 and r[1] >= 15)
    assert exp[2] != min(r[1] for r in right if r[0] == 50 and r[2] == first) and exp[4] == 0
    return cases, _join_input(cases)


def test_join_rule_on_the_host(join_cases):
    cases, text = join_cases
    exe = _build("insert_host_driver", [])
    r = subprocess.run([exe, "join"], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    _check_join(r.stdout, cases)
    tile, wg, items, run, rec = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()[1:]]
    assert tile == wg * items == 1024 and wg % 64 == 0 and run == 16 and rec == 16


# ---- the insert text ----
def _text_cases():
    rng = random.Random(77)
    cases = []
    for n in (0, 1, 2, 15, 16, 17, 300):
        lines = ["".join(rng.choice("ACGT") for _ in range(rng.randrange(1, 90))) for _ in range(n + 1)]
        text = "\n".join(lines) + "\n"
        offs, pos = [], 0
        for ln in lines:
            offs.append(pos)
            pos += len(ln) + 1
        recs = []
        for k in range(n):
            m = len(lines[k])
            kind = rng.randrange(4)
            start = rng.randrange(0, m + 1)
            end = start if kind == 0 else rng.randrange(start, m + 1)       # a quarter of the inserts (and more) are empty
            if kind == 1 and m > 40:
                start, end = 0, m                                           # a long one: several runs of 16 bytes
            recs.append((start, end, offs[k]))
        cases.append((text, recs, 0))
    # empty inserts only; one insert of exactly 15 bytes (with its newline: one run); a record beyond the text
    text = "ACGTACGTACGTACGTACGT\n"
    cases.append((text, [(3, 3, 0)] * 40, 0))
    cases.append((text, [(2, 17, 0)], 0))
    cases.append((text, [(2, 6, 0), (4, 30, 0), (1, 3, 0)], 1))
    cases.append((text, [(2, 6, 0), (4, 10, 15)], 1))
    return cases


def _text_input(cases):
    rows = []
    for text, recs, _ in cases:
        rows.append("T %d %d" % (len(recs), len(text)))
        rows.append(text.replace("\n", "|"))
        rows += ["%d %d %d" % r for r in recs]
    return "\n".join(rows) + "\n"


def _check_text(out, cases):
    lines = out.split("\n")
    at = 0
    empties = 0
    for text, recs, bad in cases:
        cut = [text[o + s:o + e] for s, e, o in recs]
        total = sum(e - s + 1 for s, e, _ in recs)
        assert lines[at] == "X %d" % total
        mapping = [tuple(int(x) for x in ln.split()) for ln in lines[at + 1:at + 1 + total]]
        assert mapping == [(k, i if i < e - s else -1) for k, (s, e, _) in enumerate(recs) for i in range(e - s + 1)]
        at += 1 + total
        assert lines[at] == "B %d" % bad
        if not bad:
            assert lines[at + 1] == "".join(c + "|" for c in cut)
        empties += sum(1 for s, e, _ in recs if s == e)
        at += 2
    assert lines[at:] in ([], [""])
    assert empties > 60


def test_insert_text_mapping_on_the_host():
    cases = _text_cases()
    exe = _build("insert_host_driver", [])
    r = subprocess.run([exe, "text"], input=_text_input(cases), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    _check_text(r.stdout, cases)


def test_insert_rule_under_sanitizers(join_cases):
    cases, text = join_cases
    exe = _build("insert_host_driver_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "join"], input=text, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    _check_join(r.stdout, cases)
    tcases = _text_cases()
    r = subprocess.run([exe, "text"], input=_text_input(tcases), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    _check_text(r.stdout, tcases)


# ---- the entries on the real library, without a GPU ----
INSERT_SYMBOLS = ("seeqdevScanRunInserts", "seeqdevScanHostInserts", "seeqdevScanInsertsDevice", "seeqdevScanCopyInserts",
                  "seeqdevScanCopyInsertOffsets", "seeqdevScanInsertText", "seeqdevScanLastInsertsMs")


def test_insert_symbols_exported(capi):
    L = capi.lib()
    for name in INSERT_SYMBOLS:
        assert name in capi.EXPORTS
        assert hasattr(L, name), name


def test_insert_record_layout(capi):
    from seeq_amd import device as dev
    assert C.sizeof(capi.seeqdev_insert_t) == 16 and capi.seeqdev_insert_t.line.offset == 0
    assert C.sizeof(capi.seeqdev_insert_counts_t) == 48
    assert dev.INSERT_DTYPE.names == ("line", "start", "end", "ldist", "rdist") and dev.INSERT_DTYPE.itemsize == 16
    assert [dev.INSERT_DTYPE.fields[f][1] for f in dev.INSERT_DTYPE.names] == [getattr(capi.seeqdev_insert_t, f).offset for f in dev.INSERT_DTYPE.names]


def _einval(call):
    C.set_errno(0)
    assert call() == -1
    assert C.get_errno() == errno.EINVAL


def test_insert_argument_checks_without_a_device(capi):
    # The checks come before the device is touched: of the stand-in context and patterns only the device numbers are read.
    L = capi.lib()
    ctx = C.addressof(C.create_string_buffer(8192))
    keep = [C.create_string_buffer(1024), C.create_string_buffer(1024), C.create_string_buffer(b"\x01" * 1024, 1024)]
    left, right, foreign = (C.addressof(k) for k in keep)               # device 0 like the context's, twice; some other device
    text = b"ACGT\n"
    cnt = capi.seeqdev_insert_counts_t()
    ok = C.byref(cnt)
    for run, tx in ((L.seeqdevScanHostInserts, text), (L.seeqdevScanRunInserts, C.cast(C.c_char_p(text), C.c_void_p))):
        _einval(lambda: run(ctx, left, right, tx, len(text), capi.SQ_ALL, 0, 0, ok))                     # every occurrence of the left flank
        _einval(lambda: run(ctx, left, right, tx, len(text), capi.SQ_COUNT, 0, 0, ok))
        _einval(lambda: run(ctx, left, right, tx, len(text), capi.SQ_BEST | capi.SEEQDEV_SINGLELINE, 0, 0, ok))
        _einval(lambda: run(ctx, left, right, tx, len(text), capi.SQ_BEST | capi.SQ_STREAM, 0, 0, ok))   # an input-mode bit
        _einval(lambda: run(None, left, right, tx, len(text), capi.SQ_BEST, 0, 0, ok))                   # NULL context
        _einval(lambda: run(ctx, None, right, tx, len(text), capi.SQ_BEST, 0, 0, ok))                    # NULL patterns
        _einval(lambda: run(ctx, left, None, tx, len(text), capi.SQ_BEST, 0, 0, ok))
        _einval(lambda: run(ctx, left, right, tx, len(text), capi.SQ_BEST, 0, 0, None))                  # NULL counts
        _einval(lambda: run(ctx, left, right, None, 5, capi.SQ_BEST, 0, 0, ok))                          # NULL text with bytes
        _einval(lambda: run(ctx, left, right, tx, len(text), capi.SQ_BEST, 15, 14, ok))                  # min_len > max_len != 0
        _einval(lambda: run(ctx, left, right, tx, len(text), capi.SQ_FIRST, 0xFFFFFFFF, 1, ok))
        _einval(lambda: run(ctx, foreign, right, tx, len(text), capi.SQ_BEST, 0, 0, ok))                 # a pattern on another device
        _einval(lambda: run(ctx, left, foreign, tx, len(text), capi.SQ_BEST, 0, 0, ok))
        _einval(lambda: run(ctx, left, left, tx, len(text), capi.SQ_BEST | capi.SEEQDEV_FASTQ | capi.SEEQDEV_FASTA, 0, 0, ok))
    got = C.c_uint64(7)
    _einval(lambda: L.seeqdevScanInsertText(None, None, 0, None, 0, C.byref(got)))
    _einval(lambda: L.seeqdevScanInsertText(ctx, None, 0, None, 0, None))
    assert L.seeqdevScanInsertText(ctx, None, 0, None, 0, C.byref(got)) == 0 and got.value == 0          # the size query of a context without a result
    _einval(lambda: L.seeqdevScanCopyInserts(ctx, None, 0, 1))
    _einval(lambda: L.seeqdevScanCopyInsertOffsets(None, None, 0, 0))
    assert L.seeqdevScanInsertsDevice(None) is None
    _einval(lambda: L.seeqdevScanLastInsertsMs(ctx, None))
