"""CPU: the base-quality rule of seeq_amd/csrc/seeq_qgate.h -- where a span's quality bytes lie, whether the record fits, how many of them
are low -- compiled for the host by plain g++ (tests/qgate_host_driver.cpp) and compared with a restatement in Python that finds the
lines with bytes.find and shares no code with it.  The driver runs every span through the rule byte by byte AND through the decision as
the kernel takes it (the walk in steps of 64 bytes, the wide loads) and fails where they differ.  Once more as a stand-alone program
under -fsanitize=address,undefined.  Then the entries on the real library: exports, the struct's layout, every refusal of the gate and
of the five tally entries for SEEQDEV_TALLY_GATED without a completed gate (which come before any device call and so fail the same way
without a GPU)."""
import ctypes as C
import errno
import functools
import os
import random
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "seeq_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "build")
SRC = os.path.join(ROOT, "tests", "qgate_host_driver.cpp")
PASS, LOW, LONG, FAR, MISFIT, BAD = range(6)
KIND_NAMES = ("pass", "low", "long", "far", "misfit", "bad")
MAX_LEN, REACH_MAX = 31, 65536
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("seeq_qgate.h", "seeq_tally.h", "seeq_strand.h", "seeq_tiles.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + ["-I" + CSRC, SRC, "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe, mode, text, env=None):
    r = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r.stdout.split("\n")


# ---- the rule, restated ----
def py_gate(text, off, start, end, min_qual=20, base=33, max_low=0, reach=1024):
    """(kind, low bytes) of the span [start, end) of the line at `off` in `text` (bytes), by the rule of seeq_qgate.h."""
    n = len(text)
    if end < start or off > n or end > n - off:
        return BAD, 0
    if end - start > MAX_LEN:
        return LONG, 0
    p = off + end
    window = text[p:min(n, p + reach)]
    e1 = window.find(b"\n")
    e2 = window.find(b"\n", e1 + 1) if e1 >= 0 else -1
    if e2 < 0:
        return (FAR if p + reach < n else MISFIT), 0
    q0, seqlen = p + e2 + 1, p + e1 - off
    if q0 + seqlen > n or (q0 + seqlen < n and text[q0 + seqlen:q0 + seqlen + 1] != b"\n"):
        return MISFIT, 0
    low = sum(1 for b in text[q0 + start:q0 + end] if b < base + min_qual)
    return (LOW if low > max_low else PASS), low


def py_gate_all(text, records, offsets, **kw):
    """The gate over rows of (line, start, end, ...) with their line offsets -> (kinds, counts dict)."""
    kinds, low_bases = [], 0
    for r, off in zip(records, offsets):
        kind, low = py_gate(text, int(off), int(r[1]), int(r[2]), **kw)
        assert kind != BAD
        kinds.append(kind)
        low_bases += low
    cnt = dict(nspans=len(kinds), npassed=kinds.count(PASS), nlow=kinds.count(LOW), nlong=kinds.count(LONG), nfar=kinds.count(FAR),
               nmisfit=kinds.count(MISFIT), low_bases=low_bases)
    return kinds, cnt


# ---- cases ----
def _bases(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _quals(rng, n, lo=33, hi=74):
    return bytes(rng.randrange(lo, hi) for _ in range(n))


class Text:
    """FASTQ text put together record by record; seq_off: the offsets of the sequence lines."""

    def __init__(self):
        self.buf, self.seq_off = bytearray(), []

    def add(self, seq, qual, plus=b"+", head=b"@r", newline=True):
        self.buf += head + b"\n"
        self.seq_off.append(len(self.buf))
        self.buf += seq + b"\n" + plus + b"\n" + qual + (b"\n" if newline else b"")
        return self.seq_off[-1]


DISTANCES = (0, 15, 16, 17, 63, 64, 65, 255, 256, 257)
PLUS_LENS = (1, 2, 16, 17, 70)
SPAN_LENS = (0, 1, 16, 17, 31, 32)


@functools.lru_cache(maxsize=None)
def _cases():
    """-> list of (text, [(what, off, start, end, min_qual, base, max_low, reach)])."""
    rng = random.Random(20)
    out = []
    # every distance from the span's end to the end of its line x every '+' line length, the span 12 bytes at 5; e2 at exactly
    # p + reach - 1 (decided) and at p + reach (FAR: the text goes on)
    t, spans = Text(), []
    for d in DISTANCES:
        for pl in PLUS_LENS:
            n = 17 + d
            off = t.add(_bases(rng, n), _quals(rng, n), b"+" + _bases(rng, pl - 1))
            spans.append(("d%d plus%d" % (d, pl), off, 5, 17, 20, 33, 2, 1024))
            spans.append(("d%d plus%d reach to e2" % (d, pl), off, 5, 17, 20, 33, 2, d + pl + 2))
            spans.append(("d%d plus%d reach short of e2" % (d, pl), off, 5, 17, 20, 33, 2, d + pl + 1))
    out.append((bytes(t.buf), spans))
    # span lengths, start == 0, end == the line's length, on lines of 40 and of 32 bytes; thresholds
    t, spans = Text(), []
    for n in (40, 32, 31):
        off = t.add(_bases(rng, n), _quals(rng, n))
        for ln in SPAN_LENS:
            if ln <= n:
                spans += [("len%d at 0 of %d" % (ln, n), off, 0, ln, 20, 33, 1, 1024), ("len%d at the end of %d" % (ln, n), off, n - ln, n, 20, 33, 1, 1024)]
    for base in (33, 64):
        thr = base + 20
        q = bytearray([thr + 5] * 30)
        q[7], q[9], q[12], q[20] = thr, thr - 1, base - 3, thr - 1        # at the bar: passes; one below: low; below base: low
        off = t.add(_bases(rng, 30), bytes(q))
        for max_low in (0, 1, 2):
            spans += [("base%d bar" % base, off, 5, 9, 20, base, max_low, 1024),          # holds the byte at the bar alone: 0 low
                      ("base%d one" % base, off, 5, 10, 20, base, max_low, 1024),         # ... and the one below it: 1 low
                      ("base%d two" % base, off, 5, 13, 20, base, max_low, 1024),         # 2 low
                      ("base%d three" % base, off, 5, 21, 20, base, max_low, 1024)]       # 3 low
    # a quality line shorter than its sequence line whose successor happens to end where it should: the '\n' is a low byte
    off = t.add(_bases(rng, 20), b"I" * 10, newline=True)
    t.buf += b"@hdr12345\n"                                 # q0 + 20 is this newline
    spans += [("newline in the span", off, 5, 15, 20, 33, 0, 1024), ("newline in the span, allowed", off, 5, 15, 20, 33, 1, 1024),
              ("before the newline", off, 2, 10, 20, 33, 0, 1024)]
    off = t.add(_bases(rng, 25), _quals(rng, 25))
    spans += [("bad: end < start", off, 9, 8, 20, 33, 0, 1024), ("bad: beyond the text", off, 0, len(t.buf), 20, 33, 0, 1024),
              ("bad: offset beyond the text", len(t.buf) + 1, 0, 0, 20, 33, 0, 1024), ("empty at the very end", len(t.buf), 0, 0, 20, 33, 0, 1024)]
    out.append((bytes(t.buf), spans))
    # the last record: without a trailing newline; cut after the sequence line, after the '+' line, in the middle of the quality line;
    # short lines, so that the quality bytes lie in the text's last 32 bytes
    for n in (12, 31, 50):
        t = Text()
        t.add(_bases(rng, 45), _quals(rng, 45))
        off = t.add(_bases(rng, n), _quals(rng, n, 50, 60), newline=False)
        whole = bytes(t.buf)
        at_seq, at_plus = off + n + 1, off + n + 3
        for what, cut in (("whole", len(whole)), ("after the sequence line", at_seq), ("after the + line", at_plus), ("mid quality", at_plus + n // 2),
                          ("one short", len(whole) - 1), ("mid sequence", off + n - 2)):
            spans = [("%s, line of %d, reach %d" % (what, n, reach), off, 2, min(n, 14) - 2, 20, 33, 0, reach) for reach in (1024, 3, n + 2)]
            spans.append(("%s, line of %d, to its end" % (what, n), off, max(0, n - 31), n, 25, 33, 1, 64))
            out.append((whole[:cut], spans))
    return out


def _fuzz_case(seed):
    """A random text of lines of random lengths (so that records fit or do not), cut at a random place; random spans and reaches."""
    rng = random.Random(seed)
    t = Text()
    for _ in range(rng.randrange(1, 12)):
        n = rng.choice((0, 1, 5, 20, 33, 64, 100, 150, 300))
        qn = n if rng.random() < 0.8 else max(0, n + rng.randrange(-3, 4))
        t.add(_bases(rng, n), _quals(rng, qn), b"+" + _bases(rng, rng.choice((0, 0, 0, 1, 15, 69))), newline=rng.random() < 0.9)
    text = bytes(t.buf)
    if rng.random() < 0.5:
        text = text[:rng.randrange(len(text) + 1)]
    spans = []
    for _ in range(60):
        off = rng.choice(t.seq_off) if rng.random() < 0.9 else rng.randrange(len(text) + 2)
        start = rng.randrange(0, 40)
        end = start + rng.choice((0, 1, 8, 16, 17, 31, 32)) if rng.random() < 0.95 else max(0, start - 1)
        spans.append(("fuzz", off, start, end, rng.choice((0, 10, 20, 30, 41)), rng.choice((33, 64)), rng.choice((0, 1, 2, 31)),
                      rng.choice((1, 2, 63, 64, 65, 128, 200, 1024, REACH_MAX))))
    return text, spans


def _input(cases):
    return "".join("T %d %s\n%s" % (len(text), text.hex(), "".join("S %d %d %d %d %d %d\n" % (off, st, en, base + mq, ml, reach)
                                                                  for _, off, st, en, mq, base, ml, reach in spans)) for text, spans in cases)


def _check(exe, cases, env=None):
    lines = _run(exe, "gate", _input(cases), env)
    got = [tuple(int(x) for x in ln.split()) for ln in lines if ln]
    exp, names = [], []
    for text, spans in cases:
        for what, off, st, en, mq, base, ml, reach in spans:
            exp.append(py_gate(text, off, st, en, mq, base, ml, reach))
            names.append((what, off, st, en, mq, base, ml, reach, len(text)))
    assert len(got) == len(exp)
    bad = [(names[i], g, exp[i]) for i, g in enumerate(got) if g != exp[i]]
    assert not bad, (len(bad), bad[:5])
    return dict(zip([n[0] for n in names], exp)), {k for k, _ in exp}


def test_the_restatement_itself():
    text = b"@a\nACGTACGTAC\n+\nIIII4IIIII\n@b\nACGT\n+x\nII\n"
    assert py_gate(text, 3, 2, 6) == (LOW, 1) and py_gate(text, 3, 2, 6, max_low=1) == (PASS, 1) and py_gate(text, 3, 5, 9) == (PASS, 0)
    assert py_gate(text, 3, 2, 6, min_qual=19) == (PASS, 0) and py_gate(text, 3, 2, 6, min_qual=20, base=32) == (PASS, 0)      # '4' is 52 = 33 + 19
    assert py_gate(text, 3, 3, 3) == (PASS, 0) and py_gate(text, 3, 0, 10) == (LOW, 1)
    assert py_gate(text, 3, 6, 5)[0] == BAD and py_gate(text, len(text) + 1, 0, 0)[0] == BAD and py_gate(text, 3, 0, len(text))[0] == BAD
    assert py_gate(text, 3, 0, 4, reach=9) == (PASS, 0) and py_gate(text, 3, 0, 4, reach=8)[0] == FAR      # e2 at p + 8
    assert py_gate(text, 30, 0, 4)[0] == MISFIT             # the quality line of the second record is too short
    assert py_gate(text[:37], 30, 0, 4)[0] == MISFIT and py_gate(text[:37], 30, 0, 4, reach=2)[0] == FAR
    assert py_gate(b"ACGT\n+\nIIII", 0, 0, 4) == (PASS, 0) and py_gate(b"ACGT\n+\nIII", 0, 0, 4)[0] == MISFIT
    long_text = b"A" * 40 + b"\n+\n" + b"I" * 40 + b"\n"
    assert py_gate(long_text, 0, 0, 32)[0] == LONG and py_gate(long_text, 0, 9, 40) == (PASS, 0)


def test_the_gate_on_the_host():
    by, kinds = _check(_build("qgate_host_driver", []), _cases())
    assert kinds == {PASS, LOW, LONG, FAR, MISFIT, BAD}
    # what the cases are for
    for d in DISTANCES:
        for pl in PLUS_LENS:
            assert by["d%d plus%d" % (d, pl)][0] in (PASS, LOW) and by["d%d plus%d reach to e2" % (d, pl)] == by["d%d plus%d" % (d, pl)]
            assert by["d%d plus%d reach short of e2" % (d, pl)] == (FAR, 0)
    for base in (33, 64):
        assert by["base%d bar" % base] == (PASS, 0) and by["base%d three" % base] == (LOW, 3)
    assert by["newline in the span"] == (LOW, 1) and by["newline in the span, allowed"] == (PASS, 1) and by["before the newline"] == (PASS, 0)
    assert by["empty at the very end"] == (MISFIT, 0)
    for n in (12, 31, 50):
        assert by["whole, line of %d, reach 1024" % n][0] in (PASS, LOW) and by["whole, line of %d, reach 3" % n] == (FAR, 0) and by["whole, line of %d, to its end" % n][0] in (PASS, LOW)
        for what in ("after the sequence line", "after the + line", "mid quality", "one short"):
            assert by["%s, line of %d, to its end" % (what, n)] == (MISFIT, 0), (what, n)
        assert by["mid sequence, line of %d, to its end" % n] == (BAD, 0)
    f = subprocess.run([_build("qgate_host_driver", [])], capture_output=True, text=True, timeout=60).stdout.split()
    assert f[0] == "B" and [int(x) for x in f[1:]] == [1024, PASS, LOW, LONG, FAR, MISFIT, BAD, REACH_MAX, 64, MAX_LEN]


def test_the_gate_on_random_texts():
    _, kinds = _check(_build("qgate_host_driver", []), [_fuzz_case(s) for s in range(150)])
    assert kinds == {PASS, LOW, LONG, FAR, MISFIT, BAD}


def test_newline_flags_of_a_word():
    rng = random.Random(5)
    words = [0, 0x0A0A0A0A, 0x0A, 0x0A000000, 0x0B0A090A, 0x8A0A8A0A, 0x0A0B0A0B, 0xFFFFFFFF, 0x0A0A0A09, 0x090A0A0A] + [rng.getrandbits(32) for _ in range(200)]
    words += [int.from_bytes(bytes(rng.choice((10, 10, 9, 11, 138, 0)) for _ in range(4)), "little") for _ in range(200)]
    lines = _run(_build("qgate_host_driver", []), "nl", "".join("%x\n" % w for w in words))
    assert [int(x) for x in lines if x] == [sum(1 << j for j in range(4) if (w >> (8 * j)) & 255 == 10) for w in words]


def test_gate_under_sanitizers():
    exe = _build("qgate_host_driver_asan", SAN)
    _, kinds = _check(exe, _cases() + [_fuzz_case(s) for s in range(150)], SAN_ENV)
    assert kinds == {PASS, LOW, LONG, FAR, MISFIT, BAD}


# ---- the entries on the real library, without a GPU ----
GATE_SYMBOLS = ("seeqdevScanQualityGate", "seeqdevScanGatedDevice", "seeqdevScanCopyGated", "seeqdevScanCopyGatedOffsets", "seeqdevScanCopyGateKinds",
                "seeqdevScanLastQualityGateMs")
FIELDS = [("nspans", 0), ("npassed", 8), ("nlow", 16), ("nlong", 24), ("nfar", 32), ("nmisfit", 40), ("low_bases", 48)]


def test_gate_symbols_exported(capi):
    L = capi.lib()
    hdr = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    for name in GATE_SYMBOLS:
        assert name in capi.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    assert capi.SEEQDEV_TALLY_GATED == 4 == int(re.search(r"#define\s+SEEQDEV_TALLY_GATED\s+(\d+)", hdr).group(1))
    for name, value in zip(KIND_NAMES[:5], (PASS, LOW, LONG, FAR, MISFIT)):
        assert int(re.search(r"#define\s+SEEQDEV_QGATE_%s\s+(\d+)" % name.upper(), hdr).group(1)) == value == getattr(capi, "SEEQDEV_QGATE_" + name.upper())


def test_gate_counts_layout(capi):
    t = capi.seeqdev_qgate_counts_t
    assert C.sizeof(t) == 56 and [(n, getattr(t, n).offset) for n, _ in t._fields_] == FIELDS
    hdr = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} seeqdev_qgate_counts_t;", hdr).group(1)
    names = [n for decl in re.findall(r"uint64_t\s+([^;]+);", body) for n in re.split(r"\s*,\s*", decl.strip())]
    assert names == [n for n, _ in FIELDS]


def _fails(call, code):
    C.set_errno(0)
    assert call() == -1
    assert C.get_errno() == code


def test_gate_argument_checks_without_a_device(capi):
    # Every refusal comes before the device is touched: the stand-in context is all zeros -- no inserts call, nothing fetched, no gate.
    L = capi.lib()
    ctx = C.addressof(C.create_string_buffer(8192))
    text = C.cast(C.c_char_p(b"ACGT\n+\nIIII\n"), C.c_void_p)
    cnt = capi.seeqdev_qgate_counts_t()
    ok = C.byref(cnt)
    INS, HITS, DEMUX, GATED = capi.SEEQDEV_TALLY_INSERTS, capi.SEEQDEV_TALLY_HITS, capi.SEEQDEV_TALLY_DEMUX, capi.SEEQDEV_TALLY_GATED
    gate = L.seeqdevScanQualityGate
    for source in (INS, HITS):
        _fails(lambda: gate(None, source, text, 12, 20, 33, 0, 1024, ok), errno.EINVAL)         # NULL context
        _fails(lambda: gate(ctx, source, text, 12, 20, 33, 0, 1024, None), errno.EINVAL)        # NULL counts
        _fails(lambda: gate(ctx, source, None, 12, 20, 33, 0, 1024, ok), errno.EINVAL)          # NULL text with bytes
        for mq, base in ((223, 33), (0, 256), (256, 0), (2 ** 32 - 1, 1), (1, 2 ** 32 - 1), (2 ** 31, 2 ** 31)):
            _fails(lambda: gate(ctx, source, text, 12, mq, base, 0, 1024, ok), errno.EINVAL)    # base + min_qual > 255 (no wrap-around)
        for reach in (0, REACH_MAX + 1, 2 ** 32 - 1):
            _fails(lambda: gate(ctx, source, text, 12, 20, 33, 0, reach, ok), errno.EINVAL)     # reach outside 1 .. 65536
        _fails(lambda: gate(ctx, source, text, 12, 20, 33, 0, 1024, ok), errno.EINVAL)          # valid arguments: the context holds no source
        assert ("no result of an inserts call" if source == INS else "no fetched records") in capi.error_text()
        _fails(lambda: gate(ctx, source, text, 12, 222, 33, 0, REACH_MAX, ok), errno.EINVAL)    # (the largest legal values: the same)
    for source in (GATED, DEMUX, 3, -1, 255):
        _fails(lambda: gate(ctx, source, text, 12, 20, 33, 0, 1024, ok), errno.EINVAL)          # the gate gates no gate, and no demux
        _fails(lambda: gate(ctx, source, None, 0, 20, 33, 0, 1024, ok), errno.EINVAL)
    ms = C.c_float(1)
    assert L.seeqdevScanLastQualityGateMs(ctx, C.byref(ms)) == 0 and ms.value == 0
    _fails(lambda: L.seeqdevScanLastQualityGateMs(None, C.byref(ms)), errno.EINVAL)
    assert L.seeqdevScanGatedDevice(ctx) is None and L.seeqdevScanGatedDevice(None) is None
    for copy in (L.seeqdevScanCopyGated, L.seeqdevScanCopyGatedOffsets, L.seeqdevScanCopyGateKinds):
        out = C.create_string_buffer(64)
        _fails(lambda: copy(ctx, out, 0, 1), errno.EINVAL)  # nothing gated: nothing to copy
        _fails(lambda: copy(None, out, 0, 0), errno.EINVAL)
        assert copy(ctx, out, 0, 0) == 0


def test_gated_source_needs_a_completed_gate(capi):
    # SEEQDEV_TALLY_GATED on a context without a completed gate: EINVAL from all five tally entries, before any device call.
    L = capi.lib()
    ctx = C.create_string_buffer(8192)
    text = C.cast(C.c_char_p(b"ACGT\n+\nIIII\n"), C.c_void_p)
    GATED = capi.SEEQDEV_TALLY_GATED
    entries = [(L.seeqdevScanTally, capi.seeqdev_tally_counts_t), (L.seeqdevScanTallyHold, capi.seeqdev_tally_hold_counts_t),
               (L.seeqdevScanTallyGrouped, capi.seeqdev_tally_grouped_counts_t), (L.seeqdevScanTallyLibrary, capi.seeqdev_tally_library_counts_t),
               (L.seeqdevScanTallyHoldLibrary, capi.seeqdev_tally_library_counts_t)]
    for entry, counts_t in entries:
        cnt = counts_t()
        for args in ((text, 12), (None, 0)):
            _fails(lambda: entry(C.addressof(ctx), GATED, args[0], args[1], C.byref(cnt)), errno.EINVAL)
        _fails(lambda: entry(C.addressof(ctx), GATED, None, 12, C.byref(cnt)), errno.EINVAL)
        _fails(lambda: entry(C.addressof(ctx), GATED, text, 12, None), errno.EINVAL)
    cnt = capi.seeqdev_tally_counts_t()
    _fails(lambda: L.seeqdevScanTally(C.addressof(ctx), GATED, text, 12, C.byref(cnt)), errno.EINVAL)
    assert "no result of a quality gate" in capi.error_text()
