"""CPU: the anchored cut of seeq_amd/csrc/seeq_anchor.h -- where the cut of a record lies, where its line ends, whether it fits -- compiled
for the host by plain g++ (tests/anchor_host_driver.cpp) and compared with a restatement in Python that finds the line's end with
bytes.find and shares no code with it.  The driver runs every record through the rule byte by byte AND through the decision as the kernel
takes it (the walk in steps of 64 bytes) and fails where they differ.  Once more as a stand-alone program under
-fsanitize=address,undefined.  Then the entries on the real library: exports, the struct's layout, every refusal of the anchor, and of the
tally entries, both appends and the gate for SEEQDEV_TALLY_ANCHORED without a completed anchor (which come before any device call and so
fail the same way without a GPU).  The texts, records and parameter sets here are the ones tests/test_gpu_anchor.py runs on the device."""
import ctypes as C
import errno
import functools
import os
import random
import re
import subprocess

from conftest import ROOT
from text_window import aligned_lead, odd_lead, place

CSRC = os.path.join(ROOT, "seeq_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "build")
SRC = os.path.join(ROOT, "tests", "anchor_host_driver.cpp")
KEPT, SHORT, FAR, BAD = range(4)
AFTER, BEFORE, LINE = "after", "before", "line"
ANCHOR_CODE = {AFTER: 0, BEFORE: 1, LINE: 2}
REACH_MAX = 65536
U32 = 2 ** 32 - 1
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
FLANK = b"GATGTAGCGCGATTAGCCTG"                              # tests/test_gpu_tally.py: LEFT -- the one flank of a read


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("seeq_anchor.h", "seeq_qgate.h", "seeq_tally.h", "seeq_strand.h", "seeq_tiles.h")]
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
def py_anchor(text, off, start, end, anchor=AFTER, skip=0, length=0, reach=1024):
    """(kind, s, e) of the cut of the record [start, end) of the line at `off` in `text` (bytes), by the rule of seeq_anchor.h."""
    n = len(text)
    if end < start or off > n or end > n - off:
        return BAD, 0, 0

    def kept(s, e):
        return (KEPT, s, e) if e <= U32 else (SHORT, 0, 0)
    if anchor == BEFORE:
        if skip > start or length > start - skip:
            return SHORT, 0, 0
        e = start - skip
        return kept(e - length if length else 0, e)
    s = (end if anchor == AFTER else 0) + skip
    e = s + length
    if length and e <= end:
        return kept(s, e)
    p = off + end
    lim = min(n, p + reach)
    i = text.find(b"\n", p, lim)
    if i < 0 and lim < n:
        return kept(s, e) if length else (FAR, 0, 0)
    L = (n if i < 0 else i) - off
    if length == 0:
        if s > L:
            return SHORT, 0, 0
        e = L
    elif e > L:
        return SHORT, 0, 0
    return kept(s, e)


def py_anchor_all(text, records, offsets, **kw):
    """The anchor over rows of (line, start, end, w) with their line offsets -> (kinds, kept rows (line, s, e, w), their offsets, counts)."""
    kinds, rows, offs, nbytes = [], [], [], 0
    for r, off in zip(records, offsets):
        kind, s, e = py_anchor(text, int(off), int(r[1]), int(r[2]), **kw)
        assert kind != BAD
        kinds.append(kind)
        if kind == KEPT:
            rows.append((int(r[0]), s, e, int(r[3])))
            offs.append(int(off))
            nbytes += e - s
    cnt = dict(nspans=len(kinds), nkept=kinds.count(KEPT), nshort=kinds.count(SHORT), nfar=kinds.count(FAR), span_bytes=nbytes)
    return kinds, rows, offs, cnt


# ---- the texts: plain lines with ONE flank, whose hits the test knows ----
class Lines:
    """Text put together line by line.  rows: per line with the flank (1-based line number, offset of the line, start, end of the flank)."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.buf, self.rows, self.nline = bytearray(), [], 0

    def bases(self, n):
        return bytes(self.rng.choices(b"ACGT", k=n))

    def add(self, pre, suf, eol=b"\n", flank=FLANK):
        """A line of `pre` bases, the flank and `suf` bases (flank None: pre + suf bases alone; pre None: an empty line)."""
        self.nline += 1
        off = len(self.buf)
        if pre is None:
            self.buf += eol
            return off
        if flank is not None:
            self.rows.append((self.nline, off, pre, pre + len(flank)))
        self.buf += self.bases(pre) + (flank or b"") + self.bases(suf) + eol
        return off

    def text(self):
        return bytes(self.buf)


# the distances from the flank's end to the end of its line: a newline at every offset 0 .. 64 behind off + end, and around 128 and 256
SUFFIXES = tuple(range(0, 67)) + (126, 127, 128, 129, 130, 255, 256, 257)
# how the text ends: (bases behind the last line's flank, a final newline?) -- off + end of the last record lies 0 (a span ending exactly at
# nbytes), 1, 15, 16, 63, 64 bytes before the text's end: the byte-wise tail of the walk
TAILS = ((0, False), (1, False), (15, False), (16, False), (63, False), (64, False), (0, True), (14, True), (70, False))


def edge_text(tail, seed=11):
    """Every suffix length x a few prefix lengths (0: the hit starts the line), an empty line behind a record now and then, '\\r\\n' lines,
    lines without the flank, and the last line by `tail`."""
    suf, newline = tail
    t = Lines(seed)
    for k, d in enumerate(SUFFIXES):
        t.add((0, 3, 17, 40)[k % 4], d)
        if k % 5 == 2:
            t.add(None, 0)                                  # an empty line behind the record
        if k % 7 == 3:
            t.add(9, 30, flank=None)
    for d in (0, 1, 12, 16, 63):
        t.add(5, d, eol=b"\r\n")                            # the '\r' belongs to the line
    t.add(None, 0, eol=b"\r\n")
    t.add(2, 12)
    t.add(7, suf, eol=b"\n" if newline else b"")
    return t


# (anchor, skip, length, reach): every anchor with length == 0 and > 0.  AFTER: e - end = skip + length in 1, 12, 15, 16, 17, 63, 64, 65, 127,
# 128, 129 and reach == skip + length; length 0 under reach 1, 63, 64, 65 (FAR and the text's end are both reached); s == L (skip 3, 64 on the
# lines with that suffix).  LINE: e - end = 0 on the lines without a prefix (length 20), below 0 (no byte loaded) and above.  BEFORE: skip >
# start, length > start - skip.
PARAMS = ([(AFTER, 0, 0, 1024), (AFTER, 3, 0, 1024), (AFTER, 64, 0, 1024), (AFTER, 0, 0, 1), (AFTER, 0, 0, 63), (AFTER, 0, 0, 64), (AFTER, 0, 0, 65),
           (AFTER, 5, 0, 63), (AFTER, 2, 0, REACH_MAX)]
          + [(AFTER, 0, n, 1024) for n in (1, 12, 15, 16, 17, 63, 64, 65, 127, 128, 129)]
          + [(AFTER, 3, 12, 1024), (AFTER, 1, 127, 128), (AFTER, 0, 1, 1), (AFTER, 0, 12, 12), (AFTER, 0, 64, 64), (AFTER, 60, 5, 65), (AFTER, 0, 16, REACH_MAX)]
          + [(LINE, 0, 0, 1024), (LINE, 16, 0, 1024), (LINE, 200, 0, 1024), (LINE, 0, 0, 1), (LINE, 0, 0, 63), (LINE, 0, 0, 64), (LINE, 21, 0, 65)]
          + [(LINE, 0, 16, 1024), (LINE, 16, 12, 1024), (LINE, 0, 1, 1), (LINE, 0, 20, 1024), (LINE, 0, 21, 1024), (LINE, 0, 23, 64), (LINE, 20, 60, 80),
             (LINE, 0, 150, 1024), (LINE, 0, 84, 1024), (LINE, 0, 85, 1024)]
          + [(BEFORE, 0, 0, 1024), (BEFORE, 3, 0, 1), (BEFORE, 17, 0, 1024), (BEFORE, 41, 0, 1024), (BEFORE, 0, 3, 1024), (BEFORE, 0, 17, 1024),
             (BEFORE, 3, 14, 1024), (BEFORE, 3, 15, 1), (BEFORE, 0, 40, 1024), (BEFORE, 0, 41, 1024)])


def _kw(param):
    return dict(anchor=param[0], skip=param[1], length=param[2], reach=param[3])


def random_lines(n, seed):
    """n lines with the flank (and one without now and then): prefixes 0 .. 30, suffixes 0 .. 150."""
    t = Lines(seed)
    for i in range(n):
        t.add(t.rng.randrange(31), t.rng.choice((0, 1, 2, 5, 11, 12, 13, 40, 63, 64, 65, 100, 150)))
        if i % 40 == 9:
            t.add(12, 20, flank=None)
    return t


# ---- the window of test_gpu_anchor.py's placement: its guards are made of bases ----
GUARD_BEFORE = b"ACGTTGCA" * 5                               # the guard in front ends in bases without a newline
GUARD_AFTER = b"TTGACCAGTA" * 30 + b"\n"                     # the guard behind begins with bases: a cut that reads on finds a longer line


def window_case(i):
    """(lines, big buffer, lo, hi) of placement i: an odd lead for even i, a 16-aligned one for odd i; the window's last line has no newline."""
    t = edge_text((15, False), seed=21 + i)
    big, lo, hi = place(t.text(), odd_lead(i) if i % 2 == 0 else aligned_lead(i), GUARD_BEFORE, GUARD_AFTER)
    return t, big, lo, hi


# ---- cases for the driver ----
@functools.lru_cache(maxsize=None)
def _cases():
    """-> list of (text, [(what, off, start, end, anchor, skip, length, reach)])."""
    out = []
    for tail in TAILS:
        t = edge_text(tail)
        text = t.text()
        out.append((text, [("tail %s %s row %d" % (tail, p, k), off, st, en) + p for p in PARAMS for k, (_, off, st, en) in enumerate(t.rows)]))
    # bad records; huge skips and lengths (the sums are taken in 64 bits)
    text = edge_text((5, True)).text()
    n = len(text)
    spans = [("bad: end < start", 0, 9, 8, AFTER, 0, 0, 64), ("bad: beyond the text", 0, 0, n + 1, LINE, 0, 0, 64), ("bad: offset beyond the text", n + 1, 0, 0, BEFORE, 0, 0, 64),
             ("bad: end beyond the rest", 10, 0, n - 9, AFTER, 0, 1, 64), ("bad: before, with a length", 0, 9, 8, BEFORE, 0, 2, 64), ("bad: line, with a length", n + 1, 0, 0, LINE, 0, 2, 64), ("empty at the very end", n, 0, 0, AFTER, 0, 0, 64), ("one byte at the very end", n, 0, 0, AFTER, 0, 1, 64),
             ("the whole text as a record", 0, 0, n, AFTER, 0, 0, 64), ("huge skip after", 0, 0, 20, AFTER, U32, 0, 1024), ("huge skip line", 0, 0, 20, LINE, U32, 0, 1024),
             ("huge skip before", 0, 5, 20, BEFORE, U32, 0, 1024), ("huge length before", 0, 5, 20, BEFORE, 0, U32, 1024), ("huge both before", 0, 5, 20, BEFORE, U32, U32, 1024),
             ("reach max", 0, 0, 20, AFTER, REACH_MAX - 1, 1, REACH_MAX), ("reach max line", 0, 0, 20, LINE, 0, REACH_MAX, REACH_MAX)]
    out.append((text, spans))
    # one line longer than the reach, in a text that goes on and in one that ends: FAR against the text's end
    long_line = FLANK + b"A" * 300
    for reach in (1, 63, 64, 65, 128, 300):
        spans = [("long line reach %d %s" % (reach, a), 0, 0, 20, a, 0, 0, reach) for a in (AFTER, LINE)]
        spans += [("long line reach %d len %d" % (reach, reach), 0, 0, 20, AFTER, 0, reach, reach)]
        out.append((long_line + b"\nACGT\n", spans))
        out.append((long_line, spans))
        out.append((long_line[:20 + reach], spans))
        out.append((long_line[:20 + reach + 1], spans))
    return out


def _fuzz_case(seed):
    """A random text of lines of random lengths, cut at a random place; random records (now and then beyond their line or the text), anchors,
    skips, lengths and reaches that pass the argument check."""
    rng = random.Random(seed)
    t = Lines(seed)
    for _ in range(rng.randrange(1, 12)):
        if rng.random() < 0.1:
            t.add(None, 0)
        else:
            t.add(rng.choice((0, 1, 5, 20)), rng.choice((0, 1, 5, 20, 33, 44, 64, 100, 150, 300)), eol=rng.choice((b"\n", b"\n", b"\n", b"\r\n", b"")))
    text = t.text()
    if rng.random() < 0.5:
        text = text[:rng.randrange(len(text) + 1)]
    starts = [0] + [i + 1 for i, b in enumerate(text) if b == 10]
    spans = []
    for _ in range(80):
        off = rng.choice(starts) if rng.random() < 0.9 else rng.randrange(len(text) + 2)
        start = rng.randrange(0, 40)
        end = start + rng.choice((0, 1, 8, 20, 31)) if rng.random() < 0.95 else max(0, start - 1)
        anchor = rng.choice((AFTER, BEFORE, LINE))
        reach = rng.choice((1, 2, 63, 64, 65, 128, 200, 1024, REACH_MAX))
        length = rng.choice((0, 0, 1, 8, 12, 16, 17, 40, 64, 65, 130))
        skip = rng.choice((0, 0, 1, 3, 16, 47, 48, 64, 100))
        if anchor != BEFORE and length and skip + length > reach:
            skip, length = 0, rng.randrange(1, reach + 1) if reach < 200 else length
        spans.append(("fuzz", off, start, end, anchor, skip, length, reach))
    return text, spans


def _input(cases):
    return "".join("T %d %s\n%s" % (len(text), text.hex(), "".join("S %d %d %d %d %d %d %d\n" % (off, st, en, ANCHOR_CODE[a], skip, ln, reach)
                                                                  for _, off, st, en, a, skip, ln, reach in spans)) for text, spans in cases)


def _check(exe, cases, env=None):
    lines = _run(exe, "cut", _input(cases), env)
    got = [tuple(int(x) for x in ln.split()) for ln in lines if ln]
    exp, names = [], []
    for text, spans in cases:
        for what, off, st, en, a, skip, ln, reach in spans:
            assert a == BEFORE or ln == 0 or skip + ln <= reach, "a case the argument check refuses: %s" % what
            exp.append(py_anchor(text, off, st, en, a, skip, ln, reach))
            names.append((what, off, st, en, a, skip, ln, reach, len(text)))
    assert len(got) == len(exp)
    bad = [(names[i], g, exp[i]) for i, g in enumerate(got) if g != exp[i]]
    assert not bad, (len(bad), bad[:5])
    return exp, {(n[4], n[6] > 0, k[0]) for n, k in zip(names, exp)}


# every anchor with length == 0 and > 0 reaches every kind it can: BEFORE is never FAR, and length > 0 never is (skip + length <= reach)
ALL_KINDS = ({(a, pos, k) for a in (AFTER, BEFORE, LINE) for pos in (False, True) for k in (KEPT, SHORT)} | {(AFTER, False, FAR), (LINE, False, FAR)}
             | {(a, pos, BAD) for a in (AFTER, BEFORE, LINE) for pos in (False, True)})


def test_the_restatement_itself():
    text = b"ACGTACGTAC\n\nGGGG\r\nTTTTTT"
    assert py_anchor(text, 0, 2, 4) == (KEPT, 4, 10) and py_anchor(text, 0, 2, 4, length=6) == (KEPT, 4, 10) and py_anchor(text, 0, 2, 4, length=7) == (SHORT, 0, 0)
    assert py_anchor(text, 0, 2, 4, skip=6) == (KEPT, 10, 10) and py_anchor(text, 0, 2, 4, skip=7) == (SHORT, 0, 0)      # s == L: empty, kept
    assert py_anchor(text, 0, 2, 4, reach=6) == (FAR, 0, 0) and py_anchor(text, 0, 2, 4, reach=7) == (KEPT, 4, 10)       # the newline at p + 6
    assert py_anchor(text, 0, 2, 4, length=6, reach=6) == (KEPT, 4, 10)                                                 # length > 0 is never FAR
    assert py_anchor(text, 0, 2, 4, LINE, 1, 3) == (KEPT, 1, 4) and py_anchor(text, 0, 2, 4, LINE, 1, 0) == (KEPT, 1, 10) and py_anchor(text, 0, 2, 4, LINE, 11, 0) == (SHORT, 0, 0)
    assert py_anchor(text, 0, 2, 4, BEFORE) == (KEPT, 0, 2) and py_anchor(text, 0, 2, 4, BEFORE, 1, 1) == (KEPT, 0, 1) and py_anchor(text, 0, 2, 4, BEFORE, 1, 2) == (SHORT, 0, 0)
    assert py_anchor(text, 0, 2, 4, BEFORE, 3) == (SHORT, 0, 0) and py_anchor(text, 0, 2, 4, BEFORE, 2) == (KEPT, 0, 0)
    assert py_anchor(text, 12, 0, 1) == (KEPT, 1, 5) and py_anchor(text, 12, 0, 1, length=4) == (KEPT, 1, 5)              # the '\r' belongs to the line
    assert py_anchor(text, 18, 0, 2) == (KEPT, 2, 6) and py_anchor(text, 18, 0, 2, reach=1) == (FAR, 0, 0) and py_anchor(text, 18, 0, 2, reach=4) == (KEPT, 2, 6)
    assert py_anchor(text, 18, 0, 2, length=4) == (KEPT, 2, 6) and py_anchor(text, 18, 0, 2, length=5) == (SHORT, 0, 0)     # a span ending exactly at nbytes
    assert py_anchor(text, 11, 0, 0) == (KEPT, 0, 0) and py_anchor(text, 11, 0, 0, length=1) == (SHORT, 0, 0)             # the empty line
    assert py_anchor(text, 0, 4, 2)[0] == BAD and py_anchor(text, 25, 0, 0)[0] == BAD and py_anchor(text, 18, 0, 7)[0] == BAD and py_anchor(text, 24, 0, 0) == (KEPT, 0, 0)


def test_the_guards_of_the_window_are_live():
    """The placement of test_gpu_anchor.py: the restatement over the whole buffer -- the records where they lie there -- gives other cuts
    than over the window: a cut that reads past nbytes returns a longer span, one that looks in front of byte 0 a longer line."""
    for i in range(2):
        t, big, lo, hi = window_case(i)
        assert (lo % 16 == 0) == (i % 2 == 1) and not t.text().endswith(b"\n") and big[lo - 1:lo] != b"\n"
        last = t.rows[-1]
        inside = py_anchor(t.text(), last[1], last[2], last[3], AFTER, 0, 0, 1024)
        outside = py_anchor(big, lo + last[1], last[2], last[3], AFTER, 0, 0, 1024)
        assert inside == (KEPT, last[3], last[3] + 15) and outside[0] == KEPT and outside[2] > inside[2]
        assert py_anchor(t.text(), last[1], last[2], last[3], AFTER, 0, 16, 1024)[0] == SHORT and py_anchor(big, lo + last[1], last[2], last[3], AFTER, 0, 16, 1024)[0] == KEPT
        # in front: the window's first line starts at byte 0; a line start taken from the guard's bases makes it longer
        first = t.rows[0]
        start_in_big = big.rfind(b"\n", 0, lo) + 1
        assert first[1] == 0 and lo - start_in_big == len(GUARD_BEFORE)
        shifted = py_anchor(big, start_in_big, first[2] + lo - start_in_big, first[3] + lo - start_in_big, LINE, 0, 0, 1024)
        assert shifted[0] == KEPT and shifted[2] == py_anchor(t.text(), 0, first[2], first[3], LINE, 0, 0, 1024)[2] + len(GUARD_BEFORE)


def test_the_cut_on_the_host():
    exp, kinds = _check(_build("anchor_host_driver", []), _cases())
    assert kinds == ALL_KINDS, (kinds ^ ALL_KINDS)
    f = subprocess.run([_build("anchor_host_driver", [])], capture_output=True, text=True, timeout=60).stdout.split()
    assert f[0] == "B" and [int(x) for x in f[1:]] == [1024, ANCHOR_CODE[AFTER], ANCHOR_CODE[BEFORE], ANCHOR_CODE[LINE], KEPT, SHORT, FAR, BAD, REACH_MAX, 6]


def test_what_the_cases_are_for():
    """The edges by name, on the restatement (which test_the_cut_on_the_host holds the driver against)."""
    for tail in TAILS:
        t = edge_text(tail)
        text = t.text()
        sufs = {}
        for _, off, st, en in t.rows:
            nl = text.find(b"\n", off)
            sufs.setdefault((nl if nl >= 0 else len(text)) - off - en, (off, st, en))
        assert set(range(65)) <= set(sufs)                  # a newline at every offset 0 .. 64 behind off + end
        for d in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129):
            off, st, en = sufs[d]
            assert py_anchor(text, off, st, en, AFTER, 0, d) == (KEPT, en, en + d) and py_anchor(text, off, st, en, AFTER, 0, d + 1)[0] == SHORT
            assert py_anchor(text, off, st, en, AFTER, d, 0) == (KEPT, en + d, en + d)      # s == L
        off, st, en = sufs[64]
        assert py_anchor(text, off, st, en, AFTER, 0, 0, 64)[0] == FAR and py_anchor(text, off, st, en, AFTER, 0, 0, 65) == (KEPT, en, en + 64)
        last = t.rows[-1]
        assert py_anchor(text, *last[1:])[0] == KEPT and last[1] + py_anchor(text, *last[1:])[2] == len(text) - (1 if tail[1] else 0)
        assert len(text) - (last[1] + last[3]) == tail[0] + (1 if tail[1] else 0)


def test_the_cut_on_random_texts():
    _, kinds = _check(_build("anchor_host_driver", []), [_fuzz_case(s) for s in range(200)])
    assert kinds == ALL_KINDS, (kinds ^ ALL_KINDS)


def test_cut_under_sanitizers():
    exe = _build("anchor_host_driver_asan", SAN)
    _, kinds = _check(exe, _cases() + [_fuzz_case(s) for s in range(200)], SAN_ENV)
    assert kinds == ALL_KINDS


# ---- the entries on the real library, without a GPU ----
ANCHOR_SYMBOLS = ("seeqdevScanAnchor", "seeqdevScanAnchoredDevice", "seeqdevScanCopyAnchored", "seeqdevScanCopyAnchoredOffsets", "seeqdevScanCopyAnchorKinds",
                  "seeqdevScanLastAnchorMs")
FIELDS = [("nspans", 0), ("nkept", 8), ("nshort", 16), ("nfar", 24), ("span_bytes", 32)]


def test_anchor_symbols_exported(capi):
    L = capi.lib()
    hdr = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    for name in ANCHOR_SYMBOLS:
        assert name in capi.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    assert capi.SEEQDEV_TALLY_ANCHORED == 5 == int(re.search(r"#define\s+SEEQDEV_TALLY_ANCHORED\s+(\d+)", hdr).group(1))
    for name, value in (("AFTER", 0), ("BEFORE", 1), ("LINE", 2), ("KEPT", KEPT), ("SHORT", SHORT), ("FAR", FAR)):
        assert int(re.search(r"#define\s+SEEQDEV_ANCHOR_%s\s+(\d+)" % name, hdr).group(1)) == value == getattr(capi, "SEEQDEV_ANCHOR_" + name)
    assert "not served" not in hdr


def test_anchor_counts_layout(capi):
    t = capi.seeqdev_anchor_counts_t
    assert C.sizeof(t) == 40 and [(n, getattr(t, n).offset) for n, _ in t._fields_] == FIELDS
    hdr = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} seeqdev_anchor_counts_t;", hdr).group(1)
    names = [n for decl in re.findall(r"uint64_t\s+([^;]+);", body) for n in re.split(r"\s*,\s*", decl.strip())]
    assert names == [n for n, _ in FIELDS]


def _fails(call, code):
    C.set_errno(0)
    assert call() == -1
    assert C.get_errno() == code


def test_anchor_argument_checks_without_a_device(capi):
    # Every refusal comes before the device is touched: the stand-in context is all zeros -- no inserts call, nothing fetched, no anchor.
    L = capi.lib()
    ctx = C.addressof(C.create_string_buffer(8192))
    text = C.cast(C.c_char_p(b"ACGTACGT\nACGT\n"), C.c_void_p)
    cnt = capi.seeqdev_anchor_counts_t()
    ok = C.byref(cnt)
    INS, HITS, DEMUX, GATED, ANCHORED = (capi.SEEQDEV_TALLY_INSERTS, capi.SEEQDEV_TALLY_HITS, capi.SEEQDEV_TALLY_DEMUX, capi.SEEQDEV_TALLY_GATED,
                                         capi.SEEQDEV_TALLY_ANCHORED)
    cut = L.seeqdevScanAnchor
    for source in (INS, HITS):
        for anchor in (0, 1, 2):
            _fails(lambda: cut(None, source, text, 14, anchor, 0, 4, 1024, ok), errno.EINVAL)         # NULL context
            _fails(lambda: cut(ctx, source, text, 14, anchor, 0, 4, 1024, None), errno.EINVAL)        # NULL counts
            _fails(lambda: cut(ctx, source, None, 14, anchor, 0, 4, 1024, ok), errno.EINVAL)          # NULL text with bytes
            for reach in (0, REACH_MAX + 1, U32):
                _fails(lambda: cut(ctx, source, text, 14, anchor, 0, 0, reach, ok), errno.EINVAL)     # reach outside 1 .. 65536
            _fails(lambda: cut(ctx, source, text, 14, anchor, 0, 4, 1024, ok), errno.EINVAL)          # valid arguments: the context holds no source
            assert ("no result of an inserts call" if source == INS else "no fetched records") in capi.error_text()
            _fails(lambda: cut(ctx, source, text, 14, anchor, 0, 0, REACH_MAX, ok), errno.EINVAL)     # (the largest legal reach: the same)
        for anchor in (-1, 3, 255):
            _fails(lambda: cut(ctx, source, text, 14, anchor, 0, 4, 1024, ok), errno.EINVAL)          # an unknown anchor
        for anchor in (0, 2):
            for skip, ln, reach in ((0, 5, 4), (4, 1, 4), (1024, 1, 1024), (U32, 1, REACH_MAX), (1, U32, REACH_MAX), (2 ** 31, 2 ** 31, REACH_MAX)):
                _fails(lambda: cut(ctx, source, text, 14, anchor, skip, ln, reach, ok), errno.EINVAL)   # skip + len > reach (no wrap-around)
        # ... which BEFORE does not ask, and len == 0 does not: these get as far as the missing source
        _fails(lambda: cut(ctx, source, text, 14, 1, U32, U32, 1, ok), errno.EINVAL)
        assert ("no result of an inserts call" if source == INS else "no fetched records") in capi.error_text()
        _fails(lambda: cut(ctx, source, text, 14, 0, U32, 0, 1, ok), errno.EINVAL)
        assert ("no result of an inserts call" if source == INS else "no fetched records") in capi.error_text()
    for source in (GATED, DEMUX, ANCHORED, 3, -1, 255):
        _fails(lambda: cut(ctx, source, text, 14, 0, 0, 4, 1024, ok), errno.EINVAL)                   # the anchor cuts no gate, no demux and no anchor
        _fails(lambda: cut(ctx, source, None, 0, 0, 0, 4, 1024, ok), errno.EINVAL)
    ms = C.c_float(1)
    assert L.seeqdevScanLastAnchorMs(ctx, C.byref(ms)) == 0 and ms.value == 0
    _fails(lambda: L.seeqdevScanLastAnchorMs(None, C.byref(ms)), errno.EINVAL)
    assert L.seeqdevScanAnchoredDevice(ctx) is None and L.seeqdevScanAnchoredDevice(None) is None
    for copy in (L.seeqdevScanCopyAnchored, L.seeqdevScanCopyAnchoredOffsets, L.seeqdevScanCopyAnchorKinds):
        out = C.create_string_buffer(64)
        _fails(lambda: copy(ctx, out, 0, 1), errno.EINVAL)  # nothing anchored: nothing to copy
        _fails(lambda: copy(None, out, 0, 0), errno.EINVAL)
        assert copy(ctx, out, 0, 0) == 0


def test_anchored_source_needs_a_completed_anchor(capi):
    # SEEQDEV_TALLY_ANCHORED on a context without a completed anchor: EINVAL from the five tally entries, both appends and the gate, before
    # any device call; the message names what is missing.
    L = capi.lib()
    ctx = C.create_string_buffer(8192)
    text = C.cast(C.c_char_p(b"ACGT\n+\nIIII\n"), C.c_void_p)
    ANCHORED = capi.SEEQDEV_TALLY_ANCHORED
    entries = [(L.seeqdevScanTally, capi.seeqdev_tally_counts_t), (L.seeqdevScanTallyHold, capi.seeqdev_tally_hold_counts_t),
               (L.seeqdevScanTallyGrouped, capi.seeqdev_tally_grouped_counts_t), (L.seeqdevScanTallyLibrary, capi.seeqdev_tally_library_counts_t),
               (L.seeqdevScanTallyHoldLibrary, capi.seeqdev_tally_library_counts_t)]
    for entry, counts_t in entries:
        cnt = counts_t()
        for args in ((text, 12), (None, 0)):
            _fails(lambda: entry(C.addressof(ctx), ANCHORED, args[0], args[1], C.byref(cnt)), errno.EINVAL)
        _fails(lambda: entry(C.addressof(ctx), ANCHORED, None, 12, C.byref(cnt)), errno.EINVAL)
        _fails(lambda: entry(C.addressof(ctx), ANCHORED, text, 12, None), errno.EINVAL)
    for entry, counts_t in ((L.seeqdevScanTally, capi.seeqdev_tally_counts_t), (L.seeqdevScanTallyHold, capi.seeqdev_tally_hold_counts_t)):
        cnt = counts_t()
        _fails(lambda: entry(C.addressof(ctx), ANCHORED, text, 12, C.byref(cnt)), errno.EINVAL)
        assert "no result of an anchor call" in capi.error_text()
    app = capi.seeqdev_tally_append_counts_t()
    for entry, column_t in ((L.seeqdevScanTallyHoldAppend, capi.seeqdev_tally_hold_counts_t), (L.seeqdevScanTallyHoldAppendLibrary, capi.seeqdev_tally_library_counts_t)):
        col = column_t()
        for args in ((text, 12), (None, 0)):
            _fails(lambda: entry(C.addressof(ctx), ANCHORED, args[0], args[1], C.byref(col), C.byref(app)), errno.EINVAL)
    g = capi.seeqdev_qgate_counts_t()
    for args in ((text, 12), (None, 0)):
        _fails(lambda: L.seeqdevScanQualityGate(C.addressof(ctx), ANCHORED, args[0], args[1], 20, 33, 0, 1024, C.byref(g)), errno.EINVAL)
        assert "no result of an anchor call" in capi.error_text()
    _fails(lambda: L.seeqdevScanQualityGate(C.addressof(ctx), ANCHORED, text, 12, 20, 33, 0, 0, C.byref(g)), errno.EINVAL)      # the gate's own checks come first
