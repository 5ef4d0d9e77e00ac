"""CPU: the rule of the appended key columns of seeq_amd/csrc/seeq_tally_append.h -- the join of a new column into the held one, the
composed key, the width check, the split -- compiled for the host by plain g++ (tests/tally_append_host_driver.cpp) and compared with a
restatement in Python built on test_tally_group_host.py_group_of.  Once more as a stand-alone program under
-fsanitize=address,undefined.  Then the entries on the real library: exports, layouts, the argument checks (which run before any device
call and so fail the same way without a GPU), seeqdevTallySplit and hold_split."""
import ctypes as C
import errno
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_tally_group_host import SAN, SAN_ENV, py_group_of

CSRC = os.path.join(ROOT, "seeq_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "build")
SRC = os.path.join(ROOT, "tests", "tally_append_host_driver.cpp")
COLUMNS, WORD_BITS = 8, 63


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("seeq_tally_append.h", "seeq_tally_group.h", "seeq_tally.h", "seeq_strand.h", "seeq_tiles.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + ["-I" + CSRC, SRC, "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe, mode, text, env=None):
    r = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r.stdout.split("\n")


# ---- the rule, restated ----
def py_width(column):
    """column: [(line, key)] -> the bit length of its largest key, 0 when no record has one."""
    return max([k.bit_length() for _, k in column], default=0)


def py_append(held, column, width=None):
    """held, column: [(line, key)] in record order; width: the new column's (None: py_width) -> (the held column afterwards, counts)."""
    w = py_width(column) if width is None else width
    out = []
    for line, key in held:
        k = py_group_of(column, line) if key else 0
        out.append((line, (key << w) | k if key and k else 0))
    nbefore, nheld = sum(1 for _, k in held if k), sum(1 for _, k in out if k)
    return out, dict(nrecords=len(held), nbefore=nbefore, nheld=nheld, ndropped=nbefore - nheld, width=w, key_bits=py_width(out))


def py_split(key, widths):
    """-> the columns' keys, or None where seeqdevTallySplit says EINVAL."""
    if not 1 <= len(widths) <= COLUMNS or sum(widths) > WORD_BITS or key >> sum(widths):
        return None
    out = []
    for w in reversed(widths):
        out.append(key & ((1 << w) - 1))
        key >>= w
    return out[::-1]


def test_the_restatement_itself():
    held = [(1, 5), (2, 0), (3, 6), (3, 7), (5, 1), (9, 2)]
    column = [(1, 3), (2, 3), (3, 0), (3, 2), (9, 1), (9, 3), (11, 2)]
    out, cnt = py_append(held, column)
    # line 3: the FIRST record of the new column decides, and it has no key -- both held records of the line are dropped; line 5 is missing
    assert out == [(1, 5 << 2 | 3), (2, 0), (3, 0), (3, 0), (5, 0), (9, 2 << 2 | 1)]
    assert cnt == dict(nrecords=6, nbefore=5, nheld=2, ndropped=3, width=2, key_bits=5)
    assert py_append(held, [])[1] == dict(nrecords=6, nbefore=5, nheld=0, ndropped=5, width=0, key_bits=0)
    assert py_split(5 << 2 | 3, [3, 2]) == [5, 3] and py_split(5 << 2 | 3, [2, 2]) is None and py_split(0, [0]) == [0]


# ---- the join ----
def _column(rng, n, bits, step=(0, 0, 1, 1, 1, 2, 7), keyless=0.2):
    line, out = 0, []
    for _ in range(n):
        line += rng.choice(step)
        out.append((max(line, 1), 0 if rng.random() < keyless or not bits else rng.getrandbits(bits) | 1))
    return out


def _join_cases():
    rng = random.Random(41)
    cases = [(0, None, [], []), (3, None, [(1, 5), (4, 7)], []), (0, None, [], [(1, 1)]),
             (3, None, [(1, 5), (2, 0), (3, 6), (3, 7), (5, 1), (9, 2)], [(1, 3), (2, 3), (3, 0), (3, 2), (9, 1), (9, 3), (11, 2)]),
             (3, None, [(2, 5), (3, 6)], [(2, 0), (3, 0)]),                                  # w == 0: every key becomes 0
             (33, 30, [(1, 2 ** 33 - 1), (2, 2 ** 32)], [(1, 2 ** 30 - 1), (2, 1)]),            # 33 + 30 = 63: fits, bits 0 .. 62 set
             (33, 31, [(1, 2 ** 33 - 1)], [(1, 2 ** 31 - 1)]),                                # 64: refused
             (41, None, [(1, 2 ** 41 - 1)], [(1, 2 ** 40)]),                                  # two 20-base columns: 41 + 41
             (63, 0, [(7, 2 ** 63 - 1)], [(7, 0)]), (63, 1, [(7, 2 ** 63 - 1)], [(7, 1)]),
             (8, 17, [(2 ** 32 - 1, 255)], [(2 ** 32 - 2, 3), (2 ** 32 - 1, 2 ** 17 - 1)])]
    for nh, nc in ((1, 1), (2, 300), (300, 2), (63, 64), (1000, 1000), (3000, 2500), (2500, 3000), (1500, 0), (0, 1500)):
        for hbits, cbits in ((33, 17), (8, 22), (1, 1)):
            held = _column(rng, nh, hbits)
            column = _column(rng, nc, cbits, step=rng.choice([(0, 1, 1, 2), (1, 3, 9), (0, 0, 0, 1)]))
            cases.append((hbits, None, held, column))
    return [(kb, py_width(col) if w is None else w, h, col) for kb, w, h, col in cases]


def _join_input(cases):
    rows = lambda col: "".join("%d %x\n" % r for r in col)      # noqa: E731
    return "".join("W %d %d\nH %d\n%sN %d\n%s" % (kb, w, len(h), rows(h), len(col), rows(col)) for kb, w, h, col in cases)


def _check_joins(lines, cases):
    at = kept = dropped = refused = 0
    for kb, w, held, column in cases:
        fits = kb + w <= WORD_BITS
        assert lines[at] == "F %d" % fits, (lines[at], kb, w)
        at += 1
        if not fits:
            refused += 1
            continue
        exp, cnt = py_append(held, column, w)
        got = [int(x, 16) for x in lines[at:at + len(held)]]
        assert got == [k for _, k in exp], (kb, w, held[:6], column[:6])
        at += len(held)
        assert lines[at] == "C %d %d %d %d" % (cnt["nbefore"], cnt["nheld"], cnt["ndropped"], cnt["key_bits"]), lines[at]
        at += 1
        assert cnt["key_bits"] <= kb + w and (cnt["key_bits"] > 0) == (cnt["nheld"] > 0)
        kept += cnt["nheld"]
        dropped += cnt["ndropped"]
    assert lines[at:] in ([], [""]) and kept > 3000 and dropped > 3000 and refused == 3


def test_the_join_on_the_host():
    cases = _join_cases()
    exe = _build("tally_append_host_driver", [])
    _check_joins(_run(exe, "join", _join_input(cases)), cases)
    f = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert f == ["A", str(COLUMNS), str(WORD_BITS), "32"]


# ---- the composed word: injective, column-major ----
def _compose_cases():
    rng = random.Random(43)
    shapes = [[33, 17], [8, 22, 17], [1] * 8, [7, 8, 8, 8, 8, 8, 8, 8], [63], [41, 22], [2, 3, 2]]
    cases = []
    for widths in shapes:
        for _ in range(60):
            cases.append((widths, [rng.choice([1, (1 << w) - 1, rng.getrandbits(w) | 1]) for w in widths]))
    # every tuple of a small shape: the map must be one-to-one and ordered as the tuples are
    cases += [([2, 3, 2], [a, b, c]) for a in range(1, 4) for b in range(1, 8) for c in range(1, 4)]
    return cases


def _check_compose(lines, cases):
    words = [tuple(int(x, 16 if i == 0 else 10) for i, x in enumerate(ln.split())) for ln in lines if ln]
    assert len(words) == len(cases)
    seen = {}
    for (widths, keys), (word, bits) in zip(cases, words):
        assert bits == word.bit_length() <= sum(widths) <= WORD_BITS
        assert py_split(word, widths) == keys                                                # nothing is lost
        assert seen.setdefault((tuple(widths), word), keys) == keys                          # one word, one tuple
    small = [(keys, word) for (widths, keys), (word, _) in zip(cases, words) if widths == [2, 3, 2]]
    assert len({w for _, w in small}) == len({tuple(k) for k, _ in small}) >= 3 * 7 * 3
    assert [k for k, _ in sorted(small, key=lambda x: x[1])] == sorted(k for k, _ in small)    # column 0 most significant, then 1, then 2


def _compose_input(cases):
    return "".join("%d %s\n" % (len(w), " ".join("%d %x" % wk for wk in zip(w, k))) for w, k in cases)


def test_composed_keys_are_injective_and_column_major():
    cases = _compose_cases()
    _check_compose(_run(_build("tally_append_host_driver", []), "compose", _compose_input(cases)), cases)


# ---- the split ----
def _split_cases():
    rng = random.Random(47)
    cases = [(0, []), (5, [3] * 9), (1, [32, 32]), (1 << 5, [3, 2]), ((1 << 63) - 1, [63]), (1 << 63, [63]), (2 ** 64 - 1, [33, 30]),
             (0, [0]), (0, [0, 0, 0]), (1, [0]), (5, [0, 3, 0]), ((1 << 63) - 1, [33, 30]), ((1 << 62) - 1, [33, 29]), (7, [1, 1, 1, 0, 0, 0, 0, 0])]
    for _ in range(200):
        widths = [rng.randrange(0, 20) for _ in range(rng.randrange(1, 9))]
        cases.append((rng.getrandbits(min(sum(widths) + rng.choice([0, 0, 0, 1]), 64)), widths))
    return cases


def _check_splits(lines, cases):
    ok = bad = 0
    for ln, (key, widths) in zip(lines, cases):
        exp = py_split(key, widths)
        got = ln.split()
        if exp is None:
            assert got == ["-1"], (key, widths, ln)
            bad += 1
        else:
            assert got[0] == "0" and [int(x, 16) for x in got[1:]] == exp, (key, widths, ln)
            ok += 1
    assert lines[len(cases):] in ([], [""]) and ok > 100 and bad > 10


def _split_input(cases):
    return "".join("%x %d %s\n" % (k, len(w), " ".join(map(str, w))) for k, w in cases)


def test_the_split_on_the_host():
    cases = _split_cases()
    _check_splits(_run(_build("tally_append_host_driver", []), "split", _split_input(cases)), cases)


def test_append_rule_under_sanitizers():
    exe = _build("tally_append_host_driver_asan", SAN)
    jc, cc, sc = _join_cases(), _compose_cases(), _split_cases()
    _check_joins(_run(exe, "join", _join_input(jc), SAN_ENV), jc)
    _check_compose(_run(exe, "compose", _compose_input(cc), SAN_ENV), cc)
    _check_splits(_run(exe, "split", _split_input(sc), SAN_ENV), sc)


# ---- the entries on the real library, without a GPU ----
APPEND_SYMBOLS = ("seeqdevScanTallyHoldAppend", "seeqdevScanTallyHoldAppendLibrary", "seeqdevScanTallyHoldColumns", "seeqdevScanCopyHeld", "seeqdevTallySplit")


def test_append_symbols_exported(capi):
    L = capi.lib()
    hdr = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    for name in APPEND_SYMBOLS:
        assert name in capi.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name


def test_append_counts_layout(capi):
    t = capi.seeqdev_tally_append_counts_t
    assert C.sizeof(t) == 48
    assert [(n, getattr(t, n).offset) for n, _ in t._fields_] == [("nrecords", 0), ("nbefore", 8), ("nheld", 16), ("ndropped", 24), ("width", 32), ("key_bits", 36),
                                                                  ("ncolumns", 40), ("reserved", 44)]
    hdr = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} seeqdev_tally_append_counts_t;\s*/\* 48 bytes \*/", hdr).group(1)
    assert re.findall(r"^\s*uint\d+_t\s+(\w+);", body, re.M) == [n for n, _ in t._fields_]
    ah = open(os.path.join(CSRC, "seeq_tally_append.h")).read()
    assert int(re.search(r"#define\s+SEEQ_TALLY_COLUMNS\s+(\d+)", ah).group(1)) == capi.SEEQDEV_TALLY_COLUMNS == COLUMNS
    assert int(re.search(r"#define\s+SEEQ_TALLY_WORD_BITS\s+(\d+)", ah).group(1)) == WORD_BITS
    assert "injective" in ah and "column-major" in ah


def _einval(call):
    C.set_errno(0)
    assert call() == -1
    assert C.get_errno() == errno.EINVAL


def test_append_argument_checks_without_a_device(capi):
    # The checks come before the device is touched: the stand-in context is all zeros -- no completed hold, no library, no inserts,
    # demux or gate result, nothing fetched.
    L = capi.lib()
    ctx = C.addressof(C.create_string_buffer(8192))
    text = C.cast(C.c_char_p(b"ACGT\n"), C.c_void_p)
    hc, lc, ac = capi.seeqdev_tally_hold_counts_t(), capi.seeqdev_tally_library_counts_t(), capi.seeqdev_tally_append_counts_t()
    INS, HITS, DEMUX, GATED = capi.SEEQDEV_TALLY_INSERTS, capi.SEEQDEV_TALLY_HITS, capi.SEEQDEV_TALLY_DEMUX, capi.SEEQDEV_TALLY_GATED
    for entry, col in ((L.seeqdevScanTallyHoldAppend, hc), (L.seeqdevScanTallyHoldAppendLibrary, lc)):
        for source in (INS, HITS, GATED):
            _einval(lambda: entry(None, source, text, 5, C.byref(col), C.byref(ac)))         # NULL context
            _einval(lambda: entry(ctx, source, text, 5, None, C.byref(ac)))                  # NULL column
            _einval(lambda: entry(ctx, source, text, 5, C.byref(col), None))                 # NULL counts
            _einval(lambda: entry(ctx, source, None, 5, C.byref(col), C.byref(ac)))          # NULL text with bytes
            _einval(lambda: entry(ctx, source, text, 5, C.byref(col), C.byref(ac)))          # no completed hold (no library)
        for source in (3, -1, 255):
            _einval(lambda: entry(ctx, source, text, 5, C.byref(col), C.byref(ac)))          # an unknown source
    for source in (INS, HITS, GATED, DEMUX):
        _einval(lambda: L.seeqdevScanTallyHoldAppend(ctx, source, text, 5, C.byref(hc), C.byref(ac)))
        assert "held column" in capi.error_text()                                           # the hold is looked for before the source's own result
    _einval(lambda: L.seeqdevScanTallyHoldAppendLibrary(ctx, INS, text, 5, C.byref(lc), C.byref(ac)))
    assert "library" in capi.error_text()
    C.set_errno(0)
    _einval(lambda: L.seeqdevScanTallyHoldAppendLibrary(ctx, DEMUX, None, 0, C.byref(lc), C.byref(ac)))      # demux names no library source
    # the columns and the copy: a context without a column has none
    w = (C.c_uint32 * 8)(*([7] * 8))
    assert L.seeqdevScanTallyHoldColumns(ctx, w, 8) == 0 and list(w) == [7] * 8 and L.seeqdevScanTallyHoldColumns(ctx, None, 0) == 0
    _einval(lambda: L.seeqdevScanTallyHoldColumns(None, w, 8))
    _einval(lambda: L.seeqdevScanTallyHoldColumns(ctx, None, 8))
    _einval(lambda: L.seeqdevScanTallyHoldColumns(ctx, w, -1))
    lines, keys = (C.c_uint32 * 2)(), (C.c_uint64 * 2)()
    _einval(lambda: L.seeqdevScanCopyHeld(None, None, None, 0, 0))
    _einval(lambda: L.seeqdevScanCopyHeld(ctx, lines, keys, 0, 1))
    _einval(lambda: L.seeqdevScanCopyHeld(ctx, lines, None, 0, 1))
    _einval(lambda: L.seeqdevScanCopyHeld(ctx, None, None, 0, 1))
    _einval(lambda: L.seeqdevScanCopyHeld(ctx, lines, keys, 1, 0))
    assert L.seeqdevScanCopyHeld(ctx, lines, keys, 0, 0) == 0 and L.seeqdevScanCopyHeld(ctx, None, None, 0, 0) == 0


def _c_split(L, key, widths):
    w = (C.c_uint32 * max(len(widths), 1))(*widths)
    out = (C.c_uint64 * max(len(widths), 1))()
    C.set_errno(0)
    rc = L.seeqdevTallySplit(key, w, len(widths), out)
    assert (rc, C.get_errno()) in ((0, 0), (-1, errno.EINVAL))
    return list(out)[:len(widths)] if rc == 0 else None


def test_tally_split_round_trips_and_refuses(capi):
    L = capi.lib()
    for key, widths in _split_cases():
        if len(widths) <= 8:                                # (beyond eight the C entry reads no width: the array may be short)
            assert _c_split(L, key, widths) == py_split(key, widths), (key, widths)
    assert _c_split(L, 5, [3] * 9) is None and _c_split(L, 0, []) is None
    for widths, keys in _compose_cases():
        word = 0
        for w, k in zip(widths, keys):
            word = word << w | k
        assert _c_split(L, word, widths) == keys
    out = (C.c_uint64 * 2)()
    _einval(lambda: L.seeqdevTallySplit(1, None, 2, out))
    _einval(lambda: L.seeqdevTallySplit(1, (C.c_uint32 * 2)(1, 1), 2, None))


def test_hold_split_is_the_split_of_every_key(capi):
    from seeq_amd import device as dev
    L = capi.lib()
    rng = random.Random(53)
    for widths in ([33, 17], [8, 22, 17], [41], [0, 5], [1] * 8, [7, 8, 8, 8, 8, 8, 8, 8]):
        keys = np.array([rng.getrandbits(sum(widths)) for _ in range(300)] + [0, (1 << sum(widths)) - 1], dtype=np.uint64)
        cols = dev.hold_split(keys, widths)
        assert len(cols) == len(widths) and all(c.dtype == np.uint64 and len(c) == len(keys) for c in cols)
        assert [[int(c[i]) for c in cols] for i in range(len(keys))] == [_c_split(L, int(k), widths) for k in keys]
    assert [c.tolist() for c in dev.hold_split(np.zeros(0, dtype=np.uint64), [3, 2])] == [[], []]
    rec = np.array([(5 << 2 | 3, 9, 1)], dtype=dev.TALLY_PAIR_DTYPE)                          # a field of a structured table: a strided view
    assert [int(c[0]) for c in dev.hold_split(rec["group"], [3, 2])] == [5, 3]
    for bad in (lambda: dev.hold_split(keys, []), lambda: dev.hold_split(keys, [1] * 9), lambda: dev.hold_split(keys, [32, 32]),
                lambda: dev.hold_split(np.array([8], dtype=np.uint64), [1, 2])):
        with pytest.raises(ValueError):
            bad()
