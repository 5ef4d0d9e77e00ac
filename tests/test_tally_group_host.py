"""CPU: the grouped tally's rule of seeq_amd/csrc/seeq_tally_group.h -- the group of a line, what a member span is, the pass count, the
head predicates, the two tables -- compiled for the host by plain g++ (tests/tally_group_host_driver.cpp) and compared with a
restatement in Python that takes a span's key from test_tally_host.py_key.  Once more as a stand-alone program under
-fsanitize=address,undefined.  Then the entries on the real library: exports, layouts, dtypes, the argument checks (which run before
any device call and so fail the same way without a GPU), the copy entries' bounds, and tally_members."""
import collections
import ctypes as C
import errno
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_tally_host import FOREIGN, LONG, OK, py_key

CSRC = os.path.join(ROOT, "seeq_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "build")
SRC = os.path.join(ROOT, "tests", "tally_group_host_driver.cpp")
BAD, UNGROUPED = 3, 4
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("seeq_tally_group.h", "seeq_tally.h", "seeq_strand.h", "seeq_tiles.h")]
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
def py_group_of(held, line):
    """held: [(line, key)] in record order -> the key of the FIRST record of that line, 0 when there is none."""
    return next((k for ln, k in held if ln == line), 0)


def py_tables(items):
    """items: [(g, m)], (0, 0) for what did not pair -> (pair table [(g, m, count)], group table [(g, count, first, ndistinct)])."""
    tab = collections.Counter(x for x in items if x[0])
    pairs = [(g, m, tab[g, m]) for g, m in sorted(tab)]
    groups = []
    for j, (g, m, c) in enumerate(pairs):
        if not groups or groups[-1][0] != g:
            groups.append([g, 0, j, 0])
        groups[-1][1] += c
        groups[-1][3] += 1
    return pairs, [tuple(x) for x in groups]


def py_passes(npaired, max_len, key_bits):
    return ((2 * max_len + 1 + 7) // 8 + (key_bits + 7) // 8) if npaired else 0


def py_pairs(held, members):
    """members: [(line, bytes, or None for a span with end < start)] -> (counts in the driver's order, pairs, groups)."""
    cnt = collections.Counter()
    items, longest = [], 0
    for line, seq in members:
        kind, m = (BAD, 0) if seq is None else py_key(seq)
        g = py_group_of(held, line)
        if kind == OK and not g:
            kind = UNGROUPED
        cnt[kind] += 1
        items.append((g, m) if kind == OK else (0, 0))
        if kind == OK:
            longest = max(longest, len(seq))
    bits = max([k.bit_length() for _, k in held], default=0)
    pairs, groups = py_tables(items)
    return (cnt[OK], cnt[LONG], cnt[FOREIGN], cnt[UNGROUPED], cnt[BAD], longest, bits, py_passes(cnt[OK], longest, bits)), pairs, groups


def _held_text(held):
    return "H %d\n%s" % (len(held), "".join("%d %x\n" % h for h in held))


def _read_tables(lines, at):
    np_ = int(lines[at].split()[1])
    assert lines[at].startswith("P ")
    pairs = [tuple(int(x, 16) if k < 2 else int(x) for k, x in enumerate(ln.split())) for ln in lines[at + 1:at + 1 + np_]]
    at += 1 + np_
    assert lines[at].startswith("G ")
    ng = int(lines[at].split()[1])
    groups = [tuple(int(x, 16) if k == 0 else int(x) for k, x in enumerate(ln.split())) for ln in lines[at + 1:at + 1 + ng]]
    return pairs, groups, at + 1 + ng


# ---- tally_group_of ----
def _group_cases():
    rng = random.Random(7)
    k = lambda s: py_key(s)[1]                              # noqa: E731
    cases = [([], [0, 1, 5, 2 ** 32 - 1]),                                                   # nh = 0
             ([(5, k(b"ACGT"))], [0, 4, 5, 6, 2 ** 32 - 1]),
             ([(3, 7), (3, 9), (3, 11), (8, 0), (8, 13), (20, 5)], [0, 1, 2, 3, 4, 7, 8, 9, 19, 20, 21]),      # repeated lines: the first wins, a keyless first too
             ([(10, 1), (12, 2), (40, 3), (41, 4), (1000, 5)], [9, 10, 11, 12, 13, 39, 40, 41, 42, 999, 1000, 1001]),      # gaps; below the first, above the last
             ([(2 ** 32 - 1, 6)], [2 ** 32 - 2, 2 ** 32 - 1, 0])]
    for nh in (1, 2, 3, 63, 64, 65, 1000):
        line, held = 0, []
        for _ in range(nh):
            line += rng.choice([0, 0, 1, 1, 1, 2, 7])
            held.append((max(line, 1), rng.choice([0, rng.getrandbits(63) | 1, rng.randrange(1, 256)])))
        qs = sorted({ln + d for ln, _ in held for d in (-1, 0, 1) if ln + d >= 0})
        cases.append((held, qs))
    return cases


def _check_groups(lines, cases):
    at = 0
    hit = miss = 0
    for held, qs in cases:
        got = [int(x, 16) for x in lines[at:at + len(qs)]]
        exp = [py_group_of(held, q) for q in qs]
        assert got == exp, (held[:8], list(zip(qs, got, exp))[:8])
        hit += sum(1 for e in exp if e)
        miss += sum(1 for e in exp if not e)
        at += len(qs)
    assert lines[at:] in ([], [""]) and hit > 500 and miss > 500


def _group_input(cases):
    return "".join(_held_text(h) + "Q %d\n%s\n" % (len(q), " ".join(map(str, q))) for h, q in cases)


def test_group_of_a_line_on_the_host():
    cases = _group_cases()
    _check_groups(_run(_build("tally_group_host_driver", []), "group", _group_input(cases)), cases)
    f = subprocess.run([_build("tally_group_host_driver", [])], capture_output=True, text=True, timeout=60).stdout.split()
    hdr = open(os.path.join(CSRC, "seeq_tally.h")).read()
    assert f[0] == "G" and int(f[1]) == int(re.search(r"#define\s+SEEQ_TALLY_TILE\s+(\d+)", hdr).group(1)) == 1024
    assert [int(x) for x in f[2:]] == [UNGROUPED, 32, 31]


# ---- the pass count, the demux group ----
PASS_CASES = [(0, 0, 0), (0, 31, 63), (5, 0, 1), (5, 3, 1), (5, 4, 1), (5, 31, 1), (5, 0, 8), (5, 0, 9), (5, 0, 63), (5, 3, 8), (5, 4, 9), (5, 31, 63),
              (1, 12, 25), (2 ** 32 - 1, 31, 63)]


def test_pass_count_on_the_host():
    lines = _run(_build("tally_group_host_driver", []), "passes", "".join("%d %d %d\n" % c for c in PASS_CASES))
    got = [tuple(int(x) for x in ln.split()) for ln in lines if ln]
    assert [g[0] for g in got] == [py_passes(*c) for c in PASS_CASES]
    by = dict(zip(PASS_CASES, got))
    assert by[0, 0, 0][0] == by[0, 31, 63][0] == 0                                   # nothing paired: no pass
    assert [by[5, n, 1] for n in (0, 3, 4, 31)] == [(2, 1), (2, 1), (3, 2), (9, 8)]    # member-only lengths beside a one-digit group
    assert [by[5, 0, b][0] - 1 for b in (1, 8, 9, 63)] == [1, 1, 2, 8]                # the group word: key_bits 1 / 8 / 9 / 63
    assert by[5, 31, 63] == (16, 8)


def test_demux_group_on_the_host():
    words = [(dist, pat, margin) for dist in (0, 3, 0xFFFF) for pat in (0, 1, 127, 254) for margin in (0, 1, 2, 255)]
    lines = _run(_build("tally_group_host_driver", []), "demux", "".join("%x\n" % (d | p << 16 | m << 24) for d, p, m in words))
    got = [tuple(int(x, 16 if k == 0 else 10) for k, x in enumerate(ln.split())) for ln in lines if ln]
    assert got == [((p + 1) if m else 0, (p + 1).bit_length() if m else 0) for d, p, m in words]
    assert max(g[1] for g in got) == 8                      # pattern 254 is group 255: eight bits, one pass


# ---- both head predicates and both tables from sorted pair lists ----
def _table_cases():
    rng = random.Random(17)
    cases = [[], [(0, 0)], [(0, 0)] * 3, [(5, 9)], [(0, 0), (5, 9)], [(5, 9)] * 4,                      # a group with one pair; one spanning everything
             [(0, 0)] * 5 + [(2, 7), (2, 7), (2, 8), (3, 7), (3, 7), (3, 7), (4, 1)],                   # (0, 0) items in front
             [(1, 1), (1, 2), (2, 1), (2, 2)],                                                         # differ in one word only
             [(7, m) for m in range(1, 40)],                                                           # one group, all distinct
             [(g, 3) for g in range(1, 40)],                                                           # all groups of one pair, one member
             [(2 ** 63 - 1, 2 ** 63 - 1)] * 2 + [(2 ** 64 - 1, 1)]]
    for _ in range(6):
        items = [(rng.randrange(1, 6), rng.randrange(1, 9)) if rng.random() < 0.8 else (0, 0) for _ in range(rng.randrange(1, 400))]
        cases.append(sorted(items))
    return cases


def _check_table_cases(lines, cases):
    at = 0
    for items in cases:
        heads = [tuple(int(x) for x in ln.split()) for ln in lines[at:at + len(items)]]
        exp = [(int(g != 0 and (i == 0 or items[i - 1] != (g, m))), int(g != 0 and (i == 0 or items[i - 1][0] != g))) for i, (g, m) in enumerate(items)]
        assert heads == exp
        assert all(ph >= gh for ph, gh in heads)            # every group head is a pair head
        pairs, groups, at = _read_tables(lines, at + len(items))
        epairs, egroups = py_tables(items)
        assert (pairs, groups) == (epairs, egroups), items[:10]
        npaired = sum(1 for g, _ in items if g)
        assert sum(c for *_, c in pairs) == npaired == sum(g[1] for g in groups) and sum(g[3] for g in groups) == len(pairs)
    assert lines[at:] in ([], [""])


def _table_input(cases):
    return "".join("N %d\n%s\n" % (len(c), " ".join("%x %x" % x for x in c)) for c in cases)


def test_heads_and_tables_on_the_host():
    cases = _table_cases()
    _check_table_cases(_run(_build("tally_group_host_driver", []), "table", _table_input(cases)), cases)


# ---- the whole rule: classification, sort, tables ----
def _pairs_cases():
    rng = random.Random(27)
    mk = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))      # noqa: E731
    k = lambda s: py_key(s)[1]                              # noqa: E731
    g1, g2 = k(b"ACGTACGTACGTACGTACGT"), k(b"ACGTACGTACGTACGTACGA")
    # the four-way classification and its order: long before foreign, both before ungrouped, on lines with and without a group
    held = [(1, g1), (2, 0), (4, g2), (4, g1), (6, g1)]
    members = [(1, b"ACGT"), (1, b"N" * 40), (1, b"ACGN"), (1, None), (2, b"ACGT"), (2, b"A" * 32), (2, b"NN"), (3, b"ACGT"), (3, b"A" * 32),
               (4, b"ACGT"), (4, b"acgu"), (4, b""), (5, b"N"), (6, b""), (7, b"G" * 31)]
    cases = [(held, members), ([], [(1, b"ACGT"), (2, b"N"), (3, b"A" * 40)]), (held, []), ([], []),
             ([(1, 1)], [(1, b"")]),                                                        # the empty insert as group and as member: key 1
             ([(1, 2 ** 63 - 1), (2, 2 ** 62)], [(1, b"G" * 31), (2, b"G" * 31), (1, b"A" * 31), (1, b"G" * 31)])]      # 16 passes
    for longest, bits in ((3, 1), (4, 8), (12, 9), (31, 63), (0, 25)):
        held, line = [], 0
        pool_g = [rng.getrandbits(bits) | (1 << (bits - 1)) for _ in range(6)]
        for _ in range(300):
            line += rng.choice([1, 1, 1, 2, 0])
            held.append((max(line, 1), rng.choice(pool_g + [0])))
        pool_m = [mk(rng.randrange(0, longest + 1)) for _ in range(12)] + [mk(longest), b"N", mk(33)]
        members = sorted(((rng.randrange(1, line + 3), rng.choice(pool_m)) for _ in range(900)), key=lambda x: x[0])
        cases.append((held, members))
    return cases


def _pairs_input(cases):
    enc = lambda s: "!" if s is None else (s.hex() or "-")   # noqa: E731
    return "".join(_held_text(h) + "M %d\n%s" % (len(m), "".join("%d %s\n" % (ln, enc(s)) for ln, s in m)) for h, m in cases)


def _check_pairs(lines, cases):
    at = 0
    seen = set()
    for held, members in cases:
        counts, pairs, groups = py_pairs(held, members)
        assert lines[at].startswith("C ") and tuple(int(x) for x in lines[at].split()[1:]) == counts, (lines[at], counts)
        gp, gg, at = _read_tables(lines, at + 1)
        assert (gp, gg) == (pairs, groups)
        assert sum(counts[:5]) == len(members) and sum(c for *_, c in gp) == counts[0]
        seen.add(counts[7])
    assert lines[at:] in ([], [""])
    assert {0, 2, 3, 6, 16, 5} <= seen


def test_the_restatement_itself():
    k = lambda s: py_key(s)[1]                              # noqa: E731
    held = [(3, 7), (3, 9), (8, 0), (8, 13)]
    assert [py_group_of(held, ln) for ln in (2, 3, 4, 8, 9)] == [0, 7, 0, 0, 0]
    counts, pairs, groups = py_pairs([(1, k(b"AC")), (2, k(b"AC")), (3, k(b"G"))], [(1, b"TT"), (2, b"TT"), (2, b"TA"), (3, b"TT"), (4, b"TT"), (1, b"N"), (1, b"A" * 32)])
    assert counts == (4, 1, 1, 1, 0, 2, 5, 2)
    assert pairs == [(k(b"G"), k(b"TT"), 1), (k(b"AC"), k(b"TA"), 1), (k(b"AC"), k(b"TT"), 2)]      # by group (the shorter first), then member
    assert groups == [(k(b"G"), 1, 0, 1), (k(b"AC"), 3, 1, 2)]


def test_classification_sort_and_tables_on_the_host():
    cases = _pairs_cases()
    _check_pairs(_run(_build("tally_group_host_driver", []), "pairs", _pairs_input(cases)), cases)


def test_grouped_tally_rule_under_sanitizers():
    exe = _build("tally_group_host_driver_asan", SAN)
    gc, tc, pc = _group_cases(), _table_cases(), _pairs_cases()
    _check_groups(_run(exe, "group", _group_input(gc), SAN_ENV), gc)
    _check_table_cases(_run(exe, "table", _table_input(tc), SAN_ENV), tc)
    _check_pairs(_run(exe, "pairs", _pairs_input(pc), SAN_ENV), pc)


# ---- the entries on the real library, without a GPU ----
GROUP_SYMBOLS = ("seeqdevScanTallyHold", "seeqdevScanTallyGrouped", "seeqdevScanTallyPairsDevice", "seeqdevScanTallyGroupsDevice",
                 "seeqdevScanCopyTallyPairs", "seeqdevScanCopyTallyGroups", "seeqdevScanLastTallyGroupedMs")


def test_grouped_tally_symbols_exported(capi):
    L = capi.lib()
    hdr = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    for name in GROUP_SYMBOLS:
        assert name in capi.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name


def test_grouped_tally_layouts(capi):
    from seeq_amd import device as dev
    offs = lambda t: [(n, getattr(t, n).offset) for n, _ in t._fields_]      # noqa: E731
    assert C.sizeof(capi.seeqdev_tally_pair_t) == 24 and offs(capi.seeqdev_tally_pair_t) == [("group", 0), ("member", 8), ("count", 16)]
    assert C.sizeof(capi.seeqdev_tally_group_t) == 24
    assert offs(capi.seeqdev_tally_group_t) == [("group", 0), ("count", 8), ("first", 16), ("ndistinct", 20)]
    assert C.sizeof(capi.seeqdev_tally_hold_counts_t) == 48
    assert offs(capi.seeqdev_tally_hold_counts_t) == [("nspans", 0), ("nheld", 8), ("nlong", 16), ("nforeign", 24), ("nambiguous", 32), ("max_len", 40),
                                                      ("key_bits", 44)]
    assert C.sizeof(capi.seeqdev_tally_grouped_counts_t) == 64
    assert offs(capi.seeqdev_tally_grouped_counts_t) == [("nspans", 0), ("npaired", 8), ("nlong", 16), ("nforeign", 24), ("nungrouped", 32), ("npairs", 40),
                                                         ("ngroups", 48), ("max_len", 56), ("passes", 60)]
    hdr = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    assert int(re.search(r"#define\s+SEEQDEV_TALLY_DEMUX\s+(\d+)", hdr).group(1)) == capi.SEEQDEV_TALLY_DEMUX == 2
    for t in ("seeqdev_tally_pair_t", "seeqdev_tally_group_t", "seeqdev_tally_hold_counts_t", "seeqdev_tally_grouped_counts_t"):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % t, hdr).group(1)
        names = [n for decl in re.findall(r"^\s*uint\d+_t\s+([^;]+);", body, re.M) for n in re.split(r"\s*,\s*", decl)]
        assert names == [n for n, _ in getattr(capi, t)._fields_], t
    assert dev.TALLY_PAIR_DTYPE.names == ("group", "member", "count") and dev.TALLY_PAIR_DTYPE.itemsize == 24
    assert dev.TALLY_GROUP_DTYPE.names == ("group", "count", "first", "ndistinct") and dev.TALLY_GROUP_DTYPE.itemsize == 24
    assert [dev.TALLY_GROUP_DTYPE.fields[n][1] for n in dev.TALLY_GROUP_DTYPE.names] == [0, 8, 16, 20]
    assert [dev.TALLY_PAIR_DTYPE.fields[n][1] for n in dev.TALLY_PAIR_DTYPE.names] == [0, 8, 16]


def _einval(call):
    C.set_errno(0)
    assert call() == -1
    assert C.get_errno() == errno.EINVAL


def test_grouped_tally_argument_checks_without_a_device(capi):
    # The checks come before the device is touched: the stand-in context is all zeros -- no completed inserts, demux or hold call,
    # nothing fetched.
    L = capi.lib()
    ctx = C.addressof(C.create_string_buffer(8192))
    text = C.cast(C.c_char_p(b"ACGT\n"), C.c_void_p)
    hc, gc = capi.seeqdev_tally_hold_counts_t(), capi.seeqdev_tally_grouped_counts_t()
    INS, HITS, DEMUX = capi.SEEQDEV_TALLY_INSERTS, capi.SEEQDEV_TALLY_HITS, capi.SEEQDEV_TALLY_DEMUX
    for source in (INS, HITS):
        _einval(lambda: L.seeqdevScanTallyHold(None, source, text, 5, C.byref(hc)))         # NULL context
        _einval(lambda: L.seeqdevScanTallyHold(ctx, source, text, 5, None))                 # NULL counts
        _einval(lambda: L.seeqdevScanTallyHold(ctx, source, None, 5, C.byref(hc)))          # NULL text with bytes
        _einval(lambda: L.seeqdevScanTallyHold(ctx, source, text, 5, C.byref(hc)))          # no completed inserts call / nothing fetched
        _einval(lambda: L.seeqdevScanTallyHold(ctx, source, None, 0, C.byref(hc)))          # ... and no staged text / hits without text
        _einval(lambda: L.seeqdevScanTallyGrouped(None, source, text, 5, C.byref(gc)))
        _einval(lambda: L.seeqdevScanTallyGrouped(ctx, source, text, 5, None))
        _einval(lambda: L.seeqdevScanTallyGrouped(ctx, source, None, 5, C.byref(gc)))
        _einval(lambda: L.seeqdevScanTallyGrouped(ctx, source, text, 5, C.byref(gc)))       # no completed hold
        _einval(lambda: L.seeqdevScanTallyGrouped(ctx, source, None, 0, C.byref(gc)))
    assert "held column" in capi.error_text()
    _einval(lambda: L.seeqdevScanTallyHold(None, DEMUX, None, 0, C.byref(hc)))
    _einval(lambda: L.seeqdevScanTallyHold(ctx, DEMUX, None, 0, None))
    for t, n in ((None, 0), (text, 5), (None, 5)):                                          # the text is ignored: no completed demux whatever it is
        _einval(lambda: L.seeqdevScanTallyHold(ctx, DEMUX, t, n, C.byref(hc)))
        assert "demux" in capi.error_text()
    for source in (3, -1, 255):
        _einval(lambda: L.seeqdevScanTallyHold(ctx, source, text, 5, C.byref(hc)))          # an unknown source
    for source in (DEMUX, 3, -1, 255):
        _einval(lambda: L.seeqdevScanTallyGrouped(ctx, source, text, 5, C.byref(gc)))       # demux names no member source
    tc = capi.seeqdev_tally_counts_t()
    _einval(lambda: L.seeqdevScanTally(ctx, DEMUX, text, 5, C.byref(tc)))                    # and the plain tally knows no source 2
    # the copy entries: a context without tables has no entry
    for copy, entry in ((L.seeqdevScanCopyTallyPairs, capi.seeqdev_tally_pair_t), (L.seeqdevScanCopyTallyGroups, capi.seeqdev_tally_group_t)):
        out = (entry * 2)()
        _einval(lambda: copy(None, None, 0, 0))
        _einval(lambda: copy(ctx, None, 0, 1))
        _einval(lambda: copy(ctx, out, 0, 1))
        _einval(lambda: copy(ctx, out, 1, 0))
        assert copy(ctx, out, 0, 0) == 0 and copy(ctx, None, 0, 0) == 0
    for ptr in (L.seeqdevScanTallyPairsDevice, L.seeqdevScanTallyGroupsDevice):
        assert ptr(None) is None and ptr(ctx) is None
    ms = C.c_float(1.0)
    _einval(lambda: L.seeqdevScanLastTallyGroupedMs(ctx, None))
    _einval(lambda: L.seeqdevScanLastTallyGroupedMs(None, C.byref(ms)))
    assert L.seeqdevScanLastTallyGroupedMs(ctx, C.byref(ms)) == 0 and ms.value == 0.0


def test_tally_members_is_a_search_over_the_groups():
    from seeq_amd import device as dev
    items = [(3, 5)] * 4 + [(3, 9)] + [(10, 1), (10, 2), (10, 2), (2 ** 63 - 1, 7), (1, 1)]
    pairs, groups = py_tables(items)
    res = dict(pairs=np.array(pairs, dtype=dev.TALLY_PAIR_DTYPE), groups=np.array(groups, dtype=dev.TALLY_GROUP_DTYPE))
    for g in (1, 3, 10, 2 ** 63 - 1):
        got = dev.tally_members(res, g)
        assert got.dtype == dev.TALLY_PAIR_DTYPE and [tuple(int(x) for x in r) for r in got] == [p for p in pairs if p[0] == g]
    assert dev.tally_members(res, 3)["count"].tolist() == [4, 1]
    for g in (0, 2, 4, 11, 2 ** 63, 2 ** 64 - 1):
        assert len(dev.tally_members(res, g)) == 0
    empty = dict(pairs=res["pairs"][:0], groups=res["groups"][:0])
    assert len(dev.tally_members(empty, 3)) == 0 and dev.tally_members(empty, 3).dtype == dev.TALLY_PAIR_DTYPE
