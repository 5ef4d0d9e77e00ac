"""CPU: the collapse rule of seeq_amd/csrc/seeq_tally_collapse.h -- precedes, the count threshold, the parent of a pair, the group rows --
compiled for the host by plain g++ (tests/tally_collapse_host_driver.cpp) and compared with a restatement in Python that knows NO
neighbours: it decodes the members of a group and takes the brute-force Hamming distance between strings of equal length.  Once more as a
stand-alone program under -fsanitize=address,undefined.  Then the entries on the real library: exports, the structs' layouts, every
refusal (which comes before any device call and so fails the same way without a GPU), and collapse_fold."""
import ctypes as C
import errno
import functools
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_tally_host import py_decode, py_key

CSRC = os.path.join(ROOT, "seeq_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "build")
SRC = os.path.join(ROOT, "tests", "tally_collapse_host_driver.cpp")
DIRECTIONAL, ANY = 0, 1
RULES = (DIRECTIONAL, ANY)
M64 = 2 ** 64 - 1
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("seeq_tally_collapse.h", "seeq_tally_library.h", "seeq_tally.h", "seeq_strand.h", "seeq_tiles.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + ["-I" + CSRC, SRC, "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe, mode, text, env=None):
    r = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r.stdout.split("\n")


# ---- the rule, restated without neighbours ----
def py_table(items):
    """items: [(group key, member bytes, count)], every (group, member) once -> (pair table [(g, m, c)] ascending by (g, m), group table
    [(g, reads, first, ndistinct)])."""
    pairs = sorted((g, py_key(m)[1], c) for g, m, c in items)
    assert all(m for _, m, _ in pairs) and len({p[:2] for p in pairs}) == len(pairs)
    return pairs, py_groups(pairs)


def py_groups(pairs):
    groups = []
    for j, (g, m, c) in enumerate(pairs):
        if not groups or groups[-1][0] != g:
            groups.append([g, 0, j, 0])
        groups[-1][1] += c
        groups[-1][3] += 1
    return [tuple(x) for x in groups]


def py_precedes(cj, mj, ci, mi):
    return cj > ci or (cj == ci and mj < mi)


def py_collapse(pairs, rule):
    """pairs: [(g, m, c)] ascending by (g, m) -> (parent [index], rows [(nroots, nabsorbed, absorbed_reads)] per group in order): per group
    every pair against every other one, the members decoded and compared base by base."""
    parent = list(range(len(pairs)))
    rows = []
    at = 0
    while at < len(pairs):
        end = at
        while end < len(pairs) and pairs[end][0] == pairs[at][0]:
            end += 1
        seqs = [py_decode(m) for _, m, _ in pairs[at:end]]
        for i in range(at, end):
            si, (_, mi, ci) = seqs[i - at], pairs[i]
            cands = []
            for j in range(at, end):
                sj, (_, mj, cj) = seqs[j - at], pairs[j]
                if len(sj) != len(si) or sum(1 for x, y in zip(si, sj) if x != y) != 1:
                    continue
                if py_precedes(cj, mj, ci, mi) and (rule == ANY or cj >= 2 * ci - 1):
                    cands.append(j)
            if cands:
                parent[i] = max(cands, key=lambda j: (pairs[j][2], -pairs[j][1]))
        absorbed = [i for i in range(at, end) if parent[i] != i]
        rows.append((end - at - len(absorbed), len(absorbed), sum(pairs[i][2] for i in absorbed)))
        at = end
    return parent, rows


def np_collapse(pairs, rule):
    """py_collapse for tables too large for it (the GPU tests' 256 tiles): still no neighbour is ever computed.  Two strings of equal length
    differ in exactly position p iff they are distinct and agree once position p is blanked: per p the pairs are bucketed by (group,
    length, blanked string), and the one pair of a bucket that precedes all its others is the only candidate the bucket can give any of
    them (it has the highest count: if it fails the threshold, so do the rest).  Checked against py_collapse below.
    pairs: structured array with fields group, member, count (uint64), ascending -> (parent uint32[n], rows [(nroots, nabsorbed, reads)])."""
    return np_collapse_both(pairs)[rule]


def np_collapse_both(pairs):
    """{rule: np_collapse's result}: the buckets are made once for both rules."""
    n = len(pairs)
    g, m, c = (np.ascontiguousarray(pairs[k], dtype=np.uint64) for k in ("group", "member", "count"))
    length = np.array([(int(x).bit_length() - 1) // 2 for x in m], dtype=np.int64) if n else np.zeros(0, dtype=np.int64)
    gid = np.unique(g, return_inverse=True)[1].astype("<u4") if n else np.zeros(0, dtype="<u4")
    rowbytes = np.full((n, 36), 255, dtype=np.uint8)        # 31 bases (255 behind the end), the length, the group's rank
    for i in range(31):
        has = length > i
        sh = (2 * (length - 1 - i)).clip(0).astype(np.uint64)
        rowbytes[has, i] = ((m >> sh) & np.uint64(3))[has].astype(np.uint8)
    rowbytes[:, 31] = length
    if n:
        rowbytes[:, 32:36] = np.ascontiguousarray(gid).view(np.uint8).reshape(n, 4)
    idx = np.arange(n, dtype=np.int64)
    best = {rule: [np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.full(n, -1, dtype=np.int64)] for rule in RULES}
    for p in range(int(length.max()) if n else 0):
        sel = idx[length > p]
        blank = rowbytes[sel].copy()
        blank[:, p] = 254
        bucket = np.unique(np.ascontiguousarray(blank).view("V36").ravel(), return_inverse=True)[1].ravel()
        order = np.lexsort((m[sel], ~c[sel], bucket))       # by bucket, then the count descending, then the member ascending
        head = np.ones(len(sel), dtype=bool)
        head[1:] = bucket[order][1:] != bucket[order][:-1]
        first = np.zeros(int(bucket.max()) + 1, dtype=np.int64)
        first[bucket[order][head]] = sel[order][head]
        cand = first[bucket]
        cc, cm, ci = c[cand], m[cand], c[sel]
        for rule in RULES:
            bc, bm, bj = best[rule]
            ok = cand != sel
            if rule != ANY:
                ok = ok & ((cc - ci) >= (ci - np.uint64(1)))  # (the bucket's first has the highest count: no wrap)
            better = ok & ((bj[sel] < 0) | (cc > bc[sel]) | ((cc == bc[sel]) & (cm < bm[sel])))
            t = sel[better]
            bc[t], bm[t], bj[t] = cc[better], cm[better], cand[better]
    out = {}
    table = py_groups_np(g, c)
    for rule in RULES:
        bj = best[rule][2]
        parent = np.where(bj >= 0, bj, idx).astype(np.uint32)
        absorbed = parent != idx
        rows = []
        for _, _, first, nd in table:
            a = absorbed[first:first + nd]
            rows.append((int(nd - a.sum()), int(a.sum()), sum(int(x) for x in c[first:first + nd][a])))
        out[rule] = (parent, rows)
    return out


def py_groups_np(g, c):
    """The group table of a pair table given as columns (ascending groups)."""
    if not len(g):
        return []
    starts = np.flatnonzero(np.concatenate(([True], g[1:] != g[:-1])))
    ends = np.concatenate((starts[1:], [len(g)]))
    return [(int(g[s]), sum(int(x) for x in c[s:e]), int(s), int(e - s)) for s, e in zip(starts, ends)]


def as_array(pairs):
    return np.array(pairs, dtype=[("group", "<u8"), ("member", "<u8"), ("count", "<u8")])


# ---- the cases ----
def _sub(seq, at, other):
    """seq with the base at `at` replaced by the other-th different base (other in 1 .. 3)."""
    return seq[:at] + bytes([b"ACGT"[(b"ACGT".index(seq[at]) + other) % 4]]) + seq[at + 1:]


def hand_groups(big=True):
    """The named cases, one group each: [(name, [(member bytes, count)], {rule: {member: parent member or None for a root}})].  big: with
    the counts near 2^63 and 2^64 that no text can produce."""
    u = b"ACGTTGCAAGCT"
    chain = [u, _sub(u, 11, 1), _sub(_sub(u, 11, 1), 10, 1)]
    x, y, z = b"TTGACCGATCAG", _sub(b"TTGACCGATCAG", 0, 1), _sub(b"TTGACCGATCAG", 5, 2)
    lo, hi = sorted((x, y), key=lambda s: py_key(s)[1])
    cases = [
        ("chain 100 - 10 - 1", [(chain[0], 100), (chain[1], 10), (chain[2], 1)],
         {r: {chain[0]: None, chain[1]: chain[0], chain[2]: chain[1]} for r in RULES}),
        ("threshold met: 9 beside 5", [(x, 9), (y, 5)], {r: {x: None, y: x} for r in RULES}),
        ("threshold missed: 8 beside 5", [(x, 8), (y, 5)], {DIRECTIONAL: {x: None, y: None}, ANY: {x: None, y: x}}),
        ("5 beside 4", [(x, 5), (y, 4)], {DIRECTIONAL: {x: None, y: None}, ANY: {x: None, y: x}}),
        ("tied at 1: the smaller member is the root", [(x, 1), (y, 1)], {r: {lo: None, hi: lo} for r in RULES}),
        ("tied at 3", [(x, 3), (y, 3)], {DIRECTIONAL: {x: None, y: None}, ANY: {lo: None, hi: lo}}),
        ("two candidates, different counts", [(x, 2), (y, 40), (z, 50)], {r: {x: z, y: None, z: None} for r in RULES}),
        ("two candidates, equal counts", [(x, 2), (y, 40), (z, 40)],
         {r: {x: min((y, z), key=lambda s: py_key(s)[1]), y: None, z: None} for r in RULES}),
        ("a group of one pair", [(x, 7)], {r: {x: None} for r in RULES}),
        ("a member and its prefix", [(u, 9), (u[:11], 1), (u[1:], 1)], {r: {u: None, u[:11]: None, u[1:]: None} for r in RULES}),
    ]
    for n in (0, 1, 16, 17, 31):
        s = (b"ACGTTGCAAGCTTGACCGATCAGGATTACAT")[:n]
        if n == 0:
            cases.append(("length 0", [(s, 3)], {r: {s: None} for r in RULES}))
        else:
            t = _sub(s, n - 1, 2)
            cases.append(("length %d" % n, [(s, 9), (t, 2), (_sub(s, 0, 1), 1)], {r: {s: None, t: s, _sub(s, 0, 1): s} for r in RULES}))
    a, b = b"ACGT", b"ACGA"
    mixed = [(b"", 5), (b"A", 5), (b"C", 1), (a, 10), (b, 1), (a + b"A", 1), (b"ACG", 1)]
    cases.append(("mixed lengths", mixed, {r: {b"": None, b"A": None, b"C": b"A", a: None, b: a, a + b"A": None, b"ACG": None} for r in RULES}))
    # the same two neighbours in two adjacent groups: nothing crosses; the high count is in the other group each time
    cases.append(("adjacent groups, first", [(x, 50), (z, 1)], {r: {x: None, z: x} for r in RULES}))
    cases.append(("adjacent groups, second", [(x, 1), (z, 50)], {r: {x: z, z: None} for r in RULES}))
    # the last member of a group beside the first of the next: G sorts last, GGGC is the smallest member of the second group
    cases.append(("last member of a group", [(b"ACGT", 1), (b"GGGG", 1)], {r: {b"ACGT": None, b"GGGG": None} for r in RULES}))
    cases.append(("first member of the next", [(b"GGGC", 90), (b"GGGT", 1)], {r: {b"GGGC": None, b"GGGT": b"GGGC"} for r in RULES}))
    if big:
        cases += [
            ("2^64 - 1 beside 2^63: 2 c - 1 exactly", [(x, M64), (y, 2 ** 63)], {r: {x: None, y: x} for r in RULES}),
            ("2^64 - 2 beside 2^63", [(x, M64 - 1), (y, 2 ** 63)], {DIRECTIONAL: {x: None, y: None}, ANY: {x: None, y: x}}),
            ("2^64 - 1 beside 2^63 + 1: 2 c - 1 wraps to 1", [(x, M64), (y, 2 ** 63 + 1)], {DIRECTIONAL: {x: None, y: None}, ANY: {x: None, y: x}}),
        ]
    return cases


def hand_items(big=True, group_of=lambda k: k + 1):
    """The named cases as one table's items, case k in the group group_of(k) (ascending in k)."""
    return [(group_of(k), m, c) for k, (_, members, _) in enumerate(hand_groups(big)) for m, c in members]


def check_hand(pairs, parent, rule, big=True):
    """What the named cases are there for, asserted on a parent array whatever made it."""
    at = 0
    for name, members, want in hand_groups(big):
        seg = pairs[at:at + len(members)]
        where = {m: at + i for i, (_, m, _) in enumerate(seg)}
        for mb, pb in want[rule].items():
            i = where[py_key(mb)[1]]
            assert parent[i] == (i if pb is None else where[py_key(pb)[1]]), (name, rule, mb, pb, parent[i])
        at += len(members)
    assert at == len(pairs)


def random_table(seed, ngroups, npairs, length=6, pool=None):
    """A table whose members crowd a small space: plenty of neighbours, ties and chains."""
    rng = random.Random(seed)
    seen, items = set(), []
    while len(items) < npairs:
        g = rng.randrange(1, ngroups + 1) * 3
        n = rng.choice(pool) if pool else length
        m = bytes(rng.choice(b"ACGT") for _ in range(n))
        if (g, py_key(m)[1]) in seen:
            continue
        seen.add((g, py_key(m)[1]))
        items.append((g, m, rng.choice([1, 1, 1, 1, 2, 2, 3, 5, 9, 17, 100, 1000])))
    return items


@functools.lru_cache(maxsize=None)
def _expected():
    """Per table and rule the brute force's (parent, rows) -- computed once, shared by the plain and the sanitizer run."""
    return {(name, rule): py_collapse(pairs, rule) for name, (pairs, _) in all_tables() for rule in RULES}


@functools.lru_cache(maxsize=None)
def all_tables():
    return [("hand", py_table(hand_items()))] + [("single: " + name, py_table([(7, m, c) for m, c in members])) for name, members, _ in hand_groups()] + [
        ("empty", ([], [])),
        ("random, one group", py_table(random_table(1, 1, 900, 5))),
        ("random, many groups", py_table(random_table(2, 40, 3000, 4))),
        ("random, mixed lengths", py_table(random_table(3, 7, 2500, pool=(0, 1, 2, 3, 4, 5, 5, 5)))),
        ("random, every pair a group", py_table([(k + 1, m, c) for k, (_, m, c) in enumerate(random_table(4, 1, 600, 8))])),
        ("random, 300 groups", py_table(random_table(5, 300, 2000, 3)))]


def _table_input(pairs, groups, rule):
    return "T %d %d %d\n%s%s" % (len(pairs), len(groups), rule, "".join("%x %x %d\n" % p for p in pairs), "".join("%x %d %d %d\n" % g for g in groups))


def _check_tables(exe, env=None):
    tables = all_tables()
    text = "".join(_table_input(p, g, rule) for _, (p, g) in tables for rule in RULES)
    lines = _run(exe, "collapse", text, env)
    at = 0
    absorbed = {r: 0 for r in RULES}
    for name, (pairs, groups) in tables:
        for rule in RULES:
            parent, rows = _expected()[name, rule]
            assert lines[at] == "R %d %d %d 0" % (sum(r[0] for r in rows), sum(r[1] for r in rows), sum(r[2] for r in rows) & M64), (name, rule, lines[at])
            got = [] if lines[at + 1] == "-" else [int(x) for x in lines[at + 1].split()]
            assert got == parent, (name, rule, [(i, a, b) for i, (a, b) in enumerate(zip(got, parent)) if a != b][:5])
            got_rows = [tuple(int(x) for x in ln.split()) for ln in lines[at + 2:at + 2 + len(groups)]]
            assert got_rows == [(a, b, q & M64) for a, b, q in rows], (name, rule)
            assert all(a + b == g[3] and a >= 1 for (a, b, _), g in zip(rows, groups))
            at += 2 + len(groups)
            absorbed[rule] += sum(r[1] for r in rows)
            if name == "hand":
                check_hand(pairs, parent, rule)
            if name.startswith("random"):
                # the vectorised restatement the GPU tests use for large tables is the brute force
                nparent, nrows = np_collapse(as_array(pairs), rule)
                assert nparent.tolist() == parent and nrows == rows, (name, rule)
    assert lines[at:] in ([], [""])
    assert absorbed[ANY] > absorbed[DIRECTIONAL] > 1000      # the cases are not vacuous, and the threshold matters


def test_the_restatement_itself():
    k = lambda s: py_key(s)[1]                              # noqa: E731
    pairs, groups = py_table([(5, b"AAAA", 100), (5, b"AAAC", 10), (5, b"AACC", 1), (5, b"GGGG", 3), (9, b"AAAA", 1), (9, b"AAAC", 1), (9, b"AAA", 7)])
    assert [p[1] for p in pairs[:4]] == [k(b"AAAA"), k(b"AAAC"), k(b"AACC"), k(b"GGGG")] and groups == [(5, 114, 0, 4), (9, 9, 4, 3)]
    for rule in RULES:
        parent, rows = py_collapse(pairs, rule)
        assert parent == [0, 0, 1, 3, 4, 5, 5]              # the chain is not followed; AAA has another length; the tie goes to AAAA
        assert rows == [(2, 2, 11), (2, 1, 1)]
    pairs, _ = py_table([(1, b"ACGT", 8), (1, b"ACGA", 5)])
    assert py_collapse(pairs, DIRECTIONAL)[0] == [0, 1] and py_collapse(pairs, ANY)[0] == [1, 1]      # (ACGA sorts first: index 0)
    assert py_precedes(3, 9, 2, 1) and py_precedes(2, 1, 2, 9) and not py_precedes(2, 9, 2, 1) and not py_precedes(2, 5, 2, 5)
    for big in (True, False):
        for rule in RULES:
            pairs, _ = py_table(hand_items(big))
            check_hand(pairs, py_collapse(pairs, rule)[0], rule, big)


def test_order_and_threshold_on_the_host():
    cases = [(9, 5, 5, 6), (8, 5, 5, 6), (5, 5, 5, 6), (5, 6, 5, 5), (5, 5, 5, 5), (1, 1, 1, 2), (2, 9, 1, 1), (M64, 1, 2 ** 63, 2), (M64 - 1, 1, 2 ** 63, 2),
             (M64, 1, 2 ** 63 + 1, 2), (M64, 1, M64, 2), (M64, 2, M64, 1), (2 ** 63, 1, 2 ** 63, 2), (3, 1, 2, 2), (2, 1, 2, 2), (1, 1, 1, 1)]
    exe = _build("tally_collapse_host_driver", [])
    lines = _run(exe, "order", "".join("%d %x %d %x\n" % c for c in cases))
    for (cj, mj, ci, mi), ln in zip(cases, lines):
        pre = py_precedes(cj, mj, ci, mi)
        got = tuple(int(x) for x in ln.split())
        assert got[0] == int(pre) and got[2] == 1, (cj, mj, ci, mi, got)
        if pre:                                             # the threshold is defined for a pair that precedes
            assert got[1] == int(cj >= 2 * ci - 1), (cj, mj, ci, mi, got)
    f = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert f[0] == "C" and [int(x) for x in f[1:]] == [DIRECTIONAL, ANY, 64, 2 ** 32 - 1, 1, 2]


def test_collapse_rule_on_the_host():
    _check_tables(_build("tally_collapse_host_driver", []))


def test_collapse_rule_under_sanitizers():
    _check_tables(_build("tally_collapse_host_driver_asan", SAN), SAN_ENV)


# ---- the entries on the real library, without a GPU ----
COLLAPSE_SYMBOLS = ("seeqdevScanTallyCollapse", "seeqdevScanTallyParentsDevice", "seeqdevScanTallyCollapseDevice", "seeqdevScanCopyTallyParents",
                    "seeqdevScanCopyTallyCollapse", "seeqdevScanLastTallyCollapseMs")
ROW_FIELDS = [("nroots", 0), ("nabsorbed", 4), ("absorbed_reads", 8)]
COUNT_FIELDS = [("npairs", 0), ("ngroups", 8), ("nroots", 16), ("nabsorbed", 24), ("absorbed_reads", 32), ("rule", 40), ("max_len", 44)]


def test_collapse_symbols_exported(capi):
    L = capi.lib()
    hdr = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    for name in COLLAPSE_SYMBOLS:
        assert name in capi.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    for name, value in (("SEEQDEV_COLLAPSE_DIRECTIONAL", 0), ("SEEQDEV_COLLAPSE_ANY", 1)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == getattr(capi, name) == value


def test_collapse_layouts(capi):
    from seeq_amd import device as dev
    offs = lambda t: [(n, getattr(t, n).offset) for n, _ in t._fields_]      # noqa: E731
    assert C.sizeof(capi.seeqdev_tally_collapse_t) == 16 and offs(capi.seeqdev_tally_collapse_t) == ROW_FIELDS
    assert C.sizeof(capi.seeqdev_tally_collapse_counts_t) == 48 and offs(capi.seeqdev_tally_collapse_counts_t) == COUNT_FIELDS
    hdr = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    for t in ("seeqdev_tally_collapse_t", "seeqdev_tally_collapse_counts_t"):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % t, hdr).group(1)
        names = [n for decl in re.findall(r"^\s*uint\d+_t\s+([^;]+);", body, re.M) for n in re.split(r"\s*,\s*", decl)]
        assert names == [n for n, _ in getattr(capi, t)._fields_], t
    assert dev.TALLY_COLLAPSE_DTYPE.names == ("nroots", "nabsorbed", "absorbed_reads") and dev.TALLY_COLLAPSE_DTYPE.itemsize == 16
    assert [dev.TALLY_COLLAPSE_DTYPE.fields[n][1] for n in dev.TALLY_COLLAPSE_DTYPE.names] == [0, 4, 8]


def _einval(call):
    C.set_errno(0)
    assert call() == -1
    assert C.get_errno() == errno.EINVAL


def test_collapse_refusals_without_a_device(capi):
    # Every refusal comes before the device is touched: the stand-in context is all zeros -- no completed grouped call.
    L = capi.lib()
    ctx = C.addressof(C.create_string_buffer(8192))
    cnt = capi.seeqdev_tally_collapse_counts_t()
    _einval(lambda: L.seeqdevScanTallyCollapse(None, DIRECTIONAL, C.byref(cnt)))       # NULL scan
    _einval(lambda: L.seeqdevScanTallyCollapse(ctx, DIRECTIONAL, None))                # NULL counts
    for rule in (-1, 2, 255):
        _einval(lambda: L.seeqdevScanTallyCollapse(ctx, rule, C.byref(cnt)))           # an unknown rule
    for rule in RULES:
        _einval(lambda: L.seeqdevScanTallyCollapse(ctx, rule, C.byref(cnt)))           # no grouped call
        assert "grouped call" in capi.error_text() and "seeqdevScanTallyGrouped" in capi.error_text()
    # the copy entries: a context without a result has no entry
    for copy, out in ((L.seeqdevScanCopyTallyParents, (C.c_uint32 * 2)()), (L.seeqdevScanCopyTallyCollapse, (capi.seeqdev_tally_collapse_t * 2)())):
        _einval(lambda: copy(None, None, 0, 0))
        _einval(lambda: copy(ctx, None, 0, 1))
        _einval(lambda: copy(ctx, out, 0, 1))
        _einval(lambda: copy(ctx, out, 1, 0))
        assert copy(ctx, out, 0, 0) == 0 and copy(ctx, None, 0, 0) == 0
    for ptr in (L.seeqdevScanTallyParentsDevice, L.seeqdevScanTallyCollapseDevice):
        assert ptr(None) is None and ptr(ctx) is None
    ms = C.c_float(1.0)
    _einval(lambda: L.seeqdevScanLastTallyCollapseMs(ctx, None))
    _einval(lambda: L.seeqdevScanLastTallyCollapseMs(None, C.byref(ms)))
    assert L.seeqdevScanLastTallyCollapseMs(ctx, C.byref(ms)) == 0 and ms.value == 0.0


def test_collapse_fold_follows_the_parents_to_the_roots():
    from seeq_amd import device as dev
    table = lambda counts: np.array([(1, 10 + i, c) for i, c in enumerate(counts)], dtype=dev.TALLY_PAIR_DTYPE)      # noqa: E731
    # a chain of three (2 -> 1 -> 0), a self-parent, a pair absorbed directly
    root, folded = dev.collapse_fold(table([100, 10, 1, 7, 2]), np.array([0, 0, 1, 3, 3], dtype=np.uint32))
    assert root.dtype == np.uint32 and folded.dtype == np.uint64
    assert root.tolist() == [0, 0, 0, 3, 3] and folded.tolist() == [111, 0, 0, 9, 0]
    # a chain as long as the table, in either direction
    n = 1000
    root, folded = dev.collapse_fold(table([1] * n), np.maximum(np.arange(n) - 1, 0))
    assert root.tolist() == [0] * n and folded.tolist() == [n] + [0] * (n - 1)
    root, folded = dev.collapse_fold(table([2] * n), np.minimum(np.arange(n) + 1, n - 1))
    assert root.tolist() == [n - 1] * n and int(folded[-1]) == 2 * n and not folded[:-1].any()
    # sums beyond 2^32; every pair its own root; the empty table
    root, folded = dev.collapse_fold(table([2 ** 40, 2 ** 40, 5]), [0, 0, 2])
    assert folded.tolist() == [2 ** 41, 0, 5]
    root, folded = dev.collapse_fold(table([3, 4]), np.arange(2, dtype=np.uint32))
    assert root.tolist() == [0, 1] and folded.tolist() == [3, 4]
    root, folded = dev.collapse_fold(table([]), np.zeros(0, dtype=np.uint32))
    assert len(root) == 0 and len(folded) == 0 and root.dtype == np.uint32 and folded.dtype == np.uint64
    for bad in ([0, 5, 1], [0, 1], [0, -1, 1], [1, 0, 2]):      # out of range; another length; negative; a cycle
        with pytest.raises(ValueError):
            dev.collapse_fold(table([1, 1, 1]), np.array(bad, dtype=np.int64))
    # the rule's forest, folded: the family sizes of the hand-made cases
    pairs, _ = py_table(hand_items(big=False))
    parent, rows = py_collapse(pairs, ANY)
    root, folded = dev.collapse_fold(np.array(pairs, dtype=dev.TALLY_PAIR_DTYPE), np.array(parent, dtype=np.uint32))
    assert int(folded.sum()) == sum(c for *_, c in pairs) and int((folded > 0).sum()) == sum(r[0] for r in rows)
    top = [m for _, m, _ in pairs].index(py_key(b"ACGTTGCAAGCT")[1])
    assert int(folded[top]) == 111 and root[:3].tolist() == [top] * 3    # the chain 100 - 10 - 1 is one family
