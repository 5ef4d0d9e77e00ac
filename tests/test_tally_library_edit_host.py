"""CPU: the one-edit mode of the library rule of seeq_amd/csrc/seeq_tally_library.h -- a key's deletion and insertion neighbours, the
assignment under SEEQ_TLIB_MODE_EDIT -- compiled for the host by plain g++ (tests/tally_library_edit_host_driver.cpp) and compared with a
restatement in Python that knows NO neighbours: a Levenshtein dynamic program over the decoded strings against every entry.  With D the
entries at distance 1 of a span that is no entry: |D| == 1 is corrected, by the class len(entry) - len(span) (0 substituted, +1 inserted,
-1 deleted); |D| >= 2 ambiguous; else unknown.  Once more as a stand-alone program under -fsanitize=address,undefined.  Then the two new
entries on the real library: exports, the 32-byte layout, every refusal (which comes before any device call and so fails the same way
without a GPU).

The dynamic program is the plain one, cut off at 2 (Ukkonen): only the cells with |i - j| <= 1 are computed, every other cell and
every value above 2 counts as 2 -- exact for min(distance, 2), since a cell off that band is at least 2.  It runs over all entries of a
length at once (numpy), and is itself checked against the full, uncut program on random pairs."""
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
from test_tally_host import LONG, OK, py_key
from test_tally_library_host import (AMBIGUOUS, BAD_LIBRARIES, CORRECTED, CSRC, BUILD, E_NOKEY, EXACT, LIB_MAX, SAN, SAN_ENV, UNKNOWN, PyLibrary, _fails, _norm,
                                     _rand, _sub)

SRC = os.path.join(ROOT, "tests", "tally_library_edit_host_driver.cpp")
MODE_EXACT, MODE_SUBST, MODE_EDIT = 0, 1, 2
BY = {0: 0, 1: +1, 2: -1}                                   # the driver's class of a neighbour -> len(entry) - len(span)
EDIT_KEYS = {0: "nsubstituted", +1: "ninserted", -1: "ndeleted"}


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("seeq_tally_library.h", "seeq_tally.h", "seeq_strand.h", "seeq_tiles.h")]
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
def levenshtein(a, b):
    """The full dynamic program, nothing cut off."""
    row = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        new = [i]
        for j in range(1, len(b) + 1):
            new.append(min(row[j - 1] + (a[i - 1] != b[j - 1]), row[j] + 1, new[j - 1] + 1))
        row = new
    return row[len(b)]


def capped_distances(rows, q):
    """min(Levenshtein(row, q), 2) for every row of rows (uint8[n, Le]) against q (uint8[Lq])."""
    n, le = rows.shape
    lq = len(q)
    two = np.full(n, 2, dtype=np.uint8)
    if abs(le - lq) >= 2:
        return two
    prev = {j: np.full(n, j, dtype=np.uint8) for j in range(min(lq, 1) + 1)}      # row 0: D[0][j] = j
    for i in range(1, le + 1):
        cur = {}
        for j in range(max(0, i - 1), min(lq, i + 1) + 1):
            if j == 0:
                v = np.full(n, min(i, 2), dtype=np.uint8)
            else:
                v = np.minimum(np.minimum(prev.get(j - 1, two) + (rows[:, i - 1] != q[j - 1]), prev.get(j, two) + 1), cur.get(j - 1, two) + 1)
            cur[j] = np.minimum(v, 2)
        prev = cur
    return prev[lq]


class PyEditLibrary(PyLibrary):
    """PyLibrary with the one-edit assignment: the distance of a span to EVERY entry, whatever its length."""

    def assign_edit(self, seq):
        """(id, kind, len(entry) - len(seq) of a corrected span, else None) of a sequence that has a key."""
        seq = _norm(seq)
        q = np.frombuffer(seq, dtype=np.uint8)
        near = []
        for n, (rows, ids) in self.by_len.items():
            dist = capped_distances(rows, q)
            if n == len(seq) and (dist == 0).any():
                assert (dist == 0).sum() == 1
                return int(ids[dist == 0][0]), EXACT, None
            near += [(int(i), n - len(seq)) for i in ids[dist == 1]]
        if len(near) == 1:
            return near[0][0], CORRECTED, near[0][1]
        return 0, AMBIGUOUS if len(near) >= 2 else UNKNOWN, None

    def tally_edit(self, spans):
        """spans: list of bytes -> (counts as PyLibrary.tally, dense count list, the id of every span, the split of ncorrected)."""
        cnt = dict(nspans=len(spans), nassigned=0, nexact=0, ncorrected=0, nambiguous=0, nunknown=0, nlong=0, nforeign=0)
        edits = dict(nsubstituted=0, ninserted=0, ndeleted=0)
        dense, ids = [0] * len(self), []
        memo = {}
        for s in spans:
            kind = py_key(s)[0]
            if kind != OK:
                cnt["nlong" if kind == LONG else "nforeign"] += 1
                ids.append(0)
                continue
            if s not in memo:
                memo[s] = self.assign_edit(s)
            i, what, by = memo[s]
            cnt[("nexact", "ncorrected", "nambiguous", "nunknown")[what]] += 1
            if what == CORRECTED:
                edits[EDIT_KEYS[by]] += 1
            ids.append(i)
            if i:
                dense[i - 1] += 1
        cnt["nassigned"] = cnt["nexact"] + cnt["ncorrected"]
        cnt["ndistinct"] = sum(1 for c in dense if c)
        return cnt, dense, ids, edits


def _del(s, at):
    return s[:at] + s[at + 1:]


def _ins(s, at, c):
    return s[:at] + bytes([c]) + s[at:]


def test_the_restatement_itself():
    rng = random.Random(3)
    for _ in range(400):                                    # the cut-off program against the full one
        a = _rand(rng, rng.choice((0, 1, 2, 3, 5, 8, 12)))
        r = rng.random()
        b = a if r < 0.1 else _rand(rng, rng.choice((0, 1, 2, 4, 8, 13))) if r < 0.3 else a
        for _ in range(rng.randrange(0, 4) if r >= 0.3 else 0):
            k = rng.randrange(3)
            at = rng.randrange(len(b) + 1)
            b = _ins(b, at, rng.choice(b"ACGT")) if k == 0 or not b else _del(b, at % len(b)) if k == 1 else _sub(b, at % len(b), rng.randrange(1, 4))
        rows = np.frombuffer(a, dtype=np.uint8).reshape(1, len(a))
        assert capped_distances(rows, np.frombuffer(b, dtype=np.uint8))[0] == min(levenshtein(a, b), 2), (a, b)
    assert levenshtein(b"ACGT", b"AGT") == 1 and levenshtein(b"", b"AC") == 2 and levenshtein(b"AAAA", b"AAA") == 1 and levenshtein(b"ACGT", b"TGCA") == 4
    lib = PyEditLibrary([b"ACGT", b"ACGA", b"TTTT", b"", b"GG", b"A" * 12, b"CATCAT", b"CATGCAT"])
    assert lib.assign_edit(b"ACGT") == (1, EXACT, None) and lib.assign_edit(b"acgu") == (1, EXACT, None)
    assert lib.assign_edit(b"ACGC")[1] == AMBIGUOUS and lib.assign_edit(b"ACG")[1] == AMBIGUOUS             # ACGT and ACGA, by substitution, by insertion
    assert lib.assign_edit(b"TTT") == (3, CORRECTED, +1) and lib.assign_edit(b"TTTTT") == (3, CORRECTED, -1) and lib.assign_edit(b"TTTA") == (3, CORRECTED, 0)
    assert lib.assign_edit(b"A" * 11) == (6, CORRECTED, +1) and lib.assign_edit(b"A" * 13) == (6, CORRECTED, -1)      # a homopolymer: one entry, found once
    assert lib.assign_edit(b"G") == (0, AMBIGUOUS, None)                                                     # "" by deletion and GG by insertion
    assert lib.assign_edit(b"C") == (4, CORRECTED, -1) and lib.assign_edit(b"TTAA")[1] == UNKNOWN
    assert lib.assign_edit(b"CATGAT") == (0, AMBIGUOUS, None)                                                # CATCAT by substitution, CATGCAT by insertion
    cnt, dense, ids, edits = lib.tally_edit([b"ACGT", b"TTT", b"TTTTT", b"TTTA", b"G", b"CCCCCC", b"N", b"A" * 32, b""])
    assert cnt == dict(nspans=9, nassigned=5, nexact=2, ncorrected=3, nambiguous=1, nunknown=1, nlong=1, nforeign=1, ndistinct=3)
    assert edits == dict(nsubstituted=1, ninserted=1, ndeleted=1) and ids == [1, 3, 3, 3, 0, 0, 0, 0, 4] and dense == [1, 0, 3, 1, 0, 0, 0, 0]


# ---- neighbours ----
def _runs(s):
    return sum(1 for i in range(len(s)) if i == 0 or s[i] != s[i - 1])


def _neighbour_keys():
    rng = random.Random(5)
    return [b"", b"A", b"A" * 31, b"G" * 30, b"AC" * 15, b"GT" * 15] + [_rand(rng, n) for n in (1, 2, 8, 12, 20, 30, 31) for _ in range(4)]


def _check_neighbours(exe, env=None):
    seqs = _neighbour_keys()
    lines = _run(exe, "neigh", "".join("K %x\n" % py_key(s)[1] for s in seqs), env)
    assert len(lines) >= 2 * len(seqs)
    for k, s in enumerate(seqs):
        dl, il = lines[2 * k].split(), lines[2 * k + 1].split()
        assert dl[0] == "D" and il[0] == "I"
        dels, inss = [int(x, 16) for x in dl[1:]], [int(x, 16) for x in il[1:]]
        n = len(s)
        # as a list: no repeats, one per run; as a set: all n one-base deletions
        assert len(dels) == len(set(dels)) == _runs(s) and set(dels) == {py_key(_del(s, at))[1] for at in range(n)}, s
        assert all(k.bit_length() == 2 * (n - 1) + 1 for k in dels)
        if n == 31:
            assert inss == []                               # a key of 32 bases does not exist
        else:
            assert len(inss) == len(set(inss)) == 3 * n + 4 and set(inss) == {py_key(_ins(s, at, c))[1] for at in range(n + 1) for c in b"ACGT"}, s
            assert all(k.bit_length() == 2 * (n + 1) + 1 for k in inss)
    return len(seqs)


def test_neighbours_on_the_host():
    exe = _build("tally_library_edit_host_driver", [])
    assert _check_neighbours(exe) >= 30
    f = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert f[0] == "B" and [int(x) for x in f[1:]] == [MODE_EXACT, MODE_SUBST, MODE_EDIT, 0, 1, 2, 30, 8]


# ---- libraries and queries ----
RUNS = b"ACCGGGTAAAATCGGATTCA"                               # an entry with runs of 2, 3 and 4 bases


def _make_library(n, seed):
    """n entries of lengths 0, 1, 8, 12, 20, 30 and 31 mixed, in shuffled order -> (sequences, what was planted).  Planted (where n
    allows): `both` an entry and its own one-base deletion; `homo` A x 12; `cross` (x, y, q) with q one substitution from x and one
    deletion from y; `twodel` (u, v, q) both deletions of q; RUNS."""
    rng = random.Random(seed)
    if n == 1:
        return [b"ACGTTGCAAGCT"], {}
    e = _rand(rng, 20)
    both = (e, _del(e, 7))
    if n == 2:
        return list(both), dict(both=both)
    q = _rand(rng, 12)
    cross = (_sub(q, 3, 1), _ins(q, 8, b"ACGT"[(b"ACGT".index(q[8]) + 1) % 4]), q)
    while True:
        q2 = _rand(rng, 20)
        if _del(q2, 4) != _del(q2, 15):
            break
    twodel = (_del(q2, 4), _del(q2, 15), q2)
    homo = b"A" * 12
    seqs = {b"", b"A", b"C", homo, RUNS} | set(both) | set(cross[:2]) | set(twodel[:2])
    assert len(seqs) == 11
    while len(seqs) < n:
        s = _rand(rng, rng.choice((8, 12, 20, 30, 31)))
        if s not in (q, q2, b"A" * 11, b"A" * 13):
            seqs.add(s)
    seqs = sorted(seqs)
    rng.shuffle(seqs)
    return seqs, dict(both=both, homo=homo, cross=cross, twodel=twodel)


def _make_queries(seqs, planted, seed, sample=40):
    rng = random.Random(seed)
    some = rng.sample(seqs, min(sample, len(seqs)))
    some += [s for s in seqs if len(s) == 30][:3] + [s for s in seqs if len(s) == 31][:3] + [s for s in (RUNS, planted.get("homo")) if s in seqs]
    q = list(seqs)                                          # every entry exactly
    for s in some:
        ats = sorted({0, len(s) // 2, len(s) - 1}) if s else []
        q += [_del(s, at) for at in ats]                    # one base lost: at the first, a middle, the last position
        if len(s) < 31:
            q += [_ins(s, at, rng.choice(b"ACGT")) for at in ats + [len(s)]]      # one base gained, up to behind the last
        else:
            q.append(_ins(s, 5, 65))                        # a 31-base entry that gained a base: long
        q += [_sub(s, at, rng.randrange(1, 4)) for at in ats]
        if len(s) >= 8:                                     # two edits
            i, j = sorted(rng.sample(range(len(s)), 2))
            q += [_del(_del(s, j), i), _sub(_del(s, j), i, 1), _ins(_sub(s, i, 2), j, rng.choice(b"ACGT"))]
            if len(s) <= 29:
                q.append(_ins(_ins(s, j, rng.choice(b"ACGT")), i, rng.choice(b"ACGT")))
    if RUNS in seqs:                                        # inside and at the edge of a run: ACC GGG T AAAA T ...
        q += [_del(RUNS, at) for at in (3, 4, 5, 7, 8, 10)] + [_ins(RUNS, at, c) for at, c in ((3, 71), (4, 71), (6, 71), (7, 65), (9, 65), (11, 65), (7, 84))]
    if "homo" in planted:
        q += [b"A" * 11, b"A" * 13, b"A" * 10, b"A" * 14]
    for key in ("cross", "twodel"):
        if key in planted:
            q.append(planted[key][2])
    q += [b"", b"T", b"G", b"GT", b"AC"]
    return [s for s in q if py_key(s)[0] == OK]             # (the driver takes keys: a span of 32 bases has none)


SIZES = (1, 2, 257, 70000)


@functools.lru_cache(maxsize=None)
def _case(n):
    """(library, queries, planted, per mode the expected (id, kind, by) of every query) -- computed once."""
    seqs, planted = _make_library(n, 3000 + n)
    lib = PyEditLibrary(seqs)
    queries = _make_queries(seqs, planted, 4000 + n)
    exp = {}
    # an entry is at distance 0 from itself: its id, exact -- the first n queries; the brute force checks a sample of them, and every other query
    head = [(i + 1, EXACT, None) for i in range(n)]
    for i in random.Random(n).sample(range(n), min(n, 50)):
        assert lib.assign_edit(queries[i]) == head[i]
    exp[MODE_EDIT] = head + [lib.assign_edit(s) for s in queries[n:]]
    for mm in (MODE_SUBST, MODE_EXACT):
        exp[mm] = head + [a + ((0 if a[1] == CORRECTED else None),) for a in (lib.assign(s, mm) for s in queries[n:])]
    by = dict(zip(queries, exp[MODE_EDIT]))
    ident = {s: i + 1 for i, s in enumerate(lib.seqs)}
    # before the code under test runs: the input holds what it is meant to hold
    assert {(k, d) for _, k, d in exp[MODE_EDIT]} >= {(EXACT, None), (CORRECTED, 0), (CORRECTED, +1), (CORRECTED, -1), (UNKNOWN, None)}
    if "both" in planted:
        x, y = planted["both"]
        assert by[x] == (ident[x], EXACT, None) and by[y] == (ident[y], EXACT, None) and levenshtein(x, y) == 1
    if "homo" in planted:
        h = ident[planted["homo"]]
        assert by[b"A" * 11] == (h, CORRECTED, +1) and by[b"A" * 13] == (h, CORRECTED, -1) and by[b"A" * 10][1] == by[b"A" * 14][1] == UNKNOWN
        x, y, q = planted["cross"]
        assert by[q] == (0, AMBIGUOUS, None) and levenshtein(x, q) == levenshtein(y, q) == 1 and len(x) == len(q) == len(y) - 1
        u, v, q2 = planted["twodel"]
        assert by[q2] == (0, AMBIGUOUS, None) and len(u) == len(v) == len(q2) - 1 and u != v
        kinds = {(k, d) for _, k, d in exp[MODE_EDIT]}
        assert kinds == {(EXACT, None), (CORRECTED, 0), (CORRECTED, +1), (CORRECTED, -1), (AMBIGUOUS, None), (UNKNOWN, None)}
        assert any(len(s) == 30 and len(lib.seqs[i - 1]) == 31 for s, (i, k, d) in by.items() if k == CORRECTED)      # a 31-base entry that lost a base
        assert any(len(s) == 31 and d == -1 for s, (i, k, d) in by.items() if k == CORRECTED)                          # a span of 31: a deletion only
        assert sum(1 for s, (i, k, d) in by.items() if k == UNKNOWN and len(s) >= 8) >= 20                             # two edits
    return lib, queries, planted, exp


def _assign_input(lib, queries, mode):
    return "L %d %d\n%s\nQ %d\n%s\n" % (len(lib), mode, " ".join("%x" % k for k in lib.keys()), len(queries), " ".join("%x" % py_key(s)[1] for s in queries))


def _check_assign(exe, n, env=None):
    lib, queries, planted, exp = _case(n)
    for mode in (MODE_EDIT, MODE_SUBST, MODE_EXACT):
        lines = _run(exe, "assign", _assign_input(lib, queries, mode), env)
        got = [tuple(int(x) for x in ln.split()) for ln in lines[:len(queries)]]
        assert lines[len(queries):] in ([], [""]) and len(got) == len(queries)
        got = [(i, k, BY[b] if b >= 0 else None) for i, k, b in got]
        bad = [(queries[i], g, exp[mode][i]) for i, g in enumerate(got) if g != exp[mode][i]]
        assert not bad, (n, mode, len(bad), bad[:5])
    # across the modes, on the same queries
    for e2, e1, e0 in zip(exp[MODE_EDIT], exp[MODE_SUBST], exp[MODE_EXACT]):
        assert (e2[1] == EXACT) == (e1[1] == EXACT) == (e0[1] == EXACT) and (e2 == e1 == e0 or e2[1] != EXACT)      # exact stays exact
        if e1[1] == CORRECTED:
            assert e2 == e1 or e2[:2] == (0, AMBIGUOUS)     # the same id, by a substitution -- or one more entry one indel away
        if e1[1] == AMBIGUOUS:
            assert e2[:2] == (0, AMBIGUOUS)


@pytest.mark.parametrize("n", SIZES)
def test_assignment_on_the_host(n):
    _check_assign(_build("tally_library_edit_host_driver", []), n)


def test_edit_rule_under_sanitizers():
    exe = _build("tally_library_edit_host_driver_asan", SAN)
    for n in SIZES:
        _check_assign(exe, n, SAN_ENV)
    _check_neighbours(exe, SAN_ENV)


# ---- the entries on the real library, without a GPU ----
EDIT_SYMBOLS = ("seeqdevScanSetLibraryMode", "seeqdevScanLastLibraryEdits")
FIELDS = [("nsubstituted", 0), ("ninserted", 8), ("ndeleted", 16), ("reserved", 24)]


def test_edit_symbols_exported(capi):
    L = capi.lib()
    hdr = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    for name in EDIT_SYMBOLS:
        assert name in capi.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name
    for name, value in (("SEEQDEV_LIBRARY_EXACT", 0), ("SEEQDEV_LIBRARY_SUBST", 1), ("SEEQDEV_LIBRARY_EDIT", 2)):
        assert getattr(capi, name) == value and re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name


def test_library_edits_layout(capi):
    t = capi.seeqdev_tally_library_edits_t
    assert C.sizeof(t) == 32 and [(n, getattr(t, n).offset) for n, _ in t._fields_] == FIELDS
    hdr = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} seeqdev_tally_library_edits_t;", hdr).group(1)
    names = [n for decl in re.findall(r"^\s*uint64_t\s+([^;]+);", body, re.M) for n in re.split(r"\s*,\s*", decl)]
    assert names == [n for n, _ in FIELDS]
    assert C.sizeof(capi.seeqdev_tally_library_counts_t) == 80      # and the counts stay what they were


def test_set_library_mode_refusals_without_a_device(capi):
    # Every refusal comes before the device is touched: the stand-in context is all zeros.
    L = capi.lib()
    ctx = C.addressof(C.create_string_buffer(8192))
    arr = lambda ks: (C.c_uint64 * len(ks))(*ks)            # noqa: E731
    good = arr([py_key(b"ACGT")[1], py_key(b"ACGA")[1], 1])
    for mode in (0, 1, 2):
        _fails(lambda: L.seeqdevScanSetLibraryMode(None, good, 3, mode), errno.EINVAL)          # NULL scan
        _fails(lambda: L.seeqdevScanSetLibraryMode(ctx, None, 3, mode), errno.EINVAL)           # NULL keys with n > 0
        for keys, code, at in BAD_LIBRARIES:
            _fails(lambda: L.seeqdevScanSetLibraryMode(ctx, arr(keys), len(keys), mode), errno.EINVAL)
            assert ("entry %d " % at) in capi.error_text() and ("no tally key" if code == E_NOKEY else "repeats") in capi.error_text()
        for n in (LIB_MAX + 1, 2 ** 32, 2 ** 40):
            _fails(lambda: L.seeqdevScanSetLibraryMode(ctx, good, n, mode), errno.E2BIG)        # (decided before a key is read)
        assert L.seeqdevScanSetLibraryMode(ctx, None, 0, mode) == 0 and L.seeqdevScanSetLibraryMode(ctx, good, 0, mode) == 0
    for mode in (3, -1, 255):
        _fails(lambda: L.seeqdevScanSetLibraryMode(ctx, good, 3, mode), errno.EINVAL)           # no mode
        _fails(lambda: L.seeqdevScanSetLibraryMode(ctx, None, 0, mode), errno.EINVAL)
        _fails(lambda: L.seeqdevScanSetLibraryMode(ctx, C.c_void_p(8), 2 ** 40, mode), errno.EINVAL)      # (before anything is read)
    _fails(lambda: L.seeqdevScanSetLibrary(ctx, good, 3, 2), errno.EINVAL)                      # the old entry keeps refusing 2
    assert L.seeqdevScanSetLibraryMode(ctx, None, 0, 2) == 0


def test_last_library_edits_without_a_device(capi):
    L = capi.lib()
    ctx = C.addressof(C.create_string_buffer(8192))
    e = capi.seeqdev_tally_library_edits_t(7, 7, 7, 7)
    _fails(lambda: L.seeqdevScanLastLibraryEdits(None, C.byref(e)), errno.EINVAL)
    _fails(lambda: L.seeqdevScanLastLibraryEdits(ctx, None), errno.EINVAL)
    assert (e.nsubstituted, e.ninserted, e.ndeleted, e.reserved) == (7, 7, 7, 7)
    assert L.seeqdevScanLastLibraryEdits(ctx, C.byref(e)) == 0                                   # before any assignment: zero
    assert (e.nsubstituted, e.ninserted, e.ndeleted, e.reserved) == (0, 0, 0, 0)
    assert L.seeqdevScanSetLibraryMode(ctx, None, 0, 2) == 0 and L.seeqdevScanLastLibraryEdits(ctx, C.byref(e)) == 0
    assert (e.nsubstituted, e.ninserted, e.ndeleted, e.reserved) == (0, 0, 0, 0)


def test_indels_want_one_mismatch():
    from seeq_amd import device as dev
    with pytest.raises(ValueError):
        dev.Scanner.set_library(object(), [b"ACGT"], max_mismatch=0, indels=True)               # (refused before the Scanner is looked at)
    with pytest.raises(ValueError):
        dev.Scanner.set_library(object(), [b"ACGT"], max_mismatch=2, indels=True)
