"""CPU: the library rule of seeq_amd/csrc/seeq_tally_library.h -- a key's neighbours, the lower bound, the assignment (exact, corrected,
ambiguous, unknown), the host-side sort and validation of a library -- compiled for the host by plain g++
(tests/tally_library_host_driver.cpp) and compared with a restatement in Python that knows NO neighbours: a brute-force Hamming distance
over the decoded strings of equal length.  Once more as a stand-alone program under -fsanitize=address,undefined.  Then the entries on the
real library: exports, the struct's layout, every refusal of the set call and of the two tally entries (which come before any device
call and so fail the same way without a GPU), and library_counts."""
import bisect
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
from test_tally_host import FOREIGN, LONG, OK, py_decode, py_key

CSRC = os.path.join(ROOT, "seeq_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "build")
SRC = os.path.join(ROOT, "tests", "tally_library_host_driver.cpp")
EXACT, CORRECTED, AMBIGUOUS, UNKNOWN = 0, 1, 2, 3
E_NOKEY, E_DUP = 1, 2
LIB_MAX = 2 ** 24 - 1
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


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
def _norm(seq):
    return bytes(seq).upper().replace(b"U", b"T")


class PyLibrary:
    """A library of sequences (bytes, pairwise distinct once upper-cased with U read as T); entry i has the id i + 1."""

    def __init__(self, seqs):
        self.seqs = [_norm(s) for s in seqs]
        assert len(set(self.seqs)) == len(self.seqs) and all(py_key(s)[0] == OK for s in self.seqs)
        by = {}
        for i, s in enumerate(self.seqs):
            by.setdefault(len(s), []).append(i)
        self.by_len = {n: (np.frombuffer(b"".join(self.seqs[i] for i in idx), dtype=np.uint8).reshape(len(idx), n), np.array(idx) + 1)
                       for n, idx in by.items()}

    def __len__(self):
        return len(self.seqs)

    def keys(self):
        return [py_key(s)[1] for s in self.seqs]

    def assign(self, seq, max_mismatch):
        """(id, kind) of a sequence that has a key: the Hamming distance to every entry of its length."""
        seq = _norm(seq)
        if len(seq) not in self.by_len:
            return 0, UNKNOWN
        rows, ids = self.by_len[len(seq)]
        dist = (rows != np.frombuffer(seq, dtype=np.uint8)).sum(axis=1)
        exact = ids[dist == 0]
        if len(exact):
            assert len(exact) == 1
            return int(exact[0]), EXACT
        near = ids[dist == 1] if max_mismatch >= 1 else ids[:0]
        if len(near) == 1:
            return int(near[0]), CORRECTED
        return 0, AMBIGUOUS if len(near) >= 2 else UNKNOWN

    def tally(self, spans, max_mismatch):
        """spans: list of bytes -> (counts dict as seeqdev_tally_library_counts_t without key_bits / passes, dense count list, the id of
        every span): long before foreign, both before the library."""
        cnt = dict(nspans=len(spans), nassigned=0, nexact=0, ncorrected=0, nambiguous=0, nunknown=0, nlong=0, nforeign=0)
        dense, ids = [0] * len(self), []
        memo = {}
        for s in spans:
            kind = py_key(s)[0]
            if kind != OK:
                cnt["nlong" if kind == LONG else "nforeign"] += 1
                ids.append(0)
                continue
            if s not in memo:
                memo[s] = self.assign(s, max_mismatch)
            i, what = memo[s]
            cnt[("nexact", "ncorrected", "nambiguous", "nunknown")[what]] += 1
            ids.append(i)
            if i:
                dense[i - 1] += 1
        cnt["nassigned"] = cnt["nexact"] + cnt["ncorrected"]
        cnt["ndistinct"] = sum(1 for c in dense if c)
        return cnt, dense, ids


def bitlen_passes(n, nassigned=1):
    return n.bit_length(), (n.bit_length() + 7) // 8 if nassigned else 0


def _sub(seq, at, other):
    """seq with the base at `at` replaced by the other-th different base (other in 1 .. 3)."""
    return seq[:at] + bytes([b"ACGT"[(b"ACGT".index(seq[at]) + other) % 4]]) + seq[at + 1:]


def _rand(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _valid_below(key):
    """The largest key below `key`, None when there is none."""
    if key <= 1:
        return None
    n = (key.bit_length() - 1) // 2
    return key - 1 if key > 1 << (2 * n) else (2 << (2 * (n - 1))) - 1


def _valid_above(key):
    if key >= 2 ** 63 - 1:
        return None
    n = (key.bit_length() - 1) // 2
    return key + 1 if key + 1 < 2 << (2 * n) else 1 << (2 * (n + 1))


# ---- libraries and queries ----
def _make_library(n, seed):
    """n entries of lengths 0, 1, 8, 12, 20 and 31 mixed, in shuffled order; planted in it (where n allows): a pair at distance 1
    and a pair at distance 2, of 12 and of 20 bases.  -> (sequences, pairs at distance 1, pairs at distance 2)"""
    rng = random.Random(seed)
    if n == 1:
        return [b"ACGTTGCAAGCT"], [], []
    a = _rand(rng, 12)
    if n == 2:
        return [a, _sub(a, 5, 2)], [(a, _sub(a, 5, 2))], []
    b, c, d = _rand(rng, 20), _rand(rng, 12), _rand(rng, 20)
    d1 = [(a, _sub(a, 5, 2)), (b, _sub(b, 19, 1))]
    d2 = [(c, _sub(_sub(c, 0, 1), 11, 3)), (d, _sub(_sub(d, 7, 2), 8, 2))]
    seqs = {b"", b"A", b"C"} | {s for pair in d1 + d2 for s in pair}
    while len(seqs) < n:
        seqs.add(_rand(rng, rng.choice((8, 12, 20, 31))))
    seqs = sorted(seqs)
    rng.shuffle(seqs)
    return seqs, d1, d2


def _make_queries(seqs, d1, d2, seed, sample=40):
    rng = random.Random(seed)
    some = rng.sample(seqs, min(sample, len(seqs)))
    q = list(seqs)                                          # every entry exactly
    for s in some:                                          # every single substitution at the first, a middle and the last position
        for at in sorted({0, len(s) // 2, len(s) - 1} if s else ()):
            q += [_sub(s, at, o) for o in (1, 2, 3)]
    for s in some:
        if len(s) >= 8:                                     # two substitutions
            i, j = rng.sample(range(len(s)), 2)
            q.append(_sub(_sub(s, i, rng.randrange(1, 4)), j, rng.randrange(1, 4)))
        if len(s) < 31:                                     # one base longer, one base shorter
            q.append(s + bytes([rng.choice(b"ACGT")]))
        if s:
            q.append(s[:-1])
            q.append(s[1:])
    keys = sorted(py_key(s)[1] for s in seqs)
    edge = [k for k in (_valid_below(keys[0]), _valid_above(keys[-1]), 1, 2 ** 63 - 1, 1 << 62) if k is not None]
    q += [py_decode(k).encode() for k in edge]              # below the smallest and above the largest entry; the empty key
    for x, y in d1:                                         # either entry of a pair at distance 1: exact wins
        q += [x, y]
    for x, y in d1:                                         # ... and the third and fourth base there: two neighbours
        at = next(i for i in range(len(x)) if x[i] != y[i])
        q += [z for z in (_sub(x, at, o) for o in (1, 2, 3)) if z != y]
    for x, y in d2:                                         # the two common neighbours of a pair at distance 2
        i, j = [k for k in range(len(x)) if x[k] != y[k]]
        q += [x[:i] + y[i:i + 1] + x[i + 1:], x[:j] + y[j:j + 1] + x[j + 1:]]
    q += [b"", b"T", b"G"]
    return q


SIZES = (1, 2, 257, 70000)


@functools.lru_cache(maxsize=None)
def _case(n):
    """(library, queries, per max_mismatch the expected (id, kind) of every query, the expected lower bounds) -- computed once."""
    seqs, d1, d2 = _make_library(n, 1000 + n)
    lib = PyLibrary(seqs)
    queries = _make_queries(seqs, d1, d2, 2000 + n)
    exp = {}
    for mm in (1, 0):
        # an entry is at distance 0 from itself and, the entries being distinct, from no other: its id, exact -- the first n queries.
        # The brute force over all of them would take a minute for the largest library: it checks a sample of them, and every other query.
        head = [(i + 1, EXACT) for i in range(n)]
        for i in random.Random(n).sample(range(n), min(n, 300)):
            assert lib.assign(queries[i], mm) == head[i]
        exp[mm] = head + [lib.assign(s, mm) for s in queries[n:]]
    keys = sorted(lib.keys())
    lower = [bisect.bisect_left(keys, py_key(s)[1]) for s in queries]
    # what the planted pairs are for
    if d1:
        by = dict(zip(queries, exp[1]))
        for x, y in d1:
            assert by[x][1] == by[y][1] == EXACT and by[x][0] != by[y][0]
            at = next(i for i in range(len(x)) if x[i] != y[i])
            assert all(by[z] == (0, AMBIGUOUS) for z in (_sub(x, at, o) for o in (1, 2, 3)) if z != y)
        for x, y in d2:
            i, j = [k for k in range(len(x)) if x[k] != y[k]]
            assert by[x[:i] + y[i:i + 1] + x[i + 1:]] == by[x[:j] + y[j:j + 1] + x[j + 1:]] == (0, AMBIGUOUS)
    return lib, queries, exp, lower


def _assign_input(lib, queries, mm):
    return "L %d %d\n%s\nQ %d\n%s\n" % (len(lib), mm, " ".join("%x" % k for k in lib.keys()), len(queries), " ".join("%x" % py_key(s)[1] for s in queries))


def _check_assign(exe, n, env=None):
    lib, queries, exp, lower = _case(n)
    seen = set()
    for mm in (1, 0):
        lines = _run(exe, "assign", _assign_input(lib, queries, mm), env)
        bits, passes = bitlen_passes(n)
        assert lines[0] == "P %d %d %d" % (bits, bits + 1, passes), lines[0]
        got = [tuple(int(x) for x in ln.split()) for ln in lines[1:1 + len(queries)]]
        assert lines[1 + len(queries):] in ([], [""]) and len(got) == len(queries)
        bad = [(queries[i], g, exp[mm][i], lower[i]) for i, g in enumerate(got) if g != exp[mm][i] + (lower[i],)]
        assert not bad, (n, mm, len(bad), bad[:5])
        kinds = {k for _, k in exp[mm]}
        seen |= {(mm, k) for k in kinds}
        if mm == 0:
            assert kinds <= {EXACT, UNKNOWN} and all(i == 0 for i, k in exp[0] if k == UNKNOWN)
        # under max_mismatch 0 the corrected and the ambiguous become unknown, everything else stays
        assert all((b == a) if a[1] in (EXACT, UNKNOWN) else (b == (0, UNKNOWN)) for a, b in zip(exp[1], exp[0]))
    return seen


def test_the_restatement_itself():
    lib = PyLibrary([b"ACGT", b"ACGA", b"TTTT", b"", b"acgu"[:0] + b"GG", b"AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA"])
    assert lib.keys()[0] == py_key(b"ACGT")[1] and len(lib) == 6
    assert lib.assign(b"ACGT", 1) == (1, EXACT) and lib.assign(b"acgu", 1) == (1, EXACT)        # exact wins over the neighbour ACGA
    assert lib.assign(b"ACGC", 1) == (0, AMBIGUOUS) and lib.assign(b"ACGC", 0) == (0, UNKNOWN)  # the third base between ACGT and ACGA
    assert lib.assign(b"TTTA", 1) == (3, CORRECTED) and lib.assign(b"TTTA", 0) == (0, UNKNOWN)
    assert lib.assign(b"TTAA", 1) == (0, UNKNOWN)                                               # two substitutions
    assert lib.assign(b"TTT", 1) == (0, UNKNOWN) and lib.assign(b"TTTTT", 1) == (0, UNKNOWN)    # a deletion, an insertion: another length
    assert lib.assign(b"", 1) == (4, EXACT) and lib.assign(b"GC", 1) == (5, CORRECTED)
    assert PyLibrary([b"A"]).assign(b"", 1) == (0, UNKNOWN)                                     # the empty key has no neighbours
    cnt, dense, ids = lib.tally([b"ACGT", b"TTTA", b"ACGC", b"CCCC", b"N", b"A" * 32, b"N" * 40, b""], 1)
    assert cnt == dict(nspans=8, nassigned=3, nexact=2, ncorrected=1, nambiguous=1, nunknown=1, nlong=2, nforeign=1, ndistinct=3)
    assert dense == [1, 0, 1, 1, 0, 0] and ids == [1, 3, 0, 0, 0, 0, 0, 4]
    assert [_valid_below(k) for k in (1, 4, 5, 16)] == [None, 1, 4, 7] and [_valid_above(k) for k in (1, 7, 2 ** 63 - 1)] == [4, 16, None]


def test_neighbours_on_the_host():
    rng = random.Random(4)
    seqs = [b"", b"A", b"G" * 31, b"A" * 31] + [_rand(rng, n) for n in (1, 2, 8, 12, 20, 31) for _ in range(4)]
    lines = _run(_build("tally_library_host_driver", []), "neigh", "".join("K %x\n" % py_key(s)[1] for s in seqs))
    for s, ln in zip(seqs, lines):
        got = [] if ln == "-" else [int(x, 16) for x in ln.split()]
        exp = [py_key(_sub(s, at, o))[1] for at in range(len(s)) for o in (1, 2, 3)]
        assert len(got) == 3 * len(s) and sorted(got) == sorted(exp), s
        # position by position: the three of a position differ from the key in that base alone
        for at in range(len(s)):
            assert sorted(got[3 * at:3 * at + 3]) == sorted(exp[3 * at:3 * at + 3])
        assert all(k.bit_length() == 2 * len(s) + 1 for k in got)
    f = subprocess.run([_build("tally_library_host_driver", [])], capture_output=True, text=True, timeout=60).stdout.split()
    assert f[0] == "B" and [int(x) for x in f[1:]] == [LIB_MAX, 64, EXACT, CORRECTED, AMBIGUOUS, UNKNOWN, E_NOKEY, E_DUP, 3, 0, 2]


@pytest.mark.parametrize("n", SIZES)
def test_assignment_on_the_host(n):
    seen = _check_assign(_build("tally_library_host_driver", []), n)
    if n >= 257:
        assert seen == {(1, EXACT), (1, CORRECTED), (1, AMBIGUOUS), (1, UNKNOWN), (0, EXACT), (0, UNKNOWN)}


BAD_LIBRARIES = [([0], E_NOKEY, 0), ([5, 1 << 63], E_NOKEY, 1), ([5, 6, 2], E_NOKEY, 2), ([5, 0b1000, 5], E_NOKEY, 1),      # no key before a duplicate
                 ([5, 5], E_DUP, 1), ([7, 5, 6, 5, 7], E_DUP, 3), ([1, 4, 5, 6, 7, 16, 1], E_DUP, 6), ([2 ** 63 - 1] * 3, E_DUP, 1)]


def _bad_input():
    return "".join("L %d 1\n%s\nQ 1\n1\n" % (len(k), " ".join("%x" % x for x in k)) for k, _, _ in BAD_LIBRARIES)


def test_validation_of_a_library_on_the_host():
    lines = _run(_build("tally_library_host_driver", []), "assign", _bad_input())
    assert [ln for ln in lines if ln] == ["E %d %d" % (code, at) for _, code, at in BAD_LIBRARIES]


def test_library_rule_under_sanitizers():
    exe = _build("tally_library_host_driver_asan", SAN)
    for n in SIZES:
        _check_assign(exe, n, SAN_ENV)
    assert [ln for ln in _run(exe, "assign", _bad_input(), SAN_ENV) if ln] == ["E %d %d" % (code, at) for _, code, at in BAD_LIBRARIES]
    assert len(_run(exe, "neigh", "K 1\nK %x\n" % (2 ** 63 - 1), SAN_ENV)[1].split()) == 93


# ---- the entries on the real library, without a GPU ----
LIBRARY_SYMBOLS = ("seeqdevScanSetLibrary", "seeqdevScanTallyLibrary", "seeqdevScanTallyHoldLibrary")
FIELDS = [("nspans", 0), ("nassigned", 8), ("nexact", 16), ("ncorrected", 24), ("nambiguous", 32), ("nunknown", 40), ("nlong", 48), ("nforeign", 56),
          ("ndistinct", 64), ("key_bits", 72), ("passes", 76)]


def test_library_symbols_exported(capi):
    L = capi.lib()
    hdr = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    for name in LIBRARY_SYMBOLS:
        assert name in capi.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name


def test_library_counts_layout(capi):
    t = capi.seeqdev_tally_library_counts_t
    assert C.sizeof(t) == 80 and [(n, getattr(t, n).offset) for n, _ in t._fields_] == FIELDS
    hdr = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} seeqdev_tally_library_counts_t;", hdr).group(1)
    names = [n for decl in re.findall(r"^\s*uint\d+_t\s+([^;]+);", body, re.M) for n in re.split(r"\s*,\s*", decl)]
    assert names == [n for n, _ in FIELDS]


def _fails(call, code):
    C.set_errno(0)
    assert call() == -1
    assert C.get_errno() == code


def test_set_library_refusals_without_a_device(capi):
    # Every refusal comes before the device is touched: the stand-in context is all zeros.
    L = capi.lib()
    ctx = C.addressof(C.create_string_buffer(8192))
    arr = lambda ks: (C.c_uint64 * len(ks))(*ks)            # noqa: E731
    good = arr([py_key(b"ACGT")[1], py_key(b"ACGA")[1], 1])
    _fails(lambda: L.seeqdevScanSetLibrary(None, good, 3, 1), errno.EINVAL)                     # NULL scan
    _fails(lambda: L.seeqdevScanSetLibrary(ctx, None, 3, 1), errno.EINVAL)                      # NULL keys with n > 0
    for mm in (2, -1, 255):
        _fails(lambda: L.seeqdevScanSetLibrary(ctx, good, 3, mm), errno.EINVAL)                 # max_mismatch outside {0, 1}
    for keys, code, at in BAD_LIBRARIES:
        _fails(lambda: L.seeqdevScanSetLibrary(ctx, arr(keys), len(keys), 1), errno.EINVAL)     # no key / a duplicate: the message names the index
        assert ("entry %d " % at) in capi.error_text() and ("no tally key" if code == E_NOKEY else "repeats") in capi.error_text()
    for n in (LIB_MAX + 1, 2 ** 32, 2 ** 40):
        _fails(lambda: L.seeqdevScanSetLibrary(ctx, good, n, 1), errno.E2BIG)                   # (decided before a key is read)
    assert L.seeqdevScanSetLibrary(ctx, None, 0, 1) == 0 and L.seeqdevScanSetLibrary(ctx, good, 0, 0) == 0      # n == 0 clears, and touches no device


def test_library_tally_argument_checks_without_a_device(capi):
    # The checks come before the device is touched: the stand-in context is all zeros -- no library, no completed inserts call.
    L = capi.lib()
    ctx = C.addressof(C.create_string_buffer(8192))
    text = C.cast(C.c_char_p(b"ACGT\n"), C.c_void_p)
    cnt = capi.seeqdev_tally_library_counts_t()
    ok = C.byref(cnt)
    INS, HITS, DEMUX = capi.SEEQDEV_TALLY_INSERTS, capi.SEEQDEV_TALLY_HITS, capi.SEEQDEV_TALLY_DEMUX
    for entry in (L.seeqdevScanTallyLibrary, L.seeqdevScanTallyHoldLibrary):
        for source in (INS, HITS):
            _fails(lambda: entry(None, source, text, 5, ok), errno.EINVAL)                      # NULL context
            _fails(lambda: entry(ctx, source, text, 5, None), errno.EINVAL)                     # NULL counts
            _fails(lambda: entry(ctx, source, None, 5, ok), errno.EINVAL)                       # NULL text with bytes
            _fails(lambda: entry(ctx, source, text, 5, ok), errno.EINVAL)                       # no library
            assert "no library" in capi.error_text()
        for source in (DEMUX, 3, -1, 255):
            _fails(lambda: entry(ctx, source, text, 5, ok), errno.EINVAL)                       # an unknown source; demux names none, for the hold either
            _fails(lambda: entry(ctx, source, None, 0, ok), errno.EINVAL)
    # what stays as it is: the plain entries know no new source
    tc, hc = capi.seeqdev_tally_counts_t(), capi.seeqdev_tally_hold_counts_t()
    for source in (2, -1, 255):
        _fails(lambda: L.seeqdevScanTally(ctx, source, text, 5, C.byref(tc)), errno.EINVAL)
    _fails(lambda: L.seeqdevScanTallyHold(ctx, 3, text, 5, C.byref(hc)), errno.EINVAL)


def test_library_counts_is_the_dense_vector():
    from seeq_amd import device as dev
    res = dict(ids=np.array([1, 3, 7], dtype=np.uint64), counts=np.array([5, 2, 2 ** 40], dtype=np.uint64))
    out = dev.library_counts(res, 8)
    assert out.dtype == np.uint64 and out.tolist() == [5, 0, 2, 0, 0, 0, 2 ** 40, 0]
    assert dev.library_counts(res, 7).tolist() == [5, 0, 2, 0, 0, 0, 2 ** 40]
    empty = dict(ids=res["ids"][:0], counts=res["counts"][:0])
    assert dev.library_counts(empty, 3).tolist() == [0, 0, 0] and dev.library_counts(empty, 0).tolist() == []
    for bad_n in (6, 2):
        with pytest.raises(ValueError):
            dev.library_counts(res, bad_n)                  # an id beyond the library
    with pytest.raises(ValueError):
        dev.library_counts(dict(ids=np.array([0], dtype=np.uint64), counts=np.array([1], dtype=np.uint64)), 3)      # id 0 is no entry
