"""GPU (-m gpu): counting spans against a known library (seeqdevScanSetLibrary / seeqdevScanTallyLibrary / seeqdevScanTallyHoldLibrary;
seeq_tally_library.h: the exact pass, the compaction of the misses, the near pass, then the tally's own sort over ids) against the
brute-force rule of test_tally_library_host.py -- a Hamming distance over strings of equal length, no neighbours -- applied to the
inserts that were PLANTED.  Built on test_gpu_tally.py: reads are prefix + exact left flank + chosen insert + exact right flank +
suffix, every case first asserts that the inserts call found exactly the planted inserts, and a device fault ends the module."""
import collections
import ctypes as C
import errno
import random

import numpy as np
import pytest

from oracle.pyoracle import SQ_ALL, SQ_BEST
from test_gpu_inserts import _fastq
from test_gpu_tally import LEFT, T, _cuda, _go, _insert_lines, _nothing_after_a_device_fault, _reads      # noqa: F401 (the fixture is this module's latch too)
from test_gpu_tally_grouped import FA, _cut, _held_of, fl      # noqa: F401
from test_gpu_tally_grouped import _reads as _guide_umi_reads
from test_gpu_tally_grouped import _same as _same_grouped
from test_gpu_tally_grouped import _text
from test_tally_host import py_key
from test_tally_library_host import EXACT, PyLibrary, _rand, _sub, bitlen_passes

pytestmark = pytest.mark.gpu
COUNTS = ("nspans", "nassigned", "nexact", "ncorrected", "nambiguous", "nunknown", "nlong", "nforeign", "ndistinct", "key_bits", "passes")


@pytest.fixture(scope="module")
def flanks(gpu):
    from seeq_amd import device as dev
    from test_gpu_tally import RIGHT
    ps = (dev.Pattern(LEFT, 0), dev.Pattern(RIGHT, 0))
    yield ps
    for p in ps:
        p.close()


# ---- expected values: the brute-force rule over spans that the code under test did not cut ----
def _same(res, lib, spans, mm):
    from seeq_amd import device as dev
    cnt, dense, _ = lib.tally(spans, mm)
    bits, passes = bitlen_passes(len(lib), cnt["nassigned"])
    assert {k: res[k] for k in COUNTS} == dict(cnt, key_bits=bits, passes=passes)
    assert res["nspans"] == res["nexact"] + res["ncorrected"] + res["nambiguous"] + res["nunknown"] + res["nlong"] + res["nforeign"]
    assert res["nassigned"] == res["nexact"] + res["ncorrected"]
    assert res["ids"].dtype == np.uint64 and res["counts"].dtype == np.uint64
    ids = res["ids"].tolist()
    assert all(a < b for a, b in zip(ids, ids[1:])) and all(1 <= i <= len(lib) for i in ids)      # the ids ascend
    exp = [(i + 1, c) for i, c in enumerate(dense) if c]
    got = list(zip(ids, res["counts"].tolist()))
    if got != exp:
        bad = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
        raise AssertionError("tables differ (%d vs %d entries; first difference at %d: %s vs %s)" % (len(got), len(exp), bad, got[bad:bad + 1], exp[bad:bad + 1]))
    assert int(res["counts"].sum()) == res["nassigned"]
    assert dev.library_counts(res, len(lib)).tolist() == dense
    return cnt


def _planted(sc, flanks, lib, inserts, what, mm=1, seed=1, fastq=False):
    """set_library, the inserts call over reads that carry `inserts` (its result checked against what was planted), then the library
    tally against the rule."""
    from seeq_amd import device as dev
    buf = _reads(inserts, seed)
    if fastq:
        buf = _fastq([ln.decode() for ln in buf.split(b"\n")[:-1]], seed + 1, LEFT)[0]
    t = _cuda(buf)

    def call(s):
        s.set_library(lib.seqs, mm)
        res = s.inserts_tensor(flanks[0], flanks[1], t, SQ_BEST | (dev.SEEQDEV_FASTQ if fastq else 0), copy=False)
        assert res["ninserts"] == len(inserts), (what, res)
        assert _insert_lines(s, t) == list(inserts), what
        return s.tally_library(t)
    got = {}
    _go(sc, what, call, lambda s, res: got.update(res=res, cnt=_same(res, lib, inserts, mm)))
    return got["res"], t


def _library(n, seed, empty=False):
    """n entries of 12 and 20 bases mixed (and the empty sequence), shuffled; its first two entries after the shuffle are NOT special.
    -> (PyLibrary, a pair of entries at distance 1)"""
    rng = random.Random(seed)
    x = _rand(rng, 12)
    seqs = {x, _sub(x, 4, 1)} | ({b""} if empty else set())
    while len(seqs) < n:
        seqs.add(_rand(rng, rng.choice((12, 20))))
    seqs = sorted(seqs)
    rng.shuffle(seqs)
    return PyLibrary(seqs), (x, _sub(x, 4, 1))


def _one_sub(rng, s, at=None):
    return _sub(s, rng.randrange(len(s)) if at is None else at, rng.randrange(1, 4))


def _mixed(rng, lib, n):
    """n inserts: mostly entries, a fifth with one substitution, some with two, some random, an N, a long one."""
    out = []
    for _ in range(n):
        s, r = rng.choice(lib.seqs), rng.random()
        if r < 0.6 or not s:
            out.append(s)
        elif r < 0.8:
            out.append(_one_sub(rng, s))
        elif r < 0.87:
            out.append(_one_sub(rng, _one_sub(rng, s)))
        elif r < 0.94:
            out.append(_rand(rng, rng.choice((11, 12, 15, 20))))
        elif r < 0.97:
            out.append(s[:3] + b"N" + s[4:])
        else:
            out.append(_rand(rng, 32))
    return out


# ---- shapes ----
@pytest.mark.parametrize("n", [1, T - 1, T, T + 1, 4 * T + 4])
def test_span_counts(gpu, capi, flanks, n):
    """Around the tile T (1 023, 1 024, 1 025), one span, more than four tiles; a library of 300 entries: ids of 9 bits, two passes."""
    from seeq_amd import device as dev
    lib, _ = _library(300, 300)
    sc = dev.Scanner()
    res, _ = _planted(sc, flanks, lib, _mixed(random.Random(n), lib, n), "%d spans" % n, seed=n)
    assert res["nspans"] == n and res["key_bits"] == 9 and res["passes"] == (2 if res["nassigned"] else 0)
    if n > 1:
        assert res["passes"] == 2 and res["ncorrected"] > 50 and res["nunknown"] > 20
    sc.close()


@pytest.mark.parametrize("nlib", [2, 255, 256, 257, 513, 5000])
def test_library_sizes(gpu, capi, flanks, nlib):
    """A workgroup keeps 256 sampled library keys in LDS, every ceil(N / 256)-th one: N at and around 256 (every key a sample, then every
    second one), N = 513 (a stride of 3 with a short last block), N = 5 000 (a stride of 20; ids of 13 bits)."""
    from seeq_amd import device as dev
    lib, _ = _library(nlib, 400 + nlib)
    sc = dev.Scanner()
    res, _ = _planted(sc, flanks, lib, _mixed(random.Random(nlib), lib, T + 50), "a library of %d" % nlib, seed=nlib)
    assert res["key_bits"] == nlib.bit_length() and res["passes"] == (nlib.bit_length() + 7) // 8 and res["ncorrected"] > 100
    sc.close()


def test_a_library_of_one_entry(gpu, capi, flanks):
    from seeq_amd import device as dev
    lib = PyLibrary([b"ACGTTGCAAGCT"])
    rng = random.Random(1)
    inserts = [rng.choice([lib.seqs[0], _one_sub(rng, lib.seqs[0]), _rand(rng, 12), b"", lib.seqs[0][:-1]]) for _ in range(T + 9)]
    sc = dev.Scanner()
    res, _ = _planted(sc, flanks, lib, inserts, "a one-entry library")
    assert (res["key_bits"], res["passes"], res["ndistinct"]) == (1, 1, 1) and res["ids"].tolist() == [1]
    assert res["nexact"] > 100 and res["ncorrected"] > 100 and res["nunknown"] > 100 and res["nambiguous"] == 0
    sc.close()


def _categories(lib, pair, empty):
    """Every category in one text -> (inserts, the numbers planted per category)."""
    rng = random.Random(77)
    long_enough = [s for s in lib.seqs if len(s) >= 12 and s not in pair]
    out = [rng.choice(lib.seqs) for _ in range(T)]                                    # exact
    for at in (0, None, -1):                                                          # one substitution at the first, a middle, the last base
        for _ in range(60):
            s = rng.choice(long_enough)
            out.append(_one_sub(rng, s, {0: 0, None: len(s) // 2, -1: len(s) - 1}[at]))
    out += [_one_sub(rng, _sub(rng.choice(long_enough), 2, 1), 9) for _ in range(40)]         # two substitutions
    out += [s[:5] + b"N" + s[6:] for s in rng.sample(long_enough, 12)]                # an N: foreign
    out += [_rand(rng, 32) for _ in range(7)] + [b"N" * 40]                           # 32 bases, and long before foreign
    out += [rng.choice(long_enough).lower().replace(b"t", b"u") for _ in range(25)]   # lower case and U: the entry
    out += [_rand(rng, 15) for _ in range(20)]                                        # a length that no entry has
    out += [s[:6] + s[7:] for s in rng.sample(long_enough, 20)]                       # an entry with one base deleted
    x, y = pair
    at = next(i for i in range(len(x)) if x[i] != y[i])
    third = [z for z in (_sub(x, at, o) for o in (1, 2, 3)) if z != y]
    out += [rng.choice(third) for _ in range(30)]                                     # ambiguous by construction
    out += [x] * 9 + [y] * 11                                                         # exact wins
    out += [b""] * 14                                                                 # the empty insert
    rng.shuffle(out)
    return out


@pytest.mark.parametrize("empty", [False, True], ids=["no_empty_key", "empty_key_in_the_library"])
@pytest.mark.parametrize("mm", [1, 0], ids=["one_mismatch", "exact_only"])
def test_the_categories_in_one_text(gpu, capi, flanks, mm, empty):
    """Exact, one substitution at the first / a middle / the last base, two substitutions, N, 32 bases, lower case and U, a length no
    entry has, a deletion, ambiguous by construction, exact wins, the empty insert with and without the empty key in the library.  Under
    max_mismatch 0 the corrected and the ambiguous spans are unknown."""
    from seeq_amd import device as dev
    lib, pair = _library(300, 301, empty)
    inserts = _categories(lib, pair, empty)
    one, _, ids = lib.tally(inserts, 1)
    # before any device call: the text holds what it is meant to hold
    assert one["ncorrected"] >= 100 and one["nambiguous"] >= 10 and one["nunknown"] >= 10 and one["nforeign"] >= 1 and one["nlong"] >= 1
    x, y = pair
    by = dict(zip(inserts, ids))
    assert by[x] and by[y] and by[x] != by[y] and bool(by[b""]) == empty
    zero = lib.tally(inserts, 0)[0]
    assert zero["ncorrected"] == zero["nambiguous"] == 0 and zero["nunknown"] == one["nunknown"] + one["ncorrected"] + one["nambiguous"]
    assert zero["nexact"] == one["nexact"] and (zero["nlong"], zero["nforeign"]) == (one["nlong"], one["nforeign"]) == (8, 12)
    sc = dev.Scanner()
    res, _ = _planted(sc, flanks, lib, inserts, "the categories, max_mismatch %d" % mm, mm=mm)
    assert res["ncorrected"] == (one["ncorrected"] if mm else 0) and res["nambiguous"] == (one["nambiguous"] if mm else 0)
    sc.close()


def _miss_shape(shape, lib):
    rng = random.Random(len(shape))
    entry = lambda: rng.choice(lib.seqs)                    # noqa: E731

    def miss():
        while True:
            s = rng.choice([_one_sub(rng, entry()), _rand(rng, 12), _rand(rng, 20), _rand(rng, 15)])
            if lib.assign(s, 1)[1] != EXACT:                # (a substitution can lead from one entry to another)
                return s
    if shape == "none":
        return [entry() for _ in range(2 * T + 3)], 0
    if shape == "all":
        return [miss() for _ in range(2 * T + 3)], 2 * T + 3
    if shape in ("1024", "1025", "3"):
        k = int(shape)
        out = [miss() for _ in range(k)] + [entry() for _ in range(3 * T + 5 - k)]
        rng.shuffle(out)
        return out, k
    assert shape == "first_and_last"
    return [miss()] + [entry() for _ in range(T + 7)] + [miss()], 2


@pytest.mark.parametrize("shape", ["none", "all", "1024", "1025", "first_and_last", "3"])
def test_shapes_of_the_miss_path(gpu, capi, flanks, shape):
    """No miss at all (the near pass is not launched); every span a miss; exactly 1 024 and 1 025 misses (the compaction's tile edge);
    a miss as the first and as the last span; an odd number of misses (the last workgroup's half-waves but one idle)."""
    from seeq_amd import device as dev
    lib, _ = _library(300, 302)
    inserts, k = _miss_shape(shape, lib)
    exp = lib.tally(inserts, 1)[0]
    assert exp["nspans"] - exp["nexact"] == k and exp["nlong"] == exp["nforeign"] == 0      # the misses are exactly those planted
    if shape == "first_and_last":
        assert lib.assign(inserts[0], 1)[1] and lib.assign(inserts[-1], 1)[1]
    sc = dev.Scanner()
    res, _ = _planted(sc, flanks, lib, inserts, "misses: %s" % shape, seed=len(shape))
    assert res["ncorrected"] + res["nambiguous"] + res["nunknown"] == k
    sc.close()


# ---- the hold ----
def test_the_hold_folds_erroneous_guides_into_their_entry(gpu, capi, fl):
    """Guides with planted errors plus 12-base UMIs: tally_hold_library on the guide inserts, then the unchanged tally_grouped on the
    UMI inserts.  The pair and group tables are a Counter over (id, UMI key); there are as many groups as library entries planted, and
    the uncorrected tally_hold over the same input gives more."""
    from seeq_amd import device as dev
    rng = random.Random(9)
    lib, _ = _library(40, 303)
    used = rng.sample(range(len(lib)), 11) + [len(lib) - 1]            # (the last entry is among them: the largest id has bitlen(N) bits)
    used = sorted(set(used))
    umis = [_rand(rng, 12) for _ in range(30)]
    spec = []
    for _ in range(2 * T + 50):
        g, r = lib.seqs[rng.choice(used)], rng.random()
        guide = g if r < 0.7 else _one_sub(rng, g) if r < 0.9 else _one_sub(rng, _one_sub(rng, g)) if r < 0.95 else g[:4] + b"N" + g[5:]
        spec.append((guide, rng.choice(umis)))
    spec += [(None, umis[0]), (lib.seqs[used[0]], None)]
    lines = _guide_umi_reads(spec, 9)
    guides = [(i + 1, g) for i, (g, _) in enumerate(spec) if g is not None]
    members = [(i + 1, u) for i, (_, u) in enumerate(spec) if u is not None]
    cnt, _, ids = lib.tally([g for _, g in guides], 1)
    held = [(ln, i) for (ln, _), i in zip(guides, ids)]
    assert cnt["ncorrected"] > 200 and cnt["nunknown"] > 20 and cnt["nforeign"] > 20 and {i for i in ids if i} == {u + 1 for u in used}
    plain_held, _ = _held_of(guides)
    t = _cuda(_text(lines))

    def call(s):
        s.set_library(lib.seqs, 1)
        _cut(s, fl["A"], fl["B"], t, guides, "guides")
        hold = s.tally_hold_library(t)
        _cut(s, fl["C"], fl["D"], t, members, "UMIs")
        corrected = s.tally_grouped(t)
        _cut(s, fl["A"], fl["B"], t, guides, "guides again")
        s.tally_hold(t)
        _cut(s, fl["C"], fl["D"], t, members, "UMIs again")
        return hold, corrected, s.tally_grouped(t)

    def check(s, got):
        hold, corrected, plain = got
        bits, _ = bitlen_passes(len(lib))
        assert {k: hold[k] for k in COUNTS} == dict(cnt, ndistinct=0, key_bits=bits, passes=0)
        pairs, groups = _same_grouped(corrected, held, members)
        by_line = dict(held)
        tab = collections.Counter((by_line[ln], py_key(u)[1]) for ln, u in members if by_line.get(ln))
        assert pairs == [(g, m, c) for (g, m), c in sorted(tab.items())]
        assert [g[0] for g in groups] == [u + 1 for u in used] and corrected["ngroups"] == len(used)
        _same_grouped(plain, plain_held, members)
        assert plain["ngroups"] > corrected["ngroups"] + 100          # every erroneous copy opens a group of its own
    sc = dev.Scanner()
    _go(sc, "the library hold", call, check)
    sc.close()


# ---- context state ----
def test_the_library_belongs_to_the_context(gpu, capi, flanks):
    """The library survives a plain scan, an inserts call, a plain tally and a demultiplex; a plain tally after a library tally gives
    the plain answer bit for bit, as on a fresh Scanner; a second set_library replaces the first; clear_library makes the library
    tally EINVAL."""
    from seeq_amd import device as dev
    lib, _ = _library(300, 304)
    other, _ = _library(70, 305)
    rng = random.Random(12)
    inserts = _mixed(rng, lib, T + 40) + [rng.choice(other.seqs) for _ in range(50)]
    sc = dev.Scanner()
    first, t = _planted(sc, flanks, lib, inserts, "the first library tally")
    table = sc.tally_table(first["ndistinct"]).tobytes()
    # a plain tally in between: the plain answer, as on a fresh Scanner
    plain = sc.tally(t, copy=False)
    plain_table = sc.tally_table(plain["ndistinct"]).tobytes()
    fresh = dev.Scanner()
    assert fresh.inserts_tensor(flanks[0], flanks[1], t, SQ_BEST, copy=False)["ninserts"] == len(inserts)
    assert fresh.tally(t, copy=False) == plain and fresh.tally_table(plain["ndistinct"]).tobytes() == plain_table
    fresh.close()
    assert plain["ndistinct"] > first["ndistinct"]
    # a plain scan, a demultiplex, an inserts call: the library is still the context's
    sc.scan_tensor(flanks[0], t, SQ_BEST, dev.WANT_RECORDS)
    assert sc.demux_tensor(list(flanks), t)["nassigned"] > 0
    assert sc.inserts_tensor(flanks[0], flanks[1], t, SQ_BEST, copy=False)["ninserts"] == len(inserts)
    again = sc.tally_library(t)
    assert {k: again[k] for k in COUNTS} == {k: first[k] for k in COUNTS} and sc.tally_table(again["ndistinct"]).tobytes() == table
    _same(again, lib, inserts, 1)
    # a second library replaces the first; with max_mismatch 0 and as an array of keys
    sc.set_library(np.array(other.keys(), dtype=np.uint64), 0)
    _same(sc.tally_library(t), other, inserts, 0)
    # a refused set leaves no library, and so does clear_library
    with pytest.raises(dev.SeeqDeviceError):
        sc.set_library([b"ACGT", b"ACGT"])
    for k in range(2):
        cnt = capi.seeqdev_tally_library_counts_t()
        C.set_errno(0)
        assert sc._lib.seeqdevScanTallyLibrary(sc._h, capi.SEEQDEV_TALLY_INSERTS, C.c_void_p(t.data_ptr()), t.numel(), C.byref(cnt)) == -1
        assert C.get_errno() == errno.EINVAL and "no library" in capi.error_text()
        with pytest.raises(dev.SeeqDeviceError):
            sc.tally_hold_library(t)
        sc.set_library(lib.seqs)
        _same(sc.tally_library(t), lib, inserts, 1)
        sc.clear_library()
    assert sc.tally(t, copy=False) == plain and sc.tally_table(plain["ndistinct"]).tobytes() == plain_table
    sc.close()


def test_hits_of_a_both_strands_call_against_a_library(gpu, capi):
    """source="hits": the matches of a pattern with four free bases, on both strands; a minus-strand hit is the bytes of the text."""
    from seeq_amd import device as dev
    rng = random.Random(14)
    hit = lambda four: b"CATGCATG" + four + b"GTACGTAC"      # noqa: E731
    rc = lambda s: s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))      # noqa: E731
    fours = [_rand(rng, 4) for _ in range(20)]
    lib = PyLibrary(sorted({hit(f) for f in fours[:12]}) + [rc(hit(fours[0]))])
    spans = []
    for _ in range(T + 30):
        s = hit(rng.choice(fours))
        r = rng.random()
        spans.append(rc(s) if r < 0.2 else _sub(s, 9, 1) if r < 0.4 else s)
    lines = [_rand(rng, rng.randrange(1, 9)).replace(b"C", b"A") + s + _rand(rng, rng.randrange(1, 9)).replace(b"G", b"T") for s in spans]
    exp = lib.tally(spans, 1)[0]
    assert exp["nexact"] > 300 and exp["ncorrected"] > 50 and exp["nambiguous"] > 10 and exp["nunknown"] > 100
    t = _cuda(b"\n".join(lines) + b"\n")
    pat = dev.Pattern("CATGCATGNNNNGTACGTAC", 0)

    def call(s):
        s.set_library(lib.seqs)
        cnt = s.strands_tensor(pat, t, SQ_ALL, dev.WANT_RECORDS, copy=False)
        assert cnt["nrecords"] == len(spans) and cnt["per_strand"][1] > 100
        rec = s.records(len(spans))
        assert [lines[i][a:b] for i, (a, b) in enumerate(zip(rec[:, 1].tolist(), rec[:, 2].tolist()))] == spans and rec[:, 0].tolist() == list(range(1, len(spans) + 1))
        return s.tally_library(t, source="hits")
    sc = dev.Scanner()
    _go(sc, "hits of a both-strands call", call, lambda s, res: _same(res, lib, spans, 1))
    pat.close()
    sc.close()


def test_library_tally_under_fastq(gpu, capi, flanks):
    """SEEQDEV_FASTQ inserts: the offsets are those of the sequence lines in the original buffer."""
    from seeq_amd import device as dev
    lib, _ = _library(300, 306)
    sc = dev.Scanner()
    res, _ = _planted(sc, flanks, lib, _mixed(random.Random(16), lib, T + 77), "FASTQ", seed=16, fastq=True)
    assert res["ncorrected"] > 100
    sc.close()
