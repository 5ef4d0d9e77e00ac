"""GPU (-m gpu): the collapse behind the grouped tally (seeqdevScanTallyCollapse; seeq_tally_collapse.h: the parent of every pair, the
prefix over the pairs, the group rows, all on the device) against the rule restated in Python (test_tally_collapse_host.py: decoded
members, Hamming distances, no neighbour ever computed) applied to the pair table that py_pairs predicts from what was PLANTED -- never to
anything the code under test made.  Reads are those of test_gpu_tally_grouped.py, and every case first asserts that the inserts calls found
exactly what was planted and that the grouped call gave the predicted tables: a vacuous case fails."""
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle.pyoracle import SQ_ALL, SQ_BEST
from test_gpu_strands import _line_offsets
from test_gpu_tally_grouped import FA, FB, FC, FD, _FAULT, _cuda, _cut, _go, _held_of, _hit, _kmer, _reads, _same, _text
from test_gpu_tally_grouped import fl  # noqa: F401  (the module's patterns: a fixture)
from test_tally_collapse_host import ANY, DIRECTIONAL, RULES, as_array, check_hand, hand_groups, np_collapse_both, py_collapse
from test_tally_host import py_key

pytestmark = pytest.mark.gpu
T = int(re.search(r"#define\s+SEEQ_TALLY_TILE\s+(\d+)", open(os.path.join(ROOT, "seeq_amd", "csrc", "seeq_tally.h")).read()).group(1))
WG = 64                                                     # pairs per workgroup of k_collapse_parent
NAMES = {DIRECTIONAL: "directional", ANY: "any"}
COUNTS = ("npairs", "ngroups", "nroots", "nabsorbed", "absorbed_reads", "rule", "max_len")
BRUTE = 400                                                 # pairs up to which the brute force restates the rule; the bucketed one beyond


@pytest.fixture(autouse=True)
def _nothing_after_a_device_fault():
    """A device fault ends the module (and is shared with test_gpu_tally_grouped.py, whose steps these tests take): what comes after it
    fails here, before it starts anything on the device."""
    if _FAULT:
        pytest.fail("a device fault earlier (%s): nothing more is started on the device" % _FAULT[0])
    yield


# ---- the expectation ----
def _restated(pairs):
    """{rule: (parent list, rows)} of a pair table [(g, m, c)]."""
    if len(pairs) <= BRUTE:
        return {rule: py_collapse(pairs, rule) for rule in RULES}
    both = np_collapse_both(as_array(pairs))
    return {rule: (both[rule][0].tolist(), both[rule][1]) for rule in RULES}


def _same_collapse(got, pairs, groups, exp, rule, max_len):
    """A tally_collapse() result (copy=True) against the restated rule over the predicted tables."""
    parent, rows = exp[rule]
    want = dict(npairs=len(pairs), ngroups=len(groups), nroots=sum(r[0] for r in rows), nabsorbed=sum(r[1] for r in rows),
                absorbed_reads=sum(r[2] for r in rows), rule=rule, max_len=max_len)
    print("collapse %s: %s" % (NAMES[rule], {k: got[k] for k in COUNTS}))
    assert {k: got[k] for k in COUNTS} == want
    assert got["parent"].dtype == np.uint32 and len(got["parent"]) == len(pairs) and len(got["groups"]) == len(groups)
    have = got["parent"].tolist()
    if have != parent:
        bad = [i for i, (a, b) in enumerate(zip(have, parent)) if a != b]
        raise AssertionError("parents differ under %s at %d of %d pairs; first at %d: %d, expected %d" % (NAMES[rule], len(bad), len(parent), bad[0], have[bad[0]],
                                                                                                         parent[bad[0]]))
    assert [tuple(int(x) for x in r) for r in got["groups"]] == rows
    assert all(int(r["nroots"]) + int(r["nabsorbed"]) == g[3] and int(r["nroots"]) >= 1 for r, g in zip(got["groups"], groups))
    assert got["nroots"] + got["nabsorbed"] == got["npairs"]


def _spec_of(items):
    """items: [(guide bytes, umi bytes, count)] -> one line per read, shuffled."""
    spec = [(g, u) for g, u, c in items for _ in range(c)]
    random.Random(len(spec)).shuffle(spec)
    return spec


def _collapsed(sc, fl, spec, what, seed=1, rules=RULES, extra=None):
    """inserts(A, B), hold, inserts(C, D), grouped, then the collapse under each rule -- over reads that carry `spec`, every step checked
    against what was planted.  -> ({rule: result}, pairs, groups, the text's tensor)"""
    lines = _reads(spec, seed)
    t = _cuda(_text(lines))
    guides = [(i + 1, g) for i, (g, _) in enumerate(spec) if g is not None]
    umis = [(i + 1, u) for i, (_, u) in enumerate(spec) if u is not None]
    held, hcnt = _held_of(guides)
    memo = {}

    def call(s):
        _cut(s, fl["A"], fl["B"], t, guides, what + ": guides")
        hold = s.tally_hold(t)
        _cut(s, fl["C"], fl["D"], t, umis, what + ": UMIs")
        res = s.tally_grouped(t)
        return hold, res, {rule: s.tally_collapse(NAMES[rule]) for rule in rules}
    out = {}

    def check(s, got):
        hold, res, col = got
        assert hold == hcnt
        if "tables" not in memo:
            memo["tables"] = _same(res, held, umis)
            memo["exp"] = _restated(memo["tables"][0])
        else:
            assert [tuple(int(x) for x in r) for r in res["pairs"]] == memo["tables"][0]
        pairs, groups = memo["tables"]
        for rule in rules:
            _same_collapse(col[rule], pairs, groups, memo["exp"], rule, res["max_len"])
        if extra:
            extra(s, res, col, pairs, groups, memo["exp"])
        out.update(col=col, pairs=pairs, groups=groups, exp=memo["exp"], res=res)
    _go(sc, what, call, check)
    return out, t


def _crowded(rng, n, guides, ulen=6):
    """n distinct (guide, UMI) pairs whose UMIs crowd a small space -- consecutive k-mers: neighbours, ties and chains everywhere -- with
    counts between 1 and 40."""
    return [(guides[k % len(guides)], _kmer(k // len(guides), ulen), rng.choice([1, 1, 1, 1, 2, 2, 3, 5, 9, 40])) for k in range(n)]


G3 = [b"ACGTACGTACGTACGTACGT", b"ACGTACGTACGTACGTACGA", b"TTGACCGATCAGGATTACAT"]


# ---- shapes ----
@pytest.mark.parametrize("n", [0, 1, WG - 1, WG, WG + 1, T - 1, T, T + 1, 2 * T + 1])
def test_pair_counts(gpu, capi, fl, n):
    """Around the 64 pairs of a workgroup of k_collapse_parent and around the tile T of the prefix.  No pair at all launches nothing and
    gives zeros.  Three lines carry a guide and no UMI."""
    from seeq_amd import device as dev
    rng = random.Random(n)
    spec = _spec_of(_crowded(rng, n, G3)) + [(G3[0], None)] * 3
    sc = dev.Scanner()
    sc.set_profiling(True)
    out, _ = _collapsed(sc, fl, spec, "%d pairs" % n, seed=n)
    for rule in RULES:
        col = out["col"][rule]
        assert col["npairs"] == n and (n == 0) == (col["nroots"] == 0)
        if n == 0:
            assert {k: col[k] for k in COUNTS} == dict(npairs=0, ngroups=0, nroots=0, nabsorbed=0, absorbed_reads=0, rule=rule, max_len=0)
            assert len(col["parent"]) == 0 and len(col["groups"]) == 0 and col["groups"].dtype == dev.TALLY_COLLAPSE_DTYPE
    assert (sc.last_tally_collapse_ms() > 0) == (n > 0)        # nothing launched, nothing timed
    if n > WG:
        assert out["col"][ANY]["nabsorbed"] > out["col"][DIRECTIONAL]["nabsorbed"] > 0
    sc.close()


def test_more_than_256_tiles(gpu, capi, fl):
    """256 T + 1 pairs in five groups: tile_top's second round, and every kernel's grid beyond one of its own rounds.  The lines are built
    with NumPy -- fixed-width reads, a guide of 4 and a UMI of 9 bases -- and so is the prediction of the pair table (the keys of
    consecutive k-mers, counted by np.unique): py_pairs would search the held column per line.  The device's pair table must BE that
    prediction before anything is said about the collapse."""
    import torch
    from seeq_amd import device as dev
    rng = np.random.default_rng(256)
    npairs, ng, glen, ulen = 256 * T + 1, 5, 4, 9
    k = np.arange(npairs)
    extra = rng.integers(0, npairs, 40000) // rng.integers(1, 50, 40000)      # skewed: a few pairs many times
    which = rng.permutation(np.concatenate((k, extra)))
    gidx, uidx = which % ng * 37 + 11, which // ng                            # guides far apart; a group's UMIs are consecutive k-mers: crowded
    assert int(uidx.max()) < 4 ** ulen

    def bases(idx, m):
        return np.frombuffer(b"ACTG", dtype=np.uint8)[(idx[:, None] >> (2 * (m - 1 - np.arange(m)))[None, :]) & 3]
    cols = [np.frombuffer(FA.encode(), dtype=np.uint8), None, np.frombuffer((FB + "ACG" + FC).encode(), dtype=np.uint8), None,
            np.frombuffer((FD + "\n").encode(), dtype=np.uint8)]
    n = len(which)
    parts = [np.broadcast_to(c, (n, len(c))) if c is not None else None for c in cols]
    parts[1], parts[3] = bases(gidx, glen), bases(uidx, ulen)
    text = np.ascontiguousarray(np.concatenate(parts, axis=1))
    t = torch.from_numpy(text.reshape(-1)).cuda()
    # the prediction: a k-mer of index i has the key (1 << 2 m) | i
    gkey, ukey = (1 << (2 * glen)) | gidx.astype(np.uint64), (1 << (2 * ulen)) | uidx.astype(np.uint64)
    both, counts = np.unique(np.stack((gkey, ukey), axis=1), axis=0, return_counts=True)
    pairs = np.zeros(len(both), dtype=dev.TALLY_PAIR_DTYPE)
    pairs["group"], pairs["member"], pairs["count"] = both[:, 0], both[:, 1], counts
    assert len(pairs) == npairs
    exp = np_collapse_both(pairs)
    sc = dev.Scanner()

    def call(s):
        assert s.inserts_tensor(fl["A"], fl["B"], t, SQ_BEST, copy=False)["ninserts"] == n
        hold = s.tally_hold(t)
        assert s.inserts_tensor(fl["C"], fl["D"], t, SQ_BEST, copy=False)["ninserts"] == n
        res = s.tally_grouped(t)
        return hold, res, {rule: s.tally_collapse(NAMES[rule]) for rule in RULES}

    def check(s, got):
        hold, res, col = got
        assert hold["nheld"] == n and res["npaired"] == n and (res["npairs"], res["ngroups"], res["max_len"]) == (npairs, ng, ulen)
        assert res["pairs"].tobytes() == pairs.tobytes()
        first = np.flatnonzero(np.concatenate(([True], pairs["group"][1:] != pairs["group"][:-1])))
        assert res["groups"]["first"].tolist() == first.tolist()
        for rule in RULES:
            parent, rows = exp[rule]
            c = col[rule]
            print("collapse %s: %s" % (NAMES[rule], {x: c[x] for x in COUNTS}))
            assert np.array_equal(c["parent"], parent), (NAMES[rule], int((c["parent"] != parent).sum()), np.flatnonzero(c["parent"] != parent)[:5])
            assert [tuple(int(x) for x in r) for r in c["groups"]] == rows
            assert {x: c[x] for x in COUNTS} == dict(npairs=npairs, ngroups=ng, nroots=sum(r[0] for r in rows), nabsorbed=sum(r[1] for r in rows),
                                                     absorbed_reads=sum(r[2] for r in rows), rule=rule, max_len=ulen)
        assert col[ANY]["nabsorbed"] > col[DIRECTIONAL]["nabsorbed"] > 10000
    _go(sc, "256 T + 1 pairs", call, check)
    sc.close()


def test_one_group_holds_every_pair(gpu, capi, fl):
    from seeq_amd import device as dev
    sc = dev.Scanner()
    out, _ = _collapsed(sc, fl, _spec_of(_crowded(random.Random(3), T + 300, G3[:1])), "one group")
    assert len(out["groups"]) == 1 and out["groups"][0][3] == T + 300
    sc.close()


def test_every_pair_a_group_of_its_own(gpu, capi, fl):
    """ngroups == npairs: nothing has a candidate, whatever its neighbours in the groups beside it."""
    from seeq_amd import device as dev
    rng = random.Random(4)
    items = [(_kmer(k, 8), _kmer(k % 7, 6), rng.choice([1, 2, 50])) for k in range(T + 5)]
    sc = dev.Scanner()
    out, _ = _collapsed(sc, fl, _spec_of(items), "every pair a group")
    assert len(out["groups"]) == len(out["pairs"]) == T + 5
    for rule in RULES:
        assert out["col"][rule]["nabsorbed"] == 0 and out["col"][rule]["parent"].tolist() == list(range(T + 5))
    sc.close()


def test_segments_that_straddle_boundaries_and_a_group_whose_ends_are_neighbours(gpu, capi, fl):
    """Groups of 90 crowded pairs each: their segments straddle the 64-pair boundaries of k_collapse_parent's workgroups and the tile
    boundary at T, and pairs on either side of such a boundary have their parent on the other.  The last group's first and last member
    are neighbours: AAAAAA and GAAAAA with nothing above it."""
    from seeq_amd import device as dev
    rng = random.Random(5)
    guides = [_kmer(k, 8) for k in range(14)]
    items = [(guides[k // 90], _kmer(k % 90 + 7 * (k // 90), 6), rng.choice([1, 1, 2, 3, 9, 40])) for k in range(13 * 90)]
    items += [(guides[13], b"AAAAAA", 1), (guides[13], b"CCCCCC", 5), (guides[13], b"TTTTTT", 5), (guides[13], b"GAAAAA", 30)]
    sc = dev.Scanner()
    out, _ = _collapsed(sc, fl, _spec_of(items), "straddling segments")
    pairs, groups = out["pairs"], out["groups"]
    assert len(pairs) == 13 * 90 + 4 > T and any(g[2] < T < g[2] + g[3] for g in groups) and sum(1 for g in groups if g[2] // WG != (g[2] + g[3] - 1) // WG) >= 13
    for rule in RULES:
        parent = out["exp"][rule][0]
        assert any(i < T <= p for i, p in enumerate(parent)) and any(p < T <= i for i, p in enumerate(parent))
        assert sum(1 for i, p in enumerate(parent) if i // WG < p // WG) > 10 and sum(1 for i, p in enumerate(parent) if i // WG > p // WG) > 10
        first, nd = groups[-1][2], groups[-1][3]
        assert nd == 4 and parent[first] == first + 3 and parent[first + 3] == first + 3
    sc.close()


# ---- the rule's cases ----
def test_every_case_of_the_rule_that_text_can_produce(gpu, capi, fl):
    """The named cases of test_tally_collapse_host.py (without the counts near 2^63), one group each, planted once in one text: the chain
    100 - 10 - 1, the threshold on both sides, 5 beside 4, tied counts, two candidates, members of 0, 1, 16, 17 and 31 bases, mixed
    lengths, a member and its prefix, the same neighbours in adjacent groups, the last member of a group beside the first of the next,
    a group of one pair."""
    from seeq_amd import device as dev
    cases = hand_groups(big=False)
    items = [(_kmer(k, 8), m, c) for k, (_, members, _) in enumerate(cases) for m, c in members]

    def extra(s, res, col, pairs, groups, exp):
        assert len(groups) == len(cases)
        for rule in RULES:
            check_hand(pairs, col[rule]["parent"].tolist(), rule, big=False)
        # the chains are not followed on the device; the host helper does that
        top = [m for _, m, _ in pairs].index(py_key(b"ACGTTGCAAGCT")[1])
        root, folded = dev.collapse_fold(res["pairs"], col[DIRECTIONAL]["parent"])
        assert root[:3].tolist() == [top] * 3 and int(folded[top]) == 111 and len(set(col[DIRECTIONAL]["parent"][:3].tolist())) == 2
        assert int(folded.sum()) == res["npaired"] and int((folded > 0).sum()) == col[DIRECTIONAL]["nroots"]
    sc = dev.Scanner()
    out, _ = _collapsed(sc, fl, _spec_of(items), "the rule's cases", extra=extra)
    assert out["res"]["max_len"] == 31 and out["col"][ANY]["nabsorbed"] > out["col"][DIRECTIONAL]["nabsorbed"] > 10
    sc.close()


# ---- other sources of groups and members ----
def _members_around(rng, n, base=b"ACGTTGCAAGCTACGTTGCA"):
    """n sequences drawn from one sequence, its substitutions at three positions, and two unrelated ones (its reverse, and a neighbour
    of that), with skewed weights."""
    near = [base] + [base[:at] + bytes([x]) + base[at + 1:] for at in (0, len(base) // 2, len(base) - 1) for x in b"ACGT" if x != base[at]]
    other = base[::-1]
    pool = near + [other, other[:-1] + bytes([b"ACGT"[(b"ACGT".index(other[-1]) + 1) % 4]])]
    assert len(set(pool)) == len(pool)
    weights = [30] + [1, 2, 1, 1, 5, 1, 1, 1, 3] + [10, 6]
    return rng.choices(pool, weights, k=n)


def _checked(s, res, col, held, members):
    pairs, groups = _same(res, held, members)
    exp = _restated(pairs)
    for rule in RULES:
        _same_collapse(col[rule], pairs, groups, exp, rule, res["max_len"])
    assert col[ANY]["nabsorbed"] >= col[DIRECTIONAL]["nabsorbed"] > 0
    return pairs, groups


def test_groups_from_a_demultiplex_hold(gpu, capi, fl):
    """The group of a line is its barcode (pattern + 1), the members are the guides: a sample's erroneous guides fold into their neighbours
    within the sample only."""
    from seeq_amd import device as dev
    rng = random.Random(6)
    codes = [_kmer(rng.getrandbits(32), 16) for _ in range(4)]
    which = [rng.randrange(4) for _ in range(400)]
    guides = _members_around(rng, 400)
    lines = [b"TT" + codes[k] + b"CAAC" + FA.encode() + g + FB.encode() + b"GT" for k, g in zip(which, guides)]
    t = _cuda(_text(lines))
    ps = [dev.Pattern(c.decode(), 0) for c in codes]
    held = [(i + 1, k + 1) for i, k in enumerate(which)]
    members = [(i + 1, g) for i, g in enumerate(guides)]
    sc = dev.Scanner()

    def call(s):
        rec = s.demux_tensor(ps, t)["records"]
        assert rec["line"].tolist() == [ln for ln, _ in held] and [int(p) + 1 for p in rec["pattern"]] == [k for _, k in held] and rec["margin"].min() > 0
        s.tally_hold(source="demux")
        _cut(s, fl["A"], fl["B"], t, members, "guides")
        res = s.tally_grouped(t)
        return res, {rule: s.tally_collapse(NAMES[rule]) for rule in RULES}

    def check(s, got):
        pairs, groups = _checked(s, got[0], got[1], held, members)
        assert [g[0] for g in groups] == [1, 2, 3, 4]
    _go(sc, "groups from a demux hold", call, check)
    sc.close()
    for p in ps:
        p.close()


def test_groups_from_a_library_hold(gpu, capi, fl):
    """tally_hold_library: the group of a line is its guide's library id, erroneous guides corrected into it; the UMIs collapse within it."""
    from seeq_amd import device as dev
    rng = random.Random(7)
    library = [b"ACGTTGCAAGCTACGTTGCA", b"TTGACCGATCAGGATTACAT", b"GGATCCGATTTACGGCATAC"]
    spec = []
    for _ in range(500):
        k = rng.randrange(3)
        g = library[k]
        if rng.random() < 0.2:                              # one substitution: corrected to the same id
            at = rng.randrange(20)
            g = g[:at] + bytes([rng.choice([x for x in b"ACGT" if x != g[at]])]) + g[at + 1:]
        spec.append((k, g, _members_around(rng, 1, b"TTGACCGATCAG")[0]))
    lines = _reads([(g, u) for _, g, u in spec], 7)
    t = _cuda(_text(lines))
    guides = [(i + 1, g) for i, (_, g, _) in enumerate(spec)]
    umis = [(i + 1, u) for i, (_, _, u) in enumerate(spec)]
    held = [(i + 1, k + 1) for i, (k, _, _) in enumerate(spec)]
    sc = dev.Scanner()

    def call(s):
        s.set_library(library, max_mismatch=1)
        _cut(s, fl["A"], fl["B"], t, guides, "guides")
        hold = s.tally_hold_library(t)
        _cut(s, fl["C"], fl["D"], t, umis, "UMIs")
        res = s.tally_grouped(t)
        return hold, res, {rule: s.tally_collapse(NAMES[rule]) for rule in RULES}

    def check(s, got):
        hold, res, col = got
        assert hold["nassigned"] == 500 and hold["ncorrected"] > 50
        pairs, groups = _checked(s, res, col, held, umis)
        assert [g[0] for g in groups] == [1, 2, 3]
    _go(sc, "groups from a library hold", call, check)
    sc.close()


def test_hits_as_members_under_sq_all(gpu, capi, fl):
    """Members from source "hits": a plain SQ_ALL scan whose lines carry 0 - 3 matches that differ in four bytes -- neighbours among them."""
    from seeq_amd import device as dev
    rng = random.Random(8)
    gs = [_kmer(rng.getrandbits(40), 20) for _ in range(3)]
    lines, guides, members = [], [], []
    for i in range(500):
        g = rng.choice(gs + [None])
        hits = [_hit(_kmer(rng.choice([0, 0, 0, 1, 2, 3, 4, 16, 17, 64, 255]), 4)) for _ in range(rng.choice([0, 1, 1, 2, 3]))]
        lines.append((b"AC" + FA.encode() + g + FB.encode() if g is not None else b"TTG") + b"".join(b"TTA" + h for h in hits) + b"CA")
        if g is not None:
            guides.append((i + 1, g))
        members += [(i + 1, h) for h in hits]
    buf = _text(lines)
    offs = _line_offsets(buf)
    t = _cuda(buf)
    held, _ = _held_of(guides)
    sc = dev.Scanner()

    def call(s):
        _cut(s, fl["A"], fl["B"], t, guides, "guides")
        s.tally_hold(t)
        cnt = s.scan_tensor(fl["HIT"], t, SQ_ALL, dev.WANT_RECORDS)
        rec = s.records(cnt["nrecords"]).tolist()
        assert [(r[0], buf[offs[r[0]] + r[1]:offs[r[0]] + r[2]]) for r in rec] == members
        res = s.tally_grouped(t, source="hits")
        return res, {rule: s.tally_collapse(NAMES[rule]) for rule in RULES}, rec

    def check(s, got):
        res, col, rec = got
        _checked(s, res, col, held, members)
        assert res["max_len"] == 20 and s.records(len(rec)).tolist() == rec      # the record arrays are what they were
    _go(sc, "hits as members", call, check)
    sc.close()


# ---- context state ----
def _view(ptr, nbytes):
    """nbytes at a device address, read by torch."""
    import torch

    class View:
        __cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2, "strides": None}
    return torch.as_tensor(View(), device="cuda").cpu().numpy().tobytes()


def test_the_collapse_leaves_everything_else_alone_and_a_second_one_replaces_the_first(gpu, capi, fl):
    """Across a collapse: the pair and group tables, the plain tally's table, the inserts result (records, offsets, text) are
    byte-identical, and the held column is what it was -- a second grouped call gives the same tables.  The other rule then replaces the
    first result; windows of both copies at first > 0; the result left on the device and read through the pointers."""
    from seeq_amd import device as dev
    rng = random.Random(9)
    spec = _spec_of(_crowded(rng, T + 77, G3))
    sc = dev.Scanner()
    sc.set_profiling(True)
    out, t = _collapsed(sc, fl, spec, "state across a collapse")
    n, np_, ng = len(spec), len(out["pairs"]), len(out["groups"])
    plain = sc.tally(t, copy=False)

    def snapshot():
        return (sc.tally_pairs_table(np_).tobytes(), sc.tally_groups_table(ng).tobytes(), sc.tally_table(plain["ndistinct"]).tobytes(),
                sc.insert_text(t).cpu().numpy().tobytes(), sc.insert_records(n).tobytes(), sc.insert_offsets(n).tobytes())
    before = snapshot()
    first = sc.tally_collapse("directional")
    assert sc.last_tally_collapse_ms() > 0
    assert snapshot() == before
    _same_collapse(first, out["pairs"], out["groups"], out["exp"], DIRECTIONAL, 6)
    # a second collapse with the other rule replaces the first
    lazy = sc.tally_collapse("any", copy=False)
    assert "parent" not in lazy and "groups" not in lazy and lazy == {k: out["col"][ANY][k] for k in COUNTS}
    assert snapshot() == before
    second = dict(lazy, parent=sc.tally_parents_table(np_), groups=sc.tally_collapse_table(ng))
    _same_collapse(second, out["pairs"], out["groups"], out["exp"], ANY, 6)
    assert second["parent"].tobytes() != first["parent"].tobytes()
    # left on the device, read through the pointers; windows of both copies
    assert sc.tally_parents_device_ptr() and sc.tally_collapse_device_ptr()
    assert _view(sc.tally_parents_device_ptr(), 4 * np_) == second["parent"].tobytes()
    assert _view(sc.tally_collapse_device_ptr(), 16 * ng) == second["groups"].tobytes()
    assert sc.tally_parents_table(100, first=T - 50).tobytes() == second["parent"].tobytes()[4 * (T - 50):4 * (T + 50)]
    assert sc.tally_collapse_table(2, first=1).tobytes() == second["groups"].tobytes()[16:48]
    assert len(sc.tally_parents_table(0, first=np_)) == 0 and len(sc.tally_collapse_table(0, first=ng)) == 0
    for bad in (lambda: sc.tally_parents_table(1, first=np_), lambda: sc.tally_collapse_table(2, first=ng - 1)):
        with pytest.raises(dev.SeeqDeviceError):
            bad()
    # the held column is what it was: the grouped call again gives the same tables (and clears the collapse: below)
    again = sc.tally_grouped(t)
    assert again["pairs"].tobytes() == before[0] and again["groups"].tobytes() == before[1]
    with pytest.raises(dev.SeeqDeviceError):
        sc.fetch()                                          # an inserts call leaves nothing to fetch, and the collapse does not change that
    sc.close()


def test_a_new_grouped_call_clears_the_result_and_the_next_collapse_answers_for_it(gpu, capi, fl):
    from seeq_amd import device as dev
    sc = dev.Scanner()
    out, t = _collapsed(sc, fl, _spec_of(_crowded(random.Random(10), 300, G3)), "the first tables")
    assert len(sc.tally_parents_table(5)) == 5 and len(sc.tally_collapse_table(1)) == 1
    # the same context, other reads: until the collapse is asked for again there is no result
    spec = _spec_of(_crowded(random.Random(11), 200, G3[1:], ulen=5))
    lines = _reads(spec, 11)
    t2 = _cuda(_text(lines))
    guides, umis = [(i + 1, g) for i, (g, _) in enumerate(spec)], [(i + 1, u) for i, (_, u) in enumerate(spec)]
    _cut(sc, fl["A"], fl["B"], t2, guides, "guides")
    sc.tally_hold(t2)
    _cut(sc, fl["C"], fl["D"], t2, umis, "UMIs")
    res = sc.tally_grouped(t2)
    for bad in (lambda: sc.tally_parents_table(1), lambda: sc.tally_collapse_table(1)):
        with pytest.raises(dev.SeeqDeviceError):
            bad()
    assert len(sc.tally_parents_table(0)) == 0 and len(sc.tally_collapse_table(0)) == 0
    pairs, groups = _same(res, _held_of(guides)[0], umis)
    exp = _restated(pairs)
    for rule in RULES:
        _same_collapse(sc.tally_collapse(NAMES[rule]), pairs, groups, exp, rule, 5)
    assert len(pairs) == 200 != len(out["pairs"])
    # a grouped call that pairs nothing is a completed one: its collapse is the empty result
    spec0 = [(None, b"ACGTAC")] * 20
    t0 = _cuda(_text(_reads(spec0, 12)))
    _cut(sc, fl["A"], fl["B"], t0, [], "no guides")
    sc.tally_hold(t0)
    _cut(sc, fl["C"], fl["D"], t0, [(i + 1, u) for i, (_, u) in enumerate(spec0)], "UMIs")
    assert sc.tally_grouped(t0)["npairs"] == 0
    empty = sc.tally_collapse("any")
    assert {k: empty[k] for k in COUNTS} == dict(npairs=0, ngroups=0, nroots=0, nabsorbed=0, absorbed_reads=0, rule=ANY, max_len=0)
    assert len(empty["parent"]) == 0 and len(empty["groups"]) == 0
    sc.close()


def test_no_collapse_without_a_grouped_call(gpu, capi, fl):
    """A fresh context, and one whose grouped call failed, refuse (EINVAL); the message names the missing call."""
    from seeq_amd import device as dev
    sc = dev.Scanner()
    with pytest.raises(dev.SeeqDeviceError):
        sc.tally_collapse()
    assert "grouped call" in capi.error_text()
    with pytest.raises(dev.SeeqDeviceError):
        sc.tally_collapse("any", copy=False)
    sc.close()
