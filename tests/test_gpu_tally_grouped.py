"""GPU (-m gpu): the grouped tally (seeqdevScanTallyHold / seeqdevScanTallyGrouped; seeq_tally_group.h: hold, pair pack, the two-word
radix sort, run lengths, both tables, all on the device) against the rule restated in Python (test_tally_group_host.py) over what was
PLANTED.  Reads are built as prefix + flank A + guide + flank B + spacer + flank C + UMI + flank D + suffix, the flanks searched at
distance 0, and every case first asserts that each inserts call (scan, demultiplex) found exactly what was planted: a vacuous case
fails."""
import ctypes as C
import errno
import os
import random
import re

import pytest

from conftest import ROOT
from oracle.pyoracle import SQ_ALL, SQ_BEST
from test_gpu_inserts import _fastq
from test_gpu_strands import _line_offsets, _step
from test_tally_group_host import py_pairs
from test_tally_host import FOREIGN, LONG, OK, py_key

pytestmark = pytest.mark.gpu
T = int(re.search(r"#define\s+SEEQ_TALLY_TILE\s+(\d+)", open(os.path.join(ROOT, "seeq_amd", "csrc", "seeq_tally.h")).read()).group(1))
FA, FB = "GATGTAGCGCGATTAGCCTG", "TTCACTGGAGTTGTCCCAAT"      # around the guide
FC, FD = "CCGATAGGCTTAACGGTCAC", "AGGTCCATTGCAGTACGGAT"      # around the UMI
HIT = "CATGCATGNNNNGTACGTAC"                                # a pattern whose matches differ in four bytes (distance 0, SQ_ALL)
GROUPED = ("nspans", "npaired", "nlong", "nforeign", "nungrouped", "npairs", "ngroups", "max_len", "passes")

_FAULT = []


@pytest.fixture(autouse=True)
def _nothing_after_a_device_fault():
    """A device fault ends the module: what comes after it fails here, before it starts anything on the device."""
    if _FAULT:
        pytest.fail("a device fault earlier in this module (%s): nothing more is started on the device" % _FAULT[0])
    yield


def _go(sc, what, call, check, fresh=None):
    """_step of test_gpu_strands.py; a device fault (it raises the SeeqDeviceError untouched) is remembered for the rest of the module."""
    from seeq_amd import device as dev
    try:
        _step(sc, what, call, check, fresh)
    except dev.SeeqDeviceError as e:
        _FAULT.append("%s: %s" % (what, e))
        raise


@pytest.fixture(scope="module")
def fl(gpu):
    from seeq_amd import device as dev
    ps = dict(A=dev.Pattern(FA, 0), B=dev.Pattern(FB, 0), C=dev.Pattern(FC, 0), D=dev.Pattern(FD, 0), HIT=dev.Pattern(HIT, 0))
    yield ps
    for p in ps.values():
        p.close()


def _cuda(buf):
    import torch
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


def _hit(four):
    return b"CATGCATG" + four + b"GTACGTAC"


# ---- reads ----
def _reads(spec, seed=1):
    """spec: per line (guide, umi), bytes or None for a line without that part -> the lines (bytes)."""
    rng = random.Random(seed)
    bases = lambda m: bytes(rng.choice(b"ACGT") for _ in range(m))      # noqa: E731
    lines = []
    for guide, umi in spec:
        parts = [bases(rng.randrange(6))]
        if guide is not None:
            parts += [FA.encode(), guide, FB.encode()]
        parts.append(bases(rng.randrange(3, 8)))
        if umi is not None:
            parts += [FC.encode(), umi, FD.encode()]
        parts.append(bases(rng.randrange(6)))
        lines.append(b"".join(parts))
    return lines


def _text(lines):
    return b"\n".join(lines) + b"\n"


def _held_of(column):
    """[(line, bytes)] -> the held column [(line, key or 0)] and the hold's expected counts."""
    held, nlong, nforeign, longest = [], 0, 0, 0
    for line, seq in column:
        kind, key = py_key(seq)
        held.append((line, key))
        nlong += kind == LONG
        nforeign += kind == FOREIGN
        if kind == OK:
            longest = max(longest, len(seq))
    cnt = dict(nspans=len(column), nheld=len(column) - nlong - nforeign, nlong=nlong, nforeign=nforeign, nambiguous=0, max_len=longest,
               key_bits=max([k.bit_length() for _, k in held], default=0))
    return held, cnt


def _same(res, held, members):
    """A tally_grouped() result (copy=True) against the rule over the held column [(line, key)] and the members [(line, bytes)]."""
    counts, pairs, groups = py_pairs(held, members)
    exp = dict(nspans=len(members), npaired=counts[0], nlong=counts[1], nforeign=counts[2], nungrouped=counts[3], npairs=len(pairs), ngroups=len(groups),
               max_len=counts[5], passes=counts[7])
    assert {k: res[k] for k in GROUPED} == exp
    assert res["nspans"] == res["npaired"] + res["nlong"] + res["nforeign"] + res["nungrouped"]
    got = [tuple(int(x) for x in r) for r in res["pairs"]]
    if got != pairs:
        bad = next((i for i, (a, b) in enumerate(zip(got, pairs)) if a != b), min(len(got), len(pairs)))
        raise AssertionError("pair tables differ (%d vs %d entries; first difference at %d: %s vs %s)" % (len(got), len(pairs), bad, got[bad:bad + 1], pairs[bad:bad + 1]))
    assert [tuple(int(x) for x in r) for r in res["groups"]] == groups
    assert int(res["pairs"]["count"].sum()) == int(res["groups"]["count"].sum()) == res["npaired"]
    assert int(res["groups"]["ndistinct"].sum()) == res["npairs"]
    return pairs, groups


def _cut(s, left, right, t, expected, what, options=SQ_BEST):
    """An inserts call that must find exactly `expected` = [(line, bytes)]."""
    res = s.inserts_tensor(left, right, t, options, copy=False)
    assert res["ninserts"] == len(expected), (what, res)
    text = s.insert_text(t).cpu().numpy().tobytes().split(b"\n")[:-1]
    assert text == [b for _, b in expected], what
    assert s.insert_records(len(expected))["line"].tolist() == [ln for ln, _ in expected], what


def _planted(sc, fl, spec, what, seed=1, fastq=False, between=None):
    """inserts(A, B), hold, inserts(C, D), grouped over reads that carry `spec`; every step checked against what was planted."""
    from seeq_amd import device as dev
    lines = _reads(spec, seed)
    buf = _fastq([ln.decode() for ln in lines], seed + 1, FA)[0] if fastq else _text(lines)
    opt = SQ_BEST | (dev.SEEQDEV_FASTQ if fastq else 0)
    t = _cuda(buf)
    guides = [(i + 1, g) for i, (g, _) in enumerate(spec) if g is not None]
    umis = [(i + 1, u) for i, (_, u) in enumerate(spec) if u is not None]
    held, hcnt = _held_of(guides)

    def call(s):
        _cut(s, fl["A"], fl["B"], t, guides, what + ": guides", opt)
        hold = s.tally_hold(t)
        if between:
            between(s, t)
        _cut(s, fl["C"], fl["D"], t, umis, what + ": UMIs", opt)
        return hold, s.tally_grouped(t)
    got = {}

    def check(s, pair):
        hold, res = pair
        assert hold == hcnt
        got["tables"] = _same(res, held, umis)
        got["res"] = res
    _go(sc, what, call, check)
    return got["res"], got["tables"], t


def _kmer(i, m):
    return bytes(b"ACTG"[(i >> (2 * (m - 1 - j))) & 3] for j in range(m))


def _random_spec(rng, n, nguides=5, numis=9, glen=20, ulen=12):
    gs = [_kmer(rng.getrandbits(2 * glen), glen) for _ in range(nguides)]
    us = [_kmer(rng.getrandbits(2 * ulen), ulen) for _ in range(numis)]
    return [(rng.choice(gs), rng.choice(us)) for _ in range(n)]


# ---- shapes ----
@pytest.mark.parametrize("n", [0, 1, T - 1, T, T + 1])
def test_member_counts(gpu, capi, fl, n):
    """Around the tile T; no member at all launches nothing and gives two empty tables.  Three lines carry a guide and no UMI."""
    from seeq_amd import device as dev
    rng = random.Random(n)
    spec = _random_spec(rng, n) + [(b"ACGTACGTACGTACGTACGT", None)] * 3
    rng.shuffle(spec)
    sc = dev.Scanner()
    res, (pairs, groups), _ = _planted(sc, fl, spec, "%d members" % n, seed=n)
    assert res["nspans"] == res["npaired"] == n and (n == 0) == (res["npairs"] == 0)
    if n == 0:
        assert res["passes"] == 0 and len(res["pairs"]) == 0 and len(res["groups"]) == 0
    else:
        assert res["passes"] == 4 + 6                       # 12-base members (25 bits), 20-base groups (41 bits)
    sc.close()


def test_heads_at_and_runs_across_tile_boundaries(gpu, capi, fl):
    """4 T + 1 members.  Exactly T of them do not pair (long, foreign, ungrouped), so the (0, 0) items fill sorted indices 0 .. T - 1 and
    the first group head (a pair head too) falls on index T: its predecessor lies in another tile.  The first pair occurs T + T / 2 times:
    its run crosses index 2 T.  The last group begins at index 3 T exactly."""
    from seeq_amd import device as dev
    rng = random.Random(77)
    g1, g2, g3 = b"A" * 20, b"C" * 20, b"G" * 20           # keys ascending: A < C < T < G
    spec = [(g1, b"A" * 12)] * (T + T // 2) + [(g1, b"ACGTACGTACGT")] * (T // 4) + [(g2, _kmer(i, 12)) for i in range(T // 4)] + [(g3, b"TTTTGGGGCCCC")] * (T + 1)
    spec += [(None, b"ACGTACGTACGT")] * (T // 2) + [(g1, b"ACGTNCGTACGT")] * (T // 4) + [(g2, b"A" * 32)] * (T // 4)
    assert len(spec) == 4 * T + 1
    rng.shuffle(spec)
    sc = dev.Scanner()
    res, (pairs, groups), _ = _planted(sc, fl, spec, "heads on tile boundaries")
    assert (res["nungrouped"], res["nforeign"], res["nlong"]) == (T // 2, T // 4, T // 4) and res["nspans"] - res["npaired"] == T
    assert pairs[0] == (py_key(g1)[1], py_key(b"A" * 12)[1], T + T // 2)      # sorted indices T .. 2 T + T / 2
    assert [g[1] for g in groups] == [T + T // 2 + T // 4, T // 4, T + 1] and groups[2][2] == 2 + T // 4
    sc.close()


# ---- cases ----
def _edge_spec(case):
    rng = random.Random(len(case))
    if case == "one_word_differs":                          # all four combinations of two guides and two UMIs: neighbours differ in one word only
        return [(rng.choice([b"ACGTACGTACGTACGTACGT", b"ACGTACGTACGTACGTACGA"]), rng.choice([b"TTGACCGATCAG", b"TTGACCGATCAT"])) for _ in range(2 * T + 3)]
    if case == "member_digits_then_group_digits":           # many members per group, groups that differ in their highest digit only
        gs = [_kmer(i, 3) + b"GATTACAGATTACAGAT" for i in range(16)]
        return [(rng.choice(gs), _kmer(rng.randrange(256), 4)) for _ in range(3 * T + 5)]
    if case == "31_G":                                      # bits 0 .. 62 set in both words: 8 + 8 passes
        return [(rng.choice([b"G" * 31, b"A" * 31, b"G" * 30]), rng.choice([b"G" * 31, b"T" * 31, b"G"])) for _ in range(T + 9)]
    if case == "empty":                                     # the empty insert as member and as group: key 1
        return [(rng.choice([b"", b"A", b"ACGT"]), rng.choice([b"", b"A", b"ACGTAC"])) for _ in range(T + 9)]
    assert case == "lower_case_and_u"
    return [(rng.choice([b"ACGTTGCAAGCT", b"acguugcaagcu", b"ACGUUGcaAGCT", b"ACGTTGCAAGCA"]), rng.choice([b"TTGACC", b"uugacc", b"TtGaCc", b"GGGGGG"]))
            for _ in range(T + 9)]


@pytest.mark.parametrize("case", ["one_word_differs", "member_digits_then_group_digits", "31_G", "empty", "lower_case_and_u"])
def test_stability_and_key_edges(gpu, capi, fl, case):
    from seeq_amd import device as dev
    spec = _edge_spec(case)
    sc = dev.Scanner()
    res, (pairs, groups), _ = _planted(sc, fl, spec, case)
    if case == "one_word_differs":
        assert (res["npairs"], res["ngroups"]) == (4, 2) and [g[3] for g in groups] == [2, 2]
        assert pairs[0][0] == pairs[1][0] and pairs[0][1] == pairs[2][1] and pairs[0][1] != pairs[1][1] and pairs[0][0] != pairs[2][0]
    elif case == "member_digits_then_group_digits":
        assert res["ngroups"] == 16 and res["npairs"] > 2000 and res["passes"] == 2 + 6
        assert len({g[0] & ((1 << 34) - 1) for g in groups}) == 1      # the groups differ in bits 34 - 39 only
    elif case == "31_G":
        assert res["passes"] == 16 and res["max_len"] == 31 and (res["npairs"], res["ngroups"]) == (9, 3)
        assert pairs[-1][:2] == ((1 << 63) - 1, (1 << 63) - 1)
    elif case == "empty":
        assert pairs[0][:2] == (1, 1) and groups[0][0] == 1 and (res["npairs"], res["ngroups"]) == (9, 3)
        assert [tuple(int(x) for x in r) for r in dev.tally_members(res, 1)] == pairs[:3]
    else:
        assert (res["npairs"], res["ngroups"]) == (4, 2) and dev.tally_key("acguugcaagcu") == groups[1][0] == dev.tally_key("ACGTTGCAAGCT")
    sc.close()


def test_members_and_lines_that_do_not_pair(gpu, capi, fl):
    """Planted among ordinary reads, one kind each: a member that is long (17), foreign (13), long and foreign (5: long), on a line without
    a guide part (19: ungrouped), on a line whose guide is long (11) or foreign (7: held without a key, the member ungrouped); and 23
    lines with a guide and no UMI part (held lines with no member).  A long member on an ungrouped line counts as long."""
    from seeq_amd import device as dev
    rng = random.Random(9)
    g = b"ACGTTGCAAGCTACGTTGCA"
    spec = _random_spec(rng, T, nguides=3, numis=4)
    spec += [(g, _kmer(rng.getrandbits(64), 32))] * 17 + [(g, b"ACGTNCGTACGT")] * 13 + [(g, b"ACGTNCGTACGT" * 3)] * 5
    spec += [(None, b"ACGTACGTACGT")] * 19 + [(b"ACGT" * 8, b"ACGTACGTACGT")] * 11 + [(b"ACGNACGT", b"ACGTACGTACGT")] * 7 + [(g, None)] * 23
    spec += [(None, b"A" * 40)] * 3
    rng.shuffle(spec)
    sc = dev.Scanner()
    res, _, _ = _planted(sc, fl, spec, "members that do not pair")
    assert (res["nlong"], res["nforeign"], res["nungrouped"]) == (17 + 5 + 3, 13, 19 + 11 + 7)
    sc.close()


def test_hits_as_members_under_sq_all(gpu, capi, fl):
    """Members from source "hits": a plain SQ_ALL scan whose lines carry 0 - 3 matches; each record is a pair of its own."""
    from seeq_amd import device as dev
    rng = random.Random(12)
    gs = [_kmer(rng.getrandbits(40), 20) for _ in range(4)]
    lines, guides, members = [], [], []
    for i in range(T + 300):
        g = rng.choice(gs + [None])
        hits = [_hit(_kmer(rng.randrange(8), 4)) for _ in range(rng.choice([0, 1, 1, 2, 3]))]
        lines.append((b"AC" + FA.encode() + g + FB.encode() if g is not None else b"TTG") + b"".join(b"TTA" + h for h in hits) + b"CA")
        if g is not None:
            guides.append((i + 1, g))
        members += [(i + 1, h) for h in hits]
    buf = _text(lines)
    offs = _line_offsets(buf)
    t = _cuda(buf)
    held, hcnt = _held_of(guides)
    sc = dev.Scanner()

    def call(s):
        _cut(s, fl["A"], fl["B"], t, guides, "guides")
        hold = s.tally_hold(t)
        cnt = s.scan_tensor(fl["HIT"], t, SQ_ALL, dev.WANT_RECORDS)
        rec = s.records(cnt["nrecords"]).tolist()
        assert [(r[0], buf[offs[r[0]] + r[1]:offs[r[0]] + r[2]]) for r in rec] == members
        return hold, s.tally_grouped(t, source="hits"), rec

    def check(s, got):
        hold, res, rec = got
        assert hold == hcnt
        _same(res, held, members)
        assert res["nungrouped"] > 50 and s.records(len(rec)).tolist() == rec      # the record arrays are what they were
    _go(sc, "hits as members", call, check)
    assert len(members) > T and max(sum(1 for ln, _ in members if ln == k) for k in range(1, 40)) >= 2
    sc.close()


def test_hits_as_the_held_column_the_first_record_of_a_line_decides(gpu, capi, fl):
    from seeq_amd import device as dev
    rng = random.Random(13)
    us = [_kmer(rng.getrandbits(24), 12) for _ in range(6)]
    lines, column, umis = [], [], []
    for i in range(T + 200):
        hits = [_hit(_kmer(rng.randrange(8), 4)) for _ in range(rng.choice([0, 1, 2, 3]))]
        u = rng.choice(us + [None])
        lines.append(b"GT" + b"".join(h + b"TTA" for h in hits) + (FC.encode() + u + FD.encode() if u is not None else b"") + b"AC")
        column += [(i + 1, h) for h in hits]
        if u is not None:
            umis.append((i + 1, u))
    buf = _text(lines)
    offs = _line_offsets(buf)
    t = _cuda(buf)
    held, hcnt = _held_of(column)
    sc = dev.Scanner()

    def call(s):
        cnt = s.scan_tensor(fl["HIT"], t, SQ_ALL, dev.WANT_RECORDS)
        rec = s.records(cnt["nrecords"]).tolist()
        assert [(r[0], buf[offs[r[0]] + r[1]:offs[r[0]] + r[2]]) for r in rec] == column
        hold = s.tally_hold(t, source="hits")
        _cut(s, fl["C"], fl["D"], t, umis, "UMIs")
        return hold, s.tally_grouped(t)

    def check(s, got):
        hold, res = got
        assert hold == hcnt
        _same(res, held, umis)
    _go(sc, "hits as the held column", call, check)
    first = {}
    for ln, h in column:
        first.setdefault(ln, h)
    assert sum(1 for ln, h in column if first[ln] != h) > 100      # later records of a line with another key: they must not decide
    sc.close()


def test_demux_as_the_held_column(gpu, capi, fl):
    """A set of 255 barcodes (the highest index, 254, is group 255), reads planted for it and for others, lines with two barcodes of the
    set (ambiguous: margin 0, held without a key, the member ungrouped), lines with none.  The pair table is the host's count per
    (pattern, guide)."""
    import collections
    from seeq_amd import device as dev
    rng = random.Random(14)
    codes = []
    while len(codes) < 255:
        c = _kmer(rng.getrandbits(32), 16)
        if c not in codes:
            codes.append(c)
    gs = [_kmer(rng.getrandbits(40), 20) for _ in range(5)]
    use = [254, 254, 254, 0, 1, 127, 200, 253]
    lines, assigned, guides, ambiguous = [], {}, [], 0
    for i in range(T + 500):
        kind = rng.choice(["one"] * 8 + ["two", "none"])
        g = rng.choice(gs)
        head = b"TT"
        if kind == "one":
            k = rng.choice(use)
            head += codes[k] + b"CA"
            assigned[i + 1] = k + 1
        elif kind == "two":
            a, b = rng.sample(use[2:], 2)
            head += codes[a] + b"CA" + codes[b]
            assigned[i + 1] = 0
            ambiguous += 1
        lines.append(head + b"AC" + FA.encode() + g + FB.encode() + b"GT")
        guides.append((i + 1, g))
    buf = _text(lines)
    t = _cuda(buf)
    ps = [dev.Pattern(c.decode(), 0) for c in codes]
    held = sorted(assigned.items())
    sc = dev.Scanner()

    def call(s):
        dm = s.demux_tensor(ps, t)
        rec = dm["records"]
        assert rec["line"].tolist() == [ln for ln, _ in held]
        assert [(int(p) + 1) if m else 0 for p, m in zip(rec["pattern"], rec["margin"])] == [k for _, k in held]
        hold = s.tally_hold(source="demux")
        _cut(s, fl["A"], fl["B"], t, guides, "guides")
        return hold, s.tally_grouped(t)

    def check(s, got):
        hold, res = got
        assert hold == dict(nspans=len(held), nheld=len(held) - ambiguous, nlong=0, nforeign=0, nambiguous=ambiguous, max_len=0, key_bits=8)
        pairs, groups = _same(res, held, guides)
        by = collections.Counter((assigned[ln], py_key(g)[1]) for ln, g in guides if assigned.get(ln))
        assert pairs == [(a, b, by[a, b]) for a, b in sorted(by)]
        assert res["passes"] == 6 + 1 and groups[-1][0] == 255 and groups[-1][1] > 100 and res["nungrouped"] > ambiguous > 50
    _go(sc, "demux as the held column", call, check)
    # a later scan invalidates the demux records for a hold; the held column itself stays
    sc.scan_tensor(fl["A"], t, SQ_BEST, dev.WANT_RECORDS)
    with pytest.raises(dev.SeeqDeviceError):
        sc.tally_hold(source="demux")
    assert "demux" in capi.error_text()
    sc.close()
    for p in ps:
        p.close()


def test_fastq_in_both_calls(gpu, capi, fl):
    """SEEQDEV_FASTQ over four-line records: both calls number by record, and the quality lines (every third opens with flank A) give nothing."""
    from seeq_amd import device as dev
    rng = random.Random(15)
    spec = _random_spec(rng, T + 50) + [(None, b"ACGTACGTACGT")] * 5 + [(b"ACGTACGTACGTACGTACGT", None)] * 5
    rng.shuffle(spec)
    sc = dev.Scanner()
    res, _, _ = _planted(sc, fl, spec, "FASTQ", seed=15, fastq=True)
    assert res["npaired"] == T + 50 and res["nungrouped"] == 5
    sc.close()


def test_tables_left_on_the_device_and_copied_in_windows(gpu, capi, fl):
    from seeq_amd import device as dev
    rng = random.Random(16)
    spec = _random_spec(rng, 2 * T + 3, nguides=40, numis=30)
    sc = dev.Scanner()
    sc.set_profiling(True)
    res, (pairs, groups), t = _planted(sc, fl, spec, "copy=False")
    assert sc.last_tally_grouped_ms() > 0
    lazy = sc.tally_grouped(t, copy=False)
    assert "pairs" not in lazy and lazy == {k: res[k] for k in GROUPED}
    assert sc.tally_pairs_device_ptr() and sc.tally_groups_device_ptr()
    assert sc.tally_pairs_table(lazy["npairs"]).tobytes() == res["pairs"].tobytes()
    assert sc.tally_groups_table(lazy["ngroups"]).tobytes() == res["groups"].tobytes()
    assert sc.tally_pairs_table(10, first=5).tobytes() == res["pairs"].tobytes()[120:360]
    assert sc.tally_groups_table(7, first=30).tobytes() == res["groups"].tobytes()[720:888]
    assert len(sc.tally_pairs_table(0, first=lazy["npairs"])) == 0 and len(sc.tally_groups_table(0, first=lazy["ngroups"])) == 0
    for bad in (lambda: sc.tally_pairs_table(1, first=lazy["npairs"]), lambda: sc.tally_groups_table(2, first=lazy["ngroups"] - 1)):
        with pytest.raises(dev.SeeqDeviceError):
            bad()
    for gkey, cnt, first, nd in groups[:5]:
        assert [tuple(int(x) for x in r) for r in dev.tally_members(res, gkey)] == pairs[first:first + nd]
    sc.close()


# ---- context state ----
def test_the_held_column_survives_and_the_grouped_call_leaves_the_rest_alone(gpu, capi, fl):
    """Between hold and grouped call: a plain scan, an inserts call, a plain tally -- the held column is what it was.  Across the grouped
    call: the plain tally's table and the insert text are byte-identical.  A second hold replaces the first."""
    from seeq_amd import device as dev
    rng = random.Random(17)
    spec = _random_spec(rng, T + 77)
    seen = {}

    def between(s, t):
        cnt = s.scan_tensor(fl["D"], t, SQ_BEST, dev.WANT_RECORDS)
        assert cnt["nrecords"] == len(spec)
        s.inserts_tensor(fl["A"], fl["B"], t, SQ_BEST, copy=False)
        assert s.tally(t, copy=False)["ndistinct"] == 5

    sc = dev.Scanner()
    res, (pairs, groups), t = _planted(sc, fl, spec, "state between hold and grouped call", between=between)
    # (the Scanner now holds the UMIs' inserts result) the plain tally of the UMIs, then a grouped call, then the same bytes
    plain = sc.tally(t, copy=False)
    before = (sc.tally_table(plain["ndistinct"]).tobytes(), sc.insert_text(t).cpu().numpy().tobytes(), sc.insert_records(len(spec)).tobytes(),
              sc.insert_offsets(len(spec)).tobytes())
    again = sc.tally_grouped(t)
    assert again["pairs"].tobytes() == res["pairs"].tobytes() and again["groups"].tobytes() == res["groups"].tobytes()
    after = (sc.tally_table(plain["ndistinct"]).tobytes(), sc.insert_text(t).cpu().numpy().tobytes(), sc.insert_records(len(spec)).tobytes(),
             sc.insert_offsets(len(spec)).tobytes())
    assert after == before and plain["ndistinct"] == 9
    with pytest.raises(dev.SeeqDeviceError):
        sc.fetch()                                          # an inserts call leaves nothing to fetch, and neither call changes that
    # a second hold replaces the first: the UMIs held, the guides as members -- the transposed matrix
    hold = sc.tally_hold(t)
    assert hold["nheld"] == len(spec) and hold["max_len"] == 12
    sc.inserts_tensor(fl["A"], fl["B"], t, SQ_BEST, copy=False)
    swapped = sc.tally_grouped(t)
    assert sorted((int(m), int(g), int(c)) for g, m, c in swapped["pairs"]) == pairs and swapped["passes"] == 6 + 4
    sc.close()


def test_a_hold_of_zero_records_is_an_empty_column(gpu, capi, fl):
    from seeq_amd import device as dev
    spec = [(None, b"ACGTACGTACGT")] * 40 + [(None, b"A" * 32)] * 2
    sc = dev.Scanner()
    res, _, t = _planted(sc, fl, spec, "an empty held column")
    assert (res["npairs"], res["ngroups"], res["passes"], res["nungrouped"], res["nlong"]) == (0, 0, 0, 40, 2)
    assert len(res["pairs"]) == 0 and len(res["groups"]) == 0
    sc.close()


def _raw(sc, capi, entry, source, t, nbytes):
    cnt = (capi.seeqdev_tally_hold_counts_t if entry == "seeqdevScanTallyHold" else capi.seeqdev_tally_grouped_counts_t)()
    C.set_errno(0)
    rc = getattr(sc._lib, entry)(sc._h, source, C.c_void_p(t.data_ptr()), nbytes, C.byref(cnt))
    return rc, C.get_errno()


def test_a_span_beyond_the_text_is_an_argument_error_in_both_calls(gpu, capi, fl):
    """nbytes cut short of the last read's insert: EIO from the hold and from the grouped call -- the kernels compare before they load, so
    nothing faults -- and the context then answers the right calls correctly."""
    from seeq_amd import device as dev
    rng = random.Random(18)
    spec = _random_spec(rng, T + 9)
    lines = _reads(spec, 18)
    buf = _text(lines)
    t = _cuda(buf)
    guides = [(i + 1, g) for i, (g, _) in enumerate(spec)]
    umis = [(i + 1, u) for i, (_, u) in enumerate(spec)]
    sc = dev.Scanner()
    INS = capi.SEEQDEV_TALLY_INSERTS

    def end_of_last(s):
        last = s.insert_records(1, first=len(spec) - 1)[0]
        return int(s.insert_offsets(1, first=len(spec) - 1)[0]) + int(last["end"])
    _cut(sc, fl["A"], fl["B"], t, guides, "guides")
    end = end_of_last(sc)
    assert _raw(sc, capi, "seeqdevScanTallyHold", INS, t, end - 1) == (-1, errno.EIO) and "outside" in capi.error_text()
    assert _raw(sc, capi, "seeqdevScanTallyGrouped", INS, t, t.numel()) == (-1, errno.EINVAL)      # a failed hold leaves no column
    assert _raw(sc, capi, "seeqdevScanTallyHold", INS, t, end) == (0, 0)
    _cut(sc, fl["C"], fl["D"], t, umis, "UMIs")
    end = end_of_last(sc)
    assert _raw(sc, capi, "seeqdevScanTallyGrouped", INS, t, end - 1) == (-1, errno.EIO) and "outside" in capi.error_text()
    with pytest.raises(dev.SeeqDeviceError):
        sc.tally_pairs_table(1)                             # a failed grouped call leaves no tables
    assert _raw(sc, capi, "seeqdevScanTallyGrouped", INS, t, end) == (0, 0)
    _same(sc.tally_grouped(t), _held_of(guides)[0], umis)
    sc.close()
