"""GPU (-m gpu): the tally of distinct spans (seeqdevScanTally; seeq_tally.h: pack, radix sort, run lengths, all on the device) against
a Python Counter by the rule of the header -- over the lines of Scanner.insert_text() copied to the host, or over the oracle's records
sliced from the host buffer.  Reads are built as prefix + exact left flank + chosen insert + exact right flank + suffix, and every case
first asserts that the inserts call found exactly the inserts that were planted: a vacuous case fails."""
import collections
import ctypes as C
import errno
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle.pyoracle import SQ_ALL, SQ_BEST, SQ_FIRST
from test_gpu_inserts import BARCODES, PAIRS, Joined, _fastq, _lines
from test_gpu_strands import Expected, _buf, _line_offsets, _step
from test_gpu_strands import _lines as _strand_lines
from test_tally_host import FOREIGN, LONG, OK, py_key

pytestmark = pytest.mark.gpu
T = int(re.search(r"#define\s+SEEQ_TALLY_TILE\s+(\d+)", open(os.path.join(ROOT, "seeq_amd", "csrc", "seeq_tally.h")).read()).group(1))
LEFT, RIGHT = "GATGTAGCGCGATTAGCCTG", "TTCACTGGAGTTGTCCCAAT"      # planted exactly, searched at distance 0
COUNTS = ("nspans", "ntallied", "nlong", "nforeign", "ndistinct", "max_len", "passes")

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
def flanks(gpu):
    from seeq_amd import device as dev
    ps = (dev.Pattern(LEFT, 0), dev.Pattern(RIGHT, 0))
    yield ps
    for p in ps:
        p.close()


# ---- expected values: the rule in Python over spans that the code under test did not cut ----
def _expected(spans):
    """spans: list of bytes -> (counts, keys, counts per key) by the rule of seeq_tally.h."""
    tab = collections.Counter()
    nlong = nforeign = longest = 0
    for s in spans:
        kind, key = py_key(s)
        if kind == OK:
            tab[key] += 1
            longest = max(longest, len(s))
        nlong += kind == LONG
        nforeign += kind == FOREIGN
    keys = sorted(tab)
    ntallied = sum(tab.values())
    cnt = dict(nspans=len(spans), ntallied=ntallied, nlong=nlong, nforeign=nforeign, ndistinct=len(keys), max_len=longest,
               passes=(2 * longest + 1 + 7) // 8 if ntallied else 0)
    return cnt, keys, [tab[k] for k in keys]


def _same(res, spans):
    cnt, keys, counts = _expected(spans)
    assert {k: res[k] for k in COUNTS} == cnt
    assert res["nspans"] == res["ntallied"] + res["nlong"] + res["nforeign"]
    assert res["keys"].dtype == np.uint64 and res["counts"].dtype == np.uint64
    got = list(zip(res["keys"].tolist(), res["counts"].tolist()))
    exp = list(zip(keys, counts))
    if got != exp:
        bad = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
        raise AssertionError("tables differ (%d vs %d entries; first difference at %d: %s vs %s)"
                             % (len(got), len(exp), bad, got[bad:bad + 1], exp[bad:bad + 1]))
    assert int(res["counts"].sum()) == res["ntallied"]


def _reads(inserts, seed=1):
    """One read per insert: 0 - 5 random bases, the left flank, the insert, the right flank, 0 - 5 random bases; then three lines that
    give no insert (random bases, a left flank alone, a right flank alone)."""
    rng = random.Random(seed)
    bases = lambda m: "".join(rng.choice("ACGT") for _ in range(m)).encode()      # noqa: E731
    le, ri = LEFT.encode(), RIGHT.encode()
    lines = [bases(rng.randrange(6)) + le + ins + ri + bases(rng.randrange(6)) for ins in inserts]
    lines += [bases(40), bases(3) + le + bases(9), bases(7) + ri]
    return b"\n".join(lines) + b"\n"


def _cuda(buf):
    import torch
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


def _insert_lines(sc, t):
    """The inserts of the Scanner's last inserts call as the gather (not under test) cuts them, on the host."""
    text = sc.insert_text(t).cpu().numpy().tobytes()
    return text.split(b"\n")[:-1]


def _planted(sc, flanks, inserts, what, seed=1, after=None):
    """The inserts call over reads that carry `inserts`, its result checked against what was planted, then the tally against the rule."""
    buf = _reads(inserts, seed)
    t = _cuda(buf)

    def call(s):
        res = s.inserts_tensor(flanks[0], flanks[1], t, SQ_BEST, copy=False)
        assert res["ninserts"] == len(inserts), (what, res)
        spans = _insert_lines(s, t)
        assert spans == list(inserts), what
        return s.tally(t), spans
    got = {}

    def check(s, pair):
        res, spans = pair
        _same(res, spans)
        got["res"] = res
        if after:
            after(s, t, res)
    _go(sc, what, call, check)
    return got["res"], t


def _random_inserts(rng, n, longest, pool=40):
    some = [bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(0, longest + 1))) for _ in range(pool)]
    some.append(bytes(rng.choice(b"ACGT") for _ in range(longest)))
    out = [rng.choice(some) for _ in range(n)]
    if n:
        out[rng.randrange(n)] = some[-1]
    return out


def _raw_tally(sc, capi, source, t, nbytes=None):
    cnt = capi.seeqdev_tally_counts_t()
    C.set_errno(0)
    rc = sc._lib.seeqdevScanTally(sc._h, source, C.c_void_p(t.data_ptr()) if t is not None else None,
                                  (t.numel() if nbytes is None else nbytes) if t is not None else 0, C.byref(cnt))
    return rc, C.get_errno()


# ---- shapes ----
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3])
def test_span_counts(gpu, capi, flanks, n):
    """Around a wave, around the sort's tile T, more than two tiles; no span at all launches nothing and gives an empty table."""
    from seeq_amd import device as dev
    sc = dev.Scanner()
    res, _ = _planted(sc, flanks, _random_inserts(random.Random(n), n, 12), "%d spans" % n, seed=n)
    assert res["nspans"] == n and (n == 0) == (res["ndistinct"] == 0)
    if n == 0:
        assert res["passes"] == 0 and len(res["keys"]) == 0
    sc.close()


@pytest.mark.parametrize("longest,passes", [(3, 1), (4, 2), (12, 4), (31, 8)])
def test_pass_counts(gpu, capi, flanks, longest, passes):
    """The host runs ceil((2 * max_len + 1) / 8) passes: inserts of at most 3, 4, 12 and 31 bases."""
    from seeq_amd import device as dev
    sc = dev.Scanner()
    res, _ = _planted(sc, flanks, _random_inserts(random.Random(longest), T + 5, longest), "inserts of at most %d bases" % longest, seed=longest)
    assert res["max_len"] == longest and res["passes"] == passes
    sc.close()


def _kmer(i, m):
    return bytes(b"ACTG"[(i >> (2 * (m - 1 - j))) & 3] for j in range(m))


def _edge_inserts(case):
    rng = random.Random(len(case))
    if case == "lowest_digit":                              # 12 bases, the last four vary: keys that differ in bits 0 - 7 only
        return [b"GATTACAG" + _kmer(rng.randrange(256), 4) for _ in range(2 * T + 3)]
    if case == "highest_digit":                             # 15 bases = 31 bits, the first three vary: keys that differ in bits 24 - 29 only
        return [_kmer(rng.randrange(64), 3) + b"GATTACAGATTA" for _ in range(2 * T + 3)]
    if case == "alternating":                               # two keys that differ in every digit, alternating over 3 T spans
        return [b"ACGTTGCAAGCT", b"TGCAACGTTCGA"] * (3 * T // 2)
    if case == "one_key":                                   # one bin larger than a tile
        return [b"ACGTTGCAAGCT"] * (3 * T + 1)
    if case == "all_distinct":
        ks = list(range(2 * T + 3))
        rng.shuffle(ks)
        return [_kmer(k * 2654435761 % (1 << 24), 12) for k in ks]
    assert case == "every_length"                           # lengths 0 .. 31 mixed, empty inserts included
    return [bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(0, 32))) if rng.random() < 0.7 else rng.choice([b"", b"A", b"G" * 31, b"A" * 31])
            for _ in range(2 * T + 3)]


@pytest.mark.parametrize("case", ["lowest_digit", "highest_digit", "alternating", "one_key", "all_distinct", "every_length"])
def test_stability_and_digit_edges(gpu, capi, flanks, case):
    from seeq_amd import device as dev
    inserts = _edge_inserts(case)
    keys = {py_key(s)[1] for s in inserts}
    if case == "lowest_digit":
        assert len(keys) > 200 and len({k >> 8 for k in keys}) == 1
    elif case == "highest_digit":
        assert len(keys) == 64 and len({k & 0xFFFFFF for k in keys}) == 1 and len({k >> 32 for k in keys}) == 1
    elif case == "alternating":
        a, b = sorted(keys)
        assert len(inserts) == 3 * T and all((a >> s) & 255 != (b >> s) & 255 for s in (0, 8, 16))
    elif case == "one_key":
        assert len(keys) == 1 and len(inserts) == 3 * T + 1
    elif case == "all_distinct":
        assert len(keys) == len(inserts)
    else:
        assert {len(s) for s in inserts} == set(range(32)) and inserts.count(b"") > 20
    sc = dev.Scanner()
    res, _ = _planted(sc, flanks, inserts, case)
    assert res["ndistinct"] == len(keys)
    sc.close()


def test_spans_that_are_not_tallied(gpu, capi, flanks):
    """Planted: 37 inserts of 32 bases and 21 of 40 (long), 29 with an N and 11 of 40 bases with an N (long: the length is decided
    first), 43 with a lower-case base (tallied as the base) among ordinary ones."""
    from seeq_amd import device as dev
    rng = random.Random(8)
    mk = lambda m: bytes(rng.choice(b"ACGT") for _ in range(m))      # noqa: E731
    inserts = [mk(rng.randrange(0, 20)) for _ in range(T)] + [b"ACGTTGCAAGCT"] * 50
    inserts += [mk(32) for _ in range(37)] + [mk(40) for _ in range(21)]
    for _ in range(29):
        s = bytearray(mk(rng.randrange(1, 32)))
        s[rng.choice([0, len(s) // 2, len(s) - 1])] = ord("N")
        inserts.append(bytes(s))
    for _ in range(11):
        s = bytearray(mk(40))
        s[rng.randrange(40)] = ord("N")
        inserts.append(bytes(s))
    inserts += [b"ACGTTGcaAGCT"] * 43
    rng.shuffle(inserts)
    sc = dev.Scanner()
    res, _ = _planted(sc, flanks, inserts, "long, foreign and lower-case inserts")
    assert res["nlong"] == 37 + 21 + 11 and res["nforeign"] == 29
    assert res["nspans"] == len(inserts) == res["ntallied"] + res["nlong"] + res["nforeign"]
    assert dev.tally_lookup(res, ["ACGTTGCAAGCT"]).tolist() == [93] and dev.tally_key("ACGTTGcaAGCT") == dev.tally_key("ACGTTGCAAGCT")
    sc.close()


def test_every_level_of_the_offsets_scan_takes_more_than_one_step(gpu, capi):
    """n = 1024 T + T + 3 spans (1 050 627 with T = 1024), reads of 21 bytes.  The offsets scan reads the digit matrix, 256 entries per
    tile, in chunks of 1 024 entries = 4 tiles (level one: more than one chunk from 5 tiles on) and scans the chunk sums in one workgroup,
    256 at a time (level two: a second step from 257 chunks = 1 025 tiles on, n > 1024 T).  The one-workgroup totals of the pack and of
    the run-length pass walk the tiles 256 at a time: more than four steps.  Inserts of 4 bases (9 bits): two passes."""
    import torch
    from seeq_amd import device as dev
    n = 1024 * T + T + 3
    le, ri = b"GATGTAGC", b"TTCACTGG"
    rng = np.random.default_rng(11)
    rows = np.empty((n, len(le) + 4 + len(ri) + 1), dtype=np.uint8)
    rows[:, :len(le)] = np.frombuffer(le, dtype=np.uint8)
    rows[:, len(le):len(le) + 4] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, 4))]
    rows[:, len(le) + 4:-1] = np.frombuffer(ri, dtype=np.uint8)
    rows[:, -1] = 10
    t = torch.from_numpy(rows.reshape(-1)).cuda()
    left, right = dev.Pattern(le.decode(), 0), dev.Pattern(ri.decode(), 0)
    sc = dev.Scanner()

    def call(s):
        res = s.inserts_tensor(left, right, t, SQ_BEST, copy=False)
        assert res["ninserts"] == n, res
        text = s.insert_text(t).cpu().numpy()
        assert text.size == 5 * n
        words, counts = np.unique(np.ascontiguousarray(text.reshape(n, 5)[:, :4]).view("<u4").reshape(-1), return_counts=True)
        exp = sorted((py_key(int(w).to_bytes(4, "little"))[1], int(c)) for w, c in zip(words.tolist(), counts.tolist()))
        return s.tally(t), exp

    def check(s, pair):
        res, exp = pair
        assert {k: res[k] for k in COUNTS} == dict(nspans=n, ntallied=n, nlong=0, nforeign=0, ndistinct=256, max_len=4, passes=2)
        assert list(zip(res["keys"].tolist(), res["counts"].tolist())) == exp and len(exp) == 256
    _go(sc, "%d spans" % n, call, check)
    assert (n + T - 1) // T > 1024 and (256 * ((n + T - 1) // T) + 1023) // 1024 > 256
    sc.close()
    left.close()
    right.close()


# ---- through the pipeline ----
@pytest.fixture(scope="module")
def texts():
    out = {}
    for name, pair in PAIRS.items():
        buf = _buf(_lines(pair))
        out[name] = (buf, _line_offsets(buf))
    return out


@pytest.fixture(scope="module")
def pats(gpu):
    from seeq_amd import device as dev
    ps = {name: (dev.Pattern(*pair[0]), dev.Pattern(*pair[1])) for name, pair in PAIRS.items()}
    yield ps
    for l, r in ps.values():
        l.close()
        r.close()


def _slices(buf, rows, offsets):
    """bytes [start, end) of every row's line, from the host buffer: rows of (line, start, end, ...)."""
    return [buf[offsets[r[0]] + r[1]:offsets[r[0]] + r[2]] for r in rows]


@pytest.mark.parametrize("window", [(10, 14), (0, 0)], ids=lambda w: "%d_%d" % w)
@pytest.mark.parametrize("mode", [SQ_BEST, SQ_FIRST], ids=["best", "first"])
@pytest.mark.parametrize("name", sorted(PAIRS))
def test_tally_of_the_inserts_of_mixed_reads(gpu, capi, oracle, texts, pats, name, mode, window):
    """test_gpu_inserts.py's text: approximate flanks, several occurrences, inserts of 0 - 60 bases, an N here and there.  Expected: the
    oracle's two scans joined by the rule, their spans sliced from the host buffer."""
    from seeq_amd import device as dev
    buf, offsets = texts[name]
    left, right = pats[name]
    rows = Joined(oracle, PAIRS[name], buf, mode).rows(window)
    spans = _slices(buf, rows, offsets)
    assert len(rows) > 100
    if window == (0, 0):
        assert any(len(s) > 31 for s in spans) and any(not s for s in spans)
    t = _cuda(buf)
    sc = dev.Scanner()

    def call(s):
        res = s.inserts_tensor(left, right, t, mode, *window, copy=False)
        assert res["ninserts"] == len(rows)
        return s.tally(t)
    _go(sc, "%s, mode %d, window %s" % (name, mode, window), call, lambda s, res: _same(res, spans))
    if name == "pair20" and window == (10, 14):
        # the guide-library count table: the 12-base gaps hold BARCODES
        res = sc.tally(t)
        by = collections.Counter(spans)
        assert dev.tally_lookup(res, BARCODES).tolist() == [by[b.encode()] for b in BARCODES] and sum(by[b.encode()] for b in BARCODES) > 100
        assert dev.tally_lookup(res, ["ACGTACGTAC" * 3]).tolist() == [by[b"ACGTACGTAC" * 3]]
    sc.close()


def test_tally_under_fastq(gpu, capi, oracle, pats):
    """SEEQDEV_FASTQ: the offsets are those of the sequence lines in the original buffer, and the tally reads them as they are."""
    from seeq_amd import device as dev
    pair = PAIRS["short"]
    left, right = pats["short"]
    lines = _lines(pair, 1500, 41)
    buf, offsets = _fastq(lines, 42, dev.plain_pattern(pair[1][0]))
    j = Joined(oracle, pair, _buf(lines), SQ_BEST)
    t = _cuda(buf)
    sc = dev.Scanner()
    for window in ((0, 0), (10, 14)):
        rows = j.rows(window)
        spans = _slices(buf, rows, offsets)
        assert len(rows) > 50

        def call(s):
            res = s.inserts_tensor(left, right, t, SQ_BEST | dev.SEEQDEV_FASTQ, *window, copy=False)
            assert res["ninserts"] == len(rows)
            return s.tally(t)
        _go(sc, "FASTQ, window %s" % (window,), call, lambda s, res: _same(res, spans))
    sc.close()


def test_tally_of_hits(gpu, capi, oracle, texts, pats):
    """source="hits": the matches themselves, after a plain SQ_ALL fetch (the oracle's records) and after a both-strands call (the
    merged records of the two oracle scans; a minus-strand hit is tallied as the bytes of the text)."""
    from seeq_amd import device as dev
    buf, offsets = texts["pair20"]
    expr, tau = PAIRS["pair20"][0]
    pat = pats["pair20"][0]
    t = _cuda(buf)
    sc = dev.Scanner()
    exp = oracle.buffer_scan(expr, tau, buf, SQ_ALL)["records"].tolist()
    spans = _slices(buf, exp, offsets)
    assert len(exp) > 2 * T and all(len(s) <= 31 for s in spans)

    def plain(s):
        cnt = s.scan_tensor(pat, t, SQ_ALL, dev.WANT_RECORDS)
        assert cnt["nrecords"] == len(exp)
        return s.tally(t, source="hits")
    _go(sc, "hits of a plain SQ_ALL scan", plain, lambda s, res: _same(res, spans))
    assert sc.records(len(exp)).tolist() == exp             # the record arrays are what they were
    # plants of the pattern and of its reverse complement (test_gpu_strands.py's lines)
    sbuf = _buf(_strand_lines(expr, tau, 1500))
    soff = _line_offsets(sbuf)
    st = _cuda(sbuf)
    both = Expected(oracle, expr, tau, sbuf, SQ_ALL).rows
    bspans = _slices(sbuf, both, soff)
    assert sum(1 for r in both if r[4]) > 100 and sum(1 for r in both if not r[4]) > 100

    def strands(s):
        cnt = s.strands_tensor(pat, st, SQ_ALL, dev.WANT_RECORDS, copy=False)
        assert cnt["nrecords"] == len(both)
        return s.tally(st, source="hits")
    _go(sc, "hits of a both-strands call", strands, lambda s, res: _same(res, bspans))
    # hits in the last 32 bytes of a text without a final newline: the pack reads them byte by byte, nothing beyond the text
    tail = ("ACGTACGTAC" * 5 + "\n" + "CATCATCAT" + LEFT + "\n" + LEFT + "ACGTACGTAC\n" + "TTGCA" + LEFT).encode()
    tt = _cuda(tail)
    exact = dev.Pattern(LEFT, 0)
    texp = oracle.buffer_scan(LEFT, 0, tail, SQ_ALL)["records"].tolist()
    assert len(texp) == 3 and texp[-1][2] == len("TTGCA" + LEFT)

    def at_the_end(s):
        assert s.scan_tensor(exact, tt, SQ_ALL, dev.WANT_RECORDS)["nrecords"] == 3
        return s.tally(tt, source="hits")
    _go(sc, "hits at the end of the text", at_the_end, lambda s, res: _same(res, _slices(tail, texp, _line_offsets(tail))))
    exact.close()
    sc.close()


# ---- state ----
def test_state_around_a_tally(gpu, capi, oracle, texts, pats, flanks):
    """Two tallies in a row give the same bytes; the inserts result (records, offsets, insert text) and, for hits, the records are after
    a tally what they were before; a plain scan after a tally gives the oracle's records in as many runs as the same scan before it."""
    from seeq_amd import device as dev
    buf, offsets = texts["pair20"]
    left, right = pats["pair20"]
    t = _cuda(buf)
    sc = dev.Scanner()
    exp = oracle.buffer_scan(PAIRS["pair20"][0][0], PAIRS["pair20"][0][1], buf, SQ_BEST)["records"]
    sc.scan_tensor(left, t, SQ_BEST, dev.WANT_RECORDS)
    cnt = sc.scan_tensor(left, t, SQ_BEST, dev.WANT_RECORDS)                 # (the second scan: the workspace has grown)
    runs = sc.last_runs()
    assert np.array_equal(sc.records(cnt["nrecords"]).astype(np.uint64), exp)
    res = sc.inserts_tensor(left, right, t, SQ_BEST, 0, 0)
    assert res["ninserts"] > T
    before = (res["records"].tobytes(), sc.insert_offsets(res["ninserts"]).tobytes(), sc.insert_text(t).cpu().numpy().tobytes())
    first = sc.tally(t, copy=False)
    assert first["ndistinct"] > 100 and sc.tally_device_ptr()
    table = sc.tally_table(first["ndistinct"]).tobytes()
    again = sc.tally(t, copy=False)
    assert again == first and sc.tally_table(again["ndistinct"]).tobytes() == table
    assert sc.tally_table(10, first=5).tobytes() == table[80:240]
    after = (sc.insert_records(res["ninserts"]).tobytes(), sc.insert_offsets(res["ninserts"]).tobytes(), sc.insert_text(t).cpu().numpy().tobytes())
    assert after == before
    with pytest.raises(dev.SeeqDeviceError):
        sc.fetch()                                          # an inserts call leaves nothing to fetch, and a tally does not change that
    cnt = sc.scan_tensor(left, t, SQ_BEST, dev.WANT_RECORDS)
    assert np.array_equal(sc.records(cnt["nrecords"]).astype(np.uint64), exp) and sc.last_runs() == runs
    hits = sc.tally(t, source="hits")
    assert hits["nspans"] == cnt["nrecords"]
    assert np.array_equal(sc.records(cnt["nrecords"]).astype(np.uint64), exp)
    cnt = sc.scan_tensor(left, t, SQ_BEST, dev.WANT_RECORDS)
    assert np.array_equal(sc.records(cnt["nrecords"]).astype(np.uint64), exp) and sc.last_runs() == runs
    # the table of the inserts is gone (the hits' took its place), the inserts are not
    assert sc.tally(t, copy=False) == first and sc.tally_table(first["ndistinct"]).tobytes() == table
    sc.close()


def test_a_tally_grows_its_own_arrays(gpu, capi, flanks):
    """A tiny reserve sizes the scan's workspace, not the tally's: the tally grows its key arrays and its table, and grows them again
    for a larger call; a smaller call afterwards is served from what is there."""
    from seeq_amd import device as dev
    sc = dev.Scanner()
    sc.reserve(4096, 16, 16, 16)
    rng = random.Random(21)
    for n in (65, 2 * T + 3, 3 * T + 7, 10):
        _planted(sc, flanks, _random_inserts(rng, n, 12, pool=n), "%d spans on one context" % n, seed=n)
    sc.close()


def test_tally_of_the_staged_text(gpu, capi, flanks):
    """inserts_host then tally() without a tensor: the context's staged text; another host call stages over it: EINVAL."""
    from seeq_amd import device as dev
    inserts = _random_inserts(random.Random(31), T + 9, 12)
    buf = _reads(inserts, 31)
    sc = dev.Scanner()

    def call(s):
        res = s.inserts_host(flanks[0], flanks[1], buf, SQ_BEST)
        assert res["ninserts"] == len(inserts) and s.insert_text().split(b"\n")[:-1] == inserts
        return s.tally()
    _go(sc, "the staged text", call, lambda s, res: _same(res, inserts))
    sc.scan_host(flanks[0], b"ACGT\n" * 10, SQ_BEST, dev.WANT_RECORDS)
    assert _raw_tally(sc, capi, capi.SEEQDEV_TALLY_INSERTS, None) == (-1, errno.EINVAL)
    with pytest.raises(dev.SeeqDeviceError):
        sc.tally()
    _same(sc.tally(_cuda(buf)), inserts)                    # the records are still there: with the text given, the same table
    sc.close()


# ---- errors ----
def test_a_span_beyond_the_text_is_an_argument_error(gpu, capi, flanks):
    """nbytes cut short of the last read: a span reaches past it, EIO.  An argument check -- the kernel compares before it loads -- so
    nothing faults and the context goes on: the same call with the right size gives the table."""
    from seeq_amd import device as dev
    inserts = _random_inserts(random.Random(41), T + 9, 12)
    buf = _reads(inserts, 41)
    t = _cuda(buf)
    sc = dev.Scanner()
    res = sc.inserts_tensor(flanks[0], flanks[1], t, SQ_BEST, copy=False)
    assert res["ninserts"] == len(inserts)
    last = sc.insert_records(1, first=len(inserts) - 1)[0]
    end_of_last = int(sc.insert_offsets(1, first=len(inserts) - 1)[0]) + int(last["end"])
    assert _raw_tally(sc, capi, capi.SEEQDEV_TALLY_INSERTS, t, end_of_last - 1) == (-1, errno.EIO)
    assert "outside" in capi.error_text()
    with pytest.raises(dev.SeeqDeviceError):
        sc.tally_table(1)                                   # a failed tally leaves no table
    assert _raw_tally(sc, capi, capi.SEEQDEV_TALLY_INSERTS, t, end_of_last) == (0, 0)
    _same(sc.tally(t), inserts)
    sc.close()


def test_hits_that_cannot_be_tallied(gpu, capi, flanks):
    """source="hits" after an inserts call (nothing to fetch) and after a packed scan (no text offsets): EINVAL; on a fresh context too."""
    import torch
    from seeq_amd import device as dev
    inserts = _random_inserts(random.Random(51), 70, 12)
    buf = _reads(inserts, 51)
    t = _cuda(buf)
    sc = dev.Scanner()
    assert _raw_tally(sc, capi, capi.SEEQDEV_TALLY_HITS, t) == (-1, errno.EINVAL)
    assert _raw_tally(sc, capi, capi.SEEQDEV_TALLY_INSERTS, t) == (-1, errno.EINVAL)
    assert sc.inserts_tensor(flanks[0], flanks[1], t, SQ_BEST, copy=False)["ninserts"] == len(inserts)
    assert _raw_tally(sc, capi, capi.SEEQDEV_TALLY_HITS, t) == (-1, errno.EINVAL)
    _same(sc.tally(t), inserts)
    # a packed scan: reads of one length
    rng = random.Random(52)
    reads = ["".join(rng.choice("ACGT") for _ in range(10)) + LEFT + "".join(rng.choice("ACGT") for _ in range(30)) for _ in range(200)]
    text = _buf(reads)
    bases, nmask, n = dev.pack_reads(text, 60)
    pb, pn = torch.from_numpy(bases).cuda(), torch.from_numpy(nmask).cuda()
    sc.run_packed(flanks[0], pb.data_ptr(), pn.data_ptr(), n, 60, options=SQ_BEST, want=dev.WANT_RECORDS)
    assert sc.fetch()["nrecords"] == 200
    assert _raw_tally(sc, capi, capi.SEEQDEV_TALLY_HITS, _cuda(text)) == (-1, errno.EINVAL)
    assert "packed" in capi.error_text()
    # the same reads as text: the hits are the planted flank
    cnt = sc.scan_tensor(flanks[0], _cuda(text), SQ_BEST, dev.WANT_RECORDS)
    assert cnt["nrecords"] == 200
    res = sc.tally(_cuda(text), source="hits")
    assert (res["ndistinct"], res["ntallied"]) == (1, 200) and dev.tally_decode(int(res["keys"][0])) == LEFT
    assert dev.tally_lookup(res, [LEFT]).tolist() == [200]
    _same(sc.tally(t), inserts)                             # and the inserts of before are still there
    sc.close()
