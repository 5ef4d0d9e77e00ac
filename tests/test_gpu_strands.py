"""GPU (-m gpu): both strands in one call (seeqdevScanRunStrands / seeqdevScanHostStrands) -- the text scanned with a pattern and with
its reverse complement, the two record sets merged on the device -- against a pure-Python merge of two oracle scans (of `expr` and of
revcomp_pattern(expr)) by the rule of seeq_strand.h: SQ_ALL in (line, end, strand) order, SQ_BEST / SQ_FIRST the winner of every line."""
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle.pyoracle import SQ_ALL, SQ_BEST, SQ_CONVERT, SQ_FIRST, SQ_IGNORE

pytestmark = pytest.mark.gpu
PAT20 = "GATGTAGCGCGATTAGCCTG"
CLASSY = "TG[AC]CANNGT"
PAT40 = "GATG[TA]AGCNCGATTAGC[CG]TGAAAATGNGAGTAC[GAT]GCGCGA"
CASES = {"pat20": (PAT20, 3), "classy": (CLASSY, 1), "gaattc": ("GAATTC", 1), "barcode": ("ACGTTGCA", 1)}
MODES = {"first": SQ_FIRST, "best": SQ_BEST, "all": SQ_ALL}
FIELDS = ("line", "start", "end", "dist", "strand")


def _mutate(rng, pat, nerr):
    s = list(pat)
    for _ in range(nerr):
        i = rng.randrange(len(s))
        k = rng.randrange(3)
        if k == 0:
            s[i] = rng.choice("ACGT")
        elif k == 1 and len(s) > 1:
            del s[i]
        else:
            s.insert(i, rng.choice("ACGT"))
    return "".join(s)


def _lines(expr, tau, n=4000, seed=5, lengths=(40, 75, 150, 151), strand_of=None):
    """n lines, each with 0 - 3 plants of the pattern or of its reverse complement (strand_of(i): 0 / 1 / None = either, per plant),
    mutated by 0 .. tau + 1 edits -- built like test_gpu_demux.py::_mixed_lines."""
    from seeq_amd import device as dev
    rng = random.Random(seed)
    plain = [dev.plain_pattern(expr), dev.plain_pattern(dev.revcomp_pattern(expr))]
    lines = []
    for i in range(n):
        m = rng.choice(lengths)
        t = [rng.choice("ACGT") for _ in range(m)]
        for _ in range(rng.choice([0, 1, 1, 2, 3])):
            which = strand_of(i) if strand_of else None
            if which is None:
                which = rng.randrange(2)
            if which < 0:
                continue
            c = _mutate(rng, plain[which], rng.randint(0, tau + 1))
            p = rng.randrange(0, max(1, m - len(c)))
            t[p:p + len(c)] = list(c)
        if rng.random() < 0.02:
            t[rng.randrange(m)] = "N"
        lines.append("".join(t)[:m])
    return lines


def _buf(lines):
    return ("\n".join(lines) + "\n").encode()


def _line_offsets(buf, fasta=False):
    """1-based counted line -> byte offset of its first byte."""
    offs, pos = [None], 0
    for ln in buf.split(b"\n")[:-1] if buf.endswith(b"\n") else buf.split(b"\n"):
        if not (fasta and ln.startswith(b">")):
            offs.append(pos)
        pos += len(ln) + 1
    return offs


class Expected:
    def __init__(self, oracle, expr, tau, buf, mode, opt=0, fasta=False):
        from seeq_amd import device as dev
        ep = oracle.buffer_scan(expr, tau, buf, (mode | opt) & 0xFF, fasta=fasta)
        em = oracle.buffer_scan(dev.revcomp_pattern(expr), tau, buf, (mode | opt) & 0xFF, fasta=fasta)
        assert ep["nlines"] == em["nlines"]
        self.plus = [tuple(r) + (0,) for r in ep["records"].tolist()]
        self.minus = [tuple(r) + (1,) for r in em["records"].tolist()]
        both = self.plus + self.minus
        if mode == SQ_ALL:
            self.rows = sorted(both, key=lambda r: (r[0], r[2], r[4]))
        else:
            per_line = {}
            for r in both:
                per_line.setdefault(r[0], []).append(r)
            pick = (lambda r: (r[3], r[4])) if mode == SQ_BEST else (lambda r: (r[2], r[4]))
            self.rows = [min(per_line[ln], key=pick) for ln in sorted(per_line)]
        self.nlines = ep["nlines"]
        self.nmatchlines = len({r[0] for r in both})
        self.per_strand = [sum(1 for r in self.rows if r[4] == 0), sum(1 for r in self.rows if r[4] == 1)]


def _rows(res):
    rec = res["records"]
    return list(zip(*(rec[f].tolist() for f in FIELDS)))


def _check(sc, res, exp, offsets, records=True):
    assert res["nlines"] == exp.nlines
    assert res["nmatchlines"] == exp.nmatchlines
    assert res["nhits"] == len(exp.rows)
    assert res["per_strand"] == exp.per_strand
    if not records:
        assert res["nrecords"] == 0 and "records" not in res
        return
    assert res["nrecords"] == len(exp.rows) == len(res["records"])
    got = _rows(res)
    if got != exp.rows:
        bad = next(i for i, (a, b) in enumerate(zip(got, exp.rows)) if a != b) if len(got) == len(exp.rows) else None
        raise AssertionError("records differ (%d vs %d; first difference at %s: %s vs %s)"
                             % (len(got), len(exp.rows), bad, got[bad] if bad is not None else None, exp.rows[bad] if bad is not None else None))
    assert sc.record_offsets(len(got)).tolist() == [offsets[r[0]] for r in exp.rows]


# ---- one step: the call, its check, and on failure the same call on a fresh Scanner ----
def _step(sc, what, call, check, fresh=None):
    """check(scanner, call(scanner)) on the long-lived context; when that fails, once more on a fresh Scanner (made by `fresh`, in the
    same environment), and the message says which of the two it is."""
    from seeq_amd import device as dev
    try:
        check(sc, call(sc))
        return
    except (AssertionError, dev.SeeqDeviceError) as e:
        first = e
    text = str(first).lower()
    if isinstance(first, dev.SeeqDeviceError) and ("illegal" in text or "launch failure" in text or "hardware" in text):
        raise first                                        # a device fault: nothing more is started on it
    other = (fresh or dev.Scanner)()
    try:
        check(other, call(other))
        verdict = "the same call on a fresh Scanner PASSES: a state bug of the long-lived context"
    except (AssertionError, dev.SeeqDeviceError) as e:
        verdict = "the same call on a fresh Scanner FAILS too (%s): a kernel bug" % (str(e).splitlines() or [""])[0][:200]
    finally:
        other.close()
    raise AssertionError("%s: %s: %s\n-- %s" % (what, type(first).__name__, first, verdict)) from first


@pytest.fixture(scope="module")
def texts():
    """Per pattern: its lines' buffer and line offsets, made once."""
    out = {}
    for name, (expr, tau) in CASES.items():
        buf = _buf(_lines(expr, tau))
        out[name] = (buf, _line_offsets(buf))
    return out


@pytest.fixture(scope="module")
def expected(oracle, texts):
    memo = {}

    def get(name, mode):
        if (name, mode) not in memo:
            expr, tau = CASES[name]
            memo[name, mode] = Expected(oracle, expr, tau, texts[name][0], mode)
        return memo[name, mode]
    return get


@pytest.fixture(scope="module")
def pats():
    from seeq_amd import device as dev
    ps = {name: dev.Pattern(expr, tau) for name, (expr, tau) in CASES.items()}
    yield ps
    for p in ps.values():
        p.close()


def test_the_text_exercises_every_branch_of_the_rule(gpu, expected):
    """What the construction gives (the oracle's numbers): records on both strands, lines hit on both, lines whose hits alternate
    strands at least twice, equal-distance ties under SQ_BEST; for the self-complementary pattern every key ties; several tiles."""
    for name in ("pat20", "classy"):
        e = expected(name, SQ_ALL)
        assert len(e.plus) > 1024 and len(e.minus) > 1024
        both = {r[0] for r in e.plus} & {r[0] for r in e.minus}
        assert len(both) > 100
        alternating, strands = 0, {}
        for r in e.rows:
            strands.setdefault(r[0], []).append(r[4])
        for s in strands.values():
            alternating += sum(1 for a, b in zip(s, s[1:]) if a != b) >= 2
        assert alternating > 10, (name, alternating)
        b = expected(name, SQ_BEST)
        dp, dm = {r[0]: r[3] for r in b.plus}, {r[0]: r[3] for r in b.minus}
        assert sum(1 for ln in dp if dm.get(ln) == dp[ln]) > 30
    g = expected("gaattc", SQ_ALL)
    assert [r[:4] for r in g.plus] == [r[:4] for r in g.minus] and len(g.rows) == 2 * len(g.plus) > 4096
    assert [r[4] for r in g.rows] == [0, 1] * len(g.plus)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_strands_vs_merged_oracle_scans(gpu, capi, texts, expected, pats, name, mode):
    from seeq_amd import device as dev
    buf, offsets = texts[name]
    sc = dev.Scanner()
    res = sc.strands_host(pats[name], buf, MODES[mode], dev.WANT_RECORDS)
    _check(sc, res, expected(name, MODES[mode]), offsets)
    with pytest.raises(dev.SeeqDeviceError):
        sc.fetch()                                          # nothing left to fetch: the call is complete
    sc.close()


@pytest.fixture(scope="module")
def many(oracle):
    """More records to merge than one round of k_strand_top takes (256 tiles: seeq_tiles.h): the seeded lines of _lines, short ones,
    repeated until even SQ_BEST leaves tile * wg + tile + 3 records on the two strands together.  -> (buffer, line offsets, that number)"""
    with open(os.path.join(ROOT, "seeq_amd", "csrc", "seeq_tiles.h")) as f:
        shape = dict(re.findall(r"^#define\s+(SEEQ_TILE\w*)\s+(\d+)", f.read(), re.M))
    tile, wg = int(shape["SEEQ_TILE"]), int(shape["SEEQ_TILE_WG"])
    need = tile * wg + tile + 3
    base = _lines(PAT20, 3, n=4000, seed=11, lengths=(40, 50, 60))
    one = Expected(oracle, PAT20, 3, _buf(base), SQ_BEST)
    buf = _buf(base * (need // (len(one.plus) + len(one.minus)) + 1))
    return buf, _line_offsets(buf), need


@pytest.mark.parametrize("mode", ["all", "best"])
def test_strands_past_one_round_of_the_top_kernel(gpu, capi, oracle, many, mode):
    """The expectation is the oracle's two scans of the same (repeated) buffer, merged by Expected as everywhere in this file."""
    from seeq_amd import device as dev
    buf, offsets, need = many
    exp = Expected(oracle, PAT20, 3, buf, MODES[mode])
    assert len(exp.plus) + len(exp.minus) >= need           # what is merged: the second round of the top kernel runs
    pat = dev.Pattern(PAT20, 3)
    sc = dev.Scanner()
    _check(sc, sc.strands_host(pat, buf, MODES[mode], dev.WANT_RECORDS), exp, offsets)
    sc.close()
    pat.close()


@pytest.mark.parametrize("name", ["classy", "barcode"])
def test_strands_count_wants(gpu, capi, texts, expected, pats, name):
    from seeq_amd import device as dev
    buf, offsets = texts[name]
    sc = dev.Scanner()
    res = sc.strands_host(pats[name], buf, SQ_BEST, dev.WANT_COUNTLINES)        # (the match mode is ignored: one record per matching line)
    _check(sc, res, expected(name, SQ_FIRST), offsets, records=False)
    res = sc.strands_host(pats[name], buf, 0, dev.WANT_COUNTMATCH)
    _check(sc, res, expected(name, SQ_ALL), offsets, records=False)
    with pytest.raises(dev.SeeqDeviceError):
        sc.records(1)
    sc.close()


def test_strands_paths(gpu, capi, texts, expected, pats, monkeypatch):
    """The barcode and its reverse complement have a union automaton: one walk.  The 20-mer: two scans.  The same bytes either way."""
    from seeq_amd import device as dev
    sc = dev.Scanner()
    one = {}
    for mode in (SQ_BEST, SQ_ALL):
        one[mode] = sc.strands_host(pats["barcode"], texts["barcode"][0], mode, dev.WANT_RECORDS)
        assert sc.last_multi_one_pass()
        one[mode]["offsets"] = sc.record_offsets(one[mode]["nrecords"])
    sc.strands_host(pats["pat20"], texts["pat20"][0], SQ_BEST, dev.WANT_RECORDS)
    assert not sc.last_multi_one_pass()
    monkeypatch.setenv("SEEQ_MULTI", "sequential")
    for mode in (SQ_BEST, SQ_ALL):
        two = sc.strands_host(pats["barcode"], texts["barcode"][0], mode, dev.WANT_RECORDS)
        assert not sc.last_multi_one_pass()
        assert two["records"].tobytes() == one[mode]["records"].tobytes()
        assert sc.record_offsets(two["nrecords"]).tobytes() == one[mode]["offsets"].tobytes()
        assert {k: v for k, v in two.items() if k != "records"} == {k: v for k, v in one[mode].items() if k not in ("records", "offsets")}
    sc.close()


@pytest.mark.parametrize("case", ["plus_then_minus", "minus_then_plus", "plus_only", "minus_only_by_the_twin", "no_hit", "empty", "self_complementary_barcode"])
def test_strands_extremes_of_the_co_rank(gpu, capi, oracle, case):
    from seeq_amd import device as dev
    expr, tau = PAT20, 1
    if case == "plus_then_minus":
        lines = _lines(expr, tau, 3000, 7, strand_of=lambda i: 0 if i < 1500 else 1)
    elif case == "minus_then_plus":
        lines = _lines(expr, tau, 3000, 8, strand_of=lambda i: 1 if i < 1500 else 0)
    elif case == "plus_only":
        lines = _lines(expr, tau, 3000, 9, strand_of=lambda i: 0)
    elif case == "minus_only_by_the_twin":
        lines = _lines(expr, tau, 3000, 9, strand_of=lambda i: 0)
        expr = dev.revcomp_pattern(expr)                    # searching the twin: na = 0
    elif case == "no_hit":
        lines = _lines(expr, tau, 3000, 10, strand_of=lambda i: -1)
    elif case == "empty":
        lines = None
    else:
        expr, tau = "AACGCGTT", 1                           # its own reverse complement, and barcode-sized: every key ties
        lines = _lines(expr, tau, 3000, 11)
    buf = _buf(lines) if lines is not None else b""
    p = dev.Pattern(expr, tau)
    sc = dev.Scanner()
    for mode in (SQ_ALL, SQ_BEST, SQ_FIRST):
        exp = Expected(oracle, expr, tau, buf, mode)
        if mode == SQ_ALL:
            n_plus, n_minus = len(exp.plus), len(exp.minus)
            if case in ("plus_then_minus", "minus_then_plus"):
                assert n_plus > 1024 and n_minus > 1024
                first, last = (exp.plus, exp.minus) if case == "plus_then_minus" else (exp.minus, exp.plus)
                assert first[-1][0] <= 1500 < last[0][0]    # every key of one list below every key of the other
            elif case == "plus_only":
                assert n_plus > 1024 and n_minus == 0
            elif case == "minus_only_by_the_twin":
                assert n_plus == 0 and n_minus > 1024
            elif case in ("no_hit", "empty"):
                assert n_plus == n_minus == 0
            else:
                assert n_plus == n_minus > 1024
        _check(sc, sc.strands_host(p, buf, mode, dev.WANT_RECORDS), exp, _line_offsets(buf))
    sc.close()
    p.close()


@pytest.mark.parametrize("case", ["two_words", "generic_100", "ignore", "convert", "fasta"])
def test_strands_over_other_kinds_of_scan(gpu, capi, oracle, case):
    from seeq_amd import device as dev
    expr, tau, opt, fasta = CLASSY, 1, 0, False
    if case == "two_words":
        expr, tau = PAT40, 5                                # 40 positions with classes and N on 250 bp lines: two-word windows
        buf = _buf(_lines(expr, tau, 800, 12, lengths=(250,)))
    elif case == "generic_100":
        rng = random.Random(13)
        expr, tau = "".join(rng.choice("ACGT") for _ in range(100)), 6      # more than 62 positions: the generic path
        buf = _buf(_lines(expr, tau, 600, 14, lengths=(250, 300)))
    elif case in ("ignore", "convert"):
        opt = SQ_IGNORE if case == "ignore" else SQ_CONVERT
        rng = random.Random(15)
        buf = bytes(c if c == 10 or rng.random() > 0.01 else ord("-X"[case == "convert"]) for c in _buf(_lines(expr, tau, 2000, 16)))
    else:
        opt, fasta = dev.SEEQDEV_FASTA, True
        buf = b"".join(b">read%d %s\n%s\n" % (i, dev.plain_pattern(expr).encode(), ln.encode()) for i, ln in enumerate(_lines(expr, tau, 1500, 17)))
    p = dev.Pattern(expr, tau)
    sc = dev.Scanner()
    offsets = _line_offsets(buf, fasta)
    for mode in (SQ_ALL, SQ_BEST):
        exp = Expected(oracle, expr, tau, buf, mode, opt, fasta)
        assert exp.per_strand[0] > 50 and exp.per_strand[1] > 50
        res = sc.strands_host(p, buf, mode | opt, dev.WANT_RECORDS)
        _check(sc, res, exp, offsets)
        if fasta:
            assert res["nheaders"] == 1500
    if case == "generic_100":
        assert sc.last_path() == "generic"
    sc.close()
    p.close()


def test_strands_fastq(gpu, capi, oracle):
    """Four-line records whose quality lines hold A / C / G and whose headers carry the pattern: only the sequence lines count."""
    from seeq_amd import device as dev
    expr, tau = "GACGCAGGAC", 1
    rng = random.Random(18)
    seqs = _lines(expr, tau, 600, 19, lengths=(75, 100, 101))
    raw = []
    for i, sq in enumerate(seqs):
        qual = [rng.choice("ACG") for _ in sq]
        if i % 3 == 0 and len(qual) > 20:
            qual[5:5 + len(expr)] = list(expr)              # a quality string that matches the pattern
        raw += ["@read%d %s" % (i, expr), sq, "+", "".join(qual)[:len(sq)]]
    buf = _buf(raw)
    seq_buf = _buf(seqs)
    raw_offsets = _line_offsets(buf)
    offsets = [None] + [raw_offsets[4 * r + 2] for r in range(len(seqs))]      # record r + 1 -> its sequence line in the ORIGINAL buffer
    p = dev.Pattern(expr, tau)
    sc = dev.Scanner()
    plain = sc.strands_host(p, buf, SQ_ALL, dev.WANT_RECORDS)                  # without the flag: headers and quality lines match too
    for mode in (SQ_ALL, SQ_BEST, SQ_FIRST):
        exp = Expected(oracle, expr, tau, seq_buf, mode)
        assert exp.per_strand[0] > 50 and exp.per_strand[1] > 50
        res = sc.strands_host(p, buf, mode | dev.SEEQDEV_FASTQ, dev.WANT_RECORDS)
        assert res["nlines"] == len(seqs) and res["nheaders"] == 0
        _check(sc, res, exp, offsets)
    assert plain["nlines"] == 4 * len(seqs) and plain["nrecords"] >= len(Expected(oracle, expr, tau, seq_buf, SQ_ALL).rows) + 150
    # SQ_IGNORE: the headers match as well ('@', digits and blanks are skipped) -- and still only the sequence lines count
    exp = Expected(oracle, expr, tau, seq_buf, SQ_ALL, SQ_IGNORE)
    _check(sc, sc.strands_host(p, buf, SQ_ALL | SQ_IGNORE | dev.SEEQDEV_FASTQ, dev.WANT_RECORDS), exp, offsets)
    assert sc.strands_host(p, buf, SQ_ALL | SQ_IGNORE, dev.WANT_RECORDS)["nrecords"] >= len(exp.rows) + 150 + len(seqs)
    res = sc.strands_host(p, buf, dev.SEEQDEV_FASTQ, dev.WANT_COUNTMATCH)
    _check(sc, res, Expected(oracle, expr, tau, seq_buf, SQ_ALL), offsets, records=False)
    sc.close()
    p.close()


def test_strands_host_and_resident_entries_and_a_plain_scan_afterwards(gpu, capi, oracle, texts, expected, pats):
    """One context: a small call, then a large one (its workspace grows), host and resident entries; the plain scan after them
    answers as the oracle's single-strand scan, no strand bit anywhere."""
    import torch
    from seeq_amd import device as dev
    buf, offsets = texts["classy"]
    small = buf[:buf.index(b"\n", 2000) + 1]
    sc = dev.Scanner()
    expr, tau = CASES["classy"]
    _check(sc, sc.strands_host(pats["classy"], small, SQ_ALL, dev.WANT_RECORDS), Expected(oracle, expr, tau, small, SQ_ALL), offsets)
    for mode in (SQ_ALL, SQ_BEST):
        host = sc.strands_host(pats["classy"], buf, mode, dev.WANT_RECORDS)
        _check(sc, host, expected("classy", mode), offsets)
        t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
        res = sc.strands_tensor(pats["classy"], t, mode, dev.WANT_RECORDS)
        assert res["records"].tobytes() == host["records"].tobytes()
        assert {k: v for k, v in res.items() if k != "records"} == {k: v for k, v in host.items() if k != "records"}
        lazy = sc.strands_tensor(pats["classy"], t, mode, dev.WANT_RECORDS, copy=False)
        assert "records" not in lazy and lazy["nrecords"] == host["nrecords"]
        raw = sc.records(lazy["nrecords"])
        assert np.array_equal(raw[:, 3] >> 31, host["records"]["strand"]) and np.array_equal(raw[:, 3] & 0x7FFFFFFF, host["records"]["dist"])
        assert sc.strand_records(10, first=5).tobytes() == host["records"][5:15].tobytes()
    for mode in (SQ_ALL, SQ_BEST):
        r = sc.scan_host(pats["classy"], buf, mode, dev.WANT_RECORDS)
        e = oracle.buffer_scan(expr, tau, buf, mode)
        assert r["nlines"] == e["nlines"] and r["nmatchlines"] == e["nmatchlines"]
        assert np.array_equal(r["records"].astype(np.uint64), e["records"])     # (dist as it is: no strand bit)
    # Pattern.revcomp(): a pattern of its own whose plain scan is the oracle's scan of the reverse-complement expression
    twin = pats["classy"].revcomp()
    assert twin.pattern == dev.revcomp_pattern(expr) and twin.tau == tau and twin.wlen == pats["classy"].wlen
    r = sc.scan_host(twin, buf, SQ_ALL, dev.WANT_RECORDS)
    assert np.array_equal(r["records"].astype(np.uint64), oracle.buffer_scan(twin.pattern, tau, buf, SQ_ALL)["records"])
    twin.close()
    sc.close()


def test_demux_in_both_orientations(gpu, capi, oracle):
    """The demultiplexer over [P_k ..., P_k.revcomp() ...]: the winner's index names the strand."""
    from seeq_amd import device as dev
    from test_gpu_demux import _check as demux_check, _expected as demux_expected, _mixed_lines
    barcodes, taus = ["ACGTTGCA", "TTGACCGA", "GGCATTAC", "CAGTGTCA"], [1, 1, 1, 1]
    exprs = barcodes + [dev.revcomp_pattern(b) for b in barcodes]
    buf = _buf(_mixed_lines(exprs, taus * 2, n=3000, seed=21))
    fwd = [dev.Pattern(b, t) for b, t in zip(barcodes, taus)]
    ps = fwd + [p.revcomp() for p in fwd]
    sc = dev.Scanner()
    res = sc.demux_host(ps, buf)
    exp = demux_expected(oracle, exprs, taus * 2, buf)
    demux_check(res, exp)
    assert all(n > 100 for n in res["assigned"])
    sc.close()
    for p in ps:
        p.close()


# ---- both strands under pressure: small segments, a tiny workspace, a one walk that gives up, shrinking and growing calls ----
SEG = 65536
TILE = 8192                    # bytes of a k_pair tile: a candidate in a tile without a newline is long-line input


def _fastq_text(seqs, expr, seed):
    """Four-line records around the sequence lines (headers that carry the pattern, quality lines of A / C / G) -> (buffer, buffer of
    the sequence lines alone, offsets: record r -> its sequence line in the buffer)."""
    rng = random.Random(seed)
    raw = []
    for i, sq in enumerate(seqs):
        raw += ["@read%d %s" % (i, expr), sq, "+", "".join(rng.choice("ACG") for _ in sq)]
    buf = _buf(raw)
    raw_offsets = _line_offsets(buf)
    return buf, _buf(seqs), [None] + [raw_offsets[4 * r + 2] for r in range(len(seqs))]


def _segments_with_both_strands(exp, offsets):
    return len({offsets[r[0]] // SEG for r in exp.plus} & {offsets[r[0]] // SEG for r in exp.minus})


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", ["barcode", "classy", "pat20"])
def test_strands_over_small_segments(gpu, capi, texts, expected, pats, name, mode, monkeypatch):
    """Segments of 64 KiB: more than six of them, records of both strands in at least three; the one walk's regions and the side
    arrays of the two scans are filled segment by segment."""
    from seeq_amd import device as dev
    monkeypatch.setenv("SEEQ_SEGMENT_BYTES", str(SEG))
    buf, offsets = texts[name]
    assert len(buf) > 6 * SEG and _segments_with_both_strands(expected(name, SQ_ALL), offsets) >= 3
    sc = dev.Scanner()

    def check(s, res):
        _check(s, res, expected(name, MODES[mode]), offsets)
        assert s.last_multi_one_pass() == (name != "pat20")      # (the class pattern is barcode-sized too: 10 positions, distance 1)
    _step(sc, "%s, mode %s, 64 KiB segments" % (name, mode), lambda s: s.strands_host(pats[name], buf, MODES[mode], dev.WANT_RECORDS), check)
    sc.close()


def test_strands_fastq_over_small_segments(gpu, capi, oracle, monkeypatch):
    from seeq_amd import device as dev
    monkeypatch.setenv("SEEQ_SEGMENT_BYTES", str(SEG))
    expr, tau = CASES["barcode"]
    buf, seq_buf, offsets = _fastq_text(_lines(expr, tau, 2400, 31, lengths=(75, 100, 101)), expr, 32)
    p = dev.Pattern(expr, tau)
    sc = dev.Scanner()
    for mode in (SQ_ALL, SQ_BEST):
        exp = Expected(oracle, expr, tau, seq_buf, mode)
        assert len(buf) > 6 * SEG and _segments_with_both_strands(exp, offsets) >= 3
        _step(sc, "FASTQ, mode %d, 64 KiB segments" % mode, lambda s: s.strands_host(p, buf, mode | dev.SEEQDEV_FASTQ, dev.WANT_RECORDS),
              lambda s, res: _check(s, res, exp, offsets))
        assert sc.last_multi_one_pass()
    sc.close()
    p.close()


@pytest.fixture(scope="module")
def skewed():
    """Barcode lines with three minus plants for every plus one: in a call of two scans the twin's scan, too, outgrows the workspace
    that the scan before it left."""
    expr, tau = CASES["barcode"]
    lines = _lines(expr, tau, 3000, 23, strand_of=lambda i: 0 if i % 4 == 0 else 1)
    return lines, _buf(lines)


def _tiny():
    from seeq_amd import device as dev
    sc = dev.Scanner()
    sc.reserve(0, 10, 2, 1)                                # every capacity overflows, and the optimistic first reservation is off for good
    return sc


@pytest.mark.parametrize("what", ["all", "best", "countmatch"])
@pytest.mark.parametrize("path", ["one_walk", "sequential"])
def test_strands_in_a_tiny_workspace(gpu, capi, oracle, pats, skewed, path, what, monkeypatch):
    from seeq_amd import device as dev
    if path == "sequential":
        monkeypatch.setenv("SEEQ_MULTI", "sequential")
    expr, tau = CASES["barcode"]
    lines, buf = skewed
    offsets = _line_offsets(buf)
    mode, want = {"all": (SQ_ALL, dev.WANT_RECORDS), "best": (SQ_BEST, dev.WANT_RECORDS), "countmatch": (0, dev.WANT_COUNTMATCH)}[what]
    exp = Expected(oracle, expr, tau, buf, SQ_ALL if what == "countmatch" else mode)
    assert len(exp.minus) > 1.5 * len(exp.plus) + 64 and len(exp.plus) > 256      # (a re-run leaves an eighth to spare: the twin needs more)
    sc = _tiny()
    for i in range(2):                                     # (the second call: in the workspace the first one grew)
        _step(sc, "tiny workspace, %s, %s, call %d" % (path, what, i), lambda s: s.strands_host(pats["barcode"], buf, mode, want),
              lambda s, res: _check(s, res, exp, offsets, records=want == dev.WANT_RECORDS), fresh=_tiny)
        assert sc.last_multi_one_pass() == (path == "one_walk")
        if i == 0:
            print(path, what, "runs of the last scan or walk:", sc.last_runs())
            assert sc.last_runs() > 1
    sc.close()


@pytest.mark.parametrize("path", ["one_walk", "sequential"])
def test_strands_fastq_in_a_tiny_workspace(gpu, capi, oracle, pats, skewed, path, monkeypatch):
    """The filter's scratch follows the record arrays that the scans and strands_merge grow (cap_fq == cap_records)."""
    from seeq_amd import device as dev
    if path == "sequential":
        monkeypatch.setenv("SEEQ_MULTI", "sequential")
    expr, tau = CASES["barcode"]
    buf, seq_buf, offsets = _fastq_text(skewed[0], expr, 33)
    sc = _tiny()
    for i, mode in enumerate((SQ_ALL, SQ_BEST, SQ_ALL)):
        exp = Expected(oracle, expr, tau, seq_buf, mode)
        assert len(exp.minus) > 1.5 * len(exp.plus) + 64 and len(exp.plus) > 256
        _step(sc, "tiny workspace, FASTQ, %s, mode %d" % (path, mode), lambda s: s.strands_host(pats["barcode"], buf, mode | dev.SEEQDEV_FASTQ, dev.WANT_RECORDS),
              lambda s, res: _check(s, res, exp, offsets), fresh=_tiny)
        assert sc.last_multi_one_pass() == (path == "one_walk")
        if i == 0:
            assert sc.last_runs() > 1
    # and unflagged afterwards: the scratch stays behind the record arrays
    plain = Expected(oracle, expr, tau, buf, SQ_ALL)
    _step(sc, "tiny workspace, after FASTQ, %s" % path, lambda s: s.strands_host(pats["barcode"], buf, SQ_ALL, dev.WANT_RECORDS),
          lambda s, res: _check(s, res, plain, _line_offsets(buf)), fresh=_tiny)
    sc.close()


def test_strands_one_walk_that_gives_up(gpu, capi, oracle, texts, expected, pats):
    """Reads with one line of four tiles that has hits on both strands: the sample says read-length lines and the context has no
    fall-back flag, so the pair is walked once -- as the clean text before it is -- until the device meets the long line
    (RERUN_NOT_ONE_WALK); two scans finish the call.  The next call on the clean text is one walk again."""
    from seeq_amd import device as dev
    expr, tau = CASES["barcode"]
    plain = [dev.plain_pattern(expr), dev.plain_pattern(dev.revcomp_pattern(expr))]
    rng = random.Random(34)
    big = [rng.choice("ACGT") for _ in range(4 * TILE)]
    for j in range(40):
        c = _mutate(rng, plain[j % 2], rng.randint(0, tau))
        q = rng.randrange(len(big) - len(c))
        big[q:q + len(c)] = list(c)
    lines = _lines(expr, tau, 3000, 35)
    lines.insert(2000, "".join(big)[:4 * TILE])
    buf = _buf(lines)
    assert sum(len(ln) + 1 for ln in lines[:2000]) > 2 * SEG           # (the sample, 64 KiB, holds reads only)
    offsets = _line_offsets(buf)
    clean, clean_offsets = texts["barcode"]
    sc = dev.Scanner()

    def one_walk(s, res):
        _check(s, res, expected("barcode", SQ_ALL), clean_offsets)
        assert s.last_multi_one_pass()
    _step(sc, "the clean text first", lambda s: s.strands_host(pats["barcode"], clean, SQ_ALL, dev.WANT_RECORDS), one_walk)
    assert sc.fallback() == (0, 0)
    for mode in (SQ_ALL, SQ_BEST):
        exp = Expected(oracle, expr, tau, buf, mode)
        if mode == SQ_ALL:
            assert sum(1 for r in exp.plus if r[0] == 2001) >= 5 and sum(1 for r in exp.minus if r[0] == 2001) >= 5

        def gave_up(s, res):
            _check(s, res, exp, offsets)
            assert not s.last_multi_one_pass()
            assert s.fallback()[0] & dev.FALLBACK_LONG_LINES       # met on the device, not planned for
        _step(sc, "reads around a long line, mode %d" % mode, lambda s: s.strands_host(pats["barcode"], buf, mode, dev.WANT_RECORDS), gave_up)
    _step(sc, "the clean text after it", lambda s: s.strands_host(pats["barcode"], clean, SQ_ALL, dev.WANT_RECORDS), one_walk)
    sc.close()


@pytest.mark.parametrize("name,expr,tau", [("barcode", "ACGTTGCA", 1), ("pat20", PAT20, 1)])
def test_strands_shrinking_and_growing(gpu, capi, oracle, name, expr, tau):
    """One context: 20 lines, the full text, 20 lines again, a text without a minus record, the full text -- under SQ_ALL, SQ_BEST and with
    SEEQDEV_FASTQ: the side arrays, the merged arrays and the one walk's regions hold the records of the larger call before beyond n."""
    from seeq_amd import device as dev
    if name == "pat20":
        seqs = {"small": _lines(expr, tau, 20, 36, strand_of=lambda i: 0), "full": _lines(expr, tau, 3000, 37),
                "plus_only": _lines(expr, tau, 3000, 38, strand_of=lambda i: 0)}
    else:
        # (random text holds the 8-mer's twin within one error now and then: lines of A and G around exact copies hold none)
        rng = random.Random(36)
        purine = ["".join(rng.choice("AG") for _ in range(40)) + (expr if i % 2 else "") + "".join(rng.choice("AG") for _ in range(40)) for i in range(400)]
        seqs = {"small": purine[:20], "full": _lines(expr, tau, 3000, 37), "plus_only": purine}
    p = dev.Pattern(expr, tau)
    sc = dev.Scanner()
    for mode, fastq in ((SQ_ALL, False), (SQ_BEST, False), (SQ_ALL, True)):
        made = {}
        for k, ls in seqs.items():
            buf, seq_buf, offsets = _fastq_text(ls, expr, 39) if fastq else (_buf(ls), _buf(ls), _line_offsets(_buf(ls)))
            made[k] = (buf, Expected(oracle, expr, tau, seq_buf, mode), offsets)
        assert len(made["full"][1].minus) > 1024 and len(made["full"][1].plus) > 1024
        assert len(made["plus_only"][1].minus) == 0 and len(made["small"][1].minus) == 0 and len(made["small"][1].plus) > 0
        for k in ("small", "full", "small", "plus_only", "full", "plus_only"):
            buf, exp, offsets = made[k]
            _step(sc, "%s, mode %d%s, the %s text" % (name, mode, ", FASTQ" if fastq else "", k),
                  lambda s: s.strands_host(p, buf, mode | (dev.SEEQDEV_FASTQ if fastq else 0), dev.WANT_RECORDS), lambda s, res: _check(s, res, exp, offsets))
            if k == "full":
                assert sc.last_multi_one_pass() == (name == "barcode")
    sc.close()
    p.close()
