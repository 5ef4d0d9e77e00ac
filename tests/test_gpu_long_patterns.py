"""GPU (-m gpu): patterns of 63 .. 512 positions on every batched entry point -- the generic path (k_nl_count / k_nl_write /
k_index_finalize, k_forward<W>, k_compact, k_seg_mid, k_exact<W, COUNT / EMIT>, k_rec_offsets, run_segments<W>) and
k_string<W> at W = 2, 4, 8, 16 column words -- bit-exact against the oracle: nlines, nmatchlines, nhits and every record.

Every test builds its text and the oracle's answers first, checks that the case is not vacuous (hit lines, near misses, lines
with several records) and only then asks for the GPU: without one the tests fail there, they never skip."""
import json
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle.pyoracle import SQ_ALL, SQ_BEST, SQ_CONVERT, SQ_COUNT, SQ_FAIL, SQ_FIRST, SQ_IGNORE, SQ_STREAM

pytestmark = pytest.mark.gpu

LENGTHS = (63, 64, 65, 96, 97, 128, 129, 200, 256, 257, 384, 511, 512)
FASTA = 0x100
WANT_COUNTLINES, WANT_COUNTMATCH, WANT_RECORDS = 0, 1, 2
FOREIGN = "RYKM-*xz@+!.\t;"


def _taus(m):
    """tau = 3, 31 / 32 / 33 where the pattern is long enough for them, and one distance of at least m / 4."""
    out = [3] + [t for t in (31, 32, 33) if t < m - 1]
    if max(out) * 4 < m:
        out.append((m + 3) // 4)
    return out


# random patterns at every length and distance; one periodic and one single-base pattern per word count (W = 4, 8, 16)
CASES = [(m, tau, "random") for m in LENGTHS for tau in _taus(m)] + \
        [(m, tau, kind) for m in (97, 200, 384) for kind in ("periodic", "single") for tau in (3, m // 8)]


def _words(m):
    return next(w for w in (1, 2, 4, 8, 16) if 32 * w >= m)


def _pattern(rng, m, kind="random"):
    if kind == "single":
        return rng.choice("ACGT") * m
    if kind == "periodic":
        unit = rng.choice(["AC", "ACG", "GATC", "TTA"])
        return (unit * m)[:m]
    out = []
    for _ in range(m):
        x = rng.random()
        out.append("N" if x < 0.04 else "[" + "".join(rng.sample("ACGT", 2)) + "]" if x < 0.10 else rng.choice("ACGT"))
    return "".join(out)


def _core(pattern):
    sys.path.insert(0, GOLDEN)
    from make_golden import plain
    return plain(pattern)


def _mutate(rng, s, e):
    sys.path.insert(0, GOLDEN)
    from make_golden import mutate
    return mutate(rng, s, e)


def _dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _near_miss(rng, core, keys, k):
    """core with k substitutions at single-letter positions away from its ends, each by a base the position does not take."""
    pos = [i for i in range(len(core) // 16, len(core) - len(core) // 16) if keys[i] in (1, 2, 4, 8)]
    s = list(core)
    for i in rng.sample(pos, min(k, len(pos))):
        s[i] = rng.choice([b for j, b in enumerate("ACGT") if not keys[i] >> j & 1])
    return "".join(s)


def _place(rng, n, cp, where):
    """A line of n bytes (n >= len(cp): else the copy alone) with cp at its start, at its end or inside."""
    if n <= len(cp):
        return cp
    q = 0 if where == "start" else n - len(cp) if where == "end" else rng.randrange(n - len(cp) + 1)
    t = _dna(rng, n)
    return t[:q] + cp + t[q + len(cp):]


def _spoil(rng, line):
    """Now and then: N, lower case, U for T, a foreign byte, a NUL, a CR at the end."""
    if not line:
        return line
    t = list(line)
    x = rng.random()
    if x < 0.06:
        t[rng.randrange(len(t))] = rng.choice("Nn")
    elif x < 0.12:
        t = [c.lower() if rng.random() < 0.5 else c for c in t]
    elif x < 0.18:
        t = [rng.choice("Uu") if c == "T" and rng.random() < 0.5 else c for c in t]
    elif x < 0.24:
        t[rng.randrange(len(t))] = rng.choice(FOREIGN)
    elif x < 0.26:
        t[rng.randrange(len(t))] = "\0"
    elif x < 0.30:
        t.append("\r")
    return "".join(t)


def _ragged_lines(rng, oracle, pattern, tau, budget):
    """Lines of 0, 1, m - tau - 1, m - tau, m - 1, m, m + tau, 150, 250, 1 000 bytes (and a few of 2 m + tau so that the longest
    patterns get room) with planted copies carrying 0 .. tau + 2 edits at the start, at the end and inside.  -> (lines, indices of
    the lines that hold nothing but a copy with tau + 1 / tau + 2 positions deleted)."""
    keys, _ = oracle.parse(pattern)
    core = _core(pattern)
    m = len(core)
    lines = ["", rng.choice("ACGT"), core[tau + 1:], core[tau:], core[1:], core, _dna(rng, tau // 2) + core + _dna(rng, tau - tau // 2)]
    lines += [_place(rng, m + 40, core, "inside"), _place(rng, 2 * m + 60, core, "start")[:m + 30] + _dna(rng, 30) + core]      # one record; two or more under SQ_ALL
    near = []
    for k in (tau + 1, tau + 2):
        # the copy alone on its line, k positions deleted: whatever the pattern, m - k bytes lie k or more edits away from it
        near.append(len(lines))
        gone = set(rng.sample(range(m), min(k, m)))
        lines.append("".join(c for i, c in enumerate(core) if i not in gone))
        lines.append(_place(rng, m + 20, _near_miss(rng, core, keys, k), "inside"))       # and with k substitutions, in random text
    nbytes = sum(len(x) + 1 for x in lines)
    while nbytes < budget:
        n = rng.choice([0, 1, m - tau - 1, m - tau, m - 1, m, m + tau, 150, 250, 1000, 2 * m + tau])
        if rng.random() < 0.7 and n >= m - tau:
            line = _place(rng, n, _mutate(rng, core, rng.randint(0, tau + 2)), rng.choice(["start", "end", "inside"]))
            if rng.random() < 0.15:
                line += _mutate(rng, core, rng.randint(0, tau))                                                                       # a tandem copy
        else:
            line = _dna(rng, n)
        lines.append(_spoil(rng, line))
        nbytes += len(lines[-1]) + 1
    head = lines[:2 * len(near) + 9]
    rest = lines[len(head):]
    rng.shuffle(rest)
    return head + rest, near


def _as_fasta(rng, lines, core):
    out = []
    for i, ln in enumerate(lines):
        if i % 3 == 0:
            out.append(rng.choice([">seq%d" % i, ">" + core, "> " + core[:40] + " len=%d" % len(ln), ">"]))
        out.append(ln)
    return out


def _same(got, exp, what):
    assert got["nlines"] == exp["nlines"], (what, got["nlines"], exp["nlines"])
    assert got["nmatchlines"] == exp["nmatchlines"], (what, got["nmatchlines"], exp["nmatchlines"])
    if "records" in got:
        assert got["nrecords"] == len(exp["records"]), (what, got["nrecords"], len(exp["records"]))
        if not np.array_equal(got["records"].astype(np.uint64), exp["records"]):
            g, e = got["records"].astype(np.uint64), exp["records"]
            bad = next(i for i in range(len(e)) if not np.array_equal(g[i], e[i]))
            raise AssertionError("%s: record %d of %d differs: %s, oracle %s" % (what, bad, len(e), g[bad].tolist(), e[bad].tolist()))


def _counts_same(sc, dev, pat, buf, opt, expa, what):
    """WANT_COUNTLINES and WANT_COUNTMATCH against the oracle's SQ_ALL scan of the same text."""
    c1 = sc.scan_host(pat, buf, opt, dev.WANT_COUNTLINES)
    assert sc.last_path() == "generic"
    assert (c1["nlines"], c1["nmatchlines"], c1["nhits"]) == (expa["nlines"], expa["nmatchlines"], expa["nmatchlines"]), (what, c1)
    c2 = sc.scan_host(pat, buf, opt, dev.WANT_COUNTMATCH)
    assert sc.last_path() == "generic"
    assert (c2["nlines"], c2["nmatchlines"], c2["nhits"]) == (expa["nlines"], expa["nmatchlines"], len(expa["records"])), (what, c2)


@pytest.mark.parametrize("m,tau,kind", CASES, ids=["%s-m%d-tau%d" % (k, m, t) for m, t, k in CASES])
def test_batch_scan_read_length_and_ragged_lines(request, oracle, m, tau, kind):
    """seeqdevScanHost over ragged text, a pattern of m positions: FIRST / BEST / ALL records x SQ_FAIL / SQ_CONVERT / SQ_IGNORE, both
    counts, with and without a trailing newline, and the same lines as FASTA records -- k_forward<W> / k_exact<W, *> for W = 2 .. 16."""
    rng = random.Random(1000 * m + tau + (7 if kind == "periodic" else 13 if kind == "single" else 0))
    pattern = _pattern(rng, m, kind)
    core = _core(pattern)
    lines, near = _ragged_lines(rng, oracle, pattern, tau, min(40000, 4_000_000 // m))
    buf = ("\n".join(lines) + "\n").encode("latin-1")
    exp = {(mo, nd): oracle.buffer_scan(pattern, tau, buf, mo | nd) for nd in (SQ_FAIL, SQ_CONVERT, SQ_IGNORE) for mo in (SQ_FIRST, SQ_BEST, SQ_ALL)}
    # the case is not vacuous: hit lines, a planted copy that is no hit, a line with several records
    expa = exp[(SQ_ALL, SQ_FAIL)]
    hit_lines = set(int(x) for x in expa["records"][:, 0])
    assert len(hit_lines) >= 3, (m, tau, kind, len(hit_lines))
    assert any(i + 1 not in hit_lines for i in near), (m, tau, kind, "both near misses match")
    assert int(expa["line_nhits"].max()) >= 2, (m, tau, kind, "no line with two records")
    cut = buf[:-1]
    exp_cut = oracle.buffer_scan(pattern, tau, cut, SQ_ALL)
    fa = ("\n".join(_as_fasta(rng, lines, core)) + "\n").encode("latin-1")
    exp_fa = {mo: oracle.buffer_scan(pattern, tau, fa, mo, fasta=True) for mo in (SQ_BEST, SQ_ALL)}
    assert len(exp_fa[SQ_ALL]["records"]) >= 3

    request.getfixturevalue("gpu")
    from seeq_amd import device as dev
    pat = dev.Pattern(pattern, tau)
    assert pat.wlen == m
    sc = dev.Scanner()
    for (mo, nd), e in exp.items():
        got = sc.scan_host(pat, buf, mo | nd, dev.WANT_RECORDS)
        assert sc.last_path() == "generic" and sc.last_kernel() == "k_forward"        # the kernels under test ran
        _same(got, e, (m, tau, kind, mo, nd))
    for nd in (SQ_FAIL, SQ_CONVERT, SQ_IGNORE):
        _counts_same(sc, dev, pat, buf, nd, exp[(SQ_ALL, nd)], (m, tau, kind, nd))
    got = sc.scan_host(pat, cut, SQ_ALL, dev.WANT_RECORDS)
    assert sc.last_path() == "generic"
    _same(got, exp_cut, (m, tau, kind, "no trailing newline"))
    for mo, e in exp_fa.items():
        got = sc.scan_host(pat, fa, mo | FASTA, dev.WANT_RECORDS)
        assert sc.last_path() == "generic"
        _same(got, e, (m, tau, kind, mo, "fasta"))
    _counts_same(sc, dev, pat, fa, FASTA, exp_fa[SQ_ALL], (m, tau, kind, "fasta"))
    sc.close()
    pat.close()


def _long_lines(rng, core, tau, sizes):
    """Lines of tens of kilobytes with planted and tandem copies (0 .. tau + 2 edits) every few hundred bytes."""
    m = len(core)
    lines = []
    for n in sizes:
        t = list(_dna(rng, n))
        q = rng.randrange(0, 300)
        while q + 2 * m + 2 * tau + 8 < n:
            cp = _mutate(rng, core, rng.randint(0, tau + 2))
            t[q:q + len(cp)] = list(cp)
            if rng.random() < 0.25:
                cp2 = _mutate(rng, core, rng.randint(0, tau))
                t[q + len(cp):q + len(cp) + len(cp2)] = list(cp2)
                q += len(cp2)
            q += len(cp) + rng.choice([3, 150, 400, 1000, 3000])
        lines.append("".join(t[:n]))
    return lines


@pytest.mark.parametrize("m,tau,sizes", [(65, 8, (150_000, 40_000, 90_000)), (129, 16, (100_000, 60_000)), (257, 33, (120_000,)),
                                         (512, 100, (60_000, 41_000))], ids=["m65", "m129", "m257", "m512"])
def test_batch_scan_long_lines(request, oracle, m, tau, sizes):
    """1-3 lines of 40-150 KB (one lane walks a whole line on the generic path) with tens to hundreds of planted and tandem copies."""
    rng = random.Random(7000 + m)
    pattern = _pattern(rng, m)
    lines = _long_lines(rng, _core(pattern), tau, sizes)
    buf = ("\n".join(lines) + "\n").encode()
    exp = {mo: oracle.buffer_scan(pattern, tau, buf, mo) for mo in (SQ_FIRST, SQ_BEST, SQ_ALL)}
    assert len(exp[SQ_ALL]["records"]) >= 10 * len(sizes) and exp[SQ_ALL]["nmatchlines"] == len(sizes), (m, len(exp[SQ_ALL]["records"]))

    request.getfixturevalue("gpu")
    from seeq_amd import device as dev
    pat = dev.Pattern(pattern, tau)
    sc = dev.Scanner()
    for mo, e in exp.items():
        got = sc.scan_host(pat, buf, mo, dev.WANT_RECORDS)
        assert sc.last_path() == "generic"
        _same(got, e, (m, tau, mo))
    _counts_same(sc, dev, pat, buf, 0, exp[SQ_ALL], (m, tau))
    sc.close()
    pat.close()


SEGMENTS = r"""
import os, sys, random, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
from oracle.pyoracle import Oracle, SQ_ALL, SQ_BEST
from seeq_amd import device as dev
import test_gpu_long_patterns as T
o = Oracle()
SEG = 65536
for m, tau in ((129, 10), (300, 24)):
    rng = random.Random(9000 + m)
    pattern = T._pattern(rng, m)
    core = T._core(pattern)
    parts, pos, seam_hits = [], 0, 0
    def add(line):
        global pos
        parts.append(line); pos += len(line) + 1
    while pos < 13 * SEG:
        room = SEG - pos %% SEG
        if pos // SEG == 3 and room > SEG - 2000:
            add(T._long_lines(rng, core, tau, (SEG + 9000,))[0])          # a line longer than a segment
        elif room < 900:
            # a line that straddles the seam AT a hit: the copy begins before the seam and ends behind it
            before = max(0, room - rng.randrange(1, m))
            add(T._dna(rng, before) + core + T._dna(rng, rng.randrange(0, 200)))
            seam_hits += 1
        else:
            n = rng.choice([0, 150, 250, 400, 700])
            line = T._dna(rng, n)
            if n >= m and rng.random() < 0.5:
                line = T._place(rng, n, T._mutate(rng, core, rng.randint(0, tau + 2)), "inside")
            add(line)
    buf = ("\n".join(parts) + "\n").encode()
    assert len(buf) >= 10 * SEG and seam_hits >= 9
    starts = np.cumsum([0] + [len(x) + 1 for x in parts])
    p = dev.Pattern(pattern, tau)
    for opt in (SQ_BEST, SQ_ALL):
        exp = o.buffer_scan(pattern, tau, buf, opt)
        # lines with a record that begins in one segment and ends in the next
        across = sum(1 for l, s_, e, d in exp["records"].tolist() if (starts[l - 1] + s_) // SEG != (starts[l - 1] + e - 1) // SEG)
        assert across >= 9 and exp["nmatchlines"] > 100, (m, across, exp["nmatchlines"])
        sc = dev.Scanner()
        sc.reserve(0, 10, 2, 1)                 # absurdly small: OVF_LINES, OVF_HITLINES and OVF_RECORDS re-runs
        got = sc.scan_host(p, buf, opt, dev.WANT_RECORDS)
        assert sc.last_path() == "generic"
        T._same(got, exp, (m, opt))
        for want in (dev.WANT_COUNTLINES, dev.WANT_COUNTMATCH):
            sc2 = dev.Scanner()
            sc2.reserve(0, 10, 2, 1)
            c = sc2.scan_host(p, buf, 0, want)
            ea = o.buffer_scan(pattern, tau, buf, SQ_ALL)
            assert (c["nlines"], c["nmatchlines"]) == (ea["nlines"], ea["nmatchlines"]), (m, want, c)
            assert c["nhits"] == (len(ea["records"]) if want == dev.WANT_COUNTMATCH else ea["nmatchlines"]), (m, want, c)
            sc2.close()
        sc.close()
    p.close()
print("SEGMENTS OK")
"""


def test_segments_and_workspace_growth_on_the_generic_path(request, oracle):
    """64 KiB segments and a workspace of (10 lines, 2 hit lines, 1 record): more than ten segments, a line longer than a segment, lines
    that straddle every seam at a hit -- the OVF_LINES / OVF_HITLINES / OVF_RECORDS re-runs and the line numbering across seams,
    m = 129 (W = 8) and m = 300 (W = 16)."""
    request.getfixturevalue("gpu")
    env = dict(os.environ, SEEQ_SEGMENT_BYTES="65536")
    r = subprocess.run([sys.executable, "-c", SEGMENTS % dict(root=ROOT)], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "SEGMENTS OK" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])


class _SQ:
    """seeqNew / seeqStringMatch of the product library."""

    def __init__(self, capi, pattern, tau):
        self.L = capi.lib()
        self.sq = self.L.seeqNew(pattern.encode(), tau, 0)
        assert self.sq, capi.error_text()

    def match(self, text, opt):
        n = self.L.seeqStringMatch(text.encode("latin-1"), self.sq, opt)
        assert n >= 0
        mt = self.sq.contents.match
        return [(mt[i].start, mt[i].end, mt[i].dist) for i in range(n)]

    def close(self):
        self.L.seeqFree(self.sq)


def test_string_match_long_golden_cases(request, oracle):
    """The reference's long-pattern fixture (tests/golden/ref_long_cases.json) through seeqStringMatch: k_string<2 / 4 / 8 / 16>."""
    with open(os.path.join(GOLDEN, "ref_long_cases.json")) as f:
        cases = json.load(f)
    assert sum(any(c["hits"]) for c in cases) * 2 >= len(cases)
    request.getfixturevalue("gpu")
    capi = request.getfixturevalue("capi")
    per_w = {}
    for c in cases:
        s = _SQ(capi, c["pattern"], c["tau"])
        w = _words(s.sq.contents.wlen)
        for opt, hits in zip(c["options"], c["hits"]):
            got = s.match(c["text"], opt)
            assert [list(h) for h in got] == hits, (c["pattern"], c["tau"], c["text"], opt)
            per_w[w] = per_w.get(w, 0) + len(hits)
        s.close()
    assert all(per_w.get(w, 0) > 50 for w in (2, 4, 8, 16)), per_w


@pytest.mark.parametrize("m,tau", [(100, 8), (200, 33), (400, 64)], ids=["W4", "W8", "W16"])
def test_string_match_long_patterns_every_size_class(request, oracle, m, tau):
    """seeqStringMatch on either side of k_string's size classes -- read over the link (<= 4 096 bytes), positions shared out over the
    workgroup (<= 32 768), staged in LDS (<= 48 KiB), one lane over device memory beyond -- with SQ_STREAM (newlines skipped: the
    one-lane scan) and a skipped byte under SQ_IGNORE."""
    rng = random.Random(31000 + m)
    pattern = _pattern(rng, m)
    core = _core(pattern)
    work = []
    for n in (1, m - tau - 1, m - tau, 4096, 4097, 32768, 32769, 49152, 49153):
        base = _long_lines(rng, core, tau, (n,))[0] if n > 2 * m + 2 * tau + 320 else (core[tau:] + "A" * n)[:n]
        texts = [(base, (SQ_FIRST, SQ_BEST, SQ_ALL))]
        if n > 40:
            texts.append((base[:n // 3] + "N" + base[n // 3 + 1:2 * n // 3] + "\n" + base[2 * n // 3 + 1:], (SQ_ALL, SQ_ALL | SQ_STREAM, SQ_BEST | SQ_STREAM)))
            texts.append((base[:n // 2] + "!" + base[n // 2 + 1:], (SQ_ALL | SQ_CONVERT, SQ_BEST | SQ_IGNORE, SQ_ALL | SQ_IGNORE)))
        for text, opts in texts:
            for opt in opts:
                work.append((n, text, opt, oracle.string_match(pattern, tau, text, opt)))
    assert sum(1 for w in work if w[3]) * 4 >= 3 * len(work) and sum(len(w[3]) for w in work) > 200
    request.getfixturevalue("gpu")
    s = _SQ(request.getfixturevalue("capi"), pattern, tau)
    for n, text, opt, exp in work:
        assert s.match(text, opt) == exp, (m, tau, n, opt)
    s.close()


def test_multi_and_demux_with_a_long_pattern_in_the_set(request, oracle):
    """seeqdevScanHostMulti / seeqdevScanHostDemux with a set of three patterns one of which has 100 positions: no union automaton, a
    scan per pattern (the long one on the generic path), every pattern's records the oracle's, the demultiplex that of the fold."""
    from test_gpu_demux import _check, _expected
    rng = random.Random(4100)
    barcodes = ["GATTACAGAC", _pattern(rng, 100), "TTGACCGATA"]
    taus = [1, 8, 1]
    cores = [_core(b) for b in barcodes]
    lines = []
    for i in range(1500):
        n = rng.choice([60, 150, 250, 400])
        t = _dna(rng, n)
        for _ in range(rng.choice([0, 1, 1, 2])):
            k = rng.randrange(3)
            cp = _mutate(rng, cores[k], rng.randint(0, taus[k] + 1))
            if n >= len(cp):
                q = rng.randrange(n - len(cp) + 1)
                t = t[:q] + cp + t[q + len(cp):]
        lines.append(_spoil(rng, t) if i % 10 == 0 else t)
    buf = ("\n".join(lines) + "\n").encode("latin-1")
    exp = {opt: [oracle.buffer_scan(b, t, buf, opt) for b, t in zip(barcodes, taus)] for opt in (SQ_BEST, SQ_ALL)}
    assert all(e["nmatchlines"] > 50 for e in exp[SQ_ALL])
    fold = _expected(oracle, barcodes, taus, buf)
    assert all(a > 20 for a in fold[1])

    request.getfixturevalue("gpu")
    from seeq_amd import device as dev
    pats = [dev.Pattern(b, t) for b, t in zip(barcodes, taus)]
    sc = dev.Scanner()
    for opt in (SQ_BEST, SQ_ALL):
        got = sc.scan_host_multi(pats, buf, opt, dev.WANT_RECORDS)
        assert not sc.last_multi_one_pass()
        for k in range(3):
            _same(got[k], exp[opt][k], ("multi", k, opt))
    for want in (dev.WANT_COUNTLINES, dev.WANT_COUNTMATCH):
        got = sc.scan_host_multi(pats, buf, 0, want)
        for k in range(3):
            e = exp[SQ_ALL][k]
            assert got[k]["nmatchlines"] == e["nmatchlines"] and got[k]["nhits"] == (len(e["records"]) if want == dev.WANT_COUNTMATCH else e["nmatchlines"])
    res = sc.demux_host(pats, buf)
    assert not sc.last_multi_one_pass()
    _check(res, fold)
    sc.close()
    for p in pats:
        p.close()


def test_demux_two_512_position_patterns_at_distance_300(request, oracle):
    """Two patterns of 512 positions at tau = 300: distances above 255 in the demux record's 16-bit field, and a runner-up 255 or more
    behind the winner (the margin saturates at 255) next to lines where it is closer."""
    from test_gpu_demux import _check, _expected
    rng = random.Random(512300)
    # a over {A, C}; b = 290 G, then a's tail: b lies exactly 290 from a copy of a (no G in it), a exactly 290 from a copy of b
    a = "".join(rng.choice("AC") for _ in range(512))
    b = "G" * 290 + a[290:]
    barcodes, taus = [a, b], [300, 300]
    lines = []
    for src in (a, b):
        for e in (0, 0, 3, 8, 40, 150):
            lines.append(_place(rng, rng.choice([512, 560, 700]), _mutate(rng, src, e), "inside"))
    # k positions of a lost to T: a at distance k, b at 290 while k <= 290
    lines += ["T" * k + a[k:] for k in (0, 10, 30, 35, 36, 100, 200, 256, 270, 289, 290, 291, 300, 301, 320)]
    lines += [_dna(rng, 300), "", a[:256] + b[256:], _dna(rng, 600)]
    buf = ("\n".join(lines) + "\n").encode()
    fold = _expected(oracle, barcodes, taus, buf)
    rows = fold[0]
    per = [oracle.buffer_scan(p, 300, buf, SQ_BEST) for p in barcodes]
    both = set(per[0]["records"][:, 0].tolist()) & set(per[1]["records"][:, 0].tolist())
    assert any(r[3] > 255 for r in rows), "no winner at a distance above 255"
    assert any(r[5] == 255 and r[0] in both for r in rows), "no runner-up 255 or more behind the winner"
    assert any(0 < r[5] < 255 for r in rows), "no unsaturated margin"

    request.getfixturevalue("gpu")
    from seeq_amd import device as dev
    pats = [dev.Pattern(p, 300) for p in barcodes]
    sc = dev.Scanner()
    _check(sc.demux_host(pats, buf), fold)
    assert not sc.last_multi_one_pass()
    sc.close()
    for p in pats:
        p.close()


def test_cli_and_file_api_with_a_100_position_pattern(request, oracle, tmp_path):
    """`seeq -d 8 -b -f` and `-c` (seeqFileMatch behind both) with a pattern of 100 positions over reads250_small.txt with copies
    planted: stdout is the oracle's compact form (as test_oracle.py::test_golden_cli_compact_and_count builds it)."""
    rng = random.Random(100250)
    pattern = _pattern(rng, 100)
    core = _core(pattern)
    reads = open(os.path.join(GOLDEN, "reads250_small.txt")).read().split("\n")
    for i in range(0, len(reads), 3):
        if len(reads[i]) >= 250:
            reads[i] = _place(rng, 250, _mutate(rng, core, rng.randint(0, 10)), rng.choice(["start", "end", "inside"]))[:250]
    data = "\n".join(reads).encode()
    path = str(tmp_path / "reads250_planted.txt")
    with open(path, "wb") as f:
        f.write(data)
    exp = oracle.buffer_scan(pattern, 8, data, SQ_BEST)
    assert 100 < exp["nmatchlines"] < len(reads) // 3
    compact = "".join("%d:%d-%d:%d\n" % (r[0], r[1], r[2] - 1, r[3]) for r in exp["records"].tolist())

    request.getfixturevalue("gpu")
    capi = request.getfixturevalue("capi")
    r = subprocess.run([capi.CLI_PATH, "-d", "8", "-b", "-f", pattern, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == compact, r.stderr[-500:]
    r = subprocess.run([capi.CLI_PATH, "-d", "8", "-c", pattern, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "%d\n" % exp["nmatchlines"], (r.stdout, r.stderr[-500:])
    # seeqFileMatch line by line: every line's hits
    L = capi.lib()
    f = L.seeqOpen(path.encode())
    sq = L.seeqNew(pattern.encode(), 8, 0)
    assert f and sq
    rec = []
    while L.seeqFileMatch(f, sq, SQ_BEST, 1) > 0:           # SQ_MATCH: the next line with a hit
        mt = L.seeqMatchIter(sq)
        rec.append((f.contents.line, mt.contents.start, mt.contents.end, mt.contents.dist))
    assert rec == [tuple(r) for r in exp["records"].tolist()]
    L.seeqClose(f)
    L.seeqFree(sq)


def _fuzz_case(rng, oracle):
    """One random case: pattern of 63 .. 512 positions, tau 0 .. min(m - 1, 120), ragged lines and now and then a long one, options at
    random.  -> what the GPU side needs, the oracle's answers included."""
    m = rng.choice([rng.randint(63, 512), rng.choice(LENGTHS), rng.randint(63, 130)])
    tau = rng.choice([rng.randint(0, min(m - 1, 120)), rng.randint(0, 12), min(m - 1, rng.choice([31, 32, 33, 63, 64, 65]))])
    pattern = _pattern(rng, m, rng.choice(["random"] * 8 + ["periodic", "single"]))
    core = _core(pattern)
    budget = min(60000, 12_000_000 // m)
    lines, _ = _ragged_lines(rng, oracle, pattern, tau, budget // 2 if rng.random() < 0.3 else budget)
    if budget >= 45000 and rng.random() < 0.5:
        lines.insert(rng.randrange(len(lines)), _long_lines(rng, core, tau, (rng.randint(40000, budget),))[0])
    rng.shuffle(lines)
    fasta = rng.random() < 0.25
    if fasta:
        lines = _as_fasta(rng, lines, core)
    buf = ("\n".join(lines) + ("\n" if rng.random() < 0.7 else "")).encode("latin-1")
    opt = rng.choice([SQ_FIRST, SQ_BEST, SQ_ALL, SQ_ALL]) | rng.choice([SQ_FAIL, SQ_CONVERT, SQ_IGNORE])
    exp = oracle.buffer_scan(pattern, tau, buf, opt, fasta=fasta)
    expa = exp if opt & 3 == SQ_ALL else oracle.buffer_scan(pattern, tau, buf, (opt & ~3) | SQ_ALL, fasta=fasta)
    return dict(m=m, tau=tau, pattern=pattern, buf=buf, opt=opt, fasta=fasta, exp=exp, expa=expa)


def _fuzz(request, oracle, seed, ncases):
    rng = random.Random(seed)
    cases = [_fuzz_case(rng, oracle) for _ in range(ncases)]
    empty = sum(1 for c in cases if not len(c["exp"]["records"]))
    assert 5 * empty <= ncases, (seed, empty, ncases)       # at most one case in five without a record
    request.getfixturevalue("gpu")
    from seeq_amd import device as dev
    sc = dev.Scanner()
    for i, c in enumerate(cases):
        what = (seed, i, c["m"], c["tau"], c["opt"], c["fasta"], c["pattern"])
        pat = dev.Pattern(c["pattern"], c["tau"])
        fl = FASTA if c["fasta"] else 0
        got = sc.scan_host(pat, c["buf"], c["opt"] | fl, dev.WANT_RECORDS)
        assert sc.last_path() == "generic", what
        _same(got, c["exp"], what)
        _counts_same(sc, dev, pat, c["buf"], (c["opt"] & ~3) | fl, c["expa"], what)
        pat.close()
    sc.close()
    return empty


def test_long_pattern_fuzz(request, oracle):
    """Random long patterns, distances, line kinds and options: one fixed seed and one fresh seed per run (SEEQ_FUZZ_SEED replays it)."""
    e1 = _fuzz(request, oracle, 20261016, 25)
    env = os.environ.get("SEEQ_FUZZ_SEED")
    seed = int(env) if env else (int(time.time() * 1000) ^ os.getpid()) % 1_000_000_007
    print("SEEQ_FUZZ_SEED=%d" % seed)
    e2 = _fuzz(request, oracle, seed, 25)
    print("long-pattern fuzz: %d + %d of 25 + 25 cases without a record" % (e1, e2))
