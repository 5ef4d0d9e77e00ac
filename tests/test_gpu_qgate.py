"""GPU (-m gpu): the base-quality gate (seeqdevScanQualityGate; seeq_qgate.h: kinds, totals, ordered compaction, all on the device) against
the rule restated in Python (test_qgate_host.py::py_gate) over spans the code under test did not cut.  Reads are built as in
test_gpu_tally.py -- prefix + exact left flank + chosen insert + exact right flank + suffix -- and wrapped as FASTQ records with quality
strings the test draws itself; the test knows where every planted insert lies (offset of its sequence line, start, end) and every case
first asserts that the inserts call found exactly those: a vacuous case fails."""
import collections
import ctypes as C
import errno
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle.pyoracle import SQ_ALL, SQ_BEST
from test_gpu_strands import _step
from test_gpu_tally import LEFT, RIGHT
from test_gpu_tally import _same as _same_tally
from test_gpu_tally_grouped import FC, FD, _held_of
from test_gpu_tally_grouped import _same as _same_grouped
from test_gpu_tally_library import _same as _same_library
from test_qgate_host import DISTANCES, FAR, LONG, LOW, MISFIT, PASS, PLUS_LENS, py_gate
from test_tally_library_host import PyLibrary

pytestmark = pytest.mark.gpu
T = int(re.search(r"#define\s+SEEQ_QGATE_TILE\s+(\d+)", open(os.path.join(ROOT, "seeq_amd", "csrc", "seeq_qgate.h")).read()).group(1))
COUNTS = ("nspans", "npassed", "nlow", "nlong", "nfar", "nmisfit", "low_bases")
RC_LEFT = LEFT[::-1].translate(str.maketrans("ACGT", "TGCA"))

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
    ps = dict(L=dev.Pattern(LEFT, 0), R=dev.Pattern(RIGHT, 0), C=dev.Pattern(FC, 0), D=dev.Pattern(FD, 0))
    yield ps
    for p in ps.values():
        p.close()


def _cuda(buf):
    import torch
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


# ---- reads: FASTQ records whose planted spans the test knows ----
class Reads:
    """FASTQ text record by record.  rows: per record with a planted insert (record number 1-based, offset of its sequence line, start, end
    of the insert); left, right: the same for the two flanks themselves (the hits of LEFT and of RIGHT)."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.buf, self.rows, self.left, self.right, self.nrec = bytearray(), [], [], [], 0

    def bases(self, n):
        return bytes(self.rng.choice(b"ACGT") for _ in range(n))

    def quals(self, n, p_low=0.04):
        """n quality bytes: 'I' (Q40) mostly, a byte of Q2 .. Q19 with probability p_low, now and then one exactly at Q20."""
        return bytes(self.rng.randrange(35, 53) if self.rng.random() < p_low else 53 if self.rng.random() < 0.05 else 73 for _ in range(n))

    def add(self, insert, prefix=None, suffix=None, plus=b"+", qual=None, newline=True, le=LEFT.encode(), ri=RIGHT.encode(), p_low=0.04):
        """A record whose sequence line is prefix + le + insert + ri + suffix (insert None: prefix + suffix alone, no flanks)."""
        prefix = self.bases(self.rng.randrange(6)) if prefix is None else prefix
        suffix = self.bases(self.rng.randrange(6)) if suffix is None else suffix
        seq = prefix + (le + insert + ri if insert is not None else b"") + suffix
        self.nrec += 1
        self.buf += b"@r%d\n" % self.nrec
        off = len(self.buf)
        if insert is not None:
            self.rows.append((self.nrec, off, len(prefix) + len(le), len(prefix) + len(le) + len(insert)))
            self.left.append((self.nrec, off, len(prefix), len(prefix) + len(le)))
            self.right.append((self.nrec, off, self.rows[-1][3], self.rows[-1][3] + len(ri)))
        qual = self.quals(len(seq), p_low) if qual is None else qual
        self.buf += seq + b"\n" + plus + b"\n" + qual + (b"\n" if newline else b"")
        return off

    def text(self):
        return bytes(self.buf)


def _expected(text, rows, **kw):
    """rows of (record, off, start, end) -> (kinds, counts) by the Python rule."""
    kinds, low = [], 0
    for _, off, start, end in rows:
        kind, nlow = py_gate(text, off, start, end, **kw)
        kinds.append(kind)
        low += nlow
    cnt = dict(nspans=len(rows), npassed=kinds.count(PASS), nlow=kinds.count(LOW), nlong=kinds.count(LONG), nfar=kinds.count(FAR),
               nmisfit=kinds.count(MISFIT), low_bases=low)
    return kinds, cnt


def _same(res, kinds, cnt, src_rec, src_off):
    """A quality_gate() result (copy=True) against the rule's kinds and counts and the SOURCE's records [n, 4] u32 and offsets."""
    assert {k: res[k] for k in COUNTS} == cnt
    assert res["nspans"] == res["npassed"] + res["nlow"] + res["nlong"] + res["nfar"] + res["nmisfit"]
    assert res["kinds"].dtype == np.uint8 and res["kinds"].tolist() == kinds
    keep = np.array(kinds, dtype=np.int64) == PASS
    assert res["records"].dtype == np.uint32 and res["records"].shape == (cnt["npassed"], 4)
    assert res["records"].tobytes() == np.ascontiguousarray(src_rec[keep]).tobytes()      # in order, byte for byte
    assert res["offsets"].tobytes() == np.ascontiguousarray(src_off[keep]).tobytes()


def _insert_source(s, flanks, t, rows, fastq=True, what=""):
    """The inserts call over t, its result held against the planted rows -> the source's records [n, 4] u32 and offsets."""
    from seeq_amd import device as dev
    res = s.inserts_tensor(flanks["L"], flanks["R"], t, SQ_BEST | (dev.SEEQDEV_FASTQ if fastq else 0), copy=False)
    assert res["ninserts"] == len(rows), (what, res)
    rec = s.insert_records(len(rows))
    off = s.insert_offsets(len(rows))
    assert off.tolist() == [r[1] for r in rows] and rec["start"].tolist() == [r[2] for r in rows] and rec["end"].tolist() == [r[3] for r in rows], what
    if fastq:
        assert rec["line"].tolist() == [r[0] for r in rows], what
    return rec.view(np.uint32).reshape(-1, 4), off


def _gate_inserts(sc, flanks, reads, what, fastq=True, **kw):
    """inserts + quality_gate over the reads, both checked -> (result, tensor, kinds)."""
    text = reads.text()
    t = _cuda(text)
    kinds, cnt = _expected(text, reads.rows, **kw)
    got = {}

    def call(s):
        src = _insert_source(s, flanks, t, reads.rows, fastq, what)
        return s.quality_gate(t, **kw), src

    def check(s, pair):
        res, (rec, off) = pair
        _same(res, kinds, cnt, rec, off)
        got["res"] = res
    _go(sc, what, call, check)
    return got["res"], t, kinds


def _random_reads(n, seed, longest=14, p_low=0.04):
    reads = Reads(seed)
    for i in range(n):
        reads.add(reads.bases(reads.rng.randrange(0, longest + 1)), p_low=p_low)
        if i % 50 == 7:
            reads.add(None, prefix=reads.bases(30))         # a record without an insert
    return reads


# ---- tile shapes ----
@pytest.mark.parametrize("n", [1, T - 1, T, T + 1, 4 * T + 4])
def test_span_counts(gpu, capi, flanks, n):
    """Around the tile T and more than four tiles: the counts, the kind of every source record, the gated records and offsets."""
    from seeq_amd import device as dev
    sc = dev.Scanner()
    res, _, kinds = _gate_inserts(sc, flanks, _random_reads(n, n), "%d spans" % n)
    assert res["nspans"] == n
    if n > 1:
        assert 0 < res["npassed"] < n and res["nlow"] > 0 and res["low_bases"] >= res["nlow"]
    assert sc.gated_device_ptr() if res["npassed"] else True
    sc.close()


# ---- geometry ----
def _geometry_reads(seed, tail):
    """Every suffix length d of test_qgate_host.py's distances x every '+' line length: the right flank's hit ends d bytes before the end of
    its line, the insert d + 20 bytes before it.  Read lengths 20 .. 300; inserts of 0, 1, 16, 17, 31 (gated) and 32, 40 (long) bytes; a
    quality line one byte short and one byte long (misfit); then the last record by `tail`, a short one, so that its quality bytes lie in
    the text's last 32 bytes."""
    reads = Reads(seed)
    le, ri = len(LEFT), len(RIGHT)
    for d in DISTANCES:
        for pl in PLUS_LENS:
            reads.add(reads.bases(12), prefix=reads.bases(3), suffix=reads.bases(d), plus=b"+" + reads.bases(pl - 1), p_low=0.03)
    for total in (20, 21, 40, 63, 64, 65, 150, 151, 299, 300):
        if total >= le + ri:
            ins = reads.bases(min(12, total - le - ri))
            reads.add(ins, prefix=b"", suffix=reads.bases(total - le - ri - len(ins)))
        else:
            reads.add(None, prefix=reads.bases(total), suffix=b"")         # (too short for the flank pair: no span)
    for ln in (0, 1, 16, 17, 31, 32, 40):
        reads.add(reads.bases(ln), p_low=0.02)
    n = le + ri + 10
    reads.add(reads.bases(10), prefix=b"", suffix=b"", qual=reads.quals(n - 1))
    reads.add(reads.bases(10), prefix=b"", suffix=b"", qual=reads.quals(n + 1))
    reads.add(reads.bases(8))
    off = reads.add(reads.bases(6), prefix=b"AC", suffix=b"", newline=False, p_low=0.1)
    n = 2 + le + 6 + ri
    cut = dict(whole=len(reads.buf), after_seq=off + n + 1, after_plus=off + n + 3, mid_qual=off + n + 3 + n // 2, one_short=len(reads.buf) - 1)[tail]
    del reads.buf[cut:]
    return reads


@pytest.mark.parametrize("reach", [64, 1024])
@pytest.mark.parametrize("tail", ["whole", "after_seq", "after_plus", "mid_qual", "one_short"])
def test_geometry(gpu, capi, flanks, tail, reach):
    """One text of every line shape and one of the text's ends, gated over its inserts and over the hits of its right flank (which end 0,
    15, 16, 17, ... bytes before the end of their line; the last one's quality bytes are the text's last 20)."""
    from seeq_amd import device as dev
    reads = _geometry_reads(7, tail)
    text = reads.text()
    sc = dev.Scanner()
    res, t, kinds = _gate_inserts(sc, flanks, reads, "geometry, %s, reach %d" % (tail, reach), reach=reach, max_low=1)
    assert res["nlong"] == 2 and res["nmisfit"] >= 2 + (tail != "whole") and res["npassed"] > 10 and res["nlow"] > 0
    assert (res["nfar"] > 10) == (reach == 64) and (reach == 64 or res["nfar"] == 0)      # 64 bytes end short of many a second newline, 1 024 of none
    assert kinds[-1] in ((PASS, LOW) if tail == "whole" else (MISFIT,))
    # the hits of the right flank
    hkinds, hcnt = _expected(text, reads.right, reach=reach, max_low=1)
    assert hkinds[-1] in ((PASS, LOW) if tail == "whole" else (MISFIT,))

    def hits(s):
        got = s.scan_tensor(flanks["R"], t, SQ_BEST | dev.SEEQDEV_FASTQ, dev.WANT_RECORDS)
        assert got["nrecords"] == len(reads.right)
        rec, off = s.records(len(reads.right)), s.record_offsets(len(reads.right))
        assert [tuple(r) for r in rec[:, :3].tolist()] == [(r[0], r[2], r[3]) for r in reads.right] and off.tolist() == [r[1] for r in reads.right]
        return s.quality_gate(t, source="hits", reach=reach, max_low=1), rec, off
    _go(sc, "geometry, %s, reach %d: hits of the right flank" % (tail, reach), hits, lambda s, tr: _same(tr[0], hkinds, hcnt, tr[1], tr[2]))
    # e2 at exactly p + reach - 1 is decided, at p + reach it is not: the first record, by its own geometry
    _, off, start, end = reads.rows[0]
    e2 = text.index(b"\n", text.index(b"\n", off + end) + 1) - (off + end)
    _insert_source(sc, flanks, t, reads.rows, True, "again")
    at = sc.quality_gate(t, reach=e2 + 1, max_low=1)["kinds"]
    short = sc.quality_gate(t, reach=e2, max_low=1)["kinds"]
    assert at[0] == kinds[0] and kinds[0] in (PASS, LOW) and short[0] == FAR
    assert at.tolist() == _expected(text, reads.rows, reach=e2 + 1, max_low=1)[0] and short.tolist() == _expected(text, reads.rows, reach=e2, max_low=1)[0]
    sc.close()


@pytest.mark.parametrize("kw", [dict(min_qual=20, base=33, max_low=0), dict(min_qual=20, base=33, max_low=2), dict(min_qual=7, base=64, max_low=1),
                                dict(min_qual=0, base=33, max_low=0), dict(min_qual=41, base=33, max_low=31)],
                         ids=lambda kw: "q%d_b%d_k%d" % (kw["min_qual"], kw["base"], kw["max_low"]))
def test_thresholds(gpu, capi, flanks, kw):
    """The bar, the base and the allowance: a byte exactly at base + min_qual passes, one below it is low (the reads' quality strings hold
    bytes at Q20 = 53 and at 35 .. 52); base 64 puts every 'I' above a bar of 71 and every other byte below it."""
    from seeq_amd import device as dev
    sc = dev.Scanner()
    res, _, _ = _gate_inserts(sc, flanks, _random_reads(T + 40, 77, p_low=0.08), "thresholds %s" % (kw,), **kw)
    if kw["min_qual"] == 0:
        assert res["npassed"] == res["nspans"] and res["low_bases"] == 0
    if kw["max_low"] == 31:
        assert res["npassed"] == res["nspans"] and res["low_bases"] > 0      # (every byte is low, every span is allowed 31 of them)
    sc.close()


# ---- both sources ----
def test_inserts_as_plain_lines(gpu, capi, flanks):
    """Without SEEQDEV_FASTQ the four lines of a record are four lines: the inserts of the sequence lines are found under other line
    numbers, and the gate, which is positional from the span on, decides the same."""
    from seeq_amd import device as dev
    reads = _random_reads(T + 9, 5)
    sc = dev.Scanner()
    plain, _, kinds = _gate_inserts(sc, flanks, reads, "plain lines", fastq=False)
    fq, _, kinds2 = _gate_inserts(sc, flanks, reads, "the same under SEEQDEV_FASTQ", fastq=True)
    assert kinds == kinds2 and {k: plain[k] for k in COUNTS} == {k: fq[k] for k in COUNTS}
    assert (plain["records"][:, 0] == 4 * (fq["records"][:, 0] - 1) + 2).all() and plain["offsets"].tobytes() == fq["offsets"].tobytes()
    sc.close()


def test_hits_as_the_source(gpu, capi, flanks):
    """source="hits": the matches of the left flank under SEEQDEV_FASTQ (SQ_BEST), then of a both-strands call (SQ_ALL) over reads
    that carry the flank or its reverse complement: bit 31 of `dist` survives the gate."""
    from seeq_amd import device as dev
    reads = _random_reads(T + 30, 9, p_low=0.01)
    text = reads.text()
    t = _cuda(text)
    sc = dev.Scanner()
    kinds, cnt = _expected(text, reads.left)
    assert 0 < cnt["npassed"] < len(reads.left)

    def plain(s):
        got = s.scan_tensor(flanks["L"], t, SQ_BEST | dev.SEEQDEV_FASTQ, dev.WANT_RECORDS)
        assert got["nrecords"] == len(reads.left)
        rec, off = s.records(len(reads.left)), s.record_offsets(len(reads.left))
        assert [tuple(r) for r in rec[:, :3].tolist()] == [(r[0], r[2], r[3]) for r in reads.left] and off.tolist() == [r[1] for r in reads.left]
        return s.quality_gate(t, source="hits"), rec, off
    _go(sc, "hits of a plain SEEQDEV_FASTQ scan", plain, lambda s, tr: _same(tr[0], kinds, cnt, tr[1], tr[2]))
    assert sc.records(len(reads.left))[:, :3].tolist() == [[r[0], r[2], r[3]] for r in reads.left]      # the record arrays are what they were
    # both strands: every other read carries the reverse complement of the flank
    both = Reads(10)
    for i in range(T + 30):
        both.add(both.bases(8), le=(RC_LEFT if i % 2 else LEFT).encode(), p_low=0.01)
    btext = both.text()
    bt = _cuda(btext)
    bkinds, bcnt = _expected(btext, both.left)

    def strands(s):
        got = s.strands_tensor(flanks["L"], bt, SQ_ALL | dev.SEEQDEV_FASTQ, dev.WANT_RECORDS, copy=False)
        assert got["nrecords"] == len(both.left), got
        rec, off = s.records(len(both.left)), s.record_offsets(len(both.left))
        assert [tuple(r) for r in rec[:, :3].tolist()] == [(r[0], r[2], r[3]) for r in both.left] and off.tolist() == [r[1] for r in both.left]
        assert ((rec[:, 3] >> 31) == np.arange(len(both.left)) % 2).all()
        return s.quality_gate(bt, source="hits"), rec, off
    got = {}

    def check(s, tr):
        _same(tr[0], bkinds, bcnt, tr[1], tr[2])
        got["res"] = tr[0]
    _go(sc, "hits of a both-strands call", strands, check)
    minus = got["res"]["records"][:, 3] >> 31
    assert 0 < int(minus.sum()) < len(minus) and (minus == (got["res"]["records"][:, 0] - 1) % 2).all()
    sc.close()


# ---- composition: the five tally entries over the gated spans ----
def _spans(text, rows, kinds):
    return [text[off + st:off + en] for (_, off, st, en), k in zip(rows, kinds) if k == PASS]


def test_tally_and_library_tally_of_the_gated_spans(gpu, capi, flanks):
    from seeq_amd import device as dev
    rng = random.Random(3)
    guides = [bytes(rng.choice(b"ACGT") for _ in range(12)) for _ in range(30)]
    reads = Reads(3)
    for _ in range(2 * T + 11):
        g = bytearray(rng.choice(guides))
        if rng.random() < 0.1:
            g[rng.randrange(12)] = rng.choice(b"ACGTN")
        reads.add(bytes(g) if rng.random() < 0.97 else reads.bases(rng.choice((0, 5, 33))), p_low=0.03)
    sc = dev.Scanner()
    res, t, kinds = _gate_inserts(sc, flanks, reads, "guides")
    spans = _spans(reads.text(), reads.rows, kinds)
    assert 100 < len(spans) < len(reads.rows) - 100
    _same_tally(sc.tally(t, source="gated"), spans)
    ungated = sc.tally(t)
    assert ungated["nspans"] == len(reads.rows) and ungated["ndistinct"] >= sc.tally(t, source="gated")["ndistinct"]
    lib = PyLibrary(guides)
    sc.set_library(lib.seqs, 1)
    _same_library(sc.tally_library(t, source="gated"), lib, spans, 1)
    sc.close()


def test_grouped_tally_of_gated_guides_and_gated_umis(gpu, capi, flanks):
    """The guide between LEFT and RIGHT is held gated, the UMI between FC and FD is a member gated: a read whose guide fails the gate leaves
    its UMI ungrouped, one whose UMI fails is no member.  Then the same with the guides assigned to a library (tally_hold_library)."""
    from seeq_amd import device as dev
    rng = random.Random(4)
    guides = [bytes(rng.choice(b"ACGT") for _ in range(20)) for _ in range(7)]
    umis = [bytes(rng.choice(b"ACGT") for _ in range(10)) for _ in range(40)]
    reads, urows = Reads(4), []
    for _ in range(T + 60):
        g, u = rng.choice(guides), rng.choice(umis)
        prefix = reads.bases(rng.randrange(4))
        suffix = reads.bases(3) + FC.encode() + u + FD.encode() + reads.bases(rng.randrange(4))
        off = reads.add(g, prefix=prefix, suffix=suffix, p_low=0.015)
        ustart = len(prefix) + len(LEFT) + 20 + len(RIGHT) + 3 + len(FC)
        urows.append((reads.nrec, off, ustart, ustart + 10))
    text = reads.text()
    t = _cuda(text)
    gkinds, _ = _expected(text, reads.rows)
    ukinds, ucnt = _expected(text, urows)
    gspans = [(r[0], text[r[1] + r[2]:r[1] + r[3]]) for r, k in zip(reads.rows, gkinds) if k == PASS]
    uspans = [(r[0], text[r[1] + r[2]:r[1] + r[3]]) for r, k in zip(urows, ukinds) if k == PASS]
    guide_failed = {r[0] for r, k in zip(reads.rows, gkinds) if k != PASS}
    assert len(guide_failed) > 50 and len({ln for ln, _ in uspans} & guide_failed) > 20 and len(uspans) < len(urows) - 50
    opt = SQ_BEST | dev.SEEQDEV_FASTQ
    sc = dev.Scanner()
    lib = PyLibrary(guides)

    def run(s, library):
        _insert_source(s, flanks, t, reads.rows, True, "guides")
        g = s.quality_gate(t, copy=False)
        assert g["npassed"] == len(gspans)
        hold = s.tally_hold_library(t, source="gated") if library else s.tally_hold(t, source="gated")
        res = s.inserts_tensor(flanks["C"], flanks["D"], t, opt, copy=False)
        assert res["ninserts"] == len(urows)
        rec, off = s.insert_records(len(urows)), s.insert_offsets(len(urows))
        assert [(int(a), int(o), int(b), int(c)) for a, o, b, c in zip(rec["line"], off, rec["start"], rec["end"])] == urows
        u = s.quality_gate(t, copy=False)
        assert {k: u[k] for k in COUNTS} == ucnt
        return hold, s.tally_grouped(t, source="gated")

    def check_plain(s, pair):
        hold, res = pair
        held, hcnt = _held_of(gspans)
        assert hold == hcnt
        _same_grouped(res, held, uspans)
        assert res["nungrouped"] == sum(1 for ln, _ in uspans if ln in guide_failed) > 20
    _go(sc, "hold gated, members gated", lambda s: run(s, False), check_plain)

    def check_library(s, pair):
        hold, res = pair
        cnt, _, ids = lib.tally([b for _, b in gspans], 1)
        assert {k: hold[k] for k in cnt if k != "ndistinct"} == {k: v for k, v in cnt.items() if k != "ndistinct"}
        _same_grouped(res, [(ln, i) for (ln, _), i in zip(gspans, ids)], uspans)
        assert res["ngroups"] == len(guides)
    sc.set_library(lib.seqs, 1)
    _go(sc, "hold gated against the library, members gated", lambda s: run(s, True), check_library)
    sc.close()


# ---- state ----
def test_state_around_a_gate(gpu, capi, flanks):
    """A gate leaves the record arrays, the inserts result, a held column and the last tally table as they were; its own arrays answer the
    same after a further scan and a further inserts call; a second gate replaces them; a gate that passes nothing is an empty result."""
    from seeq_amd import device as dev
    reads = _random_reads(T + 50, 12)
    text = reads.text()
    t = _cuda(text)
    sc = dev.Scanner()
    sc.set_profiling(True)
    # hits first (a held column of the flank hits), then the inserts and their table
    n_left = len(reads.left)
    assert sc.scan_tensor(flanks["L"], t, SQ_BEST | dev.SEEQDEV_FASTQ, dev.WANT_RECORDS)["nrecords"] == n_left
    hold = sc.tally_hold(t, source="hits")
    src = _insert_source(sc, flanks, t, reads.rows)
    table = sc.tally(t)
    before = (src[0].tobytes(), src[1].tobytes(), sc.insert_text(t).cpu().numpy().tobytes(), sc.tally_table(table["ndistinct"]).tobytes())
    kinds, cnt = _expected(text, reads.rows)
    res = sc.quality_gate(t)
    _same(res, kinds, cnt, *src)
    assert sc.last_quality_gate_ms() > 0
    after = (sc.insert_records(len(reads.rows)).tobytes(), sc.insert_offsets(len(reads.rows)).tobytes(), sc.insert_text(t).cpu().numpy().tobytes(),
             sc.tally_table(table["ndistinct"]).tobytes())
    assert after == before
    with pytest.raises(dev.SeeqDeviceError):
        sc.fetch()                                          # an inserts call leaves nothing to fetch, and a gate does not change that
    # the held column: the grouped tally over the gated inserts pairs every passed insert with its line's flank hit
    grouped = sc.tally_grouped(t, source="gated")
    assert grouped["npaired"] == cnt["npassed"] and grouped["ngroups"] == 1 and hold["nheld"] == n_left
    # a further scan and a further inserts call (of another flank pair: nothing found): the gated arrays answer the same
    gated = (res["records"].tobytes(), res["offsets"].tobytes(), res["kinds"].tobytes())
    other = _cuda(b"ACGTACGTACGT\n" * 300)
    assert sc.scan_tensor(flanks["L"], other, SQ_BEST, dev.WANT_RECORDS)["nrecords"] == 0
    assert sc.inserts_tensor(flanks["C"], flanks["D"], other, SQ_BEST, copy=False)["ninserts"] == 0
    assert (sc.gated_records(cnt["npassed"]).tobytes(), sc.gated_offsets(cnt["npassed"]).tobytes(), sc.gate_kinds(len(kinds)).tobytes()) == gated
    assert sc.gated_records(3, first=2).tobytes() == res["records"][2:5].tobytes()
    _same_tally(sc.tally(t, source="gated"), _spans(text, reads.rows, kinds))      # ... with the text the gated records were found in
    # a second gate (another bar, over the inserts of the first text again) replaces them
    _insert_source(sc, flanks, t, reads.rows)
    kinds2, cnt2 = _expected(text, reads.rows, max_low=3)
    res2 = sc.quality_gate(t, max_low=3)
    _same(res2, kinds2, cnt2, *src)
    assert cnt2["npassed"] > cnt["npassed"]
    with pytest.raises(dev.SeeqDeviceError):
        sc.gated_records(1, first=cnt2["npassed"])          # beyond the new result
    # a gate that passes nothing: a valid empty result, and a tally over it launches nothing
    none = sc.quality_gate(t, min_qual=41, max_low=0, base=33)
    spans_with_bases = sum(1 for r in reads.rows if r[3] > r[2])
    assert none["npassed"] == len(reads.rows) - spans_with_bases - none["nlong"] and len(none["records"]) == none["npassed"]
    empty = Reads(13)
    for _ in range(70):
        empty.add(empty.bases(9), qual=None, p_low=1.0)
    et = _cuda(empty.text())
    _insert_source(sc, flanks, et, empty.rows)
    zero = sc.quality_gate(et)
    assert zero["npassed"] == 0 and zero["nlow"] == 70 and len(zero["records"]) == 0 and len(zero["kinds"]) == 70
    tl = sc.tally(et, source="gated")
    assert tl["nspans"] == 0 and tl["ndistinct"] == 0 and len(tl["keys"]) == 0 and sc.last_tally_ms() == 0
    sc.close()


def test_the_staged_text_of_a_host_inserts_call(gpu, capi, flanks):
    """inserts_host, then the gate and the tally without a tensor: the context's staged text."""
    from seeq_amd import device as dev
    reads = _random_reads(300, 14)
    text = reads.text()
    sc = dev.Scanner()
    res = sc.inserts_host(flanks["L"], flanks["R"], text, SQ_BEST | dev.SEEQDEV_FASTQ)
    assert res["ninserts"] == len(reads.rows)
    kinds, cnt = _expected(text, reads.rows)
    g = sc.quality_gate()
    assert {k: g[k] for k in COUNTS} == cnt and g["kinds"].tolist() == kinds
    _same_tally(sc.tally(source="gated"), _spans(text, reads.rows, kinds))
    sc.close()


# ---- errors ----
def _raw_gate(sc, capi, source, t, nbytes=None):
    cnt = capi.seeqdev_qgate_counts_t()
    C.set_errno(0)
    rc = sc._lib.seeqdevScanQualityGate(sc._h, source, C.c_void_p(t.data_ptr()) if t is not None else None,
                                        (t.numel() if nbytes is None else nbytes) if t is not None else 0, 20, 33, 0, 1024, C.byref(cnt))
    return rc, C.get_errno()


def test_a_span_beyond_the_text_is_an_argument_error(gpu, capi, flanks):
    """nbytes cut short of the last insert: a span reaches past it, EIO.  An argument check -- the kernel compares before it loads -- so
    nothing faults and the context goes on: no gate is completed, the same call with the right size gives the result, a scan is right."""
    from seeq_amd import device as dev
    reads = _random_reads(T + 9, 41)
    text = reads.text()
    t = _cuda(text)
    sc = dev.Scanner()
    src = _insert_source(sc, flanks, t, reads.rows)
    end_of_last = reads.rows[-1][1] + reads.rows[-1][3]
    assert _raw_gate(sc, capi, capi.SEEQDEV_TALLY_INSERTS, t, end_of_last - 1) == (-1, errno.EIO)
    assert "outside" in capi.error_text()
    with pytest.raises(dev.SeeqDeviceError):
        sc.tally(t, source="gated")                         # a failed gate is no completed gate
    with pytest.raises(dev.SeeqDeviceError):
        sc.gate_kinds(1)
    assert _raw_gate(sc, capi, capi.SEEQDEV_TALLY_GATED, t) == (-1, errno.EINVAL)
    kinds, cnt = _expected(text, reads.rows)
    _same(sc.quality_gate(t), kinds, cnt, *src)
    got = sc.scan_tensor(flanks["L"], t, SQ_BEST | dev.SEEQDEV_FASTQ, dev.WANT_RECORDS)
    assert got["nrecords"] == len(reads.left) and sc.records(len(reads.left))[:, :3].tolist() == [[r[0], r[2], r[3]] for r in reads.left]
    counter = collections.Counter(kinds)
    assert counter[PASS] == cnt["npassed"]
    sc.close()
