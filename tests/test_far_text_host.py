"""CPU: the far text of tests/far_text.py is what it claims, its forward-mapped reference is the oracle's answer, and it is LIVE -- behind
tests/test_gpu_far_text.py, which puts 4 GiB on the device and never lets a reference look at them.

  composition   the same Layout with the boundaries scaled to 2^21, 0x1E0000 and 2^22 (the seam BELOW 2^21: the blocks change their
                order), and once more with the seam between the two as on the device (0x3C0000): the oracle over the WHOLE scaled text
                equals the compact reference mapped forward, for the scans (BEST and ALL), both strands, the joined insert rows and the
                demux, in both views; and a Part B row at a scaled repeat count against its replicated reference;
  phases        what every boundary of the true layout cuts (Layout.phases asserts; printed);
  liveness      over the true layout, a reference that keeps a line offset in 32 bits, or reads it as int32, or reads the
                segment-relative positions of block 2 as signed, answers otherwise: record offsets, insert text, tally table, library
                counts, gate kinds, anchored cuts;
  FarBytes      slices, single bytes and find across every piece edge against a materialised 2 MiB neighbourhood."""
import collections
import random

import numpy as np
import pytest

import far_text as F
import kernel_instances as K
import text_window as W
from oracle.pyoracle import SQ_ALL, SQ_BEST
from test_anchor_host import AFTER, LINE, py_anchor_all
from test_gpu_inserts import _host_text
from test_gpu_text_window import FLANKS, INSERT_CASES, Ref
from test_tally_library_host import PyLibrary

SCALED = {"seam below": dict(B31=1 << 21, SEAM=0x1E0000, B32=1 << 22), "seam between": dict(B31=1 << 21, SEAM=0x3C0000, B32=1 << 22)}
VIEWS = {"fastq": True, "plain": False}


@pytest.fixture(scope="module")
def true_layouts(oracle):
    out = {}
    for name, fastq in VIEWS.items():
        lay = F.Layout(oracle, fastq)
        out[name] = (lay, F.FarRef(oracle, lay))
    return out


# ---- composition ----
@pytest.mark.parametrize("bounds", list(SCALED))
@pytest.mark.parametrize("view", list(VIEWS))
def test_the_mapped_reference_is_the_oracle_over_the_whole_text(oracle, view, bounds):
    fastq = VIEWS[view]
    lay = F.Layout(oracle, fastq, SCALED[bounds])
    far = F.FarRef(oracle, lay)
    for ln in lay.phases(far):
        print("scaled, %s, %s: %s" % (view, bounds, ln))
    text = lay.far[:]
    assert len(text) == len(lay.far) and text.count(lay.block) == 3
    whole = Ref(oracle, text, fastq)
    assert len(whole.offs) - 1 == lay.nlines
    for name in FLANKS:
        for mode in (SQ_BEST, SQ_ALL):
            a, b = whole.scan(name, mode), far.scan(name, mode)
            assert a["nlines"] == b["nlines"] == lay.nlines and a["nmatchlines"] == b["nmatchlines"] > 100
            assert np.array_equal(a["records"], b["records"]) and b["records"].dtype == np.uint64
            assert [whole.offs[int(ln)] for ln in a["records"][:, 0]] == [far.offs[int(ln)] for ln in b["records"][:, 0]]
    for mode in (SQ_BEST, SQ_ALL):
        a, b = whole.strands("A", mode), far.strands("A", mode)
        assert (a.rows, a.nlines, a.nmatchlines, a.per_strand) == (b.rows, b.nlines, b.nmatchlines, b.per_strand) and min(b.per_strand) > 10
    for pair, mode, window in INSERT_CASES:
        a, b = whole.rows(pair, mode, window), far.rows(pair, mode, window)
        assert a == b and len(b) > 1000
        assert whole.joined(pair, mode).counts(window) == far.joined(pair, mode).counts(window)
        assert _host_text(text, a, whole.offs) == _host_text(lay.far, b, far.offs)
    assert whole.demux() == far.demux()
    if fastq:
        rows = far.rows("AB")
        assert whole.gate(rows) == far.gate(rows)


def test_a_row_repeated_is_its_period_replicated(oracle, harness):
    K.use_harness(harness)
    for key in (F.FAR_ROWS[1], F.FAR_ROWS[-1]):                  # a FASTA row and the generic path's (FASTA too: headers are not counted)
        row = next(r for r in F.far_rows() if r.key == key)
        fr = F.FarRow(row, oracle, b32=1 << 22)
        text = fr.materialise()
        assert len(text) == fr.nbytes >= (1 << 22) + 2 * fr.P > fr.nbytes - fr.P and 10 <= fr.K < 64
        e = oracle.buffer_scan(row.pattern, row.tau, text, fr.mode | (row.options & 0x0C), fasta=row.fasta)
        assert (e["nlines"], e["nmatchlines"], len(e["records"])) == (fr.nlines(), fr.nmatchlines(), fr.nrecords())
        assert np.array_equal(e["records"], fr.records().astype(np.uint64))
        offs = np.array(W.line_offsets(text, row.fasta), dtype=np.uint64)
        assert np.array_equal(offs[e["records"][:, 0].astype(np.int64)], fr.offsets())
        all_ = oracle.buffer_scan(row.pattern, row.tau, text, SQ_ALL | (row.options & 0x0C), fasta=row.fasta)
        assert len(all_["records"]) == fr.nhits_all()
        # the boundary lies strictly inside a record
        ln, s, en, _ = fr.hit
        line = 1 + fr.copy * fr.nper + ln
        assert int(offs[line]) + s < (1 << 22) < int(offs[line]) + en and [line, s, en] in all_["records"][:, :3].tolist()
        c, r, pl, col = fr.where(1 << 22)
        assert (c, pl) == (fr.copy, ln) and s < col < en


def test_the_far_rows_cover_the_kernel_families(oracle, harness):
    K.use_harness(harness)
    rows = F.far_rows()
    assert len(rows) >= 16 and len({r.key for r in rows}) == len(rows)
    assert F.uncovered(rows) == []
    assert F.uncovered(rows[:3]) != []                              # (the check can fail)
    for r in rows:
        assert K.instance_key(r.plan(), r.options, r.want) == r.key
        fr = F.FarRow(r, oracle)
        assert fr.nbytes >= F.B32 + 2 * fr.P and fr.nlines() < 1 << 31
        if r.want == K.RECORDS:
            assert 0 < fr.nrecords() <= F.MAX_FAR_RECORDS, (r.key, fr.nrecords())
        print(fr.describe())


# ---- phases ----
@pytest.mark.parametrize("view", list(VIEWS))
def test_what_every_boundary_cuts(true_layouts, view):
    lay, ref = true_layouts[view]
    assert lay.bounds == dict(B31=1 << 31, SEAM=0xF0000000, B32=1 << 32) and lay.order == ["B31", "SEAM", "B32"]
    assert len(lay.far) >= F.B32 + F.TAIL_MIN and len(lay.far) < F.B32 + (3 << 19)
    lines = lay.phases(ref)
    assert len(lines) == 3
    for ln in lines:
        print("%s: %s" % (view, ln))
    for pos, pad, n in lay.gaps:                                    # whole units behind one adjusted one: the line classes are undisturbed
        U = len(lay.fill.unit)
        assert lay.far[pos:pos + U + pad] == lay.fill.adjusted(pad) and lay.far[pos + U + pad:pos + 2 * U + pad] == lay.fill.unit
        assert lay.fill.adjusted(pad).count(b"\n") == 4 == lay.fill.unit.count(b"\n")
    # under 1 GiB segments the seams at 2^31 and 2^32 lie inside blocks too
    for B in (F.B31, F.B32):
        assert any(s < B < s + len(lay.block) for s in lay.block_start)


def test_the_filler_holds_no_hit(oracle, true_layouts):
    for view, (lay, _) in true_layouts.items():
        fill = lay.fill
        text = b"".join(fill.adjusted(pad) for pad in (0, 1, len(fill.unit) // 2, len(fill.unit) - 1)) + fill.unit * 3
        seq = W.fastq_seq(text)[0] if lay.fastq else text
        assert F.no_hit(oracle, seq) and len(seq) > 800
        assert len(text.split(b"\n")) - 1 == 28


# ---- liveness ----
def _low32(off):
    return off & 0xFFFFFFFF


def _int32(off):
    off &= 0xFFFFFFFF
    return off - (1 << 32) if off >= 1 << 31 else off


class _Offs:
    """the line offsets of a reference, each read wrongly"""

    def __init__(self, offs, wrong):
        self.offs, self.wrong = offs, wrong

    def __getitem__(self, line):
        return self.wrong(self.offs[line])


def _answers(ref, offs, fastq, chain):
    """what the families compare, from the reference's rows and the line offsets `offs`"""
    rows = ref.rows("AB")
    hits = ref.hit_rows("B")
    spans = [ref.window[offs[r[0]] + r[1]:offs[r[0]] + r[2]] for r in rows]
    lib = PyLibrary(chain.guides)
    out = dict(offsets=[offs[r[0]] for r in hits], text=_host_text(ref.window, rows, offs), tally=collections.Counter(spans),
               library=lib.tally(spans, 1)[0],
               cuts=[py_anchor_all(ref.window, [r[:4] for r in hits], [max(0, offs[r[0]]) for r in hits], anchor=a, skip=0, length=n, reach=1024)[:2]
                     for a, n in ((AFTER, 0), (LINE, 16))])
    if fastq:
        from test_qgate_host import py_gate
        out["gate"] = [py_gate(ref.window, max(0, offs[r[0]]), r[1], r[2])[0] for r in rows]
    return out


@pytest.mark.parametrize("view", list(VIEWS))
def test_a_reference_with_narrow_offsets_answers_otherwise(true_layouts, view):
    lay, ref = true_layouts[view]
    true = _answers(ref, ref.offs, lay.fastq, lay.chain)
    for name, wrong in (("32 bits", _low32), ("int32", _int32)):
        other = _answers(ref, _Offs(ref.offs, wrong), lay.fastq, lay.chain)
        assert set(other) == set(true)
        for what in true:
            assert other[what] != true[what], "%s: line offsets kept in %s give the same %s" % (view, name, what)
    # segment-relative positions of block 2 (default segments: it lies in segment 0, above 2^31) read as signed
    first = lay.shift[1] + lay.nblock + 1
    assert lay.order[1] == "SEAM" and F.B31 < lay.block_start[1] < lay.bounds["SEAM"]

    def signed(off):
        k = off // lay.bounds["SEAM"]
        return k * lay.bounds["SEAM"] + _int32(off - k * lay.bounds["SEAM"])
    other = _answers(ref, _Offs(ref.offs, signed), lay.fastq, lay.chain)
    rows2 = [i for i, r in enumerate(ref.hit_rows("B")) if first <= r[0] < first + lay.nblock]
    assert len(rows2) > 1000 and all(other["offsets"][i] != true["offsets"][i] for i in rows2 if true["offsets"][i] < lay.bounds["SEAM"])
    for what in true:
        assert other[what] != true[what], "%s: segment-relative positions read as signed give the same %s" % (view, what)


# ---- FarBytes ----
def _materialise(lay, lo, hi):
    """[lo, hi) of the layout's text, put together piece by piece without FarBytes' arithmetic: every piece that touches the range is
    written out whole (a run of units: the repeats that touch it)"""
    U = len(lay.fill.unit)
    out = bytearray(hi - lo)
    pos = 0
    pieces = []
    for (gpos, pad, n), start in zip(lay.gaps, lay.block_start):
        assert gpos == pos
        pieces += [(pos, lay.fill.adjusted(pad), 1), (pos + U + pad, lay.fill.unit, n), (start, lay.block, 1)]
        assert pos + U + pad + n * U == start
        pos = start + len(lay.block)
    pieces.append((pos, lay.fill.unit, (len(lay.far) - pos) // U))
    for start, data, n in pieces:
        for c in range(max(0, (lo - start) // len(data)), min(n, (hi - start) // len(data) + 1)):
            a = start + c * len(data)
            s, e = max(a, lo), min(a + len(data), hi)
            if s < e:
                out[s - lo:e - lo] = data[s - a:e - a]
    return bytes(out)


@pytest.mark.parametrize("view", list(VIEWS))
def test_far_bytes_across_every_edge(true_layouts, view):
    lay, _ = true_layouts[view]
    far = lay.far
    rng = random.Random(11)
    edges = far.starts[1:] + [len(far)]
    assert len(edges) == 10
    for e in edges + [lay.bounds[r] for r in F.ROLES]:
        lo, hi = max(0, e - (1 << 20)), min(len(far), e + (1 << 20))
        near = _materialise(lay, lo, hi)
        assert far[lo:hi] == near and len(near) == hi - lo
        for _ in range(200):
            a = rng.randrange(max(lo, e - 700), min(hi, e + 1))
            b = min(hi, a + rng.choice((0, 1, 2, 16, 17, 300, 1500)))
            assert far[a:b] == near[a - lo:b - lo]
            assert far[a] == near[a - lo] if a < len(far) else True
            assert far.find(b"\n", a, b) == (near.find(b"\n", a - lo, b - lo) + lo if near.find(b"\n", a - lo, b - lo) >= 0 else -1)
    assert far[len(far) - 5:len(far) + 100] == far[len(far) - 5:] and len(far[len(far) - 5:]) == 5 and far[-3:2] == far[0:2]
    with pytest.raises(IndexError):
        far[len(far)]
