"""GPU (-m gpu): cuts at fixed offsets from a hit or the line's start (seeqdevScanAnchor; seeq_anchor.h: kinds, totals, the rewritten spans
and their ordered compaction, all on the device) against the rule restated in Python (test_anchor_host.py::py_anchor) over records the
code under test did not place.  The texts are test_anchor_host.py's -- plain lines with ONE flank whose position the test knows -- and every
case first asserts that the scan found exactly the planted hits: a vacuous case fails.  Every comparison is of integers and bytes."""
import ctypes as C
import errno
import os
import random
import re

import numpy as np
import pytest

import late_text as L
from conftest import ROOT
from oracle.pyoracle import SQ_ALL, SQ_BEST
from test_anchor_host import (AFTER, BEFORE, FAR, FLANK, KEPT, LINE, PARAMS, REACH_MAX, SHORT, TAILS, Lines, _kw, edge_text, py_anchor_all, random_lines,
                              window_case)
from test_gpu_strands import _step
from test_gpu_tally import RIGHT
from test_gpu_tally import _same as _same_tally
from test_gpu_tally_grouped import _held_of
from test_gpu_tally_grouped import _same as _same_grouped
from test_tally_append_host import py_append

pytestmark = pytest.mark.gpu
T = int(re.search(r"#define\s+SEEQ_ANCHOR_TILE\s+(\d+)", open(os.path.join(ROOT, "seeq_amd", "csrc", "seeq_anchor.h")).read()).group(1))
COUNTS = ("nspans", "nkept", "nshort", "nfar", "span_bytes")
RC_FLANK = FLANK[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))

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
def pats(gpu):
    from seeq_amd import device as dev
    ps = dict(F=dev.Pattern(FLANK.decode(), 0), R=dev.Pattern(RIGHT, 0), N=dev.Pattern("N", 0))
    yield ps
    for p in ps.values():
        p.close()


def _cuda(buf):
    import torch
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


def _hits(s, pats, t, rows, options=SQ_BEST, what=""):
    """A fetched scan of the flank over t, its records held against the planted rows -> the source's records [n, 4] u32 and offsets."""
    from seeq_amd import device as dev
    got = s.scan_tensor(pats["F"], t, options, dev.WANT_RECORDS)
    assert got["nrecords"] == len(rows), (what, got)
    rec, off = s.records(len(rows)), s.record_offsets(len(rows))
    assert [tuple(r) for r in rec[:, :3].tolist()] == [(r[0], r[2], r[3]) for r in rows] and off.tolist() == [r[1] for r in rows], what
    return rec, off


def _same(res, text, rec, off, param):
    """An anchor() result (copy=True) against the rule over the SOURCE's records [n, 4] u32 and offsets."""
    kinds, rows, offs, cnt = py_anchor_all(text, rec.tolist(), off.tolist(), **_kw(param))
    assert {k: res[k] for k in COUNTS} == cnt, (param, {k: res[k] for k in COUNTS}, cnt)
    assert res["nspans"] == res["nkept"] + res["nshort"] + res["nfar"]
    assert res["kinds"].dtype == np.uint8 and res["kinds"].tolist() == kinds, param
    assert res["records"].dtype == np.uint32 and res["records"].shape == (cnt["nkept"], 4)
    assert res["records"].tobytes() == np.array(rows, dtype=np.uint32).reshape(-1, 4).tobytes(), param      # in order, words 0 and 3 untouched
    assert res["offsets"].tobytes() == np.array(offs, dtype=np.uint64).tobytes(), param
    return kinds, rows, offs, cnt


def _cut(s, t, param, copy=True):
    return s.anchor(t, source="hits", anchor=param[0], skip=param[1], length=param[2], reach=param[3], copy=copy)


def _spans(text, rows, offs):
    return [text[o + r[1]:o + r[2]] for r, o in zip(rows, offs)]


# ---- tile shapes ----
@pytest.mark.parametrize("n", [0, 1, 255, T - 1, T, T + 1, 2 * T + 1 + 7])
def test_record_counts(gpu, capi, pats, n):
    """No record, one, a tile and its edges, a partial last tile and a top over more than one tile: the counts, the kind of every source
    record, the anchored records and offsets -- KEPT, SHORT and FAR all inside one tile."""
    from seeq_amd import device as dev
    lines = random_lines(n, 100 + n)
    if n == 0:
        lines.add(12, 20, flank=None)
    text = lines.text()
    t = _cuda(text)
    sc = dev.Scanner()
    mix = (AFTER, 2, 0, 64)

    def call(s):
        rec, off = _hits(s, pats, t, lines.rows, what="%d records" % n)
        return rec, off, [(p, _cut(s, t, p)) for p in (mix, (AFTER, 0, 12, 1024), (LINE, 3, 16, 64), (BEFORE, 1, 9, 1), (LINE, 0, 0, 1024))]

    def check(s, out):
        rec, off, results = out
        for p, res in results:
            _same(res, text, rec, off, p)
        res = results[0][1]
        assert res["nspans"] == n
        if n >= 255:
            first_tile = res["kinds"][:T].tolist()
            assert first_tile.count(KEPT) > 20 and first_tile.count(SHORT) > 20 and first_tile.count(FAR) > 20
        assert bool(s.anchored_device_ptr()) == bool(results[-1][1]["nkept"])
    _go(sc, "%d records" % n, call, check)
    if n == 0:
        assert sc.last_anchor_ms() == 0                     # no records: nothing is launched
    sc.close()


def test_nothing_kept_is_a_result(gpu, capi, pats):
    from seeq_amd import device as dev
    lines = edge_text(TAILS[2])
    text = lines.text()
    t = _cuda(text)
    sc = dev.Scanner()
    rec, off = _hits(sc, pats, t, lines.rows)
    res = _cut(sc, t, (BEFORE, 41, 0, 1024))                # no hit starts behind column 40
    _same(res, text, rec, off, (BEFORE, 41, 0, 1024))
    assert res["nkept"] == 0 and res["nshort"] == len(lines.rows) and res["span_bytes"] == 0 and len(res["records"]) == 0 and len(res["kinds"]) == len(lines.rows)
    assert sc.anchored_device_ptr() is None
    tl = sc.tally(t, source="anchored")
    assert tl["nspans"] == 0 and tl["ndistinct"] == 0 and len(tl["keys"]) == 0
    with pytest.raises(dev.SeeqDeviceError):
        sc.anchored_records(1)
    sc.close()


# ---- the rule's edges ----
@pytest.mark.parametrize("tail", TAILS, ids=lambda tail: "%d%s" % (tail[0], "nl" if tail[1] else ""))
def test_rule_edges(gpu, capi, pats, tail):
    """test_anchor_host.py's text -- a newline at every offset 0 .. 64 behind a hit and around 128 and 256, empty lines, '\\r\\n' lines, the
    last record 0, 1, 15, 16, 63, 64 bytes before the text's end -- under every parameter set: every anchor with length == 0 and > 0,
    e - end on both sides of 16, 64 and 128, reach 1, 63, 64, 65, skip > start, length > start - skip, s == L."""
    from seeq_amd import device as dev
    lines = edge_text(tail)
    text = lines.text()
    t = _cuda(text)
    sc = dev.Scanner()

    def call(s):
        rec, off = _hits(s, pats, t, lines.rows)
        return rec, off, [_cut(s, t, p) for p in PARAMS]
    seen = set()

    def check(s, out):
        rec, off, results = out
        for p, res in zip(PARAMS, results):
            kinds, _, _, _ = _same(res, text, rec, off, p)
            seen.update((p[0], p[2] > 0, k) for k in kinds)
    _go(sc, "edges, tail %s" % (tail,), call, check)
    assert seen == ({(a, pos, k) for a in (AFTER, BEFORE, LINE) for pos in (False, True) for k in (KEPT, SHORT)} | {(AFTER, False, FAR), (LINE, False, FAR)})
    sc.close()


# ---- sources ----
def test_hits_of_a_both_strands_call(gpu, capi, pats):
    """Every other line carries the flank's reverse complement: bit 31 of `dist` arrives untouched, the positions are the text's."""
    from seeq_amd import device as dev
    lines = Lines(5)
    for i in range(T + 30):
        lines.add(lines.rng.randrange(20), lines.rng.choice((0, 3, 12, 13, 30, 70)), flank=RC_FLANK if i % 2 else FLANK)
    text = lines.text()
    t = _cuda(text)
    sc = dev.Scanner()
    param = (AFTER, 1, 12, 64)

    def call(s):
        got = s.strands_tensor(pats["F"], t, SQ_ALL, dev.WANT_RECORDS, copy=False)
        assert got["nrecords"] == len(lines.rows), got
        rec, off = s.records(len(lines.rows)), s.record_offsets(len(lines.rows))
        assert [tuple(r) for r in rec[:, :3].tolist()] == [(r[0], r[2], r[3]) for r in lines.rows] and off.tolist() == [r[1] for r in lines.rows]
        assert ((rec[:, 3] >> 31) == np.arange(len(lines.rows)) % 2).all()
        return rec, off, _cut(s, t, param), _cut(s, t, (BEFORE, 0, 0, 1))
    got = {}

    def check(s, out):
        rec, off, res, before = out
        _same(res, text, rec, off, param)
        _same(before, text, rec, off, (BEFORE, 0, 0, 1))
        got["res"] = res
    _go(sc, "hits of a both-strands call", call, check)
    minus = got["res"]["records"][:, 3] >> 31
    assert 0 < int(minus.sum()) < len(minus) and (minus == (got["res"]["records"][:, 0] - 1) % 2).all()
    sc.close()


def _insert_lines(n, seed):
    """Lines of prefix + FLANK + insert + RIGHT + suffix -> (text, rows of (line, off, start, end) of the insert)."""
    rng = random.Random(seed)
    bases = lambda m: bytes(rng.choices(b"ACGT", k=m))      # noqa: E731
    buf, rows = bytearray(), []
    for i in range(n):
        pre, ins, suf = rng.randrange(8), rng.randrange(4, 15), rng.choice((0, 1, 8, 11, 12, 13, 40, 64, 90))
        rows.append((i + 1, len(buf), pre + len(FLANK), pre + len(FLANK) + ins))
        buf += bases(pre) + FLANK + bases(ins) + RIGHT.encode() + bases(suf) + b"\n"
    return bytes(buf), rows


def test_inserts_as_the_source(gpu, capi, pats):
    """The inserts of a flank pair, cut behind (12 bases behind the right flank: skip 20), in front (what lies before the left flank) and
    from the line's start; both distances of the insert record arrive untouched.  Then with NULL text after inserts_host: the staged one."""
    from seeq_amd import device as dev
    text, rows = _insert_lines(T + 40, 8)
    t = _cuda(text)
    sc = dev.Scanner()
    params = [(AFTER, 20, 12, 64), (BEFORE, 20, 4, 1), (LINE, 0, 0, 64), (AFTER, 20, 0, 32)]

    def source(s):
        res = s.inserts_tensor(pats["F"], pats["R"], t, SQ_BEST, copy=False)
        assert res["ninserts"] == len(rows), res
        rec, off = s.insert_records(len(rows)).view(np.uint32).reshape(-1, 4), s.insert_offsets(len(rows))
        assert [tuple(r) for r in rec[:, :3].tolist()] == [(r[0], r[2], r[3]) for r in rows] and off.tolist() == [r[1] for r in rows]
        return rec, off

    def call(s):
        rec, off = source(s)
        return rec, off, [s.anchor(t, source="inserts", anchor=p[0], skip=p[1], length=p[2], reach=p[3]) for p in params]

    def check(s, out):
        rec, off, results = out
        for p, res in zip(params, results):
            kinds, _, _, _ = _same(res, text, rec, off, p)
            assert len(set(kinds)) >= 2, p
    _go(sc, "inserts, the text passed", call, check)
    # the tally over the anchored inserts: the 12 bases behind the right flank
    rec, off = source(sc)
    res = sc.anchor(t, source="inserts", skip=20, length=12, reach=64)
    _, krows, koffs, _ = _same(res, text, rec, off, params[0])
    _same_tally(sc.tally(t, source="anchored"), _spans(text, krows, koffs))
    sc.close()
    # NULL text: the text inserts_host staged
    sc = dev.Scanner()
    got = sc.inserts_host(pats["F"], pats["R"], text, SQ_BEST)
    assert got["ninserts"] == len(rows)
    rec, off = sc.insert_records(len(rows)).view(np.uint32).reshape(-1, 4), sc.insert_offsets(len(rows))
    res = sc.anchor(source="inserts", skip=20, length=12, reach=64)
    _same(res, text, rec, off, params[0])
    _same_tally(sc.tally(source="anchored"), _spans(text, krows, koffs))
    whole = sc.anchor(source="inserts", anchor=LINE, skip=0, length=0, reach=64)
    _same(whole, text, rec, off, params[2])
    with pytest.raises(dev.SeeqDeviceError):
        sc.anchor(source="hits", skip=0, length=4)          # hits need the text they were found in, and there are none
    sc.close()


# ---- FASTQ records: the scan under SEEQDEV_FASTQ, the gate behind the anchor ----
def py_quality(text, off, start, end, min_qual=20, base=33, max_low=0, reach=1024):
    """The base-quality rule of include/seeq_amd.h, restated here: -> "pass", "low", "long", "far" or "misfit" for the span [start, end) of
    the line at off.  The quality line is the second line below the span's; it must end where a line of the sequence line's length ends."""
    n = len(text)
    assert start <= end and off <= n and end <= n - off
    if end - start > 31:
        return "long"
    p = off + end
    stop = min(n, p + reach)
    e1 = text.find(b"\n", p, stop)
    e2 = text.find(b"\n", e1 + 1, stop) if e1 >= 0 else -1
    if e2 < 0:
        return "far" if p + reach < n else "misfit"
    q0, seqlen = e2 + 1, e1 - off
    if q0 + seqlen > n or (q0 + seqlen < n and text[q0 + seqlen] != 10):
        return "misfit"
    return "low" if sum(1 for b in text[q0 + start:q0 + end] if b < base + min_qual) > max_low else "pass"


GATE_NAMES = ("pass", "low", "long", "far", "misfit")


def _fastq(n, seed, p_low=0.03):
    """n four-line records whose sequence line is a 16-base cell barcode (one of 9), a 12-base UMI (one of 40) and 0 .. 60 more bases; now
    and then a read too short for the UMI or for the barcode.  -> (text, rows of (record, offset of the sequence line, its length))."""
    rng = random.Random(seed)
    bases = lambda m: bytes(rng.choices(b"ACGT", k=m))      # noqa: E731
    cells, umis = [bases(16) for _ in range(9)], [bases(12) for _ in range(40)]
    buf, rows = bytearray(), []
    for i in range(n):
        seq = rng.choice(cells) + rng.choice(umis) + bases(rng.randrange(61))
        if i % 23 == 5:
            seq = seq[:rng.choice((1, 15, 16, 20, 27))]
        qual = bytes(rng.randrange(35, 53) if rng.random() < p_low else 73 for _ in range(len(seq)))
        buf += b"@r%d\n" % (i + 1)
        rows.append((i + 1, len(buf), len(seq)))
        buf += seq + b"\n+\n" + qual + b"\n"
    return bytes(buf), rows


def test_fastq_records_and_the_gate_behind_the_anchor(gpu, capi, pats):
    """SEEQDEV_FASTQ in the scan of `N`: one record (record number, 0, 1, 0) per read, the offsets those of the sequence lines, the line's
    end the sequence line's.  The barcode and the UMI cut by position are gated (quality_gate(source="anchored")) and tallied."""
    from seeq_amd import device as dev
    text, rows = _fastq(T + 77, 3)
    t = _cuda(text)
    sc = dev.Scanner()
    opt = SQ_BEST | dev.SEEQDEV_FASTQ

    def source(s):
        got = s.scan_tensor(pats["N"], t, opt, dev.WANT_RECORDS)
        assert got["nrecords"] == len(rows), got
        rec, off = s.records(len(rows)), s.record_offsets(len(rows))
        assert rec.tolist() == [[r[0], 0, 1, 0] for r in rows] and off.tolist() == [r[1] for r in rows]
        return rec, off

    def call(s):
        rec, off = source(s)
        whole = _cut(s, t, (LINE, 0, 0, 1024))
        umi = _cut(s, t, (LINE, 16, 12, 64))
        gate = s.quality_gate(t, source="anchored")
        return rec, off, whole, umi, gate, s.tally(t, source="gated")

    def check(s, out):
        rec, off, whole, umi, gate, tl = out
        _, wrows, _, _ = _same(whole, text, rec, off, (LINE, 0, 0, 1024))
        assert [r[2] for r in wrows] == [r[2] for r in rows]                 # the line's end is the sequence line's
        _, urows, uoffs, ucnt = _same(umi, text, rec, off, (LINE, 16, 12, 64))
        assert 0 < ucnt["nshort"] < 80 and ucnt["nfar"] == 0
        kinds = [py_quality(text, o, r[1], r[2]) for r, o in zip(urows, uoffs)]
        assert gate["kinds"].tolist() == [GATE_NAMES.index(k) for k in kinds] and gate["nspans"] == len(urows)
        assert gate["npassed"] == kinds.count("pass") and gate["nlow"] == kinds.count("low") > 20 and gate["nmisfit"] == gate["nfar"] == gate["nlong"] == 0
        keep = [k == "pass" for k in kinds]
        assert gate["records"].tobytes() == np.array([r for r, k in zip(urows, keep) if k], dtype=np.uint32).reshape(-1, 4).tobytes()
        _same_tally(tl, [text[o + r[1]:o + r[2]] for r, o, k in zip(urows, uoffs, keep) if k])
    _go(sc, "FASTQ records", call, check)
    sc.close()


# ---- downstream: the barcode / UMI chain over one fetched scan of N ----
def _reads_without_a_flank(n, seed):
    """Plain lines: a 16-base cell barcode (one of 7), a 12-base UMI (one of 30) and the rest; short reads, empty lines and lines that start
    with another byte than a base now and then.  -> (text, rows of (line, off) of the lines whose first byte is a base)."""
    rng = random.Random(seed)
    bases = lambda m: bytes(rng.choices(b"ACGT", k=m))      # noqa: E731
    cells, umis = [bases(16) for _ in range(7)], [bases(12) for _ in range(30)]
    buf, rows = bytearray(), []
    for i in range(n):
        seq = rng.choice(cells) + rng.choice(umis) + bases(rng.randrange(40))
        if i % 17 == 3:
            seq = seq[:rng.choice((0, 3, 15, 16, 17, 27))]
        elif i % 29 == 7:
            seq = b"-" * len(seq)                           # no base at all: no record
        elif i % 31 == 11:
            seq = seq[:20] + b"N" + seq[21:]                # a foreign byte in the UMI
        if seq[:1] and seq[:1] in b"ACGTN":
            rows.append((i + 1, len(buf)))
        buf += seq + b"\n"
    return bytes(buf), rows


def test_lines_without_a_flank_the_barcode_umi_chain(gpu, capi, pats):
    """The pattern N at distance 0, fetched with records, gives (line, 0, 1, 0) for every line whose first byte is a base; anchor(line, 0,
    16) + tally_hold, anchor(line, 16, 12) + tally_grouped over that ONE scan is the join of the columns cut on the host; the same with
    the UMI appended as a second key column."""
    from seeq_amd import device as dev
    # the documented composition on the oracle's own example
    small = b"ACGT\n\nNNAC\nacgt\nXYZ\nGATTACA"
    sc = dev.Scanner()
    st = _cuda(small)
    got = sc.scan_tensor(pats["N"], st, SQ_BEST, dev.WANT_RECORDS)
    assert got["nrecords"] == 4 and sc.records(4).tolist() == [[1, 0, 1, 0], [3, 0, 1, 0], [4, 0, 1, 0], [6, 0, 1, 0]]
    cut = sc.anchor(st, anchor=LINE, skip=1, length=3)
    assert cut["records"].tolist() == [[1, 1, 4, 0], [3, 1, 4, 0], [4, 1, 4, 0], [6, 1, 4, 0]] and cut["nkept"] == 4
    text, rows = _reads_without_a_flank(T + 90, 6)
    t = _cuda(text)

    def source(s):
        got = s.scan_tensor(pats["N"], t, SQ_BEST, dev.WANT_RECORDS)
        assert got["nrecords"] == len(rows), got
        rec, off = s.records(len(rows)), s.record_offsets(len(rows))
        assert rec.tolist() == [[r[0], 0, 1, 0] for r in rows] and off.tolist() == [r[1] for r in rows]
        return rec, off
    cell_p, umi_p = (LINE, 0, 16, 64), (LINE, 16, 12, 64)

    def call(s):
        rec, off = source(s)
        cells = _cut(s, t, cell_p)
        hold = s.tally_hold(t, source="anchored")
        umis = _cut(s, t, umi_p)                            # the source is untouched: the second anchor sees it as the first did
        grouped = s.tally_grouped(t, source="anchored")
        # the same chain with the UMI as a second key column of the held key
        _cut(s, t, cell_p, copy=False)
        s.tally_hold(t, source="anchored")
        _cut(s, t, umi_p, copy=False)
        app = s.tally_hold_append(t, source="anchored")
        held = s.held()
        return rec, off, cells, hold, umis, grouped, app, list(zip(held["lines"].tolist(), held["keys"].tolist()))

    def check(s, out):
        rec, off, cells, hold, umis, grouped, app, held = out
        _, crows, coffs, ccnt = _same(cells, text, rec, off, cell_p)
        _, urows, uoffs, ucnt = _same(umis, text, rec, off, umi_p)
        assert 0 < ucnt["nshort"] and ucnt["nkept"] < ccnt["nkept"] < len(rows)
        ccol = [(r[0], b) for r, b in zip(crows, _spans(text, crows, coffs))]
        ucol = [(r[0], b) for r, b in zip(urows, _spans(text, urows, uoffs))]
        held0, hcnt = _held_of(ccol)
        assert hold == hcnt
        _same_grouped(grouped, held0, ucol)
        assert grouped["nforeign"] > 0 and grouped["nungrouped"] == 0 and grouped["ngroups"] == 7
        ucolumn, acol = _held_of(ucol)
        exp_held, acnt = py_append(held0, ucolumn)
        assert app["column"] == acol and held == exp_held and app["nheld"] == acnt["nheld"] and app["ndropped"] == acnt["ndropped"] > 0
    _go(sc, "barcode / UMI chain", call, check)
    sc.close()


# ---- state ----
def test_state_around_an_anchor(gpu, capi, pats):
    """An anchor leaves the record arrays, the inserts result, a held column and the last tally table as they were; its own arrays answer
    the same after a further scan and a further inserts call; a second anchor replaces them."""
    from seeq_amd import device as dev
    text, rows = _insert_lines(T + 50, 12)
    t = _cuda(text)
    sc = dev.Scanner()
    sc.set_profiling(True)
    res = sc.inserts_tensor(pats["F"], pats["R"], t, SQ_BEST, copy=False)
    assert res["ninserts"] == len(rows)
    n = len(rows)
    hold = sc.tally_hold(t)
    table = sc.tally(t)
    src = (sc.insert_records(n).view(np.uint32).reshape(-1, 4), sc.insert_offsets(n))
    before = (src[0].tobytes(), src[1].tobytes(), sc.insert_text(t).cpu().numpy().tobytes(), sc.tally_table(table["ndistinct"]).tobytes(), sc.held()["keys"].tobytes())
    p1 = (AFTER, 20, 12, 64)
    first = sc.anchor(t, source="inserts", skip=20, length=12, reach=64)
    _, krows, koffs, cnt = _same(first, text, src[0], src[1], p1)
    assert sc.last_anchor_ms() > 0 and 0 < cnt["nkept"] < n
    after = (sc.insert_records(n).tobytes(), sc.insert_offsets(n).tobytes(), sc.insert_text(t).cpu().numpy().tobytes(), sc.tally_table(table["ndistinct"]).tobytes(),
             sc.held()["keys"].tobytes())
    assert after == before and sc.held()["nrecords"] == hold["nspans"]
    # the hits of a fetched scan: byte-identical around an anchor over them
    lines = edge_text(TAILS[3])
    ht = _cuda(lines.text())
    rec, off = _hits(sc, pats, ht, lines.rows)
    # ... and the anchored arrays of the inserts survived that scan
    kept = (first["records"].tobytes(), first["offsets"].tobytes(), first["kinds"].tobytes())
    assert (sc.anchored_records(cnt["nkept"]).tobytes(), sc.anchored_offsets(cnt["nkept"]).tobytes(), sc.anchor_kinds(n).tobytes()) == kept
    assert sc.anchored_records(3, first=2).tobytes() == first["records"][2:5].tobytes()
    assert sc.inserts_tensor(pats["R"], pats["F"], ht, SQ_BEST, copy=False)["ninserts"] == 0      # a further inserts call (nothing found)
    assert (sc.anchored_records(cnt["nkept"]).tobytes(), sc.anchored_offsets(cnt["nkept"]).tobytes(), sc.anchor_kinds(n).tobytes()) == kept
    _same_tally(sc.tally(t, source="anchored"), _spans(text, krows, koffs))      # ... with the text the anchored records were found in
    # a second anchor (over the hits) replaces the first
    rec, off = _hits(sc, pats, ht, lines.rows)
    p2 = (AFTER, 0, 0, 64)
    second = _cut(sc, ht, p2)
    _, _, _, cnt2 = _same(second, lines.text(), rec, off, p2)
    assert sc.records(len(lines.rows)).tobytes() == rec.tobytes() and sc.record_offsets(len(lines.rows)).tobytes() == off.tobytes()
    with pytest.raises(dev.SeeqDeviceError):
        sc.anchored_records(1, first=cnt2["nkept"])         # beyond the new result
    assert len(sc.anchor_kinds(len(lines.rows))) == len(lines.rows)
    with pytest.raises(dev.SeeqDeviceError):
        sc.anchor_kinds(1, first=len(lines.rows))
    sc.close()


# ---- placement ----
@pytest.mark.parametrize("i", [0, 1], ids=["odd", "aligned"])
def test_a_window_of_a_larger_buffer(gpu, capi, pats, i):
    """The entry on a window of a larger tensor whose guards are BASES (test_anchor_host.py shows them live): the window's last line has no
    newline, so a cut that reads past nbytes returns a longer span -- a wrong answer, not a fault."""
    from seeq_amd import device as dev
    lines, big, lo, hi = window_case(i)
    text = lines.text()
    view = _cuda(big)[lo:hi]
    assert view.is_contiguous() and view.data_ptr() % 16 == lo % 16 and ((lo % 2 == 1) if i == 0 else (lo % 16 == 0))
    sc = dev.Scanner()

    def call(s):
        rec, off = _hits(s, pats, view, lines.rows)
        return rec, off, [_cut(s, view, p) for p in PARAMS]

    def check(s, out):
        rec, off, results = out
        for p, res in zip(PARAMS, results):
            _same(res, text, rec, off, p)
    _go(sc, "window at lead %d" % lo, call, check)
    sc.close()


# ---- a caller's non-blocking stream ----
class _LateAnchor(L.LateScanner):
    """LateScanner with the new entry armed as its siblings are: the text is late on the side stream when the anchor gets control."""

    def anchor(self, text=None, source="hits", anchor="after", skip=0, length=0, reach=1024, copy=True):
        from seeq_amd import device as dev
        return self._late(lambda: self.arm(text), lambda: dev.Scanner.anchor(self, text, source, anchor, skip, length, reach, copy))


def test_the_anchor_reads_its_text_in_stream_order(gpu, capi, pats):
    """On a caller's non-blocking stream the text arrives late before every entry (late_text.py: decoy bytes, a device-side delay, the true
    bytes).  late_text's decoy keeps every newline, which is all the anchor reads: here the decoy is the text with its newlines turned
    into bases, under which every line goes on to the reach."""
    import torch
    lines = edge_text(TAILS[2], seed=31)
    text = lines.text()
    t = _cuda(text)
    side = torch.cuda.Stream()
    flags = L.stream_flags(side)
    assert side.cuda_stream != 0 and (flags is None or flags & L.HIP_STREAM_NON_BLOCKING)
    params = [(AFTER, 0, 0, 64), (AFTER, 0, 12, 1024), (LINE, 0, 0, 1024)]
    no_newlines = text.replace(b"\n", b"A")

    def run(s):
        rec, off = _hits(s, pats, t, lines.rows)
        return rec, off, [_cut(s, t, p) for p in params], s.tally(t, source="anchored")

    def make(cycles, armed):
        s = _LateAnchor(side, cycles, armed)
        late = s.give(t, text)
        late.decoy = _cuda(no_newlines)
        torch.cuda.synchronize()
        return s
    delay = L.Delay()
    probe = make(0, False)
    for _ in ("cold", "warm"):
        probe.slowest_ms = 0.0
        run(probe)
    torch.cuda.synchronize()
    probe.close()
    sc = make(delay.cycles(max(L.MIN_DELAY_MS, 2.0 * probe.slowest_ms)), True)
    try:
        rec, off, results, tl = run(sc)
        assert sc.arms >= 5
        for p, res in zip(params, results):
            kinds, _, _, _ = _same(res, text, rec, off, p)
            assert py_anchor_all(no_newlines, rec.tolist(), off.tolist(), **_kw(p))[0] != kinds      # an entry that read early answers otherwise
        _, krows, koffs, _ = py_anchor_all(text, rec.tolist(), off.tolist(), **_kw(params[-1]))
        assert tl["nspans"] == len(krows) and tl["nlong"] == sum(1 for r in krows if r[2] - r[1] > 31)
    finally:
        torch.cuda.synchronize()
        sc.close()


# ---- errors ----
def _raw_anchor(sc, capi, source, t, nbytes, anchor=0, skip=0, length=0, reach=64):
    cnt = capi.seeqdev_anchor_counts_t()
    C.set_errno(0)
    rc = sc._lib.seeqdevScanAnchor(sc._h, source, C.c_void_p(t.data_ptr()), nbytes, anchor, skip, length, reach, C.byref(cnt))
    return rc, C.get_errno()


def test_a_record_beyond_the_text_is_an_argument_error(gpu, capi, pats):
    """nbytes cut short of the last hit: a record reaches past it, EIO.  An argument check -- the kernel compares before it loads, and no
    walk leaves the nbytes it was given -- so nothing faults and the context goes on: no anchor is completed, the same call with the right
    size gives the result."""
    from seeq_amd import device as dev
    lines = random_lines(T + 9, 41)
    text = lines.text()
    t = _cuda(text)
    sc = dev.Scanner()
    rec, off = _hits(sc, pats, t, lines.rows)
    end_of_last = lines.rows[-1][1] + lines.rows[-1][3]
    for anchor in (0, 1, 2):
        assert _raw_anchor(sc, capi, capi.SEEQDEV_TALLY_HITS, t, end_of_last - 1, anchor) == (-1, errno.EIO)
        assert "outside" in capi.error_text()
    with pytest.raises(dev.SeeqDeviceError):
        sc.tally(t, source="anchored")                      # a failed anchor is no completed anchor
    with pytest.raises(dev.SeeqDeviceError):
        sc.anchor_kinds(1)
    assert _raw_anchor(sc, capi, capi.SEEQDEV_TALLY_ANCHORED, t, len(text)) == (-1, errno.EINVAL)
    assert _raw_anchor(sc, capi, capi.SEEQDEV_TALLY_HITS, t, len(text), 0, 60, 5, 64) == (-1, errno.EINVAL)      # skip + len > reach
    assert _raw_anchor(sc, capi, capi.SEEQDEV_TALLY_HITS, t, len(text), 0, 0, 0, REACH_MAX + 1) == (-1, errno.EINVAL)
    p = (AFTER, 0, 0, 64)
    _same(_cut(sc, t, p), text, rec, off, p)
    assert sc.records(len(lines.rows)).tobytes() == rec.tobytes()
    sc.close()
