"""GPU (-m gpu): SEEQDEV_FASTQ -- a buffer of four-line FASTQ records scanned so that only the SEQUENCE lines count and hits are
numbered by record (include/seeq_amd.h; the ordered device-side filter of seeq_amd/csrc/seeq_fastq.h behind the unchanged scan).

Every expectation is the oracle's answer over the buffer that holds the sequence lines alone, "\\n".join(lines[1::4]), built with
the same trailing-newline choice as the FASTQ buffer.

The text is that of tests/test_gpu_demux.py (_mixed_lines: reads of 40 / 75 / 150 / 151 bases with planted, mutated pattern copies,
here with a foreign byte in a few of them) as the sequence lines; the other three lines of every record are made to hit:
the header is '@' + planted copies, the third line '+' + planted copies, the quality line a copy of the sequence line.  Where the
non-DNA mode lets a line that starts with '@' or '+' match at all (SQ_CONVERT, SQ_IGNORE) the unflagged scan of this text yields
at least three false records per true one; under SQ_FAIL such a line ends at its first byte, and the false records are those of
the quality lines: one per true one.  Both are asserted, so the filter is shown to be doing work."""
import ctypes as C
import errno
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle.pyoracle import SQ_ALL, SQ_BEST, SQ_CONVERT, SQ_FAIL, SQ_FIRST, SQ_IGNORE, SQ_STREAM
from test_gpu_demux import BARCODES, PAT20, TAUS, _check, _expected, _mixed_lines, _mutate

pytestmark = pytest.mark.gpu
MER8 = "ACGTTGCA"
PATTERNS = [(PAT20, 3), (MER8, 1)]
NRECORDS = 6000


def _header_constants():
    with open(os.path.join(ROOT, "seeq_amd", "csrc", "seeq_fastq.h")) as f:
        text = f.read()
    return {k: int(v) for k, v in re.findall(r"^#define\s+SEEQ_FASTQ_(TILE|WG|ITEMS)\s+(\d+)", text, re.M)}


def _planted(rng):
    """Copies of both single-pattern test patterns within their distance, and of one more barcode of the set."""
    from seeq_amd import device as dev
    k = rng.randrange(len(BARCODES))
    parts = [_mutate(rng, PAT20, rng.randint(0, 3)), _mutate(rng, MER8, rng.randint(0, 1)),
             _mutate(rng, dev.plain_pattern(BARCODES[k]).replace("N", "A"), rng.randint(0, TAUS[k]))]
    rng.shuffle(parts)
    return "".join(p + "".join(rng.choice("ACGT") for _ in range(3)) for p in parts)


def _fastq_lines(n=NRECORDS, seed=11):
    rng = random.Random(seed + 1000)
    lines = []
    for seq in _mixed_lines(BARCODES, TAUS, n=n, seed=seed):
        if rng.random() < 0.03:                            # a foreign byte: SQ_FAIL / SQ_CONVERT / SQ_IGNORE differ on this line
            p = rng.randrange(len(seq))
            seq = seq[:p] + rng.choice("X-.") + seq[p + 1:]
        lines += ["@" + _planted(rng), seq, "+" + _planted(rng), seq]
    return lines


def _buf(lines, newline=True):
    return ("\n".join(lines) + ("\n" if newline and lines else "")).encode()


def _seq_only(lines, newline=True):
    return _buf(lines[1::4], newline)


def _seq_offsets(lines):
    """Byte offset of every record's sequence line in "\\n".join(lines): index r - 1 for record number r."""
    starts = np.concatenate(([0], np.cumsum([len(ln) + 1 for ln in lines])))[:len(lines)]
    return starts[1::4].astype(np.uint64)


@pytest.fixture(scope="module")
def fq():
    lines = _fastq_lines()
    return lines, _buf(lines), _seq_only(lines), _seq_offsets(lines)


@pytest.fixture(scope="module")
def pats():
    from seeq_amd import device as dev
    ps = [dev.Pattern(p, t) for p, t in PATTERNS]
    yield ps
    for p in ps:
        p.close()


@pytest.fixture(scope="module")
def barcode_pats():
    from seeq_amd import device as dev
    ps = [dev.Pattern(b, t) for b, t in zip(BARCODES, TAUS)]
    yield ps
    for p in ps:
        p.close()


def _counts(res):
    return {k: int(res[k]) for k in ("nlines", "nmatchlines", "nhits", "nrecords", "nheaders")}


def _scan_records(sc, pat, buf, options):
    """scan_host with WANT_RECORDS -> (counts, records, offsets)."""
    from seeq_amd import device as dev
    res = sc.scan_host(pat, buf, options, dev.WANT_RECORDS)
    return _counts(res), res["records"], sc.record_offsets(int(res["nrecords"]))


def _assert_is_oracle(got, exp, seq_off):
    cnt, rec, off = got
    print("nlines %d/%d nmatchlines %d/%d nrecords %d/%d" % (cnt["nlines"], exp["nlines"], cnt["nmatchlines"], exp["nmatchlines"],
                                                             cnt["nrecords"], len(exp["records"])))
    assert cnt["nlines"] == exp["nlines"]
    assert cnt["nmatchlines"] == exp["nmatchlines"]
    assert cnt["nhits"] == cnt["nrecords"] == len(exp["records"])
    assert cnt["nheaders"] == 0
    assert np.array_equal(rec.astype(np.uint64), exp["records"])
    if seq_off is not None:
        assert np.array_equal(off, seq_off[exp["records"][:, 0].astype(np.int64) - 1])


# ---- 1. parity ----
@pytest.mark.parametrize("nondna", [SQ_FAIL, SQ_CONVERT, SQ_IGNORE])
def test_fastq_parity_with_the_sequence_lines_alone(gpu, capi, oracle, fq, pats, nondna):
    from seeq_amd import device as dev
    lines, buf, seq, seq_off = fq
    sc = dev.Scanner()
    for (pattern, tau), pat in zip(PATTERNS, pats):
        for mo in (SQ_FIRST, SQ_BEST, SQ_ALL):
            exp = oracle.buffer_scan(pattern, tau, seq, mo | nondna)
            assert exp["nlines"] == NRECORDS and len(exp["records"]) > NRECORDS // 50
            _assert_is_oracle(_scan_records(sc, pat, buf, mo | nondna | dev.SEEQDEV_FASTQ), exp, seq_off)
            # the filter is doing work: what the unflagged scan of the same buffer returns beside the true records
            plain = sc.scan_host(pat, buf, mo | nondna, dev.WANT_RECORDS)
            false = int(plain["nrecords"]) - len(exp["records"])
            print(pattern, mo, nondna, "true", len(exp["records"]), "false", false)
            assert plain["nlines"] == 4 * NRECORDS
            assert false >= (1 if nondna == SQ_FAIL else 3) * len(exp["records"])
    sc.close()


# ---- 2. count wants ----
@pytest.mark.parametrize("nondna", [SQ_FAIL, SQ_IGNORE])
def test_fastq_count_wants(gpu, capi, oracle, fq, pats, nondna):
    from seeq_amd import device as dev
    lines, buf, seq, _ = fq
    sc = dev.Scanner()
    for (pattern, tau), pat in zip(PATTERNS, pats):
        expa = oracle.buffer_scan(pattern, tau, seq, SQ_ALL | nondna)
        c1 = sc.scan_host(pat, buf, nondna | dev.SEEQDEV_FASTQ, dev.WANT_COUNTLINES)
        assert _counts(c1) == dict(nlines=NRECORDS, nmatchlines=expa["nmatchlines"], nhits=expa["nmatchlines"], nrecords=0, nheaders=0)
        with pytest.raises(dev.SeeqDeviceError):
            sc.records(1)
        # (the match bits a caller leaves in `options` do not matter to a count want, as without the flag)
        c2 = sc.scan_host(pat, buf, SQ_BEST | nondna | dev.SEEQDEV_FASTQ, dev.WANT_COUNTMATCH)
        assert _counts(c2) == dict(nlines=NRECORDS, nmatchlines=expa["nmatchlines"], nhits=len(expa["records"]), nrecords=0, nheaders=0)
        assert len(expa["records"]) >= expa["nmatchlines"] > 0
        with pytest.raises(dev.SeeqDeviceError):
            sc.records(1)
        assert len(sc.records(0)) == 0
    sc.close()


# ---- 3. filter boundaries ----
FILLER = "AC" * 75


def _boundary_lines(nlines, planted):
    """150-base lines; the raw lines (0-based) in `planted` carry the pattern, the others nothing that matches."""
    lines = [FILLER] * nlines
    for i in planted:
        p = (i * 7) % 130
        lines[i] = FILLER[:p] + PAT20 + FILLER[p + 20:]
    return lines


def _boundary_cases():
    c = _header_constants()
    tile, wg = c["TILE"], c["WG"]
    assert tile == wg * c["ITEMS"]
    return tile, wg, ["none", "one_other_line", "one_sequence_line", tile - 1, tile, tile + 1, tile * wg + tile + 3]


@pytest.mark.parametrize("case", range(7))
def test_fastq_filter_boundaries(gpu, capi, oracle, pats, case):
    """The unflagged record count n -- what the filter reads -- at 0, at 1 (kept and not kept), around one tile of the filter,
    and beyond tile x workgroup size (the top level of its scan then takes more than one round)."""
    from seeq_amd import device as dev
    tile, wg, cases = _boundary_cases()
    what = cases[case]
    if what == "none":
        nlines, planted = 8, []
    elif what == "one_other_line":
        nlines, planted = 8, [4]
    elif what == "one_sequence_line":
        nlines, planted = 8, [5]
    else:
        nlines = what + what // 3 + 5                      # (+ 5: a partial last record)
        planted = random.Random(what).sample(range(nlines), what)
    lines = _boundary_lines(nlines, planted)
    buf = _buf(lines)
    sc = dev.Scanner()
    plain = sc.scan_host(pats[0], buf, SQ_BEST, dev.WANT_RECORDS)
    assert plain["nrecords"] == len(planted) and plain["nlines"] == nlines          # n is what the case says
    exp = oracle.buffer_scan(PAT20, 3, _seq_only(lines), SQ_BEST)
    assert len(exp["records"]) == sum(1 for i in planted if i % 4 == 1)
    assert exp["nlines"] == (nlines + 2) // 4
    _assert_is_oracle(_scan_records(sc, pats[0], buf, SQ_BEST | dev.SEEQDEV_FASTQ), exp, _seq_offsets(lines))
    sc.close()


# ---- 4. tails ----
@pytest.mark.parametrize("newline", [True, False])
@pytest.mark.parametrize("extra", [0, 1, 2, 3])
def test_fastq_tails(gpu, capi, oracle, fq, pats, extra, newline):
    """4k, 4k + 1, 4k + 2, 4k + 3 raw lines, with and without a final newline: a partial last record counts iff its sequence line
    is there."""
    from seeq_amd import device as dev
    lines = fq[0][:40 + extra]
    buf = _buf(lines, newline)
    sc = dev.Scanner()
    for (pattern, tau), pat in zip(PATTERNS, pats):
        exp = oracle.buffer_scan(pattern, tau, _seq_only(lines, newline), SQ_ALL | SQ_IGNORE)
        assert exp["nlines"] == (10 if extra < 2 else 11)
        _assert_is_oracle(_scan_records(sc, pat, buf, SQ_ALL | SQ_IGNORE | dev.SEEQDEV_FASTQ), exp, _seq_offsets(lines))
    sc.close()


# ---- 5. segments, resident text, the context afterwards ----
def test_fastq_small_segments_resident_text_and_the_context_afterwards(gpu, capi, oracle, fq, pats, monkeypatch):
    import torch
    from seeq_amd import device as dev
    lines, buf, seq, seq_off = fq
    pattern, tau = PATTERNS[0]
    opt = SQ_ALL | SQ_CONVERT
    exp = oracle.buffer_scan(pattern, tau, seq, opt)
    fresh = dev.Scanner()
    want_plain = _scan_records(fresh, pats[0], buf, opt)
    whole = _scan_records(fresh, pats[0], buf, opt | dev.SEEQDEV_FASTQ)
    fresh.close()
    monkeypatch.setenv("SEEQ_SEGMENT_BYTES", str(8 * 8192))      # (read when the context is made)
    sc = dev.Scanner()
    monkeypatch.delenv("SEEQ_SEGMENT_BYTES")
    assert len(buf) > 10 * 8 * 8192
    host = _scan_records(sc, pats[0], buf, opt | dev.SEEQDEV_FASTQ)
    _assert_is_oracle(host, exp, seq_off)
    t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    cnt = _counts(sc.scan_tensor(pats[0], t, opt | dev.SEEQDEV_FASTQ, dev.WANT_RECORDS))
    resident = (cnt, sc.records(cnt["nrecords"]), sc.record_offsets(cnt["nrecords"]))
    for got in (resident, whole):
        assert got[0] == host[0] and got[1].tobytes() == host[1].tobytes() and got[2].tobytes() == host[2].tobytes()
    # a second fetch of the same scan answers the same (the records are not filtered twice)
    assert _counts(sc.fetch()) == cnt and sc.records(cnt["nrecords"]).tobytes() == host[1].tobytes()
    # the context, without the flag again: a fresh context's answer
    again = _scan_records(sc, pats[0], buf, opt)
    assert again[0] == want_plain[0] and again[1].tobytes() == want_plain[1].tobytes() and again[2].tobytes() == want_plain[2].tobytes()
    assert again[0]["nlines"] == 4 * NRECORDS and again[0]["nrecords"] > 3 * host[0]["nrecords"]
    sc.close()


# ---- 6. demultiplexing ----
@pytest.mark.parametrize("nondna", [SQ_FAIL, SQ_CONVERT])
@pytest.mark.parametrize("sequential", [False, True])
def test_fastq_demux(gpu, capi, oracle, fq, barcode_pats, sequential, nondna, monkeypatch):
    import torch
    from seeq_amd import device as dev
    lines, buf, seq, _ = fq
    exp = _expected(oracle, BARCODES, TAUS, seq, SQ_BEST | nondna)
    assert exp[3] == NRECORDS and len(exp[0]) > NRECORDS // 4
    if sequential:
        monkeypatch.setenv("SEEQ_MULTI", "sequential")
    sc = dev.Scanner()
    host = sc.demux_host(barcode_pats, buf, nondna | dev.SEEQDEV_FASTQ)
    _check(host, exp)
    if sequential:
        assert not sc.last_multi_one_pass()
    t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    res = sc.demux_tensor(barcode_pats, t, nondna | dev.SEEQDEV_FASTQ)
    _check(res, exp)
    assert res["records"].tobytes() == host["records"].tobytes()
    # the filter is doing work, and the context demultiplexes plain lines as ever afterwards
    plain = sc.demux_host(barcode_pats, buf, nondna)
    _check(plain, _expected(oracle, BARCODES, TAUS, buf, SQ_BEST | nondna))
    assert plain["nlines"] == 4 * NRECORDS and plain["nassigned"] >= 2 * host["nassigned"]
    sc.close()


# ---- 7. refusals ----
def test_fastq_refusals_leave_the_context_usable(gpu, capi, oracle, fq, pats, barcode_pats):
    import torch
    from seeq_amd import device as dev
    lines, buf, seq, seq_off = fq
    small = _buf(lines[:400])
    FQ = dev.SEEQDEV_FASTQ
    L = capi.lib()
    sc = dev.Scanner()
    t = torch.frombuffer(bytearray(small), dtype=torch.uint8).cuda()

    def refused(call):
        C.set_errno(0)
        with pytest.raises(dev.SeeqDeviceError):
            call()
        assert C.get_errno() == errno.EINVAL

    for other in (dev.SEEQDEV_FASTA, capi.SEEQDEV_SINGLELINE, SQ_STREAM):
        refused(lambda: sc.scan_host(pats[0], small, FQ | other, dev.WANT_RECORDS))
        refused(lambda: sc.run(pats[0], t.data_ptr(), t.numel(), FQ | other, dev.WANT_COUNTLINES))
        refused(lambda: sc.demux_host(barcode_pats, small, FQ | other))
        refused(lambda: sc.demux_tensor(barcode_pats, t, FQ | other))
    refused(lambda: sc.scan_host_multi(pats, small, FQ | SQ_BEST, dev.WANT_RECORDS))
    refused(lambda: sc.scan_tensor_multi(pats, t, FQ | SQ_BEST, dev.WANT_RECORDS))
    reads = ("ACGT" * 10 + "\n") * 64
    bases, nmask, n = dev.pack_reads(reads.encode(), 40)
    pb, pn = torch.from_numpy(bases).cuda(), torch.from_numpy(nmask).cuda()
    refused(lambda: sc.run_packed(pats[1], pb.data_ptr(), pn.data_ptr(), n, 40, options=FQ, want=dev.WANT_RECORDS))
    sc.run_packed(pats[1], pb.data_ptr(), pn.data_ptr(), n, 40, options=0, want=dev.WANT_RECORDS)      # (the same call without the flag is fine)
    assert sc.fetch()["nlines"] == 64
    rec, nrec = C.c_void_p(), C.c_size_t()
    C.set_errno(0)
    assert L.seeqdevStringMatch(C.c_void_p(sc._h), C.c_void_p(pats[1].handle), C.c_char_p(b"TTACGTTGCATT"), C.c_size_t(12), C.c_int(FQ),
                                C.byref(rec), C.byref(nrec)) == -1
    assert C.get_errno() == errno.EINVAL
    assert L.seeqdevStringMatch(C.c_void_p(sc._h), C.c_void_p(pats[1].handle), C.c_char_p(b"TTACGTTGCATT"), C.c_size_t(12), C.c_int(0),
                                C.byref(rec), C.byref(nrec)) == 0 and nrec.value == 1
    # the context still answers, flagged and unflagged
    pattern, tau = PATTERNS[0]
    _assert_is_oracle(_scan_records(sc, pats[0], buf, SQ_BEST | FQ), oracle.buffer_scan(pattern, tau, seq, SQ_BEST), seq_off)
    e = oracle.buffer_scan(pattern, tau, small, SQ_BEST)
    r = sc.scan_host(pats[0], small, SQ_BEST, dev.WANT_RECORDS)
    assert r["nlines"] == e["nlines"] == 400 and np.array_equal(r["records"].astype(np.uint64), e["records"])
    sc.close()
