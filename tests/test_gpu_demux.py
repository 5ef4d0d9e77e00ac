"""GPU (-m gpu): demultiplexing on the device (seeqdevScanRunDemux / seeqdevScanHostDemux) -- per line the best pattern of a
set, the runner-up's margin, in line order -- against a pure-Python fold of the oracle's per-pattern SQ_BEST records, on the
one-walk path and on every way of scanning a set pattern by pattern."""
import ctypes as C
import errno
import random

import numpy as np
import pytest

from oracle.pyoracle import SQ_BEST, SQ_CONVERT, SQ_IGNORE

pytestmark = pytest.mark.gpu
PAT20 = "GATGTAGCGCGATTAGCCTG"
BARCODES = ["ACGTTGCA", "TTGACCGA", "GGCATTAC", "CAGTGTCA", "ATATCGCG", "GATTACAG", PAT20, "TG[AC]CANNGT"]
TAUS = [1, 1, 1, 2, 0, 1, 3, 1]
FIELDS = ("line", "start", "end", "dist", "pattern", "margin")


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


def _mixed_lines(barcodes, taus, n=4000, seed=11, lengths=(40, 75, 150, 151)):
    """The text of test_gpu_parity.py::test_multi_pattern_scan_vs_independent_oracle_scans, built the same way."""
    from seeq_amd import device as dev
    rng = random.Random(seed)
    lines = []
    for _ in range(n):
        m = rng.choice(lengths)
        t = [rng.choice("ACGT") for _ in range(m)]
        for _ in range(rng.choice([0, 1, 1, 2])):
            k = rng.randrange(len(barcodes))
            c = _mutate(rng, dev.plain_pattern(barcodes[k]).replace("N", "A"), rng.randint(0, taus[k] + 1))
            p = rng.randrange(0, max(1, m - len(c)))
            t[p:p + len(c)] = list(c)
        if rng.random() < 0.02:
            t[rng.randrange(m)] = "N"
        lines.append("".join(t)[:m])
    return lines


def _expected(oracle, barcodes, taus, buf, options=SQ_BEST, fasta=False):
    """Pure-Python demultiplexing of the oracle's per-pattern records -> (records as a list of tuples, assigned per pattern,
    nambiguous, nlines)."""
    per_line = {}
    nlines = None
    for k, (b, t) in enumerate(zip(barcodes, taus)):
        e = oracle.buffer_scan(b, t, buf, options & 0xFF, fasta=fasta)
        nlines = e["nlines"]
        for ln, s, en, d in e["records"].tolist():
            per_line.setdefault(ln, []).append((d, k, s, en))
    rows, assigned, amb = [], [0] * len(barcodes), 0
    for ln in sorted(per_line):
        cand = per_line[ln]
        d, k, s, en = min(cand, key=lambda c: (c[0], c[1]))
        others = [c[0] for c in cand if c[1] != k]
        margin = 255 if not others else min(255, min(others) - d)
        rows.append((ln, s, en, d, k, margin))
        assigned[k] += 1
        amb += margin == 0
    return rows, assigned, amb, nlines


def _rows(res):
    rec = res["records"]
    return list(zip(*(rec[f].tolist() for f in FIELDS)))


def _check(res, exp):
    rows, assigned, amb, nlines = exp
    assert res["nlines"] == nlines
    assert res["nassigned"] == len(rows) == len(res["records"])
    assert res["assigned"] == assigned
    assert res["nambiguous"] == amb
    got = _rows(res)
    if got != rows:
        bad = next(i for i, (a, b) in enumerate(zip(got, rows)) if a != b) if len(got) == len(rows) else None
        raise AssertionError("records differ (%d vs %d; first difference at %s: %s vs %s)"
                             % (len(got), len(rows), bad, got[bad] if bad is not None else None, rows[bad] if bad is not None else None))


def _dense_equal(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def mixed():
    lines = _mixed_lines(BARCODES, TAUS)
    return lines, ("\n".join(lines) + "\n").encode()


@pytest.fixture(scope="module")
def pats():
    from seeq_amd import device as dev
    ps = [dev.Pattern(b, t) for b, t in zip(BARCODES, TAUS)]
    yield ps
    for p in ps:
        p.close()


def test_demux_one_walk_vs_oracle_fold(gpu, capi, oracle, mixed, pats):
    from seeq_amd import device as dev
    lines, buf = mixed
    sc = dev.Scanner()
    res = sc.demux_host(pats, buf)
    assert sc.last_multi_one_pass()                        # the set has a union automaton: one walk, records never leave the device
    exp = _expected(oracle, BARCODES, TAUS, buf)
    _check(res, exp)
    assert res["nassigned"] > len(lines) // 4
    # the same as assign_best over the multi scan's records
    dense = dev.assign_best(sc.scan_host_multi(pats, buf, SQ_BEST, dev.WANT_RECORDS), len(lines))
    assert _dense_equal(dev.demux_dense(res, len(lines)), dense)
    # SQ_FIRST in options: SQ_BEST is implied
    assert _rows(sc.demux_host(pats, buf, 0)) == exp[0]
    sc.close()


@pytest.mark.parametrize("case", ["sequential", "convert", "ignore", "fasta", "long_lines", "33_patterns", "one_pattern", "no_union"])
def test_demux_per_pattern_paths(gpu, capi, oracle, mixed, pats, case, monkeypatch):
    """Every way a set is scanned pattern by pattern: the records are folded on the device scan by scan, and the result is
    that of the pure-Python fold -- byte for byte that of the one walk where both apply."""
    from seeq_amd import device as dev
    lines, buf = mixed
    sc = dev.Scanner()
    barcodes, taus, p, opt, fasta, other = BARCODES, TAUS, pats, 0, False, None
    own = []
    if case == "sequential":
        other = sc.demux_host(pats, buf)
        monkeypatch.setenv("SEEQ_MULTI", "sequential")
    elif case == "convert":
        opt = SQ_CONVERT
        rng = random.Random(5)
        buf = bytes(c if c == 10 or rng.random() > 0.01 else ord("X") for c in buf)
    elif case == "ignore":
        opt = SQ_IGNORE
        rng = random.Random(6)
        buf = bytes(c if c == 10 or rng.random() > 0.01 else ord("-") for c in buf)
    elif case == "fasta":
        opt, fasta = dev.SEEQDEV_FASTA, True
        buf = b"".join(b">read%d\n%s\n" % (i, ln.encode()) for i, ln in enumerate(lines[:1500]))
    elif case == "long_lines":
        buf = b"\n".join(b"".join(ln.encode() for ln in lines[i:i + 12]) for i in range(0, len(lines), 12)) + b"\n"
    elif case == "33_patterns":
        rng = random.Random(7)
        barcodes = BARCODES + ["".join(rng.choice("ACGT") for _ in range(8)) for _ in range(25)]
        taus = TAUS + [1] * 25
        own = p = [dev.Pattern(b, t) for b, t in zip(barcodes, taus)]
    elif case == "one_pattern":
        barcodes, taus, p = BARCODES[:1], TAUS[:1], pats[:1]
    elif case == "no_union":
        barcodes, taus = [PAT20, "TTGACCGATTGACCGATTGA"], [6, 6]
        own = p = [dev.Pattern(b, t) for b, t in zip(barcodes, taus)]
    res = sc.demux_host(p, buf, opt)
    if case in ("sequential", "ignore", "33_patterns", "one_pattern"):
        assert not sc.last_multi_one_pass(), case
    exp = _expected(oracle, barcodes, taus, buf, SQ_BEST | opt, fasta=fasta)
    _check(res, exp)
    if case != "one_pattern":
        assert res["nassigned"] > 0
    if other is None:                                      # whichever way this set was scanned: the bytes of a scan per pattern
        monkeypatch.setenv("SEEQ_MULTI", "sequential")
        other = sc.demux_host(p, buf, opt)
        monkeypatch.delenv("SEEQ_MULTI")
    assert other["records"].tobytes() == res["records"].tobytes()
    assert {k: v for k, v in other.items() if k != "records"} == {k: v for k, v in res.items() if k != "records"}
    if case in ("convert", "fasta", "long_lines"):         # demux_dense == assign_best over the multi scan of the same text
        nl = res["nlines"]
        dense = dev.assign_best(sc.scan_host_multi(p, buf, SQ_BEST | opt, dev.WANT_RECORDS), nl)
        assert _dense_equal(dev.demux_dense(res, nl), dense)
    sc.close()
    for q in own:
        q.close()


def test_demux_ties_and_a_pattern_that_never_matches(gpu, capi, oracle, mixed, monkeypatch):
    """The same barcode at index 2 and 5: every line it wins goes to 2 with margin 0 (ambiguous); a pattern that never matches
    never wins."""
    from seeq_amd import device as dev
    lines, buf = mixed
    barcodes = ["ACGTTGCA", "TTGACCGA", "GGCATTAC", "CAGTGTCA", "ATATCGCG", "GGCATTAC", "CCCCCCCCCCCCCCCCCCCCCCCCCCCCCC"]
    taus = [1, 1, 1, 2, 0, 1, 0]
    ps = [dev.Pattern(b, t) for b, t in zip(barcodes, taus)]
    sc = dev.Scanner()
    for seq in (False, True):
        if seq:
            monkeypatch.setenv("SEEQ_MULTI", "sequential")
        res = sc.demux_host(ps, buf)
        _check(res, _expected(oracle, barcodes, taus, buf))
        rec = res["records"]
        assert res["assigned"][5] == 0 and res["assigned"][6] == 0
        tied = rec[rec["pattern"] == 2]
        assert len(tied) > 0 and (tied["margin"] == 0).all()
        assert res["nambiguous"] >= len(tied)
    sc.close()
    for p in ps:
        p.close()


@pytest.mark.parametrize("text", [b"", b"ACGTTGCA", b"\n\n\n", b"GGGGGGGG\nAAAAAAAAA\n", b"\n\nACGTTGCAxx\n\nTTGACCGA", b"AC\xffGTTGCA\n\x7fTTGACCGA\n"])
def test_demux_edges(gpu, capi, oracle, pats, text):
    """Empty text, no trailing newline, empty lines, no line assigned (zero records), foreign bytes."""
    from seeq_amd import device as dev
    sc = dev.Scanner()
    res = sc.demux_host(pats, text)
    _check(res, _expected(oracle, BARCODES, TAUS, text))
    assert len(sc.demux_records(0)) == 0
    sc.close()


def test_demux_small_segments(gpu, capi, oracle, mixed, pats, monkeypatch):
    from seeq_amd import device as dev
    lines, buf = mixed
    monkeypatch.setenv("SEEQ_SEGMENT_BYTES", "65536")
    sc = dev.Scanner()
    buf3 = buf * 3
    _check(sc.demux_host(pats, buf3), _expected(oracle, BARCODES, TAUS, buf3))
    sc.close()


def test_demux_resident_tensor_and_device_pointer(gpu, capi, mixed, pats):
    import torch
    from seeq_amd import device as dev
    lines, buf = mixed
    sc = dev.Scanner()
    host = sc.demux_host(pats, buf)
    t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    res = sc.demux_tensor(pats, t)
    assert res["records"].tobytes() == host["records"].tobytes()
    assert {k: v for k, v in res.items() if k != "records"} == {k: v for k, v in host.items() if k != "records"}
    lazy = sc.demux_tensor(pats, t, copy=False)
    assert lazy["records"] is None and lazy["nassigned"] == host["nassigned"]
    n = lazy["nassigned"]
    ptr = sc.demux_device_ptr()
    assert ptr
    # the device array, read by torch: the same bytes as the copy

    class View:
        __cuda_array_interface__ = {"shape": (n * 16,), "typestr": "|u1", "data": (ptr, False), "version": 2, "strides": None}

    dev_bytes = torch.as_tensor(View(), device="cuda").cpu().numpy()
    assert dev_bytes.tobytes() == host["records"].tobytes()
    assert sc.demux_records(10, first=5).tobytes() == host["records"][5:15].tobytes()
    with pytest.raises(dev.SeeqDeviceError):
        sc.demux_records(2, first=n - 1)
    sc.close()


def test_demux_tiny_workspace(gpu, capi, oracle, mixed, pats, monkeypatch):
    from seeq_amd import device as dev
    lines, buf = mixed
    exp = _expected(oracle, BARCODES, TAUS, buf)
    for seq in (False, True):
        if seq:
            monkeypatch.setenv("SEEQ_MULTI", "sequential")
        sc = dev.Scanner()
        sc.reserve(0, 10, 2, 1)                             # absurdly small: every capacity overflows
        _check(sc.demux_host(pats, buf), exp)
        sc.close()


def test_demux_then_scan_then_another_set(gpu, capi, oracle, mixed, pats):
    """One Scanner: demux -> a plain single-pattern scan -> a demux of a different set: every result correct."""
    from seeq_amd import device as dev
    lines, buf = mixed
    sc = dev.Scanner()
    _check(sc.demux_host(pats, buf), _expected(oracle, BARCODES, TAUS, buf))
    with pytest.raises(dev.SeeqDeviceError):
        sc.fetch()                                          # nothing left to fetch: the demux's scans are complete
    r = sc.scan_host(pats[6], buf, SQ_BEST, dev.WANT_RECORDS)
    e = oracle.buffer_scan(PAT20, 3, buf, SQ_BEST)
    assert r["nmatchlines"] == e["nmatchlines"] and np.array_equal(r["records"].astype(np.uint64), e["records"])
    other_b, other_t = ["GATTACAG", "CAGTGTCA", "TGACCGAT"], [1, 0, 1]
    other = [dev.Pattern(b, t) for b, t in zip(other_b, other_t)]
    _check(sc.demux_host(other, buf), _expected(oracle, other_b, other_t, buf))
    sc.close()
    for p in other:
        p.close()


def test_demux_argument_errors(gpu, capi, pats):
    from seeq_amd import device as dev
    L = capi.lib()
    sc = dev.Scanner()
    text = b"ACGTTGCA\n"
    cnt = capi.seeqdev_demux_counts_t()
    arr = (C.c_void_p * 256)(*([C.cast(pats[0].handle, C.c_void_p)] * 256))

    def einval(npat, p=arr, opt=0):
        C.set_errno(0)
        assert L.seeqdevScanHostDemux(sc._h, p, npat, text, len(text), opt, C.byref(cnt), None) == -1
        assert C.get_errno() == errno.EINVAL

    einval(0)
    einval(256)
    einval(2, p=None)
    einval(2, opt=capi.SQ_ALL)
    assert L.seeqdevScanHostDemux(sc._h, arr, 255, text, len(text), 0, C.byref(cnt), None) == 0     # 255 is allowed
    assert cnt.nassigned == 1
    sc.close()


def test_demux_two_million_planted_reads(gpu, capi):
    """About 2 M synthetic reads with planted barcodes (profiles/multi_bench.py's generator): the device demultiplex equals
    assign_best of the multi scan, and copy=False gives the same counts."""
    import os
    import sys
    import torch
    from seeq_amd import device as dev
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
    from multi_bench import make_reads
    rng = np.random.default_rng(3)
    barcodes = ["".join("ACGT"[i] for i in rng.integers(0, 4, size=8)) for _ in range(16)]
    n = 2_000_000
    text = make_reads(n, 150, barcodes, 0.9, 17)
    ps = [dev.Pattern(b, 1) for b in barcodes]
    sc = dev.Scanner(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    res = sc.demux_tensor(ps, text)
    assert sc.last_multi_one_pass()
    assert res["nlines"] == n and res["nassigned"] > n // 2
    dense = dev.assign_best(sc.scan_tensor_multi(ps, text, SQ_BEST, dev.WANT_RECORDS), n)
    assert _dense_equal(dev.demux_dense(res, n), dense)
    lazy = sc.demux_tensor(ps, text, copy=False)
    assert {k: v for k, v in lazy.items() if k != "records"} == {k: v for k, v in res.items() if k != "records"}
    assert sc.demux_records(lazy["nassigned"]).tobytes() == res["records"].tobytes()
    sc.close()
    for p in ps:
        p.close()
