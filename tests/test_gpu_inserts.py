"""GPU (-m gpu): the insert between two flanks (seeqdevScanRunInserts / seeqdevScanHostInserts / seeqdevScanInsertText) -- the text scanned
with a right flank under SQ_ALL and a left flank under SQ_BEST or SQ_FIRST, the two record sets joined on the device, the inserts cut
out of the text there -- against a pure-Python join of two oracle scans by the rule of seeq_insert.h and a host-built insert text."""
import ctypes as C
import errno
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle.pyoracle import SQ_ALL, SQ_BEST, SQ_CONVERT, SQ_FIRST, SQ_IGNORE
from test_gpu_strands import _buf, _line_offsets, _mutate, _step

pytestmark = pytest.mark.gpu
PAIRS = {"pair20": (("GATGTAGCGCGATTAGCCTG", 3), ("TTCACTGGAGTTGTCCCAAT", 3)), "short": (("TG[AC]CANNGT", 1), ("ACGTTGCA", 1))}
MODES = {"best": SQ_BEST, "first": SQ_FIRST}
WINDOWS = [(0, 0), (10, 14), (1, 0)]
KINDS = ["LR", "LR", "LR", "LRR", "RL", "L", "R", "", "LLR", "RLR"]
GAPS = [0, 1, 5, 12, 12, 12, 20, 30, 60]
FIELDS = ("line", "start", "end", "ldist", "rdist")
COUNTS = ("nlines", "nleft", "nright", "nboth", "ninserts", "text_bytes")
# sixteen 12-base barcodes (what stands in the 12-base gaps), demultiplexed at distance 1
BARCODES = ["ACGTTGCAAGCT", "TTGACCGATCAG", "GGCATTACCGTA", "CAGTGTCATTGC", "ATATCGCGGATC", "GATTACAGACTG", "CCTAGGTTAACG", "TGCAACTGGTCA",
            "AAGGCCTTCAGT", "GTCAGTCAAGTC", "CTTGAACCGGAT", "TCAGGACTTCGA", "AGCTCTAGGTAC", "GGTTAACCTGAG", "CACAGTGTCTGA", "TACGTACGCATG"]

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


def _lines(pair, n=4000, seed=7, kinds=KINDS, gaps=GAPS):
    """n lines; each a kind drawn from `kinds`: its letters are plants of the left (L) or right (R) flank's plain form, mutated by
    0 .. tau + 1 edits, with a gap drawn from `gaps` of random bases between consecutive plants (a gap of 12: one of BARCODES) and 1 - 19
    random bases before the first and after the last; 2 % of the lines carry one N."""
    from seeq_amd import device as dev
    rng = random.Random(seed)
    plain = {"L": (dev.plain_pattern(pair[0][0]), pair[0][1]), "R": (dev.plain_pattern(pair[1][0]), pair[1][1])}
    bases = lambda m: "".join(rng.choice("ACGT") for _ in range(m))      # noqa: E731
    lines = []
    for _ in range(n):
        t = [bases(rng.randint(1, 19))]
        for j, which in enumerate(rng.choice(kinds)):
            if j:
                g = rng.choice(gaps)
                t.append(rng.choice(BARCODES) if g == 12 else bases(g))
            t.append(_mutate(rng, plain[which][0], rng.randint(0, plain[which][1] + 1)))
        t.append(bases(rng.randint(1, 19)))
        s = list("".join(t))
        if rng.random() < 0.02:
            s[rng.randrange(len(s))] = "N"
        lines.append("".join(s))
    return lines


class Joined:
    """Two oracle scans of one buffer (left under `mode`, right under SQ_ALL) and their join by the rule, for any window."""

    def __init__(self, oracle, pair, buf, mode, opt=0, fasta=False):
        (le, lt), (ri, rt) = pair
        self.mode = mode
        el = oracle.buffer_scan(le, lt, buf, (mode | opt) & 0xFF, fasta=fasta)
        er = oracle.buffer_scan(ri, rt, buf, (SQ_ALL | opt) & 0xFF, fasta=fasta)
        assert el["nlines"] == er["nlines"]
        self.nlines = el["nlines"]
        self.left = [tuple(r) for r in el["records"].tolist()]
        self.right = {}
        for r in er["records"].tolist():
            self.right.setdefault(r[0], []).append(tuple(r))
        assert len({r[0] for r in self.left}) == len(self.left)

    def admissible(self, l, window):
        lo, hi = window
        return [r for r in self.right.get(l[0], []) if r[1] >= l[2] + lo and (hi == 0 or r[1] <= l[2] + hi)]

    def rows(self, window):
        pick = (lambda r: (r[3], r[2])) if self.mode == SQ_BEST else (lambda r: r[2])
        out = []
        for l in self.left:
            adm = self.admissible(l, window)
            if adm:
                r = min(adm, key=pick)
                out.append((l[0], l[2], r[1], l[3], r[3]))
        return out

    def counts(self, window):
        rows = self.rows(window)
        return dict(nlines=self.nlines, nleft=len(self.left), nright=len(self.right), nboth=sum(1 for l in self.left if l[0] in self.right),
                    ninserts=len(rows), text_bytes=sum(r[2] - r[1] + 1 for r in rows))


def _host_text(buf, rows, offsets):
    return b"".join(buf[offsets[r[0]] + r[1]:offsets[r[0]] + r[2]] + b"\n" for r in rows)


def _rows(res):
    rec = res["records"]
    return list(zip(*(rec[f].tolist() for f in FIELDS)))


def _check(sc, res, joined, window, offsets):
    exp = joined.rows(window)
    assert {k: res[k] for k in COUNTS} == joined.counts(window)
    assert len(res["records"]) == len(exp)
    got = _rows(res)
    if got != exp:
        bad = next(i for i, (a, b) in enumerate(zip(got, exp)) if a != b) if len(got) == len(exp) else None
        raise AssertionError("records differ (%d vs %d; first difference at %s: %s vs %s)"
                             % (len(got), len(exp), bad, got[bad] if bad is not None else None, exp[bad] if bad is not None else None))
    assert sc.insert_offsets(len(got)).tolist() == [offsets[r[0]] for r in exp]


@pytest.fixture(scope="module")
def texts():
    """Per flank pair: its lines, their buffer and line offsets, made once."""
    out = {}
    for name, pair in PAIRS.items():
        lines = _lines(pair)
        buf = _buf(lines)
        out[name] = (lines, buf, _line_offsets(buf))
    return out


@pytest.fixture(scope="module")
def joined(oracle, texts):
    memo = {}

    def get(name, mode):
        if (name, mode) not in memo:
            memo[name, mode] = Joined(oracle, PAIRS[name], texts[name][1], mode)
        return memo[name, mode]
    return get


@pytest.fixture(scope="module")
def pats():
    from seeq_amd import device as dev
    ps = {name: (dev.Pattern(*pair[0]), dev.Pattern(*pair[1])) for name, pair in PAIRS.items()}
    yield ps
    for l, r in ps.values():
        l.close()
        r.close()


def test_the_text_exercises_every_branch_of_the_rule(gpu, texts, joined):
    """What the construction gives (the oracle's numbers), for both pairs and both modes: inserts over more than one tile, lines with one
    flank only, with both and nothing admissible, with several admissible records, ties at the smallest distance, right records before
    the left one, a chosen record that is not the first admissible one, empty inserts."""
    for name in PAIRS:
        lines = texts[name][0]
        assert len(lines) == 4000 and all(0 < len(ln) <= 230 for ln in lines)
        for mode in (SQ_BEST, SQ_FIRST):
            j = joined(name, mode)
            w = (0, 0)
            rows = j.rows(w)
            what = (name, mode)
            assert len(rows) > 1024, what
            assert sum(1 for l in j.left if l[0] not in j.right) > 100, what
            assert sum(1 for l in j.left if l[0] in j.right and not j.admissible(l, w)) > 100, what
            several = [j.admissible(l, w) for l in j.left if len(j.admissible(l, w)) > 1]
            assert len(several) > 100, what
            assert sum(1 for adm in several if sum(1 for r in adm if r[3] == min(q[3] for q in adm)) >= 2) > 30, what
            assert sum(1 for l in j.left if any(r[1] < l[2] for r in j.right.get(l[0], []))) > 100, what
            if mode == SQ_BEST:
                by_line = {r[0]: r for r in rows}
                assert sum(1 for l in j.left if l[0] in by_line and by_line[l[0]][2] != min(j.admissible(l, w), key=lambda r: r[2])[1]) > 30, what
            assert sum(1 for r in rows if r[1] == r[2]) > 30, what
            w = (10, 14)
            assert len(j.rows(w)) > 100, what
            assert sum(1 for l in j.left if l[0] in j.right and not j.admissible(l, w)) > 1000, what


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "%d_%d" % w)
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(PAIRS))
def test_inserts_vs_joined_oracle_scans(gpu, capi, texts, joined, pats, name, mode, window):
    import torch
    from seeq_amd import device as dev
    _, buf, offsets = texts[name]
    left, right = pats[name]
    j = joined(name, MODES[mode])
    sc = dev.Scanner()
    host = {}

    def check(s, res):
        _check(s, res, j, window, offsets)
        host.setdefault("res", res)
    _go(sc, "%s, %s, window %s, host entry" % (name, mode, window), lambda s: s.inserts_host(left, right, buf, MODES[mode], *window), check)
    t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    other = dev.Scanner()

    def check_tensor(s, res):
        _check(s, res, j, window, offsets)
        assert res["records"].tobytes() == host["res"]["records"].tobytes()
        assert {k: res[k] for k in COUNTS} == {k: host["res"][k] for k in COUNTS}
    _go(other, "%s, %s, window %s, resident entry" % (name, mode, window), lambda s: s.inserts_tensor(left, right, t, MODES[mode], *window), check_tensor)
    lazy = other.inserts_tensor(left, right, t, MODES[mode], *window, copy=False)
    assert "records" not in lazy and lazy["ninserts"] == host["res"]["ninserts"]
    n = lazy["ninserts"]
    assert n == 0 or other.inserts_device_ptr()
    assert other.insert_records(min(10, n), first=min(5, max(0, n - 10))).tobytes() == host["res"]["records"][min(5, max(0, n - 10)):][:min(10, n)].tobytes()
    sc.close()
    other.close()


def test_context_state_after_an_inserts_call(gpu, capi, oracle, texts, joined, pats):
    """After the call there is nothing to fetch; a plain scan on the same context equals that scan on a fresh one (records, path, runs);
    the inserts call after it gives the same bytes; a small text and then the large one on one context (its workspace grows).
    The runs: a context keeps the workspace its calls grew (seeq_amd.h: seeqdevScanFetch), so on the dense 4 000-line text, which a fresh
    context scans twice to grow its own, the context that has just scanned that text needs one run; on a text that a fresh context scans
    in one run the two agree."""
    from seeq_amd import device as dev
    _, buf, offsets = texts["pair20"]
    left, right = pats["pair20"]
    j = joined("pair20", SQ_BEST)
    sc = dev.Scanner()
    small = buf[:buf.index(b"\n", 3000) + 1]
    js = Joined(oracle, PAIRS["pair20"], small, SQ_BEST)
    _go(sc, "a small text first", lambda s: s.inserts_host(left, right, small, SQ_BEST, 0, 0), lambda s, res: _check(s, res, js, (0, 0), offsets))
    first = {}

    def keep(s, res):
        _check(s, res, j, (0, 0), offsets)
        first.setdefault("records", res["records"].tobytes())
        first.setdefault("offsets", s.insert_offsets(res["ninserts"]).tobytes())
    _go(sc, "the 4 000-line text on the same context", lambda s: s.inserts_host(left, right, buf, SQ_BEST, 0, 0), keep)
    with pytest.raises(dev.SeeqDeviceError):
        sc.fetch()                                          # nothing left to fetch: the call is complete
    with pytest.raises(dev.SeeqDeviceError):
        sc.records(1)
    fresh = dev.Scanner()
    for pat, mode in ((right, SQ_ALL), (left, SQ_BEST)):
        a = sc.scan_host(pat, buf, mode, dev.WANT_RECORDS)
        b = fresh.scan_host(pat, buf, mode, dev.WANT_RECORDS)
        assert a["records"].tobytes() == b["records"].tobytes() and a["nrecords"] > 1024
        assert {k: v for k, v in a.items() if k != "records"} == {k: v for k, v in b.items() if k != "records"}
        assert sc.last_path() == fresh.last_path() and sc.last_kernel() == fresh.last_kernel()
        print("dense text, mode", mode, "runs", sc.last_runs(), "fresh", fresh.last_runs())
        assert sc.last_runs() == 1 <= fresh.last_runs()
        assert sc.record_offsets(a["nrecords"]).tobytes() == fresh.record_offsets(b["nrecords"]).tobytes()
    fresh.close()
    sparse = _buf(_lines(PAIRS["pair20"], 3000, 61, kinds=[""] * 39 + ["LR"]))
    for pat, mode in ((right, SQ_ALL), (left, SQ_BEST)):
        fresh = dev.Scanner()
        a = sc.scan_host(pat, sparse, mode, dev.WANT_RECORDS)
        b = fresh.scan_host(pat, sparse, mode, dev.WANT_RECORDS)
        assert a["records"].tobytes() == b["records"].tobytes() and a["nrecords"] > 30
        assert {k: v for k, v in a.items() if k != "records"} == {k: v for k, v in b.items() if k != "records"}
        assert (sc.last_path(), sc.last_kernel(), sc.last_runs(), sc.fallback()) == (fresh.last_path(), fresh.last_kernel(), fresh.last_runs(), fresh.fallback())
        fresh.close()
    # the result of the inserts call is still there (arrays of its own), and the call repeated gives the same bytes
    assert sc.insert_records(j.counts((0, 0))["ninserts"]).tobytes() == first["records"]
    again = sc.inserts_host(left, right, buf, SQ_BEST, 0, 0)
    assert again["records"].tobytes() == first["records"] and sc.insert_offsets(again["ninserts"]).tobytes() == first["offsets"]
    assert sc.last_runs() == 1                              # the runs of the call's last scan: the left flank under SQ_BEST
    sc.close()


def _fastq(lines, seed, plant):
    """Four-line records around the lines, quality strings drawn from ACG!I -- every third one opens with `plant`, so that quality lines
    give records to a plain scan (under SQ_FAIL a line ends at its first foreign byte) -> (buffer, offsets: record r -> its sequence line)."""
    rng = random.Random(seed)
    raw = []
    for i, sq in enumerate(lines):
        qual = "".join(rng.choice("ACG!I") for _ in sq)
        if i % 3 == 0 and len(sq) > len(plant) + 2:
            qual = "AC" + plant + qual[len(plant) + 2:]
        raw += ["@read%d" % i, sq, "+", qual]
    buf = _buf(raw)
    raw_offsets = _line_offsets(buf)
    return buf, [None] + [raw_offsets[4 * r + 2] for r in range(len(lines))]


@pytest.mark.parametrize("case", ["fasta", "fastq", "convert", "ignore"])
def test_inserts_flags(gpu, capi, oracle, pats, case):
    """SEEQDEV_FASTA / SEEQDEV_FASTQ: the call over the sequence lines alone, except that the offsets are the original buffer's;
    -x 1 (SQ_CONVERT) and -x 2 (SQ_IGNORE) on a text with a few foreign bytes."""
    from seeq_amd import device as dev
    pair = PAIRS["short"]
    left, right = pats["short"]
    lines = _lines(pair, 1500, 41)
    seq_buf = _buf(lines)
    opt, fasta = 0, False
    if case == "fasta":
        buf = b"".join(b">read%d ACGTTGCA\n%s\n" % (i, ln.encode()) for i, ln in enumerate(lines))
        opt, fasta = dev.SEEQDEV_FASTA, True
        j = Joined(oracle, pair, buf, SQ_BEST, 0, True)
        offsets = _line_offsets(buf, True)
        assert j.rows((0, 0)) == Joined(oracle, pair, seq_buf, SQ_BEST).rows((0, 0))
    elif case == "fastq":
        buf, offsets = _fastq(lines, 42, dev.plain_pattern(pair[1][0]))
        opt = dev.SEEQDEV_FASTQ
        j = Joined(oracle, pair, seq_buf, SQ_BEST)
        # quality lines give records to a plain scan of the four-line buffer
        assert len(oracle.buffer_scan(pair[1][0], pair[1][1], buf, SQ_ALL)["records"]) > sum(len(v) for v in j.right.values()) + 20
    else:
        opt = SQ_CONVERT if case == "convert" else SQ_IGNORE
        rng = random.Random(43)
        buf = bytes(c if c == 10 or rng.random() > 0.01 else ord("X-"[case == "ignore"]) for c in seq_buf)
        j = Joined(oracle, pair, buf, SQ_BEST, opt)
        offsets = _line_offsets(buf)
    assert len(j.rows((0, 0))) > 300 and len(j.rows((10, 14))) > 50
    sc = dev.Scanner()
    for window in ((0, 0), (10, 14)):
        _go(sc, "%s, window %s" % (case, window), lambda s: s.inserts_host(left, right, buf, SQ_BEST | opt, *window),
            lambda s, res: _check(s, res, j, window, offsets))
        text = sc.insert_text()
        assert text == _host_text(buf, j.rows(window), offsets)
    sc.close()


def test_insert_text(gpu, capi, oracle, texts, joined, pats):
    """The insert text equals the host-built one; a scan of it counts ninserts lines; demultiplexing it on the device equals
    demultiplexing the host-built text; ERANGE below text_bytes with nothing written; guard bytes stay; the size query."""
    import torch
    from seeq_amd import device as dev
    _, buf, offsets = texts["pair20"]
    left, right = pats["pair20"]
    sc = dev.Scanner()
    t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    barcodes = [dev.Pattern(b, 1) for b in BARCODES]
    for mode, window in ((SQ_BEST, (10, 14)), (SQ_FIRST, (0, 0))):
        j = joined("pair20", mode)
        rows = j.rows(window)
        host_text = _host_text(buf, rows, offsets)
        got = {}

        def check(s, res):
            assert {k: res[k] for k in COUNTS} == j.counts(window) and res["text_bytes"] == len(host_text)
            assert s.insert_text_bytes() == len(host_text)
            got["text"] = s.insert_text(t)
            assert got["text"].dtype == torch.uint8 and got["text"].is_cuda and got["text"].cpu().numpy().tobytes() == host_text
        _go(sc, "insert text, mode %d, window %s" % (mode, window), lambda s: s.inserts_tensor(left, right, t, mode, *window, copy=False), check)
        other = dev.Scanner()
        cnt = other.scan_tensor(left, got["text"], SQ_FIRST, dev.WANT_COUNTLINES)
        assert cnt["nlines"] == len(rows)                   # output line k is record k: an empty insert is a line too
        d_dev = other.demux_tensor(barcodes, got["text"])
        d_host = dev.Scanner().demux_host(barcodes, host_text)
        assert d_dev["records"].tobytes() == d_host["records"].tobytes()
        assert {k: v for k, v in d_dev.items() if k != "records"} == {k: v for k, v in d_host.items() if k != "records"}
        if window == (10, 14):
            assert d_dev["nassigned"] > 100                 # the 12-base gaps hold barcodes
        other.close()
        # the raw entry: guard bytes on both sides, an output that is 16-byte aligned and one that is not
        n = len(host_text)
        lib, h = sc._lib, sc._h
        for shift in (32, 33):
            guard = torch.full((n + 96,), 0xAA, dtype=torch.uint8, device="cuda")
            size = C.c_uint64(0)
            C.set_errno(0)
            assert lib.seeqdevScanInsertText(h, C.c_void_p(t.data_ptr()), t.numel(), C.c_void_p(guard.data_ptr() + shift), n - 1, C.byref(size)) == -1
            assert C.get_errno() == errno.ERANGE and size.value == n
            assert bool((guard == 0xAA).all())              # nothing is written
            assert lib.seeqdevScanInsertText(h, C.c_void_p(t.data_ptr()), t.numel(), C.c_void_p(guard.data_ptr() + shift), n, C.byref(size)) == 0
            out = guard.cpu().numpy().tobytes()
            assert out[shift:shift + n] == host_text and out[:shift] == b"\xaa" * shift and out[shift + n:] == b"\xaa" * (96 - shift)
        size = C.c_uint64(0)
        assert lib.seeqdevScanInsertText(h, None, 0, None, 0, C.byref(size)) == 0 and size.value == n         # the size query
        # a text shorter than the one that was scanned: the records reach beyond it
        short = torch.empty(n, dtype=torch.uint8, device="cuda")
        C.set_errno(0)
        assert lib.seeqdevScanInsertText(h, C.c_void_p(t.data_ptr()), offsets[rows[-1][0]], C.c_void_p(short.data_ptr()), n, C.byref(size)) == -1
        assert C.get_errno() == errno.EIO
        # no staged text behind a resident call
        with pytest.raises(dev.SeeqDeviceError):
            sc.insert_text()
    for p in barcodes:
        p.close()
    sc.close()


def test_inserts_past_one_round_of_the_top_kernel(gpu, capi, oracle, pats):
    """More inserts than one round of k_insert_top takes (256 tiles: seeq_tiles.h), so that the 64-bit prefix of the text bytes is carried
    from round to round: the seeded lines of _lines (left flank, short gap, right flank), repeated; the expectation is Joined over the
    oracle's two scans of the same buffer.  Records, offsets, counts; the gathered text, whose last insert lies at text_bytes minus its
    own length only if every carry was right."""
    import torch
    from seeq_amd import device as dev
    with open(os.path.join(ROOT, "seeq_amd", "csrc", "seeq_tiles.h")) as f:
        shape = dict(re.findall(r"^#define\s+(SEEQ_TILE\w*)\s+(\d+)", f.read(), re.M))
    need = int(shape["SEEQ_TILE"]) * int(shape["SEEQ_TILE_WG"]) + int(shape["SEEQ_TILE"]) + 3
    window = (0, 0)
    base = _lines(PAIRS["short"], n=4000, seed=13, kinds=["LR"], gaps=[0, 1, 5, 12])
    per = len(Joined(oracle, PAIRS["short"], _buf(base), SQ_BEST).rows(window))
    buf = _buf(base * (need // per + 1))
    offsets = _line_offsets(buf)
    j = Joined(oracle, PAIRS["short"], buf, SQ_BEST)
    rows = j.rows(window)
    assert len(rows) >= need                                # left records with an admissible right record
    host_text = _host_text(buf, rows, offsets)
    last = rows[-1][2] - rows[-1][1] + 1
    left, right = pats["short"]
    t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    sc = dev.Scanner()

    def check(s, res):
        _check(s, res, j, window, offsets)
        assert res["text_bytes"] == len(host_text)
        text = s.insert_text(t).cpu().numpy().tobytes()
        assert len(text) == len(host_text) and text[len(text) - last:] == host_text[len(host_text) - last:]
        assert text == host_text
    _go(sc, "inserts past one round of the top kernel", lambda s: s.inserts_tensor(left, right, t, SQ_BEST, *window), check)
    sc.close()


@pytest.mark.parametrize("case", ["empty", "no_left", "no_right", "no_final_newline", "one_handle", "long_line"])
def test_inserts_edges(gpu, capi, oracle, pats, case):
    from seeq_amd import device as dev
    pair = PAIRS["pair20"]
    left, right = pats["pair20"]
    windows = [(0, 0), (10, 14)]
    if case == "empty":
        buf = b""
    elif case == "no_left":
        buf = _buf(_lines(pair, 1500, 51, kinds=["R", "RR", ""]))
    elif case == "no_right":
        buf = _buf(_lines(pair, 1500, 52, kinds=["L", "LL", ""]))
    elif case == "no_final_newline":
        lines = _lines(pair, 1500, 53)
        lines[-1] = "ACGT" + PAIRS["pair20"][0][0] + "ACGTACGTACGT" + PAIRS["pair20"][1][0] + "ACG"
        buf = _buf(lines)[:-1]
    elif case == "one_handle":
        pair = (PAIRS["pair20"][0], PAIRS["pair20"][0])
        right = left                                        # one handle: the insert between two occurrences of one flank
        buf = _buf(_lines(pair, 1500, 54, kinds=["LL", "LLL", "L", ""]))
    else:
        # one 200 kB line: a left plant followed by 2 000 right plants, among short reads -- a long walk behind a long-line scan
        rng = random.Random(55)
        plain_l, plain_r = dev.plain_pattern(pair[0][0]), dev.plain_pattern(pair[1][0])
        big = ["".join(rng.choice("ACGT") for _ in range(30)), plain_l]
        for _ in range(2000):
            big.append("".join(rng.choice("ACGT") for _ in range(rng.randrange(70, 90))))
            big.append(_mutate(rng, plain_r, rng.randint(0, pair[1][1])))
        lines = _lines(pair, 600, 56)
        lines.insert(300, "".join(big))
        assert 190000 < len(lines[300]) < 230000
        buf = _buf(lines)
        windows = [(0, 0), (100000, 0), (150000, 150100)]
    offsets = _line_offsets(buf)
    sc = dev.Scanner()
    for mode in (SQ_BEST, SQ_FIRST):
        j = Joined(oracle, pair, buf, mode)
        n00 = j.counts((0, 0))
        if case == "empty":
            assert n00 == dict.fromkeys(COUNTS, 0)
        elif case == "no_left":
            assert n00["nleft"] == 0 and n00["nright"] > 500
        elif case == "no_right":
            assert n00["nright"] == 0 and n00["nleft"] > 500
        elif case == "no_final_newline":
            assert mode != SQ_BEST or j.rows((10, 14))[-1] == (1500, 24, 36, 0, 0)
        elif case == "one_handle":
            assert n00["nleft"] == n00["nright"] == n00["nboth"] > 500 and 300 < n00["ninserts"] < n00["nboth"]
        else:
            assert len(j.right[301]) >= 1990 and any(l[0] == 301 for l in j.left)
            chosen = next(r for r in j.rows((0, 0)) if r[0] == 301)
            assert chosen[4] == 0 if mode == SQ_BEST else chosen[2] < 250       # SQ_BEST walks on to an exact copy, SQ_FIRST takes the first
        for window in windows:
            def check(s, res):
                _check(s, res, j, window, offsets)
                assert s.insert_text() == _host_text(buf, j.rows(window), offsets)
            _go(sc, "%s, mode %d, window %s" % (case, mode, window), lambda s: s.inserts_host(left, right, buf, mode, *window), check)
    sc.close()
