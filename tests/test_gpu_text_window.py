"""GPU (-m gpu): the entries behind the scan on a window of a larger buffer, and behind a scan that took several segments.  The rule: where
the text lies, what surrounds it and how it is cut into segments changes no answer.

One text (tests/text_window.py: Chain) -- 2 T + 3 FASTQ records whose sequence lines carry a guide between FA and FB and a UMI between FC and
FD, with the flaws the features' own modules plant -- and the plain lines derived from it go through every entry in four placements:
  a   the exact tensor, as everywhere else in the suite;
  b   a window at an odd lead between hostile guards (the FASTQ text: once per tail -- cut behind the last sequence line, behind its `+`
      line, inside its quality line);
  c   b under SEEQ_SEGMENT_BYTES=65536: seven segments of the FASTQ text, four of the plain lines, records across their seams;
  d   a window at a 16-aligned, not 128-aligned lead, the guard behind it beginning with one more whole line / record.
Every answer is compared, bit for bit, with the CPU oracle or with the Python restatement the feature's own module has, run over a COPY OF THE
WINDOW'S BYTES ALONE -- never with another GPU run.  tests/test_text_window_host.py shows on the CPU that the guards are live; the
`test_the_guards_are_live_*` tests show it on the device: the same entry given the window and the guard's bytes answers as the reference
over those bytes does, which is another answer.  One more test leaves the stale tail of a longer text behind the staged copy of a shorter
one."""
import numpy as np
import pytest

import text_window as W
from oracle.pyoracle import SQ_ALL, SQ_BEST, SQ_FIRST
from test_gpu_demux import _check as _same_demux
from test_gpu_demux import _expected as _demux_expected
from test_gpu_inserts import Joined, _host_text
from test_gpu_inserts import _check as _same_inserts
from test_gpu_kernel_instances import KNOBS
from test_gpu_qgate import _same as _same_gate
from test_gpu_strands import Expected as StrandsExpected
from test_gpu_strands import _check as _same_strands
from test_gpu_strands import _step
from test_gpu_tally import _same as _same_tally
from test_gpu_tally_collapse import NAMES as RULE_NAMES
from test_gpu_tally_collapse import _restated, _same_collapse
from test_gpu_tally_grouped import _held_of
from test_gpu_tally_grouped import _same as _same_grouped
from test_gpu_tally_library import _same as _same_library
from test_qgate_host import MISFIT, PASS, py_gate_all
from test_tally_library_host import PyLibrary

pytestmark = pytest.mark.gpu
TAU = W.FLANK_TAU
FLANKS = dict(A=W.FA, B=W.FB, C=W.FC, D=W.FD)
PAIRS = {"AB": ((W.FA, TAU), (W.FB, TAU)), "CD": ((W.FC, TAU), (W.FD, TAU))}
INSERT_CASES = [("AB", SQ_BEST, (0, 0)), ("AB", SQ_FIRST, (0, 0)), ("CD", SQ_BEST, (10, 14)), ("CD", SQ_FIRST, (10, 14))]
SEGMENT = "65536"

_FAULT = []


@pytest.fixture(autouse=True)
def _nothing_after_a_device_fault(monkeypatch):
    """A device fault ends the module: what comes after it fails here, before it starts anything on the device.  Every knob is unset before a
    test makes its contexts (they are read in seeqdevScanNew)."""
    if _FAULT:
        pytest.fail("a device fault earlier in this module (%s): nothing more is started on the device" % _FAULT[0])
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    yield


def _go(sc, what, call, check, fresh=None):
    """_step of test_gpu_strands.py; a device fault (it raises the SeeqDeviceError untouched) is remembered for the rest of the module."""
    from seeq_amd import device as dev
    try:
        _step(sc, what, call, check, fresh)
    except dev.SeeqDeviceError as e:
        _FAULT.append("%s: %s" % (what, e))
        raise


# ---- the text, its windows, the references over their bytes ----
class Ref:
    """The answers over one window's bytes, from the oracle and the restated rules, each made once."""

    def __init__(self, oracle, window, fastq):
        self.oracle, self.window, self.fastq, self.memo = oracle, window, fastq, {}
        self.seq, self.offs = W.fastq_seq(window) if fastq else (window, W.line_offsets(window))

    def _once(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    def scan(self, name, mode):
        return self._once(("scan", name, mode), lambda: self.oracle.buffer_scan(FLANKS[name], TAU, self.seq, mode))

    def joined(self, pair, mode):
        return self._once(("joined", pair, mode), lambda: Joined(self.oracle, PAIRS[pair], self.seq, mode))

    def strands(self, name, mode):
        return self._once(("strands", name, mode), lambda: StrandsExpected(self.oracle, FLANKS[name], TAU, self.seq, mode))

    def demux(self):
        return self._once("demux", lambda: _demux_expected(self.oracle, list(FLANKS.values()), [TAU] * 4, self.seq, SQ_BEST))

    def rows(self, pair, mode=SQ_BEST, window=(0, 0)):
        """the inserts of a flank pair: [(line, start, end, ldist, rdist)]"""
        return self._once(("rows", pair, mode, window), lambda: self.joined(pair, mode).rows(window))

    def spans(self, rows):
        """[(line, bytes)] of rows (line, start, end, ...)"""
        return [(r[0], self.window[self.offs[r[0]] + r[1]:self.offs[r[0]] + r[2]]) for r in rows]

    def hit_rows(self, name, mode=SQ_BEST):
        return [tuple(int(x) for x in r) for r in self.scan(name, mode)["records"]]

    def gate(self, rows, **kw):
        """(kinds, counts) of rows (line, start, end, ...) by the restated gate"""
        return py_gate_all(self.window, rows, [self.offs[r[0]] for r in rows], **kw)


class View:
    """A window and where it lies: lead None = a tensor of exactly its bytes; else place()d between `before` and `after`."""

    def __init__(self, name, window, fastq, lead=None, before=b"", after=b"", segments=False):
        self.name, self.window, self.fastq, self.lead, self.before, self.after, self.segments = name, window, fastq, lead, before, after, segments
        self._t = None

    def tensor(self):
        import torch
        if self._t is None:
            if self.lead is None:
                self._t = (torch.frombuffer(bytearray(self.window), dtype=torch.uint8).cuda(),) * 2
            else:
                big, lo, hi = W.place(self.window, self.lead, self.before, self.after)
                whole = torch.frombuffer(bytearray(big), dtype=torch.uint8).cuda()
                self._t = (whole, whole[lo:hi])
                assert self._t[1].data_ptr() % 128 == self.lead % 128
            torch.cuda.synchronize()
        assert self._t[1].numel() == len(self.window)
        return self._t[1]


class Setup:
    def __init__(self, oracle):
        self.oracle = oracle
        self.chain = W.Chain()

        def hits(buf):
            e = oracle.buffer_scan(W.FA, TAU, buf, SQ_ALL)
            return W.abs_hits(e["records"], W.line_offsets(buf))
        self.h = h = W.hostile_for(hits, W.FA)
        ch = self.chain
        self.views, self.refs = {}, {}
        fq = {tail: ch.fastq_window(tail) for tail in W.TAILS + ("whole",)}
        self.fq = fq
        add = self._add
        add(View("fastq-a", fq["whole"][0], True))
        for i, tail in enumerate(W.TAILS):
            add(View("fastq-b-" + tail, fq[tail][0], True, W.GUARD + (1, 65, 129)[i], ch.FASTQ_BEFORE, fq[tail][1]))
        add(View("fastq-c", fq["mid_qual"][0], True, W.GUARD + 13, ch.FASTQ_BEFORE, fq["mid_qual"][1], segments=True))
        add(View("fastq-d", fq["whole"][0], True, W.aligned_lead(2), ch.FASTQ_BEFORE, fq["whole"][1]))
        open_, closed = ch.plain_window(h, False), ch.plain_window(h, True)
        add(View("plain-a", closed, False))
        add(View("plain-b", open_, False, W.GUARD + 7, h.before, h.after_open))
        add(View("plain-c", open_, False, W.GUARD + 127, h.before, h.after_open, segments=True))
        add(View("plain-d", closed, False, W.aligned_lead(4), h.before, h.after_closed))
        # the guards are live: the window and the guard's bytes next to it as ONE text, in the same kind of tensor
        add(View("fastq-front", ch.FASTQ_BEFORE + fq["whole"][0], True, W.GUARD + 3))
        add(View("fastq-behind", fq["mid_qual"][0] + fq["mid_qual"][1], True, W.GUARD + 5))
        add(View("plain-around", h.before + open_ + h.after_open, False, W.GUARD + 9))

    def _add(self, view):
        self.views[view.name] = view

    def ref(self, view):
        key = (view.window, view.fastq)
        if key not in self.refs:
            self.refs[key] = Ref(self.oracle, view.window, view.fastq)
        return self.refs[key]


@pytest.fixture(scope="module")
def setup(oracle):
    return Setup(oracle)


@pytest.fixture(scope="module")
def pats(gpu):
    from seeq_amd import device as dev
    ps = {k: dev.Pattern(v, TAU) for k, v in FLANKS.items()}
    yield ps
    for p in ps.values():
        p.close()


FASTQ_VIEWS = ["fastq-a"] + ["fastq-b-" + t for t in W.TAILS] + ["fastq-c", "fastq-d"]
PLAIN_VIEWS = ["plain-a", "plain-b", "plain-c", "plain-d"]


def _scanner(view, monkeypatch):
    from seeq_amd import device as dev
    if view.segments:
        monkeypatch.setenv("SEEQ_SEGMENT_BYTES", SEGMENT)      # (read when the context is made)
    return dev.Scanner()


def _opt(view, mode):
    from seeq_amd import device as dev
    return mode | (dev.SEEQDEV_FASTQ if view.fastq else 0)


def _same_scan(s, res, exp, offs, records=True):
    assert res["nlines"] == exp["nlines"] and res["nmatchlines"] == exp["nmatchlines"], (res, exp["nlines"], exp["nmatchlines"])
    if records:
        n = len(exp["records"])
        assert res["nrecords"] == n
        assert np.array_equal(s.records(n).astype(np.uint64), exp["records"])
        assert s.record_offsets(n).tolist() == [offs[int(ln)] for ln in exp["records"][:, 0]]


# ---- the families ----
def _scans(sc, view, ref, pats, fresh=None):
    from seeq_amd import device as dev
    t = view.tensor()
    what = view.name
    for mode in (SQ_BEST, SQ_ALL):
        exp = ref.scan("A", mode)
        assert len(exp["records"]) > (50 if "front" not in what else -1)
        _go(sc, "%s: scan, mode %d" % (what, mode), lambda s: s.scan_tensor(pats["A"], t, _opt(view, mode), dev.WANT_RECORDS),
            lambda s, res: _same_scan(s, res, exp, ref.offs), fresh)
    exp = ref.scan("A", SQ_ALL)
    _go(sc, what + ": line count", lambda s: s.scan_tensor(pats["A"], t, _opt(view, SQ_FIRST), dev.WANT_COUNTLINES),
        lambda s, res: _same_scan(s, res, exp, ref.offs, records=False), fresh)
    if not view.fastq:                                      # (the multi-pattern entries refuse SEEQDEV_FASTQ)
        def multi(s, got):
            for name, g in zip(FLANKS, got):
                e = ref.scan(name, SQ_BEST)
                assert g["nlines"] == e["nlines"] and g["nmatchlines"] == e["nmatchlines"], name
                assert np.array_equal(g["records"].astype(np.uint64), e["records"]), name
        _go(sc, what + ": four patterns", lambda s: s.scan_tensor_multi(list(pats.values()), t, SQ_BEST, dev.WANT_RECORDS), multi, fresh)
    _go(sc, what + ": demux", lambda s: s.demux_tensor(list(pats.values()), t, _opt(view, SQ_BEST)), lambda s, res: _same_demux(res, ref.demux()), fresh)
    for mode in (SQ_ALL, SQ_BEST):
        _go(sc, "%s: both strands, mode %d" % (what, mode), lambda s: s.strands_tensor(pats["A"], t, _opt(view, mode), dev.WANT_RECORDS),
            lambda s, res: _same_strands(s, res, ref.strands("A", mode), ref.offs), fresh)


def _inserts(sc, view, ref, pats, fresh=None):
    t = view.tensor()
    for pair, mode, window in INSERT_CASES:
        rows = ref.rows(pair, mode, window)

        def check(s, res):
            _same_inserts(s, res, ref.joined(pair, mode), window, ref.offs)
            assert s.insert_text(t).cpu().numpy().tobytes() == _host_text(view.window, rows, ref.offs)
        _go(sc, "%s: inserts %s, mode %d, window %s" % (view.name, pair, mode, window),
            lambda s: s.inserts_tensor(pats[pair[0]], pats[pair[1]], t, _opt(view, mode), *window), check, fresh)


def _cut(s, view, ref, pats, pair):
    """the inserts call of a pair (SQ_BEST, no window), its records held against the joined oracle scans -> the rows"""
    rows = ref.rows(pair)
    res = s.inserts_tensor(pats[pair[0]], pats[pair[1]], view.tensor(), _opt(view, SQ_BEST), copy=False)
    assert res["ninserts"] == len(rows), (pair, res)
    rec = s.insert_records(len(rows))
    assert list(zip(rec["line"].tolist(), rec["start"].tolist(), rec["end"].tolist())) == [r[:3] for r in rows], pair
    assert s.insert_offsets(len(rows)).tolist() == [ref.offs[r[0]] for r in rows]
    return rows


def _tallies(sc, view, ref, pats, fresh=None):
    """tally from inserts and from hits; hold + grouped; the collapse under both rules"""
    from seeq_amd import device as dev
    t = view.tensor()
    guides, umis = ref.spans(ref.rows("AB")), ref.spans(ref.rows("CD"))
    assert len(guides) > (W.tile() if "front" not in view.name else -1)

    def from_inserts(s):
        _cut(s, view, ref, pats, "AB")
        return s.tally(t)
    _go(sc, view.name + ": tally of inserts", from_inserts, lambda s, res: _same_tally(res, [b for _, b in guides]), fresh)
    hits = ref.spans([(r[0], r[1], r[2]) for r in ref.hit_rows("A")])

    def from_hits(s):
        res = s.scan_tensor(pats["A"], t, _opt(view, SQ_BEST), dev.WANT_RECORDS)
        _same_scan(s, res, ref.scan("A", SQ_BEST), ref.offs)
        return s.tally(t, source="hits")
    _go(sc, view.name + ": tally of hits", from_hits, lambda s, res: _same_tally(res, [b for _, b in hits]), fresh)
    held, hcnt = _held_of(guides)

    def grouped(s):
        _cut(s, view, ref, pats, "AB")
        hold = s.tally_hold(t)
        _cut(s, view, ref, pats, "CD")
        res = s.tally_grouped(t)
        return hold, res, {rule: s.tally_collapse(RULE_NAMES[rule]) for rule in RULE_NAMES}

    def check(s, got):
        hold, res, col = got
        assert hold == hcnt
        pairs, groups = _same_grouped(res, held, umis)
        exp = ref._once("collapse", lambda: _restated(pairs))
        for rule in RULE_NAMES:
            _same_collapse(col[rule], pairs, groups, exp, rule, res["max_len"])
    _go(sc, view.name + ": hold, grouped, collapse", grouped, check, fresh)


def _library(sc, view, ref, pats, chain, fresh=None):
    t = view.tensor()
    lib = PyLibrary(chain.guides)
    guides, umis = ref.spans(ref.rows("AB")), ref.spans(ref.rows("CD"))
    sc.set_library(lib.seqs, 1)

    def counted(s):
        _cut(s, view, ref, pats, "AB")
        return s.tally_library(t)

    def check(s, res):
        cnt = _same_library(res, lib, [b for _, b in guides], 1)
        assert "front" in view.name or (cnt["ncorrected"] > 20 and cnt["nunknown"] > 5)
    _go(sc, view.name + ": library tally", counted, check, fresh)

    def held(s):
        _cut(s, view, ref, pats, "AB")
        hold = s.tally_hold_library(t)
        _cut(s, view, ref, pats, "CD")
        return hold, s.tally_grouped(t)

    def check_held(s, got):
        hold, res = got
        cnt, _, ids = lib.tally([b for _, b in guides], 1)
        assert {k: hold[k] for k in cnt if k != "ndistinct"} == {k: v for k, v in cnt.items() if k != "ndistinct"}
        _same_grouped(res, [(ln, i) for (ln, _), i in zip(guides, ids)], umis)
    _go(sc, view.name + ": library hold, grouped", held, check_held, fresh)


def _gate(sc, view, ref, pats, fresh=None):
    """quality_gate from both sources, then tally and grouped tally over the gated spans"""
    from seeq_amd import device as dev
    t = view.tensor()
    grows, urows = ref.rows("AB"), ref.rows("CD")
    gkinds, gcnt = ref.gate(grows)
    ukinds, ucnt = ref.gate(urows)
    gspans = [sp for sp, k in zip(ref.spans(grows), gkinds) if k == PASS]
    uspans = [sp for sp, k in zip(ref.spans(urows), ukinds) if k == PASS]
    got = {}

    def inserts(s):
        _cut(s, view, ref, pats, "AB")
        src = s.insert_records(len(grows)).view(np.uint32).reshape(-1, 4), s.insert_offsets(len(grows))
        g = s.quality_gate(t)
        return g, src, s.tally(t, source="gated")

    def check(s, tr):
        g, src, tl = tr
        _same_gate(g, gkinds, gcnt, *src)
        _same_tally(tl, [b for _, b in gspans])
        got["kinds"] = g["kinds"].tolist()
    _go(sc, view.name + ": gate of inserts, tally of the gated", inserts, check, fresh)
    hrows = ref.hit_rows("B")
    hkinds, hcnt = ref.gate(hrows)

    def hits(s):
        res = s.scan_tensor(pats["B"], t, _opt(view, SQ_BEST), dev.WANT_RECORDS)
        _same_scan(s, res, ref.scan("B", SQ_BEST), ref.offs)
        rec, off = s.records(len(hrows)), s.record_offsets(len(hrows))
        return s.quality_gate(t, source="hits"), rec, off
    _go(sc, view.name + ": gate of hits", hits, lambda s, tr: _same_gate(tr[0], hkinds, hcnt, tr[1], tr[2]), fresh)
    held, hold_cnt = _held_of(gspans)

    def grouped(s):
        _cut(s, view, ref, pats, "AB")
        g = s.quality_gate(t, copy=False)
        hold = s.tally_hold(t, source="gated")
        _cut(s, view, ref, pats, "CD")
        u = s.quality_gate(t, copy=False)
        return g, hold, u, s.tally_grouped(t, source="gated")

    def check_grouped(s, tr):
        g, hold, u, res = tr
        assert g["npassed"] == len(gspans) and u["npassed"] == len(uspans) and hold == hold_cnt
        _same_grouped(res, held, uspans)
    _go(sc, view.name + ": hold gated, members gated", grouped, check_grouped, fresh)
    return gkinds, ukinds


# ---- every entry in every placement ----
@pytest.mark.parametrize("name", FASTQ_VIEWS + PLAIN_VIEWS)
def test_scans(gpu, capi, setup, pats, name, monkeypatch):
    view = setup.views[name]
    sc = _scanner(view, monkeypatch)
    _scans(sc, view, setup.ref(view), pats)
    sc.close()


@pytest.mark.parametrize("name", FASTQ_VIEWS + PLAIN_VIEWS)
def test_inserts_and_their_text(gpu, capi, setup, pats, name, monkeypatch):
    view = setup.views[name]
    sc = _scanner(view, monkeypatch)
    _inserts(sc, view, setup.ref(view), pats)
    sc.close()


@pytest.mark.parametrize("name", FASTQ_VIEWS + PLAIN_VIEWS)
def test_tallies(gpu, capi, setup, pats, name, monkeypatch):
    view = setup.views[name]
    sc = _scanner(view, monkeypatch)
    _tallies(sc, view, setup.ref(view), pats)
    sc.close()


@pytest.mark.parametrize("name", FASTQ_VIEWS + PLAIN_VIEWS)
def test_library(gpu, capi, setup, pats, name, monkeypatch):
    view = setup.views[name]
    sc = _scanner(view, monkeypatch)
    _library(sc, view, setup.ref(view), pats, setup.chain)
    sc.close()


@pytest.mark.parametrize("name", FASTQ_VIEWS)
def test_quality_gate(gpu, capi, setup, pats, name, monkeypatch):
    """In the three tails the last record's guide and UMI are MISFIT: their quality line is cut, or missing, where the window ends -- and
    goes on, with high bytes, in the guard."""
    view = setup.views[name]
    sc = _scanner(view, monkeypatch)
    gkinds, ukinds = _gate(sc, view, setup.ref(view), pats)
    cut = name not in ("fastq-a", "fastq-d")
    assert gkinds[-1] == ukinds[-1] == (MISFIT if cut else PASS)
    sc.close()


class PackedCase:
    """pack_reads_device + run_packed: fixed-length reads as a window at an odd lead, the guards holding reads with occurrences.  `t`: the
    window on the device, `pb` / `pn`: room for its packed bases and N mask, zeroed; `exp`: the ASCII oracle over the window."""

    def __init__(self, oracle):
        import torch
        from seeq_amd import device as dev
        self.expr, self.tau, self.L, self.n = expr, tau, L, n = "GATGTAGCGCGATTAGCCTG", 3, 150, 2051
        self.window = window = bytes(oracle.synth_reads(0, n, L, expr, tau))
        read = (b"ACGT" * 40)[:L - 20] + expr.encode() + b"\n"
        assert len(read) == L + 1 and len(window) == n * (L + 1)
        big, lo, hi = W.place(window, W.GUARD + 11, read * 3, read * 3)
        self.exp = exp = oracle.buffer_scan(expr, tau, window, SQ_BEST)
        ext = oracle.buffer_scan(expr, tau, read * 3 + window + read * 3, SQ_BEST)
        assert ext["nmatchlines"] == exp["nmatchlines"] + 6 and len(exp["records"]) > 50
        self.t = torch.frombuffer(bytearray(big), dtype=torch.uint8).cuda()[lo:hi]
        self.pb = torch.zeros(n * ((L + 3) // 4), dtype=torch.uint8, device="cuda")
        self.pn = torch.zeros(n * ((L + 7) // 8), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.pat = dev.Pattern(expr, tau)

    def pack(self, stream=None):
        from seeq_amd import device as dev
        dev.pack_reads_device(self.t.data_ptr(), self.n, self.L, self.pb.data_ptr(), self.pn.data_ptr(), stream=stream)

    def packed_as_on_the_host(self):
        from seeq_amd import device as dev
        hb, hn, hcount = dev.pack_reads(self.window, self.L)
        assert hcount == self.n and self.pb.cpu().numpy().tobytes() == hb.tobytes() and self.pn.cpu().numpy().tobytes() == hn.tobytes()

    def scan(self, s):
        from seeq_amd import device as dev
        s.run_packed(self.pat, self.pb.data_ptr(), self.pn.data_ptr(), self.n, self.L, options=SQ_BEST, want=dev.WANT_RECORDS)

    def same(self, s, res, exp=None):
        exp = exp or self.exp
        assert res["nlines"] == self.n and res["nmatchlines"] == exp["nmatchlines"] and res["nrecords"] == len(exp["records"])
        assert np.array_equal(s.records(res["nrecords"]).astype(np.uint64), exp["records"])

    def close(self):
        self.pat.close()


def _packed_reads(case, scanner, stream=None, late=None):
    """scanner(): the context; stream: the hipStream_t (int) the packing runs on (None: the null stream).  late(case), when given
    (tests/late_text.py), is called in front of the packing: it makes the window AND the packed arrays late on the stream -- the packing
    and the packed scan then follow each other with no host wait between them, and the packed arrays are held against the host's
    behind the fetch."""
    import torch
    sc = scanner()

    def call(s):
        if late is not None:
            late(s, case)
        case.pack(stream)
        if late is None:
            torch.cuda.synchronize()
            case.packed_as_on_the_host()
        case.scan(s)
        res = s.fetch()
        if late is not None:
            torch.cuda.synchronize()
            case.packed_as_on_the_host()
        return res
    _go(sc, "packed reads at an odd lead", call, case.same, scanner)
    sc.close()


def test_packed_reads_between_guards(gpu, capi, oracle, monkeypatch):
    from seeq_amd import device as dev
    case = PackedCase(oracle)
    _packed_reads(case, dev.Scanner)
    case.close()


# ---- the guards are live: the same entries over window + guard bytes give the reference's answer over THOSE bytes, another one ----
def _differs(a, b):
    assert a != b, "the guard's bytes change nothing in the reference: the placement proves nothing"


def test_the_guards_are_live_for_the_scans(gpu, capi, setup, pats, monkeypatch):
    for ext, alone in (("plain-around", "plain-b"), ("fastq-front", "fastq-a")):
        view = setup.views[ext]
        sc = _scanner(view, monkeypatch)
        _scans(sc, view, setup.ref(view), pats)
        sc.close()
        a, b = setup.ref(setup.views[alone]), setup.ref(view)
        _differs((a.scan("A", SQ_BEST)["nlines"], a.scan("A", SQ_BEST)["nmatchlines"]), (b.scan("A", SQ_BEST)["nlines"], b.scan("A", SQ_BEST)["nmatchlines"]))
        _differs(a.demux()[1], b.demux()[1])
        _differs(a.strands("A", SQ_ALL).per_strand, b.strands("A", SQ_ALL).per_strand)


def test_the_guards_are_live_for_the_inserts(gpu, capi, setup, pats, monkeypatch):
    view = setup.views["plain-around"]
    sc = _scanner(view, monkeypatch)
    _inserts(sc, view, setup.ref(view), pats)
    sc.close()
    a, b = setup.ref(setup.views["plain-b"]), setup.ref(view)
    # the first line: FA's first half ends the guard, its second half, a guide and FB begin the window -- an insert only with the guard
    assert b.rows("AB")[0][:3] == (2, 20, 40) and len(b.rows("AB")) == len(a.rows("AB")) + 1
    _differs(a.joined("AB", SQ_BEST).counts((0, 0)), b.joined("AB", SQ_BEST).counts((0, 0)))


def test_the_guards_are_live_for_the_tallies(gpu, capi, setup, pats, monkeypatch):
    view = setup.views["plain-around"]
    sc = _scanner(view, monkeypatch)
    _tallies(sc, view, setup.ref(view), pats)
    sc.close()
    a, b = setup.ref(setup.views["plain-b"]), setup.ref(view)
    _differs(len(a.spans(a.rows("AB"))), len(b.spans(b.rows("AB"))))
    _differs(len(a.hit_rows("A")), len(b.hit_rows("A")))


def test_the_guards_are_live_for_the_library(gpu, capi, setup, pats, monkeypatch):
    view = setup.views["plain-around"]
    sc = _scanner(view, monkeypatch)
    _library(sc, view, setup.ref(view), pats, setup.chain)
    sc.close()
    lib = PyLibrary(setup.chain.guides)
    a, b = setup.ref(setup.views["plain-b"]), setup.ref(view)
    _differs(lib.tally([s for _, s in a.spans(a.rows("AB"))], 1)[0], lib.tally([s for _, s in b.spans(b.rows("AB"))], 1)[0])


def test_the_guards_are_live_for_the_quality_gate(gpu, capi, setup, pats, monkeypatch):
    view = setup.views["fastq-behind"]
    sc = _scanner(view, monkeypatch)
    gkinds, ukinds = _gate(sc, view, setup.ref(view), pats)
    sc.close()
    a = setup.ref(setup.views["fastq-b-mid_qual"])
    n = len(setup.chain.records)
    rows = [r for r in setup.ref(view).rows("AB") if r[0] <= n]
    assert rows == a.rows("AB") and a.gate(rows)[0][-1] == MISFIT and gkinds[len(rows) - 1] == PASS
    _differs(a.gate(rows)[0], gkinds[:len(rows)])


# ---- the stale tail of a longer text behind the staged copy of a shorter one ----
def test_the_stale_tail_of_an_earlier_staged_text(gpu, capi, setup, pats):
    """A host entry stages its text in the context's buffer, which is not cleared: behind a text shorter than the one before it lies the
    longer one's tail.  window + guard first, then the window: every second answer is the reference over the window alone."""
    from seeq_amd import device as dev
    plain, fq = setup.views["plain-b"], setup.views["fastq-b-mid_qual"]
    pref, fref = setup.ref(plain), setup.ref(fq)
    longer = plain.window + plain.after
    sc = dev.Scanner()
    exp = pref.scan("A", SQ_BEST)

    def scan(s):
        first = s.scan_host(pats["A"], longer, SQ_BEST, dev.WANT_RECORDS)
        assert first["nmatchlines"] == exp["nmatchlines"] + 2
        return s.scan_host(pats["A"], plain.window, SQ_BEST, dev.WANT_RECORDS)
    _go(sc, "scan_host", scan, lambda s, res: _same_scan(s, res, exp, pref.offs))

    def strands(s):
        s.strands_host(pats["A"], longer, SQ_ALL)
        return s.strands_host(pats["A"], plain.window, SQ_ALL)
    _go(sc, "strands_host", strands, lambda s, res: _same_strands(s, res, pref.strands("A", SQ_ALL), pref.offs))

    def demux(s):
        s.demux_host(list(pats.values()), longer, SQ_BEST)
        return s.demux_host(list(pats.values()), plain.window, SQ_BEST)
    _go(sc, "demux_host", demux, lambda s, res: _same_demux(res, pref.demux()))
    rows = fref.rows("AB")
    kinds, cnt = fref.gate(rows)
    assert kinds[-1] == MISFIT
    opt = SQ_BEST | dev.SEEQDEV_FASTQ

    def inserts(s):
        first = s.inserts_host(pats["A"], pats["B"], fq.window + fq.after, opt)
        assert first["ninserts"] == len(rows) + 1
        res = s.inserts_host(pats["A"], pats["B"], fq.window, opt)
        src = s.insert_records(len(rows)).view(np.uint32).reshape(-1, 4), s.insert_offsets(len(rows))
        return res, s.tally(None), s.insert_text(None), s.quality_gate(None), src

    def check(s, tr):
        res, tl, text, g, src = tr
        _same_inserts(s, res, fref.joined("AB", SQ_BEST), (0, 0), fref.offs)
        _same_tally(tl, [b for _, b in fref.spans(rows)])
        assert text == _host_text(fq.window, rows, fref.offs)
        _same_gate(g, kinds, cnt, *src)
    _go(sc, "inserts_host, then the staged text", inserts, check)
    sc.close()
