"""GPU (-m gpu): every device entry on a caller's NON-BLOCKING stream, the text arriving late on it.  The rule: an entry is ordered behind
everything queued on its context's stream at the time of the call -- its launches, copies and memsets, the tables it builds on first use,
the EQ tables it uploads when the options change, its workspace when it grows.

Everywhere else in the suite a context's stream is of the default kind and the text came over the null stream: the null stream's implicit
barrier orders the two whatever the context does.  Here the contexts sit on torch side streams (tests/late_text.py: LateScanner), and before
every entry that reads device text the text is overwritten with a decoy and put back behind a device-side delay D, all on that stream and
with the producer still pending when the entry gets control.  Each family of tests/test_gpu_text_window.py runs TWICE on one such context
-- cold: first-use builds, workspace growth and the line-length sample under a pending producer; warm: cached tables and sample, launches
that go out with no host wait while the text is still the decoy -- over the placed views `b` (odd leads, hostile guards) and `c` (the same
in 64 KiB segments).  Every answer is the reference over the TRUE window's bytes, bit for bit, as in that module; tests/test_late_text_host.py
shows on the CPU that the decoy's answers are other ones, `test_an_unordered_context_sees_the_decoy` shows it on the device: a context on
ANOTHER non-blocking stream, ordered behind nothing on the first, answers as the reference over the decoy does.

D is twice the wall time of the slowest warm call of an unarmed context on the same view, and at least 5 ms (late_text.MIN_DELAY_MS); the
delay kernel is one spinning thread (torch.cuda._sleep), calibrated once per module.  torch.cuda.synchronize() happens only AFTER an entry
has returned."""
import contextlib

import numpy as np
import pytest

import late_text as L
import test_gpu_text_window as TW
import text_window as W
from oracle.pyoracle import SQ_ALL, SQ_BEST, SQ_FIRST
from test_gpu_demux import _check as _same_demux
from test_gpu_inserts import _check as _same_inserts
from test_gpu_inserts import _host_text
from test_gpu_strands import _check as _same_strands
from test_gpu_tally import _same as _same_tally
from test_gpu_text_window import FLANKS, SEGMENT, Ref, _cut, _gate, _go, _inserts, _library, _opt, _same_scan, _scans, _tallies
from test_gpu_text_window import _nothing_after_a_device_fault, pats, setup      # noqa: F401  (fixtures: the fault rule is this module's too)
from test_qgate_host import MISFIT

pytestmark = pytest.mark.gpu
PLAIN_VIEWS = ["plain-b", "plain-c"]
FASTQ_VIEWS = ["fastq-b-" + W.TAILS[0], "fastq-c"]
VIEWS = PLAIN_VIEWS + FASTQ_VIEWS
FAMILIES = ("scans", "inserts", "tallies", "library", "gate")


def _family(which, sc, view, ref, pats, chain, fresh):
    if which == "scans":
        return _scans(sc, view, ref, pats, fresh=fresh)
    if which == "inserts":
        return _inserts(sc, view, ref, pats, fresh=fresh)
    if which == "tallies":
        return _tallies(sc, view, ref, pats, fresh=fresh)
    if which == "library":
        return _library(sc, view, ref, pats, chain, fresh=fresh)
    assert which == "gate" and view.fastq
    return _gate(sc, view, ref, pats, fresh=fresh)


def _avg_line(view):
    return len(view.window) / max(1, view.window.count(b"\n"))


class Late:
    """What the module shares: two side streams, the calibrated delay, D per view, the arms counted."""

    def __init__(self, setup):
        import torch
        self.setup = setup
        self.side, self.other = torch.cuda.Stream(), torch.cuda.Stream()
        self.delay = L.Delay()
        self.ms, self.arms, self.decoys = {}, 0, {}

    def delay_ms(self, view, pats, monkeypatch):
        """D of a view: every family twice on an UNARMED context of the view's kind; twice the slowest call of the second, warm pass"""
        import torch
        if view.name not in self.ms:
            sc = self._make(view, monkeypatch, 0, False, None)
            ref = self.setup.ref(view)
            for _ in ("cold", "warm"):
                sc.slowest_ms = 0.0
                for which in FAMILIES[:4 + view.fastq]:
                    _family(which, sc, view, ref, pats, self.setup.chain, lambda: self._make(view, monkeypatch, 0, False, None))
            torch.cuda.synchronize()
            sc.close()
            assert sc.slowest_ms > 0
            self.ms[view.name] = max(L.MIN_DELAY_MS, 2.0 * sc.slowest_ms)
            print("late text: %s: slowest unarmed warm call %.3f ms, D = %.3f ms (%.0f cycles per ms)"
                  % (view.name, sc.slowest_ms, self.ms[view.name], self.delay.cycles_per_ms))
        return self.ms[view.name]

    def _make(self, view, monkeypatch, cycles, armed, side, hinted=False):
        if view.segments:
            monkeypatch.setenv("SEEQ_SEGMENT_BYTES", SEGMENT)      # (read when the context is made)
        sc = L.LateScanner(side or self.side, cycles, armed)
        sc.give(view.tensor(), view.window)
        if hinted:
            sc.set_line_hint(_avg_line(view))
        return sc

    def scanner(self, view, pats, monkeypatch, side=None, hinted=False):
        """-> a factory of armed LateScanners of the view (the same environment, the same stream, the same text)"""
        cycles = self.delay.cycles(self.delay_ms(view, pats, monkeypatch))
        return lambda: self._make(view, monkeypatch, cycles, True, side, hinted)

    @contextlib.contextmanager
    def closing(self, *scs):
        """the end of a test's contexts, whether it passed or not: nothing left pending on the streams, the arms counted, the contexts
        closed (after a device fault the wait raises; the contexts are closed all the same)"""
        import torch
        try:
            yield
        finally:
            try:
                torch.cuda.synchronize()
            finally:
                for sc in scs:
                    self.arms += sc.arms
                    sc.close()

    def decoy_ref(self, view):
        key = (view.window, view.fastq)
        if key not in self.decoys:
            self.decoys[key] = Ref(self.setup.oracle, L.decoy(view.window), view.fastq)
        return self.decoys[key]


@pytest.fixture(scope="module")
def late(gpu, setup):
    """Every arm asserted `not side.query()` where it was made; what is printed when the module is done is their count and D per view."""
    state = Late(setup)
    yield state
    print("late text: %d arms, each pending when its entry got control; %.0f cycles per ms; D per view (ms): %s"
          % (state.arms, state.delay.cycles_per_ms, {k: round(v, 3) for k, v in state.ms.items()}))


@contextlib.contextmanager
def _a_fault_ends_the_module(what):
    """for the steps that are not one call on one context (test_gpu_text_window.py: _go)"""
    from seeq_amd import device as dev
    try:
        yield
    except dev.SeeqDeviceError as e:
        text = str(e).lower()
        if "illegal" in text or "launch failure" in text or "hardware" in text:
            TW._FAULT.append("%s: %s" % (what, e))
        raise


def _twice(which, setup, pats, late, name, monkeypatch):
    view = setup.views[name]
    make = late.scanner(view, pats, monkeypatch)
    sc = make()
    out = None
    with late.closing(sc):
        for _ in ("cold", "warm"):
            before = sc.arms
            out = _family(which, sc, view, setup.ref(view), pats, setup.chain, make)
            assert sc.arms > before
    return out


# ---- the side streams are what a PyTorch caller passes ----
def test_the_side_streams_are_non_blocking(gpu, capi, late):
    for s in (late.side, late.other):
        assert s.cuda_stream != 0
        flags = L.stream_flags(s)
        print("late text: hipStreamGetFlags(%#x) = %s" % (s.cuda_stream, flags))
        if flags is not None:
            assert flags & L.HIP_STREAM_NON_BLOCKING, "torch.cuda.Stream() is not a non-blocking stream here (flags %#x)" % flags
    assert late.side.cuda_stream != late.other.cuda_stream


def test_every_method_that_reads_device_text_is_armed():
    """dev.Scanner's public methods with a parameter named t, d_ptr or bases_ptr: each is armed by LateScanner, or exempt with a reason"""
    from seeq_amd import device as dev
    found = L.text_methods()
    assert found, "no method of Scanner takes device text: the walk is broken"
    for name in found:
        if name in L.EXEMPT:
            assert L.EXEMPT[name].strip(), name
            continue
        assert name in L.ARMED, "Scanner.%s reads device text (%s) and LateScanner does not arm it" % (name, found[name])
        assert getattr(L.LateScanner, name) is not getattr(dev.Scanner, name), name
    assert set(L.ARMED) <= set(found), "armed, but no reader of device text: %s" % sorted(set(L.ARMED) - set(found))
    assert not set(L.EXEMPT) & set(L.ARMED)


# ---- the families, cold then warm, the text late before every entry ----
@pytest.mark.parametrize("name", VIEWS)
def test_scans(gpu, capi, setup, pats, late, name, monkeypatch):
    _twice("scans", setup, pats, late, name, monkeypatch)


@pytest.mark.parametrize("name", VIEWS)
def test_inserts_and_their_text(gpu, capi, setup, pats, late, name, monkeypatch):
    _twice("inserts", setup, pats, late, name, monkeypatch)


@pytest.mark.parametrize("name", VIEWS)
def test_tallies(gpu, capi, setup, pats, late, name, monkeypatch):
    _twice("tallies", setup, pats, late, name, monkeypatch)


@pytest.mark.parametrize("name", VIEWS)
def test_library(gpu, capi, setup, pats, late, name, monkeypatch):
    _twice("library", setup, pats, late, name, monkeypatch)


@pytest.mark.parametrize("name", FASTQ_VIEWS)
def test_quality_gate(gpu, capi, setup, pats, late, name, monkeypatch):
    """Both views end inside their last record: its guide and UMI are MISFIT (test_gpu_text_window.py: test_quality_gate)."""
    gkinds, ukinds = _twice("gate", setup, pats, late, name, monkeypatch)
    assert gkinds[-1] == ukinds[-1] == MISFIT


# ---- a hinted context: no sample, no synchronisation in front of the launches ----
@pytest.mark.parametrize("name", ["plain-b", FASTQ_VIEWS[0]])
def test_hinted_scans_launch_under_the_pending_text(gpu, capi, setup, pats, late, name, monkeypatch):
    """set_line_hint on a fresh context: scan_setup takes no sample.  SQ_BEST / SQ_ALL with records, the line count; the same scan twice
    in a row (the second has its EQ tables: its launches are out, and run() is back, while the producer is still pending); the
    four-pattern multi under two option sets in turn (its EQ tables are uploaded whenever the options change)."""
    from seeq_amd import device as dev
    view, ref = setup.views[name], setup.ref(setup.views[name])
    t = view.tensor()
    make = late.scanner(view, pats, monkeypatch, hinted=True)
    sc = make()
    with late.closing(sc):
        for mode in (SQ_BEST, SQ_ALL):
            exp = ref.scan("A", mode)
            _go(sc, "%s, hinted: scan, mode %d" % (name, mode), lambda s: s.scan_tensor(pats["A"], t, _opt(view, mode), dev.WANT_RECORDS),
                lambda s, res: _same_scan(s, res, exp, ref.offs), make)
        _go(sc, name + ", hinted: line count", lambda s: s.scan_tensor(pats["A"], t, _opt(view, SQ_FIRST), dev.WANT_COUNTLINES),
            lambda s, res: _same_scan(s, res, ref.scan("A", SQ_ALL), ref.offs, records=False), make)

        def again(s):
            s.scan_tensor(pats["A"], t, _opt(view, SQ_BEST), dev.WANT_RECORDS)
            s.run(pats["A"], t.data_ptr(), t.numel(), _opt(view, SQ_BEST), dev.WANT_RECORDS)
            early = not s.side.query()
            return early, s.fetch()

        def check_again(s, got):
            early, res = got
            assert early, "run() of a warm, hinted context came back after the text's producer had finished: it waited on the host, or D is too short"
            _same_scan(s, res, ref.scan("A", SQ_BEST), ref.offs)
        _go(sc, name + ", hinted: the same scan again", again, check_again, make)
        if not view.fastq:                                      # (the multi-pattern entries refuse SEEQDEV_FASTQ)
            # the four flanks at distance 1 have a union automaton: ONE walk, whose EQ tables go up whenever the options differ from the last call's
            for mode in (SQ_BEST, SQ_ALL, SQ_BEST, SQ_ALL):
                exp = [ref.scan(flank, mode) for flank in FLANKS]
                assert sum(len(e["records"]) for e in exp) > 200

                def multi(s, got):
                    assert s.last_multi_one_pass(), "a scan per pattern: the one-walk multi and its EQ-table upload did not run"
                    for flank, g, e in zip(FLANKS, got, exp):
                        assert g["nlines"] == e["nlines"] and g["nmatchlines"] == e["nmatchlines"], flank
                        assert np.array_equal(g["records"].astype(np.uint64), e["records"]), flank
                _go(sc, "%s, hinted: four patterns, mode %d" % (name, mode), lambda s: s.scan_tensor_multi(list(pats.values()), t, mode, dev.WANT_RECORDS),
                    multi, make)
        assert sc.arms >= 5


def test_packed_reads_on_the_callers_stream(gpu, capi, oracle, setup, pats, late, monkeypatch):
    """The packing and the packed scan on the side stream with NO host wait between them.  The packing reads the late text; the packed
    scan reads the packed arrays, which are late themselves (late_text.LatePacked: cleared, the text armed, packed again, all on the
    stream): zeros -- reads of A alone -- until the delay is over.  Then the liveness proof for this entry: a context on the second
    stream, ordered behind nothing, is back while the producer is pending and answers for the zeros.  D: that of plain-b, whose text is
    the larger one (the reads are 0.3 MB)."""
    import torch
    from seeq_amd import device as dev
    cycles = late.delay.cycles(late.delay_ms(setup.views["plain-b"], pats, monkeypatch))
    case = TW.PackedCase(oracle)
    side = late.side
    made = []

    def scanner():
        made.append(L.LateScanner(side, cycles))
        return made[-1]

    def make_late(s, case):
        s.give_packed(case.t, case.window, case.pb, case.pn, lambda: case.pack(side.cuda_stream)).clear()
        s.arm(case.t)
    # what the zeros are: reads of A alone, by the host's packing; the oracle's answer over them is another one
    blank = (b"A" * case.L + b"\n") * case.n
    hb, hn, hcount = dev.pack_reads(blank, case.L)
    assert hcount == case.n and not hb.any() and not hn.any() and len(hb) == case.pb.numel() and len(hn) == case.pn.numel()
    exp0 = oracle.buffer_scan(case.expr, case.tau, blank, SQ_BEST)
    assert exp0["nmatchlines"] != case.exp["nmatchlines"] and len(exp0["records"]) != len(case.exp["records"])
    u = dev.Scanner(late.other.cuda_stream)
    try:
        TW._packed_reads(case, scanner, side.cuda_stream, make_late)
        torch.cuda.synchronize()
        assert made[0].arms >= 2                            # (in front of the packing, in front of run_packed)
        with _a_fault_ends_the_module("packed reads: an unordered context"):
            case.scan(u)                                    # warm, on the packed arrays as they are now, nothing pending
            case.same(u, u.fetch())
            torch.cuda.synchronize()
            packed = L.LatePacked(L.LateText(case.t, case.window, side), case.pb, case.pn, lambda: case.pack(side.cuda_stream))
            packed.put_zeros()
            packed.arm(cycles)
            packed.text.pending()
            case.scan(u)
            res = u.fetch()
            early = not side.query()
            side.synchronize()                              # (the entry has returned; the arrays are packed again)
            assert early, "an unordered packed scan outlasted the producer: D is too short"
            case.same(u, res, exp0)
            case.packed_as_on_the_host()
            case.scan(u)                                    # and ordered again, it answers for the reads
            case.same(u, u.fetch())
    finally:
        try:
            torch.cuda.synchronize()
        finally:
            late.arms += sum(sc.arms for sc in made)
            u.close()
            case.close()


def test_host_entries_behind_pending_work(gpu, capi, setup, pats, late, monkeypatch):
    """The entries that stage a host text, a bare delay pending on the stream in front of each; tally() of the staged text."""
    from seeq_amd import device as dev
    plain, fq = setup.views["plain-b"], setup.views[FASTQ_VIEWS[0]]
    pref, fref = setup.ref(plain), setup.ref(fq)
    cycles = late.delay.cycles(late.delay_ms(plain, pats, monkeypatch))

    def make():
        return L.LateScanner(late.side, cycles)
    sc = make()
    with late.closing(sc):
        def behind(call):
            def go(s):
                s.bare()
                return call(s)
            return go
        _go(sc, "scan_host", behind(lambda s: s.scan_host(pats["A"], plain.window, SQ_BEST, dev.WANT_RECORDS)),
            lambda s, res: _same_scan(s, res, pref.scan("A", SQ_BEST), pref.offs), make)

        def multi(s, got):
            for flank, g in zip(FLANKS, got):
                e = pref.scan(flank, SQ_BEST)
                assert g["nlines"] == e["nlines"] and g["nmatchlines"] == e["nmatchlines"], flank
                assert np.array_equal(g["records"].astype(np.uint64), e["records"]), flank
        _go(sc, "scan_host_multi", behind(lambda s: s.scan_host_multi(list(pats.values()), plain.window, SQ_BEST, dev.WANT_RECORDS)), multi, make)
        _go(sc, "demux_host", behind(lambda s: s.demux_host(list(pats.values()), plain.window, SQ_BEST)), lambda s, res: _same_demux(res, pref.demux()), make)
        _go(sc, "strands_host", behind(lambda s: s.strands_host(pats["A"], plain.window, SQ_ALL)),
            lambda s, res: _same_strands(s, res, pref.strands("A", SQ_ALL), pref.offs), make)
        rows = fref.rows("AB")

        def inserts(s):
            s.bare()
            res = s.inserts_host(pats["A"], pats["B"], fq.window, SQ_BEST | dev.SEEQDEV_FASTQ)
            return res, s.tally(None), s.insert_text(None)      # (t=None: LateScanner puts a bare delay in front of each)

        def check(s, tr):
            res, tl, text = tr
            _same_inserts(s, res, fref.joined("AB", SQ_BEST), (0, 0), fref.offs)
            _same_tally(tl, [b for _, b in fref.spans(rows)])
            assert text == _host_text(fq.window, rows, fref.offs)
        _go(sc, "inserts_host, then the staged text", inserts, check, make)
        assert sc.arms >= 7


def test_two_contexts_on_two_streams_overlap(gpu, capi, setup, pats, late, monkeypatch):
    """Two hinted contexts on two side streams over two views, the module's Pattern objects shared (their tables are built on first use by
    whichever context comes first): run, run, fetch, fetch; then inserts and tally call by call in turn.  Each answers for its own view."""
    from seeq_amd import device as dev
    va, vb = setup.views["plain-b"], setup.views[FASTQ_VIEWS[0]]
    ra, rb = setup.ref(va), setup.ref(vb)
    ta, tb = va.tensor(), vb.tensor()
    a = late.scanner(va, pats, monkeypatch, late.side, hinted=True)()
    b = late.scanner(vb, pats, monkeypatch, late.other, hinted=True)()
    with late.closing(a, b), _a_fault_ends_the_module("two contexts on two streams"):
        a.run(pats["A"], ta.data_ptr(), ta.numel(), _opt(va, SQ_BEST), dev.WANT_RECORDS)
        b.run(pats["A"], tb.data_ptr(), tb.numel(), _opt(vb, SQ_BEST), dev.WANT_RECORDS)
        fa, fb = a.fetch(), b.fetch()
        _same_scan(a, fa, ra.scan("A", SQ_BEST), ra.offs)
        _same_scan(b, fb, rb.scan("A", SQ_BEST), rb.offs)
        for _ in range(2):
            _cut(a, va, ra, pats, "AB")
            _cut(b, vb, rb, pats, "CD")
            tla, tlb = a.tally(ta), b.tally(tb)
            _same_tally(tla, [s for _, s in ra.spans(ra.rows("AB"))])
            _same_tally(tlb, [s for _, s in rb.spans(rb.rows("CD"))])
        assert a.arms >= 5 and b.arms >= 5


# ---- the arms mean something: a context that is NOT ordered behind the producer reads the decoy ----
@pytest.mark.parametrize("name", ["plain-b", FASTQ_VIEWS[0]])
def test_an_unordered_context_sees_the_decoy(gpu, capi, setup, pats, late, name, monkeypatch):
    """A warm, hinted Scanner on a SECOND non-blocking stream while the text is armed on the first: nothing orders it behind the text's
    producer.  The decoy is in place before the arm (the arm copies the same bytes again) and every call is back while the producer is
    still pending: what it read is the decoy, and its scan, its inserts and its tally are the reference's over the decoy, other ones
    than the true ones.  It reads valid memory only: the wrong bytes, not a wrong address.  If a call outlasts the producer, D is too
    short for the arms above to mean anything."""
    import torch
    from seeq_amd import device as dev
    view = setup.views[name]
    ref, dref = setup.ref(view), late.decoy_ref(view)
    t = view.tensor()
    cycles = late.delay.cycles(late.delay_ms(view, pats, monkeypatch))
    text = L.LateText(t, view.window, late.side)
    sc = dev.Scanner(late.other.cuda_stream)
    sc.set_line_hint(_avg_line(view))
    opt = _opt(view, SQ_BEST)
    guides = ref.rows("AB")

    def unordered(call):
        text.put_decoy()
        text.arm(cycles)
        text.pending()
        res = call()
        early = not late.side.query()
        late.side.synchronize()                             # (the entry has returned; the true bytes are back)
        assert early, "an unordered call outlasted the text's producer: D is too short"
        return res
    with _a_fault_ends_the_module(name + ": an unordered context"):
        # warm, on the true text, nothing pending
        _same_scan(sc, sc.scan_tensor(pats["A"], t, opt, dev.WANT_RECORDS), ref.scan("A", SQ_BEST), ref.offs)
        _cut(sc, view, ref, pats, "AB")
        _same_tally(sc.tally(t), [s for _, s in ref.spans(guides)])
        torch.cuda.synchronize()
        # the scan
        res = unordered(lambda: sc.scan_tensor(pats["A"], t, opt, dev.WANT_RECORDS))
        _same_scan(sc, res, dref.scan("A", SQ_BEST), dref.offs)
        assert res["nlines"] == ref.scan("A", SQ_BEST)["nlines"] and res["nmatchlines"] != ref.scan("A", SQ_BEST)["nmatchlines"]
        # the inserts
        res = unordered(lambda: sc.inserts_tensor(pats["A"], pats["B"], t, opt))
        _same_inserts(sc, res, dref.joined("AB", SQ_BEST), (0, 0), dref.offs)
        assert dref.rows("AB") != guides and res["nlines"] == ref.scan("A", SQ_BEST)["nlines"]
        # the tally: the true text's insert records, their bytes read from the decoy
        _cut(sc, view, ref, pats, "AB")
        tl = unordered(lambda: sc.tally(t))
        seen = [s for _, s in dref.spans(guides)]
        _same_tally(tl, seen)
        assert seen != [s for _, s in ref.spans(guides)] and tl["ntallied"] > 0
        # and ordered again, it answers for the true text
        torch.cuda.synchronize()
        _same_scan(sc, sc.scan_tensor(pats["A"], t, opt, dev.WANT_RECORDS), ref.scan("A", SQ_BEST), ref.offs)
    torch.cuda.synchronize()
    sc.close()
