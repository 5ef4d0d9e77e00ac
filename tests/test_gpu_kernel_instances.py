"""Every kernel instance the planner can pick, run against the oracle: one scan per row of the ledger (tests/kernel_instances.py,
REPRESENTATIVES -- tests/test_kernel_instances_host.py keeps it complete), the test id spelling the instance.

A row's text (kernel_instances.build_text) is made from the row's pattern:
  * read-length recipes: ~2 400 lines of lengths mixed over m - 1, m, m + tau, 40, 75, 150, 151, 257 (400 and 550 under a hint of 400) as the
    row's line hint admits; a third of them carry a planted occurrence -- 60 %: 0 ... tau edits, 40 %: tau + 1 substitutions, the near misses --
    and one line in twelve is the pattern less tau + 1 bases.  Where a line lies over a seam of the walks the occurrence goes there: ending on the
    last byte before it, on its first byte, starting on it, across it -- the 8 KiB tile boundaries, the 128-byte lane chunks behind them and in
    the middle of the tile, and the first byte of each one's warm-up window (4 * stream_wu bytes before: 16 ... 32 for the table walks, 64 or 128
    in Myers mode).  Occurrences at the first and at the last byte of lines; the last line ends with one, and the text is scanned with its
    final newline and, in segments, without it.
  * long-line recipes: ~1 000 such lines around three lines of 40, 150 and 90 KB, 25 occurrences in each: at the start, at the end, two closer
    than m + tau.
  * SQ_CONVERT / SQ_IGNORE rows: 1 % foreign bytes, inside occurrences too (0.2 % and none for two of k_stream's variants, which hand text
    with more to other kernels by design: kernel_instances._foreign_rate); FASTA rows: header lines that hold the pattern.
Every row is asserted not to be vacuous (kernel_instances.vacuity), to have run the instance it names in ONE run, on the plan the host planner
predicts, and to give the oracle's counts, records and line offsets bit for bit -- then once more on a fresh context that scans in 64 KiB
segments: the same instance again, in one run, or -- where the exact pass walks k_pair's candidate windows -- in a second one that the seam
flag alone asked for and that differs in nothing but those windows.  A second test per row gives the same text as a window of a larger tensor,
at an odd and at a 16-aligned lead, between guards whose bytes would change the answer if a kernel used them (tests/text_window.py), and
once more in segments.  Two more tests pin what Scanner.last_plan() says after a fall-back
re-run and after a packed run."""
import numpy as np
import pytest

import kernel_instances as K
import text_window as W

pytestmark = pytest.mark.gpu

ROWS = sorted(K.rows(), key=lambda r: (r.pattern, r.tau, r.recipe, r.avg_line, r.options & ~3, r.key))
KNOBS = ("SEEQ_SEGMENT_BYTES", "SEEQ_FUSED_KERNEL", "SEEQ_PATH", "SEEQ_STREAM_WU", "SEEQ_STREAM_SUB", "SEEQ_NO_FILTER", "SEEQ_NO_WINDOW", "SEEQ_NO_MYERS",
         "SEEQ_NO_LEADERS", "SEEQ_TILE_BYTES", "SEEQ_EXPLAIN")
HITLINES = 1 << 21      # workspace for hit-list entries: room for every candidate of these texts in every wave's slice -- a run that came back for more
                        # room would be a second run, and the rows assert one


OVF_NONDNA, OVF_SEAM = 16, 128      # seeq_types.h: the fall-back bits Scanner.fallback() reports


class Shared:
    """what the rows share: device patterns, the last texts on the device, the oracle's answers"""

    def __init__(self, oracle):
        self.oracle, self.pats, self.tensors, self.exp = oracle, {}, {}, {}

    def pattern(self, expr, tau):
        from seeq_amd import device as dev
        if (expr, tau) not in self.pats:
            self.pats[expr, tau] = dev.Pattern(expr, tau)
        return self.pats[expr, tau]

    def tensor(self, text):
        import torch
        if id(text) not in self.tensors:
            if len(self.tensors) > 4:
                self.tensors.clear()
            t = torch.frombuffer(bytearray(text.buf), dtype=torch.uint8).cuda()
            torch.cuda.synchronize()
            self.tensors[id(text)] = (text, t)
        return self.tensors[id(text)][1]

    def expected(self, row, text, mode):
        key = (id(text), row.pattern, row.tau, mode | (row.options & 0x0C))
        if key not in self.exp:
            if len(self.exp) > 64:
                self.exp.clear()
            self.exp[key] = (text, self.oracle.buffer_scan(row.pattern, row.tau, text.buf, mode | (row.options & 0x0C), fasta=row.fasta))
        return self.exp[key][1]


@pytest.fixture(scope="module")
def shared(oracle, harness):
    K.use_harness(harness)
    sh = Shared(oracle)
    yield sh
    for p in sh.pats.values():
        p.close()


def _offsets(buf, fasta):
    """1-based counted line -> byte offset of its first byte"""
    offs, pos = [0], 0
    for ln in buf.split(b"\n")[:-1]:
        if not (fasta and ln.startswith(b">")):
            offs.append(pos)
        pos += len(ln) + 1
    return np.array(offs, dtype=np.uint64)


def _compare(what, sc, res, exp, exp_all, want, offsets):
    from seeq_amd import device as dev
    print(what, {k: res[k] for k in ("nlines", "nmatchlines", "nhits", "nrecords")}, "oracle:", exp["nlines"], exp["nmatchlines"], len(exp_all["records"]),
          len(exp["records"]), "| runs", sc.last_runs(), sc.last_kernel())
    assert res["nlines"] == exp["nlines"], what
    assert res["nmatchlines"] == exp["nmatchlines"], what
    if want == dev.WANT_COUNTLINES:
        assert res["nhits"] == exp["nmatchlines"] and res["nrecords"] == 0, what
    elif want == dev.WANT_COUNTMATCH:
        assert res["nhits"] == len(exp_all["records"]) and res["nrecords"] == 0, what
    else:
        n = len(exp["records"])
        assert res["nrecords"] == n, what
        rec = sc.records(n).astype(np.uint64)
        if not np.array_equal(rec, exp["records"]):
            bad = int(np.argmax((rec != exp["records"]).any(axis=1)))
            raise AssertionError("%s: records differ, first at %d: %s, oracle %s" % (what, bad, rec[bad].tolist(), exp["records"][bad].tolist()))
        assert np.array_equal(sc.record_offsets(n), offsets[exp["records"][:, 0].astype(np.int64)]), what + ": line offsets"


def _scanner(row, text, nlines):
    from seeq_amd import device as dev
    sc = dev.Scanner()
    sc.reserve(len(text.buf), nlines + 1024, HITLINES, HITLINES)
    if row.recipe != "fasta-per-read":
        sc.set_line_hint(row.avg_line)
    return sc


@pytest.mark.parametrize("row", ROWS, ids=[r.key.replace(" | ", "|") for r in ROWS])
def test_instance_against_the_oracle(gpu, capi, shared, row, monkeypatch):
    from seeq_amd import device as dev
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in row.knobs.items():
        monkeypatch.setenv(k, v)                            # (read when the context is made)
    plan = row.plan()
    assert K.instance_key(plan, row.options, row.want) == row.key
    text = row.text(plan)
    assert len(text.buf) < 1 << 20
    mode = (row.options & 3) if row.want == dev.WANT_RECORDS else K.SQ_ALL
    exp_all = shared.expected(row, text, K.SQ_ALL)
    exp = shared.expected(row, text, mode)
    # conditions on the input: a row that holds nothing to find, or nothing to reject, tests nothing
    why = K.vacuity(row, text, exp_all, plan)
    assert why is None, why
    offsets = _offsets(text.buf, row.fasta)
    pat = shared.pattern(row.pattern, row.tau)
    t = shared.tensor(text)
    options = row.options                                   # (kernel_instances.FASTA is SEEQDEV_FASTA)
    sc = _scanner(row, text, exp["nlines"])
    try:
        res = sc.scan_tensor(pat, t, options, row.want)
        got = sc.last_plan()
        # the instance ran: in one run (a fall-back re-run would have replaced it), and on the plan the host planner gives for the row
        assert sc.last_runs() == 1, ("runs", sc.last_runs(), "fallback", sc.fallback(), K.instance_key(got, row.options, row.want))
        assert K.instance_key(got, row.options, row.want) == row.key
        assert got == plan, (got, plan)
        _compare("one segment", sc, res, exp, exp_all, row.want, offsets)
    finally:
        sc.close()
    # once more across segment seams, and without the final newline (the same lines: the same answer)
    monkeypatch.setenv("SEEQ_SEGMENT_BYTES", "65536")
    sc = _scanner(row, text, exp["nlines"])
    try:
        res = sc.scan_tensor(pat, t[:-1], options, row.want)
        got, runs, fallback = sc.last_plan(), sc.last_runs(), sc.fallback()
        # the same instance crossed the seams -- not another one after a fall-back
        assert K.instance_key(got, row.options, row.want) == row.key, (runs, fallback)
        if plan["window_ok"] and runs != 1:
            # k_pair's candidate windows: a line with candidates on both sides of a seam voids the run (OVF_SEAM, seeq_order.h k_bounds2) and the
            # next one scans candidate lines whole -- the same kernels, by design.  That flag alone, one more run, nothing else of the plan
            assert runs == 2 and fallback[0] == OVF_SEAM, (runs, fallback)
            assert got == dict(plan, window_ok=0), (got, plan)
        else:
            assert runs == 1, ("runs", runs, "fallback", fallback)
            assert got == plan, (got, plan)
        _compare("64 KiB segments, no final newline", sc, res, exp, exp_all, row.want, offsets)
    finally:
        sc.close()


class _Window:
    """a row's hostile window in the shape Shared.expected takes (buf)"""

    def __init__(self, buf):
        self.buf = buf


_WINDOWS = {}       # (id of the row's text, pattern, tau, non-DNA mode, FASTA, closed) -> (_Window, before, after): rows that share a text share its window
SEEN = {}           # scan kernel -> the residues modulo 4096 of the leads it ran at


def _hostile_window(shared, row, i, plan):
    nd = row.options & 0x0C
    key = (id(row.text(plan)), row.pattern, row.tau, nd, row.fasta, bool(i % 2))
    if key not in _WINDOWS:
        if len(_WINDOWS) > 8:
            _WINDOWS.clear()

        def hits(buf):
            e = shared.oracle.buffer_scan(row.pattern, row.tau, buf, K.SQ_ALL | nd, fasta=row.fasta)
            return W.abs_hits(e["records"], W.line_offsets(buf, row.fasta))
        window, before, after, _ = W.row_case(row, i, hits, plan)
        _WINDOWS[key] = (row.text(plan), _Window(window), before, after)
    return _WINDOWS[key][1:]


@pytest.mark.parametrize("i", range(len(ROWS)), ids=[r.key.replace(" | ", "|") for r in ROWS])
def test_instance_on_a_hostile_window(gpu, capi, shared, i, monkeypatch):
    """Where the text lies and what surrounds it changes nothing (tests/text_window.py; tests/test_text_window_host.py shows on the CPU that
    every placement here is live: a kernel that used a byte outside the window would answer otherwise).  The row's text behind a first line
    that is the second half of an occurrence whose first half ends the guard (FASTA rows: the guard ends in `>`), and in front of a last
    line that is the first half of one (even rows; no final newline) or of a guard that begins with a line holding one (odd rows) --
    at an odd lead in a larger tensor and at a lead that is 16-aligned and not 128-aligned: the instance the row names, in one run, on the
    plan the host planner predicts (no planner input depends on the address), the oracle's counts, records and line offsets of the window's
    bytes alone.  Then the odd placement once more on a fresh context in 64 KiB segments."""
    import torch
    from seeq_amd import device as dev
    row = ROWS[i]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in row.knobs.items():
        monkeypatch.setenv(k, v)
    plan = row.plan()
    assert K.instance_key(plan, row.options, row.want) == row.key
    text, before, after = _hostile_window(shared, row, i, plan)
    assert len(text.buf) < (1 << 20) + W.TILE_BYTES + 256
    mode = (row.options & 3) if row.want == dev.WANT_RECORDS else K.SQ_ALL
    exp_all = shared.expected(row, text, K.SQ_ALL)
    exp = shared.expected(row, text, mode)
    offsets = _offsets(text.buf if text.buf.endswith(b"\n") else text.buf + b"\n", row.fasta)
    pat = shared.pattern(row.pattern, row.tau)
    odd = None
    for lead in (W.odd_lead(i), W.aligned_lead(i)):
        big, lo, hi = W.place(text.buf, lead, before, after)
        t = torch.frombuffer(bytearray(big), dtype=torch.uint8).cuda()[lo:hi]
        assert t.data_ptr() % 16 == lead % 16 and t.numel() == len(text.buf)
        odd = t if odd is None else odd
        sc = _scanner(row, text, exp["nlines"])
        try:
            res = sc.scan_tensor(pat, t, row.options, row.want)
            got = sc.last_plan()
            assert sc.last_runs() == 1, ("runs", sc.last_runs(), "fallback", sc.fallback(), K.instance_key(got, row.options, row.want))
            assert K.instance_key(got, row.options, row.want) == row.key
            assert got == plan, (got, plan)
            SEEN.setdefault(sc.last_kernel(), set()).add(lead - W.GUARD)
            _compare("lead %d" % lead, sc, res, exp, exp_all, row.want, offsets)
        finally:
            sc.close()
    monkeypatch.setenv("SEEQ_SEGMENT_BYTES", "65536")
    sc = _scanner(row, text, exp["nlines"])
    try:
        res = sc.scan_tensor(pat, odd, row.options, row.want)
        got, runs, fallback = sc.last_plan(), sc.last_runs(), sc.fallback()
        assert K.instance_key(got, row.options, row.want) == row.key, (runs, fallback)
        if plan["window_ok"] and runs != 1:
            assert runs == 2 and fallback[0] == OVF_SEAM, (runs, fallback)      # (as in test_instance_against_the_oracle)
            assert got == dict(plan, window_ok=0), (got, plan)
        else:
            assert runs == 1, ("runs", runs, "fallback", fallback)
            assert got == plan, (got, plan)
        _compare("lead %d, 64 KiB segments" % W.odd_lead(i), sc, res, exp, exp_all, row.want, offsets)
    finally:
        sc.close()


def test_every_scan_kernel_ran_at_small_and_at_large_odd_leads():
    """Closes test_instance_on_a_hostile_window: each scan kernel was seen at an odd lead below 16 and at one above 64 (modulo 4096)."""
    for kernel in ("k_forward", "k_direct", "k_stream", "k_pair", "k_myers"):
        leads = SEEN.get(kernel, set())
        assert any(r % 2 and r < 16 for r in leads) and any(r % 2 and r > 64 for r in leads), (kernel, sorted(leads))


def test_last_plan_after_a_fallback_rerun_is_the_reruns_plan(gpu, capi, shared, monkeypatch):
    """seeqdevScanLastPlan describes the run that produced the fetched result.  A row whose instance is k_stream's plain table walk under
    SQ_IGNORE -- exact on clean text only -- is given ITS text with 1 % foreign bytes: the first run comes back void (OVF_NONDNA), the second
    runs what the planner gives a context that carries that flag, and that is what last_plan() and last_path() / last_kernel() report."""
    from seeq_amd import device as dev
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    row = next(r for r in ROWS if (r.options & 0x0C) == K.SQ_IGNORE and not r.knobs and r.want == dev.WANT_RECORDS and r.plan()["path"] == 5
               and r.plan()["stream_sub"] == 0)
    first = row.plan()
    text = K.build_text(row.pattern, row.tau, row.recipe, row.avg_line, 4 * first["stream_wu"], 0.01, row.fasta)
    exp_all = shared.oracle.buffer_scan(row.pattern, row.tau, text.buf, K.SQ_ALL | K.SQ_IGNORE, fasta=row.fasta)
    exp = shared.oracle.buffer_scan(row.pattern, row.tau, text.buf, row.options & 0x0F, fasta=row.fasta)
    assert len(exp["records"]) > 50
    sc = _scanner(row, text, exp["nlines"])
    try:
        res = sc.scan_tensor(shared.pattern(row.pattern, row.tau), shared.tensor(text), row.options, row.want)
        got = sc.last_plan()
        assert sc.last_runs() == 2 and sc.fallback()[0] == OVF_NONDNA, (sc.last_runs(), sc.fallback())
        second = K.plan_of(K.harness_lib(), row.pattern, row.tau, row.options, row.want, row.avg_line, row.flags | K.FLAG_NO_STREAM_ND, row.kernel)
        assert got == second and got != first, (got, first, second)
        assert K.instance_key(got, row.options, row.want) != row.key
        assert sc.last_kernel() == {1: "k_forward", 3: "k_direct", 5: "k_stream", 6: "k_pair", 7: "k_myers"}[got["path"]]
        _compare("dirty text, re-run", sc, res, exp, exp_all, row.want, _offsets(text.buf, row.fasta))
    finally:
        sc.close()


def test_last_plan_of_a_packed_run(gpu, capi, shared):
    """A packed run has no ScanPlan: path 8 and the filter flag, everything else 0 -- also when the context ran a planned scan before."""
    import torch
    from seeq_amd import device as dev
    expr, tau, L = "GATGTAGCGCGATTAGCCTG", 3, 150
    text = bytes(shared.oracle.synth_reads(0, 2000, L, expr, tau))
    exp = shared.oracle.buffer_scan(expr, tau, text, K.SQ_BEST)
    pat = shared.pattern(expr, tau)
    bases, nmask, n = dev.pack_reads(text, L)
    db, dn = torch.from_numpy(bases.copy()).cuda(), torch.from_numpy(nmask.copy()).cuda()
    sc = dev.Scanner()
    try:
        assert sc.last_plan() == dict.fromkeys(K.PLAN_FIELDS, 0)                       # before the first scan
        t = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
        sc.scan_tensor(pat, t, K.SQ_BEST, dev.WANT_RECORDS)
        assert sc.last_plan()["path"] == 6
        sc.run_packed(pat, db.data_ptr(), dn.data_ptr(), n, L, options=K.SQ_BEST, want=dev.WANT_RECORDS)
        res = sc.fetch()
        assert res["nrecords"] == len(exp["records"]) > 50
        assert np.array_equal(sc.records(res["nrecords"]).astype(np.uint64), exp["records"])
        assert sc.last_plan() == dict(dict.fromkeys(K.PLAN_FIELDS, 0), path=8, filter=1) and sc.last_path() == "packed"
    finally:
        sc.close()
