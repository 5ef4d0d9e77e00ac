"""GPU (-m gpu): every device entry on a text whose offsets pass 2^31, the default segment seam (3.75 GiB) and 2^32.  The rule: how far into
its buffer a line lies changes no answer.  Everywhere else in the suite a text is a few hundred KiB, so a post-pass that kept a line offset
in 32 bits, an (int) on a segment-relative position, a 16-byte span load that drops the carry into bit 32, or a scan kernel that is wrong only
above 2^31 in its segment would pass; here they do not (tests/test_far_text_host.py shows on the CPU that such a reference answers otherwise).

Part A -- the entries behind the scan (tests/far_text.py: Layout).  4 GiB of hitless filler around three copies of the chain text, one across
each boundary, built on the device from the filler unit and the pieces; the families of tests/test_gpu_text_window.py, the anchored cut and the
appended key column run cold and then warm on ONE context per view:
  far-fastq, far-plain         default segments: the real seam lies in block 2, block 3 is 0.25 GiB into segment 1;
  far-fastq-1g, far-plain-1g   SEEQ_SEGMENT_BYTES = 1 GiB: five segments, seams exactly on 2^31 and 2^32 inside blocks.
The reference is the oracle and the restated rules over the COMPACT text -- the three blocks alone -- mapped forward (far_text.FarRef); span
bytes, insert text and gate inputs come from far_text.FarBytes.  Never another GPU run, never the oracle over 4 GiB, and nothing from the device
is mapped back.  A first test holds the device text against FarBytes around every edge and boundary.

Part B -- the scan kernels far into a segment (far_text.FarRow, FAR_ROWS): lead + K x the text of a ledger row, 2^32 inside a record; the oracle
over one period, replicated; counts, all records, all line offsets, the instance the row names, in one run (or two with the seam flag alone).
That the list covers the kernel families it is there for is asserted where it also runs without a GPU: tests/test_far_text_host.py,
test_the_far_rows_cover_the_kernel_families.

One far tensor is alive at a time; a device fault ends the module (test_gpu_text_window.py: _nothing_after_a_device_fault)."""
import inspect
import random

import numpy as np
import pytest

import far_text as F
import kernel_instances as K
import late_text as L
import test_gpu_text_window as TW
from oracle.pyoracle import SQ_BEST
from test_anchor_host import AFTER, BEFORE, LINE
from test_gpu_anchor import _same as _same_anchor
from test_gpu_kernel_instances import OVF_SEAM
from test_gpu_tally_append import APPEND, _held_arrays
from test_gpu_tally_grouped import _held_of
from test_gpu_text_window import _cut, _gate, _go, _inserts, _library, _opt, _same_scan, _scans, _tallies
from test_gpu_text_window import _nothing_after_a_device_fault, pats      # noqa: F401  (fixtures: the fault rule is this module's too)
from test_qgate_host import PASS
from test_tally_append_host import py_append
from test_tally_library_host import PyLibrary

pytestmark = pytest.mark.gpu
GIB = 1 << 30
VIEWS = {"far-fastq": (True, None), "far-fastq-1g": (True, str(GIB)), "far-plain": (False, None), "far-plain-1g": (False, str(GIB))}
FAMILIES = ("scans", "inserts", "tallies", "library", "gate", "anchor", "append")
CASES = [(name, which) for name in VIEWS for which in FAMILIES if which != "gate" or VIEWS[name][0]]
# the anchored cuts: to the line's end from behind the hit, fixed lengths behind it, columns of the line, in front of the hit
ANCHOR_PARAMS = ((AFTER, 0, 0, 1024), (AFTER, 3, 12, 1024), (AFTER, 0, 17, 64), (LINE, 0, 16, 1024), (LINE, 16, 0, 1024), (BEFORE, 0, 17, 1024))
TEXT_PARAMS = L.TEXT_PARAMS + ("text",)
# methods of Scanner that take device text and are NOT run on a far view: name -> why
EXEMPT = {"run_packed": "its input is the packed arrays of fixed-length reads, addressed by read number and stride: no text offset reaches it"}
REACHED = set()


def _text_methods():
    """late_text.text_methods(), and the entries whose text parameter is called `text`"""
    out = {}
    for name, fn in inspect.getmembers(__import__("seeq_amd.device", fromlist=["Scanner"]).Scanner, callable):
        if not name.startswith("_"):
            hit = [p for p in TEXT_PARAMS if p in inspect.signature(inspect.unwrap(fn)).parameters]
            if hit:
                out[name] = hit[0]
    return out


def _far_scanner_class():
    """Scanner that notes which of its text-taking methods were given a far text (a tensor, or an address with a length, of 4 GiB or more)"""
    from seeq_amd import device as dev

    class FarScanner(dev.Scanner):
        gates = ()

        def __init__(self, *args):
            super().__init__(*args)
            self.gates = []

    def noting(name, param):
        base = getattr(dev.Scanner, name)
        sig = inspect.signature(base)

        def method(self, *args, **kw):
            bound = sig.bind(self, *args, **kw)
            bound.apply_defaults()
            text = bound.arguments[param]
            n = bound.arguments.get("nbytes", 0) if isinstance(text, int) else 0 if text is None else text.numel()
            if n >= F.B32:
                REACHED.add(name)
            res = base(self, *args, **kw)
            if name == "quality_gate":
                self.gates.append(res)                      # (what the device said: test_family_on_a_far_text looks at the boundary records)
            return res
        method.__name__, method.__doc__ = name, base.__doc__
        return method
    for name, param in _text_methods().items():
        if name not in EXEMPT:
            setattr(FarScanner, name, noting(name, param))
    return FarScanner


class FarView:
    """What the families take for a view (test_gpu_text_window.py: View): name, window (FarBytes), fastq, tensor()"""

    def __init__(self, name, far, layout, segment):
        self.name, self.far, self.layout, self.window, self.fastq, self.segment, self.segments = name, far, layout, layout.far, layout.fastq, segment, False

    def tensor(self):
        return self.far.tensor(self.layout)


class Far:
    """What the module shares: the layouts and references of both texts, the ONE far tensor, the one context of the view in use, the
    peak of device memory."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.layouts = {fastq: F.Layout(oracle, fastq) for fastq in (True, False)}
        self.refs = {fastq: F.FarRef(oracle, lay) for fastq, lay in self.layouts.items()}
        self.views = {name: FarView(name, self, self.layouts[fastq], seg) for name, (fastq, seg) in VIEWS.items()}
        self.chain = self.layouts[True].chain
        self.held, self.t, self.sc, self.sc_view, self.peak, self.base = None, None, None, None, 0, None
        self.scanner_class = _far_scanner_class()
        for name, view in self.views.items():
            for ln in view.layout.phases(self.refs[view.fastq]):
                print("far text, %s%s: %s" % (name, ", segments of %s bytes" % view.segment if view.segment else "", ln))

    def sample(self):
        import torch
        free, total = torch.cuda.mem_get_info()
        if self.base is None:
            self.base = total - free
        self.peak = max(self.peak, total - free)

    def tensor(self, layout):
        """the layout's text on the device; the other one is freed first.  Filler runs are written as the unit broadcast over a (n, U)
        view of their bytes -- every gap has its own phase --, blocks and adjusted units are slice-assigned."""
        import torch
        if self.held is not layout:
            self.release()
            self.sample()
            unit = torch.frombuffer(bytearray(layout.fill.unit), dtype=torch.uint8).cuda()
            t = torch.empty(len(layout.far), dtype=torch.uint8, device="cuda")
            for start, piece in layout.far.items():
                if isinstance(piece, bytes):
                    t[start:start + len(piece)] = torch.frombuffer(bytearray(piece), dtype=torch.uint8).cuda()
                else:
                    t[start:start + piece * len(unit)].view(piece, len(unit)).copy_(unit)
            torch.cuda.synchronize()
            self.held, self.t = layout, t
            self.sample()
        return self.t

    def release(self):
        import torch
        self.close_scanner()
        self.held = self.t = None
        torch.cuda.empty_cache()

    def make(self, view, monkeypatch):
        """a fresh context of the view's kind (SEEQ_SEGMENT_BYTES is read when a context is made)"""
        if view.segment:
            monkeypatch.setenv("SEEQ_SEGMENT_BYTES", view.segment)
        return self.scanner_class()

    def scanner(self, view, monkeypatch):
        """the view's one context: made at the view's first family, closed when another view begins"""
        if self.sc_view != view.name:
            self.close_scanner()
            self.sc, self.sc_view = self.make(view, monkeypatch), view.name
        return self.sc

    def close_scanner(self):
        if self.sc is not None:
            self.sc.close()
        self.sc = self.sc_view = None


@pytest.fixture(scope="module")
def far(gpu, oracle):
    import torch
    state = Far(oracle)
    yield state
    state.release()
    print("far text: peak device memory in use %.2f GiB (%.2f GiB before the first far tensor); of %.0f GiB"
          % (state.peak / GIB, (state.base or 0) / GIB, torch.cuda.mem_get_info()[1] / GIB))


@pytest.fixture(autouse=True)
def _memory(request):
    yield
    if "far" in request.fixturenames and not TW._FAULT:
        request.getfixturevalue("far").sample()


# ---- the text on the device is the text the reference reads ----
@pytest.mark.parametrize("fastq", [True, False], ids=["fastq", "plain"])
def test_the_device_text_is_far_bytes(gpu, capi, far, fastq):
    lay = far.layouts[fastq]
    t = far.tensor(lay)
    fb = lay.far
    assert t.numel() == len(fb) > F.B32 and t.is_contiguous()

    def same(a, b):
        a, b = max(0, a), min(len(fb), b)
        assert t[a:b].cpu().numpy().tobytes() == fb[a:b], (a, b)
    for edge in fb.starts + [len(fb)]:
        same(edge - 600, edge + 600)
    for start in lay.block_start:
        same(start, start + len(lay.block))
    for B in lay.bounds.values():
        same(B - 4096, B + 4096)
    rng = random.Random(64)
    fills = [(s, s + p * len(fb.unit)) for s, p in fb.items() if not isinstance(p, bytes)]
    for i in range(64):
        lo, hi = fills[i % len(fills)]
        a = rng.randrange(lo, hi)
        same(a, a + 777)
    step = 1 << 28                                          # (in parts: no second tensor of the text's size)
    newlines = sum(int((t[a:a + step] == 10).sum().item()) for a in range(0, t.numel(), step))
    assert newlines == (lay.nlines * 4 if fastq else lay.nlines)


# ---- the families ----
def _anchor(sc, view, ref, pats, fresh):
    """the hits of FB, held against the reference, cut at fixed offsets: every cut against the rule over the far bytes"""
    from seeq_amd import device as dev
    t = view.tensor()
    exp = ref.scan("B", SQ_BEST)
    n = len(exp["records"])

    def call(s):
        res = s.scan_tensor(pats["B"], t, _opt(view, SQ_BEST), dev.WANT_RECORDS)
        _same_scan(s, res, exp, ref.offs)
        rec, off = s.records(n), s.record_offsets(n)
        return rec, off, [s.anchor(t, source="hits", anchor=p[0], skip=p[1], length=p[2], reach=p[3]) for p in ANCHOR_PARAMS]

    def check(s, out):
        rec, off, results = out
        for p, res in zip(ANCHOR_PARAMS, results):
            kinds, rows, _, cnt = _same_anchor(res, view.window, rec, off, p)
            assert cnt["nkept"] > 1000, (p, cnt)
    _go(sc, view.name + ": anchored cuts of the hits", call, check, fresh)


def _append(sc, view, ref, pats, chain, fresh):
    """hold the UMIs, append the guides' library ids: the held column against the host join (tests/test_tally_append_host.py)"""
    t = view.tensor()
    lib = PyLibrary(chain.guides)
    guides, umis = ref.spans(ref.rows("AB")), ref.spans(ref.rows("CD"))
    held0, hcnt = _held_of(umis)
    ids = lib.tally([b for _, b in guides], 1)[2]
    exp_held, acnt = py_append(held0, [(ln, i) for (ln, _), i in zip(guides, ids)], width=len(chain.guides).bit_length())
    acnt["ncolumns"] = 2
    assert acnt["nheld"] > 1000 and acnt["ndropped"] > 100

    def call(s):
        s.set_library(lib.seqs, 1)
        _cut(s, view, ref, pats, "CD")
        hold = s.tally_hold(t)
        _cut(s, view, ref, pats, "AB")
        app = s.tally_hold_append(t, library=True)
        return hold, app, _held_arrays(s), s.hold_columns()

    def check(s, out):
        hold, app, held, widths = out
        assert hold == hcnt and {k: app[k] for k in APPEND} == acnt
        assert held == exp_held and widths == [hcnt["key_bits"], acnt["width"]]
    _go(sc, view.name + ": hold, append a library column", call, check, fresh)


def _family(which, sc, view, ref, pats, chain, fresh):
    if which == "scans":
        return _scans(sc, view, ref, pats, fresh=fresh)
    if which == "inserts":
        return _inserts(sc, view, ref, pats, fresh=fresh)
    if which == "tallies":
        return _tallies(sc, view, ref, pats, fresh=fresh)
    if which == "library":
        return _library(sc, view, ref, pats, chain, fresh=fresh)
    if which == "anchor":
        return _anchor(sc, view, ref, pats, fresh)
    if which == "append":
        return _append(sc, view, ref, pats, chain, fresh)
    assert which == "gate" and view.fastq
    return _gate(sc, view, ref, pats, fresh=fresh)


@pytest.mark.parametrize("name,which", CASES, ids=["%s-%s" % c for c in CASES])
def test_family_on_a_far_text(gpu, capi, far, pats, name, which, monkeypatch):
    """cold, then warm, on the view's one context"""
    view = far.views[name]
    ref = far.refs[view.fastq]
    view.tensor()                                           # (first: a change of text ends the context of the view before)
    sc = far.scanner(view, monkeypatch)
    del sc.gates[:]
    for _ in ("cold", "warm"):
        _family(which, sc, view, ref, pats, far.chain, lambda: far.make(view, monkeypatch))
    if which == "gate":
        # the DEVICE's kinds of the guides the boundaries cut (the family has held all of them against the reference): PASS, cold and
        # warm -- the walk from the guide to its quality bytes crossed the seam and 2^32
        rows = ref.rows("AB")
        said = [g["kinds"].tolist() for g in sc.gates if "kinds" in g and g["nspans"] == len(rows) and len(g["kinds"]) == len(rows)]
        assert len(said) >= 2
        for role in ("SEAM", "B32"):
            assert all(kinds[rows.index(view.layout.cut[role])] == PASS for kinds in said), role


def test_every_method_that_reads_device_text_ran_on_a_far_text(far):
    """Scanner's public methods with a parameter named t, d_ptr, bases_ptr or text (late_text.text_methods, and the two entries that call
    it `text`): each was given a text of 4 GiB or more above, or is exempt with a reason"""
    found = _text_methods()
    assert set(L.text_methods()) <= set(found) and {"anchor", "tally_hold_append"} <= set(found), sorted(found)
    for name in found:
        if name in EXEMPT:
            assert EXEMPT[name].strip() and name not in REACHED
            continue
        assert name in REACHED, "Scanner.%s reads device text (%s) and no far view reached it" % (name, found[name])
    assert set(EXEMPT) <= set(found)


# ---- Part B: the scan kernels far into a segment ----
ROWS = F.far_rows()


class Periodic:
    """Part A's tensors freed; one device buffer, refilled per row; patterns"""

    def __init__(self, far):
        import torch
        far.release()
        far.sample()
        self.far, self.pats = far, {}
        self.buf = torch.empty(F.B32 + 4 * (1 << 20), dtype=torch.uint8, device="cuda")
        far.sample()

    def fill(self, fr):
        import torch
        assert fr.nbytes <= self.buf.numel()
        n = len(fr.lead)
        self.buf[:n] = torch.frombuffer(bytearray(fr.lead), dtype=torch.uint8).cuda()
        self.buf[n:fr.nbytes].view(fr.K, fr.P).copy_(torch.frombuffer(bytearray(fr.period), dtype=torch.uint8).cuda())
        torch.cuda.synchronize()
        return self.buf[:fr.nbytes]

    def pattern(self, expr, tau):
        from seeq_amd import device as dev
        if (expr, tau) not in self.pats:
            self.pats[expr, tau] = dev.Pattern(expr, tau)
        return self.pats[expr, tau]


@pytest.fixture(scope="module")
def periodic(gpu, far, harness):
    import torch
    K.use_harness(harness)
    state = Periodic(far)
    yield state
    for p in state.pats.values():
        p.close()
    state.buf = None
    torch.cuda.empty_cache()


@pytest.mark.parametrize("row", ROWS, ids=[r.key.replace(" | ", "|") for r in ROWS])
def test_instance_far_into_its_segment(gpu, capi, oracle, periodic, row, monkeypatch):
    from seeq_amd import device as dev
    for k, v in row.knobs.items():
        monkeypatch.setenv(k, v)                            # (read when the context is made; the fixture above has unset every knob)
    plan = row.plan()
    assert K.instance_key(plan, row.options, row.want) == row.key
    fr = F.FarRow(row, oracle, plan=plan)
    print("far row:", fr.describe())
    t = periodic.fill(fr)
    # spot checks of the fill: the lead, the first repeat, the repeat 2^32 lies in, the last one
    n = len(fr.lead)
    for a, b, exp in ((0, n, fr.lead), (n, n + 4096, fr.period[:4096]), (fr.nbytes - 4096, fr.nbytes, fr.period[-4096:]),
                      (n + fr.copy * fr.P, n + fr.copy * fr.P + fr.P, fr.period)):
        assert t[a:b].cpu().numpy().tobytes() == exp
    sc = dev.Scanner()
    try:
        # one run: a run that came back for more room would be a second one.  Lines: every newline of the text (FASTA headers take a place in
        # the per-line arrays; they are per segment, so this is more than enough).  Hit-list entries: the workspace is cut into a slice per
        # wave of the grid -- the rows' own test gives a text of under 1 MiB 2^21 for that reason; here the candidates are spread evenly
        # over the slices, and one entry per 64 bytes of text is several times what the densest row holds (a plant in every third line,
        # a match in nearly every line of 79 bytes).  Records: the reference's count.
        newlines = fr.lead.count(b"\n") + fr.K * fr.period.count(b"\n")
        sc.reserve(fr.nbytes, newlines + 1024, fr.nbytes // 64, max(1 << 21, fr.nrecords() + 1024))
        if row.recipe != "fasta-per-read":
            sc.set_line_hint(row.avg_line)
        res = sc.scan_tensor(periodic.pattern(row.pattern, row.tau), t, row.options, row.want)
        got, runs, fallback = sc.last_plan(), sc.last_runs(), sc.fallback()
        print("far row:", {k: res[k] for k in ("nlines", "nmatchlines", "nhits", "nrecords")}, "| runs", runs, "fallback", fallback, sc.last_kernel())
        assert K.instance_key(got, row.options, row.want) == row.key, (runs, fallback)
        if plan["window_ok"] and runs != 1:
            # (tests/test_gpu_kernel_instances.py, the segmented scan: the seam flag alone, one more run, nothing else of the plan)
            assert runs == 2 and fallback[0] == OVF_SEAM, (runs, fallback)
            assert got == dict(plan, window_ok=0), (got, plan)
        else:
            assert runs == 1, ("runs", runs, "fallback", fallback)
            assert got == plan, (got, plan)
        assert res["nlines"] == fr.nlines() and res["nmatchlines"] == fr.nmatchlines()
        if row.want == dev.WANT_COUNTLINES:
            assert res["nhits"] == fr.nmatchlines() and res["nrecords"] == 0
        elif row.want == dev.WANT_COUNTMATCH:
            assert res["nhits"] == fr.nhits_all() and res["nrecords"] == 0
        else:
            nrec = fr.nrecords()
            assert res["nrecords"] == nrec
            rec, exp = sc.records(nrec), fr.records()
            if not np.array_equal(rec, exp):
                bad = int(np.argmax((rec != exp).any(axis=1)))
                raise AssertionError("records differ, first at %d of %d: %s, expected %s" % (bad, nrec, rec[bad].tolist(), exp[bad].tolist()))
            del rec, exp
            off, exp = sc.record_offsets(nrec), fr.offsets()
            assert exp[-1] > F.B32 and off.dtype == exp.dtype == np.uint64
            if not np.array_equal(off, exp):
                bad = int(np.argmax(off != exp))
                raise AssertionError("line offsets differ, first at %d of %d: %#x, expected %#x" % (bad, nrec, int(off[bad]), int(exp[bad])))
    except dev.SeeqDeviceError as e:
        text = str(e).lower()
        if "illegal" in text or "launch failure" in text or "hardware" in text:
            TW._FAULT.append("%s: %s" % (row.key, e))         # (nothing more is started on the device: _nothing_after_a_device_fault)
        raise
    finally:
        sc.close()
