"""GPU (-m gpu): the state a scan context carries from one call to the next -- the fall-back flags with their lifetime (seeq_rerun.h),
the cached line-length sample and the caller's line hint (scan_setup), the workspace that earlier calls grew and cut into regions
(seeq_workspace.h, reserve_impl), the one multi-plan slot -- on LONG-LIVED Scanners: every step of every test is compared with the
oracle's scan of exactly the bytes scanned (counts, all record fields, record_offsets), and a step that fails says whether the same call
on a fresh Scanner in the same environment fails too (a kernel bug) or not (a state bug).  Scanner.last_runs() and Scanner.fallback()
prove that the state was exercised: a re-run happened, a flag was set and dropped again, a wrong hint changed the plan."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle.pyoracle import SQ_ALL, SQ_BEST, SQ_CONVERT, SQ_FIRST, SQ_IGNORE
from test_gpu_demux import BARCODES, TAUS, _check as demux_check, _expected as demux_expected, _mixed_lines, _mutate
from test_gpu_strands import Expected, _check as strands_check, _line_offsets, _lines as strand_lines, _step

pytestmark = pytest.mark.gpu
PAT20 = "GATGTAGCGCGATTAGCCTG"
PAT40 = "GATG[TA]AGCNCGATTAGC[CG]TGAAAATGNGAGTAC[GAT]GCGCGA"
_rng42 = random.Random(1000 * 42 + 15)
SWEEP42 = "".join(_rng42.choice("ACGT") for _ in range(42))       # the (42, 15) cell of the published sweep: no selective automaton
MER8 = "ACGTTGCA"
SEG = 65536
TILE = 8192                    # bytes of a k_pair / k_stream tile (64 lanes of 128 bytes): a candidate in a tile without a newline asks for the long-line variant


# ---- texts ----
def _dna(rng, n):
    return [rng.choice("ACGT") for _ in range(n)]


def _plant(rng, t, plants, count, both_strands=True):
    """`count` mutated copies of the patterns in `plants` [(expression, tau)] -- of the pattern or of its reverse complement -- into t."""
    from seeq_amd import device as dev
    for _ in range(count):
        expr, tau = plants[rng.randrange(len(plants))]
        if both_strands and rng.random() < 0.5:
            expr = dev.revcomp_pattern(expr)
        c = _mutate(rng, dev.plain_pattern(expr), rng.randint(0, tau + 1))
        p = rng.randrange(0, max(1, len(t) - len(c)))
        t[p:p + len(c)] = list(c)


def _read_lines(seed, n, plants, lengths=(150,), nbase=False):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        m = rng.choice(list(lengths))
        t = _dna(rng, m)
        _plant(rng, t, plants, rng.choice([0, 1, 1, 2]))
        if nbase and rng.random() < 0.02:
            t[rng.randrange(m)] = "N"
        out.append("".join(t)[:m])
    return out


def _long_line(rng, n, plants, count=25):
    t = _dna(rng, n)
    _plant(rng, t, plants, count)
    return "".join(t)[:n]


def _long_text(seed, plants, nreads=300, longs=(40_000, 120_000, 64_000, 90_000, 48_000, 100_000)):
    """About nreads reads around six long lines, ~25 plants in each of them; the first 64 KiB -- what a context samples -- are reads."""
    rng = random.Random(seed)
    reads = _read_lines(seed + 1, nreads, plants)
    first = 450 if nreads >= 450 else 0                   # (450 reads of 151 bytes: past the sample)
    lines, at = reads[:first], first
    step = max(1, (nreads - first) // len(longs))
    for n in longs:
        lines.append(_long_line(rng, n, plants))
        lines += reads[at:at + step]
        at += step
    return lines + reads[at:]


def _buf(lines):
    return ("\n".join(lines) + "\n").encode()


def _foreign(buf, seed, byte, rate=0.01):
    rng = random.Random(seed)
    return bytes(c if c == 10 or rng.random() > rate else byte for c in buf)


def _fastq(seqs, header_expr):
    """Four-line records: the header carries the pattern, the quality line is a copy of the sequence line (both would match unflagged)."""
    raw = []
    for i, sq in enumerate(seqs):
        raw += ["@r%d %s" % (i, header_expr), sq, "+", sq]
    return raw


def _fit(lines, nbytes, seed, group=1):
    """The lines (whole groups of `group`) that fit into nbytes, the last one extended with bases so that the buffer is exactly nbytes long."""
    rng = random.Random(seed)
    out, used = [], 0
    for g in range(0, len(lines) - group + 1, group):
        size = sum(len(ln) + 1 for ln in lines[g:g + group])
        if used + size > nbytes:
            break
        out += lines[g:g + group]
        used += size
    out[-1] += "".join(_dna(rng, nbytes - used))
    buf = _buf(out)
    assert len(buf) == nbytes
    return out, buf


# ---- the oracle, memoised per (text, pattern, mode) ----
class Memo:
    """oracle.buffer_scan with a memory: Expected (test_gpu_strands.py) and _expected (test_gpu_demux.py) take it for the oracle."""

    def __init__(self, oracle):
        self.oracle, self.scans, self.made = oracle, {}, {}

    def buffer_scan(self, expr, tau, buf, options=0, fasta=False):
        key = (buf, expr, tau, options & 0xFF, fasta)
        if key not in self.scans:
            self.scans[key] = self.oracle.buffer_scan(expr, tau, buf, options & 0xFF, fasta=fasta)
        return self.scans[key]

    def strands(self, expr, tau, buf, mode, opt=0, fasta=False):
        key = ("strands", buf, expr, tau, mode, opt, fasta)
        if key not in self.made:
            self.made[key] = Expected(self, expr, tau, buf, mode, opt, fasta)
        return self.made[key]

    def demux(self, exprs, taus, buf):
        key = ("demux", buf, tuple(exprs), tuple(taus))
        if key not in self.made:
            self.made[key] = demux_expected(self, exprs, taus, buf)
        return self.made[key]


@pytest.fixture(scope="module")
def memo(oracle):
    return Memo(oracle)


class Patterns:
    def __init__(self):
        self.made = {}

    def __call__(self, expr, tau):
        from seeq_amd import device as dev
        if (expr, tau) not in self.made:
            self.made[expr, tau] = dev.Pattern(expr, tau)
        return self.made[expr, tau]


@pytest.fixture(scope="module")
def pattern():
    ps = Patterns()
    yield ps
    for p in ps.made.values():
        p.close()


def _tensor(buf):
    import torch
    t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def _offsets_of(buf, fasta=False):
    return np.array([0] + _line_offsets(buf, fasta)[1:], dtype=np.uint64)      # index = counted line number (1-based)


def _plain_check(exp, offsets, want, nheaders=None):
    """-> check(sc, res) of a fetched plain scan against the oracle's result `exp` (for the count wants: the SQ_ALL scan)."""
    from seeq_amd import device as dev

    def check(sc, res):
        n = len(exp["records"])
        assert res["nlines"] == exp["nlines"], (res["nlines"], exp["nlines"])
        assert res["nmatchlines"] == exp["nmatchlines"], (res["nmatchlines"], exp["nmatchlines"])
        if nheaders is not None:
            assert res["nheaders"] == nheaders
        if want == dev.WANT_COUNTLINES:
            assert res["nhits"] == exp["nmatchlines"] and res["nrecords"] == 0
        elif want == dev.WANT_COUNTMATCH:
            assert res["nhits"] == n and res["nrecords"] == 0
        else:
            assert res["nrecords"] == n, (res["nrecords"], n)
            rec = sc.records(n)
            assert not (rec[:, 3] >> 31).any(), "a strand bit in a plain scan's dist"
            if not np.array_equal(rec.astype(np.uint64), exp["records"]):
                bad = int(np.argmax((rec.astype(np.uint64) != exp["records"]).any(axis=1)))
                raise AssertionError("records differ, first at %d: %s vs %s" % (bad, rec[bad].tolist(), exp["records"][bad].tolist()))
            assert np.array_equal(sc.record_offsets(n), offsets[exp["records"][:, 0].astype(np.int64)])
    return check


def _plain(memo, sc, what, pat, expr, tau, t, buf, options, want, fasta=False, fastq_of=None, fresh=None):
    """A resident plain scan as one step.  fastq_of = (buffer of the sequence lines alone, their offsets in `buf`): SEEQDEV_FASTQ."""
    from seeq_amd import device as dev
    mode = options & 3 if want == dev.WANT_RECORDS else SQ_ALL
    nd = options & 0x0C
    if fastq_of is not None:
        exp, offsets = memo.buffer_scan(expr, tau, fastq_of[0], mode | nd), fastq_of[1]
        opts = options | dev.SEEQDEV_FASTQ
    else:
        exp, offsets = memo.buffer_scan(expr, tau, buf, mode | nd, fasta), _offsets_of(buf, fasta)
        opts = options | (dev.SEEQDEV_FASTA if fasta else 0)
    _step(sc, what, lambda s: s.scan_tensor(pat, t, opts, want), _plain_check(exp, offsets, want), fresh)


def _strands(memo, sc, what, pat, expr, tau, t, buf, options, want, fasta=False, fastq_of=None, fresh=None):
    from seeq_amd import device as dev
    mode = options & 3 if want == dev.WANT_RECORDS else (SQ_FIRST if want == dev.WANT_COUNTLINES else SQ_ALL)
    nd = options & 0x0C
    if fastq_of is not None:
        exp, offsets = memo.strands(expr, tau, fastq_of[0], mode, nd), [None] + fastq_of[1][1:].tolist()
        opts = options | dev.SEEQDEV_FASTQ
    else:
        exp, offsets = memo.strands(expr, tau, buf, mode, nd, fasta), _line_offsets(buf, fasta)
        opts = options | (dev.SEEQDEV_FASTA if fasta else 0)

    def check(s, res):
        strands_check(s, res, exp, offsets, records=want == dev.WANT_RECORDS)
        with pytest.raises(dev.SeeqDeviceError):
            s.fetch()                                      # the call is complete: nothing left to fetch

    _step(sc, what, lambda s: s.strands_tensor(pat, t, opts, want), check, fresh)


def _fastq_of(seqs, raw_buf):
    """(the sequence lines' buffer, offset of record r's sequence line in raw_buf at index r)."""
    raw_off = _line_offsets(raw_buf)
    return _buf(seqs), np.array([0] + [raw_off[4 * r + 2] for r in range(len(seqs))], dtype=np.uint64)


# =====================================================================================================================
# 1. a line hint that is wrong in both directions
# =====================================================================================================================
HINT_PLANTS = [(PAT20, 3), (PAT40, 5), (SWEEP42, 15)]
HINTS = (0, 1, 151, 400, 5000, 1e6)


@pytest.fixture(scope="module")
def hint_texts():
    mid = _read_lines(72, 1498, HINT_PLANTS, lengths=range(258, 700)) + _read_lines(74, 1, HINT_PLANTS, lengths=(258,)) + _read_lines(75, 1, HINT_PLANTS, lengths=(699,))
    bufs = {"R": _buf(_read_lines(71, 3000, HINT_PLANTS)),
            "M": _buf(mid),                                # 259 .. 700 bytes with the newline
            "L": _buf(_long_text(73, HINT_PLANTS))}
    assert min(len(ln) + 1 for ln in bufs["M"].split(b"\n")[:-1]) == 259 and max(len(ln) + 1 for ln in bufs["M"].split(b"\n")[:-1]) == 700
    return {k: (b, _tensor(b)) for k, b in bufs.items()}


@pytest.mark.parametrize("name,expr,tau", [("pat20", PAT20, 3), ("pat40", PAT40, 5), ("sweep42", SWEEP42, 15)])
def test_a_wrong_line_hint_changes_the_plan_not_the_answer(gpu, capi, memo, pattern, hint_texts, name, expr, tau):
    """Hints of 1 byte .. 1 MB per line on reads, on lines of 259 .. 700 bytes (both planner thresholds, 260 and 600, inside) and on reads
    around lines of 40 .. 120 KB: avg_line decides use_fused, stream_ll, pair_ll, use_myers, can_sub and leaders (seeq_plan.h), the device
    notices what the plan cannot serve and the re-run policy recovers -- the result is the oracle's whatever the hint, and for some
    (text, hint) the kernel or the number of runs is not that of the sampled line length."""
    from seeq_amd import device as dev
    pat = pattern(expr, tau)
    seen = {}
    for tname, (buf, t) in hint_texts.items():
        assert len(memo.buffer_scan(expr, tau, buf, SQ_ALL)["records"]) > 50, tname
        for hint in HINTS:
            def make(hint=hint):
                s = dev.Scanner()
                if hint:
                    s.set_line_hint(hint)
                return s
            sc = make()
            for mode, want in ((SQ_BEST, dev.WANT_RECORDS), (SQ_ALL, dev.WANT_RECORDS), (0, dev.WANT_COUNTLINES)):
                _plain(memo, sc, "%s, text %s, hint %g, mode %d want %d" % (name, tname, hint, mode, want), pat, expr, tau, t, buf, mode, want, fresh=make)
                seen.setdefault((tname, hint), []).append((sc.last_kernel(), sc.last_runs()))
            sc.close()
    for key in sorted(seen, key=str):
        print(name, key, seen[key])
    assert any(seen[tname, hint] != seen[tname, 0] for tname in hint_texts for hint in HINTS[1:]), seen      # (not vacuous: a wrong hint showed)


# =====================================================================================================================
# 2. a resident buffer refilled in place
# =====================================================================================================================
RESIDENT_BYTES = 512 * 1024
REFILL_PLANTS = [(PAT20, 3), (MER8, 1)]


@pytest.fixture(scope="module")
def fillings():
    """The seven fillings, each exactly RESIDENT_BYTES long: (name, buffer, option bits, fasta, fastq_of)."""
    N = RESIDENT_BYTES
    reads = _read_lines(81, 4000, REFILL_PLANTS)
    _, b_reads = _fit(reads, N, 1)
    _, b_long = _fit(_long_text(82, REFILL_PLANTS, nreads=900), N, 2)
    fa = []
    for i, ln in enumerate(_read_lines(83, 4000, REFILL_PLANTS)):
        fa += [">read%d %s" % (i, PAT20), ln]
    _, b_fasta = _fit(fa, N, 3, group=2)
    dirty, _ = _fit(_read_lines(84, 4000, REFILL_PLANTS), N, 4)
    b_convert = _foreign(_buf(dirty), 85, ord("X"))
    b_ignore = _foreign(_buf(dirty), 85, ord("-"))
    raw, b_fastq = _fit(_fastq(_read_lines(86, 2000, REFILL_PLANTS), PAT20), N, 6, group=4)
    seqs = raw[1::4]
    _, b_again = _fit(_read_lines(87, 4000, REFILL_PLANTS), N, 7)
    out = [("reads", b_reads, 0, False, None), ("long lines", b_long, 0, False, None), ("fasta", b_fasta, 0, True, None),
           ("convert", b_convert, SQ_CONVERT, False, None), ("ignore", b_ignore, SQ_IGNORE, False, None),
           ("fastq", b_fastq, 0, False, _fastq_of(seqs, b_fastq)), ("reads again", b_again, 0, False, None)]
    assert len(raw) % 4 == 0 and all(len(f[1]) == N for f in out)
    return out


def test_a_resident_buffer_refilled_in_place(gpu, capi, memo, pattern, fillings):
    """One tensor, one Scanner, no line hint: the same (pointer, size) holds reads, long lines, FASTA, foreign bytes, FASTQ in turn, so
    the context plans up to 63 scans with the statistics of an earlier text (scan_setup samples again only after 64 scans) and carries
    the fall-back flags of the texts before.  Plain scans (SQ_BEST, SQ_ALL) and both strands (two scans for the 20-mer, one walk for the
    barcode) after every refill, twice round; at least one step after a refill needed a re-run."""
    import torch
    from seeq_amd import device as dev
    t = torch.zeros(RESIDENT_BYTES, dtype=torch.uint8, device="cuda")
    ptr, nbytes = t.data_ptr(), t.numel()
    sc = dev.Scanner()
    p20, p8 = pattern(PAT20, 3), pattern(MER8, 1)
    reruns = []
    for rnd in range(2):
        for name, buf, nd, fasta, fq in fillings:
            t.copy_(torch.frombuffer(bytearray(buf), dtype=torch.uint8))
            torch.cuda.synchronize()
            assert t.data_ptr() == ptr and t.numel() == nbytes == len(buf)
            what = "round %d, %s" % (rnd, name)
            for mode in (SQ_BEST, SQ_ALL):
                _plain(memo, sc, what + ", plain mode %d" % mode, p20, PAT20, 3, t, buf, mode | nd, dev.WANT_RECORDS, fasta, fq)
                reruns.append((rnd, name, sc.last_runs(), sc.last_kernel(), sc.fallback()))
            _strands(memo, sc, what + ", strands of the 20-mer", p20, PAT20, 3, t, buf, SQ_ALL | nd, dev.WANT_RECORDS, fasta, fq)
            reruns.append((rnd, name, sc.last_runs(), sc.last_kernel(), sc.fallback()))
            _strands(memo, sc, what + ", strands of the barcode", p8, MER8, 1, t, buf, SQ_ALL | nd, dev.WANT_RECORDS, fasta, fq)
            reruns.append((rnd, name, sc.last_runs(), sc.last_kernel(), sc.fallback()))
    sc.close()
    for r in reruns:
        print(r)
    assert any(runs > 1 for rnd, name, runs, kernel, fb in reruns if (rnd, name) != (0, "reads")), reruns      # the stale sample at work


# =====================================================================================================================
# 3. fall-back memory and its expiry
# =====================================================================================================================
def _seam_lines(lines, clean):
    """clean: every line that holds a byte k * SEG is made of N (no candidate on it, whatever the pattern); else: such a line gets an
    exact copy of PAT20 on either side of the seam, which is moved to the middle of the line by a longer first line."""
    out = list(lines)
    if not clean:
        out[0] = out[0] + "ACGT" * 19                      # 151 * 434 + 76 = 65 610: the seam falls at column 77 of a 150-base line
    pos = 0
    for i, ln in enumerate(out):
        end = pos + len(ln)                                # the line's newline
        k = (end // SEG) * SEG
        if k > pos and k <= end and i:
            if clean:
                out[i] = "N" * len(ln)
            else:
                col = k - pos
                assert 30 <= col <= len(ln) - 30, (i, col)
                out[i] = ln[:col - 25] + PAT20 + ln[col - 5:col + 5] + PAT20 + ln[col + 25:]
                assert len(out[i]) == len(ln)
        pos = end + 1
    return out


def _trigger(case):
    """-> (trigger buffer, option bits, the bit, environment, pattern)."""
    from seeq_amd import device as dev
    plants = [(PAT20, 3)]
    if case == "long_lines":
        # reads (the sample: read-length kernels) with one line of four tiles that has hits: a candidate in a tile without a newline
        reads = _read_lines(91, 2000, plants)
        lines = reads[:1200] + [_long_line(random.Random(92), 4 * TILE, plants)] + reads[1200:]
        return _buf(lines), 0, dev.FALLBACK_LONG_LINES, {}, (PAT20, 3)
    if case == "nondna":
        # FASTQ records scanned as plain lines under SQ_IGNORE, with a 6-mer that k_stream's skipping variant serves (the 20-mer's k_pair
        # verifies its candidates anyway and never asks): quality lines of skipped bytes between bases, most of their hit lines made up
        rng = random.Random(93)
        raw = []
        for i, sq in enumerate(_read_lines(94, 800, plants)):
            raw += ["@read.%d/1" % i, sq, "+", "".join(rng.choice("ACGIIIIFFFF#,:") for _ in sq)]
        return _buf(raw), SQ_IGNORE, dev.FALLBACK_NONDNA, {}, ("GAATTC", 1)
    # read-length lines; the lines across the 64 KiB seams hold the pattern on both sides of them
    return _buf(_seam_lines(_read_lines(95, 3000, plants), clean=False)), 0, dev.FALLBACK_SEAM, {"SEEQ_SEGMENT_BYTES": str(SEG)}, (PAT20, 3)


@pytest.mark.parametrize("case", ["long_lines", "nondna", "seam"])
def test_fallback_flags_are_kept_for_32_scans_and_dropped(gpu, capi, memo, pattern, case, monkeypatch):
    """A text raises a fall-back flag (its scan needs a re-run); the next SEEQ_RERUN_TTL = 32 scans -- clean read texts of four sizes, each
    sampled afresh -- are planned with it and answer as the oracle; the flag is there after scan 31, gone after scan 33, and then the
    kernel is the one a fresh context chooses; the trigger text needs its re-run again."""
    from seeq_amd import device as dev
    trig, nd, bit, env, (expr, tau) = _trigger(case)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pat = pattern(expr, tau)
    clean = [_buf(_seam_lines(_read_lines(96 + i, 2000 + 300 * i, [(PAT20, 3)]), clean=True)) for i in range(4)]
    if case == "seam":
        assert all(len(b) > 4 * SEG for b in clean + [trig])
    t_trig, t_clean = _tensor(trig), [_tensor(b) for b in clean]
    sc = dev.Scanner()
    assert sc.fallback() == (0, 0) and sc.last_runs() == 0

    def scan(i, t, buf):
        _plain(memo, sc, "%s, scan %s" % (case, i), pat, expr, tau, t, buf, (SQ_ALL if i == "trigger" or i % 2 else SQ_BEST) | nd, dev.WANT_RECORDS)

    scan("trigger", t_trig, trig)
    print(case, "trigger:", sc.last_kernel(), "runs", sc.last_runs(), "fallback", sc.fallback())
    assert sc.last_runs() > 1
    bits, left = sc.fallback()
    assert bits & bit and left == 32, (bits, left)
    history = {}
    for i in range(1, 37):
        scan(i, t_clean[i % 4], clean[i % 4])
        history[i] = (sc.fallback(), sc.last_kernel(), sc.last_runs())
    print(case, {i: history[i] for i in (1, 2, 30, 31, 32, 33, 34, 35, 36)})
    assert history[31][0][0] & bit and history[31][0][1] == 1, history[31]
    assert history[33][0] == (0, 0), history[33]
    assert all(history[i][0][0] & bit for i in range(1, 32)) and all(history[i][0] == (0, 0) for i in range(33, 37))
    for i in range(33, 37):                                # after expiry: the kernel of a fresh context, in one run
        fresh = dev.Scanner()
        fresh.scan_tensor(pat, t_clean[i % 4], (SQ_ALL if i % 2 else SQ_BEST) | nd, dev.WANT_RECORDS)
        assert (history[i][1], history[i][2]) == (fresh.last_kernel(), fresh.last_runs()), (i, history[i], fresh.last_kernel(), fresh.last_runs())
        fresh.close()
    scan("trigger", t_trig, trig)
    assert sc.last_runs() > 1
    bits, left = sc.fallback()
    assert bits & bit and left == 32, (bits, left)
    sc.close()


# =====================================================================================================================
# 4. every kind of call on one context, in different orders
# =====================================================================================================================
MULTI3 = [("ACGTTGCA", 1), ("TTGACCGA", 1), ("CAGTGTCA", 2)]
DEMUX_B = ["GGCATTAC", "ATATCGCG", "GATTACAG", "ACGTTGCA", "TTGACCGA"]
DEMUX_B_TAUS = [1, 0, 1, 1, 1]


class Calls:
    """The texts (resident), the patterns and the eleven steps."""

    def __init__(self, memo, pattern):
        import torch
        from seeq_amd import device as dev
        self.memo, self.pattern = memo, pattern
        self.bar = _buf(strand_lines(MER8, 1, n=3000, seed=41))
        self.p20 = _buf(strand_lines(PAT20, 3, n=3000, seed=42))
        self.mix = _buf(_mixed_lines(BARCODES, TAUS, n=3000, seed=43))
        seqs = strand_lines(MER8, 1, n=750, seed=44, lengths=(75, 100, 101))
        self.fq = _buf(_fastq(seqs, MER8))
        self.fq_of = _fastq_of(seqs, self.fq)
        self.packed_text = _buf(_read_lines(45, 3000, [(PAT20, 3)], nbase=True))
        bases, nmask, self.nreads = dev.pack_reads(self.packed_text, 150)
        self.pb, self.pn = torch.from_numpy(bases.copy()).cuda(), torch.from_numpy(nmask.copy()).cuda()
        rng = random.Random(46)
        s = _dna(rng, 2048)
        _plant(rng, s, [(PAT20, 3)], 6, both_strands=False)
        self.str2k = "".join(s)[:2048]
        self.t = {k: _tensor(getattr(self, k)) for k in ("bar", "p20", "mix", "fq")}
        self.set8 = [pattern(b, t) for b, t in zip(BARCODES, TAUS)]
        self.set5 = [pattern(b, t) for b, t in zip(DEMUX_B, DEMUX_B_TAUS)]
        self.set3 = [pattern(b, t) for b, t in MULTI3]

    def need_records(self):
        """The largest number of records one call wants in the record workspace: a call's total, or for a one walk its largest
        pattern's share times the patterns."""
        m, need = self.memo, 0
        for exprs, taus, buf, mode in ((BARCODES, TAUS, self.mix, SQ_BEST), (DEMUX_B, DEMUX_B_TAUS, self.mix, SQ_BEST),
                                       ([b for b, _ in MULTI3], [t for _, t in MULTI3], self.mix, SQ_ALL)):
            per = [len(m.buffer_scan(b, t, buf, mode)["records"]) for b, t in zip(exprs, taus)]
            need = max(need, max(per) * len(per), sum(per))
        for expr, tau, buf in ((MER8, 1, self.bar), (PAT20, 3, self.p20), (MER8, 1, self.fq)):
            e = m.strands(expr, tau, buf, SQ_ALL)
            need = max(need, len(e.rows), 2 * max(len(e.plus), len(e.minus)))
        return max(need, len(m.buffer_scan(PAT20, 3, self.packed_text, SQ_ALL)["records"]))

    # -- the steps: step(sc, what) --
    def strands_barcode(self, sc, what):
        from seeq_amd import device as dev
        _strands(self.memo, sc, what, self.pattern(MER8, 1), MER8, 1, self.t["bar"], self.bar, SQ_ALL, dev.WANT_RECORDS)

    def plain_best(self, sc, what):
        from seeq_amd import device as dev
        _plain(self.memo, sc, what, self.pattern(PAT20, 3), PAT20, 3, self.t["p20"], self.p20, SQ_BEST, dev.WANT_RECORDS)

    def _demux(self, sc, what, pats, exprs, taus):
        exp = self.memo.demux(exprs, taus, self.mix)
        _step(sc, what, lambda s: s.demux_tensor(pats, self.t["mix"]), lambda s, res: demux_check(res, exp))

    def demux8(self, sc, what):
        self._demux(sc, what, self.set8, BARCODES, TAUS)

    def fastq_all(self, sc, what):
        from seeq_amd import device as dev
        _plain(self.memo, sc, what, self.pattern(MER8, 1), MER8, 1, self.t["fq"], self.fq, SQ_ALL, dev.WANT_RECORDS, fastq_of=self.fq_of)

    def strands_fastq(self, sc, what):
        from seeq_amd import device as dev
        _strands(self.memo, sc, what, self.pattern(MER8, 1), MER8, 1, self.t["fq"], self.fq, SQ_BEST, dev.WANT_RECORDS, fastq_of=self.fq_of)

    def packed(self, sc, what):
        from seeq_amd import device as dev
        exp = self.memo.buffer_scan(PAT20, 3, self.packed_text, SQ_ALL)

        def call(s):
            s.run_packed(self.pattern(PAT20, 3), self.pb.data_ptr(), self.pn.data_ptr(), self.nreads, 150, options=SQ_ALL, want=dev.WANT_RECORDS)
            return s.fetch()

        def check(s, res):
            assert (res["nlines"], res["nmatchlines"], res["nrecords"]) == (exp["nlines"], exp["nmatchlines"], len(exp["records"]))
            assert np.array_equal(s.records(res["nrecords"]).astype(np.uint64), exp["records"])
        _step(sc, what, call, check)

    def multi3(self, sc, what):
        from seeq_amd import device as dev
        exps = [self.memo.buffer_scan(b, t, self.mix, SQ_ALL) for b, t in MULTI3]

        def check(s, got):
            for g, e in zip(got, exps):
                assert (g["nlines"], g["nmatchlines"], g["nrecords"]) == (e["nlines"], e["nmatchlines"], len(e["records"]))
                assert np.array_equal(g["records"].astype(np.uint64), e["records"])
        _step(sc, what, lambda s: s.scan_tensor_multi(self.set3, self.t["mix"], SQ_ALL, dev.WANT_RECORDS), check)

    def string_match(self, sc, what):
        from seeq_amd import _capi
        exp = [(1, s, e, d) for s, e, d in reversed(self.memo.oracle.string_match(PAT20, 3, self.str2k, SQ_ALL))]
        assert len(exp) >= 4
        data = self.str2k.encode()

        def call(s):
            rec, nrec = C.POINTER(_capi.seeqdev_hit_t)(), C.c_size_t()
            rc = _capi.lib().seeqdevStringMatch(C.c_void_p(s._h), C.c_void_p(self.pattern(PAT20, 3).handle), C.c_char_p(data), C.c_size_t(len(data)),
                                                C.c_int(SQ_ALL), C.byref(rec), C.byref(nrec))
            assert rc == 0, _capi.error_text()
            return [(rec[i].line, rec[i].start, rec[i].end, rec[i].dist) for i in range(nrec.value)]

        def check(s, got):
            assert got == exp
        _step(sc, what, call, check)

    def strands_two_scans(self, sc, what):
        from seeq_amd import device as dev
        _strands(self.memo, sc, what, self.pattern(PAT20, 3), PAT20, 3, self.t["p20"], self.p20, SQ_ALL, dev.WANT_RECORDS)
        assert not sc.last_multi_one_pass()

    def plain_countmatch(self, sc, what):
        from seeq_amd import device as dev
        _plain(self.memo, sc, what, self.pattern(PAT20, 3), PAT20, 3, self.t["p20"], self.p20, 0, dev.WANT_COUNTMATCH)

    def demux5(self, sc, what):
        self._demux(sc, what, self.set5, DEMUX_B, DEMUX_B_TAUS)

    def steps(self):
        return [self.strands_barcode, self.plain_best, self.demux8, self.fastq_all, self.strands_fastq, self.packed, self.multi3, self.string_match,
                self.strands_two_scans, self.plain_countmatch, self.demux5]


@pytest.fixture(scope="module")
def calls(memo, pattern):
    return Calls(memo, pattern)


@pytest.mark.parametrize("reservation", ["none", "tiny", "odd"])
def test_every_kind_of_call_on_one_context(gpu, capi, calls, reservation):
    """Strands (one walk, two scans, FASTQ), plain scans, demultiplexing of two sets, SEEQDEV_FASTQ, a packed batch, a multi scan and a
    string match share one context -- its record arrays cut into cap / npat regions, grown by strands_merge, followed by the FASTQ
    scratch, its one multi-plan slot -- forwards twice on one Scanner, backwards on another; without a reservation, with one that makes
    every capacity overflow (and switches the optimistic first reservation off for good), and with an odd record capacity that no
    number of patterns divides.  The second forward round scans a plain text after every packed, strands and demux step: no strand bit,
    the oracle's records."""
    from seeq_amd import device as dev
    steps = calls.steps()
    mixed_after = {"strands_barcode", "demux8", "strands_fastq", "packed", "strands_two_scans", "demux5"}

    def make():
        sc = dev.Scanner()
        if reservation == "tiny":
            sc.reserve(0, 10, 2, 1)
        elif reservation == "odd":
            sc.reserve(0, 4097, 8192 * 64 + 1, 2 * calls.need_records() + 1)
        return sc

    sc = make()
    reran = 0
    for rnd in range(2):
        for k, step in enumerate(steps):
            step(sc, "%s reservation, forwards round %d, step %d (%s)" % (reservation, rnd, k + 1, step.__name__))
            reran += sc.last_runs() > 1
            if rnd == 1 and step.__name__ in mixed_after:
                calls.plain_best(sc, "%s reservation, the plain scan after step %d (%s)" % (reservation, k + 1, step.__name__))
    sc.close()
    print(reservation, "steps whose last scan or walk was re-run:", reran)
    if reservation == "tiny":
        assert reran > 0
    sc = make()
    for k, step in reversed(list(enumerate(steps))):
        step(sc, "%s reservation, backwards, step %d (%s)" % (reservation, k + 1, step.__name__))
    calls.plain_best(sc, "%s reservation, the plain scan after the backward pass" % reservation)
    sc.close()
