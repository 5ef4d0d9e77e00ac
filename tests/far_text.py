"""A text whose offsets pass 2^31, the default segment seam and 2^32: how far into its buffer a line lies must not change any answer.  Behind
tests/test_gpu_far_text.py, checked on the CPU by tests/test_far_text_host.py.  Everything here runs on the CPU and never holds the 4 GiB.

Part A, the entries behind the scan.  `Layout` is filler | block | filler | block | filler | block | filler tail: three copies of the chain
text (tests/text_window.py: Chain; the FASTQ view: fastq_window("whole"), the plain view: plain_window(h, True)) between runs of ONE
filler unit -- a valid four-line FASTQ record, or four DNA lines, of READ bases, drawn with a fixed seed and rejected until the oracle finds
nothing in it for FA, FB, FC, FD and their reverse complements at FLANK_TAU under SQ_ALL.  Each gap is one unit of adjusted length (the
FASTQ view: its header line takes the pad; the plain view: its first line, cut from a longer hitless draw) and whole units behind it: the
pad sets the block's phase, the line classes stay what they are.  A block per boundary, in the boundaries' order:
  FASTQ view   B31   a sequence line starts exactly on it;
               SEAM  inside the quality bytes of a guide that passes the gate: the gate's walk starts below it and ends above it, and the
                     record's four lines lie on both sides;
               B32   strictly inside the guide (AB insert) of a record whose guide is tallied and passes the gate;
  plain view   B31   strictly inside an FB occurrence;  SEAM  strictly inside a UMI (CD insert);  B32  strictly inside an FA occurrence.
`Layout.phases()` asserts each on the finished text and says where it fell.  The reference never looks at the far text: `FarRef` is the
`Ref` of tests/test_gpu_text_window.py over the COMPACT text (the three blocks alone), its oracle wrapped (`MappedOracle`) so that every
record's line, and nlines, are those of the far text -- lines are independent and the filler holds no hit, so that is what the oracle would
say (test_far_text_host.py shows it on a scaled layout); `FarOffs` maps a far line to its far offset and `FarBytes` answers len, indexing
and slicing at absolute offsets from the pieces.  Nothing that comes from the device is mapped back.

Part B, the scan kernels far into a segment.  `FarRow` is lead + K x the text of a row of tests/kernel_instance_rows.py: the lead one
hitless line of the row's shape (random bases, N for a pattern that matches nearly everywhere; a header in front of a FASTA row's)
whose length puts B32 strictly inside a record of the period, K the smallest count that reaches B32 plus two periods;
the oracle runs over ONE period and numpy replicates its records and line offsets by per-copy shifts.  FAR_ROWS names the rows.

A plain helper module: no fixtures, no test collection."""
import bisect
import os
import random
import re

import numpy as np

import text_window as W
from oracle.pyoracle import SQ_ALL
from test_gpu_text_window import FLANKS, Ref
from test_qgate_host import PASS
from test_tally_host import OK, py_key

B31, B32 = 1 << 31, 1 << 32
READ = 120                      # bases of a filler line: about what a chain read has
TAIL_MIN = 4096                 # filler behind the last block, at least
ROLES = ("B31", "SEAM", "B32")


def seam():
    """The default segment size of a scan context (seeqdevScanNew in seeq_device.hip)"""
    with open(os.path.join(W.ROOT, "seeq_amd", "csrc", "seeq_device.hip")) as f:
        m = re.search(r"s->seg_bytes\s*=\s*\(size_t\)\s*(0x[0-9A-Fa-f]+)u\s*;", f.read())
    assert m, "seeq_device.hip no longer sets seg_bytes where this looks for it"
    return int(m.group(1), 16)


def true_bounds():
    return dict(B31=B31, SEAM=seam(), B32=B32)


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def hitless_patterns():
    """the patterns the filler is checked for, all at FLANK_TAU: what MappedOracle may be asked"""
    return list(FLANKS.values()) + [revcomp(f) for f in FLANKS.values()]


def no_hit(oracle, buf):
    return all(len(oracle.buffer_scan(p, W.FLANK_TAU, buf, SQ_ALL)["records"]) == 0 for p in hitless_patterns())


# ---- the bytes ----
class FarBytes:
    """A text given by its pieces, in order: bytes, or a count of repeats of `unit`.  len, indexing and slicing (step 1) at ABSOLUTE offsets:
    a bound below 0 is 0, one above the end is the end -- there is no counting from the end.  `starts`: where each piece begins."""

    def __init__(self, pieces, unit):
        self.unit, self.starts, self.pieces = bytes(unit), [], []
        pos = 0
        for p in pieces:
            n = len(p) if isinstance(p, bytes) else p * len(unit)
            if n:
                self.starts.append(pos)
                self.pieces.append(p)
                pos += n
        self.n = pos

    def __len__(self):
        return self.n

    def _cut(self, a, b):
        a, b = max(0, a), min(self.n, b)
        out = []
        i = bisect.bisect_right(self.starts, a) - 1
        U = len(self.unit)
        while a < b:
            s, p = self.starts[i], self.pieces[i]
            hi = min(b, self.starts[i + 1] if i + 1 < len(self.starts) else self.n)
            if isinstance(p, bytes):
                out.append(p[a - s:hi - s])
            else:
                r = (a - s) % U
                out.append((self.unit * ((r + hi - a + U - 1) // U))[r:r + hi - a])
            a = hi
            i += 1
        return b"".join(out)

    def __getitem__(self, k):
        if isinstance(k, slice):
            assert k.step in (None, 1)
            return self._cut(0 if k.start is None else int(k.start), self.n if k.stop is None else int(k.stop))
        k = int(k)
        if not 0 <= k < self.n:
            raise IndexError(k)
        return self._cut(k, k + 1)[0]

    def find(self, sub, start=0, end=None):
        """bytes.find over [start, end): for short ranges (the range is cut out)"""
        start = max(0, start)
        i = self._cut(start, self.n if end is None else end).find(sub)
        return -1 if i < 0 else start + i

    def items(self):
        """(start, piece) in order"""
        return list(zip(self.starts, self.pieces))


# ---- the filler ----
class Filler:
    """unit: the repeated bytes (four lines); adjusted(pad): one unit, pad bytes longer -- the FASTQ view's header takes the pad, the plain
    view's first line is that much more of a hitless draw.  0 <= pad < len(unit)."""

    def __init__(self, oracle, fastq, seed=20261021):
        rng = random.Random(seed + fastq)
        bases = lambda n: bytes(rng.choices(b"ACGT", k=n))      # noqa: E731
        self.fastq = fastq
        for _ in range(64):
            if fastq:
                seq = bases(READ)
                self.unit = b"@f\n" + seq + b"\n+\n" + b"I" * READ + b"\n"
                self.long = None
                probe = seq + b"\n"
            else:
                lines = [bases(READ) for _ in range(4)]
                self.unit = b"".join(ln + b"\n" for ln in lines)
                self.long = lines[0] + bases(len(self.unit))
                probe = self.long + b"\n" + self.unit
            if no_hit(oracle, probe):
                break
        else:
            raise AssertionError("no hitless filler unit in 64 draws")
        self.lines = 1 if fastq else 4                          # counted lines of a unit: records, or lines

    def adjusted(self, pad):
        assert 0 <= pad < len(self.unit)
        if self.fastq:
            return b"@f" + b"p" * pad + self.unit[2:]
        return self.long[:READ + pad] + self.unit[READ:]


# ---- the layout ----
def _block_candidates(bref, chain, fastq):
    """role -> the block offsets that may lie on the role's boundary, ascending (the rule of each role: the module's docstring)"""
    offs = bref.offs
    if not fastq:
        inside = lambda rows: sorted(offs[r[0]] + (r[1] + r[2]) // 2 for r in rows if r[2] - r[1] >= 2)      # noqa: E731
        return dict(B31=inside(bref.hit_rows("B")), SEAM=inside(bref.rows("CD")), B32=inside(bref.hit_rows("A")))
    rows = bref.rows("AB")
    kinds, _ = bref.gate(rows)
    good = [r for r, k, (_, b) in zip(rows, kinds, bref.spans(rows)) if k == PASS and py_key(b)[0] == OK and r[2] - r[1] >= 2]
    qual = lambda r: offs[r[0]] + len(chain.records[r[0] - 1][1]) + 3      # noqa: E731  (behind the sequence line and "+\n")
    return dict(B31=sorted(offs[r[0]] for r in good), SEAM=sorted(qual(r) + (r[1] + r[2]) // 2 for r in good),
                B32=sorted(offs[r[0]] + (r[1] + r[2]) // 2 for r in good))


class Layout:
    """The far text of one view (fastq: True / False) for `bounds` (role -> offset; default: the true ones).  far: FarBytes; block, nblock
    (its counted lines: records, or lines), order (the roles by offset: block k holds order[k]), block_start[k], shift[k] (counted filler
    lines in front of block k), nlines (of the whole text), compact (the three blocks alone)."""

    def __init__(self, oracle, fastq, bounds=None, chain=None, h=None):
        self.fastq, self.bounds = fastq, dict(bounds or true_bounds())
        assert sorted(self.bounds) == sorted(ROLES)
        self.chain = chain = chain or W.Chain()
        if fastq:
            self.block = chain.fastq_window("whole")[0]
        else:
            def hits(buf):
                e = oracle.buffer_scan(W.FA, W.FLANK_TAU, buf, SQ_ALL)
                return W.abs_hits(e["records"], W.line_offsets(buf))
            self.block = chain.plain_window(h or W.hostile_for(hits, W.FA), True)
        S = len(self.block)
        self.fill = fill = Filler(oracle, fastq)
        U = len(fill.unit)
        self.bref = bref = Ref(oracle, self.block, fastq)
        self.nblock = len(bref.offs) - 1
        self.order = sorted(ROLES, key=self.bounds.get)
        phase = self._phases_for(_block_candidates(bref, chain, fastq), S, U)
        pieces, pos, lines = [], 0, 0
        self.block_start, self.shift, self.gaps = [], [], []
        for role in self.order:
            start = self.bounds[role] - phase[role]
            n, pad = divmod(start - pos, U)
            assert n >= 1, (role, start, pos)
            pieces += [fill.adjusted(pad), n - 1, self.block]
            lines += n * fill.lines
            self.gaps.append((pos, pad, n - 1))
            self.block_start.append(start)
            self.shift.append(lines)
            pos = start + S
        ntail = -(-TAIL_MIN // U)
        pieces.append(ntail)
        self.far = FarBytes(pieces, fill.unit)
        self.nlines = 3 * self.nblock + lines + ntail * fill.lines
        self.compact = self.block * 3
        assert len(self.far) == pos + ntail * U and len(self.far) - pos >= TAIL_MIN
        for k, start in enumerate(self.block_start):
            assert self.far[start:start + 64] == self.block[:64] and self.far[start - 1] == 10

    def _phases_for(self, cands, S, U):
        """role -> block offset: per role up to nine candidates spread over the block; of the choices that leave every gap at least one
        unit, the one whose boundaries lie nearest the blocks' middles"""
        some = {}
        for role in ROLES:
            c = cands[role]
            assert c, "no candidate for " + role
            some[role] = sorted({min(c, key=lambda p: abs(p - S * q // 10)) for q in range(1, 10)})
        best = None
        a, b, c = self.order
        for pa in some[a]:
            for pb in some[b]:
                for pc in some[c]:
                    s = [self.bounds[a] - pa, self.bounds[b] - pb, self.bounds[c] - pc]
                    if s[0] >= U and s[1] >= s[0] + S + U and s[2] >= s[1] + S + U:
                        cost = sum(abs(2 * p - S) for p in (pa, pb, pc))
                        if best is None or cost < best[0]:
                            best = (cost, {a: pa, b: pb, c: pc})
        assert best, "the boundaries %s leave no room for three blocks of %d bytes" % (self.bounds, S)
        return best[1]

    # -- compact -> far --
    def block_of(self, line):
        """0-based block of a compact counted line (1-based)"""
        assert 1 <= line <= 3 * self.nblock, line
        return (line - 1) // self.nblock

    def far_line(self, line):
        return line + self.shift[self.block_of(line)]

    def map_records(self, records):
        """oracle records [n, 4] over the compact text -> the same over the far text: lines shifted by their block's filler lines"""
        out = np.array(records, dtype=np.uint64).reshape(-1, 4)
        if len(out):
            k = (out[:, 0].astype(np.int64) - 1) // self.nblock
            assert k.min() >= 0 and k.max() <= 2
            out[:, 0] += np.array(self.shift, dtype=np.uint64)[k]
        return out

    def far_block(self, line):
        """(block, 1-based line in it) of a FAR counted line; KeyError for a filler line"""
        for k in range(3):
            first = self.shift[k] + k * self.nblock + 1
            if first <= line < first + self.nblock:
                return k, line - first + 1
        raise KeyError("line %d of the far text is a filler line" % line)

    # -- the phases --
    def phases(self, ref):
        """Asserts what each boundary cuts, with the far reference `ref` (FarRef) -> [one line of text per boundary]"""
        out = []
        offs, far = ref.offs, self.far
        self.cut = {}                                               # role -> the reference's row that the boundary cuts

        def cut(rows, B, base=lambda r: offs[r[0]]):
            return [r for r in rows if base(r) + r[1] < B < base(r) + r[2]]
        for role in ROLES:
            B = self.bounds[role]
            k = self.order.index(role)
            assert self.block_start[k] < B < self.block_start[k] + len(self.block)
            where = "%s = %#x, block %d + %d" % (role, B, k + 1, B - self.block_start[k])
            if self.fastq:
                rows = ref.rows("AB")
                kinds, _ = ref.gate(rows)
                good = [r for r, kd, (_, b) in zip(rows, kinds, ref.spans(rows)) if kd == PASS and py_key(b)[0] == OK]
                if role == "B32":
                    (r,) = cut(good, B)
                    self.cut[role] = r
                    out.append("%s: inside the guide [%d, %d) of record %d, tallied, gate PASS" % (where, r[1], r[2], r[0]))
                elif role == "SEAM":
                    def qual(r):
                        e1 = far.find(b"\n", offs[r[0]], offs[r[0]] + 1024)
                        return far.find(b"\n", e1 + 1, e1 + 1024) + 1
                    (r,) = cut(good, B, qual)
                    self.cut[role] = r
                    off = offs[r[0]]
                    before = far[off - 256:off - 1]                                  # (the header line ends at off - 1)
                    head = off - 1 - len(before) + before.rfind(b"\n") + 1
                    end = far.find(b"\n", qual(r), qual(r) + 1024)
                    assert far[head] == ord("@") and far[head - 1] == 10 and head < off < B < end
                    assert end - qual(r) == far.find(b"\n", off, off + 1024) - off      # (a quality byte per base)
                    out.append("%s: inside the quality bytes of the guide [%d, %d) of record %d, gate PASS; its four lines are [%#x, %#x]"
                               % (where, r[1], r[2], r[0], head, end))
                else:
                    rs = [r for r in good if offs[r[0]] == B]
                    assert len(rs) == 1 and far[B - 1] == 10
                    self.cut[role] = rs[0]
                    out.append("%s: the sequence line of record %d starts on it" % (where, rs[0][0]))
            else:
                what, rows = dict(B32=("an FA occurrence", ref.hit_rows("A")), SEAM=("a UMI (CD insert)", ref.rows("CD")),
                                  B31=("an FB occurrence", ref.hit_rows("B")))[role]
                (r,) = cut(rows, B)
                self.cut[role] = r
                out.append("%s: inside %s [%d, %d) of line %d" % (where, what, r[1], r[2], r[0]))
        return out


class FarOffs:
    """far counted line (1-based) -> the offset of its first byte in the far text; a filler line is a KeyError: nothing is found there"""

    def __init__(self, layout):
        self.layout, self.block_offs = layout, layout.bref.offs

    def __getitem__(self, line):
        k, i = self.layout.far_block(int(line))
        return self.layout.block_start[k] + self.block_offs[i]


class MappedOracle:
    """buffer_scan over the compact text, answered for the far text: the records' lines shifted, nlines the far text's.  Only for the
    patterns the filler was checked for -- for those the filler adds lines and nothing else."""

    def __init__(self, oracle, layout, seq):
        self.oracle, self.layout, self.seq = oracle, layout, seq
        self.known = set(hitless_patterns())

    def buffer_scan(self, pattern, tau, buf, options=0, fasta=False):
        assert buf is self.seq and not fasta and tau == W.FLANK_TAU and pattern in self.known, (pattern, tau)
        e = self.oracle.buffer_scan(pattern, tau, buf, options)
        assert e["nlines"] == 3 * self.layout.nblock
        return dict(records=self.layout.map_records(e["records"]), nlines=self.layout.nlines, nmatchlines=e["nmatchlines"])


class FarRef(Ref):
    """Ref (tests/test_gpu_text_window.py) of the far text: the oracle over the compact text, mapped forward; the bytes from FarBytes"""

    def __init__(self, oracle, layout):
        self.window, self.fastq, self.memo, self.layout = layout.far, layout.fastq, {}, layout
        self.seq = W.fastq_seq(layout.compact)[0] if layout.fastq else layout.compact
        self.oracle = MappedOracle(oracle, layout, self.seq)
        self.offs = FarOffs(layout)


# ---- Part B: a ledger row's text, repeated ----
FAR_ROWS = (
    "k_pair<4,plain> | order2 | k_verify<1,ALL,vr?>",
    "k_pair<7,FA> | order2 | k_verify<2,BEST,vr?>+k_emit1",
    "k_pair<6,IG> | order2 | k_exact1<COUNT,2,-1,-> | k_exact1<EMIT,2,BEST,->",
    "k_pair<4,LL> | k_stream_reorder+k_stream_bounds+leaders(best) | k_exact1<COUNT,2,-1,WK>+k_lead_check+k_lead_best | k_exact1<EMIT,2,BEST,WK>",
    "k_pair<4,LL> | k_stream_reorder+k_stream_bounds | k_exact1<COUNT,1,-1,WK>",
    "k_stream<6,-,-,0> | order2 | k_verify<2,BEST,vr512>+k_emit1",
    "k_stream<8,FA,-,0> | order2 | k_verify<2,ALL,vr512>+k_emit_all<2>",
    "k_stream<4,FA,-,0> | order2 | k_verify<1,ALL,vr512>",
    "k_stream<4,-,LL,0>+ll_filter1 | k_stream_reorder+k_stream_bounds+leaders(best) | k_exact1<COUNT,2,-1,WK>+k_lead_check+k_lead_best | k_exact1<EMIT,2,BEST,WK>",
    "k_stream<4,FA,LL,0>+ll_filter2 | k_stream_reorder+k_stream_bounds+leaders(best) | k_exact1<COUNT,1,-1,WK>+k_lead_check+k_lead_best | k_exact1<EMIT,1,BEST,WK>",
    "k_stream<8,-,LL,1> | k_stream_reorder+k_stream_bounds+leaders | k_exact1<COUNT,1,-1,WK>+k_lead_check+k_lead_lines",
    "k_stream<16,-,LL,0,MY1> | k_stream_reorder+k_stream_bounds+leaders(best) | k_exact1<COUNT,1,-1,WK>+k_lead_check+k_lead_best | k_exact1<EMIT,1,BEST,WK>",
    "k_stream<32,-,LL,0,MY2> | k_stream_reorder+k_stream_bounds+leaders(best) | k_exact1<COUNT,2,-1,WK>+k_lead_check+k_lead_best | k_exact1<EMIT,2,BEST,WK>",
    "k_stream<16,FA,LL,0,MY2> | k_stream_reorder+k_stream_bounds+leaders(best) | k_exact1<COUNT,2,-1,WK>+k_lead_check+k_lead_best | k_exact1<EMIT,2,BEST,WK>",
    "k_direct<4,1> | k_fused_reorder | k_exact1<COUNT,1,-1,->",
    "k_direct<4,1> | no post-pass",
    "k_forward | k_compact | k_exact<W,COUNT> | k_exact<W,EMIT>+k_rec_offsets",
)
MAX_FAR_RECORDS = 10000000
LEAD_MAX, LEAD_MAX_LONG = 2048, 65536


def far_rows():
    """the rows of FAR_ROWS, in that order (tests/kernel_instances.py: Row)"""
    import kernel_instances as K
    by_key = {r.key: r for r in K.rows()}
    return [by_key[k] for k in FAR_ROWS]


# what the list has to cover: a name -> what a row's (key, recipe, want name) must satisfy; `scan` is the key's first part
def _scan(key):
    return key.split(" | ")[0]


COVERAGE = {
    "k_pair on reads": lambda k, rec, w: _scan(k).startswith("k_pair<") and _scan(k).endswith(",plain>") and rec == "reads",
    "k_pair, FASTA": lambda k, rec, w: _scan(k).startswith("k_pair<") and _scan(k).endswith(",FA>"),
    "k_pair, SQ_IGNORE": lambda k, rec, w: _scan(k).startswith("k_pair<") and _scan(k).endswith(",IG>"),
    "k_pair, long lines with leaders": lambda k, rec, w: _scan(k).startswith("k_pair<") and _scan(k).endswith(",LL>") and "+leaders" in k,
    "k_pair, long lines without leaders": lambda k, rec, w: _scan(k).startswith("k_pair<") and _scan(k).endswith(",LL>") and "+leaders" not in k,
    "k_stream, the table on reads": lambda k, rec, w: _scan(k).startswith("k_stream<") and "MY" not in _scan(k) and ",FA," not in _scan(k) and rec == "reads",
    "k_stream, FASTA": lambda k, rec, w: _scan(k).startswith("k_stream<") and "MY" not in _scan(k) and ",FA," in _scan(k),
    "k_stream, the long-line filter": lambda k, rec, w: "+ll_filter" in _scan(k),
    "k_stream, long-N": lambda k, rec, w: _scan(k).startswith("k_stream<") and rec == "long-N",
    "Myers, one word": lambda k, rec, w: _scan(k).endswith(",MY1>"),
    "Myers, two words": lambda k, rec, w: _scan(k).endswith(",MY2>"),
    "k_direct with k_exact1": lambda k, rec, w: _scan(k).startswith("k_direct<") and "k_exact1<" in k,
    "k_direct with no post-pass": lambda k, rec, w: _scan(k).startswith("k_direct<") and k.endswith("| no post-pass"),
    "k_forward with k_rec_offsets": lambda k, rec, w: _scan(k) == "k_forward" and "k_rec_offsets" in k,
    "k_verify, W = 1": lambda k, rec, w: "k_verify<1," in k,
    "k_verify, W = 2": lambda k, rec, w: "k_verify<2," in k,
    "k_exact1, COUNT": lambda k, rec, w: "k_exact1<COUNT," in k,
    "k_exact1, EMIT": lambda k, rec, w: "k_exact1<EMIT," in k,
    "k_exact1, the window walk": lambda k, rec, w: ",WK>" in k,
    "k_exact": lambda k, rec, w: "k_exact<W," in k,
    "k_emit1": lambda k, rec, w: "+k_emit1" in k,
    "k_emit_all": lambda k, rec, w: "+k_emit_all<" in k,
    "WANT_COUNTLINES": lambda k, rec, w: w == "COUNTLINES",
    "WANT_COUNTMATCH": lambda k, rec, w: w == "COUNTMATCH",
    "WANT_RECORDS": lambda k, rec, w: w == "RECORDS",
}


def uncovered(rows):
    import kernel_instances as K
    return [name for name, pred in COVERAGE.items() if not any(pred(r.key, r.recipe, K.WANT_NAMES[r.want]) for r in rows)]


class FarRow:
    """lead + K x period for a ledger row and the boundary b32.  period, P, lead (bytes: one counted line), K, nbytes; exp / exp_all: the
    oracle over ONE period under the row's mode / SQ_ALL; nper: counted lines of a period; hit: the SQ_ALL record of the period that b32
    cuts, copy: which repeat it is in."""

    def __init__(self, row, oracle, b32=B32, plan=None):
        import kernel_instances as K
        self.row = row
        plan = plan or row.plan()
        self.period = period = row.text(plan).buf
        self.P = P = len(period)
        assert period.endswith(b"\n")
        nd = row.options & 0x0C
        self.mode = (row.options & 3) if row.want == K.RECORDS else K.SQ_ALL
        self.exp_all = oracle.buffer_scan(row.pattern, row.tau, period, K.SQ_ALL | nd, fasta=row.fasta)
        self.exp = self.exp_all if self.mode == K.SQ_ALL else oracle.buffer_scan(row.pattern, row.tau, period, self.mode | nd, fasta=row.fasta)
        self.offs = np.array(W.line_offsets(period, row.fasta), dtype=np.uint64)
        self.nper = self.exp["nlines"]
        assert self.nper == len(self.offs) - 1
        # the lead: of the lengths that put b32 strictly inside a record of some repeat, the one nearest the row's line length
        # (records lie some hundred bytes apart -- in the long-line texts some thousand --, so the lengths that will do come in runs that
        # far apart: up to LEAD_MAX, or LEAD_MAX_LONG in a text with lines of 40 to 150 KB, is still a line of the text's kind)
        want = int(row.avg_line) if row.avg_line < 1000 else 500
        most = LEAD_MAX_LONG if row.recipe.startswith("long") else LEAD_MAX
        best = None
        for ln, s, e, d in self.exp_all["records"].tolist():
            a = int(self.offs[ln])
            for t in range(a + s + 1, a + e):
                lead = (b32 - t) % P
                if 16 <= lead <= most and (best is None or abs(lead - want) < abs(best[0] - want)):
                    best = (lead, (ln, s, e, d), t)
        assert best, "no record of the period can be put across %#x by a lead of 16 ... %d bytes" % (b32, most)
        n, self.hit, t = best
        # of the row's shape: a header in front of a FASTA row's, the period's own alphabet -- random bases, drawn again until the oracle
        # finds nothing in them; N (which matches no pattern position but N) where sixteen draws all hold a hit: the patterns that match
        # nearly everywhere, whose texts are made of N for that reason (kernel_instances.build_text, "long-N")
        head = b">l\n" if row.fasta else b""
        rng = random.Random(n * 31 + P)
        hitless = lambda buf: len(oracle.buffer_scan(row.pattern, row.tau, buf, K.SQ_ALL | nd, fasta=row.fasta)["records"]) == 0      # noqa: E731
        draws = (head + bytes(rng.choices(b"ACGT", k=n - 1 - len(head))) + b"\n" for _ in range(16))
        self.lead = next((d for d in draws if hitless(d)), head + b"N" * (n - 1 - len(head)) + b"\n")
        self.lead_bases = b"N" * 8 not in self.lead
        assert len(self.lead) == n and self.lead.count(b"\n") == 1 + bool(head) and hitless(self.lead), "the lead holds a hit"
        self.K = -(-(b32 + 2 * P - n) // P)
        self.copy = (b32 - n - t) // P
        self.nbytes = n + self.K * P
        start = n + self.copy * P + int(self.offs[self.hit[0]])
        assert start + self.hit[1] < b32 < start + self.hit[2] and 0 <= self.copy < self.K - 1 and self.nbytes >= b32 + 2 * P > self.nbytes - P

    def where(self, b):
        """what lies at offset b: (repeat, offset in the period, 1-based counted line of the period or 0 in a header, offset in that line)"""
        c, r = divmod(b - len(self.lead), self.P)
        ln = int(np.searchsorted(self.offs[1:], r, side="right"))
        return c, r, ln, r - int(self.offs[ln]) if ln else r

    def describe(self):
        """where 2^31 and the seam fall: recorded, not steered"""
        import kernel_instances as K
        a, b = self.where(B31), self.where(seam())
        return ("%s: K %d, lead %d, %d records; 2^31 in repeat %d, line %d + %d; the seam in repeat %d, line %d + %d"
                % (self.row.key, self.K, len(self.lead), self.nrecords() if self.row.want == K.RECORDS else 0, a[0], a[2], a[3], b[0], b[2], b[3]))

    # -- the replicated reference --
    def nlines(self):
        return 1 + self.K * self.nper

    def nmatchlines(self):
        return self.K * self.exp["nmatchlines"]

    def nhits_all(self):
        return self.K * len(self.exp_all["records"])

    def nrecords(self):
        return self.K * len(self.exp["records"])

    def records(self):
        """[K * n, 4] uint32, as the device keeps them: (line, start, end, dist); the line of repeat c is 1 + c * nper further on"""
        rec = self.exp["records"]
        n = len(rec)
        assert self.nlines() < 1 << 32
        out = np.empty((self.K, n, 4), dtype=np.uint32)
        out[:] = rec.astype(np.uint32)[None]
        out[:, :, 0] += (1 + np.arange(self.K, dtype=np.uint64) * self.nper).astype(np.uint32)[:, None]
        return out.reshape(-1, 4)

    def offsets(self):
        """[K * n] uint64: the offset of every record's line"""
        base = self.offs[self.exp["records"][:, 0].astype(np.int64)]
        shift = np.uint64(len(self.lead)) + np.arange(self.K, dtype=np.uint64) * np.uint64(self.P)
        return (shift[:, None] + base[None, :]).reshape(-1)

    def materialise(self):
        """the whole text: for scaled boundaries only"""
        assert self.nbytes < 1 << 26
        return self.lead + self.period * self.K
