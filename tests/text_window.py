"""Where a text lies, what surrounds it and how it is cut into segments must not change any answer: the placements behind
tests/test_gpu_kernel_instances.py (every instance on a hostile window) and tests/test_gpu_text_window.py (the entries behind the scan),
checked on the CPU by tests/test_text_window_host.py.

`place` puts a window into a larger buffer between two guards of at least GUARD bytes each, so that a kernel that does read outside the window
stays inside memory the test owns: these placements detect the USE of outside bytes, they never provoke a fault.  The guards are hostile: their
bytes next to the window are chosen so that a kernel that lets them decide anything gives another answer --
  before      the guard ends, without a newline, in `...\\n<line with an occurrence>\\nP[:k]`; the window's first line begins with P[k:]: a
              look-back sees an occurrence straddling byte 0, a line start taken from before byte 0 shifts starts and offsets;
  after open  the window ends, without a newline, in filler + P[:k]; the guard begins with P[k:] + newline + a line with an occurrence;
  after closed  the window ends in a newline; the guard begins with a complete line that holds an occurrence (nlines, nmatchlines);
  FASTA       the guard ends in `>`: a look-back turns the window's first line, which holds an occurrence, into a header;
  FASTQ       the guard ends, without a newline, in `@g\\nP[:k]` (a line start taken from before byte 0 shifts the records by a line); the
              window ends behind the last sequence line's newline, behind the `+` line, or in the middle of the quality line (the last
              span's own quality bytes inside: the line is shorter than the sequence line, MISFIT) and the guard goes on with a valid record
              of high quality bytes (a gate that reads on says PASS).
`live_*` state, with the oracle or a restated rule on the CPU, that a placement is worth running: the reference over guard tail + window +
guard head differs from the reference over the window alone in the named quantity.  A placement that is not live is a test error.

A plain helper module: no fixtures, no test collection."""
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
# the leads of a window in its buffer: odd ones (residues below 16, around 64 and around 128; in an order that gives neighbouring rows a small
# and a large one), and 16-aligned ones that are not 128-aligned
ODD_LEADS = tuple(GUARD + r for r in (1, 65, 3, 127, 5, 129, 7, 63, 9, 17, 11, 13, 15))


def odd_lead(i):
    return ODD_LEADS[i % len(ODD_LEADS)]


def aligned_lead(i):
    return GUARD + 16 * (1 + i % 7)


def dna_lines(nbytes, seed=0):
    """exactly nbytes of valid DNA lines (60 bases each, the last one shorter), ending in a newline; b"" for 0"""
    rng = random.Random(nbytes * 31 + seed)
    out = bytearray()
    while nbytes - len(out) >= 122:
        out += bytes(rng.choices(b"ACGT", k=60)) + b"\n"
    if nbytes - len(out) > 61:
        out += bytes(rng.choices(b"ACGT", k=40)) + b"\n"
    if nbytes - len(out):
        out += bytes(rng.choices(b"ACGT", k=nbytes - len(out) - 1)) + b"\n"
    assert len(out) == nbytes
    return bytes(out)


def place(window, lead, before=b"", after=b""):
    """-> (big, lo, hi), big[lo:hi] == window and lo == lead: `before` are the bytes right in front of the window, `after` the bytes right
    behind it; both guards are filled up with valid DNA lines, in front of `before` (so `before` starts a line) and behind `after` (which
    ends in a newline, or is empty behind a window that does), to `lead` bytes and to at least GUARD bytes."""
    assert lead >= GUARD and lead >= len(before) + 1, (lead, len(before))
    assert after.endswith(b"\n") or (not after and window.endswith(b"\n")), "the guard behind the window ends its last line"
    front = dna_lines(lead - len(before), 1) + before
    back = after + dna_lines(max(GUARD - len(after), 61), 2)
    big = front + window + back
    lo, hi = lead, lead + len(window)
    assert big[lo:hi] == window and lo >= GUARD and len(big) - hi >= GUARD
    return big, lo, hi


# ---- the hostile guards of a pattern's plain form ----
class Hostile:
    """The pieces around a window for the plain form P of a pattern, split at k in front and at k2 behind: `before` (the guard's last bytes),
    `first` (the window's first line, with its newline), `last_open` (the window's last line, no newline), `after_open`, `after_closed` (the
    guards' first bytes)."""

    def __init__(self, plain, k, k2=None, filler=b"N" * 9):
        P = plain.encode() if isinstance(plain, str) else bytes(plain)
        k2 = k if k2 is None else k2
        assert 0 < k < len(P) and 0 < k2 < len(P), (k, k2, len(P))
        occ = filler + P + filler + b"\n"                   # a line with a full occurrence
        self.P, self.k, self.k2 = P, k, k2
        self.before = occ + P[:k]
        self.first = P[k:] + filler + b"\n"
        self.last_open = filler + P[:k2]
        self.after_open = P[k2:] + b"\n" + occ
        self.after_closed = occ
        self.fasta_before = b">"
        self.fasta_first = filler + P + filler + b"\n"


def hostile_for(hits, plain, fasta=False):
    """The Hostile of a pattern whose placements are live: each split about m // 2, then further out -- a pattern searched at distance tau
    matches its own last m - k bases when k <= tau, so the split in front ends up above tau and the one behind below m - tau -- between
    fillers of N, which match no base.  hits(buf) -> SQ_ALL hit set (below).  AssertionError when no split is live: a test error, never a skip."""
    m = len(plain)
    assert m >= 2
    order = sorted(range(1, m), key=lambda k: (abs(k - m // 2), k))
    why = []

    def first_of(tries, what):
        for k in order:
            try:
                tries(Hostile(plain, k))
                return k
            except AssertionError as e:
                why.append("%s, k %d: %s" % (what, k, e))
        raise AssertionError("no live split of %r: %s" % (plain, why[:6]))
    rest = b"ACGTACGTNNNNNNNN\n"
    if fasta:
        live_first_line(hits, Hostile(plain, 1).fasta_first + rest, b">", True)
        k = order[0]
    else:
        k = first_of(lambda h: live_first_line(hits, h.first + rest, h.before), "in front")
    k2 = first_of(lambda h: live_last_line(hits, rest + h.last_open, h.after_open), "behind")
    return Hostile(plain, k, k2)


def abs_hits(records, offsets):
    """oracle records [n, 4] (line, start, end, dist) + 1-based line -> offset table -> {(absolute start, absolute end, dist)}"""
    return {(int(offsets[int(r[0])]) + int(r[1]), int(offsets[int(r[0])]) + int(r[2]), int(r[3])) for r in records}


def _first_line_end(window):
    e = window.find(b"\n")
    return len(window) if e < 0 else e


def live_first_line(hits, window, before, fasta=False):
    """The guard in front is live: with its tail the window's first line has a hit that starts before byte 0 or (FASTA: the line becomes a
    header) loses the one it has; alone it has none (FASTA: has one).  hits(buf) -> {(absolute start, end, dist)} under SQ_ALL."""
    e = _first_line_end(window)
    alone = {h for h in hits(window) if h[0] < e}
    b = len(before)
    ext = {(s - b, en - b, d) for s, en, d in hits(before + window) if en - b > 0 and s - b < e}
    if fasta:
        assert alone and not ext, "FASTA guard: the first line has %d hits alone and %d behind the guard's `>`" % (len(alone), len(ext))
    else:
        assert not alone, "the window's first line has a hit of its own: %s" % sorted(alone)[:2]
        assert any(s < 0 for s, _, _ in ext), "no hit straddles byte 0 behind the guard"
    return True


def live_last_line(hits, window, after):
    """The open guard behind is live: with its head the window's last line (no final newline) has a hit that ends behind the window;
    alone it has none."""
    assert not window.endswith(b"\n")
    l0 = window.rfind(b"\n") + 1
    alone = {h for h in hits(window) if h[1] > l0}
    ext = {h for h in hits(window + after) if h[0] < len(window) and h[1] > l0}
    assert not alone, "the window's last line has a hit of its own: %s" % sorted(alone)[:2]
    assert any(en > len(window) for _, en, _ in ext), "no hit straddles the window's end"
    return True


def live_closed(counts, window, after):
    """The closed guard behind is live: its first line is one more counted line and one more matching line.  counts(buf) -> (nlines,
    nmatchlines)."""
    assert window.endswith(b"\n") and after.endswith(b"\n")
    head = after[:after.index(b"\n") + 1]
    a, b = counts(window), counts(window + head)
    assert b[0] == a[0] + 1 and b[1] == a[1] + 1, "the guard's first line: counts %s -> %s" % (a, b)
    return True


def live(kind, ref, window, before=b"", after=b"", fasta=False):
    """One name for the four conditions: kind "first" / "last" (ref: hits), "closed" (ref: counts), "gate" (ref: the last span's kind)."""
    if kind == "first":
        return live_first_line(ref, window, before, fasta)
    if kind == "last":
        return live_last_line(ref, window, after)
    if kind == "closed":
        return live_closed(ref, window, after)
    assert kind == "gate", kind
    a, b = ref(window), ref(window + after)
    assert a != b, "the last span's gate kind is %s with and without the guard" % (a,)
    return True


# ---- a kernel-instance row on a hostile window ----
TILE_BYTES = 8192


def row_window(row_buf, h, fasta, closed, per_read=False, foreign=0.0, seed=3):
    """A row's text (tests/kernel_instances.py: RowText.buf) between the hostile first line and the open or closed last line -> (window,
    lines put in front).  What goes in front is TILE_BYTES long, so the occurrences the text plants on the seams of the walks stay on them:
    behind the hostile line, lines of N (N matches no pattern position but N: no occurrence) -- or, per_read (the recipe whose context
    samples the text's head: kernel_instances.build_text, "fasta-per-read"), records shaped like the text's own: a header, 150 bases, the
    text's share of foreign bytes."""
    first = h.fasta_first if fasta else h.first
    rng = random.Random(seed + len(row_buf))
    pad, n = bytearray(), 1
    while TILE_BYTES - len(first) - len(pad) > 320:
        if per_read:
            pad += b">p%04d\n" % n + bytes(rng.choice(b"X-.x") if rng.random() < foreign else rng.choice(b"ACGT") for _ in range(150)) + b"\n"
            n += 2
        else:
            pad += b"N" * rng.randrange(20, 75) + b"\n"
            n += 1
    rest = TILE_BYTES - len(first) - len(pad)
    pad += b"N" * (rest // 2 - 1) + b"\n" + b"N" * (rest - rest // 2 - 1) + b"\n"
    n += 2
    window = first + bytes(pad) + row_buf
    assert len(first) + len(pad) == TILE_BYTES and row_buf.endswith(b"\n")
    if not closed:
        window += h.last_open
    return window, n


def row_case(row, i, hits, plan=None):
    """Row i of the sorted ledger on its hostile window -> (window, before, after, closed): the open last line for even i, the closed one
    for odd i; FASTA rows behind the `>` guard.  hits: the oracle's SQ_ALL hit set of a buffer under the row's options."""
    import kernel_instances as K
    plan = plan or row.plan()
    h = hostile_for(hits, K.plain_pattern(row.pattern), row.fasta)
    closed = bool(i % 2)
    window, _ = row_window(row.text(plan).buf, h, row.fasta, closed, row.recipe == "fasta-per-read", K._foreign_rate(plan, row.options))
    return window, (h.fasta_before if row.fasta else h.before), (h.after_closed if closed else h.after_open), closed


# ---- the chain text: FASTQ records that every entry behind the scan has something to do with ----
FA, FB = "GATGTAGCGCGATTAGCCTG", "TTCACTGGAGTTGTCCCAAT"      # around the guide (tests/test_gpu_tally_grouped.py: FA, FB; test_gpu_tally.py: LEFT, RIGHT)
FC, FD = "CCGATAGGCTTAACGGTCAC", "AGGTCCATTGCAGTACGGAT"      # around the UMI
FLANK_TAU = 1
# which flanks a read carries, in order (test_gpu_inserts.py: KINDS); a: FA's reverse complement, for the both-strands entry
KINDS = ["ABCD"] * 11 + ["ABCDa", "aBCD", "AB", "CD", "ACD", "ABD", "", "ABBCD", "BACD"]
RC_FA = FA[::-1].translate(str.maketrans("ACGT", "TGCA"))
GAPS = [0, 1, 3, 5, 5, 7]                                                   # between the guide's right flank and the UMI's left one
TAILS = ("after_seq", "after_plus", "mid_qual")


def tile():
    """SEEQ_TILE: the items per workgroup of the record post-passes (the tally's and the gate's tiles are the same number)"""
    with open(os.path.join(ROOT, "seeq_amd", "csrc", "seeq_tiles.h")) as f:
        return int(re.search(r"#define\s+SEEQ_TILE\s+(\d+)", f.read()).group(1))


def _mutate1(rng, s):
    s = bytearray(s)
    s[rng.randrange(len(s))] = rng.choice(b"ACGT")
    return bytes(s)


class Chain:
    """2 T + 3 FASTQ records (T: the tile of the record post-passes).  A sequence line: 0 - 5 bases, FA, a guide (<= 20), FB, a gap, FC, a UMI
    (<= 12), FD, 0 - 5 bases -- flanks with one substitution now and then (they are searched at distance 1) and two now and then (not
    found), guides and UMIs with one substitution now and then (the library corrects, the collapse absorbs), flanks missing, doubled or
    out of order by KINDS; quality bytes as tests/test_gpu_qgate.py draws them (4 % below Q20).  The last record is a whole one: every
    flank exact, its qualities high.  `guides`, `umis`: the pools."""

    def __init__(self, seed=5, nrec=None):
        rng = random.Random(seed)
        bases = lambda n: bytes(rng.choices(b"ACGT", k=n))      # noqa: E731
        self.guides = [bases(20) for _ in range(6)] + [bases(17)]
        self.umis = [bases(12) for _ in range(30)] + [bases(10) for _ in range(4)]
        flank = dict(A=FA.encode(), B=FB.encode(), C=FC.encode(), D=FD.encode(), a=RC_FA.encode())
        nrec = nrec or 2 * tile() + 3
        self.records = []
        for i in range(nrec):
            last = i == nrec - 1
            kind = "ABCD" if last else rng.choice(KINDS)
            seq = bytearray(bases(rng.randrange(6)))
            for j, c in enumerate(kind):
                f = flank[c]
                r = rng.random()
                if not last and r < 0.10:
                    f = _mutate1(rng, f)
                    if r < 0.03:
                        f = _mutate1(rng, f)
                seq += f
                nxt = kind[j + 1] if j + 1 < len(kind) else ""
                if c == "A" and nxt == "B":
                    g = rng.choice(self.guides)
                    r = rng.random()
                    seq += g if last or r > 0.12 else _mutate1(rng, g) if r > 0.03 else bases(rng.choice((0, 5, 33)))
                elif c == "C" and nxt == "D":
                    u = rng.choice(self.umis)
                    seq += u if last or rng.random() > 0.15 else _mutate1(rng, u)
                elif nxt:
                    seq += bases(rng.choice(GAPS))
            seq += bases(5 if last else rng.randrange(6))
            if not last and rng.random() < 0.02:
                seq[rng.randrange(len(seq))] = ord("N")
            qual = bytes(73 if last else rng.randrange(35, 53) if rng.random() < 0.04 else 53 if rng.random() < 0.05 else 73 for _ in range(len(seq)))
            self.records.append((b"@r%d" % (i + 1), bytes(seq), b"+", qual))
        self.fastq = b"".join(b"\n".join(r) + b"\n" for r in self.records)
        self.plain = b"".join(r[1] + b"\n" for r in self.records)

    # -- FASTQ windows and their guards --
    def fastq_window(self, tail="whole"):
        """(window, after): the text cut at `tail` (TAILS; "whole": ends in the last record's newline) and what the guard behind it begins
        with -- the rest of the record, its quality bytes high, and one more whole record with every flank."""
        seq = self.records[-1][1]
        n = len(self.fastq)
        cut = dict(whole=n, after_seq=n - len(seq) - 3, after_plus=n - len(seq) - 1, mid_qual=n - 6)[tail]
        more = b"@g\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n"
        return self.fastq[:cut], self.fastq[cut:] + more

    FASTQ_BEFORE = b"@g\n" + FA.encode()[:10]      # the guard ends in a header and half a flank, no newline

    # -- the plain-lines window --
    def plain_window(self, h, closed):
        """The sequence lines alone between a hostile first line -- a whole read but for the first half of its FA, which ends the guard
        (Hostile h, of FA): a hit, a guide and a pair only for a kernel that looks back -- and the open or closed last line."""
        first = h.P[h.k:] + self.guides[0] + FB.encode() + b"ACG" + FC.encode() + self.umis[0] + FD.encode() + b"\n"
        return first + self.plain + (b"" if closed else h.last_open)


def fastq_seq(window):
    """The sequence lines of a FASTQ window taken by position -> (their text, one per line; 1-based record -> offset of its sequence line in
    the window).  A last record that is cut behind its sequence line, or in it, still has that line."""
    lines = window.split(b"\n")
    if lines and lines[-1] == b"" and window.endswith(b"\n"):
        lines.pop()
    offs, seqs, pos = [0], [], 0
    for i, ln in enumerate(lines):
        if i % 4 == 1:
            offs.append(pos)
            seqs.append(ln)
        pos += len(ln) + 1
    return b"".join(s + b"\n" for s in seqs), offs


def line_offsets(buf, fasta=False):
    """1-based counted line -> byte offset of its first byte (a last line without a newline counts)"""
    offs, pos = [0], 0
    lines = buf.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for ln in lines:
        if not (fasta and ln.startswith(b">")):
            offs.append(pos)
        pos += len(ln) + 1
    return offs
