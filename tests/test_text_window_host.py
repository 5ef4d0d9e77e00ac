"""CPU: the placements of tests/text_window.py are what they claim, and every one of them is LIVE for every text the GPU modules put into
them -- all rows of kernel_instances.rows() with their hostile first and last lines, and the chain text of tests/test_gpu_text_window.py in
its FASTQ and plain forms.  Live: the oracle (or the restated gate) over guard + window differs from the one over the window alone in the
quantity the placement is there for.  This is what proves, without a GPU, that the GPU tests fail if a kernel uses bytes outside its text."""
import pytest

import kernel_instances as K
import text_window as W
from oracle.pyoracle import SQ_ALL, SQ_BEST
from test_qgate_host import MISFIT, PASS, py_gate

ROWS = sorted(K.rows(), key=lambda r: (r.pattern, r.tau, r.recipe, r.avg_line, r.options & ~3, r.key))


def test_place():
    for lead in W.ODD_LEADS + tuple(W.aligned_lead(i) for i in range(7)):
        for before, window, after in ((b"", b"ACGT\n", b""), (b"ACGT\nAC", b"GT\nAAAA", b"CC\nACGT\n"), (b">", b"ACGT\n", b"GGGG\n")):
            big, lo, hi = W.place(window, lead, before, after)
            assert big[lo:hi] == window and lo == lead and big[lo - len(before):lo] == before and big[hi:hi + len(after)] == after
            assert lo >= W.GUARD and len(big) - hi >= W.GUARD
            assert big[:lo - len(before)].endswith(b"\n") and big.endswith(b"\n")
            assert set(big[:lo - len(before)] + big[hi + len(after):]) <= set(b"ACGT\n")      # the filling: valid DNA lines
            assert max(len(ln) for ln in big[hi + len(after):].split(b"\n")) <= 60
    assert {lead % 16 for lead in W.ODD_LEADS} >= {1, 3, 5, 7, 9, 11, 13, 15} and all(lead % 2 for lead in W.ODD_LEADS)
    assert all(W.aligned_lead(i) % 16 == 0 and W.aligned_lead(i) % 128 for i in range(20))
    with pytest.raises(AssertionError):
        W.place(b"ACGT", W.GUARD + 1, b"", b"")                 # an open window needs a guard that closes its line
    with pytest.raises(AssertionError):
        W.place(b"ACGT\n", 100, b"", b"")


def test_dna_lines_have_the_size_asked_for():
    for n in list(range(0, 200)) + [4095, 4096, 4097]:
        buf = W.dna_lines(n)
        assert len(buf) == n and (not n or buf.endswith(b"\n"))


def _hits_of(oracle, row):
    nd = row.options & 0x0C

    def hits(buf):
        e = oracle.buffer_scan(row.pattern, row.tau, buf, SQ_ALL | nd, fasta=row.fasta)
        return W.abs_hits(e["records"], W.line_offsets(buf, row.fasta))
    return hits


def _counts_of(oracle, row):
    def counts(buf):
        e = oracle.buffer_scan(row.pattern, row.tau, buf, SQ_ALL | (row.options & 0x0C), fasta=row.fasta)
        return e["nlines"], e["nmatchlines"]
    return counts


@pytest.mark.parametrize("part", range(8))
def test_every_row_is_live_in_its_placements(oracle, harness, part):
    """Per row: the hostile first line (FASTA rows: the `>` guard), the open or the closed last line (by row index), on the row's whole window."""
    K.use_harness(harness)
    for i, row in enumerate(ROWS):
        if i % 8 != part:
            continue
        hits = _hits_of(oracle, row)
        window, before, after, closed = W.row_case(row, i, hits)
        assert closed == bool(i % 2) and window[W.TILE_BYTES:W.TILE_BYTES + 64] == row.text().buf[:64]
        W.live("first", hits, window, before, fasta=row.fasta)
        if closed:
            W.live("closed", _counts_of(oracle, row), window, after=after)
        else:
            W.live("last", hits, window, after=after)


@pytest.fixture(scope="module")
def chain():
    return W.Chain()


def _flank_hits(oracle, expr, fastq):
    def hits(buf):
        if fastq:
            seq, offs = W.fastq_seq(buf)
        else:
            seq, offs = buf, W.line_offsets(buf)
        e = oracle.buffer_scan(expr, W.FLANK_TAU, seq, SQ_ALL)
        return W.abs_hits(e["records"], offs)
    return hits


def test_the_chain_text(chain):
    assert len(chain.records) == 2 * W.tile() + 3 and 5 * 65536 < len(chain.fastq) < 1 << 20
    assert chain.plain == W.fastq_seq(chain.fastq)[0]
    for tail in W.TAILS + ("whole",):
        window, after = chain.fastq_window(tail)
        assert (window + after).startswith(chain.fastq) and after.endswith(b"\n")
        seq, offs = W.fastq_seq(window)
        assert seq == chain.plain and len(offs) == len(chain.records) + 1
        assert window[offs[-1]:offs[-1] + len(chain.records[-1][1])] == chain.records[-1][1]


def test_the_chain_text_is_live_as_plain_lines(oracle, chain):
    hits = _flank_hits(oracle, W.FA, False)
    h = W.hostile_for(hits, W.FA)
    W.live("first", hits, chain.plain_window(h, False), h.before)
    W.live("last", hits, chain.plain_window(h, False), after=h.after_open)

    def counts(buf):
        e = oracle.buffer_scan(W.FA, W.FLANK_TAU, buf, SQ_ALL)
        return e["nlines"], e["nmatchlines"]
    W.live("closed", counts, chain.plain_window(h, True), after=h.after_closed)


def test_the_chain_text_is_live_as_fastq(oracle, chain):
    """In front: the guard's header and half flank shift the records by a line.  Behind: each tail changes the gate kind of the last
    record's guide and UMI spans (MISFIT alone, PASS with the guard); the whole text gains a record that matches."""
    window, _ = chain.fastq_window("whole")

    def records(buf):
        seq, offs = W.fastq_seq(buf)
        e = oracle.buffer_scan(W.FA, W.FLANK_TAU, seq, SQ_BEST)
        return e["nlines"], e["nmatchlines"], len(e["records"])
    alone, ext = records(window), records(chain.FASTQ_BEFORE + window)
    assert alone[0] == len(chain.records) and alone[1] > alone[0] // 2
    assert ext[1] < alone[1] // 4, "behind the guard the records are other lines: %s -> %s" % (alone, ext)
    seq = chain.records[-1][1]
    spans = {name: (seq.index(le.encode()) + 20, seq.index(ri.encode())) for name, le, ri in (("guide", W.FA, W.FB), ("umi", W.FC, W.FD))}
    for tail in W.TAILS:
        window, after = chain.fastq_window(tail)
        off = W.fastq_seq(window)[1][-1]
        for name, (start, end) in spans.items():
            assert 0 < end - start <= 20
            kind = lambda buf: py_gate(buf, off, start, end)[0]      # noqa: E731
            W.live("gate", kind, window, after=after)
            assert kind(window) == MISFIT and kind(window + after) == PASS, (tail, name)
    window, after = chain.fastq_window("whole")
    alone, ext = records(window), records(window + after)
    assert ext[0] == alone[0] + 1 and ext[1] == alone[1] + 1, "the guard's record: %s -> %s" % (alone, ext)
