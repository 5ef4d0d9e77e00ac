"""CPU: the decoy of tests/late_text.py is LIVE for every view tests/test_gpu_caller_stream.py runs -- with nothing but the oracle and the
restated rules (test_gpu_text_window.py: Ref), the reference over decoy(window) differs from the reference over the window in every
quantity the GPU module compares, while the lines and records are the same ones.  This is what proves, without a GPU, that an entry which
read the text before its producer had finished would have answered something else."""
import collections

import numpy as np
import pytest

import late_text as L
import text_window as W
from oracle.pyoracle import SQ_ALL, SQ_BEST
from test_gpu_text_window import FLANKS, Ref, Setup

# the views of tests/test_gpu_caller_stream.py
PLAIN_VIEWS = ["plain-b", "plain-c"]
FASTQ_VIEWS = ["fastq-b-" + W.TAILS[0], "fastq-c"]


def test_decoy_keeps_every_byte_but_the_bases():
    every = bytes(range(256))
    d = L.decoy(every)
    assert len(d) == 256
    for b, x in zip(every, d):
        assert x == (ord("A") if b in b"CGT" else ord("a") if b in b"cgt" else b)
    fq = b"@r1 CGT\nACGTNacgtn\n+\nIIII5#CGTI\n"
    assert L.decoy(fq) == b"@r1 AAA\nAAAANaaaan\n+\nIIII5#AAAI\n"
    assert L.decoy(L.decoy(fq)) == L.decoy(fq)


@pytest.fixture(scope="module")
def setup(oracle):
    return Setup(oracle)


@pytest.mark.parametrize("name", PLAIN_VIEWS + FASTQ_VIEWS)
def test_the_decoy_is_live(oracle, setup, name):
    view = setup.views[name]
    true = setup.ref(view)
    dec = Ref(oracle, L.decoy(view.window), view.fastq)
    assert len(dec.window) == len(true.window) and dec.window != true.window
    # the same lines, the same records
    assert dec.offs == true.offs
    assert dec.scan("A", SQ_BEST)["nlines"] == true.scan("A", SQ_BEST)["nlines"] > 0
    if view.fastq:
        assert [ln for i, ln in enumerate(dec.window.split(b"\n")) if i % 4 != 1] == [ln for i, ln in enumerate(true.window.split(b"\n")) if i % 4 != 1], \
            "the decoy changes a header, a `+` line or a quality line of this text"

    def differs(what, a, b):
        assert a != b, "%s: %s is the same over the decoy: an entry that read it would go unnoticed" % (name, what)
    for flank in FLANKS:
        for mode in (SQ_BEST, SQ_ALL):
            a, b = true.scan(flank, mode), dec.scan(flank, mode)
            assert not np.array_equal(a["records"], b["records"]), (name, flank, mode)
            differs("matching lines of %s" % flank, a["nmatchlines"], b["nmatchlines"])
    differs("the demux records", true.demux()[0], dec.demux()[0])
    differs("the demux counts", true.demux()[1], dec.demux()[1])
    for mode in (SQ_ALL, SQ_BEST):
        differs("both strands, mode %d" % mode, true.strands("A", mode).rows, dec.strands("A", mode).rows)
        differs("both strands per strand, mode %d" % mode, true.strands("A", mode).per_strand, dec.strands("A", mode).per_strand)
    for pair in ("AB", "CD"):
        differs("the rows of the %s inserts" % pair, true.rows(pair), dec.rows(pair))
    tally = lambda ref: collections.Counter(b for _, b in ref.spans(ref.rows("AB")))      # noqa: E731
    differs("the plain tally of the guides", tally(true), tally(dec))
    if view.fastq:
        differs("the gate's kinds", list(true.gate(true.rows("AB"))[0]), list(dec.gate(dec.rows("AB"))[0]))
        differs("the gate's kinds of the hits", list(true.gate(true.hit_rows("B"))[0]), list(dec.gate(dec.hit_rows("B"))[0]))
