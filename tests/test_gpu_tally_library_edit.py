"""GPU (-m gpu): assigning spans to a library within ONE EDIT (seeqdevScanSetLibraryMode with SEEQDEV_LIBRARY_EDIT,
seeqdevScanLastLibraryEdits; seeq_tally_library.h: k_tally_assign_near_edit, the near pass's second instance) against the brute force of
test_tally_library_edit_host.py -- a Levenshtein dynamic program over the decoded strings against every entry, no neighbours -- applied
to the inserts that were PLANTED.  Built on test_gpu_tally_library.py and test_gpu_tally.py: reads are prefix + exact left flank + chosen
insert + exact right flank + suffix, every case first asserts that the inserts call found exactly the planted inserts and, on the CPU,
that the planted input holds the kinds it is meant to exercise; a device fault ends the module."""
import collections
import random

import numpy as np
import pytest

import text_window as W
from oracle.pyoracle import SQ_ALL, SQ_BEST
from test_gpu_inserts import _fastq
from test_gpu_tally import LEFT, RIGHT, T, _cuda, _go, _insert_lines, _nothing_after_a_device_fault, _reads      # noqa: F401 (the fixture is this module's latch too)
from test_gpu_tally_append import _columns, _counts, _held_arrays, _reads3, fl      # noqa: F401
from test_gpu_tally_grouped import _cut, _held_of, _text
from test_gpu_tally_grouped import _reads as _guide_umi_reads
from test_gpu_tally_grouped import _same as _same_grouped
from test_gpu_tally_library import COUNTS, flanks      # noqa: F401
from test_tally_append_host import py_append
from test_tally_host import py_key
from test_tally_library_edit_host import PyEditLibrary, _del, _ins
from test_tally_library_host import AMBIGUOUS, CORRECTED, EXACT, UNKNOWN, _rand, _sub, bitlen_passes

pytestmark = pytest.mark.gpu
ZERO = dict(nsubstituted=0, ninserted=0, ndeleted=0)
EDIT = "edit"


# ---- expected values: the brute force over spans that the code under test did not cut ----
def _expected(lib, spans, mode):
    """-> (counts, dense, ids, the split) under mode EDIT, 1 or 0"""
    if mode == EDIT:
        return lib.tally_edit(spans)
    cnt, dense, ids = lib.tally(spans, mode)
    return cnt, dense, ids, dict(ZERO, nsubstituted=cnt["ncorrected"])


def _same(res, edits, lib, spans, mode):
    from seeq_amd import device as dev
    cnt, dense, _, split = _expected(lib, spans, mode)
    bits, passes = bitlen_passes(len(lib), cnt["nassigned"])
    assert {k: res[k] for k in COUNTS} == dict(cnt, key_bits=bits, passes=passes)
    assert res["nspans"] == res["nexact"] + res["ncorrected"] + res["nambiguous"] + res["nunknown"] + res["nlong"] + res["nforeign"]
    assert edits == split and sum(edits.values()) == res["ncorrected"]
    ids = res["ids"].tolist()
    assert all(a < b for a, b in zip(ids, ids[1:])) and all(1 <= i <= len(lib) for i in ids)
    exp = [(i + 1, c) for i, c in enumerate(dense) if c]
    got = list(zip(ids, res["counts"].tolist()))
    if got != exp:
        bad = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
        raise AssertionError("tables differ (%d vs %d entries; first difference at %d: %s vs %s)" % (len(got), len(exp), bad, got[bad:bad + 1], exp[bad:bad + 1]))
    assert dev.library_counts(res, len(lib)).tolist() == dense
    return cnt, split


def _set(s, lib, mode):
    if mode == EDIT:
        s.set_library(lib.seqs, 1, indels=True)
    else:
        s.set_library(lib.seqs, mode)
    assert s.library_edits() == ZERO                        # a set call leaves no split


def _planted(sc, flanks, lib, inserts, what, mode=EDIT, seed=1, fastq=False):
    """set_library, the inserts call over reads that carry `inserts` (its result checked against what was planted), then the library
    tally and its split against the brute force.  -> (result, split, the text)"""
    from seeq_amd import device as dev
    buf = _reads(inserts, seed)
    if fastq:
        buf = _fastq([ln.decode() for ln in buf.split(b"\n")[:-1]], seed + 1, LEFT)[0]
    t = _cuda(buf)

    def call(s):
        _set(s, lib, mode)
        res = s.inserts_tensor(flanks[0], flanks[1], t, SQ_BEST | (dev.SEEQDEV_FASTQ if fastq else 0), copy=False)
        assert res["ninserts"] == len(inserts), (what, res)
        assert _insert_lines(s, t) == list(inserts), what
        return s.tally_library(t), s.library_edits()
    got = {}
    _go(sc, what, call, lambda s, out: got.update(res=out[0], edits=out[1], exp=_same(out[0], out[1], lib, inserts, mode)))
    return got["res"], got["edits"], t


def _library(n, seed, extra=()):
    """n entries of 12 and 20 bases mixed, `extra` among them, shuffled"""
    rng = random.Random(seed)
    seqs = set(extra)
    while len(seqs) < n:
        seqs.add(_rand(rng, rng.choice((12, 20))))
    seqs = sorted(seqs)
    rng.shuffle(seqs)
    return PyEditLibrary(seqs)


def _one_sub(rng, s):
    return _sub(s, rng.randrange(len(s)), rng.randrange(1, 4))


def _one_del(rng, s):
    return _del(s, rng.randrange(len(s)))


def _one_ins(rng, s):
    return _ins(s, rng.randrange(len(s) + 1), rng.choice(b"ACGT"))


def _one_edit(rng, s):
    return rng.choice((_one_sub, _one_del, _one_ins))(rng, s)


def _mixed(rng, lib, n):
    """n inserts: half of them entries, then one substitution, one deletion, one insertion, two edits, random, an N, a 32-mer."""
    out = []
    for _ in range(n):
        s, r = rng.choice([e for e in lib.seqs if len(e) >= 8]), rng.random()
        out.append(s if r < 0.5 else _one_sub(rng, s) if r < 0.62 else _one_del(rng, s) if r < 0.74 else _one_ins(rng, s) if r < 0.86
                   else _one_edit(rng, _one_edit(rng, s)) if r < 0.91 else _rand(rng, rng.choice((11, 12, 13, 19, 20, 21))) if r < 0.96
                   else s[:3] + b"N" + s[4:] if r < 0.98 else _rand(rng, 32))
    return out


def _holds_every_kind(lib, inserts, least=1):
    """On the CPU, before any device call: the brute force finds each of the three classes, an unknown span and an exact one."""
    cnt, _, _, split = lib.tally_edit(inserts)
    assert min(split.values()) >= least and cnt["nunknown"] >= least and cnt["nexact"] >= least, (cnt, split)
    return cnt, split


# ---- shapes ----
@pytest.mark.parametrize("n", [1, T - 1, T, T + 1, 4 * T + 4])
def test_span_counts(gpu, capi, flanks, n):
    """Around the tile T, one span, more than four tiles; a library of 300 entries."""
    from seeq_amd import device as dev
    lib = _library(300, 500)
    inserts = _mixed(random.Random(n), lib, n)
    if n > 1:
        _holds_every_kind(lib, inserts, 30)
    else:
        inserts = [_del(lib.seqs[0], 4)]
        assert lib.assign_edit(inserts[0])[1:] == (CORRECTED, +1)
    sc = dev.Scanner()
    res, edits, _ = _planted(sc, flanks, lib, inserts, "%d spans" % n, seed=n)
    assert res["nspans"] == n and res["key_bits"] == 9
    sc.close()


def _misses(lib, k, total, seed, ends=False):
    rng = random.Random(seed)
    entry = lambda: rng.choice(lib.seqs)                    # noqa: E731

    def miss():
        while True:
            s = rng.choice([_one_sub, _one_del, _one_ins, lambda r, e: _one_edit(r, _one_edit(r, e)), lambda r, e: _rand(r, len(e))])(rng, entry())
            if lib.assign_edit(s)[1] != EXACT:              # (an edit can lead from one entry to another)
                return s
    if ends:
        return [miss()] + [entry() for _ in range(total - 2)] + [miss()]
    out = [miss() for _ in range(k)] + [entry() for _ in range(total - k)]
    rng.shuffle(out)
    return out


@pytest.mark.parametrize("k", [0, 1, 7, 8, 9, 63, 64, 65, 1025, "first_and_last"])
def test_miss_counts(gpu, capi, flanks, k):
    """No miss (the near pass is not launched); around a round's eight half-waves, a workgroup's 64 misses and the compaction's tile
    edge; a miss as the first and as the last span."""
    from seeq_amd import device as dev
    lib = _library(300, 501)
    ends = k == "first_and_last"
    nmiss = 2 if ends else k
    inserts = _misses(lib, nmiss, T + 9 + nmiss, 600 + nmiss, ends)
    cnt, _, _, split = lib.tally_edit(inserts)
    assert cnt["nspans"] - cnt["nexact"] == nmiss and cnt["nlong"] == cnt["nforeign"] == 0      # the misses are exactly those planted
    if ends:
        assert lib.assign_edit(inserts[0])[1] != EXACT and lib.assign_edit(inserts[-1])[1] != EXACT
    if nmiss >= 63:
        assert min(split.values()) >= 5 and cnt["nunknown"] >= 5
    sc = dev.Scanner()
    res, edits, _ = _planted(sc, flanks, lib, inserts, "misses: %s" % k, seed=nmiss)
    assert res["ncorrected"] + res["nambiguous"] + res["nunknown"] == nmiss
    sc.close()


@pytest.mark.parametrize("nlib", [2, 255, 256, 257, 513, 5000])
def test_library_sizes(gpu, capi, flanks, nlib):
    """The sampled top's strides: every key a sample, every second one, a stride of 3 with a short last block, a stride of 20."""
    from seeq_amd import device as dev
    lib = _library(nlib, 700 + nlib)
    inserts = _mixed(random.Random(nlib), lib, T + 50)
    _holds_every_kind(lib, inserts, 30)
    sc = dev.Scanner()
    res, _, _ = _planted(sc, flanks, lib, inserts, "a library of %d" % nlib, seed=nlib)
    assert res["key_bits"] == nlib.bit_length()
    sc.close()


# ---- lengths ----
def _length_case(empty):
    """Entries of 0 (empty) or 1 base, 2, 30 and 31 bases, the homopolymer A x 12, a cross-class pair -> (library, inserts, the spans
    whose assignment the case is about: span -> (kind, len(entry) - len(span)))"""
    rng = random.Random(41 + empty)
    e30, e31 = [_rand(rng, 30) for _ in range(3)], [_rand(rng, 31) for _ in range(3)]
    q = _rand(rng, 12)
    cross = (_sub(q, 3, 1), _ins(q, 8, b"ACGT"[(b"ACGT".index(q[8]) + 1) % 4]))
    lib = _library(60, 42, extra=[b"", b"TA"] if empty else [b"C", b"TA"])
    lib = PyEditLibrary(lib.seqs + e30 + e31 + [b"A" * 12] + list(cross))
    about = {b"A" * 11: (CORRECTED, +1), b"A" * 13: (CORRECTED, -1), q: (AMBIGUOUS, None),
             _del(e31[0], 0): (CORRECTED, +1), _del(e31[1], 17): (CORRECTED, +1), _del(e31[2], 30): (CORRECTED, +1),      # spans of 30 that reach a 31-base entry
             _ins(e30[0], 0, 71): (CORRECTED, -1), _ins(e30[1], 30, 65): (CORRECTED, -1), _sub(e31[0], 30, 2): (CORRECTED, 0),      # spans of 31: a deletion or a substitution only
             _del(_del(e31[0], 3), 9): (UNKNOWN, None), e30[2]: (EXACT, None), e31[2]: (EXACT, None), b"TA": (EXACT, None)}
    if empty:
        about.update({b"": (EXACT, None), b"G": (CORRECTED, -1), b"T": (AMBIGUOUS, None)})       # a span of 1 reaches the empty entry by deletion; T: "" and TA
    else:
        about.update({b"": (CORRECTED, +1), b"C": (EXACT, None), b"G": (CORRECTED, 0), b"T": (AMBIGUOUS, None)})      # a span of 0 reaches the one-base entry by insertion
    inserts = [s for s in about for _ in range(3)] + [_ins(e31[0], 5, 65)] * 4 + [rng.choice(lib.seqs) for _ in range(T)]      # a 31-base entry that gained a base: long
    rng.shuffle(inserts)
    return lib, inserts, about


@pytest.mark.parametrize("empty", [False, True], ids=["one_base_entry", "empty_entry"])
def test_lengths_at_both_ends(gpu, capi, flanks, empty):
    from seeq_amd import device as dev
    lib, inserts, about = _length_case(empty)
    for s, (kind, by) in about.items():                     # on the CPU first: the planted spans are what the case says they are
        got = lib.assign_edit(s)
        assert got[1:] == (kind, by), (s, got)
    cnt, _, _, split = lib.tally_edit(inserts)
    assert cnt["nlong"] == 4 and min(split.values()) >= 3 and cnt["nambiguous"] >= 6 and cnt["nunknown"] >= 3
    sc = dev.Scanner()
    res, edits, _ = _planted(sc, flanks, lib, inserts, "lengths, %s" % ("the empty entry" if empty else "a one-base entry"))
    assert res["nlong"] == 4
    sc.close()


# ---- modes 0 and 1 through the new entry ----
@pytest.mark.parametrize("mode", [0, 1])
def test_modes_0_and_1_are_max_mismatch(gpu, capi, flanks, mode):
    from seeq_amd import device as dev
    lib = _library(300, 502)
    inserts = _mixed(random.Random(50 + mode), lib, T + 60)
    t = _cuda(_reads(inserts, 5))
    keys = np.array(lib.keys(), dtype=np.uint64)
    out = []
    for by_mode in (True, False):
        sc = dev.Scanner()

        def call(s):
            if by_mode:
                assert s._lib.seeqdevScanSetLibraryMode(s._h, keys.ctypes.data, len(keys), mode) == 0
            else:
                s.set_library(lib.seqs, mode)
            assert s.inserts_tensor(flanks[0], flanks[1], t, SQ_BEST, copy=False)["ninserts"] == len(inserts)
            assert _insert_lines(s, t) == list(inserts)
            res = s.tally_library(t)
            return res, s.library_edits(), s.tally_table(res["ndistinct"]).tobytes()
        _go(sc, "mode %d, %s" % (mode, "by mode" if by_mode else "by max_mismatch"), call,
            lambda s, o: (_same(o[0], o[1], lib, inserts, mode), out.append(o)))
        sc.close()
    (a, ea, ta), (b, eb, tb) = out
    assert {k: a[k] for k in COUNTS} == {k: b[k] for k in COUNTS} and ea == eb and ta == tb
    assert ea["ninserted"] == ea["ndeleted"] == 0 and (ea["nsubstituted"] > 50) == bool(mode)


# ---- the other library entries ----
def test_the_hold_folds_indel_copies_into_their_entry(gpu, capi, fl):
    """Guides with planted edits plus 12-base UMIs: tally_hold_library on the guide inserts, then the unchanged tally_grouped on the UMI
    inserts: as many groups as library entries planted."""
    from seeq_amd import device as dev
    rng = random.Random(9)
    lib = _library(40, 503)
    used = sorted(set(rng.sample(range(len(lib)), 11) + [len(lib) - 1]))
    umis = [_rand(rng, 12) for _ in range(30)]
    spec = []
    for _ in range(T + 150):
        g, r = lib.seqs[rng.choice(used)], rng.random()
        guide = g if r < 0.55 else _one_sub(rng, g) if r < 0.65 else _one_del(rng, g) if r < 0.78 else _one_ins(rng, g) if r < 0.9 else _one_edit(rng, _one_edit(rng, g))
        spec.append((guide, rng.choice(umis)))
    spec += [(None, umis[0]), (lib.seqs[used[0]], None)]
    lines = _guide_umi_reads(spec, 9)
    guides = [(i + 1, g) for i, (g, _) in enumerate(spec) if g is not None]
    members = [(i + 1, u) for i, (_, u) in enumerate(spec) if u is not None]
    cnt, _, ids, split = lib.tally_edit([g for _, g in guides])
    held = [(ln, i) for (ln, _), i in zip(guides, ids)]
    assert min(split.values()) > 50 and cnt["nunknown"] > 20 and {i for i in ids if i} == {u + 1 for u in used}
    t = _cuda(_text(lines))

    def call(s):
        _set(s, lib, EDIT)
        _cut(s, fl["A"], fl["B"], t, guides, "guides")
        hold = s.tally_hold_library(t)
        edits = s.library_edits()
        _cut(s, fl["C"], fl["D"], t, members, "UMIs")
        return hold, edits, s.tally_grouped(t)

    def check(s, got):
        hold, edits, grouped = got
        bits, _ = bitlen_passes(len(lib))
        assert {k: hold[k] for k in COUNTS} == dict(cnt, ndistinct=0, key_bits=bits, passes=0) and edits == split
        pairs, groups = _same_grouped(grouped, held, members)
        by_line = dict(held)
        tab = collections.Counter((by_line[ln], py_key(u)[1]) for ln, u in members if by_line.get(ln))
        assert pairs == [(g, m, c) for (g, m), c in sorted(tab.items())]
        assert [g[0] for g in groups] == [u + 1 for u in used] and grouped["ngroups"] == len(used)
    sc = dev.Scanner()
    _go(sc, "the library hold under the edit mode", call, check)
    sc.close()


def test_the_appended_library_column_under_the_edit_mode(gpu, capi, fl):
    """(cell, guide) x UMI with the guide column assigned within one edit: the held tuples are those of the brute force."""
    from seeq_amd import device as dev
    rng = random.Random(24)
    lib = _library(13, 504)
    cells, umis = [_rand(rng, 16) for _ in range(5)], [_rand(rng, 12) for _ in range(7)]
    spec = []
    for _ in range(T + 120):
        g, r = rng.choice(lib.seqs), rng.random()
        seen = g if r < 0.5 else _one_sub(rng, g) if r < 0.62 else _one_del(rng, g) if r < 0.75 else _one_ins(rng, g) if r < 0.88 else _rand(rng, 20) if r < 0.95 else None
        spec.append((rng.choice(cells), seen, rng.choice(umis)))
    cells_c, guides, members = _columns(spec)
    cnt, _, ids, split = lib.tally_edit([g for _, g in guides])
    assert min(split.values()) > 50 and cnt["nunknown"] > 20
    held0, hcnt = _held_of(cells_c)
    exp_held, acnt = py_append(held0, [(ln, i) for (ln, _), i in zip(guides, ids)], width=len(lib).bit_length())
    acnt["ncolumns"] = 2
    t = _cuda(_text(_reads3(spec, 24)))

    def call(s):
        _set(s, lib, EDIT)
        _cut(s, fl["E"], fl["F"], t, cells_c, "cells")
        hold = s.tally_hold(t)
        _cut(s, fl["A"], fl["B"], t, guides, "guides")
        app = s.tally_hold_append(t, library=True)
        edits = s.library_edits()
        held = _held_arrays(s)
        _cut(s, fl["C"], fl["D"], t, members, "UMIs")
        return hold, app, edits, held, s.tally_grouped(t)

    def check(s, out):
        hold, app, edits, held, res = out
        bits, _ = bitlen_passes(len(lib))
        assert hold == hcnt and _counts(app) == acnt and held == exp_held and edits == split
        assert {k: app["column"][k] for k in COUNTS} == dict(cnt, ndistinct=0, key_bits=bits, passes=0)
        _same_grouped(res, exp_held, members)
    sc = dev.Scanner()
    _go(sc, "library append under the edit mode", call, check)
    sc.close()


def test_hits_against_a_library_whose_entries_differ_in_length(gpu, capi):
    """source="hits": the matches of a pattern with four free bases are all 20 bytes; the entries are such matches, some with a base
    less and some with a base more -- reached by an insertion, by a deletion."""
    from seeq_amd import device as dev
    rng = random.Random(15)
    hit = lambda four: b"CATGCATG" + four + b"GTACGTAC"      # noqa: E731
    fours = sorted({_rand(rng, 4) for _ in range(24)})
    rng.shuffle(fours)
    lib = PyEditLibrary([hit(f) for f in fours[:6]] + [_del(hit(f), 9) for f in fours[6:11]] + [_ins(hit(f), 10, 65) for f in fours[11:16]])
    spans = [hit(rng.choice(fours)) for _ in range(T + 30)]
    cnt, split = _holds_every_kind(lib, spans, 30)
    lines = [_rand(rng, rng.randrange(1, 9)).replace(b"C", b"A") + s + _rand(rng, rng.randrange(1, 9)).replace(b"G", b"T") for s in spans]
    t = _cuda(b"\n".join(lines) + b"\n")
    pat = dev.Pattern("CATGCATGNNNNGTACGTAC", 0)

    def call(s):
        _set(s, lib, EDIT)
        got = s.scan_tensor(pat, t, SQ_ALL, dev.WANT_RECORDS)
        assert got["nrecords"] == len(spans)
        rec = s.records(len(spans))
        assert [lines[i][a:b] for i, (a, b) in enumerate(zip(rec[:, 1].tolist(), rec[:, 2].tolist()))] == spans
        return s.tally_library(t, source="hits"), s.library_edits()
    sc = dev.Scanner()
    _go(sc, "hits under the edit mode", call, lambda s, o: _same(o[0], o[1], lib, spans, EDIT))
    pat.close()
    sc.close()


def test_gated_spans_under_the_edit_mode(gpu, capi, flanks):
    """source="gated": FASTQ inserts behind a quality gate that passes every span but the long ones."""
    from seeq_amd import device as dev
    lib = _library(300, 505)
    inserts = _mixed(random.Random(17), lib, T + 40)
    _holds_every_kind(lib, inserts, 30)
    buf = _fastq([ln.decode() for ln in _reads(inserts, 17).split(b"\n")[:-1]], 18, LEFT)[0]
    passed = [x for x in inserts if len(x) <= 31]            # (the gate passes no long span: no tally would count it)
    assert 0 < len(passed) < len(inserts)
    t = _cuda(buf)

    def call(s):
        _set(s, lib, EDIT)
        assert s.inserts_tensor(flanks[0], flanks[1], t, SQ_BEST | dev.SEEQDEV_FASTQ, copy=False)["ninserts"] == len(inserts)
        assert _insert_lines(s, t) == list(inserts)
        gate = s.quality_gate(t, min_qual=0, copy=False)
        assert gate["npassed"] == len(passed) and gate["nlong"] == len(inserts) - len(passed)
        return s.tally_library(t, source="gated"), s.library_edits()
    sc = dev.Scanner()
    _go(sc, "gated spans under the edit mode", call, lambda s, o: _same(o[0], o[1], lib, passed, EDIT))
    sc.close()


def test_anchored_spans_under_the_edit_mode(gpu, capi):
    """source="anchored": every line is one span -- the pattern N finds a line by its first base, the anchor cuts the whole line."""
    from seeq_amd import device as dev
    lib = _library(300, 506)
    spans = [s for s in _mixed(random.Random(19), lib, T + 40) if s]
    _holds_every_kind(lib, spans, 30)
    t = _cuda(b"\n".join(spans) + b"\n")
    pat = dev.Pattern("N", 0)

    def call(s):
        _set(s, lib, EDIT)
        assert s.scan_tensor(pat, t, SQ_BEST, dev.WANT_RECORDS)["nrecords"] == len(spans)
        cut = s.anchor(t, source="hits", anchor="line", skip=0, length=0, reach=64)
        assert cut["nkept"] == len(spans) and cut["records"][:, 1].tolist() == [0] * len(spans) and cut["records"][:, 2].tolist() == [len(x) for x in spans]
        return s.tally_library(t, source="anchored"), s.library_edits()
    sc = dev.Scanner()
    _go(sc, "anchored spans under the edit mode", call, lambda s, o: _same(o[0], o[1], lib, spans, EDIT))
    pat.close()
    sc.close()


def test_the_edit_mode_under_fastq(gpu, capi, flanks):
    from seeq_amd import device as dev
    lib = _library(300, 507)
    inserts = _mixed(random.Random(21), lib, T + 77)
    _holds_every_kind(lib, inserts, 30)
    sc = dev.Scanner()
    _planted(sc, flanks, lib, inserts, "FASTQ", seed=21, fastq=True)
    sc.close()


# ---- state ----
def test_one_scanner_through_the_modes(gpu, capi, flanks):
    """Edit mode, substitution mode, edit mode again over the same text on one Scanner: each result is a fresh Scanner's."""
    from seeq_amd import device as dev
    lib = _library(300, 508)
    inserts = _mixed(random.Random(23), lib, T + 90)
    _holds_every_kind(lib, inserts, 30)
    sc = dev.Scanner()
    seen = []
    for mode in (EDIT, 1, EDIT):
        res, edits, t = _planted(sc, flanks, lib, inserts, "one Scanner, mode %s" % mode, mode=mode, seed=23)
        fresh = dev.Scanner()
        other, other_edits, _ = _planted(fresh, flanks, lib, inserts, "a fresh Scanner, mode %s" % mode, mode=mode, seed=23)
        assert {k: res[k] for k in COUNTS} == {k: other[k] for k in COUNTS} and edits == other_edits
        assert res["ids"].tobytes() == other["ids"].tobytes() and res["counts"].tobytes() == other["counts"].tobytes()
        fresh.close()
        seen.append((res, edits))
    assert seen[0][1] == seen[2][1] and seen[0][0]["ids"].tobytes() == seen[2][0]["ids"].tobytes()
    assert seen[1][1]["ninserted"] == seen[1][1]["ndeleted"] == 0 and seen[1][0]["ncorrected"] < seen[0][0]["ncorrected"]
    sc.set_library(lib.seqs, 1, indels=True)
    assert sc.library_edits() == ZERO                       # zero after set_library, whatever the assignment before
    sc.clear_library()
    assert sc.library_edits() == ZERO
    with pytest.raises(ValueError):
        sc.set_library(lib.seqs, 0, indels=True)
    sc.close()


# ---- placement ----
def test_a_window_of_a_larger_buffer(gpu, capi, flanks):
    """The reads as a window of a larger tensor at an odd lead; the guard in front ends in the first half of a left flank, the window
    begins with the second half, an entry and a right flank: an insert only for a kernel that looks in front of the window."""
    from seeq_amd import device as dev
    lib = _library(300, 509)
    inserts = _mixed(random.Random(25), lib, T + 33)
    _holds_every_kind(lib, inserts, 30)
    window = LEFT.encode()[10:] + lib.seqs[0] + RIGHT.encode() + b"\n" + _reads(inserts, 25)
    big, lo, hi = W.place(window, W.odd_lead(1), before=LEFT.encode()[:10])
    assert lo % 2 == 1
    view = _cuda(big)[lo:hi]
    assert view.is_contiguous() and view.data_ptr() % 16 == lo % 16
    got = []
    for what, t in (("a window at lead %d" % lo, view), ("the window alone", _cuda(window))):
        def call(s):
            _set(s, lib, EDIT)
            assert s.inserts_tensor(flanks[0], flanks[1], t, SQ_BEST, copy=False)["ninserts"] == len(inserts), what
            assert _insert_lines(s, t) == list(inserts), what
            return s.tally_library(t), s.library_edits()
        sc = dev.Scanner()
        _go(sc, what, call, lambda s, o: (_same(o[0], o[1], lib, inserts, EDIT), got.append(o)))
        sc.close()
    assert got[0][1] == got[1][1] and got[0][0]["ids"].tobytes() == got[1][0]["ids"].tobytes() and got[0][0]["counts"].tobytes() == got[1][0]["counts"].tobytes()
