"""GPU (-m gpu): the tally of the held column itself (seeqdevScanTallyHeld / seeqdevScanTallyHeldDense; seeq_tally_held.h: the pack of the
held words, the single-word radix sort, the two-row run-length pass, both tables and the dense scatter, all on the device) against the rule
restated in Python (test_tally_held_host.py: py_held, py_dense) over what was PLANTED.  Held columns are built three ways, and every case
first asserts that the scans found exactly what was planted -- a vacuous case fails:

  lines     a text whose every line IS a key: the pattern N at distance 0 finds a line by its first base, anchor="line" cuts the whole line,
            a hold (or an append) of the anchored spans takes it.  One record per line; a line with an N inside is held without a key.
  tails     lines that carry the pattern HA once, twice or three times, found under SQ_ALL; anchor="after" cuts the four bytes behind every
            match, a hold of the anchored spans takes them: several records per line, any of them with or without a key.
  screen    sample barcode by demultiplex, guide between two flanks by an inserts call, assigned to a library: sample x library id."""
import ctypes as C
import errno
import random

import numpy as np
import pytest

import late_text as L
from oracle.pyoracle import SQ_ALL, SQ_BEST
from test_gpu_strands import _step
from test_gpu_tally_grouped import FA, FB, FC, FD, T, _cuda, _cut, _kmer, _text
from test_tally_append_host import py_append
from test_tally_held_host import COUNTED, DENSE, HELD, REPEAT, py_dense, py_held, py_kinds
from test_tally_host import OK, py_key

pytestmark = pytest.mark.gpu
HA = "CATGNNNNGTAC"                                         # found under SQ_ALL at distance 0: the tails' anchor
HIT = b"CATGAAAAGTAC"

_FAULT = []


@pytest.fixture(autouse=True)
def _nothing_after_a_device_fault():
    """A device fault ends the module: what comes after it fails here, before it starts anything on the device."""
    if _FAULT:
        pytest.fail("a device fault earlier in this module (%s): nothing more is started on the device" % _FAULT[0])
    yield


def _go(sc, what, call, check, fresh=None):
    """_step of test_gpu_strands.py; a device fault (it raises the SeeqDeviceError untouched) is remembered for the rest of the module."""
    from seeq_amd import device as dev
    try:
        _step(sc, what, call, check, fresh)
    except dev.SeeqDeviceError as e:
        _FAULT.append("%s: %s" % (what, e))
        raise


@pytest.fixture(scope="module")
def pats(gpu):
    from seeq_amd import device as dev
    ps = {k: dev.Pattern(v, 0) for k, v in dict(N="N", HA=HA, A=FA, B=FB, C=FC, D=FD).items()}
    yield ps
    for p in ps.values():
        p.close()


# ---- held columns ----
def _key(seq):
    kind, key = py_key(seq)
    return key if kind == OK else 0


def _pool(rng, n, m):
    out = []
    while len(out) < n:
        s = _kmer(rng.getrandbits(2 * m), m)
        if s not in out:
            out.append(s)
    return out


def _lines_column(s, pats, t, lines, what):
    """The anchored spans of a text whose every line is one span -> the column [(line, key)] they make."""
    from seeq_amd import device as dev
    n = len(lines)
    assert s.scan_tensor(pats["N"], t, SQ_BEST, dev.WANT_RECORDS)["nrecords"] == n, what
    cut = s.anchor(t, source="hits", anchor="line", skip=0, length=0, reach=64)
    rec = cut["records"]
    assert cut["nkept"] == n and np.array_equal(rec[:, 0], np.arange(1, n + 1)) and not rec[:, 1].any(), what
    assert np.array_equal(rec[:, 2], np.array([len(x) for x in lines], dtype=np.uint32)), what
    return [(i + 1, _key(x)) for i, x in enumerate(lines)]


def _tails_text(spec):
    """spec: per line its tails (4 bytes each, in order; none: a line without a record) -> the text."""
    return _text([b"GT" + b"".join(HIT + tail + b"TT" for tail in tails) + b"A" for tails in spec])


def _tails_column(s, pats, t, buf, spec, what):
    from seeq_amd import device as dev
    exp = [(i + 1, tail) for i, tails in enumerate(spec) for tail in tails]
    assert s.scan_tensor(pats["HA"], t, SQ_ALL, dev.WANT_RECORDS)["nrecords"] == len(exp), what
    cut = s.anchor(t, source="hits", anchor="after", skip=0, length=4, reach=64)
    rec, off = cut["records"], cut["offsets"]
    assert cut["nkept"] == len(exp) and rec[:, 0].tolist() == [ln for ln, _ in exp], what
    assert [buf[int(o) + int(r[1]):int(o) + int(r[2])] for o, r in zip(off, rec)] == [tail for _, tail in exp], what
    return [(ln, _key(tail)) for ln, tail in exp]


def _held_arrays(s):
    h = s.held()
    assert h["nrecords"] == len(h["lines"]) == len(h["keys"]) and h["columns"] == s.hold_columns()
    return list(zip(h["lines"].tolist(), h["keys"].tolist()))


def _table(res):
    return list(zip(res["table"]["key"].tolist(), res["table"]["count"].tolist()))


def _rows(res):
    r = res["rows"]
    return list(zip(r["group"].tolist(), r["count"].tolist(), r["first"].tolist(), r["ndistinct"].tolist()))


def _same(s, res, held, m):
    """A tally_held(m) result (copy=True) against the rule over the held column [(line, key)] -> (counts, table, rows) of the rule."""
    cnt, table, rows = py_held(held, s.hold_columns(), m)
    assert {k: res[k] for k in HELD} == cnt
    assert res["nrecords"] == res["ncounted"] + res["nkeyless"] + res["nrepeat"] == len(held)
    got = _table(res)
    if got != table:
        bad = next((i for i, (a, b) in enumerate(zip(got, table)) if a != b), min(len(got), len(table)))
        raise AssertionError("key tables differ (%d vs %d entries; first difference at %d: %s vs %s)" % (len(got), len(table), bad, got[bad:bad + 1], table[bad:bad + 1]))
    assert _rows(res) == rows
    assert int(res["table"]["count"].sum()) == res["ncounted"] and (not m or int(res["rows"]["count"].sum()) == res["ncounted"])
    assert not m or int(res["rows"]["ndistinct"].sum()) == res["ndistinct"]
    assert s.tally_table(res["ndistinct"]).tobytes() == res["table"].tobytes()      # the key table is the Scanner's tally table
    assert s.tally_held_rows_table(res["nrows"]).tobytes() == res["rows"].tobytes() and (not res["nrows"] or s.tally_held_rows_device_ptr())
    return cnt, table, rows


def _twice(s, m):
    """tally_held(m), twice: the same answer."""
    a, b = s.tally_held(m), s.tally_held(m)
    assert {k: a[k] for k in HELD} == {k: b[k] for k in HELD} and a["table"].tobytes() == b["table"].tobytes() and a["rows"].tobytes() == b["rows"].tobytes()
    return a


def _matrix(s, table, shift, nrows, ncols, out=None):
    """held_matrix against np.zeros plus a host scatter of the rule's table."""
    import torch
    got, cnt = s.held_matrix(nrows, ncols, out)
    cells, exp = py_dense(table, shift, nrows, ncols)
    host = np.zeros(nrows * ncols, dtype=np.int64)
    for cell, count in cells.items():
        host[cell] = count
    assert cnt == exp and tuple(cnt) == DENSE and got.dtype == torch.int64 and tuple(got.shape) == (nrows, ncols) and got.is_cuda
    assert out is None or got is out
    assert np.array_equal(got.cpu().numpy().reshape(-1), host)
    assert cnt["ninside"] + cnt["noutside"] == len(table) and cnt["inside_reads"] + cnt["outside_reads"] == sum(c for _, c in table) == int(host.sum()) + cnt["outside_reads"]
    return cnt


# ---- 1. held records around the tile ----
@pytest.mark.parametrize("n", [0, 1, T - 1, T, T + 1, 2 * T + 1])
def test_held_record_counts(gpu, capi, pats, n):
    """One column, member_columns 0: no record (nothing is launched), one, a tile less one, a tile, a tile and one, two tiles and one."""
    from seeq_amd import device as dev
    rng = random.Random(n + 5)
    pool = _pool(rng, 40, 6)
    lines = [b"ACNTAC" if i % 13 == 5 else rng.choice(pool) for i in range(n)]
    t = _cuda(_text(lines) if n else b"ACGTACGTAC\n")
    sc = dev.Scanner()

    def call(s):
        if n:
            held = _lines_column(s, pats, t, lines, "%d lines" % n)
            hold = s.tally_hold(t, source="anchored")
        else:
            _cut(s, pats["A"], pats["B"], t, [], "no record")
            held, hold = [], s.tally_hold(t)
        assert hold["nspans"] == n and _held_arrays(s) == held
        return held, _twice(s, 0)

    def check(s, out):
        held, res = out
        cnt, table, _ = _same(s, res, held, 0)
        assert cnt["nrepeat"] == 0 and cnt["nkeyless"] == sum(1 for i in range(n) if i % 13 == 5) and cnt["passes"] == (2 if n else 0)
        assert res["nrows"] == 0 and len(res["rows"]) == 0 and (n < 100 or len(table) == 40)
    _go(sc, "%d held records" % n, call, check)
    sc.close()


# ---- 2. several records per line; the tile seam ----
@pytest.mark.parametrize("pair_at", [T - 1, T - 2])
def test_a_repeat_across_the_tile_seam_and_a_line_that_opens_behind_it(gpu, capi, pats, pair_at):
    """pair_at T - 1: records T - 1 and T lie on one line -- the first record of the second tile is a repeat, which only the last record of
    the tile before it tells.  pair_at T - 2: records T - 2 and T - 1 share a line and record T opens its own.  Either way record T carries a
    key no other record has.  Further on: a keyless first record with a keyed repeat, a keyed first with a keyless repeat, three records
    on a line, lines without any."""
    from seeq_amd import device as dev
    rng = random.Random(pair_at)
    pool = [_kmer(i, 4) for i in range(0, 200, 7)]
    only = b"GGGG"
    assert only not in pool
    spec = [[rng.choice(pool)] for _ in range(pair_at)]
    spec.append([rng.choice(pool), only] if pair_at == T - 1 else [rng.choice(pool), rng.choice(pool)])
    if pair_at == T - 2:
        spec.append([only])
    for i in range(T // 4):
        spec += [[rng.choice(pool)], [b"ANNA", rng.choice(pool)], [], [rng.choice(pool), b"ANNA"], [rng.choice(pool), rng.choice(pool), rng.choice(pool)], [b"ANNA"]]
    buf = _tails_text(spec)
    t = _cuda(buf)
    sc = dev.Scanner()

    def call(s):
        held = _tails_column(s, pats, t, buf, spec, "tails")
        hold = s.tally_hold(t, source="anchored")
        assert hold["nspans"] == len(held) and hold["key_bits"] == 9 and _held_arrays(s) == held
        return held, _twice(s, 0)

    def check(s, out):
        held, res = out
        kinds = py_kinds(held)
        assert held[T][1] == _key(only) and held[T - 1][0] == (held[T][0] if pair_at == T - 1 else held[T - 2][0])
        assert kinds[T] == (REPEAT if pair_at == T - 1 else COUNTED)
        cnt, table, _ = _same(s, res, held, 0)
        assert (_key(only) in dict(table)) == (pair_at == T - 2)
        assert cnt["nrepeat"] == 1 + 4 * (T // 4) and cnt["nkeyless"] == 2 * (T // 4) and cnt["passes"] == 2
        # the keyed repeats behind a keyless first record are not counted: the counts are those of the first records alone
        first = {}
        for ln, k in held:
            first.setdefault(ln, k)
        assert cnt["ncounted"] == sum(1 for k in first.values() if k) < sum(1 for _, k in held if k) - T // 4
    _go(sc, "a pair of records at %d" % pair_at, call, check)
    sc.close()


# ---- 3. nothing counted ----
def test_every_record_keyless(gpu, capi, pats):
    from seeq_amd import device as dev
    lines = [b"ACNTAC"] * (T + 5)
    t = _cuda(_text(lines))
    sc = dev.Scanner()

    def call(s):
        held = _lines_column(s, pats, t, lines, "foreign lines")
        assert s.tally_hold(t, source="anchored")["nheld"] == 0 and s.hold_columns() == [0]
        return held, _twice(s, 0)

    def check(s, out):
        cnt, table, rows = _same(s, out[1], out[0], 0)
        assert cnt == dict(nrecords=T + 5, ncounted=0, nkeyless=T + 5, nrepeat=0, ndistinct=0, nrows=0, key_bits=0, shift=0, passes=0, member_columns=0)
        assert table == [] and rows == []
    _go(sc, "every record keyless", call, check)
    sc.close()


# ---- 4. records an append dropped ----
def test_records_dropped_by_an_append_count_as_keyless(gpu, capi, pats):
    from seeq_amd import device as dev
    rng = random.Random(44)
    p0, p1 = _pool(rng, 6, 3), _pool(rng, 30, 4)
    n = T + 300
    lines0 = [rng.choice(p0) for _ in range(n)]
    lines1 = [b"ACNT" if i % 7 == 3 else rng.choice(p1) for i in range(n)]
    t0, t1 = _cuda(_text(lines0)), _cuda(_text(lines1))
    sc = dev.Scanner()

    def call(s):
        held0 = _lines_column(s, pats, t0, lines0, "column 0")
        s.tally_hold(t0, source="anchored")
        col = _lines_column(s, pats, t1, lines1, "column 1")
        app = s.tally_hold_append(t1, source="anchored")
        held, acnt = py_append(held0, col)
        assert app["ndropped"] == acnt["ndropped"] == sum(1 for i in range(n) if i % 7 == 3) and _held_arrays(s) == held and s.hold_columns() == [7, 9]
        return held, _twice(s, 1), s.tally_held(0)

    def check(s, out):
        held, res, flat = out
        cnt, table, rows = _same(s, flat, held, 0)
        assert flat["nrows"] == 0 and cnt["shift"] == 0
        res = s.tally_held(1)
        cnt, table, rows = _same(s, res, held, 1)
        assert cnt["nkeyless"] == sum(1 for i in range(n) if i % 7 == 3) > 100 and cnt["shift"] == 9 and cnt["passes"] == 2
        assert len(rows) == 6 and len(table) > 100 and [r[0] for r in rows] == sorted(_key(x) for x in p0)
    _go(sc, "records dropped by an append", call, check)
    sc.close()


# ---- 5. one demux column alone ----
def _screen(rng, n, codes, guides, umis=None, noise=True):
    """-> (lines, the demux column [(line, pattern + 1 or 0)], the guide column [(line, bytes)], the UMI column)."""
    lines, dheld, gcol, ucol = [], [], [], []
    for i in range(n):
        kind = rng.choice(["one"] * 8 + ["two", "none"]) if noise else "one"
        head = b"TT"
        if kind == "one":
            k = rng.randrange(len(codes))
            head += codes[k] + b"CA"
            dheld.append((i + 1, k + 1))
        elif kind == "two":
            a, b = rng.sample(range(len(codes)), 2)
            head += codes[a] + b"CA" + codes[b]
            dheld.append((i + 1, 0))
        g = rng.choice(guides + [None]) if noise else rng.choice(guides)
        body = head + b"AC" + (FA.encode() + g + FB.encode() if g is not None else b"") + b"GT"
        if g is not None:
            gcol.append((i + 1, g))
        if umis:
            u = rng.choice(umis)
            body += FC.encode() + u + FD.encode() + b"TG"
            ucol.append((i + 1, u))
        lines.append(body)
    return lines, dheld, gcol, ucol


def _demux(s, ps, t, dheld):
    rec = s.demux_tensor(ps, t)["records"]
    assert rec["line"].tolist() == [ln for ln, _ in dheld]
    assert [(int(p) + 1) if m else 0 for p, m in zip(rec["pattern"], rec["margin"])] == [k for _, k in dheld]


def test_one_demux_column_alone(gpu, capi, pats):
    """key_bits <= 8: one pass of the sort, member_columns 0; an ambiguous line is keyless, a line without a barcode has no record."""
    from seeq_amd import device as dev
    rng = random.Random(45)
    codes = _pool(rng, 5, 16)
    lines, dheld, _, _ = _screen(rng, T + 300, codes, _pool(rng, 3, 12))
    t = _cuda(_text(lines))
    ps = [dev.Pattern(c.decode(), 0) for c in codes]
    sc = dev.Scanner()

    def call(s):
        _demux(s, ps, t, dheld)
        hold = s.tally_hold(source="demux")
        assert hold["key_bits"] == 3 and _held_arrays(s) == dheld
        return _twice(s, 0)

    def check(s, res):
        cnt, table, _ = _same(s, res, dheld, 0)
        assert cnt["passes"] == 1 and cnt["key_bits"] == 3 and [k for k, _ in table] == [1, 2, 3, 4, 5] and cnt["nkeyless"] > 50 and cnt["nrepeat"] == 0
    _go(sc, "one demux column", call, check)
    sc.close()
    for p in ps:
        p.close()


# ---- 6. sample x library id, and the dense matrix ----
def _sub(seq, at, base):
    return seq[:at] + bytes([base]) + seq[at + 1:]


def _screen_hold(s, pats, ps, t, dheld, gcol, lib):
    """hold(demux), append(library ids of the guides) -> the held column the rule expects."""
    _demux(s, ps, t, dheld)
    s.tally_hold(source="demux")
    _cut(s, pats["A"], pats["B"], t, gcol, "guides")
    app = s.tally_hold_append(t, library=True)
    ids = [(ln, lib.index(g) + 1 if g in lib else 0) for ln, g in gcol]
    held, acnt = py_append(dheld, ids, width=len(lib).bit_length())
    assert app["nheld"] == acnt["nheld"] and app["column"]["nexact"] == sum(1 for _, i in ids if i) and _held_arrays(s) == held
    return held


def test_sample_by_library_id_and_the_dense_matrix(gpu, capi, pats):
    """hold demux, tally_hold_append(library=True), member_columns 1: the row is the sample, the column part the guide's id.  The dense
    matrix against np.zeros plus a host scatter: the full shape, shapes smaller than the largest ids (entries outside), 1 x 1, a shape
    larger than the ids, and a caller's tensor every cell of which is written."""
    import torch
    from seeq_amd import device as dev
    rng = random.Random(46)
    codes, lib = _pool(rng, 5, 16), _pool(rng, 12, 20)
    unknown = _kmer(rng.getrandbits(40), 20)
    assert unknown not in lib
    lines, dheld, gcol, _ = _screen(rng, T + 500, codes, lib + [unknown])
    t = _cuda(_text(lines))
    ps = [dev.Pattern(c.decode(), 0) for c in codes]
    sc = dev.Scanner()
    sc.set_library([g.decode() for g in lib], max_mismatch=0)

    def call(s):
        held = _screen_hold(s, pats, ps, t, dheld, gcol, lib)
        assert s.hold_columns() == [3, 4]
        return held, _twice(s, 1)
    got = {}

    def check(s, out):
        held, res = out
        cnt, table, rows = _same(s, res, held, 1)
        assert cnt["shift"] == 4 and cnt["key_bits"] == 7 and cnt["passes"] == 1 and [r[0] for r in rows] == [1, 2, 3, 4, 5] and len(table) == 5 * 12
        assert cnt["nkeyless"] > 200                        # ambiguous samples, lines without a guide, the unknown guide
        full = _matrix(s, table, 4, 5, 12)
        assert full["noutside"] == 0 and full["inside_reads"] == cnt["ncounted"]
        part = _matrix(s, table, 4, 3, 7)
        assert part["ninside"] == 3 * 7 and part["noutside"] == 60 - 21
        assert _matrix(s, table, 4, 1, 1)["ninside"] == 1
        assert _matrix(s, table, 4, 9, 40)["noutside"] == 0
        mine = torch.full((5, 12), -1, dtype=torch.int64, device="cuda")
        _matrix(s, table, 4, 5, 12, out=mine)
        assert int(mine.min()) >= 1                         # every sample saw every guide
        for bad in (torch.zeros((5, 11), dtype=torch.int64, device="cuda"), torch.zeros((5, 12), dtype=torch.int32, device="cuda"),
                    torch.zeros((12, 5), dtype=torch.int64, device="cuda").t(), torch.zeros((5, 12), dtype=torch.int64)):
            with pytest.raises(ValueError):
                s.held_matrix(5, 12, out=bad)
        got.update(table=table)
    _go(sc, "sample x library id", call, check)
    # the cells are where held_cell says
    assert all(dev.held_cell(k, 4, 5, 12) == ((k >> 4) - 1) * 12 + (k & 15) - 1 for k, _ in got["table"])
    sc.close()
    for p in ps:
        p.close()


# ---- 7. three columns ----
def _three(s, pats, texts, lines3, library=None):
    """hold(lines of texts[0]), append(texts[1]), append(texts[2]; library: assigned to it) -> the held column the rule expects."""
    held = _lines_column(s, pats, texts[0], lines3[0], "column 0")
    s.tally_hold(texts[0], source="anchored")
    col = _lines_column(s, pats, texts[1], lines3[1], "column 1")
    s.tally_hold_append(texts[1], source="anchored")
    held = py_append(held, col)[0]
    col = _lines_column(s, pats, texts[2], lines3[2], "column 2")
    s.tally_hold_append(texts[2], source="anchored", library=library is not None)
    if library is not None:
        col = [(ln, library.index(x) + 1) for ln, x in zip(range(1, len(col) + 1), lines3[2])]
    held = py_append(held, col, width=len(library).bit_length() if library is not None else None)[0]
    assert _held_arrays(s) == held
    return held


def test_three_columns_with_one_and_two_member_columns(gpu, capi, pats):
    from seeq_amd import device as dev
    rng = random.Random(47)
    pools = _pool(rng, 4, 3), _pool(rng, 5, 4), _pool(rng, 6, 5)
    n = T + 200
    lines3 = [[b"ANA" if c == 0 and i % 29 == 7 else rng.choice(p) for i in range(n)] for c, p in enumerate(pools)]
    texts = [_cuda(_text(x)) for x in lines3]
    sc = dev.Scanner()

    def call(s):
        held = _three(s, pats, texts, lines3)
        assert s.hold_columns() == [7, 9, 11]
        return held, _twice(s, 1), _twice(s, 2)

    def check(s, out):
        held, one, two = out
        res = s.tally_held(2)
        cnt, table, rows = _same(s, res, held, 2)
        assert res["table"].tobytes() == two["table"].tobytes() and res["rows"].tobytes() == two["rows"].tobytes()
        assert cnt["shift"] == 20 and len(rows) == 4 and 100 < len(table) <= 4 * 5 * 6 and cnt["passes"] == 4
        res = s.tally_held(1)
        cnt, table1, rows = _same(s, res, held, 1)
        assert res["table"].tobytes() == one["table"].tobytes() and res["rows"].tobytes() == one["rows"].tobytes()
        assert cnt["shift"] == 11 and len(rows) == 4 * 5 and table1 == table and max(r[3] for r in rows) == 6
        # raw sequence columns fall outside every matrix: the sparse tables serve them
        dense = _matrix(s, table, 11, 64, 64)
        assert dense["ninside"] == 0 and dense["outside_reads"] == cnt["ncounted"]
    _go(sc, "three columns", call, check)
    sc.close()


# ---- 8. a composed word of 63 bits ----
def test_a_word_of_63_bits_takes_eight_passes(gpu, capi, pats):
    """16 bases (33 bits), 12 bases (25) and the ids of a library of 20 entries (5): 63 bits, bit 62 set in every key."""
    from seeq_amd import device as dev
    rng = random.Random(48)
    lib = _pool(rng, 20, 8)
    pools = _pool(rng, 6, 16), _pool(rng, 5, 12), lib
    n = T + 100
    lines3 = [[rng.choice(p) for _ in range(n)] for p in pools]
    texts = [_cuda(_text(x)) for x in lines3]
    sc = dev.Scanner()
    sc.set_library([g.decode() for g in lib], max_mismatch=0)

    def call(s):
        held = _three(s, pats, texts, lines3, library=lib)
        assert s.hold_columns() == [33, 25, 5]
        return held, _twice(s, 2)

    def check(s, out):
        held, res = out
        cnt, table, rows = _same(s, res, held, 2)
        assert cnt["key_bits"] == 63 and cnt["passes"] == 8 and cnt["shift"] == 30 and all(k >> 62 == 1 for k, _ in table) and len(rows) == 6
        assert cnt["ncounted"] == n and len(table) > 300
    _go(sc, "63 bits", call, check)
    sc.close()


# ---- 9. rows against the tiles of the sorted array ----
def test_a_row_that_spans_tiles_and_a_row_head_at_the_seam(gpu, capi, pats):
    """24 keyless records and a first row of 1 000 reads: the second row's head is sorted item 1 024 exactly, the first item of the second
    tile, and its 1 500 items reach into the third."""
    from seeq_amd import device as dev
    rng = random.Random(49)
    r0, r1, r2 = b"AAA", b"AAC", b"AAT"
    assert _key(r0) < _key(r1) < _key(r2)
    p1 = _pool(rng, 30, 4)
    col0 = [b"ANA"] * 24 + [r0] * (T - 24) + [r1] * 1500 + [r2] * 50
    rng.shuffle(col0)
    col1 = [rng.choice(p1) for _ in col0]
    t0, t1 = _cuda(_text(col0)), _cuda(_text(col1))
    sc = dev.Scanner()

    def call(s):
        held0 = _lines_column(s, pats, t0, col0, "rows")
        s.tally_hold(t0, source="anchored")
        col = _lines_column(s, pats, t1, col1, "columns")
        s.tally_hold_append(t1, source="anchored")
        held = py_append(held0, col)[0]
        assert _held_arrays(s) == held
        return held, _twice(s, 1)

    def check(s, out):
        held, res = out
        words = sorted(k for _, k in held)
        at = next(i for i, w in enumerate(words) if w >> 9 == _key(r1))
        assert at == T and words[at - 1] >> 9 == _key(r0) and words[2 * T] >> 9 == _key(r1) and words[T + 1499] >> 9 == _key(r1)
        cnt, table, rows = _same(s, res, held, 1)
        assert [(r[0], r[1]) for r in rows] == [(_key(r0), T - 24), (_key(r1), 1500), (_key(r2), 50)] and cnt["nkeyless"] == 24
    _go(sc, "rows against the tiles", call, check)
    sc.close()


# ---- 10. more than 256 tiles ----
def test_more_than_256_tiles(gpu, capi, pats):
    """257 x 1 024 + 1 held records: the one-workgroup tops take a second round of 256 tiles; 3 000 distinct keys: the key table itself
    is more than one tile of the table kernel's grid."""
    from seeq_amd import device as dev
    rng = random.Random(50)
    n = 257 * T + 1
    pool = _pool(rng, 3000, 8)
    keys = [_key(x) for x in pool]
    pick = [rng.randrange(3000) for _ in range(n)]
    lines = [b"ACGTNCGT" if i % 97 == 11 else pool[p] for i, p in enumerate(pick)]
    t = _cuda(_text(lines))
    sc = dev.Scanner()

    def call(s):
        from seeq_amd import device as dev
        assert s.scan_tensor(pats["N"], t, SQ_BEST, dev.WANT_RECORDS)["nrecords"] == n
        cut = s.anchor(t, source="hits", anchor="line", skip=0, length=8, reach=64, copy=False)
        assert cut["nkept"] == n and cut["span_bytes"] == 8 * n
        hold = s.tally_hold(t, source="anchored")
        assert hold["nspans"] == n and hold["nforeign"] == len(range(11, n, 97)) and hold["key_bits"] == 17
        h = s.held()
        exp = np.array([0 if i % 97 == 11 else keys[p] for i, p in enumerate(pick)], dtype=np.uint64)
        assert np.array_equal(h["lines"], np.arange(1, n + 1)) and np.array_equal(h["keys"], exp)
        return list(zip(range(1, n + 1), exp.tolist())), s.tally_held(0)

    def check(s, out):
        held, res = out
        cnt, table, _ = _same(s, res, held, 0)
        assert cnt["ndistinct"] == 3000 and cnt["passes"] == 3 and cnt["nkeyless"] == len(range(11, n, 97)) and cnt["nrepeat"] == 0
    _go(sc, "257 tiles and one record", call, check)
    sc.close()


# ---- 11. what the held tally leaves alone, and what it replaces ----
def _raw_dense(sc, capi, ptr, nrows, ncols):
    cnt = capi.seeqdev_tally_dense_counts_t()
    C.set_errno(0)
    rc = sc._lib.seeqdevScanTallyHeldDense(sc._h, C.c_void_p(ptr), nrows, ncols, C.byref(cnt))
    return rc, C.get_errno()


def _raw_held(sc, capi, m):
    cnt = capi.seeqdev_tally_held_counts_t()
    C.set_errno(0)
    rc = sc._lib.seeqdevScanTallyHeld(sc._h, m, C.byref(cnt))
    return rc, C.get_errno()


def test_the_held_tally_reads_the_held_column_and_replaces_the_tally_table(gpu, capi, pats):
    import torch
    from seeq_amd import device as dev
    rng = random.Random(51)
    codes, lib, us = _pool(rng, 5, 16), _pool(rng, 12, 20), _pool(rng, 7, 12)
    lines, dheld, gcol, ucol = _screen(rng, T + 200, codes, lib, umis=us)
    t = _cuda(_text(lines))
    ps = [dev.Pattern(c.decode(), 0) for c in codes]
    sc = dev.Scanner()
    sc.set_library([g.decode() for g in lib], max_mismatch=0)
    held = _screen_hold(sc, pats, ps, t, dheld, gcol, lib)
    _cut(sc, pats["C"], pats["D"], t, ucol, "UMIs")
    grouped = sc.tally_grouped(t)
    collapse = sc.tally_collapse()
    plain = sc.tally(t)
    assert grouped["npairs"] > 100 and collapse["npairs"] == grouped["npairs"] and plain["ndistinct"] == 7

    def state(s):
        h = s.held()
        return dict(lines=h["lines"].tobytes(), keys=h["keys"].tobytes(), columns=h["columns"], pairs=s.tally_pairs_table(grouped["npairs"]).tobytes(),
                    groups=s.tally_groups_table(grouped["ngroups"]).tobytes(), parent=s.tally_parents_table(collapse["npairs"]).tobytes(),
                    rows=s.tally_collapse_table(collapse["ngroups"]).tobytes(), inserts=s.insert_records(len(ucol)).tobytes(),
                    offsets=s.insert_offsets(len(ucol)).tobytes(), library=s.library_edits())
    before = state(sc)
    res = _twice(sc, 1)
    cnt, table, rows = _same(sc, res, held, 1)
    assert state(sc) == before
    assert sc.tally_table(cnt["ndistinct"]).tobytes() == res["table"].tobytes() and cnt["ndistinct"] != plain["ndistinct"]      # the tally table is replaced
    _matrix(sc, table, 4, 5, 12)
    assert state(sc) == before
    small = torch.zeros((5, 12), dtype=torch.int64, device="cuda")
    # a refused held tally changes nothing: the table and the matrix are still served
    for m in (-1, 2, 3, 8):
        assert _raw_held(sc, capi, m) == (-1, errno.EINVAL) and "member columns" in capi.error_text()
    _matrix(sc, table, 4, 5, 12, out=small)
    assert _raw_dense(sc, capi, small.data_ptr(), 1 << 14, (1 << 14) + 1) == (-1, errno.E2BIG)
    assert _raw_dense(sc, capi, small.data_ptr(), 0, 12) == (-1, errno.EINVAL) and _raw_dense(sc, capi, small.data_ptr(), 5, 0) == (-1, errno.EINVAL)
    # a plain tally, or a library tally, in between: the tally table is theirs, the matrix is refused
    for other in (lambda: sc.tally(t), lambda: sc.tally_library(t)):
        assert _raw_dense(sc, capi, small.data_ptr(), 5, 12) == (0, 0)
        other()
        assert _raw_dense(sc, capi, small.data_ptr(), 5, 12) == (-1, errno.EINVAL) and "held tally" in capi.error_text()
        with pytest.raises(dev.SeeqDeviceError):
            sc.held_matrix(5, 12)
        _same(sc, sc.tally_held(1), held, 1)
    # member_columns 0: a table, no rows, no matrix
    flat = sc.tally_held(0)
    assert _same(sc, flat, held, 0)[1] == table and flat["nrows"] == 0
    assert _raw_dense(sc, capi, small.data_ptr(), 5, 12) == (-1, errno.EINVAL) and "member columns" in capi.error_text()
    assert state(sc) == before
    # a further append, then a new held tally: the new word
    _demux(sc, ps, t, dheld)
    sc.tally_hold_append(source="demux")
    held3 = py_append(held, dheld)[0]
    assert _held_arrays(sc) == held3 and sc.hold_columns() == [3, 4, 3]
    cnt1, table1, rows1 = _same(sc, sc.tally_held(1), held3, 1)
    cnt2, table2, rows2 = _same(sc, sc.tally_held(2), held3, 2)
    assert (cnt1["shift"], cnt2["shift"]) == (3, 7) and table1 == table2 != table and len(rows2) == 5 and len(rows1) == len(table) == len(table1)
    _matrix(sc, table2, 7, 5, 12 << 3 | 5)
    sc.close()
    for p in ps:
        p.close()


# ---- 12. stream order ----
def test_hold_held_tally_and_matrix_on_a_callers_non_blocking_stream(gpu, capi, pats):
    """A Scanner bound to the caller's non-blocking stream: hold, append, held tally, held_matrix into a tensor the caller then reads on that
    stream.  The caller's own last writer of that tensor is still pending on the stream when held_matrix gets control (a device-side delay,
    then a fill with -1): a memset or a scatter that ran off the stream would be overwritten by it."""
    import torch
    from seeq_amd import device as dev
    rng = random.Random(52)
    codes, lib = _pool(rng, 5, 16), _pool(rng, 12, 20)
    lines, dheld, gcol, _ = _screen(rng, T + 100, codes, lib)
    side = torch.cuda.Stream()
    flags = L.stream_flags(side)
    assert side.cuda_stream != 0 and (flags is None or flags & L.HIP_STREAM_NON_BLOCKING)
    delay = L.Delay()
    with torch.cuda.stream(side):
        t = _cuda(_text(lines))
        out = torch.zeros((5, 12), dtype=torch.int64, device="cuda")
    side.synchronize()
    ps = [dev.Pattern(c.decode(), 0) for c in codes]
    sc = dev.Scanner(side.cuda_stream)
    try:
        sc.set_library([g.decode() for g in lib], max_mismatch=0)
        held = _screen_hold(sc, pats, ps, t, dheld, gcol, lib)
        res = sc.tally_held(1)
        cnt, table, rows = _same(sc, res, held, 1)
        with torch.cuda.stream(side):
            torch.cuda._sleep(delay.cycles(4 * L.MIN_DELAY_MS))
            out.fill_(-1)
        assert not side.query(), "the side stream has run dry before held_matrix got control: the case proves nothing"
        got, dense = sc.held_matrix(5, 12, out=out)
        with torch.cuda.stream(side):
            seen = got.clone()
        side.synchronize()
        cells, exp = py_dense(table, 4, 5, 12)
        host = np.zeros(60, dtype=np.int64)
        for cell, count in cells.items():
            host[cell] = count
        assert dense == exp and np.array_equal(seen.cpu().numpy().reshape(-1), host) and int(host.min()) >= 0 and int(host.sum()) == cnt["ncounted"] > T // 2
    finally:
        torch.cuda.synchronize()
        sc.close()
        for p in ps:
            p.close()
