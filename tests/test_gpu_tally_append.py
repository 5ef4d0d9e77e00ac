"""GPU (-m gpu): key columns appended to the held column (seeqdevScanTallyHoldAppend / seeqdevScanTallyHoldAppendLibrary;
seeq_tally_append.h: the new column by the hold's own kernels, the join by k_tally_hold_join) against the rule restated in Python
(test_tally_append_host.py) over what was PLANTED.  Reads are built as test_gpu_tally_grouped.py builds them, with a third flanked part in
front: prefix + flank E + cell + flank F + spacer + flank A + guide + flank B + spacer + flank C + UMI + flank D + suffix, the flanks
searched at distance 0, and every case first asserts that each inserts call (scan, demultiplex, gate) found exactly what was planted: a
vacuous case fails.  Cells are 16 bases (33 bits), guides 12 (25 bits) unless a case says otherwise: the widths must sum to at most 63."""
import ctypes as C
import errno
import random

import numpy as np
import pytest

import late_text as L
import text_window as W
from oracle.pyoracle import SQ_ALL, SQ_BEST
from test_gpu_strands import _line_offsets, _step
from test_gpu_tally_grouped import FA, FB, FC, FD, T, _cuda, _cut, _held_of, _kmer, _same, _text
from test_tally_append_host import py_append
from test_tally_collapse_host import DIRECTIONAL, py_collapse
from test_tally_host import OK, py_key

pytestmark = pytest.mark.gpu
FE, FF = "TGCAAGGTCATCGGATACCT", "GTTACGACCTAGGCATTCGA"      # around the cell barcode
HA, HB = "CATGNNNNGTAC", "ACCTNNNNAGGT"                     # two patterns whose matches (12 bytes) differ in four bytes (distance 0, SQ_ALL)
APPEND = ("nrecords", "nbefore", "nheld", "ndropped", "width", "key_bits", "ncolumns")

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
def fl(gpu):
    from seeq_amd import device as dev
    ps = {k: dev.Pattern(v, 0) for k, v in dict(A=FA, B=FB, C=FC, D=FD, E=FE, F=FF, HA=HA, HB=HB).items()}
    yield ps
    for p in ps.values():
        p.close()


# ---- reads ----
def _reads3(spec, seed=1):
    """spec: per line (cell, guide, umi), bytes or None for a line without that part -> the lines (bytes)."""
    rng = random.Random(seed)
    bases = lambda m: bytes(rng.choice(b"ACGT") for _ in range(m))      # noqa: E731
    lines = []
    for row in spec:
        parts = [bases(rng.randrange(6))]
        for part, (left, right) in zip(row, ((FE, FF), (FA, FB), (FC, FD))):
            if part is not None:
                parts += [left.encode(), part, right.encode()]
            parts.append(bases(rng.randrange(3, 8)))
        lines.append(b"".join(parts))
    return lines


def _fastq3(lines, low=None):
    """Four-line records around the lines, the quality bytes high ('I') but for `low`: {record (1-based): (first, end) byte positions of
    the sequence line whose quality is '#'}."""
    out = []
    for i, ln in enumerate(lines):
        q = bytearray(b"I" * len(ln))
        if low and i + 1 in low:
            a, b = low[i + 1]
            q[a:b] = b"#" * (b - a)
        out += [b"@r%d" % (i + 1), ln, b"+", bytes(q)]
    return _text(out)


def _columns(spec):
    return tuple([(i + 1, row[c]) for i, row in enumerate(spec) if row[c] is not None] for c in range(3))


def _pool(rng, n, m):
    out = []
    while len(out) < n:
        s = _kmer(rng.getrandbits(2 * m), m)
        if s not in out:
            out.append(s)
    return out


def _held_arrays(s):
    h = s.held()
    assert h["nrecords"] == len(h["lines"]) == len(h["keys"]) and h["columns"] == s.hold_columns()
    return list(zip(h["lines"].tolist(), h["keys"].tolist()))


def _counts(app):
    return {k: app[k] for k in APPEND}


def _run3(sc, fl, texts, cols, what, opt=SQ_BEST, between=None):
    """hold(cells of texts[0]), append(guides of texts[1]), grouped(UMIs of texts[2]); every step against what was planted and the rule.
    -> dict: the grouped result, the held column afterwards, the append's dict, the widths."""
    cells, guides, umis = cols
    held0, hcnt = _held_of(cells)
    col, ccnt = _held_of(guides)
    exp_held, acnt = py_append(held0, col)
    acnt["ncolumns"] = 2

    def call(s):
        _cut(s, fl["E"], fl["F"], texts[0], cells, what + ": cells", opt)
        hold = s.tally_hold(texts[0])
        if between:
            between(s)
        _cut(s, fl["A"], fl["B"], texts[1], guides, what + ": guides", opt)
        app = s.tally_hold_append(texts[1])
        held = _held_arrays(s)
        widths = s.hold_columns()
        _cut(s, fl["C"], fl["D"], texts[2], umis, what + ": UMIs", opt)
        return hold, app, held, widths, s.tally_grouped(texts[2])
    got = {}

    def check(s, out):
        hold, app, held, widths, res = out
        assert hold == hcnt
        assert app["column"] == ccnt and _counts(app) == acnt
        assert app["nbefore"] == app["nheld"] + app["ndropped"] == hcnt["nheld"]
        assert held == exp_held and widths == [hcnt["key_bits"], ccnt["key_bits"]]
        _same(res, exp_held, umis)
        got.update(res=res, held=held, app=app, widths=widths)
    _go(sc, what, call, check)
    return got


# ---- 1. three planted columns against the host join ----
def _spec_three(nh, more, seed):
    """nh lines carry a cell; `more`: the guide column has more records than the cell column (lines without a cell), else fewer."""
    rng = random.Random(seed)
    cells, guides, umis = _pool(rng, 6, 16), _pool(rng, 5, 12), _pool(rng, 9, 12)
    spec = []
    for i in range(nh):
        g = rng.choice(guides) if more or i % 3 else None                                  # lines missing from the guide column
        spec.append((rng.choice(cells), g, rng.choice(umis) if i % 11 else None))
    spec[1] = (b"ACGTACGTNCGTACGT", guides[0], umis[0])                                      # a foreign and a long span in each column
    spec[2] = (_kmer(rng.getrandbits(64), 32), guides[1], umis[1])
    spec[3] = (cells[0], b"ACGTACNTACGT", umis[2])
    spec[4] = (cells[1], _kmer(rng.getrandbits(64), 32), umis[3])
    spec += [(None, rng.choice(guides), rng.choice(umis)) for _ in range(nh // 2 + 37 if more else 19)]      # lines missing from the cell column
    rng.shuffle(spec)
    return spec


@pytest.mark.parametrize("nh,more", [(T - 1, True), (T, False), (T + 1, True), (2 * T + 3, False)])
def test_three_planted_columns_against_the_host_join(gpu, capi, fl, nh, more):
    """Held records around the tile T and beyond two tiles; the appended column has more records than the held one, or fewer; lines are
    missing from either; a foreign and a long span in each.  hold_split gives back the planted cells and guides."""
    from seeq_amd import device as dev
    spec = _spec_three(nh, more, nh)
    cols = _columns(spec)
    assert len(cols[0]) == nh and (len(cols[1]) > nh) == more
    t = _cuda(_text(_reads3(spec, nh)))
    sc = dev.Scanner()
    got = _run3(sc, fl, (t, t, t), cols, "%d held records" % nh)
    app, res = got["app"], got["res"]
    assert got["widths"] == [33, 25] and app["key_bits"] == 58 and app["ndropped"] >= 2 and app["column"]["nlong"] == app["column"]["nforeign"] == 1
    assert res["passes"] == 4 + 8                           # 12-base members (25 bits), then the 58 bits of (cell, guide)
    planted = {(py_key(c)[1], py_key(g)[1]) for c, g, u in spec if None not in (c, g, u) and py_key(c)[0] == py_key(g)[0] == py_key(u)[0] == OK}
    c0, c1 = dev.hold_split(res["groups"]["group"], sc.hold_columns())
    assert set(zip(c0.tolist(), c1.tolist())) == planted and len(planted) == len(res["groups"]) > 20
    p0, p1 = dev.hold_split(res["pairs"]["group"], got["widths"])
    assert set(zip(p0.tolist(), p1.tolist())) == planted
    sc.close()


# ---- 2. SQ_ALL: several records per line in either column ----
def test_several_records_per_line_in_both_columns_the_first_of_the_new_column_decides(gpu, capi, fl):
    from seeq_amd import device as dev
    rng = random.Random(22)
    us = _pool(rng, 6, 12)
    lines, colh, coln, umis = [], [], [], []
    for i in range(T + 200):
        hs = [b"CATG" + _kmer(rng.randrange(8), 4) + b"GTAC" for _ in range(rng.choice([0, 1, 2, 3]))]
        ns = [b"ACCT" + _kmer(rng.randrange(8), 4) + b"AGGT" for _ in range(rng.choice([0, 1, 1, 2, 3]))]
        u = rng.choice(us + [None])
        lines.append(b"GT" + b"".join(h + b"TTA" for h in hs) + b"".join(n + b"TTA" for n in ns) + (FC.encode() + u + FD.encode() if u is not None else b"") + b"AC")
        colh += [(i + 1, h) for h in hs]
        coln += [(i + 1, n) for n in ns]
        if u is not None:
            umis.append((i + 1, u))
    buf = _text(lines)
    offs = _line_offsets(buf)
    t = _cuda(buf)
    held0, hcnt = _held_of(colh)
    col, ccnt = _held_of(coln)
    exp_held, acnt = py_append(held0, col)
    acnt["ncolumns"] = 2
    sc = dev.Scanner()

    def records(s, pat, column):
        cnt = s.scan_tensor(pat, t, SQ_ALL, dev.WANT_RECORDS)
        rec = s.records(cnt["nrecords"]).tolist()
        assert [(r[0], buf[offs[r[0]] + r[1]:offs[r[0]] + r[2]]) for r in rec] == column

    def call(s):
        records(s, fl["HA"], colh)
        hold = s.tally_hold(t, source="hits")
        records(s, fl["HB"], coln)
        app = s.tally_hold_append(t, source="hits")
        held = _held_arrays(s)
        _cut(s, fl["C"], fl["D"], t, umis, "UMIs")
        return hold, app, held, s.tally_grouped(t)

    def check(s, out):
        hold, app, held, res = out
        assert hold == hcnt and app["column"] == ccnt and _counts(app) == acnt and held == exp_held
        _same(res, exp_held, umis)
    _go(sc, "SQ_ALL in both columns", call, check)
    first = {}
    for ln, n in coln:
        first.setdefault(ln, n)
    assert sum(1 for ln, n in coln if first[ln] != n) > 100      # later records of a line with another key: they must not decide
    per_line = {}
    for ln, k in exp_held:
        per_line.setdefault(ln, []).append(k)
    assert sum(1 for ks in per_line.values() if len(ks) >= 2 and all(ks)) > 100      # every held record of a line is composed
    assert acnt["ndropped"] > 50 and acnt["key_bits"] == 50
    sc.close()


# ---- 3. the library on the appended column ----
def _sub(seq, at, base):
    return seq[:at] + bytes([base]) + seq[at + 1:]


def _assign(lib, seq):
    """The library's rule (seeq_amd.h), restated: exact -> id; else exactly one entry one substitution away -> its id; else 0."""
    if py_key(seq)[0] != OK:
        return 0
    if seq in lib:
        return lib.index(seq) + 1
    near = [i + 1 for i, e in enumerate(lib) if len(e) == len(seq) and sum(1 for x, y in zip(e, seq) if x != y) == 1]
    return near[0] if len(near) == 1 else 0


def test_a_library_on_the_appended_column(gpu, capi, fl):
    """Guides with planted single substitutions: the composed groups are those of the clean guides; a guide one substitution from two
    entries (ambiguous) and an unknown one are dropped.  `column` is what tally_hold_library reports for the same source."""
    from seeq_amd import device as dev
    rng = random.Random(23)
    lib = _pool(rng, 12, 20)
    twin = _sub(_sub(lib[0], 3, ord("A") if lib[0][3] != ord("A") else ord("C")), 11, ord("G") if lib[0][11] != ord("G") else ord("T"))
    lib.append(twin)                                        # two positions from lib[0]: a read with one of them changed is one away from both
    cells, umis = _pool(rng, 5, 16), _pool(rng, 7, 12)
    noisy, clean = [], []
    for i in range(T + 300):
        g = rng.choice(lib)
        kind = rng.choice(["exact"] * 5 + ["sub", "sub", "both", "unknown", "none"])
        seen = g
        if kind == "sub":
            at = rng.randrange(20)
            seen = _sub(g, at, rng.choice([b for b in b"ACGT" if b != g[at]]))
        elif kind == "both":
            seen = _sub(lib[0], 3, twin[3])
        elif kind == "unknown":
            seen = _kmer(rng.getrandbits(40), 20)
        elif kind == "none":
            seen = None
        ident = _assign(lib, seen) if seen is not None else 0
        c, u = rng.choice(cells), rng.choice(umis)
        noisy.append((c, seen, u))
        clean.append((c, lib[ident - 1] if ident else None, u))
    sc = dev.Scanner()
    sc.set_library([g.decode() for g in lib], max_mismatch=1)
    tables = {}
    for name, spec in (("noisy", noisy), ("clean", clean)):
        cols = _columns(spec)
        cells_c, guides, members = cols
        t = _cuda(_text(_reads3(spec, 23)))
        held0, hcnt = _held_of(cells_c)
        col = [(ln, _assign(lib, g)) for ln, g in guides]
        exp_held, acnt = py_append(held0, col, width=len(lib).bit_length())
        acnt["ncolumns"] = 2

        def call(s):
            _cut(s, fl["E"], fl["F"], t, cells_c, name + ": cells")
            hold = s.tally_hold(t)
            _cut(s, fl["A"], fl["B"], t, guides, name + ": guides")
            app = s.tally_hold_append(t, library=True)
            held = _held_arrays(s)
            _cut(s, fl["C"], fl["D"], t, members, name + ": UMIs")
            return hold, app, held, s.tally_grouped(t)

        def check(s, out):
            hold, app, held, res = out
            assert hold == hcnt and _counts(app) == acnt and held == exp_held and s.hold_columns() == [33, 4]
            tables[name] = (_same(res, exp_held, members), app)
        _go(sc, "library append, %s guides" % name, call, check)
        if name == "noisy":
            other = dev.Scanner()
            other.set_library([g.decode() for g in lib], max_mismatch=1)
            _cut(other, fl["A"], fl["B"], t, guides, "guides on a fresh context")
            assert tables[name][1]["column"] == other.tally_hold_library(t)
            other.close()
    column = tables["noisy"][1]["column"]
    assert column["ncorrected"] > 100 and column["nambiguous"] > 50 and column["nunknown"] > 50 and column["key_bits"] == 4
    assert tables["noisy"][0] == tables["clean"][0]          # the same pair and group tables
    assert tables["noisy"][1]["ndropped"] == column["nambiguous"] + column["nunknown"] + sum(1 for _, g, _ in noisy if g is None)
    c0, c1 = dev.hold_split([g[0] for g in tables["noisy"][0][1]], [33, 4])
    assert set(c1.tolist()) <= set(range(1, len(lib) + 1)) and len(set(c1.tolist())) == len(lib)
    sc.close()


# ---- 4. demux records as the first column and as the appended one ----
def test_demux_first_and_demux_appended(gpu, capi, fl):
    from seeq_amd import device as dev
    rng = random.Random(24)
    codes = _pool(rng, 5, 16)
    gs, us = _pool(rng, 5, 12), _pool(rng, 6, 12)
    lines, assigned, guides, umis, ambiguous = [], {}, [], [], 0
    for i in range(T + 300):
        kind = rng.choice(["one"] * 8 + ["two", "none"])
        head = b"TT"
        if kind == "one":
            k = rng.randrange(5)
            head += codes[k] + b"CA"
            assigned[i + 1] = k + 1
        elif kind == "two":
            a, b = rng.sample(range(5), 2)
            head += codes[a] + b"CA" + codes[b]
            assigned[i + 1] = 0
            ambiguous += 1
        g, u = rng.choice(gs + [None]), rng.choice(us)
        lines.append(head + b"AC" + (FA.encode() + g + FB.encode() if g is not None else b"") + b"GT" + FC.encode() + u + FD.encode() + b"TG")
        if g is not None:
            guides.append((i + 1, g))
        umis.append((i + 1, u))
    t = _cuda(_text(lines))
    ps = [dev.Pattern(c.decode(), 0) for c in codes]
    dheld = sorted(assigned.items())
    dcnt = dict(nspans=len(dheld), nheld=len(dheld) - ambiguous, nlong=0, nforeign=0, nambiguous=ambiguous, max_len=0, key_bits=3)
    gheld, gcnt = _held_of(guides)
    sc = dev.Scanner()

    def demux(s):
        rec = s.demux_tensor(ps, t)["records"]
        assert rec["line"].tolist() == [ln for ln, _ in dheld]
        assert [(int(p) + 1) if m else 0 for p, m in zip(rec["pattern"], rec["margin"])] == [k for _, k in dheld]

    def demux_first(s):
        demux(s)
        hold = s.tally_hold(source="demux")
        _cut(s, fl["A"], fl["B"], t, guides, "guides")
        app = s.tally_hold_append(t)
        held = _held_arrays(s)
        _cut(s, fl["C"], fl["D"], t, umis, "UMIs")
        return hold, app, held, s.tally_grouped(t)

    def demux_appended(s):
        _cut(s, fl["A"], fl["B"], t, guides, "guides")
        hold = s.tally_hold(t)
        demux(s)
        app = s.tally_hold_append(source="demux")
        held = _held_arrays(s)
        _cut(s, fl["C"], fl["D"], t, umis, "UMIs")
        return hold, app, held, s.tally_grouped(t)

    for what, call, first, fcnt, second, scnt in (("demux first", demux_first, dheld, dcnt, gheld, gcnt), ("demux appended", demux_appended, gheld, gcnt, dheld, dcnt)):
        exp_held, acnt = py_append(first, second)
        acnt["ncolumns"] = 2

        def check(s, out):
            hold, app, held, res = out
            assert hold == fcnt and app["column"] == scnt and _counts(app) == acnt and held == exp_held
            assert s.hold_columns() == [fcnt["key_bits"], scnt["key_bits"]] and app["key_bits"] == 28
            _same(res, exp_held, umis)
            assert res["nungrouped"] >= ambiguous > 50
        _go(sc, what, call, check)
        dropped = [ln for (ln, k0), (_, k1) in zip(first, exp_held) if k0 and not k1]
        assert acnt["ndropped"] == len(dropped) > 20
        if what == "demux appended":
            assert sum(1 for ln in dropped if assigned.get(ln) == 0) > 20      # ambiguous lines are dropped
    sc.close()
    for p in ps:
        p.close()


# ---- 5. the collapse behind a two-column hold ----
def test_collapse_behind_a_two_column_hold(gpu, capi, fl):
    """The same UMI, one substitution apart, under two different (cell, guide) groups stays two roots; under the same group it is
    absorbed.  Against the rule of test_tally_collapse_host.py over the pair table of the composed keys."""
    from seeq_amd import device as dev
    rng = random.Random(25)
    cells, guides = _pool(rng, 3, 16), _pool(rng, 3, 12)
    u = b"ACGTTGCAAGCT"
    u1 = _sub(u, 5, ord("A"))
    spec = [(cells[0], guides[0], u)] * 10 + [(cells[0], guides[0], u1)]                      # same group: absorbed
    spec += [(cells[0], guides[1], u)] * 10 + [(cells[1], guides[1], u1)]                     # another cell: a root
    spec += [(cells[1], guides[0], u)] * 10 + [(cells[1], guides[2], u1)]                     # another guide: a root
    umis = _pool(rng, 12, 12)
    for _ in range(T + 50):
        m = rng.choice(umis)
        if rng.random() < 0.2:
            at = rng.randrange(12)
            m = _sub(m, at, rng.choice([b for b in b"ACGT" if b != m[at]]))
        spec.append((rng.choice(cells), rng.choice(guides), m))
    rng.shuffle(spec)
    t = _cuda(_text(_reads3(spec, 25)))
    sc = dev.Scanner()
    got = _run3(sc, fl, (t, t, t), _columns(spec), "collapse behind two columns")
    pairs = [tuple(int(x) for x in r) for r in got["res"]["pairs"]]
    parent, rows = py_collapse(pairs, DIRECTIONAL)
    col = sc.tally_collapse()
    assert col["parent"].tolist() == parent and [tuple(int(x) for x in r) for r in col["groups"]] == rows
    assert col["nabsorbed"] == sum(1 for i, p in enumerate(parent) if p != i) > 10
    key = lambda c, g: py_key(c)[1] << 25 | py_key(g)[1]      # noqa: E731
    at = {(g, m): i for i, (g, m, _) in enumerate(pairs)}
    same, k1 = at[key(cells[0], guides[0]), py_key(u1)[1]], py_key(u1)[1]
    assert parent[same] == at[key(cells[0], guides[0]), py_key(u)[1]]
    for c, g in ((cells[1], guides[1]), (cells[1], guides[2])):
        i = at[key(c, g), k1]
        assert parent[i] == i and col["parent"][i] == i
    sc.close()


# ---- 6. the appended column from the quality gate's output ----
def test_the_appended_column_from_gated_records(gpu, capi, fl):
    from seeq_amd import device as dev
    rng = random.Random(26)
    cells, gs, us = _pool(rng, 5, 16), _pool(rng, 5, 12), _pool(rng, 7, 12)
    spec = [(rng.choice(cells), rng.choice(gs), rng.choice(us)) for _ in range(T + 100)]
    lines = _reads3(spec, 26)
    low = {}
    for i, ln in enumerate(lines):
        if i % 4 == 1:                                      # one low base under the guide
            at = ln.index(FA.encode()) + 20 + rng.randrange(12)
            low[i + 1] = (at, at + 1)
        elif i % 4 == 2:                                    # a low base in the flank beside it: the guide passes
            at = ln.index(FA.encode()) + 19
            low[i + 1] = (at, at + 1)
    t = _cuda(_fastq3(lines, low))
    cols = _columns(spec)
    cells_c, guides, umis = cols
    passed = [(ln, g) for ln, g in guides if (ln - 1) % 4 != 1]
    held0, hcnt = _held_of(cells_c)
    col, ccnt = _held_of(passed)
    exp_held, acnt = py_append(held0, col)
    acnt["ncolumns"] = 2
    opt = SQ_BEST | dev.SEEQDEV_FASTQ
    sc = dev.Scanner()

    def call(s):
        _cut(s, fl["E"], fl["F"], t, cells_c, "cells", opt)
        hold = s.tally_hold(t)
        _cut(s, fl["A"], fl["B"], t, guides, "guides", opt)
        gate = s.quality_gate(t, min_qual=20)
        assert gate["npassed"] == len(passed) and gate["nlow"] == len(guides) - len(passed) and gate["records"][:, 0].tolist() == [ln for ln, _ in passed]
        _cut(s, fl["C"], fl["D"], t, umis, "UMIs", opt)      # (the gated arrays are copies: another inserts call in between)
        app = s.tally_hold_append(t, source="gated")
        return hold, app, _held_arrays(s), s.tally_grouped(t)

    def check(s, out):
        hold, app, held, res = out
        assert hold == hcnt and app["column"] == ccnt and _counts(app) == acnt and held == exp_held
        _same(res, exp_held, umis)
        assert app["ndropped"] == len(guides) - len(passed) > 200
    _go(sc, "gated source", call, check)
    sc.close()


# ---- 7. two buffers ----
def _two_buffers(seed, n):
    """-> (single FASTQ buffer, FASTQ of cell + UMI, FASTQ of the guide alone, the columns): the same records, numbered alike."""
    rng = random.Random(seed)
    cells, gs, us = _pool(rng, 5, 16), _pool(rng, 5, 12), _pool(rng, 7, 12)
    spec = [(rng.choice(cells + [None]), rng.choice(gs + [None]), rng.choice(us + [None])) for _ in range(n)]
    one = _fastq3(_reads3(spec, seed))
    read1 = _fastq3(_reads3([(c, None, u) for c, _, u in spec], seed + 1))
    read2 = _fastq3(_reads3([(None, g, None) for _, g, _ in spec], seed + 2))
    return one, read1, read2, _columns(spec)


def test_the_appended_column_from_a_second_buffer(gpu, capi, fl):
    """Cell and UMI in one FASTQ buffer, the guide in a second whose records number alike (read 1 and read 2 of a paired run): the tables
    are those of the single-buffer layout of the same reads."""
    from seeq_amd import device as dev
    one, read1, read2, cols = _two_buffers(27, T + 100)
    t0, t1, t2 = _cuda(one), _cuda(read1), _cuda(read2)
    opt = SQ_BEST | dev.SEEQDEV_FASTQ
    sc = dev.Scanner()
    single = _run3(sc, fl, (t0, t0, t0), cols, "one buffer", opt)
    paired = _run3(sc, fl, (t1, t2, t1), cols, "two buffers", opt)
    assert paired["held"] == single["held"] and _counts(paired["app"]) == _counts(single["app"])
    assert paired["res"]["pairs"].tobytes() == single["res"]["pairs"].tobytes() and paired["res"]["groups"].tobytes() == single["res"]["groups"].tobytes()
    assert single["res"]["npaired"] > T // 2 and single["app"]["ndropped"] > 50
    sc.close()


def test_hold_and_grouped_call_on_two_buffers_number_lines_alike(gpu, capi, fl):
    """The documented rule of seeqdevScanTallyGrouped itself: the held column from one buffer, the members from another whose records
    number alike -- the tables of the single-buffer layout."""
    from seeq_amd import device as dev
    one, read1, read2, (_, guides, umis) = _two_buffers(28, T + 100)
    opt = SQ_BEST | dev.SEEQDEV_FASTQ
    held, hcnt = _held_of(guides)
    tables = []
    sc = dev.Scanner()
    for what, tg, tu in (("one buffer", _cuda(one), None), ("two buffers", _cuda(read2), _cuda(read1))):
        tu = tg if tu is None else tu

        def call(s):
            _cut(s, fl["A"], fl["B"], tg, guides, what + ": guides", opt)
            hold = s.tally_hold(tg)
            _cut(s, fl["C"], fl["D"], tu, umis, what + ": UMIs", opt)
            return hold, s.tally_grouped(tu)

        def check(s, out):
            assert out[0] == hcnt
            _same(out[1], held, umis)
            tables.append(out[1])
        _go(sc, what, call, check)
    assert tables[0]["pairs"].tobytes() == tables[1]["pairs"].tobytes() and tables[0]["npaired"] > T // 2
    sc.close()


# ---- 8. widths ----
def _raw_append(sc, capi, source, t, nbytes, library=False):
    col = (capi.seeqdev_tally_library_counts_t if library else capi.seeqdev_tally_hold_counts_t)()
    cnt = capi.seeqdev_tally_append_counts_t()
    entry = sc._lib.seeqdevScanTallyHoldAppendLibrary if library else sc._lib.seeqdevScanTallyHoldAppend
    C.set_errno(0)
    rc = entry(sc._h, source, C.c_void_p(t.data_ptr()) if t is not None else None, nbytes, C.byref(col), C.byref(cnt))
    return rc, C.get_errno()


def test_widths_beyond_63_bits_a_ninth_column_and_an_empty_column(gpu, capi, fl):
    from seeq_amd import device as dev
    rng = random.Random(29)
    INS, DEMUX = capi.SEEQDEV_TALLY_INSERTS, capi.SEEQDEV_TALLY_DEMUX
    sc = dev.Scanner()
    # two 20-base columns: 41 + 41 bits
    c20, g20, us = _pool(rng, 4, 20), _pool(rng, 4, 20), _pool(rng, 5, 12)
    spec = [(rng.choice(c20), rng.choice(g20), rng.choice(us)) for _ in range(200)]
    cells, guides, umis = _columns(spec)
    t = _cuda(_text(_reads3(spec, 29)))
    _cut(sc, fl["E"], fl["F"], t, cells, "20-base cells")
    assert sc.tally_hold(t)["key_bits"] == 41
    before = _held_arrays(sc)
    _cut(sc, fl["A"], fl["B"], t, guides, "20-base guides")
    assert _raw_append(sc, capi, INS, t, t.numel()) == (-1, errno.E2BIG) and "41" in capi.error_text()
    assert _held_arrays(sc) == before == _held_of(cells)[0] and sc.hold_columns() == [41]
    _cut(sc, fl["C"], fl["D"], t, umis, "UMIs")
    _same(sc.tally_grouped(t), before, umis)                 # the held column is what it was: the two-key tally of before
    # 16 + 14 bases: 33 + 29 = 62 bits
    c16, g14 = _pool(rng, 4, 16), _pool(rng, 4, 14)
    spec = [(rng.choice(c16), rng.choice(g14), rng.choice(us)) for _ in range(200)]
    t2 = _cuda(_text(_reads3(spec, 30)))
    got = _run3(sc, fl, (t2, t2, t2), _columns(spec), "33 + 29 bits")
    assert got["widths"] == [33, 29] and got["app"]["key_bits"] == 62 and got["res"]["passes"] == 4 + 8
    # eight columns of three bits, a ninth is refused, a new hold resets to one
    codes = _pool(rng, 5, 16)
    lines = [b"TT" + codes[i % 5] + b"CA" for i in range(300)]
    td = _cuda(_text(lines))
    ps = [dev.Pattern(c.decode(), 0) for c in codes]
    assert sc.demux_tensor(ps, td)["records"]["line"].tolist() == list(range(1, 301))
    assert sc.tally_hold(source="demux")["key_bits"] == 3
    for n in range(2, 9):
        app = sc.tally_hold_append(source="demux")
        assert (app["ncolumns"], app["width"], app["key_bits"], app["ndropped"], app["nheld"]) == (n, 3, 3 * n, 0, 300)
    assert sc.hold_columns() == [3] * 8
    word = lambda k: sum(k << (3 * c) for c in range(8))    # noqa: E731
    assert _held_arrays(sc) == [(i + 1, word(i % 5 + 1)) for i in range(300)]
    assert _raw_append(sc, capi, DEMUX, None, 0) == (-1, errno.EINVAL) and "8 columns" in capi.error_text()
    assert sc.hold_columns() == [3] * 8 and _held_arrays(sc)[0] == (1, word(1))
    assert all(int(c[0]) == 3 for c in dev.hold_split(np.array([word(3)], dtype=np.uint64), sc.hold_columns()))
    assert sc.tally_hold(source="demux")["key_bits"] == 3 and sc.hold_columns() == [3]
    for p in ps:
        p.close()
    # w == 0: no record of the new column has a key -- every key becomes 0, a grouped call pairs nothing
    spec = [(rng.choice(c16), b"ACGTNNACGTAC", rng.choice(us)) for _ in range(150)]
    cells, guides, umis = _columns(spec)
    t3 = _cuda(_text(_reads3(spec, 31)))
    _cut(sc, fl["E"], fl["F"], t3, cells, "cells")
    sc.tally_hold(t3)
    _cut(sc, fl["A"], fl["B"], t3, guides, "foreign guides")
    app = sc.tally_hold_append(t3)
    assert _counts(app) == dict(nrecords=150, nbefore=150, nheld=0, ndropped=150, width=0, key_bits=0, ncolumns=2) and app["column"]["nforeign"] == 150
    assert sc.hold_columns() == [33, 0] and _held_arrays(sc) == [(i + 1, 0) for i in range(150)]
    _cut(sc, fl["C"], fl["D"], t3, umis, "UMIs")
    res = sc.tally_grouped(t3)
    assert (res["npaired"], res["nungrouped"], res["npairs"], res["ngroups"], res["passes"]) == (0, 150, 0, 0, 0)
    # an append behind a hold of no record: nothing is launched
    empty = _cuda(_text([b"ACGTACGTAC"] * 5))
    _cut(sc, fl["E"], fl["F"], empty, [], "no cells")
    assert sc.tally_hold(empty)["nspans"] == 0
    _cut(sc, fl["A"], fl["B"], t3, guides, "guides")
    app = sc.tally_hold_append(t3)
    assert _counts(app) == dict(nrecords=0, nbefore=0, nheld=0, ndropped=0, width=0, key_bits=0, ncolumns=2) and sc.held()["nrecords"] == 0
    sc.close()


# ---- 9. survival ----
def test_the_held_column_survives_and_a_bad_span_leaves_it_alone(gpu, capi, fl):
    """A plain tally, a scan and an inserts call between hold and append leave the column intact.  A span of the appended source outside
    nbytes: EIO, the held column and the context as they were, and the append then succeeds."""
    from seeq_amd import device as dev
    rng = random.Random(32)
    cells, gs, us = _pool(rng, 5, 16), _pool(rng, 5, 12), _pool(rng, 7, 12)
    spec = [(rng.choice(cells), rng.choice(gs), rng.choice(us)) for _ in range(T + 77)]
    t = _cuda(_text(_reads3(spec, 32)))
    cols = _columns(spec)
    seen = {}

    def between(s):
        seen["held"] = _held_arrays(s)
        assert s.tally(t, copy=False)["ndistinct"] == 5      # (the cells' inserts result is still the context's)
        assert s.scan_tensor(fl["D"], t, SQ_BEST, dev.WANT_RECORDS)["nrecords"] == len(spec)
        s.inserts_tensor(fl["C"], fl["D"], t, SQ_BEST, copy=False)
        assert s.tally(t, copy=False)["ndistinct"] == 7
        assert _held_arrays(s) == seen["held"] and s.hold_columns() == [33]
    sc = dev.Scanner()
    _run3(sc, fl, (t, t, t), cols, "state between hold and append", between=between)
    assert seen["held"] == _held_of(cols[0])[0]
    # a bad span in the appended source
    INS = capi.SEEQDEV_TALLY_INSERTS
    _cut(sc, fl["E"], fl["F"], t, cols[0], "cells")
    sc.tally_hold(t)
    _cut(sc, fl["A"], fl["B"], t, cols[1], "guides")
    last = sc.insert_records(1, first=len(spec) - 1)[0]
    end = int(sc.insert_offsets(1, first=len(spec) - 1)[0]) + int(last["end"])
    assert _raw_append(sc, capi, INS, t, end - 1) == (-1, errno.EIO) and "outside" in capi.error_text()
    assert _held_arrays(sc) == seen["held"] and sc.hold_columns() == [33]
    assert _raw_append(sc, capi, INS, t, end) == (0, 0) and sc.hold_columns() == [33, 25]
    exp_held, _ = py_append(seen["held"], _held_of(cols[1])[0])
    assert _held_arrays(sc) == exp_held
    _cut(sc, fl["C"], fl["D"], t, cols[2], "UMIs")
    _same(sc.tally_grouped(t), exp_held, cols[2])
    # without a library the library entry is refused and the column stays; a hold that fails leaves none, and then so does the append
    assert _raw_append(sc, capi, INS, t, t.numel(), library=True) == (-1, errno.EINVAL) and sc.hold_columns() == [33, 25]
    _cut(sc, fl["E"], fl["F"], t, cols[0], "cells")
    hc = capi.seeqdev_tally_hold_counts_t()
    assert sc._lib.seeqdevScanTallyHold(sc._h, INS, C.c_void_p(t.data_ptr()), 10, C.byref(hc)) == -1
    assert sc.hold_columns() == [] and sc.held()["nrecords"] == 0
    assert _raw_append(sc, capi, INS, t, t.numel()) == (-1, errno.EINVAL) and "held column" in capi.error_text()
    sc.close()


# ---- 10. placement and stream order ----
def _window_case(seed):
    """A text whose first line lacks the first half of flank E, which ends the bytes in front of the window: a kernel that looks back finds a
    cell on line 1."""
    rng = random.Random(seed)
    cells, gs, us = _pool(rng, 5, 16), _pool(rng, 5, 12), _pool(rng, 7, 12)
    spec = [(rng.choice(cells), rng.choice(gs + [None]), rng.choice(us)) for _ in range(T + 30)]
    lines = _reads3(spec, seed)
    first = FE.encode()[10:] + cells[0] + FF.encode() + b"ACG" + FA.encode() + gs[0] + FB.encode() + b"ACG" + FC.encode() + us[0] + FD.encode()
    window = _text([first] + lines)
    spec = [(None, gs[0], us[0])] + spec
    return window, FE.encode()[:10], _columns(spec)


@pytest.mark.parametrize("lead", ["odd", "aligned"])
def test_a_window_of_a_larger_buffer(gpu, capi, fl, lead):
    from seeq_amd import device as dev
    window, before, cols = _window_case(33)
    big, lo, hi = W.place(window, W.odd_lead(1) if lead == "odd" else W.aligned_lead(2), before=before)
    assert (lo % 2 == 1) if lead == "odd" else (lo % 16 == 0 and lo % 128 != 0)
    view = _cuda(big)[lo:hi]
    assert view.is_contiguous() and view.data_ptr() % 16 == lo % 16
    sc = dev.Scanner()
    placed = _run3(sc, fl, (view, view, view), cols, "window at lead %d" % lo)
    alone = _cuda(window)
    plain = _run3(sc, fl, (alone, alone, alone), cols, "the window alone")
    assert placed["held"] == plain["held"] and placed["res"]["pairs"].tobytes() == plain["res"]["pairs"].tobytes()
    assert placed["held"][0][0] == 2                        # line 1 has no cell: half its flank lies in front of the window
    sc.close()


class _LateAppend(L.LateScanner):
    """LateScanner with the new entry armed as its siblings are: the text is late on the side stream when the append gets control."""

    def tally_hold_append(self, text=None, source="inserts", library=False):
        from seeq_amd import device as dev
        return self._late(lambda: self.arm(text), lambda: dev.Scanner.tally_hold_append(self, text, source, library))


def test_the_append_reads_its_text_in_stream_order(gpu, capi, fl):
    """On a caller's non-blocking stream the text arrives late before every entry (decoy bytes, a device-side delay, the true bytes): the
    append, like the hold and the grouped call, answers over the true bytes."""
    import torch
    window, _, cols = _window_case(34)
    t = _cuda(window)
    side = torch.cuda.Stream()
    flags = L.stream_flags(side)
    assert side.cuda_stream != 0 and (flags is None or flags & L.HIP_STREAM_NON_BLOCKING)
    delay = L.Delay()
    probe = _LateAppend(side, 0, armed=False)
    probe.give(t, window)
    for _ in ("cold", "warm"):
        probe.slowest_ms = 0.0
        _run3(probe, fl, (t, t, t), cols, "unarmed on the side stream")
    torch.cuda.synchronize()
    probe.close()
    ms = max(L.MIN_DELAY_MS, 2.0 * probe.slowest_ms)
    sc = _LateAppend(side, delay.cycles(ms), armed=True)
    sc.give(t, window)
    try:
        got = _run3(sc, fl, (t, t, t), cols, "late text on the side stream")
        assert sc.arms >= 9 and got["app"]["nheld"] > T // 2
        # the decoy's answer differs: its guides are other keys, so an append that read early composed other words
        decoy_cols = [(ln, L.decoy(g)) for ln, g in cols[1]]
        assert py_append(_held_of(cols[0])[0], _held_of(decoy_cols)[0])[0] != got["held"]
    finally:
        torch.cuda.synchronize()
        sc.close()
