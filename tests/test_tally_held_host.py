"""CPU: the rule of the tally of the held column itself, seeq_amd/csrc/seeq_tally_held.h -- the kinds of the held records, the shift of the
member columns, the two head rows and both tables over a sorted array, the dense cell -- compiled for the host by plain g++
(tests/tally_held_host_driver.cpp) and compared with a restatement in Python.  Once more as a stand-alone program under
-fsanitize=address,undefined.  Then the entries on the real library: exports, layouts, the argument checks (which run before any device
call and so fail the same way without a GPU) and seeqdevTallyHeldCell."""
import ctypes as C
import errno
import os
import random
import re
import subprocess

from conftest import ROOT
from test_tally_group_host import SAN, SAN_ENV

CSRC = os.path.join(ROOT, "seeq_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "build")
SRC = os.path.join(ROOT, "tests", "tally_held_host_driver.cpp")
COLUMNS, WORD_BITS = 8, 63
REPEAT, KEYLESS, COUNTED = 0, 1, 2
HELD = ("nrecords", "ncounted", "nkeyless", "nrepeat", "ndistinct", "nrows", "key_bits", "shift", "passes", "member_columns")
DENSE = ("ninside", "noutside", "inside_reads", "outside_reads")


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("seeq_tally_held.h", "seeq_tally_append.h", "seeq_tally_group.h", "seeq_tally.h", "seeq_strand.h", "seeq_tiles.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + ["-I" + CSRC, SRC, "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe, mode, text, env=None):
    r = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r.stdout.split("\n")


# ---- the rule, restated ----
def py_shift(widths, member_columns):
    """-> the bits of the last member_columns columns, or None where seeqdevScanTallyHeld says EINVAL."""
    if not 1 <= len(widths) <= COLUMNS or not 0 <= member_columns < len(widths) or sum(widths) > WORD_BITS:
        return None
    return sum(widths[len(widths) - member_columns:])


def py_kinds(held):
    """held: [(line, key)] in record order -> per record its kind."""
    return [REPEAT if i and held[i - 1][0] == line else COUNTED if key else KEYLESS for i, (line, key) in enumerate(held)]


def py_tables(words, shift, rows=True):
    """The nonzero words, in any order -> (table [(key, count)] ascending, rows [(group, count, first, ndistinct)] ascending)."""
    counts = {}
    for w in words:
        if w:
            counts[w] = counts.get(w, 0) + 1
    table = sorted(counts.items())
    out = []
    for rank, (key, count) in enumerate(table):
        if out and out[-1][0] == key >> shift:
            out[-1] = (out[-1][0], out[-1][1] + count, out[-1][2], out[-1][3] + 1)
        else:
            out.append((key >> shift, count, rank, 1))
    return table, out if rows else []


def py_held(held, widths, member_columns):
    """held: [(line, key)] in record order; widths: the held key's columns -> (counts, table, rows) as Scanner.tally_held reports them."""
    shift = py_shift(widths, member_columns)
    assert shift is not None
    kinds = py_kinds(held)
    counted = [key for (_, key), kind in zip(held, kinds) if kind == COUNTED]
    table, rows = py_tables(counted, shift, member_columns > 0)
    held_bits = max([k.bit_length() for _, k in held], default=0)
    cnt = dict(nrecords=len(held), ncounted=len(counted), nkeyless=kinds.count(KEYLESS), nrepeat=kinds.count(REPEAT), ndistinct=len(table), nrows=len(rows),
               key_bits=max([k.bit_length() for k in counted], default=0), shift=shift, passes=(held_bits + 7) // 8 if counted else 0,
               member_columns=member_columns)
    return cnt, table, rows


def py_cell(key, shift, nrows, ncols):
    r, c = key >> shift, key & ((1 << shift) - 1)
    return (r - 1) * ncols + (c - 1) if 1 <= r <= nrows and 1 <= c <= ncols else None


def py_dense(table, shift, nrows, ncols):
    """table: [(key, count)] -> (the matrix as {cell: count} of its nonzero cells, counts)."""
    cells, cnt = {}, dict(ninside=0, noutside=0, inside_reads=0, outside_reads=0)
    for key, count in table:
        cell = py_cell(key, shift, nrows, ncols)
        if cell is None:
            cnt["noutside"] += 1
            cnt["outside_reads"] += count
        else:
            assert cell not in cells                        # distinct keys, distinct cells
            cells[cell] = count
            cnt["ninside"] += 1
            cnt["inside_reads"] += count
    return cells, cnt


def test_the_restatement_itself():
    # widths [3, 2]: a key is (sample << 2) | guide.  Line 3 has two records, the first one decides; line 4's first record has no key and its
    # keyed repeat does not count; line 7 again (2, 1)
    held = [(1, 2 << 2 | 1), (2, 0), (3, 1 << 2 | 3), (3, 2 << 2 | 1), (4, 0), (4, 1 << 2 | 1), (7, 2 << 2 | 1), (9, 5 << 2 | 2)]
    assert py_kinds(held) == [COUNTED, KEYLESS, COUNTED, REPEAT, KEYLESS, REPEAT, COUNTED, COUNTED]
    cnt, table, rows = py_held(held, [3, 2], 1)
    assert cnt == dict(nrecords=8, ncounted=4, nkeyless=2, nrepeat=2, ndistinct=3, nrows=3, key_bits=5, shift=2, passes=1, member_columns=1)
    assert table == [(1 << 2 | 3, 1), (2 << 2 | 1, 2), (5 << 2 | 2, 1)]
    assert rows == [(1, 1, 0, 1), (2, 2, 1, 1), (5, 1, 2, 1)]
    cnt0, table0, rows0 = py_held(held, [3, 2], 0)
    assert table0 == table and rows0 == [] and (cnt0["shift"], cnt0["nrows"]) == (0, 0)
    # two entries of one row
    assert py_tables([9, 10, 9, 5], 2) == ([(5, 1), (9, 2), (10, 1)], [(1, 1, 0, 1), (2, 3, 1, 2)])
    cells, dc = py_dense(table, 2, 2, 3)
    assert cells == {0 * 3 + 2: 1, 1 * 3 + 0: 2} and dc == dict(ninside=2, noutside=1, inside_reads=3, outside_reads=1)
    assert py_dense(table, 2, 1, 1) == ({}, dict(ninside=0, noutside=3, inside_reads=0, outside_reads=4))
    assert py_shift([3, 2], 2) is None and py_shift([3, 2], -1) is None and py_shift([], 0) is None and py_shift([8, 17, 4], 2) == 21
    assert py_held([], [5], 0) == (dict(nrecords=0, ncounted=0, nkeyless=0, nrepeat=0, ndistinct=0, nrows=0, key_bits=0, shift=0, passes=0, member_columns=0), [], [])


# ---- the kinds and the shift ----
def _column(rng, n, bits, step=(0, 0, 1, 1, 1, 2, 7), keyless=0.2, pool=None):
    line, out = 0, []
    for _ in range(n):
        line += rng.choice(step)
        key = rng.choice(pool) if pool else rng.getrandbits(bits) | 1 if bits else 0
        out.append((max(line, 1), 0 if rng.random() < keyless else key))
    return out


def _kinds_cases():
    rng = random.Random(61)
    cases = [([3, 2], 1, [(1, 9), (2, 0), (3, 7), (3, 9), (4, 0), (4, 5), (7, 9), (9, 22)]),
             ([5], 0, []), ([5], 0, [(4, 0)]), ([5], 0, [(4, 17)]), ([5], 0, [(4, 0), (4, 17)]),      # a keyless first record with a keyed repeat
             ([5], 0, [(2 ** 32 - 1, 1), (2 ** 32 - 1, 2)]),
             ([33, 30], 1, [(1, 2 ** 63 - 1), (2, 2 ** 62)]), ([0, 63], 1, [(1, 2 ** 63 - 1)]), ([63, 0], 1, [(1, 2 ** 63 - 1)]),
             ([3, 2], 2, [(1, 9)]), ([3, 2], -1, [(1, 9)]), ([3, 2, 4], 3, []), ([1] * 8, 7, [(1, 255)]), ([1] * 9, 1, [(1, 1)]), ([], 0, [(1, 1)])]
    for n in (1, 2, 63, 64, 65, 300, 1023, 1024, 1025, 3000):
        for widths, m in (([8], 0), ([8, 12], 1), ([33, 17], 1), ([8, 22, 17], 2), ([8, 22, 17], 1), ([3] * 8, 4)):
            cases.append((widths, m, _column(rng, n, sum(widths), step=rng.choice([(0, 0, 1, 1, 1, 2, 7), (1,), (0, 0, 0, 1)]))))
    return cases


def _kinds_input(cases):
    return "".join("M %d %d %s\nH %d\n%s" % (len(w), m, " ".join(map(str, w)), len(h), "".join("%d %x\n" % r for r in h)) for w, m, h in cases)


def _check_kinds(lines, cases):
    at = refused = repeats = keyless = 0
    for widths, m, held in cases:
        shift = py_shift(widths, m)
        assert lines[at] == ("S -1 0" if shift is None else "S 0 %d" % shift), (lines[at], widths, m)
        at += 1
        refused += shift is None
        kinds = py_kinds(held)
        got = [ln.split() for ln in lines[at:at + len(held)]]
        assert [(int(k), int(w, 16)) for k, w in got] == [(kind, key if kind == COUNTED else 0) for kind, (_, key) in zip(kinds, held)], (widths, m, held[:8])
        at += len(held)
        counted = [key for (_, key), kind in zip(held, kinds) if kind == COUNTED]
        held_bits = max([k.bit_length() for _, k in held], default=0)
        assert lines[at] == "C %d %d %d %d %d" % (len(counted), kinds.count(KEYLESS), kinds.count(REPEAT), max([k.bit_length() for k in counted], default=0),
                                                 (held_bits + 7) // 8 if counted else 0), (lines[at], widths, m)
        at += 1
        repeats += kinds.count(REPEAT)
        keyless += kinds.count(KEYLESS)
    assert lines[at:] in ([], [""]) and refused == 5 and repeats > 3000 and keyless > 1000


def test_the_kinds_and_the_shift_on_the_host():
    cases = _kinds_cases()
    exe = _build("tally_held_host_driver", [])
    _check_kinds(_run(exe, "kinds", _kinds_input(cases)), cases)
    f = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert f == ["H", str(REPEAT), str(KEYLESS), str(COUNTED), str(COLUMNS), str(WORD_BITS)]


def test_a_line_whose_first_record_is_keyless_and_whose_second_has_a_key():
    held = [(1, 0), (1, 6), (2, 6), (2, 0), (3, 0)]
    cnt, table, rows = py_held(held, [2, 1], 1)
    assert (cnt["ncounted"], cnt["nkeyless"], cnt["nrepeat"]) == (1, 2, 2) and table == [(6, 1)] and rows == [(3, 1, 0, 1)]
    lines = _run(_build("tally_held_host_driver", []), "kinds", _kinds_input([([2, 1], 1, held)]))
    assert lines[:7] == ["S 0 1", "1 0", "0 0", "2 6", "0 0", "1 0", "C 1 2 2 3 1"]


# ---- the heads and both tables over a sorted array ----
def _tables_cases():
    rng = random.Random(67)
    cases = [(2, []), (2, [0]), (2, [0, 0, 0]), (2, [5]), (0, [5, 5, 5]), (2, [0, 5, 9, 9, 10]), (63, [1, 2 ** 63 - 1]), (62, [2 ** 62, 2 ** 63 - 1]),
             (0, [0, 1, 2, 3]), (1, [2, 3, 3, 4]), (17, [1 << 17 | 1] * 1500)]
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000):
        for shift, nrow, ncol in ((0, 1, 40), (4, 6, 15), (17, 30, 2000), (17, 900, 3), (30, 5, 5)):
            def word():
                if rng.random() < 0.15:
                    return 0
                if not shift:
                    return rng.randrange(1, ncol + 1)
                return rng.randrange(1, nrow + 1) << shift | rng.randrange(1, min(ncol, (1 << shift) - 1) + 1)
            cases.append((shift, sorted(word() for _ in range(n))))
    return cases


def _tables_input(cases):
    return "".join("T %d %d\n%s" % (shift, len(w), "".join("%x\n" % x for x in w)) for shift, w in cases)


def _check_tables(lines, cases):
    at = nkeys = nrows = 0
    for shift, words in cases:
        table, rows = py_tables(words, shift)
        assert lines[at] == "K %d" % len(table), (lines[at], shift, words[:8])
        got = [ln.split() for ln in lines[at + 1:at + 1 + len(table)]]
        assert [(int(k, 16), int(c)) for k, c in got] == table, (shift, words[:8])
        at += 1 + len(table)
        assert lines[at] == "R %d" % len(rows), (lines[at], shift, words[:8])
        got = [ln.split() for ln in lines[at + 1:at + 1 + len(rows)]]
        assert [(int(g, 16), int(c), int(f), int(d)) for g, c, f, d in got] == rows, (shift, words[:8])
        at += 1 + len(rows)
        assert sum(c for _, c in table) == sum(r[1] for r in rows) == sum(1 for w in words if w) and sum(r[3] for r in rows) == len(table)
        nkeys += len(table)
        nrows += len(rows)
    assert lines[at:] in ([], [""]) and nkeys > 5000 and nrows > 1000 and nkeys > 2 * nrows


def test_the_heads_and_both_tables_on_the_host():
    cases = _tables_cases()
    _check_tables(_run(_build("tally_held_host_driver", []), "tables", _tables_input(cases)), cases)


# ---- the dense cell ----
def _dense_cases():
    rng = random.Random(71)
    cases = [(0, 0, 1, 1), (1, 0, 1, 1), (1 << 2 | 1, 2, 1, 1), (1 << 2 | 2, 2, 1, 1), (2 << 2 | 1, 2, 1, 1), (1 << 2, 2, 4, 4), (3, 2, 4, 4),
             (2 ** 63 - 1, 63, 1, 1), (2 ** 63 - 1, 62, 1, 2 ** 32 - 1), ((2 ** 32 - 1) << 31 | (2 ** 31 - 1), 31, 2 ** 32 - 1, 2 ** 32 - 1),
             (4096 << 11 | 2000, 11, 4096, 2000), (4097 << 11 | 2000, 11, 4096, 2000), (4096 << 11 | 2001, 11, 4096, 2000)]
    for _ in range(400):
        shift = rng.randrange(0, 40)
        nrows, ncols = rng.choice([1, 7, 300, 4096]), rng.choice([1, 5, 2000])
        r, c = rng.randrange(0, nrows + 3), rng.randrange(0, ncols + 3) & ((1 << shift) - 1)
        cases.append((r << shift | c, shift, nrows, ncols))
    return cases


def _check_dense(lines, cases):
    inside = 0
    for ln, (key, shift, nrows, ncols) in zip(lines, cases):
        cell = py_cell(key, shift, nrows, ncols)
        assert ln == ("0 0" if cell is None else "1 %d" % cell), (ln, key, shift, nrows, ncols)
        inside += cell is not None
    assert lines[len(cases):] in ([], [""]) and 100 < inside < len(cases) - 100


def _dense_input(cases):
    return "".join("%x %d %d %d\n" % c for c in cases)


def test_the_dense_cell_on_the_host():
    cases = _dense_cases()
    _check_dense(_run(_build("tally_held_host_driver", []), "dense", _dense_input(cases)), cases)


def test_held_rule_under_sanitizers():
    exe = _build("tally_held_host_driver_asan", SAN)
    kc, tc, dc = _kinds_cases(), _tables_cases(), _dense_cases()
    _check_kinds(_run(exe, "kinds", _kinds_input(kc), SAN_ENV), kc)
    _check_tables(_run(exe, "tables", _tables_input(tc), SAN_ENV), tc)
    _check_dense(_run(exe, "dense", _dense_input(dc), SAN_ENV), dc)


# ---- the entries on the real library, without a GPU ----
HELD_SYMBOLS = ("seeqdevScanTallyHeld", "seeqdevScanTallyHeldRowsDevice", "seeqdevScanCopyTallyHeldRows", "seeqdevScanTallyHeldDense",
                "seeqdevScanLastTallyHeldMs", "seeqdevTallyHeldCell")


def test_held_symbols_exported(capi):
    L = capi.lib()
    hdr = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    for name in HELD_SYMBOLS:
        assert name in capi.EXPORTS and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, hdr), name


def test_held_counts_layouts(capi):
    hdr = open(os.path.join(ROOT, "include", "seeq_amd.h")).read()
    for t, size, name in ((capi.seeqdev_tally_held_counts_t, 64, "seeqdev_tally_held_counts_t"), (capi.seeqdev_tally_dense_counts_t, 32, "seeqdev_tally_dense_counts_t")):
        assert C.sizeof(t) == size
        body = re.search(r"typedef struct \{([^}]*)\} %s;\s*/\* %d bytes \*/" % (name, size), hdr).group(1)
        assert re.findall(r"^\s*uint\d+_t\s+(\w+);", body, re.M) == [n for n, _ in t._fields_]
    assert tuple(n for n, _ in capi.seeqdev_tally_held_counts_t._fields_) == HELD and tuple(n for n, _ in capi.seeqdev_tally_dense_counts_t._fields_) == DENSE
    t = capi.seeqdev_tally_held_counts_t
    assert [getattr(t, n).offset for n in HELD] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60]
    assert int(re.search(r"#define\s+SEEQDEV_TALLY_DENSE_MAX\s+\(\(uint64_t\)1 << (\d+)\)", hdr).group(1)) == 28 and capi.SEEQDEV_TALLY_DENSE_MAX == 1 << 28


def _fails(call, err):
    C.set_errno(0)
    assert call() == -1
    assert C.get_errno() == err


def test_held_argument_checks_without_a_device(capi):
    # The checks come before the device is touched: the stand-in context is all zeros -- no completed hold, no held tally.
    L = capi.lib()
    ctx = C.addressof(C.create_string_buffer(8192))
    hc, dc = capi.seeqdev_tally_held_counts_t(), capi.seeqdev_tally_dense_counts_t()
    out = C.addressof(C.create_string_buffer(64))
    for m in (0, 1, 7):
        _fails(lambda: L.seeqdevScanTallyHeld(None, m, C.byref(hc)), errno.EINVAL)               # NULL context
        _fails(lambda: L.seeqdevScanTallyHeld(ctx, m, None), errno.EINVAL)                       # NULL counts
        _fails(lambda: L.seeqdevScanTallyHeld(ctx, m, C.byref(hc)), errno.EINVAL)                # no completed hold
        assert "held column" in capi.error_text()
    for m in (-1, 8, 2 ** 31 - 1, -2 ** 31):
        _fails(lambda: L.seeqdevScanTallyHeld(ctx, m, C.byref(hc)), errno.EINVAL)                # member_columns outside any held key
    _fails(lambda: L.seeqdevScanTallyHeldDense(None, out, 2, 2, C.byref(dc)), errno.EINVAL)      # NULL context
    _fails(lambda: L.seeqdevScanTallyHeldDense(ctx, None, 2, 2, C.byref(dc)), errno.EINVAL)      # NULL output
    _fails(lambda: L.seeqdevScanTallyHeldDense(ctx, out, 2, 2, None), errno.EINVAL)              # NULL counts
    _fails(lambda: L.seeqdevScanTallyHeldDense(ctx, out, 2, 2, C.byref(dc)), errno.EINVAL)       # no completed held tally
    assert "held tally" in capi.error_text()
    _fails(lambda: L.seeqdevScanTallyHeldDense(ctx, out, 0, 2, C.byref(dc)), errno.EINVAL)
    _fails(lambda: L.seeqdevScanTallyHeldDense(ctx, out, 2, 0, C.byref(dc)), errno.EINVAL)
    # the shape is an argument: it is judged before the context is looked at -- 2^28 cells pass (and then the held tally is missed), one more does not
    _fails(lambda: L.seeqdevScanTallyHeldDense(ctx, out, 1 << 14, 1 << 14, C.byref(dc)), errno.EINVAL)
    assert "held tally" in capi.error_text()
    _fails(lambda: L.seeqdevScanTallyHeldDense(ctx, out, 1 << 14, (1 << 14) + 1, C.byref(dc)), errno.E2BIG)
    _fails(lambda: L.seeqdevScanTallyHeldDense(ctx, out, 2 ** 32 - 1, 2 ** 32 - 1, C.byref(dc)), errno.E2BIG)
    _fails(lambda: L.seeqdevScanTallyHeldDense(ctx, out, 2 ** 32 - 1, 0, C.byref(dc)), errno.EINVAL)
    # (a held tally with member_columns 0, and a plain tally since: test_gpu_tally_held.py -- they need a completed hold)
    # the rows and the time: a context without a held tally has none
    assert L.seeqdevScanTallyHeldRowsDevice(None) is None and L.seeqdevScanTallyHeldRowsDevice(ctx) is None
    rows = (capi.seeqdev_tally_group_t * 2)()
    _fails(lambda: L.seeqdevScanCopyTallyHeldRows(None, rows, 0, 0), errno.EINVAL)
    _fails(lambda: L.seeqdevScanCopyTallyHeldRows(ctx, rows, 0, 1), errno.EINVAL)
    _fails(lambda: L.seeqdevScanCopyTallyHeldRows(ctx, rows, 1, 0), errno.EINVAL)
    assert L.seeqdevScanCopyTallyHeldRows(ctx, rows, 0, 0) == 0 and L.seeqdevScanCopyTallyHeldRows(ctx, None, 0, 0) == 0
    ms = C.c_float(7)
    _fails(lambda: L.seeqdevScanLastTallyHeldMs(None, C.byref(ms)), errno.EINVAL)
    _fails(lambda: L.seeqdevScanLastTallyHeldMs(ctx, None), errno.EINVAL)
    assert L.seeqdevScanLastTallyHeldMs(ctx, C.byref(ms)) == 0 and ms.value == 0.0


def test_tally_held_cell_is_the_dense_rule(capi):
    from seeq_amd import device as dev
    L = capi.lib()
    for key, shift, nrows, ncols in _dense_cases():
        cell = C.c_uint64(77)
        C.set_errno(0)
        rc = L.seeqdevTallyHeldCell(key, shift, nrows, ncols, C.byref(cell))
        exp = py_cell(key, shift, nrows, ncols)
        assert (rc, cell.value) == ((0, 77) if exp is None else (1, exp)) and C.get_errno() == 0, (key, shift, nrows, ncols)
        assert dev.held_cell(key, shift, nrows, ncols) == exp
    # a whole table against py_dense
    rng = random.Random(73)
    table = sorted({(rng.randrange(0, 9) << 5 | rng.randrange(0, 32)): rng.randrange(1, 50) for _ in range(200)}.items())
    for nrows, ncols in ((8, 31), (3, 7), (1, 1), (20, 40)):
        cells, cnt = py_dense(table, 5, nrows, ncols)
        got = {dev.held_cell(k, 5, nrows, ncols): c for k, c in table if dev.held_cell(k, 5, nrows, ncols) is not None}
        assert got == cells and cnt["ninside"] == len(got) and cnt["ninside"] + cnt["noutside"] == len(table)
        assert cnt["inside_reads"] + cnt["outside_reads"] == sum(c for _, c in table)
    _fails(lambda: L.seeqdevTallyHeldCell(5, 2, 4, 4, None), errno.EINVAL)
    _fails(lambda: L.seeqdevTallyHeldCell(5, 64, 4, 4, C.byref(C.c_uint64())), errno.EINVAL)
