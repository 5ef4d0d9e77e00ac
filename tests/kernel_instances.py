"""Which template instance of the scan kernels and of the post-pass a scan runs -- the ledger behind tests/test_kernel_instances_host.py
(complete, on the CPU) and tests/test_gpu_kernel_instances.py (every row against the oracle, on the GPU).

The planner (seeq_amd/csrc/seeq_plan.h) returns a ScanPlan; run_setup, seg_onepass and seg_post (seeq_amd/csrc/seeq_device.hip) turn it into
kernel instances.  `instance_key` restates that dispatch over the sixteen numbers Scanner.last_plan() and the host harness's harness_plan both
report; `census` enumerates the plans of a grid of scans through the harness and so the keys the library can reach; `REPRESENTATIVES` names one
scan per key; `UNREACHABLE` the instances that are compiled and that no plan of the grid selects.

TO EXTEND: a new instantiation in the dispatch code gets a rule in instance_key (naming the statement it restates) and an entry in COMPILED; the
ledger test then fails and prints the new keys, each with a row that reaches it.  `python tests/kernel_instances.py --rows` writes
tests/kernel_instance_rows.py anew (to stdout) -- the rows are data, 436 lines, kept beside this module and imported here as REPRESENTATIVES;
without --rows the command prints the census.  A plain helper module: no fixtures, no test collection."""
import ctypes as C
import os
import random
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from seeq_amd.device import PLAN_FIELDS, plain_pattern      # noqa: E402  (the sixteen numbers of harness_plan and of seeqdevScanLastPlan, in order)

SQ_FIRST, SQ_BEST, SQ_ALL, SQ_COUNT = 0, 1, 2, 3
SQ_FAIL, SQ_CONVERT, SQ_IGNORE = 0, 4, 8
FASTA = 0x100
COUNTLINES, COUNTMATCH, RECORDS = 0, 1, 2
WANT_NAMES = {COUNTLINES: "COUNTLINES", COUNTMATCH: "COUNTMATCH", RECORDS: "RECORDS"}

# flags of harness_plan: what a scan context has collected of earlier texts (RerunFallback, seeq_rerun.h) and of the sample
FLAG_FORCE_LL, FLAG_NO_STREAM_ND, FLAG_SAMPLE_DIRTY = 1, 4, 16
# knob `kernel` of harness_plan = SEEQ_FUSED_KERNEL: 0 auto, 1 stream, 2 direct, 3 pair
KERNEL_KNOB = {0: None, 1: "stream", 2: "direct", 3: "pair"}

# the suite's two class patterns (tests/test_gpu_parity.py: the 40-position pattern of configs[4]; the sweep's head with two classes)
CLASS_PATTERNS = ("GATG[TA]AGCNCGATTAGC[CG]TGAAAATGNGAGTAC[GAT]GCGCGA", "GATGTAGC[GC]CGATTAG[CT]CTG")


def instance_key(plan, options, want):
    """The scan kernel's template arguments and the post-pass variant of a scan with this plan (a dict over PLAN_FIELDS), these options and
    this `want`, as the dispatch code derives them -> a string, "scan kernel | hit list | exact pass [| records]".  Every rule names the
    function of seeq_device.hip and the macro or statement in it that it restates (seeq_plan.h: the statement that sets the field)."""
    p = plan
    fasta = bool(options & FASTA)
    nd = options & 0x0C
    match = options & 3
    fw = p["fw"]
    if p["rc"]:
        return "none (rc %d)" % p["rc"]
    # ---- the scan kernel (run_setup) ----
    if p["path"] == 1:
        # seg_index_forward<W>: k_forward<W> -- W is the pattern's Peq words (SEEQ_FOR_WORDS in dispatch_run), not part of the plan: one family here
        scan = "k_forward"
    elif p["path"] == 3:
        # run_setup, `const void *fn = ...`: fw == 1 ? k_direct<4, 1> : k_direct<4, 2>
        scan = "k_direct<4,%d>" % fw
    elif p["use_pair"]:
        # run_setup, SEEQ_PAIR_FN: stream_wu 4, 5, 6, 7 pick their instance, everything else k_pair<8>
        wu = p["stream_wu"] if p["stream_wu"] in (4, 5, 6, 7) else 8
        # run_setup, `r.stream_fn = fasta ? SEEQ_PAIR_FN(true) : plan.ig ? ... : plan.pair_ll ? ... : SEEQ_PAIR_FN(false)`
        #      (seeq_plan.h: `p.ig = nd == PLAN_SQ_IGNORE` behind use_pair; `p.stream_ll = p.pair_ll` behind use_pair)
        var = "FA" if fasta else "IG" if nd == SQ_IGNORE else "LL" if p["stream_ll"] else "plain"
        scan = "k_pair<%d,%s>" % (wu, var)
    elif p["use_myers"]:
        # run_setup, SEEQ_MYERS_FN: stream_wu == 16 ? k_stream<16, FA, true, 0, MY> : k_stream<32, ...>; MY = fw; FA = fasta
        scan = "k_stream<%d,%s,LL,0,MY%d>" % (16 if p["stream_wu"] == 16 else 32, "FA" if fasta else "-", fw)
    else:
        # run_setup, SEEQ_STREAM_FN: stream_wu 4 and 6 pick their instance, everything else k_stream<8>
        wu = p["stream_wu"] if p["stream_wu"] in (4, 6) else 8
        # run_setup, `r.stream_fn = plan.stream_sub == 2 ? SEEQ_STREAM_FN(false, false, 2) : plan.stream_sub ? (ll, 1) : (fasta, ll)`
        if p["stream_sub"] == 2:
            fa, ll, sub = False, False, 2
        elif p["stream_sub"]:
            fa, ll, sub = False, bool(p["stream_ll"]), 1
        else:
            fa, ll, sub = fasta, bool(p["stream_ll"]), 0
        scan = "k_stream<%d,%s,%s,%d>" % (wu, "FA" if fa else "-", "LL" if ll else "-", sub)
        # seg_onepass, `f.dfa = ...`: the restart table of a long-line filter (ll_filter 2) is other data, not another instance -- but
        # seg_onepass, `f.ll_filter = ...` switches the kernel's candidate bookkeeping, so it is part of what ran
        if p["ll_filter"]:
            scan += "+ll_filter%d" % p["ll_filter"]
    fused = p["path"] != 1
    superset = bool(p["use_stream"])                      # seeq_plan.h: `p.superset = p.use_stream`
    # run_segments, `if (s->want != SEEQDEV_WANT_COUNTLINES || plan.superset)`: no post-pass for line counts of a kernel whose verdicts are
    # exact per line (k_direct, the generic path)
    if want == COUNTLINES and not superset:
        return scan + " | no post-pass"
    # ---- the hit list (seg_onepass behind the scan launch; seg_post, "K3: compaction") ----
    if not fused:
        hitlist = "k_compact"                               # seg_post, `if (!plan.use_fused) ... k_compact`
    elif p["order2"]:
        # seg_onepass, `if (order2)`: seeq_launch_tiles_post + seeq_launch_order; seg_post: seeq_launch_bounds2.  The plan's order2 is what is
        # meant: seg_onepass, `order2 = plan.order2 && order_nb <= SEEQ_ORDER_MAX_BLOCKS && ...` falls back to the chain below for a segment
        # of more tiles than the block sums hold (hundreds of MB), which the plan does not show -- the key then names a chain that did not run;
        # the rows' texts stay below 1 MB
        hitlist = "order2"
    elif p["use_stream"]:
        hitlist = "k_stream_reorder+k_stream_bounds"        # seg_onepass, `else ... k_fused_post` + launch_scanset + k_stream_reorder; seg_post: k_stream_bounds
    else:
        hitlist = "k_fused_reorder"                         # seg_onepass: k_fused_post + launch_scanset + k_fused_reorder
    nh_is_count = want == COUNTMATCH or (want == RECORDS and match == SQ_ALL)      # seeq_plan.h: `p.need_nh = ...; p.nh_is_count = p.need_nh`
    need_nh = nh_is_count or superset                                               # seeq_plan.h: `if (p.superset) p.need_nh = true`
    lead_best = want == RECORDS and match == SQ_BEST                                # seeq_plan.h: `p.lead_best = ...`
    # seg_post, `if (plan.leaders)`: k_lead_reduce, k_lead_top, k_lead_apply (with the keys under lead_best), k_lead_commit
    if p["leaders"]:
        hitlist += "+leaders(best)" if lead_best else "+leaders"
    wk = "WK" if p["stream_ll"] and p["use_stream"] else "-"      # seg_onepass, `a.stream_ch = plan.stream_ll ? STREAM_CH_HOST : 0u` (the one-pass kernels only)
    emitted = False
    if p["verify"]:
        # verify_variant: RECORDS under SQ_BEST -> BEST; hits counted per line -> ALL; else ANY
        var = "BEST" if lead_best else "ALL" if nh_is_count else "ANY"
        # seg_post, `a.vrange = ...`: parts of the walked automaton > 1 ? 512 : 0.  Behind k_stream k_verify runs only behind a filter
        #       (seeq_plan.h: `p.verify = ... p.filter ...`), and a k_stream filter is an automaton of more than one part (`p.filter = ...
        #       au.sdfa_parts > 1`): 512.  Behind k_pair it follows the pair automaton's parts, which the plan does not carry: left open ("vr?")
        vr = "vr?" if p["use_pair"] else "vr512"
        exact = "k_verify<%d,%s,%s>" % (fw, var, vr)
        if want == RECORDS and var != "ALL":
            exact += "+k_emit1"                             # seg_post: seeq_launch_emit1
            emitted = True
        elif want == RECORDS:
            exact += "+k_emit_all<%d>" % fw                 # seg_post: seeq_launch_emit_all (ecache: fused, need_nh, RECORDS -- `uint4 *ecache = ...`)
            emitted = True
    elif need_nh:
        if fused:
            exact = "k_exact1<COUNT,%d,-1,%s>" % (fw, wk)   # seg_post, SEEQ_COUNT1
        else:
            exact = "k_exact<W,COUNT>"                      # seg_post, `else ... k_exact<W, SQ_MODE_COUNT>`
        if p["leaders"]:
            exact += "+k_lead_check+" + ("k_lead_best" if lead_best else "k_lead_lines")      # seg_post, `if (plan.leaders)` behind the COUNT pass
        elif superset and nh_is_count:
            exact += "+k_count_nonzero"                     # seg_post, `else if (plan.superset && plan.nh_is_count)`
    else:
        exact = "no count pass"
    key = "%s | %s | %s" % (scan, hitlist, exact)
    # ---- the records (seg_post, "K5: records") ----
    if want == RECORDS and not emitted:
        if fused:
            mo = SQ_FIRST if match == SQ_COUNT else match   # seg_post, `const int mo = ...`
            key += " | k_exact1<EMIT,%d,%s,%s>" % (fw, "BEST" if mo == SQ_BEST else "-1", wk)      # seg_post, SEEQ_EMIT1
        else:
            key += " | k_exact<W,EMIT>+k_rec_offsets"        # seg_post, `else ... k_exact<W, SQ_MODE_EMIT>` + k_rec_offsets
    return key


# ---------------------------------------------------------------------------------------------------------------------------------------
# the harness
# ---------------------------------------------------------------------------------------------------------------------------------------
_H = None


def use_harness(H):
    """Tests hand over the library their `harness` fixture (tests/conftest.py) has built and loaded."""
    global _H
    _H = bind(H)
    return _H


def harness_lib():
    """The harness in use: what use_harness was given, else -- the command line, which has no fixtures -- tests/libharness.so, built as the
    fixture builds it when it is missing or older than its sources."""
    global _H
    if _H is None:
        so = os.path.join(ROOT, "tests", "libharness.so")
        srcs = [os.path.join(ROOT, "tests", "host_harness.cpp")] + [os.path.join(ROOT, "seeq_amd", "csrc", f)
                                                                    for f in ("seeq_kernel_core.h", "seeq_dfa.h", "seeq_plan.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", srcs[0], "-o", so])
        _H = bind(C.CDLL(so))
    return _H


def bind(H):
    H.harness_compile.restype = C.c_int
    H.harness_compile.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_int)]
    H.harness_plan.restype = C.c_int
    H.harness_plan.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_int)]
    H.harness_plan_many.restype = C.c_int
    H.harness_plan_many.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return H


def compile_pattern(H, expr):
    keys = C.create_string_buffer(2048)
    err = C.c_int(0)
    m = H.harness_compile(expr.encode(), keys, C.byref(err))
    assert m > 0, (expr, err.value)
    return keys, m


def plan_of(H, expr, tau, options, want, avg_line, flags=0, kernel=0):
    """harness_plan over one scan -> dict over PLAN_FIELDS"""
    keys, m = compile_pattern(H, expr)
    out = (C.c_int * 16)()
    assert H.harness_plan(keys, m, tau, options, want, float(avg_line), flags, kernel, out) == 0
    return dict(zip(PLAN_FIELDS, list(out)))


def plans_of(H, expr, tau, rows, avg_lines):
    """harness_plan_many: the plans of many scans of ONE pattern, its automata built once.  rows: int32 [n, 4] (options, want, flags, kernel);
    avg_lines: float64 [n] -> int32 [n, 16]"""
    keys, m = compile_pattern(H, expr)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    avg = np.ascontiguousarray(avg_lines, dtype=np.float64)
    out = np.zeros((len(rows), 16), dtype=np.int32)
    H.harness_plan_many(keys, m, tau, len(rows), rows.ctypes.data, avg.ctypes.data, out.ctypes.data)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------------------------
MATCH_WANT = ((SQ_FIRST, COUNTLINES), (SQ_BEST, RECORDS), (SQ_ALL, RECORDS), (SQ_FIRST, COUNTMATCH))
AVG_LINES = (79.0, 151.0, 400.0, 5000.0)
FLAGS = (0, FLAG_FORCE_LL, FLAG_NO_STREAM_ND, FLAG_SAMPLE_DIRTY)
# Distances: the pattern API admits tau < m; the automata of every (m, tau) with tau <= min(m - 1, 15) build in 14 s together, none of
# them in more than 50 ms (measured over lengths 4 ... 62) -- so that bound stands as it is, nothing cut by build time.
TAU_MAX = 15
CENSUS_SEED = 20251019


def census_patterns():
    """(expression, m): random ACGT of every length 4 ... 62 from a fixed seed, and the suite's two class patterns"""
    rng = random.Random(CENSUS_SEED)
    pats = [("".join(rng.choice("ACGT") for _ in range(m)), m) for m in range(4, 63)]
    H = harness_lib()
    return pats + [(e, compile_pattern(H, e)[1]) for e in CLASS_PATTERNS]


def census_grid():
    """The scans planned for every (pattern, tau): int32 rows (options, want, flags, kernel) and their avg_line -- ordered so that the first
    input found for a key needs as little as possible: no knob before knobs, no flag before flags"""
    rows, avg = [], []
    for kernel in (0, 1, 2, 3):
        for flags in FLAGS:
            for nd in (SQ_FAIL, SQ_CONVERT, SQ_IGNORE):
                for fa in (0, FASTA):
                    for al in AVG_LINES:
                        for match, want in MATCH_WANT:
                            rows.append((match | nd | fa, want, flags, kernel))
                            avg.append(al)
    return np.array(rows, dtype=np.int32), np.array(avg, dtype=np.float64)


def census_all():
    """{instance key: (level, [inputs])}: every (pattern, tau) that reaches the key at the key's lowest level -- 0: the library's own choice,
    1: a flag of the context, 2: a knob -- each with the first scan of the grid that does; an input is dict(pattern, tau, options, want,
    avg_line, flags, kernel).  The grid: census_patterns() x tau 0 ... min(m - 1, TAU_MAX) x census_grid()."""
    H = harness_lib()
    grid, avg = census_grid()
    level = (grid[:, 3] != 0) * 2 + (grid[:, 2] != 0)
    found = {}
    for expr, m in census_patterns():
        for tau in range(0, min(m - 1, TAU_MAX) + 1):
            out = plans_of(H, expr, tau, grid, avg)
            # the key is a function of (plan, options, want): one call per distinct combination, the first scan of each
            combo = np.concatenate([out, grid[:, :2]], axis=1)
            _, first = np.unique(combo, axis=0, return_index=True)
            for i in sorted(first):
                key = instance_key(dict(zip(PLAN_FIELDS, (int(v) for v in out[i]))), int(grid[i, 0]), int(grid[i, 1]))
                lv = int(level[i])
                if key not in found or lv < found[key][0]:
                    found[key] = (lv, [])
                if lv == found[key][0]:
                    found[key][1].append(dict(pattern=expr, tau=tau, options=int(grid[i, 0]), want=int(grid[i, 1]), avg_line=float(avg[i]),
                                              flags=int(grid[i, 2]), kernel=int(grid[i, 3])))
    return found


def census(found=None):
    """{instance key: the first input that yields it, at the key's lowest level} (of census_all(), or of `found`, its result)"""
    return {key: inputs[0] for key, (lv, inputs) in (found or census_all()).items()}


# ---------------------------------------------------------------------------------------------------------------------------------------
# the rows' texts
# ---------------------------------------------------------------------------------------------------------------------------------------
CHUNK, TILE_BYTES = 128, 8192      # bytes per lane of k_stream / k_pair; per tile (64 lanes)
FOREIGN = b"X-.x"


def _single_positions(expr):
    """indices of the pattern positions that take exactly one base"""
    out, i, k = [], 0, 0
    while i < len(expr):
        if expr[i] == "[":
            i = expr.index("]", i) + 1
        else:
            if expr[i] in "ACGTacgt":
                out.append(k)
            i += 1
        k += 1
    return out


def _edit(rng, s, nerr):
    s = list(s)
    for _ in range(nerr):
        i = rng.randrange(len(s))
        k = rng.randrange(3)
        if k == 0:
            s[i] = rng.choice("ACGT")
        elif k == 1 and len(s) > 1:
            del s[i]
        else:
            s.insert(i, rng.choice("ACGT"))
    return "".join(s)


def _near_miss(rng, plain, singles, tau):
    """the pattern with tau + 1 substitutions at distinct one-base positions, each by another base: one edit too many (where the pattern
    has fewer such positions, or the substitutions can be had cheaper with gaps, the oracle decides -- the rows count what it rejects)"""
    s = list(plain)
    for i in rng.sample(singles, min(tau + 1, len(singles))):
        s[i] = rng.choice([b for b in "ACGT" if b != s[i]])
    return "".join(s)


class RowText:
    """buf (bytes, final newline), nplanted (lines that carry a plant), near (0-based indices, among ALL lines, of the lines whose only plant is a
    near miss), fasta"""

    def __init__(self, buf, nplanted, near, fasta):
        self.buf, self.nplanted, self.near, self.fasta = buf, nplanted, near, fasta

    def counted_near(self):
        """the near-miss lines as 1-based COUNTED line numbers (FASTA: header lines are not counted)"""
        lines = self.buf.split(b"\n")[:-1]
        out, n = [], 0
        near = set(self.near)
        for i, ln in enumerate(lines):
            if self.fasta and ln.startswith(b">"):
                continue
            n += 1
            if i in near:
                out.append(n)
        return out


def _foreign_rate(row_plan, options):
    """Bytes outside the alphabet in a row's text: 1 % under SQ_CONVERT / SQ_IGNORE -- but none where the instance is k_stream's plain table
    walk, which is exact on clean text only and hands dirty text to another kernel (seeq_scan_common.h, k_fused_post: OVF_NONDNA), and 0.2 %
    for k_stream's skipping variant (SUB 2): a skipped byte in a chain's 32-byte warm-up window makes a made-up candidate, two windows per lane,
    and a wave with more of them than a quarter of its lines sends the scan to the per-line kernels (seeq_stream.h, wv_fakes; same flag) -- at
    1 % that is 128 * (1 - 0.99^32) = 35 per tile of ~55 to ~100 lines, always; at 0.2 % it is 8."""
    nd = options & 0x0C
    if not nd:
        return 0.0
    table_stream = row_plan["path"] == 5
    if table_stream and row_plan["stream_sub"] == 0:
        return 0.0
    if table_stream and row_plan["stream_sub"] == 2:
        return 0.002
    return 0.01


def build_text(expr, tau, recipe, avg_line, warm_bytes, foreign_rate, fasta, seed=1):
    """The text of a row (see tests/test_gpu_kernel_instances.py for what it has to hold).  recipe "reads": ~2 400 read-length lines;
    "long": ~1 000 read-length lines and three lines of 40 - 150 KB; "long-N": the same, the long lines made of N between their occurrences -- for
    patterns that match nearly everywhere in random DNA (2 tau >= m: the only ones that reach some instances), where hits without end in a long
    line send the scan off the leaders by design (OVF_LEADER, seeq_stream.h k_lead_check) and the instance would not be the one tested; "fasta-per-read": a header before every read, the first 64 KiB -- what a
    context samples -- records of 7 + 151 bytes (average line 79, foreign bytes enough for sample_dirty), the rest as "reads"."""
    rng = random.Random(seed * 7919 + len(expr) * 131 + tau)
    plain = plain_pattern(expr)
    singles = _single_positions(expr)
    m = len(plain)

    def plant_copy():
        """(copy, is a near miss)"""
        if rng.random() < 0.4:
            return _near_miss(rng, plain, singles, tau), True
        return _edit(rng, plain, rng.randint(0, tau)), False

    lengths = [m - 1, m, m + tau, 40, 75, 75, 75]
    if avg_line > 100:
        lengths += [150, 150, 151, 151, 257]
    if avg_line > 300 and recipe != "long-N":             # (long-N: a line of 550 random bases is a long line with hits without end, in small)
        lengths += [400, 550]
    lengths = [n for n in lengths if n >= 1]
    lines, nplanted, near = [], 0, []
    state = {"off": 0}
    # seams: every tile boundary, the three lane-chunk boundaries behind it, and the first byte of the warm-up window of each -- an occurrence
    # ends on the last byte before the seam, ends on the first byte after it, starts on it, or lies across it, in turn
    seams = []

    def seam_targets(limit):
        t = TILE_BYTES
        k = 0
        while t < limit:
            for s in (t, t + CHUNK, t + 2 * CHUNK, t + 37 * CHUNK):
                for q in (s, s - warm_bytes):
                    seams.append((q, k % 4))
                    k += 1
            t += TILE_BYTES
        seams.sort()
    seam_targets(1 << 20)
    seam_at = [0]

    def add_line(t, planted, is_near):
        nonlocal nplanted
        if planted:
            nplanted += 1
            if is_near:
                near.append(len(lines))
        lines.append(t)
        state["off"] += len(t) + 1

    def read_line(n, force=None):
        """a read of n bytes: a seam plant when a seam lies in it, else a random plant in a third of the lines (force: 'start' / 'end')"""
        off = state["off"]
        t = rng.choices("ACGT", k=n)
        while seam_at[0] < len(seams) and seams[seam_at[0]][0] < off:
            seam_at[0] += 1
        cp, is_near, col = None, False, None
        if not force and m - tau - 1 >= 1 and rng.random() < 0.08:
            # a near miss of its own kind: the whole line is the pattern less tau + 1 of its bases -- too short to hold an occurrence, whatever
            # else matches (at large tau a line of any other length does)
            keep = sorted(rng.sample(range(m), m - tau - 1))
            add_line("".join(plain[i] for i in keep), True, True)
            return
        if force:
            cp, is_near = plant_copy()
            col = 0 if force == "start" else max(0, n - len(cp))
        elif seam_at[0] < len(seams) and seams[seam_at[0]][0] < off + n:
            q, how = seams[seam_at[0]]
            seam_at[0] += 1
            cp, is_near = plant_copy()
            col = q - off - (len(cp), len(cp) - 1, 0, len(cp) // 2)[how]
        elif rng.random() < 1.0 / 3:
            cp, is_near = plant_copy()
            col = rng.choice([0, n - len(cp), rng.randrange(0, max(1, n - len(cp) + 1))])
        if cp is not None and len(cp) <= n:
            col = min(max(col, 0), n - len(cp))
            t[col:col + len(cp)] = list(cp)
            add_line("".join(t), True, is_near)
        else:
            add_line("".join(t), False, False)

    def long_line(n):
        t = rng.choices("ACGT", k=n) if recipe == "long" else ["N"] * n
        cols = [0, n - m - tau - 1] + [rng.randrange(m + tau, n - 2 * (m + tau)) for _ in range(22)]
        cols.append(cols[5] + m + rng.randrange(0, tau + 1))      # closer to its neighbour than m + tau
        for c in cols:
            cp, _ = plant_copy()
            c = min(max(c, 0), n - len(cp))
            t[c:c + len(cp)] = list(cp)
        t[n - m:] = list(plain)                               # the line's last bytes
        add_line("".join(t), True, False)

    if recipe == "fasta-per-read":
        i = 0
        while state["off"] < 70000:
            add_line(">r%04d" % i, False, False)
            read_line(150)
            i += 1
    if recipe in ("long", "long-N"):
        for k, n in enumerate((40000, 150000, 90000)):
            for _ in range(300):
                read_line(rng.choice(lengths))
            long_line(n)
        nreads = 100
    else:
        nreads = 2400
    for i in range(nreads):
        if fasta and (recipe == "fasta-per-read" or i % 7 == 0):
            add_line(">read%d %s len" % (i, plain), False, False)      # a header that holds the pattern
        read_line(rng.choice(lengths))
    read_line(150 if avg_line > 100 else 75, force="start")
    read_line(150 if avg_line > 100 else 75, force="end")     # the text's last line ends with an occurrence
    buf = bytearray(("\n".join(lines) + "\n").encode())
    if foreign_rate:
        hdr = False
        for i in range(len(buf)):
            c = buf[i]
            if c == 10:
                hdr = False
            elif fasta and c == 62 and (i == 0 or buf[i - 1] == 10):
                hdr = True
            elif not hdr and rng.random() < foreign_rate:
                buf[i] = rng.choice(FOREIGN)
    return RowText(bytes(buf), nplanted, near, fasta)



# ---------------------------------------------------------------------------------------------------------------------------------------
# the rows
# ---------------------------------------------------------------------------------------------------------------------------------------
_OPT_NAMES = (("BEST", SQ_BEST), ("ALL", SQ_ALL), ("CONVERT", SQ_CONVERT), ("IGNORE", SQ_IGNORE), ("FASTA", FASTA))


def options_text(options):
    return "|".join(n for n, b in _OPT_NAMES if options & b) or "FIRST"


def options_of(text):
    return sum(b for n, b in _OPT_NAMES if n in text.split("|"))


class Row:
    """One line of REPRESENTATIVES: (key, pattern expression, tau, options, want, avg_line, recipe, knobs).  options: names joined by | (FIRST: none);
    avg_line: the line hint the scan is given (recipe "fasta-per-read": no hint -- the context samples the text, and the sample has to come
    out dirty); knobs: the environment a context needs to get there ({} = the library's own choice)."""

    def __init__(self, key, pattern, tau, options, want, avg_line, recipe, knobs):
        self.key, self.pattern, self.tau, self.avg_line, self.recipe, self.knobs = key, pattern, tau, float(avg_line), recipe, dict(knobs)
        self.options = options_of(options)
        self.want = {v: k for k, v in WANT_NAMES.items()}[want]
        self.flags = FLAG_SAMPLE_DIRTY if recipe == "fasta-per-read" else 0
        self.kernel = {v: k for k, v in KERNEL_KNOB.items()}[self.knobs.get("SEEQ_FUSED_KERNEL")]
        assert set(self.knobs) <= {"SEEQ_FUSED_KERNEL"}, self.knobs

    @property
    def fasta(self):
        return bool(self.options & FASTA)

    def plan(self, H=None, avg_line=None):
        return plan_of(H or harness_lib(), self.pattern, self.tau, self.options, self.want, self.avg_line if avg_line is None else avg_line,
                       self.flags, self.kernel)

    def text(self, plan=None):
        """the row's text (cached per what it depends on)"""
        plan = plan or self.plan()
        # the warm-up window of the walk: 4 * stream_wu bytes before a chunk -- 16 ... 32 for the table walks, 64 or 128 in Myers mode; k_direct and
        # the generic path walk lines, not chunks, and have no such seam: 32 as a filler
        warm = 4 * plan["stream_wu"] if plan["use_stream"] else 32
        args = (self.pattern, self.tau, self.recipe, self.avg_line, warm, _foreign_rate(plan, self.options), self.fasta)
        if args not in _TEXTS:
            if len(_TEXTS) > 16:
                _TEXTS.pop(next(iter(_TEXTS)))
            _TEXTS[args] = build_text(*args)
        return _TEXTS[args]

    def line(self):
        return "    (%r, %r, %d, %r, %r, %g, %r, %r)," % (self.key, self.pattern, self.tau, options_text(self.options), WANT_NAMES[self.want], self.avg_line,
                                                         self.recipe, self.knobs)


_TEXTS = {}
MIN_MATCH_LINES, MIN_NEAR_MISSES = 50, 50


def vacuity(row, text, exp, plan):
    """What keeps a row from passing without testing anything -> None, or what is wrong: the oracle finds at least 50 matching lines, rejects
    at least 50 planted near misses, and (behind a filter) fewer lines match than hold a plant."""
    rejected = sum(1 for n in text.counted_near() if exp["line_nhits"][n - 1] == 0)
    if exp["nmatchlines"] < MIN_MATCH_LINES:
        return "%d matching lines" % exp["nmatchlines"]
    if rejected < MIN_NEAR_MISSES:
        return "%d near misses rejected" % rejected
    if plan["filter"] and not exp["nmatchlines"] < text.nplanted:
        return "a filter, and %d lines match of %d planted" % (exp["nmatchlines"], text.nplanted)
    return None


from kernel_instance_rows import REPRESENTATIVES      # noqa: E402  (data: one tuple per key, the columns of Row; beside this module, written by --rows)


def rows():
    return [Row(*r) for r in REPRESENTATIVES]


# Compiled and never selected: the instance (as it appears in a key) and the planner statement that excludes it.  The ledger test checks that no
# key of the census holds one.
UNREACHABLE = (
    ("k_stream<32,-,LL,0,MY1>", "seeq_plan.h, `if (p.use_myers) p.stream_wu = in.wlen + in.tau - 1 <= 64 ? 16 : 32` -- 32 warm-up dwords serve m + tau - 1 > 64, "
                                "one Myers word (`p.fw = in.wlen <= PLAN_MAX_WLEN ? 1 : 2`) m <= 30, and tau < m: at most 58"),
    ("k_stream<32,FA,LL,0,MY1>", "seeq_plan.h, the same statement"),
)

# What the dispatch code instantiates (seeq_device.hip: run_setup's SEEQ_STREAM_FN, SEEQ_MYERS_FN, SEEQ_PAIR_FN and k_direct; seg_post's seeq_launch_verify / _emit1 / _emit_all,
# SEEQ_COUNT1, SEEQ_EMIT1, the leaders and the hit-list kernels), spelled as the parts of a key: each is in a
# key of the census or in UNREACHABLE -- the ledger test says which one is neither
COMPILED = tuple(
    ["k_pair<%d,%s>" % (wu, v) for wu in (4, 5, 6, 7, 8) for v in ("plain", "FA", "IG", "LL")] +
    ["k_stream<%d,%s>" % (wu, v) for wu in (4, 6, 8) for v in ("-,-,0", "FA,-,0", "-,LL,0", "FA,LL,0", "-,-,1", "-,LL,1", "-,-,2")] +
    ["k_stream<%d,%s,LL,0,MY%d>" % (wu, fa, my) for wu in (16, 32) for fa in ("-", "FA") for my in (1, 2)] +
    ["k_direct<4,1>", "k_direct<4,2>"] +
    ["k_verify<%d,%s," % (fw, v) for fw in (1, 2) for v in ("ANY", "BEST", "ALL")] +
    ["k_emit1", "k_emit_all<1>", "k_emit_all<2>", "vr512"] +
    ["k_exact1<COUNT,%d,-1,%s>" % (fw, wk) for fw in (1, 2) for wk in ("-", "WK")] +
    ["k_exact1<EMIT,%d,%s,%s>" % (fw, o, wk) for fw in (1, 2) for o in ("BEST", "-1") for wk in ("-", "WK")] +
    ["+leaders |", "+leaders(best)", "k_lead_lines", "k_lead_best", "k_count_nonzero", "order2", "k_stream_reorder+k_stream_bounds", "k_fused_reorder"])


def _row_of(key, inp):
    assert inp["flags"] in (0, FLAG_SAMPLE_DIRTY), "a key that only a fall-back flag reaches: give Row and the GPU test a way to set it"
    recipe = "fasta-per-read" if inp["flags"] else "reads" if inp["avg_line"] <= 600 else "long-N" if 2 * inp["tau"] >= len(plain_pattern(inp["pattern"])) else "long"
    knobs = {"SEEQ_FUSED_KERNEL": KERNEL_KNOB[inp["kernel"]]} if inp["kernel"] else {}
    return Row(key, inp["pattern"], inp["tau"], options_text(inp["options"]), WANT_NAMES[inp["want"]], inp["avg_line"], recipe, knobs)


def choose_rows(cand, orc, log=None):
    """REPRESENTATIVES anew: a row per key of `cand` (census_all(), or a part of it), at the key's lowest level of knobs, on as few (pattern, tau) as
    will do -- greedily, the pair that serves most open keys next -- and only rows whose text passes `vacuity` with the oracle `orc`.
    -> ({key: Row}, the keys left without one)"""
    by_pair = {}
    for key, (lv, inputs) in cand.items():
        for inp in inputs:
            by_pair.setdefault((inp["pattern"], inp["tau"]), {}).setdefault(key, inp)
    open_keys, chosen, tried = set(cand), {}, set()
    memo = {}
    while open_keys:
        # (a pair with 2 <= tau <= m / 4 -- edits to get wrong, near misses that are near -- counts five times)
        pair = max((p for p in by_pair if p not in tried),
                   key=lambda p: (len(open_keys & set(by_pair[p])) * (5 if 2 <= p[1] <= len(plain_pattern(p[0])) // 4 else 1), -p[1]), default=None)
        if pair is None or not open_keys & set(by_pair[pair]):
            break
        tried.add(pair)
        for key in sorted(open_keys & set(by_pair[pair])):
            row = _row_of(key, by_pair[pair][key])
            plan = row.plan()
            text = row.text(plan)
            mk = (id(text), row.options & 0x0C)
            if mk not in memo:
                memo[mk] = (text, orc.buffer_scan(row.pattern, row.tau, text.buf, SQ_ALL | (row.options & 0x0C), fasta=row.fasta))
            why = vacuity(row, text, memo[mk][1], plan)
            if log:
                log("%s tau %d: %s -> %s" % (pair[0], pair[1], key, why or "ok"))
            if why is None:
                chosen[key] = row
                open_keys.discard(key)
    return chosen, sorted(open_keys)


if __name__ == "__main__":
    t0 = time.time()
    if "--rows" in sys.argv:
        from oracle.pyoracle import Oracle
        chosen, missing = choose_rows(census_all(), Oracle(), log=lambda s: sys.stderr.write(s + "\n"))
        print('"""One scan per kernel-instance key (tests/kernel_instances.py: Row says what the columns are) -- written by\n'
              '`python tests/kernel_instances.py --rows`, which picks them from the census and checks each text with the oracle; rows may be edited by hand.\n'
              '%d keys, %d of them reached without a knob."""' % (len(chosen), sum(1 for r in chosen.values() if not r.knobs)))
        print("REPRESENTATIVES = [")
        for key in sorted(chosen, key=lambda k: (bool(chosen[k].knobs), chosen[k].recipe, k)):
            print(chosen[key].line())
        print("]")
        sys.stderr.write("%d rows, %d keys without one: %s, %.0f s\n" % (len(chosen), len(missing), missing, time.time() - t0))
    else:
        cs = census()
        print("# %d keys, %.1f s" % (len(cs), time.time() - t0))
        for key in sorted(cs, key=lambda k: (cs[k]["kernel"], cs[k]["flags"], k)):
            print(key, cs[key])
