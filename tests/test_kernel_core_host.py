"""CPU: the per-line DEVICE functions (seeq_kernel_core.h), compiled for the host by
tests/host_harness.cpp, fuzzed against the oracle.  This checks the Myers column,
the acceptance rules and the reverse scan before any GPU time is spent; the GPU
tests then check the kernels that call these functions."""
import random
import sys

import numpy as np

import known_answers as KA
from conftest import GOLDEN
from oracle.pyoracle import SQ_ALL, SQ_BEST, SQ_CONVERT, SQ_COUNT, SQ_FAIL, SQ_FIRST, SQ_IGNORE, SQ_STREAM

ANY, COUNT, EMIT = 0, 1, 2


def run(H, oracle, pat, tau, text, opt, mode=EMIT, wforce=0):
    keys, err = oracle.parse(pat)
    assert keys is not None
    tb = text.encode("latin-1")
    out = np.zeros(3 * 4096, dtype=np.uint32)
    n = H.harness_scan(tb, len(tb), bytes(keys), len(keys), tau, opt, mode, wforce, out.ctypes.data, 4096)
    if mode != EMIT:
        return n
    return [tuple(int(x) for x in out[3 * k:3 * k + 3]) for k in range(n)]


def test_pattern_compiler(harness, oracle):
    import ctypes as C
    for pat, keys in KA.PARSE_OK:
        kb = C.create_string_buffer(len(pat) + 1)
        err = C.c_int(0)
        assert harness.harness_compile(pat.encode(), kb, C.byref(err)) == len(keys)
        assert list(kb.raw[:len(keys)]) == keys
    for pat, e in KA.PARSE_ERR + [(p, e) for p, t, e in KA.SEEQNEW_ERR if e in (2, 3, 4, 5)]:
        kb = C.create_string_buffer(len(pat) + 1)
        err = C.c_int(0)
        assert harness.harness_compile(pat.encode(), kb, C.byref(err)) == -1 and err.value == e, pat


def test_known_answers(harness, oracle):
    mode = dict(FIRST=SQ_FIRST, BEST=SQ_BEST, ALL=SQ_ALL)
    for pat, tau, text, mo, exp in KA.STRING_MATCH:
        assert run(harness, oracle, pat, tau, text, mode[mo]) == exp[::-1]


def test_golden_string_cases(harness, oracle, string_cases):
    for c in string_cases:
        got = run(harness, oracle, c["pattern"], c["tau"], c["text"], c["options"])
        assert [list(h) for h in got] == c["hits"][::-1], c


def test_fuzz_vs_oracle(harness, oracle):
    sys.path.insert(0, GOLDEN)
    from make_golden import plain, rand_pattern, rand_text
    rng = random.Random(4242)
    for _ in range(1500):
        pat = rand_pattern(rng)
        m = len(plain(pat))
        tau = rng.randint(0, min(m - 1, rng.choice([0, 1, 2, 3, 3, 5, 8])))
        text = rand_text(rng, pat, tau, rng.choice([0, 1, 5, 20, 60, 150, 250]))
        for mo in (SQ_FIRST, SQ_BEST, SQ_ALL, SQ_COUNT):
            nd = rng.choice([SQ_FAIL, SQ_CONVERT, SQ_IGNORE])
            st = rng.choice([0, 0, SQ_STREAM])
            opt = mo | nd | st
            exp = oracle.string_match(pat, tau, text, opt)[::-1]
            wf = rng.choice([0] + [w for w in (2, 4, 8, 16) if 32 * w >= m])
            assert run(harness, oracle, pat, tau, text, opt, EMIT, wf) == exp, (pat, tau, text, opt, wf)
        allh = oracle.string_match(pat, tau, text, (opt & ~3) | SQ_ALL)
        assert run(harness, oracle, pat, tau, text, opt, ANY) == (1 if allh else 0)
        assert run(harness, oracle, pat, tau, text, opt, COUNT) == len(allh)


def test_string_positions_in_blocks_vs_oracle(harness, oracle, string_cases):
    """Host side of k_string: the positions of a string shared out in blocks (block sizes 1, 2, 7 and 'whole string'),
    every block from a fresh column through sq_emit_window -- the function the kernel's threads call -- with the
    acceptance rules evaluated per position from three consecutive scores: the same hits as the oracle's line-long scan,
    for the golden string cases and random patterns / texts / options.  Strings with a skipped byte before the
    terminator (SQ_IGNORE, SQ_STREAM) are left to the one-lane scan by the kernel (-1 here)."""
    import ctypes as C
    H = harness
    H.harness_string_par.restype = C.c_long
    H.harness_string_par.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_size_t]

    def par(pat, tau, text, opt, block, wforce=0):
        keys, _ = oracle.parse(pat)
        tb = text.encode("latin-1")
        out = np.zeros(3 * 4096, dtype=np.uint32)
        n = H.harness_string_par(tb, len(tb), bytes(keys), len(keys), tau, opt, block, wforce, out.ctypes.data, 4096)
        return None if n < 0 else [tuple(int(x) for x in out[3 * k:3 * k + 3]) for k in range(n)]

    npar = 0
    for c in string_cases:
        for block in (1, 3, 1 << 20):
            got = par(c["pattern"], c["tau"], c["text"], c["options"], block)
            if got is not None:
                npar += 1
                assert [list(h) for h in got] == c["hits"][::-1], (c, block)
    sys.path.insert(0, GOLDEN)
    from make_golden import plain, rand_pattern, rand_text
    rng = random.Random(77)
    for _ in range(1200):
        pat = rand_pattern(rng)
        m = len(plain(pat))
        tau = rng.randint(0, min(m - 1, rng.choice([0, 1, 2, 3, 3, 5, 8])))
        text = rand_text(rng, pat, tau, rng.choice([0, 1, 5, 20, 60, 150, 250, 700]))
        for mo in (SQ_FIRST, SQ_BEST, SQ_ALL, SQ_COUNT):
            opt = mo | rng.choice([SQ_FAIL, SQ_CONVERT, SQ_CONVERT, SQ_IGNORE]) | rng.choice([0, 0, 0, SQ_STREAM])
            wf = rng.choice([0] + [w for w in (2, 4, 8, 16) if 32 * w >= m])
            got = par(pat, tau, text, opt, rng.choice([1, 2, 7, 64, 1 << 20]), wf)
            if got is None:
                continue
            npar += 1
            assert got == oracle.string_match(pat, tau, text, opt)[::-1], (pat, tau, text, opt, wf)
    assert npar > 3000


def _long_cases(oracle, nfresh, seed):
    """(pattern, tau, text, options, hits or None): the reference's long-pattern fixture (tests/golden/ref_long_cases.json), then fresh
    cases of its generator with distances up to m - 1, the three non-DNA modes and SQ_STREAM (hits None: ask the oracle)."""
    import json
    import os
    sys.path.insert(0, GOLDEN)
    from make_golden import LONG_M, long_text, pattern_of_length
    with open(os.path.join(GOLDEN, "ref_long_cases.json")) as f:
        for c in json.load(f):
            for opt, hits in zip(c["options"], c["hits"]):
                yield c["pattern"], c["tau"], c["text"], opt, [tuple(h) for h in hits]
    rng = random.Random(seed)
    for i in range(nfresh):
        m = LONG_M[i % len(LONG_M)]
        pat = pattern_of_length(rng, m)
        tau = rng.choice([rng.randint(0, 8), rng.randint(0, m - 1), m - 1, rng.choice([31, 32, 33, 63, 64, 65])])
        tau = min(tau, m - 1)
        text = long_text(rng, pat, tau, rng.choice([0, m - 1, m, m + 5, 600, 1500]))
        for mo in (SQ_FIRST, SQ_BEST, SQ_ALL):
            yield pat, tau, text, mo | rng.choice([SQ_FAIL, SQ_CONVERT, SQ_IGNORE]) | rng.choice([0, 0, SQ_STREAM]), None


def _one_size_up(m):
    """The next word count the kernels are instantiated for above the pattern's own (0: it has the largest)."""
    own = next(w for w in (1, 2, 4, 8, 16) if 32 * w >= m)
    return 2 * own if own < 16 else 0


def test_long_patterns_scan_vs_oracle(harness, oracle):
    """sq_scan_line<W> at real multi-word lengths (63 .. 512 positions: W = 2, 4, 8, 16 with a full last word, one bit in a new word,
    padded words), distances up to m - 1: records, the any-hit verdict and the count, at the pattern's own word count and one size up."""
    n = nhits = 0
    for pat, tau, text, opt, hits in _long_cases(oracle, 360, 6300):
        exp = (hits if hits is not None else oracle.string_match(pat, tau, text, opt))[::-1]
        m = len(oracle.parse(pat)[0])
        for wf in (0, _one_size_up(m)):
            assert run(harness, oracle, pat, tau, text, opt, EMIT, wf) == exp, (pat, tau, text, opt, wf)
        allh = oracle.string_match(pat, tau, text, (opt & ~3) | SQ_ALL)
        assert run(harness, oracle, pat, tau, text, opt, ANY) == (1 if allh else 0), (pat, tau, text, opt)
        assert run(harness, oracle, pat, tau, text, opt, COUNT, _one_size_up(m) if n % 3 == 0 else 0) == len(allh), (pat, tau, text, opt)
        n += 1
        nhits += len(exp)
    assert n >= 2000 and nhits >= 2000, (n, nhits)


def test_long_patterns_string_positions_in_blocks_vs_oracle(harness, oracle):
    """Host side of k_string<4 / 8 / 16>: a string's positions shared out in blocks of 1, 7, 64 and the whole string, every block from
    a fresh column (sq_emit_window), at 63 .. 512 positions and distances up to m - 1."""
    import ctypes as C
    H = harness
    H.harness_string_par.restype = C.c_long
    H.harness_string_par.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_size_t]
    npar = nhits = 0
    for i, (pat, tau, text, opt, hits) in enumerate(_long_cases(oracle, 240, 6301)):
        if len(text) > 700 and i % 4:
            continue                                       # (block size 1 is O(n x (m + tau)) column steps: a quarter of the long texts)
        keys, _ = oracle.parse(pat)
        tb = text.encode("latin-1")
        exp = (hits if hits is not None else oracle.string_match(pat, tau, text, opt))[::-1]
        for block in (1, 7, 64, 1 << 20):
            out = np.zeros(3 * 4096, dtype=np.uint32)
            wf = _one_size_up(len(keys)) if block == 7 else 0
            n = H.harness_string_par(tb, len(tb), bytes(keys), len(keys), tau, opt, block, wf, out.ctypes.data, 4096)
            if n < 0:
                break                                      # a skipped byte in front of the terminator: the kernel's one-lane scan
            npar += 1
            nhits += n
            assert [tuple(int(x) for x in out[3 * k:3 * k + 3]) for k in range(n)] == exp, (pat, tau, text, opt, block, wf)
    assert npar >= 2000 and nhits >= 1500, (npar, nhits)


def test_stream_automaton_vs_oracle(harness, oracle):
    """Host side of k_stream: the complete Levenshtein automaton (seeq_dfa.h) walked chunk by chunk with a warm-up,
    exactly as the kernel decomposes the text, reports a first-hit event in a line iff the oracle finds a hit in it
    (clean text: A C G T N, both cases, newlines) -- for chunk sizes 128 / 64 / 16 and the smallest legal warm-up."""
    import ctypes as C
    harness.harness_dfa_stream.restype = C.c_long
    harness.harness_dfa_stream.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    rng = random.Random(11)
    cases = [("GATGTAGCGCGATTAGCCTG", 3), ("GATTAGC", 1), ("CACAGAT", 3), ("ACGT", 1), ("A", 0), ("ACNNGT[AC]TTG", 2),
             ("GATGTAGCGCGATTAGCCTGAAAATG", 2), ("TTTTTTTT", 2), ("GATGTAGCGCGATTAG", 4)]
    for pat, tau in cases:
        keys, _ = oracle.parse(pat)
        m = len(keys)
        core = "".join("ACGT"[(k & -k).bit_length() - 1] if k != 0x1F else "N" for k in keys)
        lines = []
        for _ in range(400):
            n = rng.choice([0, 3, 20, 60, 150, 151, 400])
            t = [rng.choice("ACGT") for _ in range(n)]
            if n >= m and rng.random() < 0.5:
                c = list(core.replace("N", "A"))
                for _e in range(rng.randint(0, tau + 2)):
                    i = rng.randrange(len(c))
                    k = rng.randrange(3)
                    if k == 0:
                        c[i] = rng.choice("ACGT")
                    elif k == 1 and len(c) > 1:
                        del c[i]
                    else:
                        c.insert(i, rng.choice("ACGT"))
                p = rng.randrange(0, max(1, n - len(c) + 1))
                t[p:p + len(c)] = c
            if n and rng.random() < 0.1:
                t[rng.randrange(len(t))] = "N"
            s = "".join(t)[:n]
            lines.append(s.lower() if rng.random() < 0.05 else s)
        buf = ("\n".join(lines) + "\n").encode()
        exp = oracle.buffer_scan(pat, tau, buf, SQ_FIRST)
        want = sorted(set(int(x) for x in exp["records"][:, 0]))
        starts = np.cumsum([0] + [len(x) + 1 for x in lines])            # byte offset of every line
        for chunk in (128, 64, 16):
            warm = m + tau - 1
            out = np.zeros(1 << 16, dtype=np.uint64)
            ns = C.c_uint32(0)
            ne = harness.harness_dfa_stream(buf, len(buf), bytes(keys), m, tau, chunk, warm, out.ctypes.data, out.size,
                                            C.byref(ns))
            assert ne >= 0, (pat, tau)
            got = sorted(set(int(np.searchsorted(starts, int(p), side="right")) for p in out[:ne]))   # 1-based line numbers
            assert got == want, (pat, tau, chunk)
        if (pat, tau) == ("GATGTAGCGCGATTAGCCTG", 3):
            assert ns.value == 3342


def test_filter_automaton_is_a_superset(harness, oracle):
    """Host side of k_stream for patterns whose complete automaton does not fit: the partition filter automaton
    (seeq_dfa.h) walked chunk by chunk with its own warm-up flags EVERY line the oracle finds a hit in (and few
    others) -- BASELINE configs[4]'s pattern and random class/N patterns of 24..62 positions, distances up to 6."""
    import ctypes as C
    sys.path.insert(0, GOLDEN)
    from make_golden import mutate, plain
    harness.harness_dfa_filter.restype = C.c_long
    harness.harness_dfa_filter.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    rng = random.Random(77)
    cases = [("GATG[TA]AGCNCGATTAGC[CG]TGAAAATGNGAGTAC[GAT]GCGCGA", 5, 0), ("GATGTAGCGCGATTAGCCTGAAAA", 3, 0),
             ("GATGTAGCGCGATTAGCCTG", 4, 0), ("GATGTAGCGCGATTAGCCTG", 3, 2), ("GATGTAGCGCGATTAGCCTG", 3, 4),
             ("GATGAAGCACGATTAGCCTGAAAATGAGAG", 5, 0)]
    for _ in range(6):
        m = rng.choice([24, 31, 40, 50, 62])
        pat = "".join("N" if rng.random() < 0.05 else "[" + "".join(rng.sample("ACGT", 2)) + "]" if rng.random() < 0.08
                      else rng.choice("ACGT") for _ in range(m))
        cases.append((pat, rng.randint(2, 6), 0))
    seen_filter = 0
    for pat, tau, parts in cases:
        keys, _ = oracle.parse(pat)
        m = len(keys)
        core = plain(pat)
        lines = []
        for i in range(500):
            n = rng.choice([0, 20, 150, 250, 400])
            t = "".join(rng.choice("ACGT") for _ in range(n))
            if i % 3 == 0 and n >= m:
                cp = mutate(rng, core, rng.randint(0, tau + 2))
                q = rng.randrange(n - len(cp) + 1) if n >= len(cp) else 0
                t = (t[:q] + cp + t[q + len(cp):])[:n]
            if i % 41 == 0 and n:
                q = rng.randrange(n)
                t = t[:q] + "N" + t[q + 1:]
            lines.append(t.lower() if i % 29 == 0 else t)
        buf = ("\n".join(lines) + "\n").encode()
        want = set(int(x) for x in oracle.buffer_scan(pat, tau, buf, SQ_FIRST)["records"][:, 0])
        assert len(want) > 20
        starts = np.cumsum([0] + [len(x) + 1 for x in lines])
        for chunk in (128, 64):
            out = np.zeros(1 << 16, dtype=np.uint64)
            info = (C.c_uint32 * 4)()
            ne = harness.harness_dfa_filter(buf, len(buf), bytes(keys), m, tau, parts, chunk, out.ctypes.data, out.size, info)
            if ne < 0:
                continue                                   # nothing fits: the per-line kernel serves this pattern
            got = set(int(np.searchsorted(starts, int(p), side="right")) for p in out[:ne])
            assert want <= got, (pat, tau, parts, chunk, sorted(want - got)[:5])
            assert info[2] <= 32 and info[0] <= 4000
            if info[1] > 1:
                seen_filter += 1
                # selectivity: beyond the planted near misses (copies with tau+1 / tau+2 edits, at most 1 line in 3 holds a
                # copy at all) the false candidates are what the library's accept-rate estimate predicts for random text
                extra = len(got - want)
                assert extra <= len(lines) // 3 - len(want) + 5 + 6 * (info[3] * 1e-9) * len(buf), (pat, tau, extra, info[3])
    assert seen_filter >= 8


def test_restart_table_names_every_occurrence_on_long_lines(harness, oracle):
    """Round 5, the long-line filter's restart table (seeq_dfa_restart_variant) under the kernel's chunked walk: EVERY occurrence the oracle
    reports on a long line (SQ_ALL records) holds a candidate -- a position s <= c <= e -- so that the exact pass may scan m + tau either side
    of a candidate and nothing else (seeq_exact1.h, ScanArgs.ll_restart).  The absorbing table of round 4 does not have the property (one
    candidate per chain and line): checked too, so that the test would notice if it were handed the wrong table."""
    import ctypes as C
    sys.path.insert(0, GOLDEN)
    from make_golden import mutate, plain
    harness.harness_dfa_filter_restart.restype = C.c_long
    harness.harness_dfa_filter_restart.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    harness.harness_dfa_filter.restype = C.c_long
    harness.harness_dfa_filter.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    rng = random.Random(505)
    full = "GATGTAGCGCGATTAGCCTGAAAATGCGAGTACGGCGCGAAT"
    cases = [(full[:34], 6, 0), (full[:34], 8, 0), (full[:27], 4, 0), (full[:27], 5, 0), (full, 8, 0), ("GATGTAGCGCGATTAGCCTGAAAA", 3, 0),
             ("GATG[TA]AGCNCGATTAGC[CG]TGAAAATGNGAGTAC[GAT]GCGCGA", 5, 0), (full[:34], 6, 2), (full[:30], 5, 3)]
    checked = absorbing_misses = 0
    for pat, tau, parts in cases:
        keys, _ = oracle.parse(pat)
        m = len(keys)
        core = plain(pat)
        lines = []
        for _ in range(3):                                  # long lines with copies all over: clean hits, near misses, tandem copies
            n = rng.choice([20000, 40000])
            t = [rng.choice("ACGT") for _ in range(n)]
            q = rng.randrange(0, 300)
            while q + 2 * m + 20 < n:
                cp = mutate(rng, core.replace("N", "A"), rng.randint(0, tau + 2))
                t[q:q + len(cp)] = list(cp)
                if rng.random() < 0.2:                      # a tandem copy right behind
                    cp2 = mutate(rng, core.replace("N", "A"), rng.randint(0, tau))
                    t[q + len(cp):q + len(cp) + len(cp2)] = list(cp2)
                q += rng.choice([m + 3, 150, 400, 1000])
            lines.append("".join(t[:n]))
        buf = ("\n".join(lines) + "\n").encode()
        starts = np.cumsum([0] + [len(x) + 1 for x in lines])
        rec = oracle.buffer_scan(pat, tau, buf, SQ_ALL)["records"]
        assert len(rec) > 50
        occ = [(int(starts[int(l) - 1]) + int(s_), int(starts[int(l) - 1]) + int(e) - 1) for l, s_, e, _d in rec.tolist()]     # absolute [s, e]
        for chain in (64, 128):
            out = np.zeros(1 << 18, dtype=np.uint64)
            info = (C.c_uint32 * 4)()
            ne = harness.harness_dfa_filter_restart(buf, len(buf), bytes(keys), m, tau, parts, chain, 0, out.ctypes.data, out.size, info)
            if ne < 0:
                continue
            cand = np.sort(out[:ne].astype(np.int64))
            for s_, e in occ:
                k = int(np.searchsorted(cand, s_, side="left"))
                assert k < len(cand) and cand[k] <= e, (pat, tau, parts, chain, s_, e, cand[max(0, k - 1):k + 2].tolist())
                checked += 1
            ne2 = harness.harness_dfa_filter(buf, len(buf), bytes(keys), m, tau, parts, chain, out.ctypes.data, out.size, info)
            cand2 = np.sort(out[:max(ne2, 0)].astype(np.int64))
            for s_, e in occ:
                k = int(np.searchsorted(cand2, s_, side="left"))
                absorbing_misses += not (k < len(cand2) and cand2[k] <= e)
    assert checked > 2000 and absorbing_misses > 100, (checked, absorbing_misses)


def _pair_events(harness, buf, keys, m, tau, chain=64, warm=0):
    import ctypes as C
    harness.harness_pair_walk.restype = C.c_long
    harness.harness_pair_walk.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    out = np.zeros(1 << 17, dtype=np.uint64)
    info = (C.c_uint32 * 6)()
    ne = harness.harness_pair_walk(buf, len(buf), bytes(keys), m, tau, chain, warm, out.ctypes.data, out.size, info)
    return ne, out[:max(ne, 0)], list(info)


def test_pair_automaton_is_a_superset_and_its_first_candidate_bounds_the_scan(harness, oracle):
    """Host side of k_pair (seeq_dfa.h section 3): the pair automaton of the pattern's longest prefix that fits, walked
    two bytes per step in 64-byte chains with the kernel's warm-up and restart-on-accept, over text where every byte
    outside A C G T aliases onto a base (newline -> C, N -> G):
      (1) every line the oracle finds a hit in gets a candidate (position of a pair's second byte; the line is the one
          that byte lies in, a newline belonging to the line it ends);
      (2) the exact pass may start m + tau columns before a line's FIRST candidate: the oracle over that suffix reports
          the same hits (shifted) as over the whole line -- for SQ_ALL, hence for every match option."""
    sys.path.insert(0, GOLDEN)
    from make_golden import mutate, plain
    rng = random.Random(2026)
    cases = [("GATGTAGCGCGATTAGCCTG", 3), ("GATTAGC", 1), ("CACAGAT", 3), ("ACGT", 1), ("AC", 0), ("ACNNGT[AC]TTG", 2),
             ("GATGTAGCGCGATTAGCCTGAAAATG", 2), ("TTTTTTTT", 2), ("GATGTAGCGCGATTAG", 4), ("GATGTAGCGCGATTAGCCTGAAAA", 3),
             ("GATG[TA]AGCNCGATTAGC[CG]TGAAAATGNGAGTAC[GAT]GCGCGA", 5), ("AAAAAAAAAAAAAAAAAAAA", 3), ("ACGTACGTACGTACGT", 2)]
    for _ in range(8):
        m = rng.choice([6, 12, 20, 31, 45])
        pat = "".join("N" if rng.random() < 0.05 else "[" + "".join(rng.sample("ACGT", 2)) + "]" if rng.random() < 0.08
                      else rng.choice("ACGT") for _ in range(m))
        cases.append((pat, rng.randint(0, min(5, m - 2))))
    nwalked = 0
    for pat, tau in cases:
        keys, _ = oracle.parse(pat)
        m = len(keys)
        core = plain(pat)
        lines = []
        for i in range(500):
            n = rng.choice([0, 1, 3, 20, 60, 150, 151, 400])
            t = "".join(rng.choice("ACGT") for _ in range(n))
            if i % 2 == 0 and n >= m:
                cp = mutate(rng, core.replace("N", "A"), rng.randint(0, tau + 2))
                q = rng.choice([0, 0, max(0, n - len(cp)), rng.randrange(max(1, n - len(cp) + 1))])   # also flush with either end of the line
                t = (t[:q] + cp + t[q + len(cp):])[:n]
            if i % 17 == 0 and n:
                q = rng.randrange(n)
                t = t[:q] + "N" + t[q + 1:]
            lines.append(t.lower() if i % 29 == 0 else t)
        if len(set(core)) <= 2:
            # periodic patterns: occurrences overlap and follow each other across line ends, so walks restart inside their
            # warm-up windows -- runs of the pattern's own bases, m - tau - 1 .. m + 2 long, at either end of short lines
            lines = []
            for i in range(3000):
                unit = core[:2] if len(set(core)) == 2 else core[:1]
                run = (unit * m)[:rng.randint(max(1, m - tau - 1), m + 2)]
                junk = lambda k: "".join(rng.choice("ACGT") for _ in range(k))
                lines.append(rng.choice([run + junk(rng.randint(0, 50)), junk(rng.randint(0, 50)) + run,
                                         run, junk(rng.randint(0, 30)) + run + junk(rng.randint(0, 30))]))
        buf = ("\n".join(lines) + ("\n" if rng.random() < 0.5 else "")).encode()
        exp = oracle.buffer_scan(pat, tau, buf, SQ_ALL)
        want = {}
        for ln, st, en, di in exp["records"]:
            want.setdefault(int(ln), []).append((int(st), int(en), int(di)))
        starts = np.cumsum([0] + [len(x) + 1 for x in lines])            # byte offset of every line
        for chain, warm in ((64, 0), (64, 32), (16, 0)):
            ne, ev, info = _pair_events(harness, buf, keys, m, tau, chain, warm)
            if ne < 0:
                continue                                   # no prefix of >= tau + 2 positions fits: another kernel serves the pattern
            nwalked += 1
            assert info[0] + 5 <= 2047 and info[0] <= info[1] and tau + 2 <= info[2] <= m and info[3] <= 32
            assert info[5] > 1 or info[3] == info[2] + tau - 1
            first = {}
            for p in ev:
                p = int(p)
                ln = int(np.searchsorted(starts, p, side="right"))        # 1-based; a newline at p belongs to the line it ends
                first.setdefault(ln, p - int(starts[ln - 1]))
            missing = sorted(set(want) - set(first))
            assert not missing, (pat, tau, chain, warm, missing[:5])
            for ln, hits in want.items():
                col = first[ln]
                pos = max(0, col - (m + tau))
                line = lines[ln - 1]
                sub = oracle.string_match(pat, tau, line[pos:], SQ_ALL)[::-1]
                assert [(s + pos, e + pos, d) for s, e, d in sub] == hits, (pat, tau, chain, ln, col, pos)
        if (pat, tau) == ("GATGTAGCGCGATTAGCCTG", 3):
            assert info[2] == 17 and info[1] == 1839, info
    assert nwalked >= 40


def test_pair_automaton_names_every_occurrence_on_long_lines(harness, oracle):
    """Round 5, k_pair's long-line variant: with every flag of a chain kept, EVERY occurrence the oracle reports on a long line holds a
    candidate or ends on the byte before one (s <= c <= e + 1: a candidate is the second byte of a pair) -- what the window walk's
    m + tau + 1 columns either side of a candidate rest on (seeq_pair.h LL, seeq_exact1.h ll_restart)."""
    sys.path.insert(0, GOLDEN)
    from make_golden import mutate, plain
    rng = random.Random(506)
    full = "GATGTAGCGCGATTAGCCTGAAAATGCGAGTACGGCGCGAAT"
    checked = 0
    for pat, tau in ((full[:20], 3), (full[:27], 3), (full[:27], 5), (full[:34], 5), (full[:34], 7), ("GATG[TA]AGCNCGATTAGC[CG]TGAAAATGNGAGTAC[GAT]GCGCGA", 5)):
        keys, _ = oracle.parse(pat)
        m = len(keys)
        core = plain(pat)
        lines = []
        for _ in range(3):
            n = rng.choice([20000, 40000])
            t = [rng.choice("ACGT") for _ in range(n)]
            q = rng.randrange(0, 300)
            while q + 2 * m + 20 < n:
                cp = mutate(rng, core.replace("N", "A"), rng.randint(0, tau + 2))
                t[q:q + len(cp)] = list(cp)
                if rng.random() < 0.2:
                    cp2 = mutate(rng, core.replace("N", "A"), rng.randint(0, tau))
                    t[q + len(cp):q + len(cp) + len(cp2)] = list(cp2)
                q += rng.choice([m + 3, 150, 400, 1000])
            lines.append("".join(t[:n]))
        buf = ("\n".join(lines) + "\n").encode()
        starts = np.cumsum([0] + [len(x) + 1 for x in lines])
        rec = oracle.buffer_scan(pat, tau, buf, SQ_ALL)["records"]
        assert len(rec) > 50
        ne, ev, info = _pair_events(harness, buf, keys, m, tau)
        assert ne > 0, (pat, tau)
        cand = np.sort(ev.astype(np.int64))
        for l, s_, e, _d in rec.tolist():
            a, b = int(starts[int(l) - 1]) + int(s_), int(starts[int(l) - 1]) + int(e) - 1      # the occurrence, absolute [a, b]
            k = int(np.searchsorted(cand, a, side="left"))
            assert k < len(cand) and cand[k] <= b + 1, (pat, tau, a, b, cand[max(0, k - 1):k + 2].tolist())
            checked += 1
    assert checked > 1500, checked


def test_quad_automaton_flags_every_hit_read_and_bounds_its_window(harness, oracle):
    """Host side of the packed walk's four-bases-per-step table (seeq_dfa.h section 3b): every line is a read walked from the root,
    a packed byte per step.  (1) Every read the oracle finds a hit in gets a candidate; (2) the exact pass over the window
    [first candidate - (m + tau), last candidate + m + tau + 2) of the read reports the read's own hits (SQ_ALL, hence every
    option) -- what k_verify_packed scans; (3) the headline pattern is served by its two-part filter: 95 states."""
    import ctypes as C
    sys.path.insert(0, GOLDEN)
    from make_golden import mutate, plain
    rng = random.Random(4242)
    harness.harness_quad_walk.restype = C.c_long
    harness.harness_quad_walk.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    cases = [("GATGTAGCGCGATTAGCCTG", 3), ("GATTAGC", 1), ("CACAGAT", 3), ("ACGT", 1), ("ACNNGT[AC]TTG", 2), ("GATGTAGCGCGATTAGCCTGAAAATG", 2),
             ("TTTTTTTT", 2), ("GATGTAGCGCGATTAG", 4), ("GATG[TA]AGCNCGATTAGC[CG]TGAAAATGNGAGTAC[GAT]GCGCGA", 5), ("AAAAAAAAAAAAAAAAAAAA", 3),
             ("ACGTACGTACGTACGT", 2), ("GATGTAGCGCGATTAGCCTG", 1), ("GATGTAGCGCGATTAGCCTG", 5)]
    for _ in range(8):
        m = rng.choice([6, 12, 20, 31, 45])
        pat = "".join("N" if rng.random() < 0.05 else "[" + "".join(rng.sample("ACGT", 2)) + "]" if rng.random() < 0.08
                      else rng.choice("ACGT") for _ in range(m))
        cases.append((pat, rng.randint(0, min(5, m - 2))))
    nwalked = 0
    for pat, tau in cases:
        keys, _ = oracle.parse(pat)
        m = len(keys)
        core = plain(pat)
        lines = []
        for i in range(600):
            n = rng.choice([1, 3, 20, 60, 150, 151, 250])
            t = "".join(rng.choice("ACGT") for _ in range(n))
            if i % 2 == 0 and n >= m:
                cp = mutate(rng, core.replace("N", "A"), rng.randint(0, tau + 2))
                q = rng.choice([0, 0, max(0, n - len(cp)), rng.randrange(max(1, n - len(cp) + 1))])
                t = (t[:q] + cp + t[q + len(cp):])[:n]
            if len(set(core)) <= 2 and i % 3 == 0:
                unit = core[:2] if len(set(core)) == 2 else core[:1]
                t = ((unit * m)[:rng.randint(max(1, m - tau - 1), m + 2)] + t)[:max(n, 1)]
            if i % 17 == 0:
                q = rng.randrange(n)
                t = t[:q] + "N" + t[q + 1:]                  # (an N aliases onto G in the walk: a superset)
            lines.append(t)
        buf = ("\n".join(lines) + "\n").encode()
        exp = oracle.buffer_scan(pat, tau, buf, SQ_ALL)
        want = {}
        for ln, st, en, di in exp["records"]:
            want.setdefault(int(ln), []).append((int(st), int(en), int(di)))
        out = np.zeros(1 << 18, dtype=np.uint64)
        info = (C.c_uint32 * 5)()
        ne = harness.harness_quad_walk(buf, len(buf), bytes(keys), m, tau, out.ctypes.data, out.size, info)
        if ne < 0:
            continue
        assert ne <= out.size
        nwalked += 1
        assert 1 <= info[0] <= 127 and info[0] <= info[1], list(info)
        starts = np.cumsum([0] + [len(x) + 1 for x in lines])
        first, last = {}, {}
        for p in out[:ne]:
            p = int(p)
            ln = int(np.searchsorted(starts, p, side="right"))
            col = p - int(starts[ln - 1])
            first.setdefault(ln, col)
            last[ln] = col
        missing = sorted(set(want) - set(first))
        assert not missing, (pat, tau, missing[:5])
        for ln, hits in want.items():
            line = lines[ln - 1]
            pos = max(0, first[ln] - (m + tau))
            stop = min(len(line), last[ln] + m + tau + 2)
            sub = oracle.string_match(pat, tau, line[pos:stop], SQ_ALL)[::-1]
            assert [(s + pos, e + pos, d) for s, e, d in sub] == hits, (pat, tau, ln, first[ln], last[ln])
        if (pat, tau) == ("GATGTAGCGCGATTAGCCTG", 3):
            assert info[0] == 95 and info[3] == 2, list(info)
    assert nwalked >= 12, nwalked


def test_quad_automaton_under_the_chunked_walk(harness, oracle):
    """The quad table under the ASCII walk of seeq_pair.h (QD): 64-byte chains, each warmed up over the automaton's own warm-up (whole words)
    and restarted when it accepts, newlines and N aliased onto bases.  (1) every line with a hit gets a candidate (the line of the
    candidate's byte, a newline belonging to the line it ends); (2) the oracle over the line from m + tau columns before its FIRST candidate
    reports the line's own hits -- what the exact pass scans."""
    import ctypes as C
    sys.path.insert(0, GOLDEN)
    from make_golden import mutate, plain
    rng = random.Random(777001)
    harness.harness_quad_chain_walk.restype = C.c_long
    harness.harness_quad_chain_walk.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                C.POINTER(C.c_uint32)]
    cases = [("GATGTAGCGCGATTAGCCTG", 3), ("GATTAGC", 1), ("CACAGAT", 3), ("ACNNGT[AC]TTG", 2), ("GATGTAGCGCGATTAGCCTGAAAATG", 2), ("TTTTTTTT", 2),
             ("GATGTAGCGCGATTAG", 4), ("AAAAAAAAAAAAAAAAAAAA", 3), ("ACGTACGTACGTACGT", 2), ("GATGTAGCGCGATTAGCCTG", 1), ("GATGTAGCGCGATTAGCCTG", 5)]
    for _ in range(6):
        m = rng.choice([6, 12, 20, 31])
        pat = "".join("N" if rng.random() < 0.05 else "[" + "".join(rng.sample("ACGT", 2)) + "]" if rng.random() < 0.08
                      else rng.choice("ACGT") for _ in range(m))
        cases.append((pat, rng.randint(0, min(4, m - 2))))
    nwalked = 0
    for pat, tau in cases:
        keys, _ = oracle.parse(pat)
        m = len(keys)
        core = plain(pat)
        lines = []
        for i in range(500):
            n = rng.choice([0, 1, 3, 20, 60, 150, 151, 400])
            t = "".join(rng.choice("ACGT") for _ in range(n))
            if i % 2 == 0 and n >= m:
                cp = mutate(rng, core.replace("N", "A"), rng.randint(0, tau + 2))
                q = rng.choice([0, 0, max(0, n - len(cp)), rng.randrange(max(1, n - len(cp) + 1))])
                t = (t[:q] + cp + t[q + len(cp):])[:n]
            if i % 17 == 0 and n:
                q = rng.randrange(n)
                t = t[:q] + "N" + t[q + 1:]
            lines.append(t.lower() if i % 29 == 0 else t)
        if len(set(core)) <= 2:
            lines = []
            for i in range(3000):
                unit = core[:2] if len(set(core)) == 2 else core[:1]
                run = (unit * m)[:rng.randint(max(1, m - tau - 1), m + 2)]
                junk = lambda k: "".join(rng.choice("ACGT") for _ in range(k))
                lines.append(rng.choice([run + junk(rng.randint(0, 50)), junk(rng.randint(0, 50)) + run, run, junk(rng.randint(0, 30)) + run + junk(rng.randint(0, 30))]))
        buf = ("\n".join(lines) + ("\n" if rng.random() < 0.5 else "")).encode()
        exp = oracle.buffer_scan(pat, tau, buf, SQ_ALL)
        want = {}
        for ln, st, en, di in exp["records"]:
            want.setdefault(int(ln), []).append((int(st), int(en), int(di)))
        starts = np.cumsum([0] + [len(x) + 1 for x in lines])
        for chain, warm in ((64, 0), (64, 32), (16, 0)):
            out = np.zeros(1 << 18, dtype=np.uint64)
            info = (C.c_uint32 * 6)()
            ne = harness.harness_quad_chain_walk(buf, len(buf), bytes(keys), m, tau, chain, warm, out.ctypes.data, out.size, info)
            if ne < 0:
                continue
            assert ne <= out.size
            nwalked += 1
            first = {}
            for p in out[:ne]:
                p = int(p)
                ln = int(np.searchsorted(starts, p, side="right"))
                first.setdefault(ln, p - int(starts[ln - 1]))
            missing = sorted(set(want) - set(first))
            assert not missing, (pat, tau, chain, warm, missing[:5])
            for ln, hits in want.items():
                pos = max(0, first[ln] - (m + tau))
                line = lines[ln - 1]
                sub = oracle.string_match(pat, tau, line[pos:], SQ_ALL)[::-1]
                assert [(s + pos, e + pos, d) for s, e, d in sub] == hits, (pat, tau, chain, ln, first[ln], pos)
    assert nwalked >= 24, nwalked


def test_multi_pattern_automata_cover_every_pattern_of_every_line(harness, oracle):
    """Host side of the one-pass multi-pattern scan (seeq_dfa.h section 4): the UNION pair automaton of a barcode set walked
    in 64-byte chains as k_pair walks it, then the resolve automaton over each candidate line's window
    [first candidate - maxspan, last candidate + maxspan + 2):
      (1) every line in which the oracle finds ANY of the patterns gets a candidate;
      (2) the window's pattern mask holds every pattern the oracle finds in the line (exactly those when the automata carry
          the whole patterns);
      (3) each such pattern scanned over the window alone gives the line's own records (SQ_ALL, hence every option)."""
    import ctypes as C
    sys.path.insert(0, GOLDEN)
    from make_golden import mutate, plain
    rng = random.Random(77)
    harness.harness_multi_walk.restype = C.c_long
    harness.harness_multi_walk.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int,
                                           C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    harness.harness_multi_resolve.restype = C.c_int
    harness.harness_multi_resolve.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_size_t, C.c_void_p]
    sets = [(["ACGTTGCA", "TTGACCGA", "GGCATTAC", "CAGTGTCA", "ATATCGCG", "GATTACAG"], [1, 1, 1, 1, 0, 1]),
            (["".join(rng.choice("ACGT") for _ in range(10)) for _ in range(16)], [1] * 16),
            (["".join(rng.choice("ACGT") for _ in range(rng.choice([8, 9, 11, 12]))) for _ in range(16)], [rng.choice([0, 1]) for _ in range(16)]),
            (["ACGTTGCA", "TG[AC]CANNGT", "GATGTAGCGCGATTAGCCTG", "AAAAAAAA"], [1, 1, 3, 2]),
            (["ACACACAC", "CACACACA", "ACACACACAC"], [1, 1, 2])]
    nsets = 0
    for pats, taus in sets:
        keysl = [oracle.parse(p)[0] for p in pats]
        ms = [len(k) for k in keysl]
        cat = bytes(b for k in keysl for b in k)
        npat = len(pats)
        cm = (C.c_int * npat)(*ms); ct = (C.c_int * npat)(*taus)
        lines = []
        for i in range(700):
            n = rng.choice([0, 5, 30, 60, 150, 151, 300])
            t = [rng.choice("ACGT") for _ in range(n)]
            for _ in range(rng.choice([0, 1, 1, 2, 3])):
                k = rng.randrange(npat)
                cp = mutate(rng, plain(pats[k]).replace("N", "A"), rng.randint(0, taus[k] + 1))
                if n >= len(cp):
                    q = rng.choice([0, n - len(cp), rng.randrange(n - len(cp) + 1)])
                    t[q:q + len(cp)] = list(cp)
            if i % 19 == 0 and n:
                t[rng.randrange(n)] = "N"
            t = "".join(t)[:n]
            lines.append(t.lower() if i % 31 == 0 else t)
        if len(set("".join(pats))) <= 2:
            lines += ["AC" * rng.randint(2, 9) + "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 20))) for _ in range(300)]
        buf = ("\n".join(lines) + "\n").encode()
        starts = np.cumsum([0] + [len(x) + 1 for x in lines])
        out = np.zeros(1 << 18, dtype=np.uint64)
        info = (C.c_uint32 * 8)()
        ne = harness.harness_multi_walk(buf, len(buf), cat, cm, ct, npat, 64, out.ctypes.data, out.size, info)
        assert ne >= 0, pats
        nsets += 1
        maxspan = int(info[6])
        assert maxspan == max(m + t for m, t in zip(ms, taus)) and info[0] + 5 <= 2047 and info[3] <= 32
        first, last = {}, {}
        for p in out[:ne]:
            p = int(p)
            ln = int(np.searchsorted(starts, p, side="right"))
            first.setdefault(ln, p - int(starts[ln - 1]))
            last[ln] = p - int(starts[ln - 1])
        want = [{} for _ in pats]
        for k, (pt, tau) in enumerate(zip(pats, taus)):
            for ln, st, en, di in oracle.buffer_scan(pt, tau, buf, SQ_ALL)["records"]:
                want[k].setdefault(int(ln), []).append((int(st), int(en), int(di)))
        hit_lines = set().union(*[set(w) for w in want])
        assert not (hit_lines - set(first)), (pats, sorted(hit_lines - set(first))[:5])
        cand = sorted(first)
        lo = np.array([starts[ln - 1] + max(0, first[ln] - maxspan) for ln in cand], dtype=np.uint64)
        hi = np.array([starts[ln - 1] + min(len(lines[ln - 1]), last[ln] + maxspan + 2) for ln in cand], dtype=np.uint64)
        masks = np.zeros(len(cand), dtype=np.uint32)
        assert harness.harness_multi_resolve(buf, cat, cm, ct, npat, lo.ctypes.data, hi.ctypes.data, len(cand), masks.ctypes.data) == 0
        for ln, a, b, mk in zip(cand, lo, hi, masks):
            truth = sum(1 << k for k in range(npat) if ln in want[k])
            assert (int(mk) & truth) == truth, (pats, ln, bin(int(mk)), bin(truth))
            if info[5] and "N" not in lines[ln - 1].upper():
                assert int(mk) == truth, (pats, ln, bin(int(mk)), bin(truth))
            a, b = int(a - starts[ln - 1]), int(b - starts[ln - 1])
            for k in range(npat):
                if truth >> k & 1:
                    sub = oracle.string_match(pats[k], taus[k], lines[ln - 1][a:b], SQ_ALL)[::-1]
                    assert [(s + a, e + a, d) for s, e, d in sub] == want[k][ln], (pats[k], ln, a, b)
    assert nsets == len(sets)


def test_scan_plans_of_the_baseline_configurations(harness):
    """The planner (seeq_amd/csrc/seeq_plan.h) is a pure host function -- run_segments only executes what it returns -- so which
    kernels serve the BASELINE configurations, the published sweep's cells and the FASTQ shape can be pinned without a GPU."""
    import ctypes as C
    H = harness
    H.harness_plan.restype = C.c_int
    H.harness_plan.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_int)]
    names = ["rc", "path", "fw", "use_stream", "use_pair", "use_myers", "filter", "stream_ll", "stream_sub", "stream_wu", "verify", "order2",
             "leaders", "window_ok", "ll_filter", "skip_back"]

    def plan(expr, tau, options, want, avg_line, flags=0, kernel=0):
        keys = C.create_string_buffer(2048)
        err = C.c_int(0)
        m = H.harness_compile(expr.encode(), keys, C.byref(err))
        assert m > 0
        out = (C.c_int * 16)()
        assert H.harness_plan(keys, m, tau, options, want, avg_line, flags, kernel, out) == 0
        return dict(zip(names, list(out)))
    SQ_BEST, SQ_ALL, SQ_CONVERT, SQ_IGNORE, FASTA = 1, 2, 4, 8, 0x100
    COUNTLINES, COUNTMATCH, RECORDS = 0, 1, 2
    head = "GATGTAGCGCGATTAGCCTG"
    # configs[1] / [2]: 150 bp reads, 20-mer, d = 3 -- k_pair over the prefix automaton, candidate windows, k_verify, three-launch ordering
    for opt, want in ((0, COUNTLINES), (SQ_BEST, RECORDS), (SQ_ALL, RECORDS), (0, COUNTMATCH)):
        p = plan(head, 3, opt, want, 151.0)
        assert (p["rc"], p["path"], p["fw"], p["use_pair"], p["filter"], p["stream_ll"]) == (0, 6, 1, 1, 1, 0), p
        assert p["verify"] == 1 and p["order2"] == 1 and p["window_ok"] == 1 and p["leaders"] == 0 and p["skip_back"] == 23, p
    # configs[4]: 40 positions, d = 5, 250 bp reads, --all: two-word column, a partition filter on k_pair
    p = plan("GATG[TA]AGCNCGATTAGC[CG]TGAAAATGNGAGTAC[GAT]GCGCGA", 5, SQ_ALL, RECORDS, 251.0)
    assert (p["path"], p["fw"], p["use_pair"], p["filter"], p["verify"], p["order2"]) == (6, 2, 1, 1, 1, 1), p
    # SQ_IGNORE on read-length lines: k_pair too since round 5 (a line that holds a skipped byte is named whole by a marker: seeq_pair.h IG), with
    # k_exact1 -- which knows how to skip -- behind it instead of k_verify; k_stream's skip variant where k_pair is told off or the input is FASTA
    p = plan(head, 3, SQ_BEST | SQ_IGNORE, RECORDS, 79.0)
    assert (p["path"], p["use_pair"], p["stream_sub"], p["filter"], p["verify"], p["order2"], p["window_ok"]) == (6, 1, 0, 1, 0, 1, 1), p
    p = plan(head, 3, SQ_BEST | SQ_IGNORE, RECORDS, 79.0, kernel=1)
    assert (p["path"], p["use_pair"], p["stream_sub"], p["filter"], p["verify"], p["order2"]) == (5, 0, 2, 0, 0, 1), p
    # FASTQ-shaped sample (foreign bytes), SQ_FAIL / SQ_CONVERT: k_pair since round 5 (dirty tiles remake their newline masks from registers,
    # k_verify looks at the bytes before a window); FASTA records with such a sample stay with k_stream
    for opt in (SQ_BEST, SQ_BEST | SQ_CONVERT):
        p = plan(head, 3, opt, RECORDS, 79.0, flags=16)
        assert (p["path"], p["use_pair"], p["stream_sub"], p["verify"], p["window_ok"]) == (6, 1, 0, 1, 1), p
    p = plan(head, 3, SQ_BEST | FASTA, RECORDS, 79.0, flags=16)
    assert (p["path"], p["use_pair"]) == (5, 0), p
    # the published sweep (chromosome lines): complete automaton / partition filter on long lines / Myers mode
    # (round 5: where the pair automaton is selective enough k_pair's long-line variant walks, its candidates go through the window walk -- ll_filter 2:
    #  windows of the restart walk; forced onto k_stream the plans of round 4 stay: the complete automaton, the filters' absorbing / restart tables)
    full = "GATGTAGCGCGATTAGCCTGAAAATGCGAGTACGGCGCGAAT"
    p = plan(head, 3, SQ_ALL, RECORDS, 1.3e8)
    assert (p["path"], p["use_pair"], p["stream_ll"], p["filter"], p["ll_filter"], p["leaders"], p["verify"], p["order2"], p["window_ok"]) == (6, 1, 1, 1, 2, 1, 0, 0, 0), p
    p = plan(head, 3, SQ_ALL, RECORDS, 1.3e8, kernel=1)
    assert (p["path"], p["stream_ll"], p["filter"], p["ll_filter"], p["leaders"], p["verify"], p["order2"]) == (5, 1, 0, 0, 1, 0, 0), p
    p = plan(full[:27], 3, SQ_ALL, RECORDS, 1.3e8, kernel=1)          # a selective filter: the absorbing table
    assert (p["path"], p["stream_ll"], p["filter"], p["ll_filter"], p["leaders"]) == (5, 1, 1, 1, 1), p
    p = plan(full[:27], 4, SQ_ALL, RECORDS, 1.3e8, kernel=1)          # filters that flag more than a position in 20 KB walk their restart table
    assert (p["path"], p["stream_ll"], p["filter"], p["ll_filter"], p["leaders"]) == (5, 1, 1, 2, 1), p
    p = plan(full[:34], 7, SQ_ALL, RECORDS, 1.3e8)
    assert (p["path"], p["fw"], p["stream_ll"], p["filter"], p["ll_filter"], p["leaders"]) == (6, 2, 1, 1, 2, 1), p
    p = plan(full[:34], 7, SQ_ALL, RECORDS, 1.3e8, kernel=1)
    assert (p["path"], p["fw"], p["stream_ll"], p["filter"], p["ll_filter"], p["leaders"]) == (5, 2, 1, 1, 2, 1), p
    p = plan(full, 8, SQ_ALL, RECORDS, 1.3e8)                          # (its pair automaton flags 2.4 positions per KB: k_stream's filter, 0.035)
    assert (p["path"], p["stream_ll"], p["filter"]) == (5, 1, 1), p
    p = plan(full, 15, SQ_ALL, RECORDS, 1.3e8)
    assert (p["path"], p["use_myers"], p["fw"], p["stream_ll"], p["filter"]) == (7, 1, 2, 1, 0), p
    # patterns beyond the two-word column, SQ_STREAM input: the generic path; a multi-pattern scan that is not k_pair's: a scan per pattern
    assert plan("ACGT" * 20, 4, 0, COUNTLINES, 151.0)["path"] == 1
    for m in (63, 512):                                                # the first length beyond the two-word column and the longest there is
        long_pat = ("GATGTAGCGCGATTAGCCTGAAAATGCGAGTACGGCGCGAAT" * 13)[:m]
        for opt, want, avg in ((SQ_CONVERT, RECORDS, 151.0), (SQ_IGNORE | SQ_BEST, RECORDS, 151.0), (FASTA | SQ_ALL, RECORDS, 151.0),
                               (SQ_ALL, RECORDS, 1.3e8), (0, COUNTMATCH, 1.3e8), (SQ_CONVERT | FASTA, COUNTLINES, 1.3e8)):
            assert plan(long_pat, 8, opt, want, avg)["path"] == 1, (m, opt, want, avg)
    assert plan(head, 3, 0x10, COUNTLINES, 151.0)["path"] in (1, 3)
    assert plan(head, 3, SQ_IGNORE, COUNTLINES, 151.0, flags=32)["rc"] == -2
    # a context that has met a line of a whole tile (force_ll) goes to the long-line variants: k_pair's own (round 5), k_stream's under SQ_IGNORE
    p = plan(head, 3, SQ_BEST, RECORDS, 151.0, flags=1)
    assert (p["path"], p["use_pair"], p["stream_ll"], p["window_ok"], p["order2"]) == (6, 1, 1, 0, 0), p
    p = plan(head, 3, SQ_BEST | SQ_IGNORE, RECORDS, 151.0, flags=1)
    assert (p["use_pair"], p["stream_ll"]) == (0, 1) or p["path"] in (1, 3), p
    # ... but several patterns in one walk are not kept off k_pair by it: the walk notices a long line itself and gives up (RERUN_NOT_ONE_WALK)
    p = plan(head[:10], 1, SQ_BEST, RECORDS, 151.0, flags=1 | 32)
    assert (p["rc"], p["path"], p["use_pair"], p["stream_ll"], p["window_ok"]) == (0, 6, 1, 0, 1), p
    assert plan(head[:10], 1, SQ_BEST, RECORDS, 1.3e8, flags=32)["rc"] == -2      # (a sample of long lines: a scan per pattern, as before)


def test_workspace_growth_is_grouped_and_every_refusal_leaves_it_whole(harness):
    """The owner of a scan context's buffers (seeq_workspace.h) over fake hooks (host_harness.cpp: harness_ws_script): the call pattern of a
    context -- first growths of five capacity groups, two fixed-size sets, a larger growth of every group, every call once more, free-all --
    run clean, then once for EVERY request of the clean run with that request refused.  After every step the live blocks are the pointers the
    registered slots hold, nothing is released twice or unasked, no slot has lost its block or sits on one smaller than its group's capacity
    says; the refused call returns -1 with its capacity untouched (a fixed-size set: with none of its slots set) and the same call made again
    succeeds."""
    import ctypes as C
    H = harness
    H.harness_ws_script.restype = C.c_int
    H.harness_ws_script.argtypes = [C.c_long, C.c_void_p, C.c_int]
    GROW, MAKE, FREE = 0, 1, 2
    cols = ("kind", "g", "rc", "cap0", "cap", "want", "requests", "live", "held", "bad", "set_held", "members", "lost", "small")

    def script(refuse_at):
        rows = np.zeros((64, len(cols)), dtype=np.int64)
        n = H.harness_ws_script(refuse_at, rows.ctypes.data, 64)
        assert 0 < n < 64
        return [dict(zip(cols, (int(v) for v in row))) for row in rows[:n]]

    def check_invariants(rows, tag):
        for i, r in enumerate(rows):
            assert r["live"] == r["held"], (tag, i, r)             # a block that exists is registered, a registered pointer is a live block
            assert r["bad"] == 0 and r["lost"] == 0 and r["small"] == 0, (tag, i, r)
            if r["kind"] == GROW and r["rc"] == 0:
                assert r["cap"] == max(r["cap0"], r["want"]) and r["set_held"] == r["members"], (tag, i, r)
            if r["kind"] == MAKE and r["rc"] == 0:
                assert r["set_held"] == r["members"], (tag, i, r)
        assert rows[-1]["kind"] == FREE and rows[-1]["live"] == 0 and rows[-1]["held"] == 0, (tag, rows[-1])

    clean = script(0)
    check_invariants(clean, "clean")
    assert all(r["rc"] == 0 for r in clean)
    total = clean[-1]["requests"]
    assert total >= H.harness_ws_members() >= 24                   # every member of every group and set was requested at least once
    assert max(r["live"] for r in clean) == H.harness_ws_members()
    final_cap = {r["g"]: r["cap"] for r in clean if r["kind"] == GROW}
    for n in range(1, total + 1):
        rows = script(n)
        check_invariants(rows, n)
        failed = [i for i, r in enumerate(rows) if r["rc"] != 0]
        assert len(failed) == 1, (n, failed)                       # the N-th request exists in every run: exactly one call meets the refusal
        i = failed[0]
        r = rows[i]
        assert r["rc"] == -1 and r["kind"] in (GROW, MAKE) and r["requests"] >= n > (rows[i - 1]["requests"] if i else 0), (n, r)
        if r["kind"] == GROW:
            assert r["cap"] == r["cap0"] < r["want"], (n, r)
        else:
            assert r["set_held"] == 0, (n, r)                      # all or nothing
        # the script goes on: the same group grows later, the same set is made later
        later = [q for q in rows[i + 1:] if (q["kind"], q["g"]) == (r["kind"], r["g"])]
        assert later and all(q["rc"] == 0 for q in later), (n, r)
        if r["kind"] == GROW:
            assert later[0]["cap"] == later[0]["want"] > r["cap0"], (n, later[0])
        else:
            assert later[0]["set_held"] == later[0]["members"], (n, later[0])
        assert {q["g"]: q["cap"] for q in rows if q["kind"] == GROW} == final_cap, n


def test_a_buffer_grown_with_its_contents_keeps_them_or_stays_as_it_was(harness):
    """ws_grow_keep (seeq_workspace.h) over the fake hooks (host_harness.cpp: harness_ws_keep): one slot grown 0 -> 100 -> 300 bytes (keeping
    100), asked for 200, grown to 1000 (keeping 300), asked again, freed.  Clean: the kept bytes arrive, the old block goes exactly once (one
    live block, no bad release), `want <= cap` asks for nothing.  Every request refused in turn, every copy failed in turn: -1, and slot,
    block, contents and capacity are what they were, the new block is given back; the same call made again succeeds.  After ws_free_all every
    block handed out has come back."""
    import ctypes as C
    H = harness
    H.harness_ws_keep.restype = C.c_int
    H.harness_ws_keep.argtypes = [C.c_long, C.c_long, C.c_void_p, C.c_int]
    cols = ("rc", "cap0", "cap", "requests", "live", "bad", "copies", "intact", "same", "size")

    def script(refuse_at, fail_copy_at):
        rows = np.zeros((8, len(cols)), dtype=np.int64)
        n = H.harness_ws_keep(refuse_at, fail_copy_at, rows.ctypes.data, 8)
        assert n == 6
        return [dict(zip(cols, (int(v) for v in row))) for row in rows[:n]]

    clean = script(0, 0)
    assert [r["rc"] for r in clean] == [0] * 6 and all(r["bad"] == 0 and r["intact"] == 1 for r in clean), clean
    assert [(r["cap0"], r["cap"], r["size"]) for r in clean[:5]] == [(0, 100, 100), (100, 300, 300), (300, 300, 300), (300, 1000, 1000), (1000, 1000, 1000)]
    assert [r["live"] for r in clean] == [1, 1, 1, 1, 1, 0]            # the old block went with every growth; free-all gave the last one back
    assert [r["requests"] for r in clean] == [1, 2, 2, 3, 3, 3] and [r["copies"] for r in clean] == [0, 1, 1, 2, 2, 2]
    assert [r["same"] for r in clean[:5]] == [0, 0, 1, 0, 1]           # want <= cap: nothing asked for, nothing copied, nothing moved
    assert clean[5]["size"] == -1
    for refuse_at, fail_copy_at in [(n, 0) for n in (1, 2, 3)] + [(0, n) for n in (1, 2)]:
        rows = script(refuse_at, fail_copy_at)
        tag = (refuse_at, fail_copy_at)
        failed = [i for i, r in enumerate(rows) if r["rc"] != 0]
        assert len(failed) == 1 and all(r["bad"] == 0 for r in rows), (tag, rows)
        i = failed[0]
        r, before = rows[i], (rows[i - 1] if i else dict(cap=0, size=-1, live=0))
        assert r["rc"] == -1 and r["cap"] == r["cap0"] == before["cap"] and r["same"] == 1 and r["size"] == before["size"], (tag, r)
        assert r["intact"] == 1 and r["live"] == before["live"], (tag, r)      # contents as they were; the new block (a failed copy) given back
        assert r["requests"] == (refuse_at or before.get("requests", 0) + 1), (tag, r)
        later = rows[i + 1:-1]
        assert all(q["rc"] == 0 and q["intact"] == 1 for q in later), (tag, later)
        if i in (1, 3):                                                # asked again (300: by the growth to 1000 that follows): it grows, contents kept
            assert rows[4]["cap"] == 1000 and rows[4]["size"] == 1000 and rows[4]["live"] == 1, (tag, rows[4])
        assert rows[-1]["live"] == 0 and rows[-1]["size"] == -1, (tag, rows[-1])


# ---- the re-run policy (seeq_amd/csrc/seeq_rerun.h) over host_harness.cpp.  Every expected number below is written out from the arithmetic the
#      host driver carried before the policy had a header of its own: a grown capacity is need + need // 8 + 64. ----
OVF_LINES, OVF_HITLINES, OVF_RECORDS, OVF_NO_STREAM, OVF_NONDNA, OVF_LONG_LINES, OVF_BAD_ENTRY, OVF_SEAM, OVF_LEADER = 1, 2, 4, 8, 16, 32, 64, 128, 256
DONE, AGAIN, BAD_ENTRY, NOT_ONE_WALK, NO_CONVERGENCE = range(5)
MAX_RUNS = 8


def _decide(H, cap, overflow, need=(0, 0, 0), per=None, run=0):
    """-> (verdict, (lines, hit lines, records) to reserve, bits to note)"""
    import ctypes as C
    H.harness_rerun_decide.restype = None
    H.harness_rerun_decide.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    c = np.array(cap, dtype=np.uint64)
    p = np.array(per if per else [[0, 0, 0]], dtype=np.uint64).reshape(-1, 3)
    out = np.zeros(5, dtype=np.uint64)
    H.harness_rerun_decide(run, c.ctypes.data, overflow, need[0], need[1], need[2], len(per) if per else 0, p.ctypes.data, out.ctypes.data)
    return int(out[0]), tuple(int(v) for v in out[1:4]), int(out[4])


def _fallback(H, ops):
    """ops: 0 = age(), else note(op) -> per op a dict of the state after it"""
    import ctypes as C
    H.harness_fallback.restype = None
    H.harness_fallback.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    o = np.array(ops, dtype=np.uint32)
    rows = np.zeros((len(ops), 7), dtype=np.int32)
    H.harness_fallback(o.ctypes.data, len(ops), rows.ctypes.data)
    return [dict(zip(("bits", "ttl", "no_stream", "no_stream_nd", "force_ll", "no_window", "no_leaders"), (int(v) for v in r))) for r in rows]


def test_rerun_decisions_of_a_single_pattern_scan(harness):
    """What seeqdevScanFetch does with the counters of a void run: a workspace whose bit is set grows to need + need / 8 + 64, a line overflow
    brings the hit lines to at least lines / 8 + 64, a fall-back bit is noted and leaves the capacities alone, a bad entry fails the scan."""
    H = harness
    cap = (10, 2, 1)
    assert _decide(H, cap, 0) == (DONE, cap, 0)
    assert _decide(H, cap, 0, need=(1000, 5000, 100000)) == (DONE, cap, 0)                       # needs without their bit say nothing
    need = (1000, 5000, 100000)
    assert _decide(H, cap, OVF_LINES, need) == (AGAIN, (1189, 212, 1), 0)                        # 1000 + 125 + 64; 1189 // 8 + 64
    assert _decide(H, cap, OVF_HITLINES, need) == (AGAIN, (10, 5689, 1), 0)                      # 5000 + 625 + 64
    assert _decide(H, cap, OVF_RECORDS, need) == (AGAIN, (10, 2, 112564), 0)                     # 100000 + 12500 + 64
    assert _decide(H, cap, OVF_LINES | OVF_HITLINES | OVF_RECORDS, need) == (AGAIN, (1189, 5689, 112564), 0)
    # hit lines after a line overflow: the reported need where it is the larger (100 + 12 + 64 = 176 >= 1189 // 8 = 148), else lines // 8 + 64
    assert _decide(H, cap, OVF_LINES | OVF_HITLINES, (1000, 100, 0)) == (AGAIN, (1189, 176, 1), 0)
    assert _decide(H, cap, OVF_LINES | OVF_HITLINES, (1000, 10, 0)) == (AGAIN, (1189, 212, 1), 0)     # 10 + 1 + 64 = 75 < 148
    assert _decide(H, (10, 5000, 1), OVF_LINES, need) == (AGAIN, (1189, 5000, 1), 0)
    assert _decide(H, cap, OVF_RECORDS, (0, 0, 5_000_000_000)) == (AGAIN, (10, 2, 5_625_000_064), 0)   # the record total is 64 bits wide
    # the fall-back bits: exactly the matching flag, 32 scans to live, the capacities as they were
    flag_of = {OVF_NO_STREAM: "no_stream", OVF_NONDNA: "no_stream_nd", OVF_LONG_LINES: "force_ll", OVF_SEAM: "no_window", OVF_LEADER: "no_leaders"}
    for bit, name in flag_of.items():
        assert _decide(H, cap, bit, need) == (AGAIN, cap, bit)
        st = _fallback(H, [bit])[0]
        assert st == dict({n: int(n == name) for n in flag_of.values()}, bits=bit, ttl=32), (bit, st)
    every = sum(flag_of)
    assert every == 0x1B8
    assert _decide(H, cap, every, need) == (AGAIN, cap, every)
    assert _fallback(H, [every])[0] == dict({n: 1 for n in flag_of.values()}, bits=every, ttl=32)
    assert _decide(H, cap, every | OVF_HITLINES, need) == (AGAIN, (10, 5689, 1), every)
    assert _fallback(H, [OVF_LINES | OVF_HITLINES | OVF_RECORDS | OVF_BAD_ENTRY])[0]["bits"] == 0 # only fall-back bits are remembered
    # a bad entry fails the scan whatever else is set, and nothing of that run is noted
    for other in (0, OVF_LINES, OVF_RECORDS | OVF_SEAM, every | 7):
        v, _, note = _decide(H, cap, OVF_BAD_ENTRY | other, need)
        assert (v, note) == (BAD_ENTRY, 0), other


def test_rerun_decisions_of_a_one_walk_multi_scan(harness):
    """The same function in the mode of multi_one_pass: the patterns' largest needs count npat times (their regions share the arrays) and are taken
    only above what the walk's own counters ask for, hit lines after a line overflow are lines / 2 + 64, only the seam flag is remembered, and text
    that is not k_pair's ends the walk with nothing noted."""
    H = harness
    cap = (10, 2, 1)
    quiet = [[0, 0, 0]] * 4
    assert _decide(H, cap, 0, per=quiet) == (DONE, cap, 0)
    per = [[OVF_HITLINES, 300, 0], [0, 100, 0], [OVF_RECORDS, 0, 7000], [OVF_RECORDS, 50, 9000]]
    # (300 + 37 + 64) * 4 = 1604; (9000 + 1125 + 64) * 4 = 40756
    assert _decide(H, cap, 0, per=per) == (AGAIN, (10, 1604, 40756), 0)
    assert _decide(H, cap, 0, per=[[OVF_HITLINES, 300, 9000]] + quiet[1:]) == (AGAIN, (10, 1604, 1), 0)      # a need without its bit says nothing
    assert _decide(H, cap, OVF_HITLINES, (0, 4000, 0), per=per) == (AGAIN, (10, 4564, 40756), 0)             # the walk's 4000 + 500 + 64 is larger
    assert _decide(H, cap, OVF_HITLINES, (0, 100, 0), per=per) == (AGAIN, (10, 1604, 40756), 0)              # ... 100 + 12 + 64 is not
    assert _decide(H, (10, 2, 50000), 0, per=per) == (AGAIN, (10, 1604, 50000), 0)                            # nor is a region sum below the capacity
    assert _decide(H, cap, OVF_LINES, (1000, 0, 0), per=quiet) == (AGAIN, (1189, 658, 1), 0)                  # 1189 // 2 + 64
    assert _decide(H, cap, OVF_LINES, (1000, 0, 0), per=per) == (AGAIN, (1189, 1604, 40756), 0)
    assert _decide(H, cap, OVF_RECORDS, (0, 0, 100000), per=quiet) == (AGAIN, cap, 0)         # records are the patterns' business: the walk's bit grows nothing
    assert _decide(H, cap, OVF_SEAM, per=quiet) == (AGAIN, cap, OVF_SEAM)
    assert _fallback(H, [OVF_SEAM])[0] == dict(bits=OVF_SEAM, ttl=32, no_stream=0, no_stream_nd=0, force_ll=0, no_window=1, no_leaders=0)
    assert _decide(H, cap, OVF_SEAM | OVF_LEADER | OVF_HITLINES, (0, 4000, 0), per=per) == (AGAIN, (10, 4564, 40756), OVF_SEAM)
    for bit in (OVF_NO_STREAM, OVF_NONDNA, OVF_LONG_LINES):
        for other in (0, OVF_SEAM, OVF_LINES | OVF_HITLINES):
            assert _decide(H, cap, bit | other, (1000, 4000, 0), per=per) == (NOT_ONE_WALK, cap, 0), (bit, other)
        assert _decide(H, cap, bit | OVF_BAD_ENTRY, per=quiet)[0] == BAD_ENTRY


def test_rerun_loop_converges_against_a_scripted_device(harness):
    """The loop both callers run, against a fake device that reports as the real one does -- one stage per run: lines, then hit lines, then records,
    then a fall-back bit -- until the capacities reach fixed needs: done within the eight runs the policy allows, every capacity at least its need and
    never smaller than before.  A device that never clears gets the non-convergence verdict on the eighth run, not earlier and not later."""
    H = harness
    # (needs, one walk for four patterns?, first capacities, runs: a one-walk scan's lines / 2 + 64 hit lines cover the second stage)
    for needs, per_walk, first, want_runs in (((200000, 90000, 3000000), False, (10, 2, 1), 5), ((200000, 90000, 3000000), True, (10, 2, 1), 4),
                                              ((29000, 600000, 700000), False, (29336, 524288, 524288), 4), ((5, 1, 1), False, (10, 2, 1), 2)):
        cap, noted, runs, fb = first, 0, 0, OVF_SEAM if per_walk else OVF_LONG_LINES
        quiet = [[0, 0, 0]] * 4
        while True:
            assert runs < MAX_RUNS
            # the fake device: the first stage that does not fit; a one-walk scan reports hit lines and records per pattern (a quarter each)
            ovf, need, per = 0, (0, 0, 0), quiet if per_walk else None
            if cap[0] < needs[0]:
                ovf, need = OVF_LINES, (needs[0], 0, 0)
            elif cap[1] < needs[1]:
                if per_walk:
                    per = [[OVF_HITLINES, needs[1] // 4, 0]] + quiet[1:]
                else:
                    ovf, need = OVF_HITLINES, (0, needs[1], 0)
            elif cap[2] < needs[2]:
                if per_walk:
                    per = quiet[:3] + [[OVF_RECORDS, 0, needs[2] // 4]]
                else:
                    ovf, need = OVF_RECORDS, (0, 0, needs[2])
            elif not noted & fb:
                ovf = fb
            verdict, nxt, note = _decide(H, cap, ovf, need, per=per, run=runs)
            runs += 1
            noted |= note
            if verdict == DONE:
                break
            assert verdict == AGAIN, (needs, runs, verdict)
            assert all(n >= c for n, c in zip(nxt, cap)), (cap, nxt)
            cap = nxt
        assert all(c >= n for c, n in zip(cap, needs)) and noted == fb, (cap, needs, noted)
        assert runs == want_runs, (needs, runs)
    # eight stages, none of which clears: whatever was asked for, the next run needs more
    stages = (OVF_LINES, OVF_HITLINES, OVF_RECORDS, OVF_NO_STREAM, OVF_NONDNA, OVF_LONG_LINES, OVF_SEAM, OVF_LEADER | OVF_RECORDS)
    for per in (None, [[OVF_HITLINES | OVF_RECORDS, 10**6, 10**7]] * 4):
        cap, verdicts = (10, 2, 1), []
        for run, ovf in enumerate(stages):
            if per:
                ovf &= ~(OVF_NO_STREAM | OVF_NONDNA | OVF_LONG_LINES)
            verdict, nxt, _ = _decide(H, cap, ovf, (2 * cap[0], 2 * cap[1], 2 * cap[2]), per=per, run=run)
            verdicts.append(verdict)
            assert all(n >= c for n, c in zip(nxt, cap))
            cap = nxt
        assert verdicts == [AGAIN] * 7 + [NO_CONVERGENCE]
    assert _decide(H, (10, 2, 1), 0, run=7) == (DONE, (10, 2, 1), 0)                             # the result of the eighth run counts


def test_fallback_flags_age_out_after_32_scans(harness):
    """A noted flag holds for the 31 scans that follow and is gone on the 32nd; noting again restarts the count; without a flag nothing is counted."""
    H = harness
    st = _fallback(H, [OVF_SEAM] + [0] * 40)
    assert [s["no_window"] for s in st] == [1] * 32 + [0] * 9
    assert [s["ttl"] for s in st[:33]] == list(range(32, -1, -1)) and all(s["ttl"] == 0 and s["bits"] == 0 for s in st[32:])
    st = _fallback(H, [OVF_SEAM] + [0] * 10 + [OVF_LEADER] + [0] * 32)
    assert st[10]["ttl"] == 22 and st[11] == dict(bits=OVF_SEAM | OVF_LEADER, ttl=32, no_stream=0, no_stream_nd=0, force_ll=0, no_window=1, no_leaders=1)
    assert all(s["bits"] == OVF_SEAM | OVF_LEADER for s in st[11:43]) and st[42]["ttl"] == 1
    assert st[43]["bits"] == 0                                                                   # both flags go together
    st = _fallback(H, [OVF_LINES, 0, 0, OVF_LONG_LINES, 0])                                       # a workspace bit is no flag and restarts nothing
    assert [(s["bits"], s["ttl"]) for s in st] == [(0, 0), (0, 0), (0, 0), (OVF_LONG_LINES, 32), (OVF_LONG_LINES, 31)]


def test_first_reservation_of_ascii_and_packed_scans(harness):
    """What a scan reserves before its first run: seg / 32 + 1024 lines, one hit line in hl_div (+ 1024), at least 8192 * 64 hit lines for the
    one-pass kernels, records at least hit lines; a packed batch: one read in eight (+ 1024).  Never less than the context has, and exactly what it
    has where the caller sized the workspace."""
    import ctypes as C
    H = harness
    H.harness_first_reservation.restype = None
    H.harness_first_reservation.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]

    def first(seg, hl_div=8, cap=(0, 0, 0), packed=0, single=0, user=0):
        c, out = np.array(cap, dtype=np.uint64), np.zeros(3, dtype=np.uint64)
        H.harness_first_reservation(packed, seg, single, hl_div, c.ctypes.data, user, out.ctypes.data)
        return tuple(int(v) for v in out)
    reads = 6000 * 151                                                       # 906 000 bytes: 28 312 + 1024 lines, 3667 + 1024 hit lines -> the floor
    assert first(reads) == (29336, 524288, 524288)
    assert first(reads, hl_div=2) == (29336, 524288, 524288)                 # 14 668 + 1024: the floor still
    seg = 0xF0000000                                                         # a 3.75 GiB segment: 125 829 120 + 1024 lines
    assert first(seg) == (125830144, 15729792, 15729792)                     # 15 728 768 + 1024
    assert first(seg, hl_div=2) == (125830144, 62916096, 62916096)           # 62 915 072 + 1024
    assert first(seg, single=1) == (1, 1024, 1024)                           # SEEQDEV_SINGLELINE: one line, no floor
    assert first(seg, single=1, cap=(7, 5000, 3)) == (7, 5000, 5000)
    # a context that holds more keeps it; records follow the hit lines up
    assert first(reads, cap=(50000, 10, 10)) == (50000, 524288, 524288)      # 6250 + 1024 from the lines it has
    assert first(seg, cap=(10, 20000000, 30000000)) == (125830144, 20000000, 30000000)
    assert first(6000, packed=1) == (0, 1774, 1774)                          # 750 + 1024
    assert first(1 << 26, packed=1) == (0, 8389632, 8389632)                 # the largest packed segment: 2^23 + 1024
    assert first(6000, packed=1, cap=(10, 2, 1)) == (10, 1774, 1774)
    assert first(6000, packed=1, cap=(10, 5000, 9000)) == (10, 5000, 9000)
    for cap in ((10, 2, 1), (0, 0, 0), (125830144, 7, 3)):
        for kw in (dict(), dict(hl_div=2), dict(single=1), dict(packed=1)):
            assert first(reads, cap=cap, user=1, **kw) == cap, (cap, kw)
