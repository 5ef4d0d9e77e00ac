"""Counting the guides of 10 M resident reads against their KNOWN library within ONE EDIT (a substitution, a base lost, a base gained):
the library tally under the edit mode (set_library(..., indels=True)) beside the substitution mode of the same run, and against the
route a caller had before -- the plain tally, its table to the host, an exact look-up of the library's keys and a NumPy walk of the
substitution, deletion and insertion neighbours of every distinct key that is no entry.
Usage (GPU box): python3 profiles/tally_library_edit_bench.py [--lines N] [--distinct M] [--guides G] [--runs K] [--reps R] [--no-host]
  -> one JSON line, appended to profiles/tally_library_edit_bench.jsonl.
Input: tally_library_bench.py's (N x 150 bp lines, M distinct lines tiled on the device, about 90 % of them with flank A + a guide (one of
G, 20 bases) + flank B ...), with ONE EDIT planted in about 10 % of the guides, a third each a substitution, an insertion and a deletion
(the line keeps its length: what lies behind the guide moves by one base); the inserts window is the guide's length widened by one on
either side.  The scanner profiles, so the tallies' own HIP-event times (last_tally_ms) are recorded: R repetitions of best-of-K for
either mode, alternating.  The host route runs once; both routes must give the same dense count vector and the same split of the
corrected spans.  --no-host leaves the host route out (for a run under a profiler)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from seeq_amd import device as dev
from inserts_bench import L, best_of
from tally_grouped_bench import ACGT, FA, FB, FC, FD, GUIDE, SPACER, UMI, keys_of


def make_lines(m, nguides, seed, error_rate=0.1):
    """m lines of L bases + newline as one uint8 array, and the library (nguides x GUIDE bases)."""
    rng = np.random.default_rng(seed)
    a = ACGT[rng.integers(0, 4, size=(m, L + 1))]
    a[:, L] = 10
    planted = np.nonzero(rng.random(m) < 0.9)[0]
    span = 4 * 20 + GUIDE + UMI + SPACER
    col = rng.integers(3, L - span - 4, size=planted.size)
    code = rng.integers(0, 4, size=(nguides, GUIDE))
    which = rng.integers(0, nguides, size=planted.size)
    r = rng.random(planted.size)
    kind = np.where(r < error_rate / 3, 1, np.where(r < 2 * error_rate / 3, 2, np.where(r < error_rate, 3, 0)))      # 1 substitution, 2 insertion, 3 deletion
    at = rng.integers(0, GUIDE, size=planted.size)
    base = rng.integers(0, 4, size=planted.size)
    for k, glen in ((0, GUIDE), (1, GUIDE), (2, GUIDE + 1), (3, GUIDE - 1)):
        rows = np.nonzero(kind == k)[0]
        g = code[which[rows]]
        if k == 1:
            g[np.arange(rows.size), at[rows]] = (g[np.arange(rows.size), at[rows]] + 1 + base[rows] % 3) % 4
        elif k == 2:                                        # a base in front of position at
            j = np.arange(GUIDE + 1)[None, :]
            g = np.where(j < at[rows, None], g[:, np.minimum(np.arange(GUIDE + 1), GUIDE - 1)], np.where(j == at[rows, None], base[rows, None], g[:, np.maximum(np.arange(GUIDE + 1) - 1, 0)]))
        elif k == 3:                                        # the base at position at removed
            j = np.arange(GUIDE - 1)[None, :]
            g = np.where(j < at[rows, None], g[:, :GUIDE - 1], g[:, 1:])
        assert g.shape == (rows.size, glen)
        off = 0
        for part in (FA, ACGT[g], FB, None, FC, None, FD):
            if part is None:
                off += SPACER if off == 2 * 20 + glen else UMI
                continue
            block = np.frombuffer(part.encode(), dtype=np.uint8)[None, :] if isinstance(part, str) else part
            for i in range(block.shape[1]):
                a[planted[rows], col[rows] + off + i] = block[:, i]
            off += block.shape[1]
        assert off == span + glen - GUIDE
    return a.reshape(-1), ACGT[code], {k: int((kind == k).sum()) for k in (1, 2, 3)}


def host_route(sc, t, lib_keys):
    """What a caller did before: the plain tally, its table to the host, the library's keys looked up exactly, and for every distinct key
    that is no entry its neighbours of the three classes looked up in NumPy -> the dense count vector, the split, the tally's result."""
    res = sc.tally(t)
    return host_assign(res["keys"], res["counts"], lib_keys) + (res,)


def host_assign(keys, counts, lib_keys):
    """The distinct keys of a plain tally and their counts -> (the dense count vector of the library, the split of the corrected)."""
    order = np.argsort(lib_keys)
    skey = lib_keys[order]
    u = np.uint64

    def find(q):                                            # -> index into the library, -1: no entry
        at = np.minimum(np.searchsorted(skey, q), len(skey) - 1)
        return np.where(skey[at] == q, order[at], -1)
    dense = np.zeros(len(lib_keys), dtype=np.uint64)
    exact = find(keys)
    np.add.at(dense, exact[exact >= 0], counts[exact >= 0])
    rest, rcount = keys[exact < 0], counts[exact < 0]
    length = (np.floor(np.log2(rest.astype(np.float64))).astype(np.int64)) // 2
    nfound = np.zeros(len(rest), dtype=np.int64)
    which = np.zeros(len(rest), dtype=np.int64)
    by = np.zeros(len(rest), dtype=np.int64)

    def take(hit, ok, cls):
        nonlocal nfound, which, by
        hit = np.where(ok, hit, -1)
        nfound += hit >= 0
        which = np.where(hit >= 0, hit, which)
        by = np.where(hit >= 0, cls, by)
    top = int(length.max()) if len(rest) else 0
    for p in range(top + 1):
        low = (u(2) * (length - 1 - p).clip(0).astype(u))               # bits of the bases behind p
        lowi = (u(2) * (length - p).clip(0).astype(u))                   # bits of the bases from p on
        here = (rest >> low) & u(3)
        prev = (rest >> lowi) & u(3) if p else np.full(len(rest), 4, dtype=u)      # the base in front of p; 4: none
        inside = length > p
        for s in (1, 2, 3):
            take(find(rest ^ (u(s) << low)), inside, 0)
        take(find(((rest >> (low + u(2))) << low) | (rest & ((u(1) << low) - u(1)))), inside & (here != prev), 2)
        for c in range(4):
            take(find(((((rest >> lowi) << u(2)) | u(c)) << lowi) | (rest & ((u(1) << lowi) - u(1)))), (length >= p) & (length <= 30) & (u(c) != prev), 1)
    one = nfound == 1
    np.add.at(dense, which[one], rcount[one])
    split = dict(nsubstituted=int(rcount[one & (by == 0)].sum()), ninserted=int(rcount[one & (by == 1)].sum()), ndeleted=int(rcount[one & (by == 2)].sum()))
    return dense, split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--distinct", type=int, default=1_000_000)
    ap.add_argument("--guides", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "tally_library_edit_bench.jsonl"))
    args = ap.parse_args()
    distinct = min(args.distinct, args.lines)
    torch.cuda.set_device(0)
    lines, library, planted = make_lines(distinct, args.guides, 31)
    t = torch.from_numpy(lines).cuda().repeat(max(1, args.lines // distinct))
    nlines = t.numel() // (L + 1)
    lib_keys = keys_of(library)
    assert len(np.unique(lib_keys)) == len(lib_keys), "the random library holds a duplicate: another seed"
    pats = [dev.Pattern(f, 0) for f in (FA, FB)]
    sc = dev.Scanner()
    sc.set_profiling(True)
    ins = sc.inserts_tensor(pats[0], pats[1], t, dev.SQ_BEST, min_len=GUIDE - 1, max_len=GUIDE + 1, copy=False)
    edit_ms, subst_ms = [], []
    for _ in range(args.reps):                              # the two modes alternate: the box is shared
        sc.set_library(lib_keys, 1, indels=True)
        _, lazy = best_of(lambda: sc.tally_library(t, copy=False), args.runs)
        edit_ms.append(round(sc.last_tally_ms(), 3))
        edits = sc.library_edits()
        sc.set_library(lib_keys, 1)
        _, lazy1 = best_of(lambda: sc.tally_library(t, copy=False), args.runs)
        subst_ms.append(round(sc.last_tally_ms(), 3))
    sc.set_library(lib_keys, 1, indels=True)
    t_dev, res = best_of(lambda: sc.tally_library(t), args.runs)
    edits = sc.library_edits()
    dense = dev.library_counts(res, len(lib_keys))
    assert int(dense.sum()) == res["nassigned"] and sum(edits.values()) == res["ncorrected"] and ins["ninserts"] == res["nspans"]
    names = ("nspans", "nassigned", "nexact", "ncorrected", "nambiguous", "nunknown", "nlong", "nforeign", "ndistinct", "key_bits", "passes")
    row = {"lines": nlines, "read_len": L, "text_bytes_scanned": t.numel(), "guides": args.guides, "planted_per_distinct_line": planted,
           "counts": {k: res[k] for k in names}, "edits": edits, "substitution_mode_corrected": lazy1["ncorrected"],
           "edit_mode_event_ms": edit_ms, "substitution_mode_event_ms": subst_ms, "edit_mode_tally_and_table_wall_ms": round(t_dev * 1e3, 3)}
    if not args.no_host:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        host_dense, host_split, plain = host_route(sc, t, lib_keys)
        t_host = time.perf_counter() - t0
        same = bool(np.array_equal(dense, host_dense)) and host_split == edits and plain["nspans"] == res["nspans"]
        assert same, ("the two routes differ", host_split, edits, int(host_dense.sum()), int(dense.sum()))
        row.update(host_route_ms=round(t_host * 1e3, 3), host_over_device=round(t_host / t_dev, 1), plain_tally_distinct=plain["ndistinct"], identical=same)
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    sc.close()


if __name__ == "__main__":
    main()
