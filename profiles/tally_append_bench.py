"""Counting the UMIs per (cell, guide) of 10 M resident reads: the device route (inserts_tensor + tally_hold of the cell barcodes,
inserts_tensor + tally_hold_append(library=True) of the guides, inserts_tensor + tally_grouped of the UMIs, tally_collapse) against the
route a caller had before the appended columns -- three inserts_tensor calls with their records, the three insert texts copied to the
host, the guides assigned to the library, the join by line and np.unique over the (cell, guide id, UMI) rows in NumPy.
Usage (GPU box): python3 profiles/tally_append_bench.py [--lines N] [--distinct M] [--guides G] [--runs K]
  -> one JSON line, appended to profiles/tally_append_bench.jsonl.
Input: N x 200 bp lines (M distinct lines tiled on the device), about 90 % of them with flank E + a 16-base cell barcode (one of 4 096) +
flank F, three bases, flank A + a 20-base guide (one of G; one read in twenty with one substitution) + flank B, three bases, flank C + a
12-base UMI + flank D; the six 20-mer flanks are planted exactly and searched at distance 0 under SQ_BEST.  The device route is timed with
profiling on, so the grouped call's own HIP-event time (last_tally_grouped_ms) -- the number the append is to be compared with -- is
recorded beside the wall times of the append alone, of the hold alone and of the whole route.  Best of K timed runs (after one untimed
run); the host route runs once.  Both routes must give the same pair table after hold_split."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from seeq_amd import device as dev
from inserts_bench import best_of
from tally_grouped_bench import ACGT, FA, FB, FC, FD, keys_of

FE, FF = "TGCAAGGTCATCGGATACCT", "GTTACGACCTAGGCATTCGA"
L, CELL, GUIDE, UMI, SPACER, NCELLS = 200, 16, 20, 12, 3, 4096


def make_lines(m, nguides, seed):
    """m lines of L bases + newline as one uint8 array, and the guide library (rows of bases)."""
    rng = np.random.default_rng(seed)
    a = ACGT[rng.integers(0, 4, size=(m, L + 1))]
    a[:, L] = 10
    planted = np.nonzero(rng.random(m) < 0.9)[0]
    span = 6 * 20 + CELL + GUIDE + UMI + 2 * SPACER
    col = rng.integers(3, L - span - 3, size=planted.size)
    library = np.unique(ACGT[rng.integers(0, 4, size=(nguides, GUIDE))], axis=0)
    cells = ACGT[rng.integers(0, 4, size=(NCELLS, CELL))]
    guide = library[rng.integers(0, len(library), size=planted.size)].copy()
    hit = np.nonzero(rng.random(planted.size) < 0.05)[0]    # one substitution: the base three codes on (never the same base)
    at = rng.integers(0, GUIDE, size=hit.size)
    guide[hit, at] = ACGT[(np.searchsorted(ACGT, guide[hit, at]) + rng.integers(1, 4, size=hit.size)) % 4]
    cell = cells[rng.integers(0, NCELLS, size=planted.size)]
    at = 0
    for part in (FE, cell, FF, SPACER, FA, guide, FB, SPACER, FC, UMI, FD):
        if isinstance(part, int):                           # a spacer or the UMI: the random bases that are there
            at += part
            continue
        block = np.frombuffer(part.encode(), dtype=np.uint8)[None, :] if isinstance(part, str) else part
        for i in range(block.shape[1]):
            a[planted, col + at + i] = block[:, i]
        at += block.shape[1]
    assert at == span
    return a.reshape(-1), library


def assign(keys, lib_keys):
    """Tally keys of 20-mers -> library ids (entry i has id i + 1; 0: none) by the library's rule, exact or one substitution, in NumPy."""
    order = np.argsort(lib_keys)
    skey = lib_keys[order]

    def find(k):
        at = np.minimum(np.searchsorted(skey, k), len(skey) - 1)
        return np.where(skey[at] == k, order[at] + 1, 0).astype(np.uint64)
    uniq, inv = np.unique(keys, return_inverse=True)
    ids = find(uniq)
    miss = np.nonzero(ids == 0)[0]
    found, total = np.zeros(len(miss), dtype=np.int64), np.zeros(len(miss), dtype=np.uint64)
    for p in range(GUIDE):
        for s in (1, 2, 3):
            got = find(uniq[miss] ^ np.uint64(s << (2 * p)))
            found += got != 0
            total += got
    ids[miss] = np.where(found == 1, total, 0)
    return ids[inv]


def host_route(sc, pats, t, lib_keys):
    """Three inserts calls, their records and insert texts to the host, the library there, the join by line and np.unique."""
    cols = []
    for (left, right), width in zip(((4, 5), (0, 1), (2, 3)), (CELL, GUIDE, UMI)):
        r = sc.inserts_tensor(pats[left], pats[right], t, dev.SQ_BEST)
        text = sc.insert_text(t).cpu().numpy()
        assert text.size == r["ninserts"] * (width + 1), "this input's inserts have one length each"
        cols.append((r["records"]["line"], keys_of(text.reshape(-1, width + 1)[:, :width])))
    (cl, ck), (gl, gk), (ul, uk) = cols
    gid = assign(gk, lib_keys)
    _, ci, gi = np.intersect1d(cl, gl, assume_unique=True, return_indices=True)
    keep = gid[gi] != 0
    jl, jc, jg = cl[ci][keep], ck[ci][keep], gid[gi][keep]
    _, ji, ui = np.intersect1d(jl, ul, assume_unique=True, return_indices=True)
    rows = np.stack((jc[ji], jg[ji], uk[ui]), axis=1)
    uniq, counts = np.unique(rows, axis=0, return_counts=True)      # (ordered by cell, then id, then UMI: the pair table's order)
    return uniq, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--distinct", type=int, default=1_000_000)
    ap.add_argument("--guides", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "tally_append_bench.jsonl"))
    args = ap.parse_args()
    distinct = min(args.distinct, args.lines)
    torch.cuda.set_device(0)
    lines, library = make_lines(distinct, args.guides, 41)
    t = torch.from_numpy(lines).cuda().repeat(max(1, args.lines // distinct))
    nlines = t.numel() // (L + 1)
    lib_keys = keys_of(library)
    pats = [dev.Pattern(f, 0) for f in (FA, FB, FC, FD, FE, FF)]
    sc = dev.Scanner()
    sc.set_profiling(True)
    sc.set_library(lib_keys, max_mismatch=1)
    state = {}

    def device_route():
        sc.inserts_tensor(pats[4], pats[5], t, dev.SQ_BEST, copy=False)
        state["hold"] = sc.tally_hold(t)
        sc.inserts_tensor(pats[0], pats[1], t, dev.SQ_BEST, copy=False)
        state["append"] = sc.tally_hold_append(t, library=True)
        sc.inserts_tensor(pats[2], pats[3], t, dev.SQ_BEST, copy=False)
        res = sc.tally_grouped(t)
        state["collapse"] = sc.tally_collapse(copy=False)
        return res
    t_dev, res = best_of(device_route, args.runs)
    grouped_event_ms = sc.last_tally_grouped_ms()
    widths = sc.hold_columns()

    def append_alone():                                     # hold + append over records that are there: the append is the difference to the hold
        sc.inserts_tensor(pats[4], pats[5], t, dev.SQ_BEST, copy=False)
        sc.tally_hold(t)
        sc.inserts_tensor(pats[0], pats[1], t, dev.SQ_BEST, copy=False)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        sc.tally_hold_append(t, library=True)
        return time.perf_counter() - t0
    t_append = min(append_alone() for _ in range(args.runs))
    t_hold_lib, _ = best_of(lambda: sc.tally_hold_library(t), args.runs)      # the same column held: the append minus this is the join
    torch.cuda.synchronize(); t0 = time.perf_counter()
    rows, counts = host_route(sc, pats, t, lib_keys)
    t_host = time.perf_counter() - t0
    c0, c1 = dev.hold_split(res["pairs"]["group"], widths)
    same = (len(rows) == len(c0) and np.array_equal(rows[:, 0], c0) and np.array_equal(rows[:, 1], c1) and np.array_equal(rows[:, 2], res["pairs"]["member"])
            and np.array_equal(counts.astype(np.uint64), res["pairs"]["count"]))
    assert same, "the two routes differ"
    app = state["append"]
    row = {"lines": nlines, "read_len": L, "text_bytes_scanned": t.numel(), "guides": int(len(library)), "widths": widths,
           "hold": {k: state["hold"][k] for k in ("nspans", "nheld", "key_bits")},
           "append": {k: app[k] for k in ("nrecords", "nbefore", "nheld", "ndropped", "width", "key_bits", "ncolumns")},
           "column": {k: app["column"][k] for k in ("nspans", "nexact", "ncorrected", "nambiguous", "nunknown")},
           "counts": {k: res[k] for k in ("nspans", "npaired", "nungrouped", "npairs", "ngroups", "max_len", "passes")},
           "collapse": {k: state["collapse"][k] for k in ("nroots", "nabsorbed")},
           "append_wall_ms": round(t_append * 1e3, 3), "hold_library_wall_ms": round(t_hold_lib * 1e3, 3), "grouped_event_ms": round(grouped_event_ms, 3),
           "device_route_ms": round(t_dev * 1e3, 3), "host_route_ms": round(t_host * 1e3, 3), "host_over_device": round(t_host / t_dev, 1),
           "identical": bool(same)}
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    sc.close()


if __name__ == "__main__":
    main()
