"""Counting the reads per (cell, guide) of 10 M resident reads with no UMI at all: the device route (a hold of the cells, an append of the
guides' library ids, tally_held(1) and held_matrix(4096, 2000)) against the route a caller had before the held tally -- held() to the host
(12 bytes per record), np.unique over the first-of-line keyed records, the rows by a second np.unique and a scatter into a NumPy matrix.
Usage (GPU box): python3 profiles/tally_held_bench.py [--lines N] [--distinct M] [--guides G] [--runs K]
  -> one JSON line, appended to profiles/tally_held_bench.jsonl.
Input: tally_append_bench.py's (the append row): N x 200 bp lines, about 90 % of them with a 16-base cell barcode (one
of 4 096), a 20-base guide (one of G; one read in twenty with one substitution) and a UMI between exact flanks.  Two holds are measured:
  raw   the cells held as they are read (33 bits) and the guide ids appended (11): the 44-bit word of the append row.  Its rows are raw
        sequence keys, so every entry lies OUTSIDE a 4 096 x 2 000 matrix: the dense call is timed as the memset plus a scatter that stores
        nothing, and the sparse tables are the result.
  ids   the cells assigned to their whitelist (the distinct cells seen, exact: 13 bits) and the guide ids appended: a 24-bit word, and the
        matrix a screen wants.
Both are timed with profiling on: the held tally's and the dense call's own HIP-event times (last_tally_held_ms) beside their wall times,
and the grouped call of the same run (the UMIs as members, last_tally_grouped_ms) beside them.  Best of K timed runs (after one untimed
run); the host route runs once.  Both routes must give the same table, rows and matrix."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from seeq_amd import device as dev
from inserts_bench import best_of
from tally_append_bench import FE, FF, L, NCELLS, make_lines
from tally_grouped_bench import FA, FB, FC, FD, keys_of


def host_route(sc, shift, nrows, ncols):
    """held() to the host, the first keyed record of every line, np.unique, the rows, the matrix."""
    h = sc.held()
    lines, keys = h["lines"], h["keys"]
    opens = np.ones(len(lines), dtype=bool)
    opens[1:] = lines[1:] != lines[:-1]
    uniq, counts = np.unique(keys[opens & (keys != 0)], return_counts=True)
    r, c = uniq >> np.uint64(shift), uniq & np.uint64((1 << shift) - 1)
    groups, first, ndistinct = np.unique(r, return_index=True, return_counts=True)
    reads = np.add.reduceat(counts, first) if len(first) else np.zeros(0, dtype=np.int64)
    inside = (r >= 1) & (r <= nrows) & (c >= 1) & (c <= ncols)
    matrix = np.zeros((nrows, ncols), dtype=np.int64)
    matrix[(r[inside] - 1).astype(np.int64), (c[inside] - 1).astype(np.int64)] = counts[inside]
    return uniq, counts, (groups, reads, first, ndistinct), matrix


def measure(sc, t, pats, nrows, ncols, runs):
    """The held column is built: tally_held(1), held_matrix, the host route, the grouped call of the same run -> the row's part."""
    widths = sc.hold_columns()
    t_held, _ = best_of(lambda: sc.tally_held(1, copy=False), runs)
    held_event_ms = sc.last_tally_held_ms()
    res = sc.tally_held(1)
    out = torch.empty((nrows, ncols), dtype=torch.int64, device="cuda")
    t_dense, (_, dense) = best_of(lambda: sc.held_matrix(nrows, ncols, out=out), runs)
    dense_event_ms = sc.last_tally_held_ms()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    uniq, counts, (groups, reads, first, ndistinct), matrix = host_route(sc, res["shift"], nrows, ncols)
    t_host = time.perf_counter() - t0
    same = (np.array_equal(uniq, res["table"]["key"]) and np.array_equal(counts.astype(np.uint64), res["table"]["count"])
            and np.array_equal(groups, res["rows"]["group"]) and np.array_equal(reads.astype(np.uint64), res["rows"]["count"])
            and np.array_equal(first.astype(np.uint32), res["rows"]["first"]) and np.array_equal(ndistinct.astype(np.uint32), res["rows"]["ndistinct"])
            and np.array_equal(matrix, out.cpu().numpy()))
    assert same, "the two routes differ"
    sc.inserts_tensor(pats[2], pats[3], t, dev.SQ_BEST, copy=False)
    grouped = sc.tally_grouped(t, copy=False)
    return {"widths": widths, "counts": {k: res[k] for k in ("nrecords", "ncounted", "nkeyless", "nrepeat", "ndistinct", "nrows", "key_bits", "shift", "passes")},
            "dense": dense, "held_event_ms": round(held_event_ms, 3), "held_wall_ms": round(t_held * 1e3, 3), "dense_event_ms": round(dense_event_ms, 3),
            "dense_wall_ms": round(t_dense * 1e3, 3), "host_route_ms": round(t_host * 1e3, 3), "host_over_device": round(t_host / (t_held + t_dense), 1),
            "grouped_event_ms": round(sc.last_tally_grouped_ms(), 3), "grouped_passes": grouped["passes"], "identical": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--distinct", type=int, default=1_000_000)
    ap.add_argument("--guides", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "tally_held_bench.jsonl"))
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
    row = {"lines": nlines, "read_len": L, "text_bytes_scanned": t.numel(), "guides": int(len(library)), "matrix": [NCELLS, args.guides]}
    # raw: the cells as they are read, the guides' ids behind them
    sc.set_library(lib_keys, max_mismatch=1)
    sc.inserts_tensor(pats[4], pats[5], t, dev.SQ_BEST, copy=False)
    sc.tally_hold(t)
    whitelist = sc.tally(t)["keys"]                         # the distinct cells seen, ascending: the ids of the second hold
    sc.inserts_tensor(pats[0], pats[1], t, dev.SQ_BEST, copy=False)
    sc.tally_hold_append(t, library=True)
    row["raw"] = measure(sc, t, pats, NCELLS, args.guides, args.runs)
    # ids: the cells assigned to their whitelist
    assert len(whitelist) <= NCELLS
    sc.set_library(whitelist, max_mismatch=0)
    sc.inserts_tensor(pats[4], pats[5], t, dev.SQ_BEST, copy=False)
    sc.tally_hold_library(t)
    sc.set_library(lib_keys, max_mismatch=1)
    sc.inserts_tensor(pats[0], pats[1], t, dev.SQ_BEST, copy=False)
    sc.tally_hold_append(t, library=True)
    row["ids"] = measure(sc, t, pats, NCELLS, args.guides, args.runs)
    assert row["ids"]["dense"]["noutside"] == 0 and row["raw"]["dense"]["ninside"] == 0
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    sc.close()


if __name__ == "__main__":
    main()
