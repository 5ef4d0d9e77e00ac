"""Counting the distinct inserts of 10 M resident reads: the device route (seeqdevScanRunInserts + seeqdevScanTally: inserts_tensor, tally)
against the route a caller had before the tally -- inserts_tensor, insert_text, the insert text copied to the host, np.unique with counts
over its lines.
Usage (GPU box): python3 profiles/tally_bench.py [--lines N] [--distinct M] [--runs K]
  -> one JSON line, appended to profiles/tally_bench.jsonl.
Input: profiles/inserts_bench.py's own (its generator): N x 150 bp lines (M distinct lines tiled on the device), about 90 % of them with
both 20-mer flanks around a 12-base insert; SQ_BEST, window min_len 8, max_len 16.  The device route is timed with profiling on, so the
tally's own HIP-event time (last_tally_ms) is recorded beside the wall times of the tally alone, of the inserts call alone and of the two
together (table copied to the host).  Best of K timed runs (after one untimed run); the host route runs once.  Both routes must give the
same table: the host's distinct lines are keyed by the rule of seeq_tally.h in NumPy and ordered by key."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from seeq_amd import device as dev
from inserts_bench import LEFT, RIGHT, TAU, L, MIN_LEN, MAX_LEN, best_of, make_lines


def host_route(sc, left, right, t):
    """What a caller did before the tally: the insert text gathered on the device, copied, counted on the host."""
    sc.inserts_tensor(left, right, t, dev.SQ_BEST, MIN_LEN, MAX_LEN, copy=False)
    text = sc.insert_text(t).cpu().numpy()
    lines = np.array(text.tobytes().split(b"\n")[:-1])
    return np.unique(lines, return_counts=True)


def keyed(lines, counts):
    """Distinct lines (a NumPy bytes array) and their counts -> the tally's table by the rule: keys ascending, their counts; the lines
    that are long or foreign are left out and counted."""
    width = lines.dtype.itemsize
    a = np.frombuffer(lines.tobytes(), dtype=np.uint8).reshape(len(lines), width) if len(lines) else np.zeros((0, 1), dtype=np.uint8)
    length = (a != 0).sum(axis=1)
    up = a & 0xDF
    base = (up == 65) | (up == 67) | (up == 71) | (up == 84) | (up == 85)
    ok = (length <= 31) & ((base | (a == 0)).all(axis=1))
    key = np.ones(len(lines), dtype=np.uint64)
    for j in range(min(width, 31)):
        live = j < length
        key = np.where(live, (key << np.uint64(2)) | ((a[:, j] >> 1) & 3).astype(np.uint64), key)
    order = np.argsort(key[ok], kind="stable")
    k, c = key[ok][order], counts[ok][order].astype(np.uint64)
    first = np.concatenate(([True], k[1:] != k[:-1])) if len(k) else np.zeros(0, dtype=bool)      # lines that differ in case share a key
    return k[first], np.add.reduceat(c, np.nonzero(first)[0]) if len(k) else c, int(counts[~ok & (length > 31)].sum()), int(counts[~ok & (length <= 31)].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--distinct", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "tally_bench.jsonl"))
    args = ap.parse_args()
    distinct = min(args.distinct, args.lines)
    torch.cuda.set_device(0)
    t = torch.from_numpy(make_lines(distinct, 29)).cuda().repeat(max(1, args.lines // distinct))
    nlines = t.numel() // (L + 1)
    left, right = dev.Pattern(LEFT, TAU), dev.Pattern(RIGHT, TAU)
    sc = dev.Scanner()
    sc.set_profiling(True)
    state = {}

    def device_route():
        state["ins"] = sc.inserts_tensor(left, right, t, dev.SQ_BEST, MIN_LEN, MAX_LEN, copy=False)
        return sc.tally(t)
    t_dev, res = best_of(device_route, args.runs)
    tally_event_ms = sc.last_tally_ms()
    t_tally, lazy = best_of(lambda: sc.tally(t, copy=False), args.runs)
    t_copy, _ = best_of(lambda: sc.tally_table(lazy["ndistinct"]), args.runs)
    t_ins, _ = best_of(lambda: sc.inserts_tensor(left, right, t, dev.SQ_BEST, MIN_LEN, MAX_LEN, copy=False), args.runs)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    lines, counts = host_route(sc, left, right, t)
    t_host = time.perf_counter() - t0
    hk, hc, hlong, hforeign = keyed(lines, counts)
    same = (np.array_equal(hk, res["keys"]) and np.array_equal(hc, res["counts"]) and (hlong, hforeign) == (res["nlong"], res["nforeign"])
            and int(counts.sum()) == res["nspans"] == state["ins"]["ninserts"])
    assert same, "the two routes differ"
    row = {"lines": nlines, "read_len": L, "text_bytes_scanned": t.numel(), "window": [MIN_LEN, MAX_LEN],
           "counts": {k: res[k] for k in ("nspans", "ntallied", "nlong", "nforeign", "ndistinct", "max_len", "passes")},
           "tally_event_ms": round(tally_event_ms, 3), "tally_wall_ms": round(t_tally * 1e3, 3), "table_copy_ms": round(t_copy * 1e3, 3),
           "inserts_ms": round(t_ins * 1e3, 3), "device_route_ms": round(t_dev * 1e3, 3), "host_route_ms": round(t_host * 1e3, 3),
           "host_over_device": round(t_host / t_dev, 1), "identical": same}
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    sc.close()


if __name__ == "__main__":
    main()
