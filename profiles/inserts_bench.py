"""The insert between two flanks over 10 M resident reads: the device route (seeqdevScanRunInserts + seeqdevScanInsertText:
inserts_tensor, insert_text) against the route a caller had before it -- two scan_tensor calls with records, both record and offset
arrays copied to the host, the join by the same rule in NumPy, the inserts cut from a host copy of the text.
Usage (GPU box): python3 profiles/inserts_bench.py [--lines N] [--distinct M] [--best] [--first] [--runs K]
  -> one JSON line per mode, appended to profiles/inserts_bench.jsonl.
Input: N x 150 bp lines (M distinct lines tiled on the device), about 90 % of them with both 20-mer flanks (0 - 3 substitutions each) at
distance 3 around a 12-base insert; window min_len 8, max_len 16.  The device route is timed with profiling on, so the join's own
HIP-event time is recorded; the gather (insert_text) and one plain scan of the same context are timed beside it.  Best of K timed runs
(after one untimed run); the host route runs twice, the second is timed.  Both routes must give the same records and the same text."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from seeq_amd import device as dev

LEFT, RIGHT, TAU, L, INSERT = "GATGTAGCGCGATTAGCCTG", "TTCACTGGAGTTGTCCCAAT", 3, 150, 12
MIN_LEN, MAX_LEN = 8, 16


def make_lines(m, seed):
    """m lines of L bases + newline as one uint8 array."""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(m, L + 1))]
    a[:, L] = 10
    planted = np.nonzero(rng.random(m) < 0.9)[0]
    col = rng.integers(5, L - 2 * 20 - INSERT - 5, size=planted.size)
    for flank, shift in ((LEFT, 0), (RIGHT, 20 + INSERT)):
        f = np.frombuffer(flank.encode(), dtype=np.uint8)
        for i in range(20):
            a[planted, col + shift + i] = f[i]
        for _ in range(3):                                  # up to three substitutions per flank (a draw may repeat a position or the base)
            hit = rng.random(planted.size) < 0.3
            a[planted[hit], col[hit] + shift + rng.integers(0, 20, size=int(hit.sum()))] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(hit.sum()))]
    return a.reshape(-1)


def best_of(fn, runs):
    out, best = None, None
    for it in range(runs + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if it and (best is None or dt < best): best = dt
    return best, out


def host_route(sc, left, right, t, host, mode):
    """What a caller did before the device join: two scans for records, four arrays to the host, the rule in NumPy, the cut on the host."""
    cr = sc.scan_tensor(right, t, dev.SQ_ALL, dev.WANT_RECORDS)
    rr, ro = sc.records(cr["nrecords"]), sc.record_offsets(cr["nrecords"])
    cl = sc.scan_tensor(left, t, mode, dev.WANT_RECORDS)
    lr, lo = sc.records(cl["nrecords"]), sc.record_offsets(cl["nrecords"])
    del ro
    lend = np.full(cl["nlines"] + 1, -1, dtype=np.int64)    # per line the left record's end, its distance, its index
    lidx = np.zeros(cl["nlines"] + 1, dtype=np.int64)
    lend[lr[:, 0]] = lr[:, 2]
    lidx[lr[:, 0]] = np.arange(len(lr))
    e = lend[rr[:, 0]]
    start = rr[:, 1].astype(np.int64)
    adm = np.nonzero((e >= 0) & (start >= e + MIN_LEN) & ((MAX_LEN == 0) | (start <= e + MAX_LEN)))[0]
    if mode == dev.SQ_BEST:                                 # smallest dist, the smaller end on a tie; the records are in (line, end) order
        adm = adm[np.lexsort((rr[adm, 2], rr[adm, 3], rr[adm, 0]))]
    lines, first = np.unique(rr[adm, 0], return_index=True)
    chosen = rr[adm[first]]
    li = lidx[lines]
    rec = np.zeros(len(lines), dtype=dev.INSERT_DTYPE)
    rec["line"], rec["start"], rec["end"], rec["ldist"], rec["rdist"] = lines, lr[li, 2], chosen[:, 1], lr[li, 3], chosen[:, 3]
    off = lo[li]
    lens = (rec["end"] - rec["start"]).astype(np.int64) + 1
    pos = np.cumsum(lens) - lens
    total = int(lens.sum())
    idx = np.arange(total, dtype=np.int64) - np.repeat(pos, lens) + np.repeat(off.astype(np.int64) + rec["start"], lens)
    idx[pos + lens - 1] = 0
    text = host[idx]
    text[pos + lens - 1] = 10
    return rec, off, text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--distinct", type=int, default=1_000_000)
    ap.add_argument("--best", action="store_true")
    ap.add_argument("--first", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "inserts_bench.jsonl"))
    args = ap.parse_args()
    modes = [m for m, on in (("best", args.best), ("first", args.first)) if on] or ["best", "first"]
    distinct = min(args.distinct, args.lines)
    torch.cuda.set_device(0)
    one = make_lines(distinct, 29)
    t = torch.from_numpy(one).cuda().repeat(max(1, args.lines // distinct))
    host = t.cpu().numpy()
    nlines = t.numel() // (L + 1)
    left, right = dev.Pattern(LEFT, TAU), dev.Pattern(RIGHT, TAU)
    sc = dev.Scanner()
    sc.set_profiling(True)
    for name in modes:
        mode = dev.SQ_BEST if name == "best" else dev.SQ_FIRST
        state = {}

        def device_route():
            state["res"] = sc.inserts_tensor(left, right, t, mode, MIN_LEN, MAX_LEN, copy=False)
            state["join_ms"] = sc.last_inserts_join_ms()
            return sc.insert_text(t)
        t_dev, text = best_of(device_route, args.runs)
        res = state["res"]
        t_gather, _ = best_of(lambda: sc.insert_text(t), args.runs)
        rec, off = sc.insert_records(res["ninserts"]), sc.insert_offsets(res["ninserts"])
        t_plain, cnt = best_of(lambda: sc.scan_tensor(left, t, mode, dev.WANT_RECORDS), args.runs)
        plain_dev_ms = sc.last_times_ms()["total"]
        t_host, (hrec, hoff, htext) = best_of(lambda: host_route(sc, left, right, t, host, mode), 1)
        same = rec.tobytes() == hrec.tobytes() and off.tobytes() == hoff.tobytes() and text.cpu().numpy().tobytes() == htext.tobytes()
        assert same, "the two routes differ"
        row = {"mode": name, "lines": nlines, "read_len": L, "text_bytes_scanned": t.numel(), "window": [MIN_LEN, MAX_LEN],
               "counts": {k: res[k] for k in ("nleft", "nright", "nboth", "ninserts", "text_bytes")},
               "device_route_ms": round(t_dev * 1e3, 3), "join_event_ms": round(state["join_ms"], 3), "gather_ms": round(t_gather * 1e3, 3),
               "plain_scan_wall_ms": round(t_plain * 1e3, 3), "plain_scan_event_ms": round(plain_dev_ms, 3), "plain_scan_records": cnt["nrecords"],
               "host_route_ms": round(t_host * 1e3, 3), "host_over_device": round(t_host / t_dev, 1), "identical": same}
        print(json.dumps(row), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")
    sc.close()


if __name__ == "__main__":
    main()
