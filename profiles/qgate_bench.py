"""Counting the distinct inserts of 10 M resident FASTQ records behind a base-quality bar: the device route (inserts_tensor +
quality_gate + tally(source="gated")) against the route a caller had before the gate -- the insert records, their offsets and the text
copied to the host, every record's quality line found and the bar applied in NumPy, np.unique over the spans that pass -- and beside
both the ungated tally of the same run.
Usage (GPU box): python3 profiles/qgate_bench.py [--lines N] [--distinct M] [--runs K]
  -> one JSON line, appended to profiles/qgate_bench.jsonl.
Input: profiles/tally_bench.py's own (inserts_bench.py's generator: N x 150 bp lines, M distinct ones tiled on the device, about 90 % with
both 20-mer flanks around a 12-base insert; SQ_BEST, window 8 .. 16), every line wrapped as a four-line record "@r", the line, "+", 150
quality bytes: 'I' with probability 0.97, else one of '#' .. '4' (below Q20).  The bar: min_qual 20, base 33, max_low 0, reach 1024.
The device route is timed with profiling on, so the gate's own HIP-event time (last_quality_gate_ms) stands beside the plain tally's
(last_tally_ms) of the same run.  Best of K timed runs (after one untimed run); the host route runs once.  Both routes must give the same
table."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from seeq_amd import device as dev
from inserts_bench import LEFT, RIGHT, TAU, L, MIN_LEN, MAX_LEN, best_of, make_lines
from tally_bench import keyed

MIN_QUAL, BASE, MAX_LOW, REACH = 20, 33, 0, 1024
REC = 3 + (L + 1) + 2 + (L + 1)                             # bytes of a record


def make_records(m, seed):
    """m four-line records around make_lines' lines, as one uint8 array."""
    rng = np.random.default_rng(seed + 1)
    a = np.empty((m, REC), dtype=np.uint8)
    a[:, 0:3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    a[:, 3:3 + L + 1] = make_lines(m, seed).reshape(m, L + 1)
    a[:, 3 + L + 1:3 + L + 3] = np.frombuffer(b"+\n", dtype=np.uint8)
    q = np.full((m, L), ord("I"), dtype=np.uint8)
    low = rng.random((m, L)) < 0.03
    q[low] = rng.integers(ord("#"), ord("5"), size=int(low.sum()))
    a[:, 3 + L + 3:REC - 1] = q
    a[:, REC - 1] = 10
    return a.reshape(-1)


def host_route(sc, left, right, t):
    """What a caller did before the gate: records, offsets and text to the host, the rule in NumPy, np.unique."""
    n = sc.inserts_tensor(left, right, t, dev.SQ_BEST | dev.SEEQDEV_FASTQ, MIN_LEN, MAX_LEN, copy=False)["ninserts"]
    rec, off, text = sc.insert_records(n), sc.insert_offsets(n).astype(np.int64), t.cpu().numpy()
    start, end = rec["start"].astype(np.int64), rec["end"].astype(np.int64)
    nl = np.flatnonzero(text == 10)
    at = np.searchsorted(nl, off + end)                     # the first newline at or behind the span's end, and the one behind it
    e1, e2 = nl[at], nl[at + 1]
    q0, seqlen = e2 + 1, e1 - off
    fits = (e2 - (off + end) < REACH) & (q0 + seqlen < len(text)) & (text[np.minimum(q0 + seqlen, len(text) - 1)] == 10) & (end - start <= 31)
    width = int((end - start).max())
    cols = np.arange(width)
    live = cols[None, :] < (end - start)[:, None]
    qual = text[np.minimum((q0 + start)[:, None] + cols[None, :], len(text) - 1)]
    nlow = ((qual < BASE + MIN_QUAL) & live).sum(axis=1)
    keep = fits & (nlow <= MAX_LOW)
    span = np.where(live, text[np.minimum((off + start)[:, None] + cols[None, :], len(text) - 1)], 0).astype(np.uint8)[keep]
    lines, counts = np.unique(np.ascontiguousarray(span).view("S%d" % width).reshape(-1), return_counts=True)
    return lines, counts, int(keep.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--distinct", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "qgate_bench.jsonl"))
    args = ap.parse_args()
    distinct = min(args.distinct, args.lines)
    torch.cuda.set_device(0)
    t = torch.from_numpy(make_records(distinct, 29)).cuda().repeat(max(1, args.lines // distinct))
    nrec = t.numel() // REC
    left, right = dev.Pattern(LEFT, TAU), dev.Pattern(RIGHT, TAU)
    sc = dev.Scanner()
    sc.set_profiling(True)
    opt = dev.SQ_BEST | dev.SEEQDEV_FASTQ
    gate = lambda: sc.quality_gate(t, "inserts", MIN_QUAL, BASE, MAX_LOW, REACH, copy=False)      # noqa: E731
    state = {}

    def device_route():
        state["ins"] = sc.inserts_tensor(left, right, t, opt, MIN_LEN, MAX_LEN, copy=False)
        state["gate"] = gate()
        return sc.tally(t, source="gated")
    t_dev, res = best_of(device_route, args.runs)
    gate_event_ms, gated_tally_event_ms = sc.last_quality_gate_ms(), sc.last_tally_ms()
    t_gate, _ = best_of(gate, args.runs)
    t_gated_tally, _ = best_of(lambda: sc.tally(t, source="gated", copy=False), args.runs)
    t_tally, plain = best_of(lambda: sc.tally(t, copy=False), args.runs)
    tally_event_ms = sc.last_tally_ms()
    t_ins, _ = best_of(lambda: sc.inserts_tensor(left, right, t, opt, MIN_LEN, MAX_LEN, copy=False), args.runs)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    lines, counts, kept = host_route(sc, left, right, t)
    t_host = time.perf_counter() - t0
    hk, hc, hlong, hforeign = keyed(lines, counts)
    same = (np.array_equal(hk, res["keys"]) and np.array_equal(hc, res["counts"]) and (hlong, hforeign) == (res["nlong"], res["nforeign"])
            and kept == res["nspans"] == state["gate"]["npassed"] and state["gate"]["nspans"] == state["ins"]["ninserts"] == plain["nspans"])
    assert same, "the two routes differ"
    row = {"records": nrec, "read_len": L, "text_bytes": t.numel(), "window": [MIN_LEN, MAX_LEN],
           "bar": {"min_qual": MIN_QUAL, "base": BASE, "max_low": MAX_LOW, "reach": REACH}, "gate": state["gate"],
           "gated_tally": {k: res[k] for k in ("nspans", "ntallied", "ndistinct", "max_len", "passes")}, "plain_tally_ndistinct": plain["ndistinct"],
           "gate_event_ms": round(gate_event_ms, 3), "gate_wall_ms": round(t_gate * 1e3, 3),
           "plain_tally_event_ms": round(tally_event_ms, 3), "plain_tally_wall_ms": round(t_tally * 1e3, 3),
           "gated_tally_event_ms": round(gated_tally_event_ms, 3), "gated_tally_wall_ms": round(t_gated_tally * 1e3, 3),
           "inserts_ms": round(t_ins * 1e3, 3), "device_route_ms": round(t_dev * 1e3, 3), "host_route_ms": round(t_host * 1e3, 3),
           "host_over_device": round(t_host / t_dev, 1), "identical": same}
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    sc.close()


if __name__ == "__main__":
    main()
