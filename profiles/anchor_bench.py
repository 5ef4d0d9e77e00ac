"""Counting what lies at a fixed offset from ONE flank, or in fixed columns, of 10 M resident reads: the device route (a fetched scan of
the flank + anchor + tally(source="anchored")) against the route a caller had before the anchor -- the hit records, their offsets and the
text copied to the host, the line ends found and the spans sliced in NumPy, np.unique over them -- and beside both the quality gate and the
plain tally over the same hit records in the same run.
Usage (GPU box): python3 profiles/anchor_bench.py [--lines N] [--distinct M] [--runs K]
  -> one JSON line, appended to profiles/anchor_bench.jsonl.
Input: profiles/tally_append_bench.py's own (N x 200 bp lines, M distinct ones tiled on the device, about 90 % with the six flanks); the
records are the hits of one flank at distance 0 under SQ_BEST.  Two cuts:
  after   the hits of flank C, the one in front of the 12-base UMI; anchor "after", skip 0, length 12: the UMI -- one step of the walk
          per record, whatever the reach;
  line    the hits of flank E, the first one of a read; anchor "line", skip 188, length 0: the last 12 bases of the read -- the walk to
          the line's end, 157 .. 177 bytes behind the hit: three steps.
The device route is timed with profiling on, so the anchor's own HIP-event time (last_anchor_ms) stands beside the gate's
(last_quality_gate_ms: flank C's records, the same reach; on plain lines its "quality line" is the line two below, the walk and the loads are what
they are on FASTQ) and the plain tally's (last_tally_ms, over the 20-base hits themselves).  Best of K timed runs (after one untimed run);
the host route runs once per cut.  Both routes must give the same table."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from seeq_amd import device as dev
from inserts_bench import best_of
from tally_bench import keyed
from tally_append_bench import FC, FE, L, UMI, make_lines

REACH = 1024
CUTS = {"after": dict(flank=FC, anchor="after", skip=0, length=UMI), "line": dict(flank=FE, anchor="line", skip=L - UMI, length=0)}


def host_route(sc, pat, t, cut):
    """What a caller did before the anchor: records, offsets and text to the host, the rule in NumPy, np.unique."""
    n = sc.scan_tensor(pat, t, dev.SQ_BEST, dev.WANT_RECORDS)["nrecords"]
    rec, off, text = sc.records(n), sc.record_offsets(n).astype(np.int64), t.cpu().numpy()
    end = rec[:, 2].astype(np.int64)
    nl = np.flatnonzero(text == 10)
    at = np.searchsorted(nl, off + end)                     # the first newline at or behind the hit's end: the line's end
    length = np.where(at < len(nl), nl[np.minimum(at, len(nl) - 1)], len(text)) - off
    assert int((length - end).max()) < REACH
    s = (end if cut["anchor"] == "after" else np.zeros_like(end)) + cut["skip"]
    e = s + cut["length"] if cut["length"] else length
    keep = (s <= length) & (e <= length)
    s, e, off = s[keep], e[keep], off[keep]
    width = int((e - s).max())
    cols = np.arange(width)
    live = cols[None, :] < (e - s)[:, None]
    span = np.where(live, text[np.minimum((off + s)[:, None] + cols[None, :], len(text) - 1)], 0).astype(np.uint8)
    lines, counts = np.unique(np.ascontiguousarray(span).view("S%d" % width).reshape(-1), return_counts=True)
    return lines, counts, int(keep.sum()), int((e - s).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--distinct", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "anchor_bench.jsonl"))
    args = ap.parse_args()
    distinct = min(args.distinct, args.lines)
    torch.cuda.set_device(0)
    lines, _ = make_lines(distinct, 2000, 41)
    t = torch.from_numpy(lines).cuda().repeat(max(1, args.lines // distinct))
    nlines = t.numel() // (L + 1)
    pats = {f: dev.Pattern(f, 0) for f in (FC, FE)}
    sc = dev.Scanner()
    sc.set_profiling(True)
    row = {"lines": nlines, "read_len": L, "text_bytes": t.numel(), "reach": REACH, "cuts": {}}
    for name, cut in CUTS.items():
        pat = pats[cut["flank"]]
        scan = lambda: sc.scan_tensor(pat, t, dev.SQ_BEST, dev.WANT_RECORDS)      # noqa: E731
        cut_it = lambda: sc.anchor(t, "hits", cut["anchor"], cut["skip"], cut["length"], REACH, copy=False)      # noqa: E731
        state = {}

        def device_route():
            state["scan"] = scan()
            state["cut"] = cut_it()
            return sc.tally(t, source="anchored")
        t_dev, res = best_of(device_route, args.runs)
        anchor_event_ms, tally_event_ms = sc.last_anchor_ms(), sc.last_tally_ms()
        t_cut, _ = best_of(cut_it, args.runs)
        t_tally, _ = best_of(lambda: sc.tally(t, source="anchored", copy=False), args.runs)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        hl, hcounts, kept, nbytes = host_route(sc, pat, t, cut)
        t_host = time.perf_counter() - t0
        hk, hc, hlong, hforeign = keyed(hl, hcounts)
        same = (np.array_equal(hk, res["keys"]) and np.array_equal(hc, res["counts"]) and (hlong, hforeign) == (res["nlong"], res["nforeign"])
                and kept == res["nspans"] == state["cut"]["nkept"] and nbytes == state["cut"]["span_bytes"] and state["cut"]["nspans"] == state["scan"]["nrecords"])
        assert same, "the two routes differ (%s)" % name
        row["cuts"][name] = {"cut": cut, "anchor": state["cut"], "tally": {k: res[k] for k in ("nspans", "ntallied", "ndistinct", "max_len", "passes")},
                             "anchor_event_ms": round(anchor_event_ms, 3), "anchor_wall_ms": round(t_cut * 1e3, 3),
                             "anchored_tally_event_ms": round(tally_event_ms, 3), "anchored_tally_wall_ms": round(t_tally * 1e3, 3),
                             "device_route_ms": round(t_dev * 1e3, 3), "host_route_ms": round(t_host * 1e3, 3), "host_over_device": round(t_host / t_dev, 1),
                             "identical": same}
    # beside them, over flank C's hit records in the same run: the scan, the quality gate, the plain tally
    t_scan, _ = best_of(lambda: sc.scan_tensor(pats[FC], t, dev.SQ_BEST, dev.WANT_RECORDS), args.runs)
    t_gate, gate = best_of(lambda: sc.quality_gate(t, "hits", 20, 33, 0, REACH, copy=False), args.runs)
    gate_event_ms = sc.last_quality_gate_ms()
    t_plain, plain = best_of(lambda: sc.tally(t, source="hits", copy=False), args.runs)
    row.update({"records": gate["nspans"], "scan_ms": round(t_scan * 1e3, 3), "gate_event_ms": round(gate_event_ms, 3), "gate_wall_ms": round(t_gate * 1e3, 3),
                "plain_tally_event_ms": round(sc.last_tally_ms(), 3), "plain_tally_wall_ms": round(t_plain * 1e3, 3), "plain_tally_ndistinct": plain["ndistinct"]})
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    sc.close()


if __name__ == "__main__":
    main()
