"""Both strands over 10 M synthetic 150 bp reads resident in HBM: the strands call (seeqdevScanRunStrands: strands_tensor, the merged
records left on the device) against what a caller had to do before it existed -- two run + fetch scans of one context (the pattern, its
reverse complement), both record sets and their line offsets copied to the host, a NumPy merge by the same key (line << 32 | end, plus
first; SQ_BEST: per line the smaller distance, plus on a tie).
Usage (GPU box): python3 profiles/strands_bench.py [reads] -> one JSON line per pattern and mode, appended to profiles/strands_bench.jsonl.
Patterns: the headline 20-mer at d = 3 (two scans) and one barcode at d = 1 (one walk).  Reads: the generator of multi_bench.py with
the pattern and its reverse complement planted in 0.9 of them.  Per cell: 2 untimed runs, then the median and the best of 7 timed ones
(host clock around synchronous calls, the device idle before each); the merge's own device time from HIP events (profiling on).  The
two routes' records are compared."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from seeq_amd import device as dev
from multi_bench import make_reads

PATTERNS = (("20-mer, d 3", "GATGTAGCGCGATTAGCCTG", 3), ("barcode 8 bp, d 1", "ACGTTGCA", 1))
MODES = (("best", dev.SQ_BEST), ("all", dev.SQ_ALL))


def timed(fn, warm=2, runs=7):
    out, ts = None, []
    for it in range(warm + runs):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        if it >= warm: ts.append(dt)
    return statistics.median(ts), min(ts), out


def baseline(sc, pat, twin, text, mode):
    """Two scans, four copies, a NumPy merge -> records [n, 5] u32 (line, start, end, dist, strand)."""
    parts = []
    for strand, p in enumerate((pat, twin)):
        sc.run(p, text.data_ptr(), text.numel(), mode, dev.WANT_RECORDS)
        n = sc.fetch()["nrecords"]
        rec = sc.records(n)
        sc.record_offsets(n)
        parts.append(np.concatenate([rec, np.full((n, 1), strand, dtype=np.uint32)], axis=1))
    both = np.concatenate(parts)
    key = (both[:, 0].astype(np.uint64) << np.uint64(32)) | both[:, 2].astype(np.uint64)
    both = both[np.argsort(key, kind="stable")]             # (stable: plus before minus on a tie)
    if mode == dev.SQ_BEST:
        # per line the smaller distance, plus on a tie: order by (line, dist, strand), keep each line's first
        order = np.lexsort((both[:, 4], both[:, 3], both[:, 0]))
        both = both[order]
        both = both[np.concatenate([[True], both[1:, 0] != both[:-1, 0]])] if len(both) else both
    return both


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    L = 150
    torch.cuda.set_device(0)
    out_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "strands_bench.jsonl")
    for name, expr, tau in PATTERNS:
        text = make_reads(n, L, [expr, dev.revcomp_pattern(expr)], 0.9, 17)
        pat = dev.Pattern(expr, tau)
        twin = pat.revcomp()
        sc = dev.Scanner(torch.cuda.current_stream().cuda_stream)
        for mname, mode in MODES:
            t_plain, _, _ = timed(lambda: (sc.run(pat, text.data_ptr(), text.numel(), mode, dev.WANT_RECORDS), sc.fetch()))
            t_base, t_base_min, exp = timed(lambda: baseline(sc, pat, twin, text, mode))
            t_dev, t_dev_min, res = timed(lambda: sc.strands_tensor(pat, text, mode, dev.WANT_RECORDS, copy=False))
            one_walk = sc.last_multi_one_pass()
            sc.set_profiling(True)
            merge_ms = []
            for _ in range(5):
                sc.strands_tensor(pat, text, mode, dev.WANT_RECORDS, copy=False)
                merge_ms.append(sc.last_strands_merge_ms())
            sc.set_profiling(False)
            got = sc.strand_records(res["nrecords"])
            same = (len(got) == len(exp) and all(np.array_equal(got[f], exp[:, i]) for i, f in enumerate(("line", "start", "end", "dist", "strand"))))
            row = {"pattern": name, "mode": mname, "reads": n, "read_len": L, "one_walk": one_walk, "records": int(res["nrecords"]),
                   "per_strand": res["per_strand"], "plain_scan_ms": round(t_plain * 1e3, 3),
                   "baseline_ms": round(t_base * 1e3, 3), "baseline_best_ms": round(t_base_min * 1e3, 3),
                   "strands_ms": round(t_dev * 1e3, 3), "strands_best_ms": round(t_dev_min * 1e3, 3),
                   "baseline_over_strands": round(t_base / t_dev, 2), "strands_over_plain_scan": round(t_dev / t_plain, 2),
                   "merge_device_ms": round(statistics.median(merge_ms), 4), "identical_to_baseline": bool(same)}
            print(json.dumps(row), flush=True)
            with open(out_path, "a") as f:
                f.write(json.dumps(row) + "\n")
        sc.close()
        twin.close()
        pat.close()
        del text
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
