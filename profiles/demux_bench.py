"""Demultiplexing sixteen barcodes over 10 M reads: the host route (scan_tensor_multi's records + assign_best in NumPy) against
the device route (seeqdevScanRunDemux: demux_tensor), on the five barcode sets of multi_bench.py.
Usage (GPU box): python3 profiles/demux_bench.py [reads] [set index ...] -> one JSON line per barcode set.
  (a) host:   scan_tensor_multi(SQ_BEST, WANT_RECORDS, copy=False), then assign_best -- the two parts timed apart
  (b) device: demux_tensor(copy=False) -- one record per assigned read, left on the device
  (c) device: demux_tensor(copy=True)  -- the same records copied to the host
Best of 4 timed runs each (after one untimed run); (b) and (c) are checked against (a) through demux_dense."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from seeq_amd import device as dev
from multi_bench import make_reads

SETS = (("16 x 8 bp, d 1", 8, 1, 0.9), ("16 x 10 bp, d 1", 10, 1, 0.9), ("16 x 12 bp, d 1", 12, 1, 0.9),
        ("16 x 10 bp, d 1, no barcode planted", 10, 1, 0.0), ("16 x 8 bp, d 0", 8, 0, 0.9))


def best_of(fn, runs=4):
    out, best = None, None
    for it in range(runs + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        if it and (best is None or dt < best): best = dt
    return best, out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    only = {int(a) for a in sys.argv[2:]}
    L = 150
    torch.cuda.set_device(0)
    rng = np.random.default_rng(3)
    for i, (name, blen, tau, planted) in enumerate(SETS):
        barcodes = ["".join("ACGT"[j] for j in rng.integers(0, 4, size=blen)) for _ in range(16)]      # (drawn for every set: the sets of multi_bench.py)
        if only and i not in only:
            continue
        text = make_reads(n, L, barcodes, planted, 17)
        pats = [dev.Pattern(b, tau) for b in barcodes]
        sc = dev.Scanner(torch.cuda.current_stream().cuda_stream)
        t_scan, got = best_of(lambda: sc.scan_tensor_multi(pats, text, dev.SQ_BEST, dev.WANT_RECORDS, copy=False))
        one_pass = sc.last_multi_one_pass()
        records = sum(int(g["nrecords"]) for g in got)
        t_np, dense = best_of(lambda: dev.assign_best(got, n))
        t_dev, lazy = best_of(lambda: sc.demux_tensor(pats, text, copy=False))
        assert sc.last_multi_one_pass() == one_pass
        t_copy, res = best_of(lambda: sc.demux_tensor(pats, text, copy=True))
        assert all(np.array_equal(x, y) for x, y in zip(dev.demux_dense(res, n), dense)), name
        assert {k: v for k, v in lazy.items() if k != "records"} == {k: v for k, v in res.items() if k != "records"}
        assert res["nassigned"] == int((dense[0] >= 0).sum())
        row = {"set": name, "reads": n, "read_len": L, "one_pass": one_pass,
               "host_route": {"scan_records_ms": round(t_scan * 1e3, 3), "assign_best_ms": round(t_np * 1e3, 3),
                              "total_ms": round((t_scan + t_np) * 1e3, 3), "records": records},
               "demux_device_ms": round(t_dev * 1e3, 3), "demux_copy_ms": round(t_copy * 1e3, 3),
               "assigned": res["nassigned"], "ambiguous": res["nambiguous"],
               "speedup_vs_host_route": round((t_scan + t_np) / t_dev, 2), "device_vs_scan_part": round(t_dev / t_scan, 3),
               "identical_to_assign_best": True}
        print(json.dumps(row), flush=True)
        sc.close()
        for p in pats: p.close()
        del text, got, dense, res, lazy
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
