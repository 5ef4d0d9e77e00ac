#!/usr/bin/env python3
"""What SEEQDEV_FASTQ costs on the README's shape Q: 25 M four-line FASTQ records (100 M lines, 7.9 GB) resident in HBM, `--best`
with WANT_RECORDS, non-DNA modes -x 0 / 1 / 2 -- each scanned plain (as lines) and with the flag, by the SAME context over the
SAME buffer, warmed, median of the steps (a step = seeqdevScanRun + seeqdevScanFetch, wall clock around both).

The flagged step is the plain step plus the record filter of seeq_amd/csrc/seeq_fastq.h (three launches, at most 24 bytes read and
as many written per record of the plain scan) and the host's second synchronisation.  On a tree without the flag (the parent
commit) only the plain rows are measured: `--root DIR` takes the package from another tree.

Each row is appended to --out as one JSON line.
Usage: python profiles/fastq_records_bench.py [--records N] [--steps K] [--warmup W] [--out FILE] [--root DIR] [--label TEXT]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--records", type=int, default=25_000_000)
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "fastq_records_bench.jsonl"))
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from seeq_amd import device as dev                       # noqa: E402

PATTERN, TAU, L = "GATGTAGCGCGATTAGCCTG", 3, 150
FASTQ = getattr(dev, "SEEQDEV_FASTQ", None)
nrec = args.records
d = torch.device("cuda:0")

# the text of profiles/fastq_shape_bench.py: "@r%09d" / a shape-R read / "+" / 150 Phred+33 bytes
reads = torch.empty(nrec * (L + 1), dtype=torch.uint8, device=d)
dev.synth_reads(reads.data_ptr(), 0, nrec, L, PATTERN, TAU)
torch.cuda.synchronize()
HDR = 12
REC = HDR + (L + 1) + 2 + (L + 1)
buf = torch.empty((nrec, REC), dtype=torch.uint8, device=d)
idx = torch.arange(nrec, device=d, dtype=torch.int64)
buf[:, 0] = ord("@"); buf[:, 1] = ord("r")
for k in range(9):
    buf[:, 2 + k] = (48 + (idx // (10 ** (8 - k))) % 10).to(torch.uint8)
buf[:, 11] = 10
buf[:, HDR:HDR + L + 1] = reads.view(nrec, L + 1)
buf[:, HDR + L + 1] = ord("+"); buf[:, HDR + L + 2] = 10
g = torch.Generator(device=d); g.manual_seed(7)
buf[:, HDR + L + 3:HDR + L + 3 + L] = torch.randint(33, 75, (nrec, L), device=d, generator=g, dtype=torch.uint8)
buf[:, REC - 1] = 10
text = buf.view(-1)
del reads, idx
torch.cuda.synchronize()

pat = dev.Pattern(PATTERN, TAU)
sc = dev.Scanner()


def timed(opt):
    for _ in range(args.warmup):
        cnt = sc.scan_tensor(pat, text, opt, dev.WANT_RECORDS)
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        cnt = sc.scan_tensor(pat, text, opt, dev.WANT_RECORDS)
        ms.append((time.perf_counter() - t0) * 1e3)
    return cnt, sc.records(cnt["nrecords"]), ms


with open(args.out, "a") as out:
    for name, nondna in (("fail", 0), ("convert", dev.SQ_CONVERT), ("ignore", dev.SQ_IGNORE)):
        row = {"shape": "Q (4-line FASTQ records)", "label": args.label, "records": nrec, "bytes": int(text.numel()), "nondna": name,
               "steps": args.steps, "warmup": args.warmup}
        cnt, plain, ms = timed(dev.SQ_BEST | nondna)
        row.update(plain_ms_median=statistics.median(ms), plain_ms_min=min(ms), plain_ms_max=max(ms), plain_nlines=int(cnt["nlines"]),
                   plain_nrecords=int(cnt["nrecords"]), kernel=sc.last_kernel())
        if FASTQ is not None:
            cnt, flagged, ms = timed(dev.SQ_BEST | nondna | FASTQ)
            keep = ((plain[:, 0] - 1) & 3) == 1
            want = plain[keep].copy()
            want[:, 0] = ((want[:, 0] - 1) >> 2) + 1
            row.update(fastq_ms_median=statistics.median(ms), fastq_ms_min=min(ms), fastq_ms_max=max(ms), fastq_nlines=int(cnt["nlines"]),
                       fastq_nrecords=int(cnt["nrecords"]), fastq_nmatchlines=int(cnt["nmatchlines"]),
                       fastq_minus_plain_ms=statistics.median(ms) - row["plain_ms_median"],
                       fastq_is_the_filtered_plain_scan=bool(np.array_equal(flagged, want)))
        line = json.dumps(row)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
sc.close()
