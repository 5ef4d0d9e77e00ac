#!/usr/bin/env python3
"""bench.py -- headline benchmark of seeq-mi355x (BASELINE.json):
lines/s and GB/s scanned, 20 bp pattern, d=3, 150 bp synthetic reads, 1 -> 8 MI355X.

A "step" is one pass of the whole hot path (newline handling, automaton / bit-vector scan,
compaction, exact pass with start recovery, ordered records) over one batch of
reads that is already resident in HBM.  Workloads:

  best  (default) BASELINE configs[2]: 100 M x 150 bp reads per GPU, 20 bp pattern, d=3, --best with positions
  count           BASELINE configs[1] shape: -c count-only
  all             the same reads, --all with positions
  cfg5            BASELINE configs[4]: 100 M x 250 bp reads, 40-position bracketed / N pattern, d=5, --all
  chrom           the reference's own published benchmark shape (one chromosome per line, 24 x 128 MiB), --all; one GPU

Multi-GPU (`--gpus N`): one process per GPU (torch.distributed over RCCL), each rank scans its own contiguous
range of read indices (weak scaling, no data-path collective); the global counts are all-reduced inside the
step.  Started without WORLD_SIZE in the environment, `--gpus N` launches the N ranks itself (as a child
`python -m torch.distributed.run`, before this process has touched the GPU) and relays rank 0's line; under the
driver's own torch.distributed.run it is a rank.  Every rank checks that N ranks joined the all-reduce.

A plain run does only what the headline needs: it sets up (the text in the buffer the product's allocator chooses), warms up,
times the steps, writes `--dump-outputs` and prints its line.  `--full` adds everything else: the plain first allocation beside
`value`, the oracle sample and the comparison of every line with the reference binary, and on one GPU the sections (pinned-host
end to end, packed batch, multi-pattern, per call, FASTQ shape, CPU baseline + timed regions + CLI, configs[4]).

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0                 # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)
SEG_BYTES_DEFAULT = 0xF0000000        # the library's segment size (one scan-kernel launch)

WORKLOADS = {
    # name: (pattern, distance, read length, match option, want, description)
    "best": ("GATGTAGCGCGATTAGCCTG", 3, 150, "best", "records",
             "BASELINE configs[2]: %d x 150 bp reads per GPU, 20 bp pattern, d=3, --best with positions (ordered hit records)"),
    "count": ("GATGTAGCGCGATTAGCCTG", 3, 150, "first", "countlines",
              "BASELINE configs[1]: %d x 150 bp reads per GPU, 20 bp pattern, d=3, -c count-only"),
    "all": ("GATGTAGCGCGATTAGCCTG", 3, 150, "all", "records",
            "%d x 150 bp reads per GPU, 20 bp pattern, d=3, --all with positions"),
    "cfg5": ("GATG[TA]AGCNCGATTAGC[CG]TGAAAATGNGAGTAC[GAT]GCGCGA", 5, 250, "all", "records",
             "BASELINE configs[4]: %d x 250 bp reads per GPU, 40-position bracketed/IUPAC pattern, d=5, --all matches with positions"),
}


def host_cores():
    import multiprocessing
    cores = max(1, multiprocessing.cpu_count() // 2)      # physical cores if SMT-2, else a conservative half
    try:
        out = subprocess.run(["lscpu", "-p=CORE,SOCKET"], capture_output=True, text=True).stdout
        phys = {tuple(l.split(",")) for l in out.splitlines() if l and not l.startswith("#")}
        sock0 = {c for c, s in phys if s == "0"}
        if sock0:
            cores = len(sock0)
    except Exception:
        pass
    return min(cores, multiprocessing.cpu_count())


def cpu_quota():
    """CPUs this process may use at once according to its cgroup (None: no limit found)."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else float(q) / float(per)
    except Exception:
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else q / per
    except Exception:
        return None


def cpu_baseline(sample_lines, pattern, tau, read_len, mode):
    """The reference itself (oracle/_ref/seeq_ref, built from /root/reference in the build container) timed on this box's
    host cores over a bounded sample of the same workload, as BASELINE.md section 3 prescribes: P = physical cores of one
    socket, P single-threaded processes, each pinned to its own core (sched_setaffinity) and scanning its OWN contiguous
    shard of the sample (page-cache warm, /dev/shm), best of 2; and one process alone."""
    from oracle.pyoracle import Oracle, REF_BIN
    from seeq_amd.device import plain_pattern
    orc = Oracle()
    cores = host_cores()
    try:
        allowed = sorted(os.sched_getaffinity(0))
    except AttributeError:
        allowed = list(range(cores))
    cores = max(1, min(cores, len(allowed)))
    phys = cores
    quota = cpu_quota()
    if quota and quota < cores:                              # a container's CPU share: more processes than that only take turns
        cores = max(1, int(quota))
    tmpdir = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    per = max(100_000, sample_lines // 2)                   # lines per shard (about 0.7 s of work for one process): the sample is `cores` shards
    flags = {"first": ["-c"], "best": ["-b", "-f"], "all": ["-a", "-f"]}[mode]
    paths = []
    try:
        if os.path.exists(REF_BIN):
            kind = "reference"
            for k in range(cores):
                path = os.path.join(tmpdir, "seeq_bench_shard_%d_%d.txt" % (os.getpid(), k))
                orc.synth_reads(k * per, per, read_len, plain_pattern(pattern), tau).tofile(path)
                paths.append(path)

            def run_parallel(p):
                t0 = time.perf_counter()
                procs = [subprocess.Popen([REF_BIN, "-d", str(tau)] + flags + [pattern, paths[k]], stdout=subprocess.DEVNULL,
                                          preexec_fn=(lambda c=allowed[k]: os.sched_setaffinity(0, {c}))) for k in range(p)]
                for q in procs:
                    q.wait()
                return time.perf_counter() - t0
            run_parallel(1)                                   # page cache + DFA warm
            t1 = min(run_parallel(1) for _ in range(2))
            tp = min(run_parallel(cores) for _ in range(2)) if cores > 1 else t1
            one = per / t1
            agg = cores * per / tp
            sample = ("%d shards of %d synthetic %d bp reads (same generator/seed as the GPU run), %s; %d single-threaded processes, "
                      "each pinned to its own core and scanning its own shard (page-cache warm), best of 2"
                      % (cores, per, read_len, " ".join(["seeq", "-d", str(tau)] + flags), cores))
        else:
            kind = "port"
            cores = 1
            data = orc.synth_reads(0, per, read_len, plain_pattern(pattern), tau)
            t0 = time.perf_counter()
            orc.buffer_scan(pattern, tau, data, 1)
            one = agg = per / (time.perf_counter() - t0)
            sample = "%d synthetic %d bp reads through the repo's own CPU restatement (oracle/), NOT the reference" % (per, read_len)
    finally:
        for path in paths:
            try:
                os.unlink(path)
            except OSError:
                pass
    return {"value": agg, "unit": "lines/s", "cores": cores, "kind": kind, "one_core_lines_per_s": one, "pinned": True,
            "own_shards": True, "sample": sample, "physical_cores_one_socket": phys, "cpu_quota": quota,
            "whole_socket_estimate_lines_per_s": one * phys,
            "note": "cores = the processes actually run: the physical cores of one socket, capped by the container's CPU quota; "
                    "whole_socket_estimate = one-core rate x physical cores (an extrapolation, not a measurement)"}


def cli_wall_clock(pattern, tau, read_len, lines=10_000_000):
    """Timed region (iii) of SURVEY 8d: `seeq -c -d 3 PATTERN file` wall clock on a page-cache-warm file of 10 M lines, the
    product CLI (process start, HIP start-up, reader threads, H2D, kernels) beside the reference binary on one core."""
    from oracle.pyoracle import Oracle, REF_BIN
    from seeq_amd import _capi
    from seeq_amd.device import plain_pattern
    orc = Oracle()
    tmpdir = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    path = os.path.join(tmpdir, "seeq_bench_cli_%d.txt" % os.getpid())
    out = {"lines": lines, "command": "seeq -c -d %d %s <file of %d x %d bp reads, page-cache warm>" % (tau, pattern, lines, read_len)}
    try:
        with open(path, "wb") as f:
            for first in range(0, lines, 1_000_000):
                orc.synth_reads(first, min(1_000_000, lines - first), read_len, plain_pattern(pattern), tau).tofile(f)
        cmd = ["-c", "-d", str(tau), pattern, path]

        def timed(exe):
            best, res = None, None
            for _ in range(3):
                t0 = time.perf_counter()
                r = subprocess.run([exe] + cmd, capture_output=True, text=True)
                dt = time.perf_counter() - t0
                if r.returncode != 0:
                    return None, r.stderr[-200:]
                best, res = (dt if best is None else min(best, dt)), r.stdout.strip()
            return best, res
        g, gres = timed(_capi.CLI_PATH)
        out["gpu_seconds"], out["gpu_count"] = g, gres
        if g:
            out["gpu_lines_per_s"] = lines / g
        if os.path.exists(REF_BIN):
            c, cres = timed(REF_BIN)
            out["reference_seconds_one_core"], out["reference_count"] = c, cres
            if c and g:
                out["counts_identical"] = gres == cres
                out["reference_lines_per_s_one_core"] = lines / c
    finally:
        try:
            os.unlink(path)
        except OSError:
            pass
    return out


def source_hash():
    """Content hash of the kernel sources: ties measured-once figures (PMC traffic) to the build they were measured on."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "seeq_amd", "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".h", ".hip", ".c")):
            h.update(name.encode())
            h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()[:16]


def seeq_scan_host_ptr(scanner, pat, host_ptr, nbytes, opt, want):
    """seeqdevScanHost on a raw host pointer (pinned torch tensor)."""
    import ctypes as C
    from seeq_amd import _capi
    cnt = _capi.seeqdev_counts_t()
    rc = _capi.lib().seeqdevScanHost(scanner._h, pat.handle, C.cast(host_ptr, C.c_char_p), nbytes, opt, want, C.byref(cnt))
    assert rc == 0, _capi.error_text()
    return dict(nlines=cnt.nlines, nmatchlines=cnt.nmatchlines, nhits=cnt.nhits, nrecords=cnt.nrecords)


# ---------------------------------------------------------------------------------------------------------------
# Full-size parity: blocks of the scanned text against the oracle (outside the timed region)
# ---------------------------------------------------------------------------------------------------------------
def parity_blocks(n, read_len, seg_bytes, prefix_lines, block_lines=65536, every=97, seam_lines=2048):
    """[first, count) line ranges to verify: a prefix, every `every`-th block of `block_lines`, and the lines
    around every segment seam (a line there is split between two scan-kernel launches)."""
    prefix = min(n, prefix_lines)
    out = [(f, min(block_lines, prefix - f)) for f in range(0, prefix, block_lines)]      # the prefix, cut for the pool
    nblocks = (n + block_lines - 1) // block_lines
    for b in range(every, nblocks, every):
        first = b * block_lines
        if first >= prefix:
            out.append((first, min(block_lines, n - first)))
    seams = []
    k = 1
    while k * seg_bytes < n * (read_len + 1):
        line = (k * seg_bytes) // (read_len + 1)
        first = max(0, line - seam_lines // 2)
        seams.append((first, min(seam_lines, n - first)))
        k += 1
    return out, seams


_CHECK_CHILD = r'''
import json, sys
import numpy as np
sys.path.insert(0, %r)
from oracle.pyoracle import Oracle
o = Oracle()
job = json.load(open(sys.argv[1]))
res = []
for blk in job["blocks"]:
    data = np.fromfile(blk["file"], dtype=np.uint8)
    exp = o.buffer_scan(job["pattern"], job["tau"], data, job["opt"])
    np.save(blk["file"] + ".rec.npy", exp["records"])
    res.append({"nlines": int(exp["nlines"]), "nmatchlines": int(exp["nmatchlines"])})
json.dump(res, open(sys.argv[1] + ".out", "w"))
'''


class ClockSampler:
    """Core clock / power of the GPU while the timed steps run, read from sysfs every 20 ms by a thread (no GPU call, no
    subprocess): the scan kernel comes in two speeds box by box -- is it the clock?  Empty when the files are not readable."""

    def __init__(self, index):
        import glob
        self.files = {}
        cards = sorted(glob.glob("/sys/class/drm/card*/device"))
        cards = [c for c in cards if os.path.exists(os.path.join(c, "pp_dpm_sclk"))]
        if index < len(cards):
            base = cards[index]
            self.files["sclk_dpm"] = os.path.join(base, "pp_dpm_sclk")
            for h in glob.glob(os.path.join(base, "hwmon", "hwmon*")):
                for name, key in (("freq1_input", "sclk_hz"), ("power1_average", "power_uw"), ("power1_input", "power_uw"),
                                  ("temp1_input", "temp_mc")):
                    f = os.path.join(h, name)
                    if os.path.exists(f) and key not in self.files:
                        self.files[key] = f
        self.samples = {k: [] for k in self.files}
        self._stop = False
        self._thread = None

    def _read(self):
        for k, f in self.files.items():
            try:
                txt = open(f).read()
            except OSError:
                continue
            if k == "sclk_dpm":
                cur = [ln for ln in txt.splitlines() if ln.rstrip().endswith("*")]
                if cur:
                    try:
                        self.samples[k].append(float(cur[0].split(":")[1].strip().rstrip("*").strip().lower().replace("mhz", "")))
                    except (ValueError, IndexError):
                        pass
            else:
                try:
                    self.samples[k].append(float(txt.strip()))
                except ValueError:
                    pass

    def _loop(self):
        while not self._stop:
            self._read()
            time.sleep(0.02)

    def start(self):
        import threading
        if not self.files:
            return
        self._read()
        self._thread = threading.Thread(target=self._loop, daemon=True)
        self._thread.start()

    def stop(self):
        self._stop = True
        if self._thread:
            self._thread.join()
            self._read()

    def summary(self):
        out = {}
        scale = {"sclk_dpm": ("sclk_mhz_dpm", 1.0), "sclk_hz": ("sclk_mhz", 1e-6), "power_uw": ("power_w", 1e-6), "temp_mc": ("temp_c", 1e-3)}
        for k, v in self.samples.items():
            if v:
                name, f = scale[k]
                out[name] = {"min": min(v) * f, "mean": sum(v) / len(v) * f, "max": max(v) * f, "samples": len(v)}
        return out or None


def stats3(v):
    v = sorted(v)
    return {"min": v[0], "median": v[len(v) // 2], "max": v[-1]} if v else None


DUMP_MAX_RECORDS = 1 << 20            # --dump-outputs: 32 MiB of records + 8 MiB of their indices (float64), under the 64 MB cap
DUMP_SEED = 0x5EE9


def dump_outputs(dirname, counts, rec):
    """--dump-outputs DIR: what a caller of the timed path received from its last step, as float64 .npy files --
    counts.npy (lines, matching lines, hits, records, headers) and, for the record workloads, records.npy [k, 4]
    (line, start, end, dist) with record_index.npy [k], the positions of those rows in the full record list: all of
    them up to DUMP_MAX_RECORDS, else a sorted sample of that many drawn with a fixed seed."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    keys = ("nlines", "nmatchlines", "nhits", "nrecords", "nheaders")
    np.save(os.path.join(dirname, "counts.npy"), np.array([counts[k] for k in keys], dtype=np.float64))
    if rec is None:
        return
    n = len(rec)
    if n > DUMP_MAX_RECORDS:
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(n, DUMP_MAX_RECORDS, replace=False))
    else:
        idx = np.arange(n)
    np.save(os.path.join(dirname, "records.npy"), rec[idx].astype(np.float64))
    np.save(os.path.join(dirname, "record_index.npy"), idx.astype(np.float64))


def reference_full_check(text, n, read_len, pattern, tau, mode, rec, matching_lines, shard_lines=1_000_000):
    """EVERY line of the run against the reference itself (oracle/_ref/seeq_ref, the reference's own C files): the device text
    goes to /dev/shm in waves of P shards (P = the host cores this process may use), P pinned reference processes print
    `line:start-end:dist` rows (src/seeq.c:131-137, -f) -- or their count (-c) -- and every row is compared with the GPU's record
    list; the total with the GPU's count.  Returns a dict for the bench line, or None when the binary is not there."""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    from oracle.pyoracle import REF_BIN
    if not os.path.exists(REF_BIN):
        return None
    try:
        allowed = sorted(os.sched_getaffinity(0))
    except AttributeError:
        allowed = list(range(os.cpu_count() or 1))
    procs = len(allowed)
    quota = cpu_quota()
    if quota and quota < procs:
        procs = max(1, int(quota))
    tmpdir = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    base = os.path.join(tmpdir, "seeq_bench_full_%d" % os.getpid())
    L = read_len + 1
    flags = {"first": ["-c"], "best": ["-b", "-f"], "all": ["-a", "-f"]}[mode]
    shards = [(f0, min(shard_lines, n - f0)) for f0 in range(0, n, shard_lines)]
    t0 = time.perf_counter()
    rows_total = lines_total = count_total = 0
    ref_seconds = 0.0
    table = bytes.maketrans(b":-", b"  ")
    files = []
    try:
        with ThreadPoolExecutor(max_workers=min(8, procs)) as pool:
            for w0 in range(0, len(shards), procs):
                wave = shards[w0:w0 + procs]
                paths = ["%s_%d.txt" % (base, k) for k in range(len(wave))]
                files = paths + [p_ + ".out" for p_ in paths]

                def dump(k):
                    f0, cnt = wave[k]
                    text[f0 * L:(f0 + cnt) * L].cpu().numpy().tofile(paths[k])
                list(pool.map(dump, range(len(wave))))
                t1 = time.perf_counter()
                children = []
                for k in range(len(wave)):
                    out = open(paths[k] + ".out", "wb")
                    children.append((subprocess.Popen([REF_BIN, "-d", str(tau)] + flags + [pattern, paths[k]], stdout=out,
                                                      preexec_fn=(lambda c=allowed[k % len(allowed)]: os.sched_setaffinity(0, {c}))), out))
                for proc, out in children:
                    assert proc.wait() == 0, "the reference binary failed"
                    out.close()
                ref_seconds += time.perf_counter() - t1
                for k, (f0, cnt) in enumerate(wave):
                    raw = open(paths[k] + ".out", "rb").read()
                    if mode == "first":
                        count_total += int(raw.split()[0]) if raw.split() else 0
                    else:
                        exp = np.array(raw.translate(table).split(), dtype=np.int64).reshape(-1, 4) if raw else np.zeros((0, 4), np.int64)
                        exp[:, 0] += f0                               # the shard's line numbers start at 1
                        exp[:, 2] += 1                                # printed end is inclusive (seeq.c:135)
                        lo = np.searchsorted(rec[:, 0], f0 + 1, side="left")
                        hi = np.searchsorted(rec[:, 0], f0 + cnt, side="right")
                        got = rec[lo:hi].astype(np.int64)
                        assert np.array_equal(got, exp), "GPU records differ from the reference binary in lines [%d, %d)" % (f0, f0 + cnt)
                        rows_total += len(exp)
                        count_total += len(np.unique(exp[:, 0]))
                    lines_total += cnt
                for f in files:
                    if os.path.exists(f):
                        os.unlink(f)
                files = []
    finally:
        for f in files:
            if os.path.exists(f):
                os.unlink(f)
    assert count_total == matching_lines, ("matching lines: reference %d, GPU %d" % (count_total, matching_lines))
    if rec is not None:
        assert rows_total == len(rec), ("records: reference %d, GPU %d" % (rows_total, len(rec)))
    return {"reference_lines_checked": lines_total, "reference_rows_compared": rows_total, "matching_lines": count_total,
            "command": " ".join(["seeq", "-d", str(tau)] + flags + [pattern]), "processes": procs, "shard_lines": shard_lines,
            "reference_seconds": ref_seconds, "reference_check_seconds": time.perf_counter() - t0, "reference_result": "identical"}


def fastq_shape(reads, nrec, L, pattern, tau, pat, steps=5):
    """Section `fastq_shape` of the bench line: `nrec` four-line FASTQ records built on the device from the resident reads (torch:
    plumbing), scanned through the C-ABI under SQ_FAIL / SQ_CONVERT / SQ_IGNORE."""
    import numpy as np
    import torch
    from seeq_amd import device as dev
    from oracle.pyoracle import Oracle, REF_BIN
    d = reads.device
    HDR = 12                                                 # "@r%09d\n"
    REC = HDR + (L + 1) + 2 + (L + 1)
    buf = torch.empty((nrec, REC), dtype=torch.uint8, device=d)
    idx = torch.arange(nrec, device=d, dtype=torch.int64)
    buf[:, 0] = ord("@"); buf[:, 1] = ord("r")
    for k in range(9):
        buf[:, 2 + k] = (48 + (idx // (10 ** (8 - k))) % 10).to(torch.uint8)
    buf[:, 11] = 10
    buf[:, HDR:HDR + L + 1] = reads[:nrec * (L + 1)].view(nrec, L + 1)
    buf[:, HDR + L + 1] = ord("+"); buf[:, HDR + L + 2] = 10
    g = torch.Generator(device=d); g.manual_seed(7)
    buf[:, HDR + L + 3:HDR + L + 3 + L] = torch.randint(33, 75, (nrec, L), device=d, generator=g, dtype=torch.uint8)
    buf[:, REC - 1] = 10
    text = buf.view(-1)
    del idx
    torch.cuda.synchronize()
    res = {"records": nrec, "lines": 4 * nrec, "bytes": int(text.numel()), "match_option": "--best with positions", "modes": {}}
    # the reference's counts over the whole buffer: shards of 500 k whole records in /dev/shm, waves of P pinned processes, the three modes per wave
    ref_counts = None
    files = []
    if os.path.exists(REF_BIN):
        try:
            allowed = sorted(os.sched_getaffinity(0))
        except AttributeError:
            allowed = list(range(os.cpu_count() or 1))
        procs = len(allowed)
        quota = cpu_quota()
        if quota and quota < procs:
            procs = max(1, int(quota))
        tmpdir = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
        per = 500_000
        shards = [(lo, min(nrec, lo + per)) for lo in range(0, nrec, per)]
        ref_counts = {"fail": 0, "convert": 0, "ignore": 0}
        tref = time.perf_counter()
        try:
            for w0 in range(0, len(shards), procs):
                wave = shards[w0:w0 + procs]
                files = [os.path.join(tmpdir, "seeq_bench_fq_%d_%d.txt" % (os.getpid(), k)) for k in range(len(wave))]
                for f, (lo, hi) in zip(files, wave):
                    buf[lo:hi].reshape(-1).cpu().numpy().tofile(f)
                for name, x in (("fail", "0"), ("convert", "1"), ("ignore", "2")):
                    ps = [subprocess.Popen([REF_BIN, "-c", "-d", str(tau), "-x", x, pattern, f], stdout=subprocess.PIPE, text=True,
                                           preexec_fn=(lambda c=allowed[k % len(allowed)]: os.sched_setaffinity(0, {c}))) for k, f in enumerate(files)]
                    ref_counts[name] += sum(int(p_.communicate()[0].split()[0]) for p_ in ps)
                for f in files:
                    os.unlink(f)
                files = []
        finally:
            for f in files:
                if os.path.exists(f):
                    os.unlink(f)
        res["reference_count_seconds"] = round(time.perf_counter() - tref, 1)
    orc = Oracle()
    kpre = 50_000                                            # records of the oracle prefix (200 k lines)
    host = text[:kpre * REC].cpu().numpy()
    for name, nd in (("fail", 0), ("convert", dev.SQ_CONVERT), ("ignore", dev.SQ_IGNORE)):
        sc = dev.Scanner()
        sc.set_profiling(True)
        opt = dev.SQ_BEST | nd
        for _ in range(2):
            cnt = sc.scan_tensor(pat, text, opt, dev.WANT_RECORDS)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            cnt = sc.scan_tensor(pat, text, opt, dev.WANT_RECORDS)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        kern = sc.last_kernel()
        exp = orc.buffer_scan(pattern, tau, host, opt)
        s2 = dev.Scanner()
        c2 = s2.scan_tensor(pat, text[:kpre * REC], opt, dev.WANT_RECORDS)
        ok = c2["nmatchlines"] == exp["nmatchlines"] and c2["nlines"] == exp["nlines"] and \
            np.array_equal(s2.records(c2["nrecords"]).astype(np.uint64), exp["records"])
        s2.close()
        tm = sc.last_times_ms()
        row = {"lines_per_s": cnt["nlines"] / dt, "gb_per_s": text.numel() / dt / 1e9, "whole_step_frac": text.numel() / dt / 1e9 / HBM_PEAK_GBS,
               "ms_per_step": dt * 1e3, "kernel": kern, "scan_launches": tm["forward_launches"], "forward_scan_ms": round(tm["forward"], 4),
               "post_pass_ms": round(tm["exact"], 4), "matching_lines": int(cnt["nmatchlines"]), "oracle_prefix_records_identical": bool(ok)}
        if ref_counts is not None:
            row["reference_matching_lines"] = ref_counts[name]
            row["identical_to_reference_count"] = ref_counts[name] == int(cnt["nmatchlines"])
            assert row["identical_to_reference_count"], ("FASTQ shape, -x mode %s: GPU %d matching lines, reference %d" % (name, cnt["nmatchlines"], ref_counts[name]))
        assert ok, "FASTQ shape, mode %s: records of the prefix differ from the oracle's" % name
        res["modes"][name] = row
        sc.close()
    del buf, text
    return res


def oracle_check(text, ranges, read_len, pattern, tau, opt, want_records, rec, scan_block, procs):
    """Run the oracle over the given line ranges of the device text in `procs` child processes (the text of each
    range is copied from HBM to /dev/shm) and compare: records (line, start, end, dist) bit for bit, and per range
    the number of lines / matching lines.  `rec`: all GPU records of this rank (or None for count workloads, then
    `scan_block(first, count)` rescans the range on the GPU).  Returns (lines checked, ranges checked)."""
    import numpy as np
    tmpdir = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    base = os.path.join(tmpdir, "seeq_bench_chk_%d" % os.getpid())
    L = read_len + 1
    jobs = [[] for _ in range(max(1, procs))]
    files = []
    order = sorted(range(len(ranges)), key=lambda i: -ranges[i][1])          # longest first, round robin
    for j, i in enumerate(order):
        first, count = ranges[i]
        path = "%s_%d.bin" % (base, i)
        text[first * L:(first + count) * L].cpu().numpy().tofile(path)
        files.append(path)
        jobs[j % len(jobs)].append({"idx": i, "file": path})
    children = []
    try:
        for k, blocks in enumerate(jobs):
            if not blocks:
                continue
            jp = "%s_job%d.json" % (base, k)
            json.dump({"pattern": pattern, "tau": tau, "opt": opt, "blocks": blocks}, open(jp, "w"))
            files += [jp, jp + ".out"]
            children.append((subprocess.Popen([sys.executable, "-c", _CHECK_CHILD % ROOT, jp]), jp, blocks))
        lines_checked = 0
        for proc, jp, blocks in children:
            assert proc.wait() == 0, "oracle child failed"
            res = json.load(open(jp + ".out"))
            for blk, r in zip(blocks, res):
                first, count = ranges[blk["idx"]]
                exp_rec = np.load(blk["file"] + ".rec.npy")
                files.append(blk["file"] + ".rec.npy")
                assert r["nlines"] == count, ("line count", first, count, r)
                if want_records:
                    lo = np.searchsorted(rec[:, 0], first + 1, side="left")
                    hi = np.searchsorted(rec[:, 0], first + count, side="right")
                    got = rec[lo:hi].astype(np.uint64)
                    got[:, 0] -= first
                    assert np.array_equal(got, exp_rec), "GPU records differ from the oracle in lines [%d, %d)" % (first, first + count)
                    assert len(np.unique(got[:, 0])) == r["nmatchlines"], ("matching lines", first, count)
                else:
                    c = scan_block(first, count)
                    assert c["nlines"] == count and c["nmatchlines"] == r["nmatchlines"], \
                        "GPU counts differ from the oracle in lines [%d, %d): %r vs %r" % (first, first + count, c, r)
                lines_checked += count
        return lines_checked, len(ranges)
    finally:
        for f in files:
            try:
                os.unlink(f)
            except OSError:
                pass


def per_call_rates(pattern, tau, read_len, nstrings=20000):
    """strings/s through the per-string entry point seeqStringMatch (what the reference's Python module calls,
    seeqmodule.c:858) and through the batched module calls, next to the reference's own per-call rate."""
    import ctypes as C
    import numpy as np
    import seeq_amd as seeq
    from oracle.pyoracle import Oracle, REF_LIB
    from seeq_amd import _capi
    from seeq_amd.device import plain_pattern
    orc = Oracle()
    data = orc.synth_reads(0, nstrings, read_len, plain_pattern(pattern), tau).tobytes()
    strings = data.split(b"\n")[:nstrings]
    out = {"strings": nstrings, "string_len": read_len}
    L = _capi.lib()
    sq = L.seeqNew(pattern.encode(), tau, 0)
    for s in strings[:50]:
        L.seeqStringMatch(s, sq, 1)
    t0 = time.perf_counter()
    nh = 0
    k = min(len(strings), 4000)
    for s in strings[:k]:
        nh += L.seeqStringMatch(s, sq, 1) > 0
    dt = time.perf_counter() - t0
    out["seeqStringMatch"] = {"strings_per_s": k / dt, "us_per_call": 1e6 * dt / k, "matched": int(nh), "calls": k}
    L.seeqFree(sq)
    m = seeq.compile(pattern, tau)
    texts = [s.decode() for s in strings]
    m.matchBestBatch(texts)                      # (workspace sized by the first batch of this size, like the 1 000 warm-up calls below)
    t0 = time.perf_counter()
    res = m.matchBestBatch(texts)
    dt = time.perf_counter() - t0
    out["matchBestBatch"] = {"strings_per_s": len(texts) / dt, "matched": sum(1 for r in res if r),
                             "note": "one call with all strings, second call of this size (str -> one buffer, H2D, scan, D2H, Python lists)"}
    if os.path.exists(REF_LIB):
        R = C.CDLL(REF_LIB)
        R.seeqNew.restype = C.c_void_p
        R.seeqNew.argtypes = [C.c_char_p, C.c_int, C.c_size_t]
        R.seeqStringMatch.restype = C.c_long
        R.seeqStringMatch.argtypes = [C.c_char_p, C.c_void_p, C.c_int]
        R.seeqFree.argtypes = [C.c_void_p]
        rsq = R.seeqNew(pattern.encode(), tau, 0)
        for s in strings[:1000]:
            R.seeqStringMatch(s, rsq, 1)
        t0 = time.perf_counter()
        nr = 0
        for s in strings:
            nr += R.seeqStringMatch(s, rsq, 1) > 0
        dt = time.perf_counter() - t0
        out["reference_seeqStringMatch"] = {"strings_per_s": len(strings) / dt, "matched": int(nr),
                                            "note": "reference libseeq through ctypes, one host core (ctypes call overhead included on both sides)"}
        R.seeqFree(rsq)
    return out


def bench_chrom(args):
    """--workload chrom: the reference's own published benchmark shape (doc/response.tex:181-232) -- a genome with one
    chromosome per line: 24 lines x 128 MiB of random DNA (3.2 GB) with planted approximate copies, pattern = a prefix of
    GATGTAGCGCGATTAGCCTGAAAATGCGAGTACGGCGCGAAT (--pattern, default its first 20 positions; --distance, default 3), `--all`
    with positions.  One step = one scan of the resident text.  With --full: records checked against the oracle on the tails of two
    lines; cpu_baseline = the reference binary over the same bytes on one core."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import chrom_sweep
    from seeq_amd import device as dev
    from oracle.pyoracle import Oracle, REF_BIN
    pattern = args.pattern or chrom_sweep.FULL[:20]
    tau = 3 if args.distance is None else args.distance
    nlines, L = 24, 128 << 20
    torch.cuda.set_device(0)
    text = chrom_sweep.make_text(nlines, L, torch.device("cuda:0"))
    nbytes = int(text.numel())
    pat = dev.Pattern(pattern, tau)
    sc = dev.Scanner(torch.cuda.current_stream().cuda_stream)
    sc.set_profiling(True)
    for _ in range(max(1, args.warmup)):
        cnt = sc.scan_tensor(pat, text, dev.SQ_ALL, dev.WANT_RECORDS)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fwd = 0.0
    for _ in range(args.steps):
        cnt = sc.scan_tensor(pat, text, dev.SQ_ALL, dev.WANT_RECORDS)
        fwd += sc.last_times_ms()["forward"]
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / args.steps
    rec = sc.records(cnt["nrecords"])
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, cnt, rec)
    if args.full:
        k = 64 << 20
        sample = torch.cat([text[L - k:L], text[2 * L - k:2 * L]]).contiguous()
        exp = Oracle().buffer_scan(pattern, tau, sample.cpu().numpy(), dev.SQ_ALL)
        s2 = dev.Scanner()
        got = s2.scan_tensor(pat, sample, dev.SQ_ALL, dev.WANT_RECORDS)
        assert np.array_equal(s2.records(got["nrecords"]).astype(np.uint64), exp["records"]), "GPU records differ from the oracle on the sampled lines"
    fwd_ms = fwd / args.steps
    algo = nbytes + 16 * cnt["nrecords"] + 8
    out = {"metric": "GB/s scanned, one chromosome per line (24 x 128 MiB), %d bp pattern, d=%d, --all with positions" % (len(dev.plain_pattern(pattern)), tau),
           "value": nbytes / el / 1e9, "unit": "GB/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": el * 1e3,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "u32 bit-vectors" if sc.last_kernel() == "k_myers" else "int (u16 automaton state ids)", "data": "synthetic",
           "config": {"workload": "reference's published benchmark shape: 24 lines x 128 MiB random DNA, planted copies", "pattern": pattern, "distance": tau},
           "results": {"lines": int(cnt["nlines"]), "records": int(cnt["nrecords"]),
                       "oracle_check": "records of two 64 MiB line tails bit-exact" if args.full else None},
           "roofline": {"bound": "hbm", "kernel": sc.last_kernel(), "achieved": algo / (fwd_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": algo / (fwd_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None, "avg_launch_ms": fwd_ms, "algorithmic_bytes_per_launch": algo}}
    if args.full and not args.no_cpu_baseline and os.path.exists(REF_BIN):
        path = "/dev/shm/seeq_bench_chrom_%d.txt" % os.getpid()
        try:
            text.cpu().numpy().tofile(path)
            t1 = time.perf_counter()
            r = subprocess.run([REF_BIN, "-d", str(tau), "-a", "-f", pattern, path], capture_output=True, text=True)
            secs = time.perf_counter() - t1
            got_rows = ["%d:%d-%d:%d" % (a, b, c - 1, d) for a, b, c, d in rec.tolist()]
            out["cpu_baseline"] = {"value": nbytes / secs / 1e9, "unit": "GB/s", "cores": 1, "kind": "reference", "seconds": secs,
                                   "sample": "the same 3.2 GB, seeq -d %d -a -f, one process" % tau, "records_identical": r.stdout.splitlines() == got_rows}
            out["gpu_over_cpu"] = out["value"] / out["cpu_baseline"]["value"]
        finally:
            if os.path.exists(path):
                os.remove(path)
    print(json.dumps(out))


def launch_ranks(args):
    """--gpus N without a launcher: start N ranks (one per GPU) as a child torch.distributed.run BEFORE this process
    touches the GPU, relay rank 0's JSON line, exit with the child's status."""
    import socket
    import torch
    share = os.environ.get("SEEQ_BENCH_SHARE_GPU") == "1"       # test mode: all ranks on GPU 0, gloo collectives
    ndev = torch.cuda.device_count()                            # does not initialise the GPU on this image
    if not share and ndev < args.gpus:
        sys.stderr.write("bench.py: --gpus %d but only %d GPU(s) visible\n" % (args.gpus, ndev))
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for l in proc.stdout.splitlines():
        if l.startswith("{") and '"metric"' in l:
            line = l
    if proc.returncode != 0 or line is None:
        sys.stderr.write("bench.py: the %d-rank launch failed (exit %d)\n%s\n" % (args.gpus, proc.returncode, proc.stdout[-2000:]))
        return proc.returncode or 1
    if json.loads(line)["n_gpus"] != args.gpus:
        sys.stderr.write("bench.py: asked for %d ranks, the line reports %d\n" % (args.gpus, json.loads(line)["n_gpus"]))
        return 1
    print(line)
    return 0


class Ctx:
    """What every section of a run needs: the modules, the process-group facts, the command line."""
    pass


def timed_steps(ctx, sc, pat, text_ptr, nbytes, opt, want, steps, barrier):
    """`steps` passes of the hot path over resident text (seeqdevScanRun + seeqdevScanFetch + the count reduce), bracketed as the driver's
    contract says; returns the host-clock seconds and the device-side sums."""
    import gc
    torch, dist, shard = ctx.torch, ctx.dist, ctx.shard
    if barrier and ctx.world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    gc.disable()                                               # (no collector pause inside the timed region)
    acc = {"fwd_ms": 0.0, "launches": 0, "idx_ms": 0.0, "ex_ms": 0.0, "step_wall": [], "step_fwd": [], "step_post": [], "launch_ms": [], "clk": []}
    total = local = None
    t0 = time.perf_counter()
    for _ in range(steps):
        ts = time.perf_counter()
        sc.run(pat, text_ptr, nbytes, opt, want)
        local = sc.fetch()
        total = shard.reduce_counts(local, device=ctx.red_device, force=ctx.force_dist)
        acc["step_wall"].append(1e3 * (time.perf_counter() - ts))
        tm = sc.last_times_ms()
        acc["fwd_ms"] += tm["forward"]; acc["launches"] += tm["forward_launches"]; acc["idx_ms"] += tm["index"]; acc["ex_ms"] += tm["exact"]
        acc["step_fwd"].append(tm["forward"]); acc["step_post"].append(tm["exact"])
        acc["launch_ms"].extend(sc.last_launch_times_ms())
        clk = sc.last_clock_mhz()
        if clk > 0:
            acc["clk"].append(clk)
    if barrier and ctx.world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    gc.enable()
    return elapsed, acc, total, local


def run_workload(ctx, name, n, steps, warmup, candidates, first_steps, check_lines, check_mode, keep):
    """One workload of WORKLOADS at `n` reads per rank: the text in a buffer from the PRODUCT's allocator (seeqdevTextAllocFor through
    dev.TextBuffer: `candidates` probed, the fastest kept), `steps` timed steps, the checks outside the timed region.  Before that, when
    candidates > 1, the same text in a plain first allocation (what a caller that hipMallocs once gets) for `first_steps` timed steps:
    `first_allocation`.  Returns the section of the bench line; with `keep` also the live objects (text, scanner, pattern, records)."""
    torch, np, dev = ctx.torch, ctx.np, ctx.dev
    args = ctx.args
    wl = WORKLOADS[name]
    PATTERN = (args.pattern if (args.pattern and name == args.workload) else wl[0])
    TAU = wl[1] if (args.distance is None or name != args.workload) else args.distance
    READ_LEN = (args.read_len if (args.read_len and name == args.workload) else wl[2])
    mode, want_name = wl[3], wl[4]
    L = READ_LEN + 1
    first = ctx.rank * n                                       # this rank's read-index range (weak scaling)
    nbytes = n * L
    stream = torch.cuda.current_stream().cuda_stream
    opt = {"best": dev.SQ_BEST, "first": 0, "all": dev.SQ_ALL}[mode]
    want = dev.WANT_RECORDS if want_name == "records" else dev.WANT_COUNTLINES
    mem_free0, mem_total = torch.cuda.mem_get_info(ctx.dev_index)
    pat = dev.Pattern(PATTERN, TAU)
    sc = dev.Scanner(stream)
    seg = int(os.environ.get("SEEQ_SEGMENT_BYTES", str(SEG_BYTES_DEFAULT)))
    seg_lines = min(n, seg // L + 2)
    rec_cap = n // 8 + 1024 if mode != "all" else n // 4 + 1024
    sc.reserve(nbytes, seg_lines + 64, max(seg_lines // 6 + 1024, 8192 * 64), rec_cap)
    sc.set_profiling(True)

    def synth(ptr):
        dev.synth_reads(ptr, first, n, READ_LEN, dev.plain_pattern(PATTERN), TAU, stream=stream)
        torch.cuda.synchronize()

    first_alloc = None
    if candidates > 1 and first_steps > 0 and not args.dry_run:
        # the plain allocation a caller that hipMallocs once gets -- this process's first buffer of the size
        tb0 = dev.TextBuffer(nbytes, 1)
        synth(tb0.ptr)
        for _ in range(2):
            sc.run(pat, tb0.ptr, nbytes, opt, want); sc.fetch()
        el0, a0, tot0, _ = timed_steps(ctx, sc, pat, tb0.ptr, nbytes, opt, want, first_steps, barrier=False)
        full0 = [x for i, x in enumerate(a0["launch_ms"]) if (i + 1) % max(1, a0["launches"] // first_steps) != 0 or a0["launches"] == first_steps]
        first_alloc = {"steps": first_steps, "ms_per_step": 1e3 * el0 / first_steps, "value": n / (el0 / first_steps),
                       "scan_launch_ms": round(a0["fwd_ms"] / max(1, a0["launches"]), 4), "scan_launch_ms_full_segments": stats3(full0),
                       "what": "the same text in a plain hipMalloc (seeqdevTextAlloc with one candidate), this rank only"}
        tb0.free()
    # (the candidates are probed with THIS scan context, reserved above: the launch time is a property of the pair text buffer / workspace)
    tb = dev.TextBuffer(nbytes, 1 if args.dry_run else candidates, scanner=sc)
    text = tb.tensor(ctx.device)
    if not args.dry_run:
        synth(tb.ptr)
    torch.cuda.synchronize()
    mem_free1, _ = torch.cuda.mem_get_info(ctx.dev_index)
    hbm = {"total_bytes": int(mem_total), "free_before_bytes": int(mem_free0), "text_bytes": int(nbytes), "text_allocated_bytes": tb.allocated_bytes,
           "text_workspace_records_bytes": int(mem_free0 - mem_free1), "free_after_bytes": int(mem_free1)}
    if args.dry_run:
        hbm["ranks"] = args.gpus
        hbm["fits"] = bool(mem_free1 > (1 << 30))               # a GiB to spare for the later sections' own buffers
        hbm["note"] = ("one rank's allocations (text + scan workspace reserved for its segments + record buffers), measured with hipMemGetInfo "
                       "around them; every rank of a multi-GPU run holds the same")
        return {"dry_run": True, "workload": wl[5] % n, "hbm_per_rank": hbm}, None
    placement = {"api": "seeqdevTextAllocFor", "candidates": candidates, "probed": len(tb.probe_ms), "chosen": tb.chosen,
                 "probe_forward_ms": [round(x, 3) for x in tb.probe_ms], "allocated_bytes": tb.allocated_bytes, "selected": len(tb.probe_ms) > 1}

    for _ in range(warmup):
        sc.run(pat, text.data_ptr(), nbytes, opt, want); sc.fetch()
    clocks = ClockSampler(ctx.dev_index) if (ctx.rank == 0 and args.log_clocks) else None
    if clocks:
        clocks.start()
    elapsed, acc, total, local = timed_steps(ctx, sc, pat, text.data_ptr(), nbytes, opt, want, steps, barrier=True)
    ctx.t_timed_end = time.perf_counter()
    if clocks:
        clocks.stop()
    own_elapsed = elapsed
    rank_rows = None
    if ctx.world > 1:
        dist = ctx.dist
        mine = torch.tensor([elapsed, float(first), float(n), float(local["nlines"]), float(local["nmatchlines"]),
                             acc["fwd_ms"] / max(1, steps), acc["ex_ms"] / max(1, steps), float(tb.chosen),
                             acc["fwd_ms"] / max(1, acc["launches"])], dtype=torch.float64, device=ctx.red_device)
        rows = [torch.zeros_like(mine) for _ in range(ctx.world)]
        dist.all_gather(rows, mine)
        rank_rows = [{"rank": r, "ms_per_step": 1e3 * float(x[0]) / steps, "first_read": int(x[1]), "reads": int(x[2]),
                      "lines": int(x[3]), "matching_lines": int(x[4]), "forward_scan_ms": float(x[5]),
                      "compaction_exact_records_ms": float(x[6]), "placement_chosen": int(x[7]), "scan_launch_ms": round(float(x[8]), 4)} for r, x in enumerate(rows)]
        t = torch.tensor([elapsed], dtype=torch.float64, device=ctx.red_device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # ---- parity (rank 0, outside the timed region): prefix + every 97th block + segment seams vs the oracle; every line vs the reference ----
    check = None
    rec = None
    if ctx.rank == 0 and check_lines > 0:
        blocks, seams = parity_blocks(n, READ_LEN, seg, check_lines)
        ranges = blocks + seams
        rec = sc.records(local["nrecords"]) if want == dev.WANT_RECORDS else None
        sc_chk = dev.Scanner(stream) if rec is None else None

        def scan_block(f0, cnt_):
            return sc_chk.scan_tensor(pat, text[f0 * L:(f0 + cnt_) * L], opt, want)
        tchk = time.perf_counter()
        lines_checked, nranges = oracle_check(text, ranges, READ_LEN, PATTERN, TAU, opt, rec is not None, rec, scan_block,
                                              procs=min(32, max(1, (os.cpu_count() or 2) - 1)))
        if rec is not None:       # size-independent properties of the whole record list
            assert np.all(np.diff(rec[:, 0].astype(np.int64)) >= (0 if mode == "all" else 1)), "records not ordered by line"
            assert np.all(rec[:, 1] <= rec[:, 2]) and np.all(rec[:, 2] <= READ_LEN) and np.all(rec[:, 3] <= TAU)
            assert len(np.unique(rec[:, 0])) == local["nmatchlines"]
        check = {"oracle_lines_checked": lines_checked, "ranges": nranges, "segment_seams_checked": len(seams),
                 "seconds": round(time.perf_counter() - tchk, 2), "result": "bit-exact"}
        if check_mode == "full":
            # the whole buffer against the reference itself (bit-exact match start / end / distance / count)
            full = reference_full_check(text, n, READ_LEN, PATTERN, TAU, "first" if want != dev.WANT_RECORDS else mode, rec, local["nmatchlines"])
            if full:
                check.update(full)

    sec = None
    if ctx.rank == 0:
        ms_per_step = 1e3 * elapsed / steps
        lines_total = total["nlines"]
        assert lines_total == n * ctx.world, (lines_total, n, ctx.world)
        value = lines_total / (elapsed / steps)
        # roofline of the dominant kernel (the scan kernel): algorithmic bytes per launch / mean launch time (HIP events on the scan's stream)
        launches_per_step = acc["launches"] / steps
        algo_bytes_launch = (n * L + 16 * local["nrecords"]) / launches_per_step + 8
        fwd_avg_ms = acc["fwd_ms"] / max(1, acc["launches"])
        achieved = algo_bytes_launch / (fwd_avg_ms * 1e-3) / 1e9
        kern = sc.last_kernel()
        filt = sc.last_filter()
        traffic, traffic_src = None, None
        pmc = os.path.join(ROOT, "profiles", "pmc_scan_kernels.json")
        if os.path.exists(pmc):
            try:
                pj = json.load(open(pmc)).get(kern)
                # HBM bytes per text byte measured with rocprofv3 PMC passes (profiles/), scaled to this launch size -- only when the kernel
                # sources are the ones it was measured on (else: null, the figure is not this build's)
                if pj and pj.get("source_hash") == source_hash():
                    traffic = pj["hbm_bytes_per_text_byte"] * (n * L / launches_per_step)
                    traffic_src = "profiles/pmc_scan_kernels.json (rocprofv3 --pmc passes, source hash %s) x this launch's text bytes" % pj["source_hash"]
                elif pj:
                    traffic_src = "none: profiles/pmc_scan_kernels.json was measured on other kernel sources (%s, now %s)" % (pj.get("source_hash"), source_hash())
            except Exception:
                traffic = None
        full_seg = [x for i, x in enumerate(acc["launch_ms"]) if (i + 1) % max(1, int(launches_per_step)) != 0 or launches_per_step == 1]
        sec = {
            "workload": wl[5] % n, "value": value, "gb_per_s": value * L / 1e9, "ms_per_step": ms_per_step, "steps": steps,
            "config": {"pattern": PATTERN, "distance": TAU, "read_len": READ_LEN, "reads_per_gpu": n},
            "device_ms_per_step": {"newline_index": round(acc["idx_ms"] / steps, 4), "forward_scan": round(acc["fwd_ms"] / steps, 4),
                                   "compaction_exact_records": round(acc["ex_ms"] / steps, 4)},
            "per_step": {"ms": stats3(acc["step_wall"]), "forward_scan_ms": stats3(acc["step_fwd"]), "post_pass_ms": stats3(acc["step_post"]),
                         "scan_launch_ms_full_segments": stats3(full_seg), "scan_kernel_core_clock_mhz": stats3(acc["clk"]),
                         "gpu_clock_power_during_steps": clocks.summary() if clocks else None},
            "hbm_per_rank": hbm, "placement": placement, "first_allocation": first_alloc, "ranks": rank_rows,
            "results": {"lines": lines_total, "matching_lines": total["nmatchlines"], "hits": total["nhits"],
                        "oracle_check": check, "oracle_lines_checked": check["oracle_lines_checked"] if check else 0},
            "roofline": {"bound": "hbm", "kernel": kern + (" (pair automaton: prefix / partition filter; candidates, verified by the exact pass)" if kern == "k_pair"
                                                           else " (partition filter automaton)" if filt else ""),
                         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                         "launches_per_step": launches_per_step, "avg_launch_ms": fwd_avg_ms, "algorithmic_bytes_per_launch": algo_bytes_launch,
                         "whole_step_frac": (n * L + 16 * local["nrecords"] + 8 * launches_per_step) / (own_elapsed / steps) / 1e9 / HBM_PEAK_GBS},
            "dtype": "int (u16 automaton state ids; exact-pass columns u32 bit-vectors)" if kern in ("k_stream", "k_pair") else "u32 bit-vectors",
        }
    live = {"text": text, "tb": tb, "sc": sc, "pat": pat, "rec": rec, "local": local, "total": total, "opt": opt, "want": want, "mode": mode,
            "PATTERN": PATTERN, "TAU": TAU, "READ_LEN": READ_LEN, "rec_cap": rec_cap, "stream": stream}
    if not keep:
        sc.close(); pat.close()
        del text
        tb.free()
        live = None
    return sec, live


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true",
                    help="everything besides the headline: the oracle sample and the comparison with the reference binary (--check, --check-lines), "
                         "the plain first allocation (--first-steps), the single-GPU sections (--sections and the --no-* switches); for --workload "
                         "chrom the oracle sample and the reference binary over the same bytes.  Without it a run sets up, warms up, times the "
                         "steps, writes --dump-outputs and prints its line")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reads", type=int, default=100_000_000, help="reads per GPU")
    ap.add_argument("--workload", choices=sorted(WORKLOADS) + ["chrom"], default="best")
    ap.add_argument("--pattern", default=None, help="non-default patterns are for experiments (config names them)")
    ap.add_argument("--distance", type=int, default=None)
    ap.add_argument("--read-len", type=int, default=None)
    ap.add_argument("--sections", choices=["auto", "all", "none"], default="auto",
                    help="with --full, the single-GPU sections behind the timed steps (full check against the reference, pinned-host end to end, packed batch, "
                         "FASTQ shape, multi-pattern, per call, CPU baseline + regions + CLI, configs[4]): auto = all of them on one GPU, none of them under "
                         "--gpus N > 1 (ranks 1 .. N-1 would only wait for rank 0); none: none of them on one GPU either; all: under N > 1 rank 0 "
                         "runs the --check mode of one GPU")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-e2e", action="store_true", help="skip the host-memory end-to-end measurement")
    ap.add_argument("--no-per-call", action="store_true", help="skip the seeqStringMatch per-call measurement")
    ap.add_argument("--no-packed", action="store_true", help="skip the packed-batch scan of the same reads")
    ap.add_argument("--no-cli", action="store_true", help="skip the CLI wall-clock measurement (timed region iii)")
    ap.add_argument("--no-multi", action="store_true", help="skip the sixteen-barcode multi-pattern measurement")
    ap.add_argument("--no-fastq", action="store_true", help="skip the FASTQ-shaped text section (shape Q of SURVEY 8d)")
    ap.add_argument("--no-cfg5", action="store_true", help="skip the BASELINE configs[4] section of the default run")
    ap.add_argument("--fastq-records", type=int, default=25_000_000, help="four-line records of the FASTQ section (25 M = 100 M lines, 7.9 GB)")
    ap.add_argument("--cfg5-reads", type=int, default=100_000_000, help="reads of the configs[4] section (its stated size: 100 M x 250 bp)")
    ap.add_argument("--cpu-sample", type=int, default=4_000_000)
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise torch.distributed (nccl = RCCL) even at world size 1 and run the step's collectives over it "
                         "(start it under torch.distributed.run --nproc-per-node 1, or alone: the rendezvous variables are set here)")
    ap.add_argument("--dry-run", action="store_true",
                    help="allocate ONE rank's text, workspace and record buffers, print what it needs of the GPU's memory "
                         "(per rank of --gpus N: every rank holds the same) and exit -- no scan, no launcher")
    ap.add_argument("--placement-candidates", type=int, default=12,
                    help="candidates the PRODUCT's allocator (seeqdevTextAllocFor) probes for the resident text: the plain allocation, then power-of-two "
                         "blocks; the fastest is kept (k_pair's launch time follows the physical pages a buffer gets: DESIGN.md section 5).  The plain "
                         "first allocation's figure is reported beside `value` as `first_allocation` (--full); 1 = the plain allocation only; capped at 4 per rank "
                         "under --gpus N > 1")
    ap.add_argument("--first-steps", type=int, default=20, help="with --full, timed steps over the plain first allocation (`first_allocation`)")
    ap.add_argument("--log-clocks", action="store_true", help="sample the GPU's clock / power from sysfs during the timed steps (a thread)")
    ap.add_argument("--check", choices=["full", "sample"], default="full",
                    help="with --full: full (default on one GPU when oracle/_ref/seeq_ref exists): besides the oracle sample, EVERY line of the run is "
                         "compared with the reference binary's output, outside the timed region; sample: the oracle sample only")
    ap.add_argument("--check-lines", type=int, default=1_000_000,
                    help="with --full, prefix verified against the oracle (plus every 97th 64 Ki-line block and the segment seams); 0 = no check")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (counts; records, or a seeded sample of at most "
                         "%d of them) as float64 .npy files under DIR (rank 0)" % DUMP_MAX_RECORDS)
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def run_plan(args, world, rank):
    """What a run does besides setting up, warming up and timing its steps.  A plain run: nothing but --dump-outputs.  --full: the plain
    first allocation and the single-GPU sections (one GPU), the oracle / reference checks (rank 0)."""
    sections = args.sections if args.sections != "auto" else ("all" if world == 1 else "none")
    return {
        "extra": args.full and sections == "all" and rank == 0 and world == 1,    # (the sections run on one GPU: under N ranks the others would only wait)
        "first_steps": args.first_steps if (args.full and world == 1) else 0,
        "check_lines": args.check_lines if args.full else 0,
        "check_mode": args.check if (world == 1 or sections == "all") else "sample",
        "candidates": args.placement_candidates if world == 1 else min(4, args.placement_candidates),
    }


def main():
    args = parse_args()
    if args.workload == "chrom":
        if args.gpus != 1:
            sys.exit("bench.py: --workload chrom runs on one GPU")
        return bench_chrom(args)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1 and not args.dry_run:
        sys.exit(launch_ranks(args))

    import numpy as np
    import torch
    import torch.distributed as dist
    from seeq_amd import device as dev
    from seeq_amd import shard

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and not args.dry_run:
        sys.stderr.write("bench.py: --gpus %d but WORLD_SIZE=%d\n" % (args.gpus, world))
        sys.exit(2)
    share = os.environ.get("SEEQ_BENCH_SHARE_GPU") == "1"
    dev_index = 0 if share else local_rank
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    dist_info = None
    if world == 1 and args.force_dist and not args.dry_run:
        # the RCCL rehearsal: the same process group, all-reduce and all-gather the multi-GPU line uses, over one rank
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("nccl", device_id=device)         # RCCL
        ones = torch.ones(1, dtype=torch.int64, device=device)
        dist.all_reduce(ones, op=dist.ReduceOp.SUM)
        gathered = [torch.zeros(1, dtype=torch.int64, device=device)]
        dist.all_gather(gathered, torch.full((1,), 7, dtype=torch.int64, device=device))
        torch.cuda.synchronize()
        dist_info = {"backend": dist.get_backend(), "world": dist.get_world_size(), "all_reduce_of_ones": int(ones.item()),
                     "all_gather_ok": int(gathered[0].item()) == 7}
        if dist_info["all_reduce_of_ones"] != 1 or not dist_info["all_gather_ok"]:
            sys.stderr.write("bench.py: the RCCL collectives over one rank returned %r\n" % (dist_info,))
            sys.exit(3)
    if world > 1 and not args.dry_run:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)     # RCCL
        # every rank must have joined: a sum of ones over the collective the step uses
        ones = torch.ones(1, dtype=torch.int64, device="cpu" if share else device)
        dist.all_reduce(ones, op=dist.ReduceOp.SUM)
        if int(ones.item()) != args.gpus:
            sys.stderr.write("bench.py: %d ranks joined the all-reduce, expected %d\n" % (int(ones.item()), args.gpus))
            sys.exit(3)
        dist_info = {"backend": dist.get_backend(), "world": dist.get_world_size(), "ranks_joined": int(ones.item())}

    ctx = Ctx()
    ctx.args, ctx.torch, ctx.np, ctx.dist, ctx.dev, ctx.shard = args, torch, np, dist, dev, shard
    ctx.world, ctx.rank, ctx.device, ctx.dev_index = world, rank, device, dev_index
    ctx.red_device = "cpu" if (share and world > 1) else device
    ctx.force_dist = world == 1 and args.force_dist and not args.dry_run
    plan = run_plan(args, world, rank)
    extra, candidates, check_mode = plan["extra"], plan["candidates"], plan["check_mode"]
    t_start = time.perf_counter()

    n = args.reads
    sec, live = run_workload(ctx, args.workload, n, args.steps, args.warmup, candidates, plan["first_steps"],
                             plan["check_lines"], check_mode, keep=True)
    if args.dry_run:
        print(json.dumps(sec))
        return
    if rank == 0 and args.dump_outputs:
        rec = live["rec"]
        if rec is None and live["want"] == dev.WANT_RECORDS:
            rec = live["sc"].records(live["local"]["nrecords"])
        dump_outputs(args.dump_outputs, dict(live["local"], **live["total"]), rec)     # (the all-reduced counts over this rank's)
    if ctx.force_dist:      # the all-gather of the global line numbering (seeq.c:377) through the shard layer, over RCCL
        dist_info["line_base_of_rank0"] = shard.line_base(live["local"]["nlines"], device=device, force=True)
        dist_info["count_reduce_per_step"] = "all_reduce of (lines, matching lines, hits) over RCCL inside every timed step"
    t_steps_done = ctx.t_timed_end

    if rank == 0:
        text, sc, pat, local, opt, want, mode = live["text"], live["sc"], live["pat"], live["local"], live["opt"], live["want"], live["mode"]
        PATTERN, TAU, READ_LEN, rec_cap, stream = live["PATTERN"], live["TAU"], live["READ_LEN"], live["rec_cap"], live["stream"]
        value = sec["value"]
        out = {
            "metric": "lines/s scanned (20 bp pattern, d=3, 150 bp reads; GB/s in gb_per_s)" if args.workload != "cfg5" else
                      "lines/s scanned (40-position class/N pattern, d=5, 250 bp reads, --all; GB/s in gb_per_s)",
            "value": value, "unit": "lines/s", "gb_per_s": sec["gb_per_s"],
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": sec["ms_per_step"],
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": sec["dtype"], "data": "synthetic",
            "config": dict(sec["config"], workload=sec["workload"], parallelism="line-sharded x%d, RCCL count all-reduce" % world),
            "dist": dist_info, "hbm_per_rank": sec["hbm_per_rank"], "device_ms_per_step": sec["device_ms_per_step"], "per_step": sec["per_step"],
        }
        if sec["ranks"] is not None:
            out["ranks"] = sec["ranks"]
            out["slowest_rank"] = max(sec["ranks"], key=lambda r: r["ms_per_step"])
        if extra and not args.no_e2e:
            # Timed region (ii) of SURVEY 8d: same path fed from page-locked HOST memory (H2D + scan + D2H of the
            # records), on a 10 M-line sample.  PCIe-bound; reported beside, never as, `value`.
            ne = min(n, 10_000_000)
            hostbuf = text[:ne * (READ_LEN + 1)].cpu().pin_memory()
            sc2 = dev.Scanner()
            best = None
            for _ in range(3):
                t1 = time.perf_counter()
                cnt2 = seeq_scan_host_ptr(sc2, pat, hostbuf.data_ptr(), hostbuf.numel(), opt, want)
                if want == dev.WANT_RECORDS:
                    sc2.records(cnt2["nrecords"])
                dt = time.perf_counter() - t1
                best = dt if best is None else min(best, dt)
            out["end_to_end_pinned_host"] = {"lines": ne, "seconds": best, "lines_per_s": ne / best, "gb_per_s": ne * (READ_LEN + 1) / best / 1e9,
                                             "note": "H2D over PCIe + scan + D2H records; best of 3"}
            sc2.close()
            del hostbuf
        if extra and not args.no_packed and READ_LEN <= 256:
            # The same reads as a PACKED batch (2 bits per base + an N mask: seeq_amd.h seeqdev_packed_t; SURVEY 8d allows a scan-only
            # figure on pre-packed data beside the headline): packed on the device here, scanned from HBM, every count and every record
            # compared with the ASCII run's; then timed region (ii) again with the packed bytes coming from page-locked host memory.
            try:
                stride, nstride = (READ_LEN + 3) // 4, (READ_LEN + 7) // 8
                pb = torch.empty(n * stride, dtype=torch.uint8, device=device)
                pn = torch.empty(n * nstride, dtype=torch.uint8, device=device)
                dev.pack_reads_device(text.data_ptr(), n, READ_LEN, pb.data_ptr(), pn.data_ptr(), stream=stream)
                torch.cuda.synchronize()
                scp = dev.Scanner(stream)
                scp.reserve(0, 0, max(n // 6 + 1024, 8192 * 64), rec_cap)
                scp.set_profiling(True)
                for _ in range(2):
                    scp.run_packed(pat, pb.data_ptr(), pn.data_ptr(), n, READ_LEN, options=opt, want=want)
                    pc = scp.fetch()
                torch.cuda.synchronize()
                tp0 = time.perf_counter()
                psteps = max(3, min(50, args.steps // 2))
                pfwd = 0.0
                plaunch = 0
                for _ in range(psteps):
                    scp.run_packed(pat, pb.data_ptr(), pn.data_ptr(), n, READ_LEN, options=opt, want=want)
                    pc = scp.fetch()
                    tm = scp.last_times_ms()
                    pfwd += tm["forward"]
                    plaunch += tm["forward_launches"]
                torch.cuda.synchronize()
                pel = (time.perf_counter() - tp0) / psteps
                same = all(pc[k] == local[k] for k in ("nlines", "nmatchlines", "nhits", "nrecords"))
                if want == dev.WANT_RECORDS and same:
                    same = bool(np.array_equal(scp.records(pc["nrecords"]), sc.records(local["nrecords"])))
                pbytes = n * (stride + nstride)
                out["packed_scan"] = {"lines_per_s": n / pel, "ms_per_step": pel * 1e3, "bytes_per_read": stride + nstride,
                                      "packed_gb_per_s": pbytes / pel / 1e9, "ascii_equivalent_gb_per_s": n * (READ_LEN + 1) / pel / 1e9,
                                      "scan_kernel_ms_per_launch": pfwd / max(1, plaunch), "scan_kernel_launches_per_step": plaunch / psteps,
                                      "scan_kernel_hbm_frac": (pbytes / (plaunch / psteps)) / (pfwd / max(1, plaunch) * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                      "identical_to_ascii_run": same,
                                      "walk_table": "quad (four bases per gather, two-part filter)" if scp.last_packed_quad() else "pair (two bases per gather)"}
                if not args.no_e2e:
                    ne = min(n, 10_000_000)
                    hb = pb[:ne * stride].cpu().pin_memory()
                    hn = pn[:ne * nstride].cpu().pin_memory()
                    db = torch.empty_like(pb[:ne * stride])
                    dn = torch.empty_like(pn[:ne * nstride])
                    sc3 = dev.Scanner(stream)
                    best = None
                    for _ in range(3):
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        db.copy_(hb, non_blocking=True)
                        dn.copy_(hn, non_blocking=True)
                        sc3.run_packed(pat, db.data_ptr(), dn.data_ptr(), ne, READ_LEN, options=opt, want=want)
                        c3 = sc3.fetch()
                        if want == dev.WANT_RECORDS:
                            sc3.records(c3["nrecords"])
                        dt = time.perf_counter() - t1
                        best = dt if best is None else min(best, dt)
                    out["end_to_end_pinned_host_packed"] = {"lines": ne, "seconds": best, "lines_per_s": ne / best,
                                                            "packed_gb_per_s": ne * (stride + nstride) / best / 1e9,
                                                            "note": "packed bases + N mask from page-locked host memory: H2D + scan + D2H records; best of 3"}
                    sc3.close()
                    del hb, hn, db, dn
                scp.close()
                del pb, pn
            except Exception as e:                      # (reported, not fatal: the ASCII line above is the graded one)
                out["packed_scan"] = {"error": str(e)}
        if extra and not args.no_multi and args.workload in ("best", "count", "all"):
            # Sixteen barcodes over the first 10 M reads of the buffer (row f4b, seeq_multi.h): ONE walk for the set against a scan per
            # pattern (SEEQ_MULTI=sequential) -- the set holds three windows of the planted pattern and thirteen random 10-mers, d = 1;
            # counts and (for the records run) every record of every pattern compared between the two paths.
            try:
                import random as _random
                rng_ = _random.Random(2025)
                m_plain = dev.plain_pattern(PATTERN)
                m_names = [m_plain[i:i + 10] for i in (0, 5, 10) if len(m_plain) >= i + 10]
                while len(m_names) < 16:
                    m_names.append("".join(rng_.choice("ACGT") for _ in range(10)))
                mp = [dev.Pattern(b, 1) for b in m_names]
                m_nm = min(n, 10_000_000)
                m_sub = text[:m_nm * (READ_LEN + 1)]
                scm = dev.Scanner(stream)
                m_res = {}
                for m_mode in ("one_walk", "per_pattern"):
                    if m_mode == "per_pattern":
                        os.environ["SEEQ_MULTI"] = "sequential"
                    else:
                        os.environ.pop("SEEQ_MULTI", None)
                    for m_wname, o_, w_ in (("count_lines", 0, dev.WANT_COUNTLINES), ("best_records", dev.SQ_BEST, dev.WANT_RECORDS)):
                        m_best = None
                        for m_it in range(3):
                            torch.cuda.synchronize()
                            m_t1 = time.perf_counter()
                            m_got = scm.scan_tensor_multi(mp, m_sub, o_, w_, copy=False)
                            m_dt = time.perf_counter() - m_t1
                            if m_it:
                                m_best = m_dt if m_best is None else min(m_best, m_dt)
                        m_res[(m_mode, m_wname)] = (m_best, scm.last_multi_one_pass(), [g["nmatchlines"] for g in m_got],
                                                    [g["records"].copy() for g in m_got] if w_ == dev.WANT_RECORDS else None)
                os.environ.pop("SEEQ_MULTI", None)
                m_sec = {"patterns": 16, "pattern_len": 10, "distance": 1, "lines": m_nm}
                for m_wname in ("count_lines", "best_records"):
                    a_, b_ = m_res[("one_walk", m_wname)], m_res[("per_pattern", m_wname)]
                    m_same = a_[2] == b_[2] and (a_[3] is None or all(np.array_equal(x, y) for x, y in zip(a_[3], b_[3])))
                    m_sec[m_wname] = {"one_walk_ms": a_[0] * 1e3, "per_pattern_ms": b_[0] * 1e3, "speedup": b_[0] / a_[0], "one_walk_ran": bool(a_[1]),
                                      "matching_line_pattern_pairs": int(sum(a_[2])), "identical_results": bool(m_same)}
                out["multi_pattern"] = m_sec
                scm.close()
                for p_ in mp:
                    p_.close()
            except Exception as e:
                out["multi_pattern"] = {"error": str(e)}
        if extra and not args.no_per_call:
            out["per_call"] = per_call_rates(PATTERN, TAU, READ_LEN)
        fq = None
        if extra and not args.no_fastq and args.workload in ("best", "count", "all"):
            # Shape Q (the north star's "FASTQ-shaped reads"): the first 25 M reads as four-line FASTQ records ("@r<id>", read, "+", 150
            # Phred+33 bytes that alias onto the alphabet and onto the newline column: libseeq.c:265-270) = 100 M lines, 7.9 GB, several
            # scan-kernel launches, scanned as plain lines under the reference's three non-DNA modes (-x 0 / 1 / 2), --best with positions; the
            # matching-line count of the WHOLE buffer against the reference binary's (seeq -c -x <mode>), the records of a 200 k-line prefix
            # against the oracle.
            try:
                fq = fastq_shape(text, min(n, args.fastq_records), READ_LEN, PATTERN, TAU, pat)
            except Exception as e:                      # (reported, not fatal)
                fq = {"error": repr(e)}
        regions = None
        if extra and not args.no_cpu_baseline:
            sample = args.cpu_sample if args.workload != "cfg5" else max(200_000, args.cpu_sample // 4)
            out["cpu_baseline"] = cpu_baseline(sample, PATTERN, TAU, READ_LEN, mode)
            cpu = out["cpu_baseline"]["value"]
            out["gpu_over_cpu"] = value / cpu
            # the three timed regions, each against the P-core CPU aggregate (region iii: one reference process, what a user of
            # the CLI runs) and against the whole-socket estimate, and whether the north star's 10x holds for it (README: where 10x holds)
            est = out["cpu_baseline"].get("whole_socket_estimate_lines_per_s") or cpu

            def region(lps, **kw):
                return dict({"lines_per_s": lps, "gpu_over_cpu": lps / cpu, "over_whole_socket_estimate": lps / est, "meets_10x": lps / cpu >= 10.0,
                             "meets_10x_whole_socket_estimate": lps / est >= 10.0}, **kw)
            regions = {"cpu": {"measured_processes": out["cpu_baseline"]["cores"], "measured_lines_per_s": cpu, "whole_socket_estimate_lines_per_s": est},
                       "device_resident": region(value)}
            if "end_to_end_pinned_host_packed" in out:
                regions["end_to_end_pinned_host_packed"] = region(out["end_to_end_pinned_host_packed"]["lines_per_s"], bytes_per_read_over_the_link=57)
            if "end_to_end_pinned_host" in out:
                e2e = out["end_to_end_pinned_host"]
                regions["end_to_end_pinned_host"] = region(e2e["lines_per_s"], bytes_per_read_over_the_link=READ_LEN + 1,
                                                           link_gb_per_s=e2e["gb_per_s"], note="one PCIe link per GPU: ASCII text at ~55 GB/s caps this region near 0.37 G lines/s; SEEQ_DEVICES spreads a file's chunks over several GPUs (links)")
            if not args.no_cli and args.workload in ("best", "count", "all"):
                cw = cli_wall_clock(PATTERN, TAU, READ_LEN)
                out["cli_wall_clock"] = cw
                if cw.get("gpu_lines_per_s"):
                    r1 = cw["gpu_lines_per_s"] / cw["reference_lines_per_s_one_core"] if cw.get("reference_lines_per_s_one_core") else None
                    regions["cli_wall_clock"] = region(cw["gpu_lines_per_s"], over_one_reference_process=r1,
                                                       note="10 M-line file, page-cache warm; includes process start and HIP start-up (0.25-0.35 s of it)")
        # ---- BASELINE configs[4] at its stated size, as a section of the default line (the headline's buffers are released first) ----
        cfg5 = None
        if extra and not args.no_cfg5 and args.workload == "best":
            sc.close(); pat.close()
            del text
            live["tb"].free()
            live = None
            torch.cuda.empty_cache()
            try:
                c5, _ = run_workload(ctx, "cfg5", args.cfg5_reads, 3, 2, min(4, candidates), 0, plan["check_lines"], check_mode, keep=False)
                cfg5 = {k: c5[k] for k in ("workload", "value", "gb_per_s", "ms_per_step", "steps", "device_ms_per_step", "placement", "results", "roofline")}
                cfg5["whole_step_frac"] = c5["roofline"]["whole_step_frac"]
            except Exception as e:                      # (reported, not fatal: the headline above is the graded line)
                cfg5 = {"error": repr(e)}
        # ---- the tail of the line: what the driver's record keeps (its last 8 KB) ----
        if fq is not None:
            out["fastq_shape"] = fq
        if regions is not None:
            out["regions"] = regions
        if cfg5 is not None:
            out["cfg5"] = cfg5
        out["seconds"] = {"to_end_of_timed_steps": round(t_steps_done - t_start, 1), "sections_after": round(time.perf_counter() - t_steps_done, 1)}
        out["placement"] = sec["placement"]
        out["first_allocation"] = sec["first_allocation"]
        out["results"] = sec["results"]
        out["roofline"] = sec["roofline"]
        print(json.dumps(out))
        sys.stdout.flush()
    if world > 1:
        # every rank waits here for rank 0's line, says so, and leaves together
        dist.barrier()
        sys.stderr.write("bench.py: rank %d of %d done %.1f s after its timed steps; leaving the process group\n" % (rank, world, time.perf_counter() - t_steps_done))
        dist.destroy_process_group()
    elif dist_info is not None and dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
