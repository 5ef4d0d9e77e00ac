"""Batched device-level scans (include/seeq_amd.h) for Python callers.

`Pattern` is a compiled pattern living in HBM; `Scanner` owns a HIP stream +
workspace and runs the whole per-file hot path over a text buffer that is
already in HBM (a torch uint8 CUDA tensor, or any device pointer).
torch is used only for memory and streams; all compute is in libseeq_amd.so.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import (SQ_ALL, SQ_BEST, SQ_CONVERT, SQ_FAIL, SQ_FIRST, SQ_IGNORE, SEEQDEV_FASTA, SEEQDEV_FASTQ,  # noqa: F401
                    WANT_COUNTLINES, WANT_COUNTMATCH, WANT_RECORDS)


class SeeqDeviceError(RuntimeError):
    pass


def _check(rc):
    if rc != 0:
        raise SeeqDeviceError(_capi.error_text())


def pack_reads(text, read_len, with_nmask=True):
    """ASCII reads (bytes, one per line, each exactly read_len bases) -> (bases, nmask, nreads): numpy uint8 arrays in the
    packed layout of seeq_amd.h (stride ceil(read_len / 4), nstride ceil(read_len / 8)); nmask is None without with_nmask."""
    stride, nstride = (read_len + 3) // 4, (read_len + 7) // 8
    nmax = len(text) // read_len + 1
    bases = np.zeros(nmax * stride, dtype=np.uint8)
    nmask = np.zeros(nmax * nstride, dtype=np.uint8) if with_nmask else None
    n = _capi.lib().seeqdevPackReads(text, len(text), read_len, bases.ctypes.data, nmask.ctypes.data if with_nmask else None, stride, nstride)
    if n < 0:
        raise SeeqDeviceError("seeqdevPackReads: a line of another length, or a byte that is not A C G T U N")
    return bases[:n * stride], (nmask[:n * nstride] if with_nmask else None), int(n)


class TextBuffer:
    """Device memory for resident text chosen by measurement (seeqdevTextAllocInfo): the scan kernel's speed follows the physical pages a
    buffer gets, so up to `candidates` allocations are probed and the fastest kept.  `ptr` is the device address, `probe_ms` the candidates'
    scan-kernel times (empty when nothing was probed; candidate 0 is the plain allocation), `chosen` the index of the one kept,
    `allocated_bytes` the size of the allocation behind it (a power-of-two block may be up to twice `nbytes`), `probe_peak_bytes` what the
    call held on the device at its peak.  Contents undefined; free() or the garbage collector releases it.  `tensor()`: a torch uint8
    view of the first `nbytes` bytes (plumbing for callers that slice / copy with torch; the buffer must outlive the view)."""

    def __init__(self, nbytes, candidates=12, scanner=None):
        """scanner: the Scanner that will scan the text (seeqdevTextAllocFor: the candidates are probed with ITS workspace -- reserve() it first);
        None: a context made for the probe."""
        info = _capi.seeqdev_textinfo_t()
        if scanner is not None:
            p = _capi.lib().seeqdevTextAllocFor(scanner._h, int(nbytes), int(candidates), C.byref(info))
        else:
            p = _capi.lib().seeqdevTextAllocInfo(int(nbytes), int(candidates), C.byref(info))
        if not p:
            raise SeeqDeviceError(_capi.error_text())
        self.ptr, self.nbytes = int(p), int(nbytes)
        self.probe_ms = [float(info.probe_ms[i]) for i in range(info.nprobed)]
        self.chosen = int(info.chosen)
        self.allocated_bytes = int(info.allocated_bytes)
        self.probe_peak_bytes = int(info.probe_peak_bytes)

    @property
    def __cuda_array_interface__(self):
        return {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 2, "strides": None}

    def tensor(self, device=None):
        import torch
        return torch.as_tensor(self, device=device if device is not None else "cuda")

    def free(self):
        if self.ptr:
            _capi.lib().seeqdevTextFree(C.c_void_p(self.ptr))
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def pack_reads_device(text_ptr, nreads, read_len, bases_ptr, nmask_ptr=None, stream=None):
    """ASCII reads in HBM (nreads lines of read_len bases + newline) -> the packed layout in HBM (device pointers)."""
    _check(_capi.lib().seeqdevPackReadsDevice(C.c_void_p(text_ptr), nreads, read_len, C.c_void_p(bases_ptr), C.c_void_p(nmask_ptr) if nmask_ptr else None,
                                              (read_len + 3) // 4, (read_len + 7) // 8, C.c_void_p(stream) if stream else None))


def device_count():
    return _capi.lib().seeqdevDeviceCount()


def plain_pattern(pattern):
    """One concrete base per pattern position (first member of a class, 'A' for N):
    the string the synthetic-read generator plants."""
    out, i = [], 0
    while i < len(pattern):
        c = pattern[i]
        if c == '[':
            j = pattern.index(']', i)
            if j > i + 1:
                out.append(pattern[i + 1].upper().replace('U', 'T').replace('N', 'A'))
            i = j + 1
        else:
            out.append('A' if c in 'Nn' else c.upper().replace('U', 'T'))
            i += 1
    return ''.join(out)


_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "U": "A", "N": "N", "a": "t", "c": "g", "g": "c", "t": "a", "u": "a", "n": "n"}


def revcomp_pattern(pattern):
    """The reverse complement of a pattern EXPRESSION: the tokens (a base, N, or a bracket class) in reverse order, every base
    complemented -- a class member by member, so [AC] becomes [GT] and [] stays [].  U is read as T (its complement is A, and the
    complement of A is written T); N stays N; case is preserved.  Compiles to the key bytes seeqdevPatternRevComp makes of the
    compiled pattern."""
    tokens, i = [], 0
    try:
        while i < len(pattern):
            if pattern[i] == "[":
                j = pattern.index("]", i)
                tokens.append("[" + "".join(_COMPLEMENT[c] for c in pattern[i + 1:j]) + "]")
                i = j + 1
            else:
                tokens.append(_COMPLEMENT[pattern[i]])
                i += 1
    except (KeyError, ValueError):
        raise ValueError("not a pattern expression: %r" % (pattern,))
    return "".join(reversed(tokens))


class Pattern:
    def __init__(self, pattern, tau):
        self._lib = _capi.lib()
        self.pattern, self.tau = pattern, tau
        self._sq = self._lib.seeqNew(pattern.encode(), int(tau), 0)
        if not self._sq:
            raise SeeqDeviceError("seeqNew(%r, %d): %s" % (pattern, tau, _capi.error_text()))
        self.wlen = self._sq.contents.wlen
        self.handle = self._lib.seeqdevPatternOf(self._sq)

    def close(self):
        sq, self._sq = self._sq, None
        if sq:
            self._lib.seeqFree(sq)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def revcomp(self):
        """The reverse complement as a pattern of its own (seeqdevPatternRevComp: same device, same tau), usable wherever a Pattern
        is -- a barcode set with both orientations of every member, for one."""
        return RevCompPattern(self)


class RevCompPattern:
    """What Pattern.revcomp() returns: `handle`, `pattern` (the expression, revcomp_pattern of the original's), `tau`, `wlen`;
    close() frees it.  It does not depend on the Pattern it was made from."""

    def __init__(self, of):
        self._lib = _capi.lib()
        self.pattern, self.tau, self.wlen = revcomp_pattern(of.pattern), of.tau, of.wlen
        self.handle = self._lib.seeqdevPatternRevComp(of.handle)
        if not self.handle:
            raise SeeqDeviceError("seeqdevPatternRevComp(%r): %s" % (of.pattern, _capi.error_text()))

    def close(self):
        h, self.handle = self.handle, None
        if h:
            self._lib.seeqdevPatternFree(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# the sixteen numbers of seeqdevScanLastPlan (and of tests/host_harness.cpp: harness_plan), in order
PLAN_FIELDS = ("rc", "path", "fw", "use_stream", "use_pair", "use_myers", "filter", "stream_ll", "stream_sub", "stream_wu", "verify", "order2",
               "leaders", "window_ok", "ll_filter", "skip_back")

# the names of the record arrays the tally entries take as `source` (seeq_amd.h); the holds and the append take a demultiplex too
_SPAN_SOURCES = {"inserts": _capi.SEEQDEV_TALLY_INSERTS, "hits": _capi.SEEQDEV_TALLY_HITS, "gated": _capi.SEEQDEV_TALLY_GATED,
                 "anchored": _capi.SEEQDEV_TALLY_ANCHORED}
_HOLD_SOURCES = dict(_SPAN_SOURCES, demux=_capi.SEEQDEV_TALLY_DEMUX)
_ANCHORS = {"after": _capi.SEEQDEV_ANCHOR_AFTER, "before": _capi.SEEQDEV_ANCHOR_BEFORE, "line": _capi.SEEQDEV_ANCHOR_LINE}


class Scanner:
    def __init__(self, stream=None):
        """stream: a hipStream_t as int (e.g. torch.cuda.current_stream().cuda_stream) or None.  None and 0 (torch's
        default stream is the legacy null stream, handle 0) both give the scanner a private stream of the default,
        "blocking" kind: HIP orders it after work already queued on the null stream and the null stream after it."""
        self._lib = _capi.lib()
        self._h = self._lib.seeqdevScanNew(C.c_void_p(stream) if stream else None)
        if not self._h:
            raise SeeqDeviceError("seeqdevScanNew: " + _capi.error_text())

    def close(self):
        h, self._h = self._h, None
        if h:
            self._lib.seeqdevScanFree(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, max_bytes=0, max_lines=0, max_hitlines=0, max_records=0):
        _check(self._lib.seeqdevScanReserve(self._h, max_bytes, max_lines, max_hitlines, max_records))

    def set_profiling(self, on=True):
        _check(self._lib.seeqdevScanSetProfiling(self._h, 1 if on else 0))

    def set_line_hint(self, avg_bytes_per_line):
        _check(self._lib.seeqdevScanSetLineHint(self._h, float(avg_bytes_per_line)))

    def last_path(self):
        return {1: "generic", 3: "fused", 5: "fused", 6: "fused", 7: "fused", 8: "packed"}.get(self._lib.seeqdevScanLastPath(self._h), "none")

    def last_kernel(self):
        return {1: "k_forward", 3: "k_direct", 5: "k_stream", 6: "k_pair", 7: "k_myers", 8: "k_packed"}.get(self._lib.seeqdevScanLastPath(self._h), "none")

    def last_filter(self):
        """True when the last k_stream run walked a partition filter automaton (candidates verified by the exact pass)."""
        return bool(self._lib.seeqdevScanLastFilter(self._h))

    def last_plan(self):
        """The plan the last run executed (seeqdevScanLastPlan) as a dict over PLAN_FIELDS: the scan kernel's instance and the post-pass
        behind it; after a fall-back re-run, the re-run's."""
        out = (C.c_int * 16)()
        _check(self._lib.seeqdevScanLastPlan(self._h, out))
        return dict(zip(PLAN_FIELDS, (int(v) for v in out)))

    def last_packed_quad(self):
        """True when the last packed run walked the quad table (four bases per table step)."""
        return bool(self._lib.seeqdevScanLastPackedQuad(self._h))

    def last_runs(self):
        """Runs the last completed scan took (1: no re-run; of a multi, demux or both-strands call: those of its last scan or walk)."""
        return int(self._lib.seeqdevScanLastRuns(self._h))

    def fallback(self):
        """(bits, scans_left): the fall-back flags the context remembers of earlier texts (FALLBACK_* below; 0: none) and the scans
        they stay in force for."""
        bits, left = C.c_uint(0), C.c_int(0)
        _check(self._lib.seeqdevScanFallback(self._h, C.byref(bits), C.byref(left)))
        return int(bits.value), int(left.value)

    def last_times_ms(self):
        ms = (C.c_float * 4)()
        _check(self._lib.seeqdevScanLastTimes(self._h, ms))
        return dict(index=ms[0], forward=ms[1], exact=ms[2], total=ms[3],
                    forward_launches=self._lib.seeqdevScanLastLaunches(self._h))

    def last_clock_mhz(self):
        """Core clock the last run's scan launches ran at (k_pair's own clock readings; profiling on), 0 when not measured."""
        return float(self._lib.seeqdevScanLastClockMHz(self._h))

    def last_launch_times_ms(self):
        """Duration of every forward-scan launch of the last fetched scan (profiling on), in launch order."""
        n = self._lib.seeqdevScanLastLaunches(self._h)
        ms = (C.c_float * max(1, n))()
        got = self._lib.seeqdevScanLastLaunchTimes(self._h, ms, n)
        return [float(ms[i]) for i in range(max(0, min(got, n)))]

    def run(self, pattern, d_ptr, nbytes, options=0, want=WANT_COUNTLINES):
        """Enqueue the scan (asynchronous).  options: libseeq.h bits | SEEQDEV_FASTA | SEEQDEV_FASTQ -- with SEEQDEV_FASTQ the buffer is
        four-line FASTQ records taken by position, and everything fetch() / records() / record_offsets() report is that of a scan of the
        sequence lines alone: `line` is the 1-based record number, nlines counts records; record_offsets() are offsets of the
        sequence lines in THIS buffer (seeq_amd.h)."""
        _check(self._lib.seeqdevScanRun(self._h, pattern.handle, C.c_void_p(d_ptr), nbytes, options, want))

    def fetch(self):
        cnt = _capi.seeqdev_counts_t()
        _check(self._lib.seeqdevScanFetch(self._h, C.byref(cnt)))
        return dict(nlines=cnt.nlines, nmatchlines=cnt.nmatchlines, nhits=cnt.nhits, nrecords=cnt.nrecords,
                    nheaders=cnt.nheaders)

    def records(self, n=None, first=0):
        """Copy hit records to the host -> ndarray [n,4] u32 (line,start,end,dist)."""
        if n is None:
            raise ValueError("n required")
        out = np.zeros((n, 4), dtype=np.uint32)
        if n:
            _check(self._lib.seeqdevScanCopyRecords(self._h, out.ctypes.data, first, n))
        return out

    def record_offsets(self, n, first=0):
        """Per record: byte offset of its line in the scanned buffer -> ndarray [n] u64."""
        out = np.zeros(n, dtype=np.uint64)
        if n:
            _check(self._lib.seeqdevScanCopyOffsets(self._h, out.ctypes.data, first, n))
        return out

    def records_device_ptr(self):
        return self._lib.seeqdevScanRecordsDevice(self._h)

    def scan_tensor(self, pattern, t, options=0, want=WANT_COUNTLINES):
        """t: torch uint8 CUDA tensor (contiguous).  Runs and fetches."""
        self.run(pattern, t.data_ptr(), t.numel(), options, want)
        return self.fetch()

    def run_packed(self, pattern, bases_ptr, nmask_ptr, nreads, read_len, stride=None, nstride=None, options=0, want=WANT_COUNTLINES):
        """Enqueue the scan of a packed read batch resident in HBM (seeq_amd.h: seeqdev_packed_t); fetch() waits."""
        b = _capi.seeqdev_packed_t(bases_ptr, nmask_ptr or None, nreads, read_len, stride or (read_len + 3) // 4,
                                   nstride or (read_len + 7) // 8)
        _check(self._lib.seeqdevScanPacked(self._h, pattern.handle, C.byref(b), options, want))

    def scan_host(self, pattern, data, options=0, want=WANT_COUNTLINES):
        """data: bytes.  H2D + scan + fetch (+ records when want == WANT_RECORDS).  options may hold SEEQDEV_FASTQ (see run)."""
        cnt = _capi.seeqdev_counts_t()
        _check(self._lib.seeqdevScanHost(self._h, pattern.handle, data, len(data), options, want, C.byref(cnt)))
        res = dict(nlines=cnt.nlines, nmatchlines=cnt.nmatchlines, nhits=cnt.nhits, nrecords=cnt.nrecords,
                   nheaders=cnt.nheaders)
        if want == WANT_RECORDS:
            res["records"] = self.records(cnt.nrecords)
        return res


    # ---- both strands in one call (include/seeq_amd.h: seeqdevScanRunStrands / seeqdevScanHostStrands) ----
    def _strands(self, call, want, copy):
        cnt = _capi.seeqdev_counts_t()
        per = (C.c_uint64 * 2)()
        _check(call(C.byref(cnt), per))
        res = dict(nlines=cnt.nlines, nmatchlines=cnt.nmatchlines, nhits=cnt.nhits, nrecords=cnt.nrecords, nheaders=cnt.nheaders,
                   per_strand=[int(per[0]), int(per[1])])
        if want == WANT_RECORDS and copy:
            res["records"] = self.strand_records(cnt.nrecords)
        return res

    def strand_records(self, n, first=0):
        """Copy records [first, first + n) of the last both-strands scan to the host -> structured array of STRAND_DTYPE: `dist`
        without the strand bit, `strand` 0 (the pattern as given) or 1 (its reverse complement)."""
        raw = self.records(n, first)
        out = np.zeros(n, dtype=STRAND_DTYPE)
        out["line"], out["start"], out["end"] = raw[:, 0], raw[:, 1], raw[:, 2]
        out["dist"] = raw[:, 3] & np.uint32(~_capi.SEEQDEV_HIT_MINUS & 0xFFFFFFFF)
        out["strand"] = raw[:, 3] >> np.uint32(31)
        return out

    def last_strands_merge_ms(self):
        """Device time of the last both-strands call's merge (its kernels and device copies; profiling on), 0 when not measured."""
        ms = C.c_float(0)
        _check(self._lib.seeqdevScanLastStrandsMs(self._h, C.byref(ms)))
        return float(ms.value)

    def strands_host(self, pattern, data, options=0, want=WANT_RECORDS):
        """data: bytes, staged once.  The text searched with `pattern` and with its reverse complement, the two record sets merged on
        the device (seeq_amd.h: SQ_ALL every record of both in (line, end, strand) order; SQ_BEST / SQ_FIRST the winner of every line)
        -> the counts dict plus per_strand [plus, minus] and, with WANT_RECORDS, records (STRAND_DTYPE); record_offsets() serves the
        merged records' line offsets.  options may hold SEEQDEV_FASTA or SEEQDEV_FASTQ."""
        return self._strands(lambda cnt, per: self._lib.seeqdevScanHostStrands(self._h, pattern.handle, data, len(data), options, want, cnt, per), want, True)

    def strands_tensor(self, pattern, t, options=0, want=WANT_RECORDS, copy=True):
        """t: torch uint8 CUDA tensor (contiguous), resident.  As strands_host; copy=False leaves the records on the device
        (records_device_ptr / strand_records / records: seeqdev_hit_t with SEEQDEV_HIT_MINUS in dist)."""
        return self._strands(lambda cnt, per: self._lib.seeqdevScanRunStrands(self._h, pattern.handle, C.c_void_p(t.data_ptr()), t.numel(), options, want,
                                                                             cnt, per), want, copy)

    # ---- the insert between two flanks (include/seeq_amd.h: seeqdevScanRunInserts / seeqdevScanHostInserts) ----
    def _inserts(self, call, copy):
        cnt = _capi.seeqdev_insert_counts_t()
        _check(call(C.byref(cnt)))
        res = dict(nlines=int(cnt.nlines), nleft=int(cnt.nleft), nright=int(cnt.nright), nboth=int(cnt.nboth), ninserts=int(cnt.ninserts),
                   text_bytes=int(cnt.text_bytes))
        if copy:
            res["records"] = self.insert_records(res["ninserts"])
        return res

    def inserts_host(self, left, right, data, options=0, min_len=0, max_len=0):
        """data: bytes, staged once.  Per line the insert between the `left` flank's record (options: SQ_BEST or SQ_FIRST) and the chosen
        occurrence of the `right` flank at min_len .. max_len bytes behind it (max_len 0: no upper bound), joined on the device
        (seeq_amd.h) -> dict: nlines, nleft, nright, nboth, ninserts, text_bytes, records (INSERT_DTYPE, in line order).
        insert_offsets() serves the records' line offsets, insert_text() the inserts themselves.  options may hold SEEQDEV_FASTA or
        SEEQDEV_FASTQ."""
        return self._inserts(lambda cnt: self._lib.seeqdevScanHostInserts(self._h, left.handle, right.handle, data, len(data), options, min_len, max_len, cnt), True)

    def inserts_tensor(self, left, right, t, options=0, min_len=0, max_len=0, copy=True):
        """t: torch uint8 CUDA tensor (contiguous), resident.  As inserts_host; copy=False leaves the records on the device
        (inserts_device_ptr / insert_records)."""
        return self._inserts(lambda cnt: self._lib.seeqdevScanRunInserts(self._h, left.handle, right.handle, C.c_void_p(t.data_ptr()), t.numel(), options,
                                                                         min_len, max_len, cnt), copy)

    def insert_records(self, n, first=0):
        """Copy records [first, first + n) of the last inserts call to the host -> structured array of INSERT_DTYPE."""
        out = np.zeros(n, dtype=INSERT_DTYPE)
        _check(self._lib.seeqdevScanCopyInserts(self._h, out.ctypes.data if n else None, first, n))
        return out

    def insert_offsets(self, n, first=0):
        """Per insert record: byte offset of its line in the scanned buffer -> ndarray [n] u64."""
        out = np.zeros(n, dtype=np.uint64)
        _check(self._lib.seeqdevScanCopyInsertOffsets(self._h, out.ctypes.data if n else None, first, n))
        return out

    def inserts_device_ptr(self):
        """Device address of the last inserts call's records (seeqdev_insert_t, in line order; valid until this Scanner's next inserts call)."""
        return self._lib.seeqdevScanInsertsDevice(self._h)

    def insert_text_bytes(self):
        """Size of the last inserts call's insert text (seeqdevScanInsertText's size query)."""
        n = C.c_uint64(0)
        _check(self._lib.seeqdevScanInsertText(self._h, None, 0, None, 0, C.byref(n)))
        return int(n.value)

    def insert_text(self, t=None):
        """The inserts of the last call cut out of its text on the device: every insert followed by a newline, in record order.
        t: the tensor inserts_tensor scanned -> a torch uint8 tensor on t's device (the next stage's input: scan_tensor,
        demux_tensor); None: the text inserts_host staged -> bytes."""
        import torch
        n = self.insert_text_bytes()
        out = torch.empty(n, dtype=torch.uint8, device=t.device if t is not None else "cuda")
        got = C.c_uint64(0)
        _check(self._lib.seeqdevScanInsertText(self._h, C.c_void_p(t.data_ptr()) if t is not None else None, t.numel() if t is not None else 0,
                                               C.c_void_p(out.data_ptr()) if n else None, n, C.byref(got)))
        return out if t is not None else out.cpu().numpy().tobytes()

    def last_inserts_join_ms(self):
        """Device time of the last inserts call's join (its four launches; profiling on), 0 when not measured."""
        ms = C.c_float(0)
        _check(self._lib.seeqdevScanLastInsertsMs(self._h, C.byref(ms)))
        return float(ms.value)

    # ---- the tally of distinct spans (include/seeq_amd.h: seeqdevScanTally) ----
    def tally(self, t=None, source="inserts", copy=True):
        """How often each distinct sequence occurs among the inserts of the last inserts call (source "inserts") or among the matches
        [start, end) of the records this Scanner serves now (source "hits": a fetched scan with WANT_RECORDS, a both-strands call),
        counted on the device.  t: the torch uint8 CUDA tensor those records were found in; None (inserts only): the text inserts_host
        staged.  -> dict: nspans, ntallied, nlong, nforeign, ndistinct, max_len, passes; copy adds keys and counts, uint64 arrays in
        ascending key order (by length, then A < C < T < G): tally_key / tally_decode / tally_lookup.  copy=False leaves the table on
        the device (tally_device_ptr / tally_table)."""
        src = _SPAN_SOURCES.get(source, source)
        cnt = _capi.seeqdev_tally_counts_t()
        _check(self._lib.seeqdevScanTally(self._h, src, C.c_void_p(t.data_ptr()) if t is not None else None, t.numel() if t is not None else 0, C.byref(cnt)))
        res = dict(nspans=int(cnt.nspans), ntallied=int(cnt.ntallied), nlong=int(cnt.nlong), nforeign=int(cnt.nforeign), ndistinct=int(cnt.ndistinct),
                   max_len=int(cnt.max_len), passes=int(cnt.passes))
        if copy:
            tab = self.tally_table(res["ndistinct"])
            res["keys"] = np.ascontiguousarray(tab["key"])
            res["counts"] = np.ascontiguousarray(tab["count"])
        return res

    def tally_table(self, n, first=0):
        """Copy entries [first, first + n) of the last tally's table to the host -> structured array of TALLY_DTYPE."""
        out = np.zeros(n, dtype=TALLY_DTYPE)
        _check(self._lib.seeqdevScanCopyTally(self._h, out.ctypes.data if n else None, first, n))
        return out

    def tally_device_ptr(self):
        """Device address of the last tally's table (seeqdev_tally_t, ascending keys; valid until this Scanner's next tally)."""
        return self._lib.seeqdevScanTallyDevice(self._h)

    def last_tally_ms(self):
        """Device time of the last tally (its launches and counter copies; profiling on), 0 when not measured."""
        ms = C.c_float(0)
        _check(self._lib.seeqdevScanLastTallyMs(self._h, C.byref(ms)))
        return float(ms.value)

    # ---- the grouped tally: counts per (group, member) pair (include/seeq_amd.h: seeqdevScanTallyHold / seeqdevScanTallyGrouped) ----
    @staticmethod
    def _text_args(t):
        return (C.c_void_p(t.data_ptr()) if t is not None else None, t.numel() if t is not None else 0)

    def tally_hold(self, t=None, source="inserts"):
        """Keep the keys of a record array as this Scanner's held column, the GROUP of every line for tally_grouped: the inserts of the
        last inserts call ("inserts"), the matches of the records served now ("hits"; of several on a line the first decides), or the
        winning pattern + 1 of the last demultiplex ("demux"; t is not needed; an ambiguous line is held without a key).  t: as in
        tally().  -> dict: nspans, nheld, nlong, nforeign, nambiguous, max_len, key_bits.  The column survives scans, inserts calls,
        demultiplexes and plain tallies; the next tally_hold replaces it."""
        src = _HOLD_SOURCES.get(source, source)
        cnt = _capi.seeqdev_tally_hold_counts_t()
        _check(self._lib.seeqdevScanTallyHold(self._h, src, *self._text_args(t), C.byref(cnt)))
        return dict(nspans=int(cnt.nspans), nheld=int(cnt.nheld), nlong=int(cnt.nlong), nforeign=int(cnt.nforeign), nambiguous=int(cnt.nambiguous),
                    max_len=int(cnt.max_len), key_bits=int(cnt.key_bits))

    def tally_grouped(self, t=None, source="inserts", copy=True):
        """How often each distinct (group, member) pair occurs: the spans of `source` ("inserts" or "hits", as in tally()) are the
        members, the held column of tally_hold names the group of their line -- paired, sorted and counted on the device.  The two scans
        must number lines alike (SEEQDEV_FASTQ in both or in neither; the buffers may differ).  -> dict: nspans, npaired, nlong, nforeign,
        nungrouped, npairs, ngroups, max_len, passes; copy adds pairs (TALLY_PAIR_DTYPE, ordered by group, then member: the sparse count
        matrix in row order) and groups (TALLY_GROUP_DTYPE: per group its reads, the rank of its first pair and its distinct members:
        tally_members).  copy=False leaves both on the device (tally_pairs_device_ptr / tally_pairs_table, tally_groups_device_ptr /
        tally_groups_table)."""
        src = _SPAN_SOURCES.get(source, source)
        cnt = _capi.seeqdev_tally_grouped_counts_t()
        _check(self._lib.seeqdevScanTallyGrouped(self._h, src, *self._text_args(t), C.byref(cnt)))
        res = dict(nspans=int(cnt.nspans), npaired=int(cnt.npaired), nlong=int(cnt.nlong), nforeign=int(cnt.nforeign), nungrouped=int(cnt.nungrouped),
                   npairs=int(cnt.npairs), ngroups=int(cnt.ngroups), max_len=int(cnt.max_len), passes=int(cnt.passes))
        if copy:
            res["pairs"] = self.tally_pairs_table(res["npairs"])
            res["groups"] = self.tally_groups_table(res["ngroups"])
        return res

    def tally_pairs_table(self, n, first=0):
        """Copy entries [first, first + n) of the last grouped tally's pair table to the host -> structured array of TALLY_PAIR_DTYPE."""
        out = np.zeros(n, dtype=TALLY_PAIR_DTYPE)
        _check(self._lib.seeqdevScanCopyTallyPairs(self._h, out.ctypes.data if n else None, first, n))
        return out

    def tally_groups_table(self, n, first=0):
        """Copy entries [first, first + n) of the last grouped tally's group table to the host -> structured array of TALLY_GROUP_DTYPE."""
        out = np.zeros(n, dtype=TALLY_GROUP_DTYPE)
        _check(self._lib.seeqdevScanCopyTallyGroups(self._h, out.ctypes.data if n else None, first, n))
        return out

    def tally_pairs_device_ptr(self):
        """Device address of the last grouped tally's pair table (seeqdev_tally_pair_t; valid until this Scanner's next grouped tally)."""
        return self._lib.seeqdevScanTallyPairsDevice(self._h)

    def tally_groups_device_ptr(self):
        """Device address of the last grouped tally's group table (seeqdev_tally_group_t; valid until this Scanner's next grouped tally)."""
        return self._lib.seeqdevScanTallyGroupsDevice(self._h)

    def last_tally_grouped_ms(self):
        """Device time of the last grouped tally (its launches and counter copies; profiling on), 0 when not measured."""
        ms = C.c_float(0)
        _check(self._lib.seeqdevScanLastTallyGroupedMs(self._h, C.byref(ms)))
        return float(ms.value)

    # ---- collapsing UMI errors behind the grouped tally (include/seeq_amd.h: seeqdevScanTallyCollapse) ----
    def tally_collapse(self, rule="directional", copy=True):
        """Per pair of the last tally_grouped's pair table: a molecule of its own (a root, its own parent) or an erroneous copy, one
        substitution away, of another pair of its group (its parent's index) -- decided on the device.  rule "directional": a parent
        has at least 2 c - 1 reads for a child of c; "any": every neighbour that precedes (higher count, then smaller member).
        -> dict: npairs, ngroups, nroots, nabsorbed, absorbed_reads, rule, max_len; copy adds parent (uint32 per pair) and groups
        (TALLY_COLLAPSE_DTYPE, row r for row r of the group table: nroots, nabsorbed, absorbed_reads).  Chains are not followed:
        collapse_fold does that.  copy=False leaves both on the device (tally_parents_device_ptr / tally_parents_table,
        tally_collapse_device_ptr / tally_collapse_table)."""
        r = {"directional": _capi.SEEQDEV_COLLAPSE_DIRECTIONAL, "any": _capi.SEEQDEV_COLLAPSE_ANY}.get(rule, rule)
        cnt = _capi.seeqdev_tally_collapse_counts_t()
        _check(self._lib.seeqdevScanTallyCollapse(self._h, r, C.byref(cnt)))
        res = {name: int(getattr(cnt, name)) for name, _ in _capi.seeqdev_tally_collapse_counts_t._fields_}
        if copy:
            res["parent"] = self.tally_parents_table(res["npairs"])
            res["groups"] = self.tally_collapse_table(res["ngroups"])
        return res

    def tally_parents_table(self, n, first=0):
        """Copy entries [first, first + n) of the last collapse's parents to the host -> uint32 array (indices into the pair table)."""
        out = np.zeros(n, dtype=np.uint32)
        _check(self._lib.seeqdevScanCopyTallyParents(self._h, out.ctypes.data if n else None, first, n))
        return out

    def tally_collapse_table(self, n, first=0):
        """Copy rows [first, first + n) of the last collapse's group rows to the host -> structured array of TALLY_COLLAPSE_DTYPE."""
        out = np.zeros(n, dtype=TALLY_COLLAPSE_DTYPE)
        _check(self._lib.seeqdevScanCopyTallyCollapse(self._h, out.ctypes.data if n else None, first, n))
        return out

    def tally_parents_device_ptr(self):
        """Device address of the last collapse's parents (uint32 per pair; valid until this Scanner's next grouped tally or collapse)."""
        return self._lib.seeqdevScanTallyParentsDevice(self._h)

    def tally_collapse_device_ptr(self):
        """Device address of the last collapse's group rows (seeqdev_tally_collapse_t; valid until the next grouped tally or collapse)."""
        return self._lib.seeqdevScanTallyCollapseDevice(self._h)

    def last_tally_collapse_ms(self):
        """Device time of the last collapse (its launches and its counters copy; profiling on), 0 when not measured."""
        ms = C.c_float(0)
        _check(self._lib.seeqdevScanLastTallyCollapseMs(self._h, C.byref(ms)))
        return float(ms.value)

    # ---- counting against a known library (include/seeq_amd.h: seeqdevScanSetLibrary / seeqdevScanTallyLibrary / seeqdevScanTallyHoldLibrary) ----
    def set_library(self, sequences, max_mismatch=1, indels=False):
        """Give this Scanner a library of known sequences -- guides, a barcode whitelist: str or bytes of at most 31 bases ACGTU each, or
        an integer array of tally keys.  Entry i has the id i + 1.  max_mismatch 1: a span one substitution away from exactly one entry
        counts for it; 0: exact only.  indels=True (with max_mismatch 1): one EDIT away -- a substitution, or one base lost or gained
        (seeqdevScanSetLibraryMode, SEEQDEV_LIBRARY_EDIT); library_edits() then splits the corrected spans by the kind of the edit.  The
        library stays with the Scanner until the next set_library or clear_library; an empty one clears it.  ValueError for a sequence
        that has no key and for indels with max_mismatch 0, SeeqDeviceError for a duplicate."""
        if indels and int(max_mismatch) != 1:
            raise ValueError("indels=True is one edit: it goes with max_mismatch=1, not %r" % (max_mismatch,))
        if isinstance(sequences, np.ndarray):
            keys = np.ascontiguousarray(sequences, dtype=np.uint64)
        else:
            keys = np.array([q if isinstance(q, (int, np.integer)) else tally_key(q) for q in sequences], dtype=np.uint64)
        if indels:
            _check(self._lib.seeqdevScanSetLibraryMode(self._h, keys.ctypes.data if len(keys) else None, len(keys), _capi.SEEQDEV_LIBRARY_EDIT))
        else:
            _check(self._lib.seeqdevScanSetLibrary(self._h, keys.ctypes.data if len(keys) else None, len(keys), int(max_mismatch)))

    def clear_library(self):
        _check(self._lib.seeqdevScanSetLibrary(self._h, None, 0, 0))

    def library_edits(self):
        """The corrected spans of the last library assignment (tally_library, tally_hold_library, tally_hold_append(library=True)) by the
        kind of their one edit -> dict(nsubstituted, ninserted, ndeleted), summing to its ncorrected: the entry has the span's length, is
        one base longer (the read lost a base), is one base shorter (the read gained one).  All zero after set_library and before any
        assignment; without indels, ninserted = ndeleted = 0."""
        e = _capi.seeqdev_tally_library_edits_t()
        _check(self._lib.seeqdevScanLastLibraryEdits(self._h, C.byref(e)))
        return dict(nsubstituted=int(e.nsubstituted), ninserted=int(e.ninserted), ndeleted=int(e.ndeleted))

    @staticmethod
    def _library_counts(cnt):
        return {name: int(getattr(cnt, name)) for name, _ in _capi.seeqdev_tally_library_counts_t._fields_}

    def tally_library(self, t=None, source="inserts", copy=True):
        """One count per library entry seen among the spans of `source` ("inserts" or "hits", t as in tally()), assigned and counted on
        the device: a span is exact (its sequence is an entry), corrected (one substitution away from exactly one entry, under
        max_mismatch 1), ambiguous (from two or more), unknown, long or foreign.  -> dict: nspans, nassigned, nexact, ncorrected,
        nambiguous, nunknown, nlong, nforeign, ndistinct, key_bits, passes; copy adds ids and counts, uint64 arrays in ascending id
        order, entries without a read absent (library_counts makes the dense vector).  The table is the Scanner's tally table
        (tally_device_ptr / tally_table, `key` = id), replaced by the next tally of either kind."""
        src = _SPAN_SOURCES.get(source, source)
        cnt = _capi.seeqdev_tally_library_counts_t()
        _check(self._lib.seeqdevScanTallyLibrary(self._h, src, *self._text_args(t), C.byref(cnt)))
        res = self._library_counts(cnt)
        if copy:
            tab = self.tally_table(res["ndistinct"])
            res["ids"] = np.ascontiguousarray(tab["key"])
            res["counts"] = np.ascontiguousarray(tab["count"])
        return res

    def tally_hold_library(self, t=None, source="inserts"):
        """tally_hold ("inserts" or "hits") with the held keys assigned to the library: the group of a line is its entry's id, or none.
        A following tally_grouped has one group per library entry seen, erroneous copies folded into their entry.  -> the dict of
        tally_library (ndistinct and passes 0)."""
        src = _HOLD_SOURCES.get(source, source)
        cnt = _capi.seeqdev_tally_library_counts_t()
        _check(self._lib.seeqdevScanTallyHoldLibrary(self._h, src, *self._text_args(t), C.byref(cnt)))
        return self._library_counts(cnt)

    # ---- key columns appended to the held column (include/seeq_amd.h: seeqdevScanTallyHoldAppend / seeqdevScanTallyHoldAppendLibrary) ----
    def tally_hold_append(self, text=None, source="inserts", library=False):
        """Append a key column to the held column, on the device: the keys of `source` ("inserts", "hits", "gated", "anchored", "demux" -- built as
        tally_hold builds them; library=True: assigned to the library as tally_hold_library assigns them, "demux" excluded) are joined
        to the held records by line, the first record of a line deciding, and every held key becomes (key << width) | new key -- or 0
        where either is missing.  tally_grouped, tally_collapse and the library then work on the tuples: (cell, guide) x UMI.  text: the
        tensor of THIS source (as t in tally()), which may be another buffer than the hold's as long as its lines number alike.  -> dict: column (what the
        corresponding hold returns for the source), nrecords, nbefore, nheld, ndropped, width, key_bits, ncolumns.  The widths sum to at
        most 63 bits (SeeqDeviceError, E2BIG, the held column unchanged); hold_columns / hold_split take the group words apart."""
        src = _HOLD_SOURCES.get(source, source)
        cnt = _capi.seeqdev_tally_append_counts_t()
        if library:
            col = _capi.seeqdev_tally_library_counts_t()
            _check(self._lib.seeqdevScanTallyHoldAppendLibrary(self._h, src, *self._text_args(text), C.byref(col), C.byref(cnt)))
            column = self._library_counts(col)
        else:
            col = _capi.seeqdev_tally_hold_counts_t()
            _check(self._lib.seeqdevScanTallyHoldAppend(self._h, src, *self._text_args(text), C.byref(col), C.byref(cnt)))
            column = {name: int(getattr(col, name)) for name, _ in _capi.seeqdev_tally_hold_counts_t._fields_}
        res = {name: int(getattr(cnt, name)) for name, _ in _capi.seeqdev_tally_append_counts_t._fields_ if name != "reserved"}
        res["column"] = column
        return res

    def hold_columns(self):
        """The widths in bits of the held key's columns, column 0 (the hold's) first; [] without a held column."""
        w = (C.c_uint32 * _capi.SEEQDEV_TALLY_COLUMNS)()
        n = self._lib.seeqdevScanTallyHoldColumns(self._h, w, _capi.SEEQDEV_TALLY_COLUMNS)
        _check(min(n, 0))
        return [int(w[c]) for c in range(n)]

    def held_count(self):
        """Records of the held column (0 without one): the largest `first` seeqdevScanCopyHeld accepts, found on the host."""
        fits = lambda k: self._lib.seeqdevScanCopyHeld(self._h, None, None, k, 0) == 0      # noqa: E731
        lo, hi = 0, 1 << 32                                 # fits(lo), not fits(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if fits(mid) else (lo, mid)
        return lo

    def held(self, copy=True):
        """The held column as it stands: -> dict: nrecords, columns (hold_columns()); copy adds lines (uint32) and keys (uint64, 0: no
        key), one per held record in record order."""
        res = dict(nrecords=self.held_count(), columns=self.hold_columns())
        if copy:
            n = res["nrecords"]
            res["lines"], res["keys"] = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
            _check(self._lib.seeqdevScanCopyHeld(self._h, res["lines"].ctypes.data if n else None, res["keys"].ctypes.data if n else None, 0, n))
        return res

    # ---- the tally of the held column itself (include/seeq_amd.h: seeqdevScanTallyHeld / seeqdevScanTallyHeldDense) ----
    def tally_held(self, member_columns=0, copy=True):
        """How often each distinct held word occurs, one count per line (its first held record decides), counted on the device: the
        bulk screen -- sample x guide with no UMI -- behind tally_hold and tally_hold_append.  member_columns m: the last m columns of
        the held key are the column part of a key, the ones before them its row (0: no row table).  -> dict: nrecords, ncounted,
        nkeyless, nrepeat, ndistinct, nrows, key_bits, shift, passes, member_columns; copy adds table (TALLY_DTYPE: the held words
        ascending with their counts -- this Scanner's tally table, replaced by the next tally of any kind) and rows
        (TALLY_GROUP_DTYPE: per row its reads, the rank of its first entry in the table and its entries; empty for m == 0).
        copy=False leaves both on the device (tally_device_ptr / tally_table, tally_held_rows_device_ptr / tally_held_rows_table)."""
        cnt = _capi.seeqdev_tally_held_counts_t()
        _check(self._lib.seeqdevScanTallyHeld(self._h, int(member_columns), C.byref(cnt)))
        res = {name: int(getattr(cnt, name)) for name, _ in _capi.seeqdev_tally_held_counts_t._fields_}
        if copy:
            res["table"] = self.tally_table(res["ndistinct"])
            res["rows"] = self.tally_held_rows_table(res["nrows"])
        return res

    def tally_held_rows_table(self, n, first=0):
        """Copy entries [first, first + n) of the last held tally's row table to the host -> structured array of TALLY_GROUP_DTYPE."""
        out = np.zeros(n, dtype=TALLY_GROUP_DTYPE)
        _check(self._lib.seeqdevScanCopyTallyHeldRows(self._h, out.ctypes.data if n else None, first, n))
        return out

    def tally_held_rows_device_ptr(self):
        """Device address of the last held tally's row table (seeqdev_tally_group_t; valid until this Scanner's next held tally)."""
        return self._lib.seeqdevScanTallyHeldRowsDevice(self._h)

    def held_matrix(self, nrows, ncols, out=None):
        """The dense count matrix of the last tally_held(member_columns >= 1), scattered on the device: cell [r - 1, c - 1] is the count
        of the key with row r and column part c (demux keys and library ids are 1-based); keys outside 1 .. nrows x 1 .. ncols are
        counted, not stored.  out: a contiguous int64 CUDA tensor of shape [nrows, ncols] to fill (every cell is written), None: a new
        one on the current CUDA device.  -> (the tensor, dict: ninside, noutside, inside_reads, outside_reads).  SeeqDeviceError
        (EINVAL) when this Scanner's tally table is no held tally's (a plain or library tally since), E2BIG beyond 2^28 cells."""
        import torch
        nrows, ncols = int(nrows), int(ncols)
        if not (0 <= nrows <= 0xFFFFFFFF and 0 <= ncols <= 0xFFFFFFFF):
            raise ValueError("held_matrix: %d x %d is no matrix shape" % (nrows, ncols))
        if out is None:
            # (a shape the C entry refuses -- no cell, or more than 2^28 -- is refused there, before d_out is touched: nothing is allocated for it)
            fits = 0 < nrows * ncols <= _capi.SEEQDEV_TALLY_DENSE_MAX
            out = torch.empty((nrows, ncols) if fits else (0, 0), dtype=torch.int64, device=torch.device("cuda", torch.cuda.current_device()))
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and tuple(out.shape) == (nrows, ncols)):
            raise ValueError("held_matrix: out must be a contiguous int64 CUDA tensor of shape (%d, %d)" % (nrows, ncols))
        cnt = _capi.seeqdev_tally_dense_counts_t()
        _check(self._lib.seeqdevScanTallyHeldDense(self._h, C.c_void_p(out.data_ptr() if out.numel() else 16), nrows, ncols, C.byref(cnt)))
        return out, {name: int(getattr(cnt, name)) for name, _ in _capi.seeqdev_tally_dense_counts_t._fields_}

    def last_tally_held_ms(self):
        """Device time of the last held tally or held_matrix, whichever came last (profiling on), 0 when not measured."""
        ms = C.c_float(0)
        _check(self._lib.seeqdevScanLastTallyHeldMs(self._h, C.byref(ms)))
        return float(ms.value)

    # ---- the base-quality gate in front of the tallies (include/seeq_amd.h: seeqdevScanQualityGate) ----
    def quality_gate(self, t=None, source="inserts", min_qual=20, base=33, max_low=0, reach=1024, copy=True):
        """Keep the spans of `source` ("inserts", "hits" or "anchored", t as in tally()) whose FASTQ quality bytes are good enough: a span passes when
        at most max_low of the quality bytes under it -- in the line two below its own, found within `reach` bytes behind the span --
        are below base + min_qual.  Decided and compacted on the device; the tallies then take source="gated".  -> dict: nspans,
        npassed, nlow, nlong, nfar, nmisfit, low_bases; copy adds records ([npassed, 4] uint32: the source's 16-byte records unchanged,
        in order), offsets (uint64) and kinds (uint8 per SOURCE record: GATE_PASS, GATE_LOW, GATE_LONG, GATE_FAR, GATE_MISFIT).  The
        gated arrays are copies: they survive later scans and inserts calls, until the next quality_gate."""
        src = {"inserts": _capi.SEEQDEV_TALLY_INSERTS, "hits": _capi.SEEQDEV_TALLY_HITS, "anchored": _capi.SEEQDEV_TALLY_ANCHORED}.get(source, source)
        cnt = _capi.seeqdev_qgate_counts_t()
        _check(self._lib.seeqdevScanQualityGate(self._h, src, *self._text_args(t), min_qual, base, max_low, reach, C.byref(cnt)))
        res = {name: int(getattr(cnt, name)) for name, _ in _capi.seeqdev_qgate_counts_t._fields_}
        if copy:
            res["records"] = self.gated_records(res["npassed"])
            res["offsets"] = self.gated_offsets(res["npassed"])
            res["kinds"] = self.gate_kinds(res["nspans"])
        return res

    def gated_records(self, n, first=0):
        """Copy records [first, first + n) the last quality gate passed to the host -> ndarray [n, 4] u32: the words of the source's
        records (hits: line, start, end, dist with its strand bit; inserts: view as INSERT_DTYPE)."""
        out = np.zeros((n, 4), dtype=np.uint32)
        _check(self._lib.seeqdevScanCopyGated(self._h, out.ctypes.data if n else None, first, n))
        return out

    def gated_offsets(self, n, first=0):
        """Per gated record: byte offset of its line in the scanned buffer -> ndarray [n] u64."""
        out = np.zeros(n, dtype=np.uint64)
        _check(self._lib.seeqdevScanCopyGatedOffsets(self._h, out.ctypes.data if n else None, first, n))
        return out

    def gate_kinds(self, n, first=0):
        """Per record of the last quality gate's SOURCE: what its span was -> ndarray [n] u8."""
        out = np.zeros(n, dtype=np.uint8)
        _check(self._lib.seeqdevScanCopyGateKinds(self._h, out.ctypes.data if n else None, first, n))
        return out

    def gated_device_ptr(self):
        """Device address of the records the last quality gate passed (16 bytes each; valid until this Scanner's next quality_gate);
        None when it passed none."""
        return self._lib.seeqdevScanGatedDevice(self._h)

    def last_quality_gate_ms(self):
        """Device time of the last quality gate (its launches and counter copies; profiling on), 0 when not measured."""
        ms = C.c_float(0)
        _check(self._lib.seeqdevScanLastQualityGateMs(self._h, C.byref(ms)))
        return float(ms.value)

    # ---- cuts at fixed offsets from a hit or the line's start (include/seeq_amd.h: seeqdevScanAnchor) ----
    def anchor(self, text=None, source="hits", anchor="after", skip=0, length=0, reach=1024, copy=True):
        """Rewrite the span of every record of `source` ("hits" or "inserts"; text: as t in tally()) to a cut at fixed offsets, on the device:
        anchor "after": `length` bytes from `skip` bytes behind the record's end; "before": `length` bytes that end `skip` bytes in front
        of its start; "line": columns [skip, skip + length) of its line.  length 0: as far as the line goes (its end is searched within
        `reach` bytes behind the record's end).  The records whose cut fits are kept in arrays of the anchor's own; the tallies and the
        quality gate then take source="anchored".  -> dict: nspans, nkept, nshort, nfar, span_bytes; copy adds records ([nkept, 4]
        uint32: line, the cut's start and end, the source's fourth word), offsets (uint64) and kinds (uint8 per SOURCE record:
        ANCHOR_KEPT, ANCHOR_SHORT, ANCHOR_FAR).  The anchored arrays are copies: they survive later scans and inserts calls, until the
        next anchor; the source is untouched, so a second anchor over it sees what the first one saw."""
        src = {"inserts": _capi.SEEQDEV_TALLY_INSERTS, "hits": _capi.SEEQDEV_TALLY_HITS}.get(source, source)
        cnt = _capi.seeqdev_anchor_counts_t()
        _check(self._lib.seeqdevScanAnchor(self._h, src, *self._text_args(text), _ANCHORS.get(anchor, anchor), skip, length, reach, C.byref(cnt)))
        res = {name: int(getattr(cnt, name)) for name, _ in _capi.seeqdev_anchor_counts_t._fields_}
        if copy:
            res["records"] = self.anchored_records(res["nkept"])
            res["offsets"] = self.anchored_offsets(res["nkept"])
            res["kinds"] = self.anchor_kinds(res["nspans"])
        return res

    def anchored_records(self, n, first=0):
        """Copy records [first, first + n) the last anchor kept to the host -> ndarray [n, 4] u32: line, the cut [start, end), and the
        source's fourth word (hits: dist with its strand bit; inserts: view as INSERT_DTYPE)."""
        out = np.zeros((n, 4), dtype=np.uint32)
        _check(self._lib.seeqdevScanCopyAnchored(self._h, out.ctypes.data if n else None, first, n))
        return out

    def anchored_offsets(self, n, first=0):
        """Per anchored record: byte offset of its line in the scanned buffer -> ndarray [n] u64."""
        out = np.zeros(n, dtype=np.uint64)
        _check(self._lib.seeqdevScanCopyAnchoredOffsets(self._h, out.ctypes.data if n else None, first, n))
        return out

    def anchor_kinds(self, n, first=0):
        """Per record of the last anchor's SOURCE: what its cut was -> ndarray [n] u8."""
        out = np.zeros(n, dtype=np.uint8)
        _check(self._lib.seeqdevScanCopyAnchorKinds(self._h, out.ctypes.data if n else None, first, n))
        return out

    def anchored_device_ptr(self):
        """Device address of the records the last anchor kept (16 bytes each; valid until this Scanner's next anchor); None when it
        kept none."""
        return self._lib.seeqdevScanAnchoredDevice(self._h)

    def last_anchor_ms(self):
        """Device time of the last anchor (its launches and counter copies; profiling on), 0 when not measured."""
        ms = C.c_float(0)
        _check(self._lib.seeqdevScanLastAnchorMs(self._h, C.byref(ms)))
        return float(ms.value)

    # ---- several patterns, one text (include/seeq_amd.h: seeqdevScanRunMulti / seeqdevScanHostMulti) ----
    def _multi(self, patterns, call, want, copy=True):
        n = len(patterns)
        arr = (C.c_void_p * n)(*[C.cast(p.handle, C.c_void_p) for p in patterns])
        cnts = (_capi.seeqdev_counts_t * n)()
        _check(call(arr, n, C.cast(cnts, C.c_void_p)))
        out = []
        for k in range(n):
            c = cnts[k]
            res = dict(nlines=c.nlines, nmatchlines=c.nmatchlines, nhits=c.nhits, nrecords=c.nrecords, nheaders=c.nheaders)
            if want == WANT_RECORDS:
                ptr, m = C.c_void_p(), C.c_size_t()
                _check(self._lib.seeqdevScanMultiRecords(self._h, k, C.byref(ptr), C.byref(m)))
                if copy:
                    rec = np.zeros((m.value, 4), dtype=np.uint32)
                    if m.value:
                        C.memmove(rec.ctypes.data, ptr.value, m.value * 16)
                elif m.value:
                    # a view of the context's page-locked buffer: valid until the next multi scan of this Scanner
                    rec = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint32)), shape=(m.value, 4))
                else:
                    rec = np.zeros((0, 4), dtype=np.uint32)
                res["records"] = rec
            out.append(res)
        return out

    def last_multi_one_pass(self):
        """True when the last multi-pattern scan walked the text once for all its patterns (seeq_multi.h)."""
        return bool(self._lib.seeqdevScanLastMulti(self._h))

    def scan_host_multi(self, patterns, data, options=0, want=WANT_COUNTLINES, copy=True):
        """data: bytes, staged ONCE.  -> one result dict per pattern (copy=False: records are views of the Scanner's buffer,
        valid until its next multi scan)."""
        return self._multi(patterns, lambda arr, n, cnts: self._lib.seeqdevScanHostMulti(self._h, arr, n, data, len(data), options, want, cnts), want, copy)

    def scan_tensor_multi(self, patterns, t, options=0, want=WANT_COUNTLINES, copy=True):
        """t: torch uint8 CUDA tensor (contiguous), resident.  -> one result dict per pattern (copy: see scan_host_multi)."""
        return self._multi(patterns, lambda arr, n, cnts: self._lib.seeqdevScanRunMulti(self._h, arr, n, C.c_void_p(t.data_ptr()), t.numel(),
                                                                                     options, want, cnts), want, copy)

    # ---- demultiplexing on the device (include/seeq_amd.h: seeqdevScanRunDemux / seeqdevScanHostDemux) ----
    def _demux(self, patterns, call, copy):
        n = len(patterns)
        arr = (C.c_void_p * n)(*[C.cast(p.handle, C.c_void_p) for p in patterns])
        cnt = _capi.seeqdev_demux_counts_t()
        per = (C.c_uint64 * n)()
        _check(call(arr, n, C.byref(cnt), per))
        res = dict(nlines=int(cnt.nlines), nassigned=int(cnt.nassigned), nambiguous=int(cnt.nambiguous), assigned=[int(x) for x in per],
                   records=None)
        if copy:
            res["records"] = self.demux_records(int(cnt.nassigned))
        return res

    def demux_records(self, n, first=0):
        """Copy records [first, first + n) of the last demultiplex to the host -> structured array of DEMUX_DTYPE."""
        out = np.zeros(n, dtype=DEMUX_DTYPE)
        _check(self._lib.seeqdevScanCopyDemux(self._h, out.ctypes.data if n else None, first, n))
        return out

    def demux_device_ptr(self):
        """Device address of the last demultiplex's records (seeqdev_demux_t, in line order; valid until this Scanner's next scan)."""
        return self._lib.seeqdevScanDemuxDevice(self._h)

    def demux_host(self, patterns, data, options=0):
        """data: bytes, staged once.  Per line the best pattern of the set, demultiplexed on the device -> dict: nlines, nassigned,
        nambiguous, assigned (lines won per pattern), records (one per assigned line, in line order; DEMUX_DTYPE).  With SEEQDEV_FASTQ in
        options only the sequence lines of four-line FASTQ records count: `line` is the record number, nlines counts records."""
        return self._demux(patterns, lambda arr, n, cnt, per: self._lib.seeqdevScanHostDemux(self._h, arr, n, data, len(data), options, cnt, per), True)

    def demux_tensor(self, patterns, t, options=0, copy=True):
        """t: torch uint8 CUDA tensor (contiguous), resident.  As demux_host; copy=False leaves the records on the device
        (records None: demux_device_ptr / demux_records)."""
        return self._demux(patterns, lambda arr, n, cnt, per: self._lib.seeqdevScanRunDemux(self._h, arr, n, C.c_void_p(t.data_ptr()), t.numel(),
                                                                                         options, cnt, per), copy)


# Scanner.fallback(): the bits (csrc/seeq_types.h, OVF_*) that set a context's fall-back flags
FALLBACK_NO_STREAM, FALLBACK_NONDNA, FALLBACK_LONG_LINES, FALLBACK_SEAM, FALLBACK_LEADER = 8, 16, 32, 128, 256

# One record of seeqdevScanRunStrands as strand_records() returns it: the 16-byte seeqdev_hit_t with the strand bit of `dist` taken out.
STRAND_DTYPE = np.dtype([("line", "<u4"), ("start", "<u4"), ("end", "<u4"), ("dist", "<u4"), ("strand", "u1")])

# One record of seeqdevScanRunInserts (seeq_amd.h: seeqdev_insert_t, 16 bytes): bytes [start, end) of line `line` are the insert.
INSERT_DTYPE = np.dtype([("line", "<u4"), ("start", "<u4"), ("end", "<u4"), ("ldist", "<u2"), ("rdist", "<u2")])

# One entry of seeqdevScanTally's table (seeq_amd.h: seeqdev_tally_t, 16 bytes).
TALLY_DTYPE = np.dtype([("key", "<u8"), ("count", "<u8")])
# what Scanner.quality_gate's `kinds` hold, per source record
GATE_PASS, GATE_LOW, GATE_LONG, GATE_FAR, GATE_MISFIT = (_capi.SEEQDEV_QGATE_PASS, _capi.SEEQDEV_QGATE_LOW, _capi.SEEQDEV_QGATE_LONG,
                                                         _capi.SEEQDEV_QGATE_FAR, _capi.SEEQDEV_QGATE_MISFIT)
# what Scanner.anchor's `kinds` hold, per source record
ANCHOR_KEPT, ANCHOR_SHORT, ANCHOR_FAR = _capi.SEEQDEV_ANCHOR_KEPT, _capi.SEEQDEV_ANCHOR_SHORT, _capi.SEEQDEV_ANCHOR_FAR


def tally_key(seq):
    """The tally's key of a sequence of at most 31 bases ACGTU in either case (str or bytes); ValueError for a long or foreign one."""
    raw = seq.encode("latin-1") if isinstance(seq, str) else bytes(seq)
    key = C.c_uint64(0)
    if _capi.lib().seeqdevTallyKey(raw, len(raw), C.byref(key)):
        raise ValueError("no tally key: %r is longer than 31 bases or holds a byte that is no base" % (seq,))
    return int(key.value)


def tally_decode(key):
    """The sequence a tally key stands for, upper case (A C T G); ValueError for a value that is no key."""
    out = C.create_string_buffer(32)
    n = _capi.lib().seeqdevTallyDecode(int(key), out)
    if n < 0:
        raise ValueError("no tally key: %#x" % int(key))
    return out.raw[:n].decode("ascii")


def tally_lookup(result, sequences):
    """One count per given sequence from a tally() result (copy=True): a binary search over the key-ordered table, 0 when the
    sequence was not seen -- the count table of a guide or barcode library.  Host NumPy over the distinct keys only."""
    keys, counts = result["keys"], result["counts"]
    want = np.array([tally_key(q) for q in sequences], dtype=np.uint64)
    out = np.zeros(len(want), dtype=np.uint64)
    if len(keys) and len(want):
        at = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
        hit = keys[at] == want
        out[hit] = counts[at[hit]]
    return out


def library_counts(result, n):
    """The dense count vector of a library of n entries from a tally_library() result (copy=True): uint64[n], entry i the count of
    id i + 1, 0 for an entry without a read."""
    ids, counts = np.asarray(result["ids"], dtype=np.uint64), np.asarray(result["counts"], dtype=np.uint64)
    if len(ids) and (int(ids.min()) < 1 or int(ids.max()) > n):
        raise ValueError("an id outside 1 .. %d: the result is not that of a library of %d entries" % (n, n))
    out = np.zeros(n, dtype=np.uint64)
    out[ids.astype(np.int64) - 1] = counts
    return out


# One entry of seeqdevScanTallyGrouped's pair table / group table (seeq_amd.h: seeqdev_tally_pair_t, seeqdev_tally_group_t, 24 bytes each).
TALLY_PAIR_DTYPE = np.dtype([("group", "<u8"), ("member", "<u8"), ("count", "<u8")])
TALLY_GROUP_DTYPE = np.dtype([("group", "<u8"), ("count", "<u8"), ("first", "<u4"), ("ndistinct", "<u4")])


def tally_members(result, group):
    """The pairs of one group from a tally_grouped() result (copy=True): the slice of result["pairs"] that the group's entry of
    result["groups"] names, found by a binary search over the group keys; empty when the group was not seen.  group: the key (an int:
    tally_key(sequence), or pattern + 1 after a demux hold)."""
    groups, pairs = result["groups"], result["pairs"]
    at = int(np.searchsorted(groups["group"], np.uint64(group)))
    if at == len(groups) or int(groups["group"][at]) != int(group):
        return pairs[:0]
    first = int(groups["first"][at])
    return pairs[first:first + int(groups["ndistinct"][at])]


def hold_split(keys, widths):
    """Group words of a held key of several columns -> a tuple of uint64 arrays, one per column (column 0, the hold's, first): what
    seeqdevTallySplit does per key, for a whole array -- result["groups"]["group"], result["pairs"]["group"] of a tally_grouped() behind
    tally_hold_append, with widths = Scanner.hold_columns().  ValueError: no column or more than 8, widths that sum to more than 63 bits,
    a key with bits above them."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    widths = [int(w) for w in widths]
    if not 1 <= len(widths) <= _capi.SEEQDEV_TALLY_COLUMNS or any(w < 0 for w in widths) or sum(widths) > 63:
        raise ValueError("hold_split: 1 .. %d columns whose widths sum to at most 63 bits, not %r" % (_capi.SEEQDEV_TALLY_COLUMNS, widths))
    if len(keys) and int(keys.max()) >> sum(widths):
        raise ValueError("hold_split: a key with bits above the %d of its columns" % sum(widths))
    out, rest = [], keys
    for w in reversed(widths):
        out.append(rest & np.uint64((1 << w) - 1))
        rest = rest >> np.uint64(w)
    return tuple(reversed(out))


def held_cell(key, shift, nrows, ncols):
    """Where Scanner.held_matrix puts the count of a held word (seeqdevTallyHeldCell, on the host): with r = key >> shift and
    c = key & ((1 << shift) - 1), the flat index (r - 1) * ncols + (c - 1) when 1 <= r <= nrows and 1 <= c <= ncols, else None."""
    cell = C.c_uint64(0)
    rc = _capi.lib().seeqdevTallyHeldCell(int(key), int(shift), int(nrows), int(ncols), C.byref(cell))
    _check(min(rc, 0))
    return int(cell.value) if rc == 1 else None


# One row of seeqdevScanTallyCollapse's group rows (seeq_amd.h: seeqdev_tally_collapse_t, 16 bytes).
TALLY_COLLAPSE_DTYPE = np.dtype([("nroots", "<u4"), ("nabsorbed", "<u4"), ("absorbed_reads", "<u8")])


def collapse_fold(pairs, parent):
    """Follow the parents of a tally_collapse() result to their roots, on the host: -> (root, folded).  root[i] (uint32) is the index of
    the root of pair i's family (i itself for a root); folded[i] (uint64) is, for a root, the reads of its whole family -- its own count
    and those of every pair absorbed into it, directly or through a chain -- and 0 for a pair that is no root.  pairs: the pair table
    (TALLY_PAIR_DTYPE) the parents belong to.  Pointer doubling: O(log depth) gathers.  ValueError: parent and pairs differ in length, a
    parent index lies outside the table, or the parents do not form a forest."""
    parent = np.asarray(parent)
    n = len(pairs)
    if parent.ndim != 1 or len(parent) != n:
        raise ValueError("%d parents for %d pairs" % (parent.size, n))
    up = parent.astype(np.int64)
    if n and (int(up.min()) < 0 or int(up.max()) >= n):
        raise ValueError("a parent index outside the %d pairs of the table" % n)
    root = up
    for _ in range(max(n, 1).bit_length() + 1):             # (a chain of n pairs is done after ceil(log2 n) doublings)
        root = root[root]
    if not np.array_equal(up[root], root):                  # (what a pair ends on is its own parent, or it went round a cycle)
        raise ValueError("the parents do not form a forest (a cycle)")
    folded = np.zeros(n, dtype=np.uint64)
    np.add.at(folded, root, np.asarray(pairs["count"], dtype=np.uint64))
    return root.astype(np.uint32), folded


# One record of seeqdevScanRunDemux (seeq_amd.h: seeqdev_demux_t, 16 bytes).
DEMUX_DTYPE = np.dtype([("line", "<u4"), ("start", "<u4"), ("end", "<u4"), ("dist", "<u2"), ("pattern", "u1"), ("margin", "u1")])


def demux_dense(result, nlines):
    """A demux_host / demux_tensor result (copy=True) -> the dense per-line arrays assign_best returns:
    (which [nlines] int32, -1 = no pattern matched; dist [nlines] int32, -1 there; start, end [nlines] int64)."""
    rec = result["records"]
    if rec is None:
        raise ValueError("demux_dense needs the records: demultiplex with copy=True")
    which = np.full(nlines, -1, dtype=np.int32)
    dist = np.full(nlines, -1, dtype=np.int32)
    start = np.zeros(nlines, dtype=np.int64)
    end = np.zeros(nlines, dtype=np.int64)
    ln = rec["line"].astype(np.int64) - 1
    which[ln] = rec["pattern"]
    dist[ln] = rec["dist"]
    start[ln] = rec["start"]
    end[ln] = rec["end"]
    return which, dist, start, end


def assign_best(results, nlines):
    """Demultiplexing rule on top of a multi-pattern SQ_BEST scan: per line the pattern with the smallest distance
    (ties: the first pattern in the list).  results: what scan_*_multi(..., SQ_BEST, WANT_RECORDS) returned.
    -> (which [nlines] int32, -1 = no pattern matched; dist [nlines] int32; start, end [nlines] int64)."""
    which = np.full(nlines, -1, dtype=np.int32)
    dist = np.full(nlines, np.iinfo(np.int32).max, dtype=np.int32)
    start = np.zeros(nlines, dtype=np.int64)
    end = np.zeros(nlines, dtype=np.int64)
    for k, r in enumerate(results):
        rec = r["records"]
        if not len(rec):
            continue
        ln = rec[:, 0].astype(np.int64) - 1
        better = rec[:, 3].astype(np.int32) < dist[ln]           # strict: an earlier pattern keeps a tie
        ln = ln[better]
        which[ln] = k
        dist[ln] = rec[better, 3]
        start[ln] = rec[better, 1]
        end[ln] = rec[better, 2]
    dist[which < 0] = -1
    return which, dist, start, end


def synth_reads(d_ptr, first, n, length, pattern_plain, tau, seed=0x5EE92025, stream=None):
    """Fill device memory with n synthetic reads (length bases + newline each)."""
    p = pattern_plain.encode() if isinstance(pattern_plain, str) else pattern_plain
    _check(_capi.lib().seeqdevSynthReads(C.c_void_p(d_ptr), first, n, length, p, len(p), tau, seed,
                                         C.c_void_p(stream) if stream else None))
