/*
 * include/seeq_amd.h -- batched, device-level C-ABI of seeq-mi355x.
 *
 * This is the boundary the HIP kernels sit behind.  Plain pointers and sizes
 * only (no torch / C++ types).  What it replaces in the reference is the
 * per-file hot loop: one `getline` + one `seeqStringMatch` per line
 * (reference seeq.c:361-387 calling libseeq.c:171-352).  One `seeqdevScanRun`
 * call performs that whole loop for every line of a text buffer that is
 * already resident in HBM, and leaves counts + ordered hit records in HBM.
 *
 * The libseeq.h / seeq.h entry points (seeqStringMatch, seeqFileMatch) are
 * implemented on top of these calls; bench.py and the Python module call
 * them directly through ctypes with device pointers.
 *
 * Error convention (same as libseeq.h): functions return NULL / -1, set
 * `seeqerr = 0` and `errno` (ENODEV: no usable GPU, ENOMEM: device or host
 * allocation failed, EIO: a HIP call failed, EINVAL/E2BIG: bad arguments);
 * seeqdevLastError() returns the HIP error text.
 */
#ifndef SEEQ_AMD_H_
#define SEEQ_AMD_H_

#include <stddef.h>
#include <stdint.h>

#include "libseeq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SEEQ_AMD_VERSION "seeq-mi355x-0.1"

/* Longest pattern (positions) the kernels are instantiated for. */
#define SEEQDEV_MAX_WLEN 512

/* What a scan must produce (`want`): mirrors the file options of reference
 * seeq.h:64-68.  Counts are always produced; RECORDS adds hit records. */
#define SEEQDEV_WANT_COUNTLINES 0   /* SQ_COUNTLINES: #lines with >=1 hit (seeq.c:349 forces FIRST)   */
#define SEEQDEV_WANT_COUNTMATCH 1   /* SQ_COUNTMATCH: total hits under SQ_ALL (seeq.c:348)             */
#define SEEQDEV_WANT_RECORDS    2   /* (line,start,end,dist) per hit under match_opt FIRST/BEST/ALL    */

/* Extra scan flags, OR-ed into `options` above the libseeq.h option bits. */
#define SEEQDEV_FASTA       0x100   /* lines starting with '>' are headers: skipped, not counted (seeq.c:367-374) */
#define SEEQDEV_SINGLELINE  0x200   /* the buffer is ONE string (seeqStringMatch semantics, libseeq.c:171): no
                                       newline index; with SQ_STREAM newlines are skipped (libseeq.c:265)  */
#define SEEQDEV_FASTQ       0x400   /* the buffer is four-line FASTQ records: only the sequence lines count (below)   */

/* SEEQDEV_FASTQ.  The buffer is a sequence of four-line FASTQ records, taken purely BY POSITION: raw line 4r + 2 (1-based) is the
 * sequence line of record r + 1; nothing looks for '@' or '+', and a trailing partial record counts when its sequence line is
 * there.  (Without the flag a FASTQ buffer is scanned as plain lines: headers, '+' lines and quality strings -- Phred+33 holds
 * A, C and G -- give records of their own, numbered by raw line.)  Every observable result is that of the same call, with the
 * same `options` and `want`, over a buffer that holds the sequence lines alone -- seeqdev_hit_t.line / seeqdev_demux_t.line is the
 * 1-based RECORD number, nlines = (raw lines + 2) / 4, nmatchlines / nhits / nrecords / nassigned / nambiguous / per_pattern count
 * sequence lines only, seeqdevScanRecordsDevice / CopyRecords / CopyOffsets / DemuxDevice / CopyDemux see the filtered, still
 * ordered arrays -- with two exceptions: seeqdevScanCopyOffsets reports each record's sequence-line offset in the ORIGINAL
 * buffer, and nheaders is 0.
 * Accepted by seeqdevScanRun, seeqdevScanHostBegin, seeqdevScanHost (seeqdevScanFetch completes it) and seeqdevScanRunDemux /
 * seeqdevScanHostDemux.  EINVAL: together with SEEQDEV_FASTA, SEEQDEV_SINGLELINE or SQ_STREAM; given to seeqdevScanPacked,
 * seeqdevScanRunMulti / seeqdevScanHostMulti or seeqdevStringMatch.
 * How, and what it costs: the scan kernels run unchanged over all four lines, and seeqdevScanFetch (the demultiplexer: its last
 * step) runs one ordered compaction of the records on the device (seeq_fastq.h: three launches, at most 24 bytes read and
 * written per record).  A context that has been given the flag keeps a second record array and a second offset array
 * (16 + 8 bytes per record of workspace capacity, sized by seeqdevScanReserve's max_records like the first; allocated by the
 * context's first flagged call, so a seeqdevScanReserve AFTER that call is the one after which Run and Fetch do not allocate).
 * The workspace must hold the records of all four lines.  SEEQDEV_WANT_COUNTLINES / COUNTMATCH have no records to filter: under the
 * flag the scan runs for records (SQ_FIRST / SQ_ALL) and the counts come from the filter -- nrecords is 0 and
 * seeqdevScanCopyRecords refuses as ever, but the count modes need record workspace for EVERY hit of the buffer. */

/* One hit.  `line` is the 1-based index among counted lines of the scanned
 * buffer (reference seeq.c:377); `end` is exclusive (libseeq.h:62-66).
 * 16 bytes: the "algorithmic bytes per hit" of SURVEY section 8d. */
typedef struct {
   uint32_t line;
   uint32_t start;
   uint32_t end;
   uint32_t dist;
} seeqdev_hit_t;

/* A record of a both-strands scan (seeqdevScanRunStrands below) carries its strand in bit 31 of `dist` -- a distance never exceeds
 * SEEQDEV_MAX_WLEN - 1 = 511, so the bit is free; every other scan leaves it clear. */
#define SEEQDEV_HIT_MINUS 0x80000000u
#define SEEQDEV_HIT_DIST(hit_dist)   ((hit_dist) & ~SEEQDEV_HIT_MINUS)           /* the distance of a record's `dist` word */
#define SEEQDEV_HIT_STRAND(hit_dist) (((hit_dist) & SEEQDEV_HIT_MINUS) ? 1 : 0)   /* 0: the pattern as given (plus); 1: its reverse complement (minus) */

typedef struct {
   uint64_t nlines;       /* counted lines (FASTA headers excluded)            */
   uint64_t nmatchlines;  /* lines with at least one hit                       */
   uint64_t nhits;        /* hits under the requested match mode               */
   uint64_t nrecords;     /* records stored (== nhits for WANT_RECORDS else 0) */
   uint64_t nheaders;     /* FASTA header lines skipped                        */
} seeqdev_counts_t;

typedef struct seeqdev_pattern seeqdev_pattern_t;   /* pattern tables in HBM */
typedef struct seeqdev_scan    seeqdev_scan_t;      /* stream + workspace    */

/* Number of usable HIP devices (0 if none / no runtime).  Never fails. */
int seeqdevDeviceCount(void);
/* Select the device used by subsequent seeqdevPatternNew / seeqdevScanNew calls of this thread (hipSetDevice).
 * Patterns and scan contexts remember the device they were created on; every call on them runs there. */
int seeqdevSetDevice(int device);
const char * seeqdevLastError(void);

/* Upload the compiled pattern.  `keys` is the output of the pattern
 * compiler (one byte per position, reference libseeq.c:517-543), wlen <=
 * SEEQDEV_MAX_WLEN, 0 <= tau < wlen (reference libseeq.c:69-72,92-96). */
seeqdev_pattern_t * seeqdevPatternNew(const char * keys, int wlen, int tau);
void                seeqdevPatternFree(seeqdev_pattern_t * pat);
/* The device pattern behind a seeq_t made by seeqNew() (sq->dfa). */
seeqdev_pattern_t * seeqdevPatternOf(const seeq_t * sq);
/* The HIP device a pattern lives on (the device that was current in seeqdevPatternNew); -1 for NULL.  A pattern and
 * the scan contexts that use it must live on the same device: a caller that spreads chunks over several GPUs
 * (seeqFileMatch with SEEQ_DEVICES) makes one pattern per device. */
int seeqdevPatternDevice(const seeqdev_pattern_t * pat);

/* A scan context owns its workspace in HBM and runs on `hip_stream`
 * (a hipStream_t passed as void*; NULL => a private stream). */
seeqdev_scan_t * seeqdevScanNew(void * hip_stream);
void             seeqdevScanFree(seeqdev_scan_t * scan);
/* Pre-size the workspace so that seeqdevScanRun never allocates (so it can
 * sit inside a timed region / graph).  Any argument may be 0 = keep. */
int seeqdevScanReserve(seeqdev_scan_t * scan, size_t max_bytes, size_t max_lines, size_t max_hitlines,
                       size_t max_records);

/* Optional: average bytes per line (newline included) of the buffers to come; sizes the text
 * tiles of the fused kernel.  0 (default) = estimate it from a 64 KiB sample of each new buffer. */
int seeqdevScanSetLineHint(seeqdev_scan_t * scan, double avg_bytes_per_line);
/* Which device path served the last run: 1 = generic (newline index + k_forward<W>),
 * 3 = one-pass per-line bit-vector kernel, text in registers (k_direct),
 * 5 = one-pass table-driven line-agnostic kernel (k_stream: every lane walks a fixed chunk of the text
 *     through the pattern's Levenshtein automaton held in LDS),
 * 6 = the same walk, two text bytes per table step, over the pattern's pair automaton (k_pair: candidates, verified),
 * 7 = the same frame with the bit-vector column instead of a table (k_stream's Myers mode: patterns without an automaton on
 *     long lines), 8 = a packed read batch (seeqdevScanPacked).
 * The one-pass kernels serve patterns <= 62 positions in ONE pass over the text. */
int seeqdevScanLastPath(const seeqdev_scan_t * scan);
/* 1 when the last run's k_stream walked a partition FILTER automaton (candidates verified by the exact pass)
 * instead of the pattern's complete automaton. */
int seeqdevScanLastFilter(const seeqdev_scan_t * scan);
/* The plan the last run executed (seeq_plan.h: which kernel instance scanned, which post-pass followed), as sixteen numbers:
 * rc, path (as seeqdevScanLastPath), fw (words of the one-pass kernels' column), use_stream, use_pair, use_myers, filter, stream_ll,
 * stream_sub (0, 1 SQ_CONVERT, 2 SQ_IGNORE), stream_wu (warm-up dwords of the scan kernel), verify, order2, leaders, window_ok,
 * ll_filter (0, 1 the absorbing table, 2 the restart table / k_pair's long-line windows), skip_back.  Like seeqdevScanLastPath it
 * describes the run that produced the fetched result: after a fall-back re-run, the re-run's plan.  A packed run (path 8) has no
 * such plan: path and filter are set, the rest is 0.  All 0 before the first scan.  Read-only, for tests and diagnostics: the
 * numbers follow the planner and may change with it.  0, or -1 (EINVAL) for a NULL argument. */
int seeqdevScanLastPlan(const seeqdev_scan_t * scan, int out[16]);
/* 1 when the last packed run (path 8) walked the pattern's QUAD table -- four bases, one packed byte, per table step over a small
 * partition-filter automaton (seeq_dfa.h section 3b) -- instead of the pair table (two bases per step). */
int seeqdevScanLastPackedQuad(const seeqdev_scan_t * scan);
/* The runs the last completed scan took: 1 = the first run's counters were the result, more = the device reported a workspace too
 * small or a kernel that could not serve the text, and the scan was run again (seeqdevScanFetch).  Of a multi-pattern, demux or
 * both-strands call: the runs of its last scan or walk.  0 before the first scan. */
int seeqdevScanLastRuns(const seeqdev_scan_t * scan);
/* The fall-back flags the context remembers of earlier texts (a long line among reads, foreign bytes, a line across a segment
 * seam ...: internal bits, 0 = none) and the scans they stay in force for; either pointer may be NULL.  Read-only. */
int seeqdevScanFallback(const seeqdev_scan_t * scan, unsigned * bits, int * scans_left);

/* Enqueue (asynchronously, on the context's stream) the whole hot path over
 * d_text[0..nbytes): newline index -> per-line forward scan -> hit-line
 * compaction -> exact pass (acceptance rules + reverse start recovery) ->
 * ordered records.  `options` = libseeq.h match/non-DNA/input bits |
 * SEEQDEV_* flags.  d_text must stay valid until seeqdevScanFetch returns. */
int seeqdevScanRun(seeqdev_scan_t * scan, const seeqdev_pattern_t * pat, const void * d_text, size_t nbytes,
                   int options, int want);

/* Wait for the scan and return its counts.  If the workspace was too small
 * the scan is transparently re-run with a larger one (never happens after a
 * sufficient seeqdevScanReserve). */
int seeqdevScanFetch(seeqdev_scan_t * scan, seeqdev_counts_t * counts);

/* Hit records of the last fetched scan: device pointer / copy to host. */
const seeqdev_hit_t * seeqdevScanRecordsDevice(const seeqdev_scan_t * scan);
int seeqdevScanCopyRecords(seeqdev_scan_t * scan, seeqdev_hit_t * host_out, size_t first, size_t n);
/* Per record, the byte offset (within the scanned buffer) of the first byte of its line: lets a caller that
 * holds the text go from hit to hit without walking the lines in between. */
int seeqdevScanCopyOffsets(seeqdev_scan_t * scan, uint64_t * host_out, size_t first, size_t n);

/* Page-locked host memory (hipHostMalloc / hipHostFree) for buffers handed to seeqdevScanHost.  May be called from any thread (seeqFileMatch's
 * reader thread does): NULL + errno = ENOMEM on failure, and -- alone among these entries -- seeqerr is left untouched (it is the reference's plain
 * global, libseeq.h:38, and belongs to the thread that calls the seeq API). */
void * seeqdevHostAlloc(size_t bytes);
void   seeqdevHostFree(void * p);

/* Device memory for RESIDENT text, chosen by measurement: the scan kernel's time per 3.75 GiB follows the physical pages a buffer gets
 * from the driver (0.77 / 0.87 / 0.92 ms for the same text, stable for the life of the allocation), so a caller that
 * keeps text buffers resident picks each once.  Up to `candidates` (<= 12) allocations -- the plain one, then power-of-two blocks, which are
 * fast far more often -- are filled with synthetic reads and scanned; the fastest is returned, the others freed.  candidates < 2 (or a
 * buffer under 64 MiB): a plain allocation.  probe_ms (room for 12 floats) / nprobed (may be NULL): the candidates' scan-kernel times.
 * Contents undefined.
 * NULL + errno on failure.  (The reference has no device memory: an addition of this boundary, like seeqdevHostAlloc.) */
void * seeqdevTextAlloc(size_t bytes, int candidates, float * probe_ms, int * nprobed);
/* The same, telling the caller what it got: the block returned may be LARGER than `bytes` (a power-of-two block: up to 2 x bytes stay
 * allocated until seeqdevTextFree), and while the candidates are probed up to candidates x 2 x bytes + the probing scan's workspace
 * (about half a segment's bytes + 256 MiB) are held on the device -- probe_peak_bytes; other allocations of the caller may fail meanwhile. */
typedef struct seeqdev_textinfo {
   float  probe_ms[12];        /* the candidates' scan-kernel times (nprobed of them; candidate 0 = the plain allocation) */
   int    nprobed;             /* 0: nothing was probed (one candidate, a small buffer, or the probe failed: the plain allocation) */
   int    chosen;              /* index of the candidate returned */
   size_t allocated_bytes;     /* size of the allocation behind the returned pointer (>= bytes) */
   size_t probe_peak_bytes;    /* device memory held at the peak of the call */
} seeqdev_textinfo_t;
void * seeqdevTextAllocInfo(size_t bytes, int candidates, seeqdev_textinfo_t * info);
/* The same with the candidates probed by the CALLER's scan context.  The scan kernel's time is a property of the pair (text buffer, scan context's
 * workspace): one text runs at 0.72 or at 0.84 ms per 3.75 GiB with two contexts of one process, reproducibly (profiles/r05/workspace_probe.txt) --
 * so the candidate that is fastest with a context made for the probe need not be the fastest with the context that will scan the text.  `scan`: the
 * context that will (seeqdevScanReserve it first, so that its workspace is the one that stays); NULL: as seeqdevTextAllocInfo.  The context is
 * left with no scan to fetch: seeqdevScanFetch fails (EINVAL) until its next scan. */
void * seeqdevTextAllocFor(seeqdev_scan_t * scan, size_t bytes, int candidates, seeqdev_textinfo_t * info);
void   seeqdevTextFree(void * d_text);

/* Convenience: host buffer in, counts (+ records) out.  Stages through the
 * context's pinned buffer, H2D, ScanRun, ScanFetch. */
int seeqdevScanHost(seeqdev_scan_t * scan, const seeqdev_pattern_t * pat, const char * host_text, size_t nbytes,
                    int options, int want, seeqdev_counts_t * counts);

/* One string in ONE kernel launch -- what seeqStringMatch (reference libseeq.c:171-352, called once per string by
 * seeqmodule.c:858) runs on: data[0..n) is staged (short strings are read by the kernel straight from page-locked
 * host memory), scanned with `options` (libseeq.h match / non-DNA / input bits; SINGLELINE semantics) and the hits
 * land in page-locked host memory: *rec (left to right, valid until the next call on this context), *nrec. */
int seeqdevStringMatch(seeqdev_scan_t * scan, const seeqdev_pattern_t * pat, const char * data, size_t n, int options,
                       const seeqdev_hit_t ** rec, size_t * nrec);

/* The asynchronous half of seeqdevScanHost: stage (H2D on the context's stream) and enqueue the scan, return at once;
 * seeqdevScanFetch() then waits for it.  host_text must stay valid and unchanged until the fetch returns.  A reader
 * that fills the next chunk meanwhile, and one context per GPU, is how seeqFileMatch pipelines its ingest. */
int seeqdevScanHostBegin(seeqdev_scan_t * scan, const seeqdev_pattern_t * pat, const char * host_text, size_t nbytes,
                         int options, int want);
/* SEVERAL PATTERNS, ONE TEXT (barcode sets -- the demultiplexing itself is seeqdevScanRunDemux below; the reference names the multi-pattern search as the place where its
 * algorithm has parallel work, doc/response.tex:358-360, and runs one pattern per scan, seeq.c:307-437).  The text is staged
 * once (seeqdevScanHostMulti) or is already resident (seeqdevScanRunMulti).  A set of 2 .. 32 patterns that has a union
 * automaton (seeq_multi.h: barcodes of 8 .. 12 positions at distance <= 1 do, sixteen at a time) is scanned in ONE walk over
 * the text -- read-length lines, SQ_FAIL or SQ_CONVERT -- that finds the candidate (line, pattern) pairs; the exact pass
 * verifies each pair.  Every other set / text / option, and any set under SEEQ_MULTI=sequential, gets a scan per pattern over
 * the resident text, back to back on the context's stream (seeqdevScanLastMulti tells which it was).  Synchronous.
 * counts[k] (may be NULL) = pattern k's counts; with SEEQDEV_WANT_RECORDS pattern k's ordered records are kept on the host
 * (seeqdevScanMultiRecords: context-owned, valid until the next multi scan).  All patterns must live on the context's
 * device.  Results per pattern are those of a seeqdevScanRun of its own -- whichever way the set was scanned. */
int seeqdevScanRunMulti(seeqdev_scan_t * scan, const seeqdev_pattern_t * const * pats, int npat, const void * d_text, size_t nbytes,
                        int options, int want, seeqdev_counts_t * counts);
int seeqdevScanHostMulti(seeqdev_scan_t * scan, const seeqdev_pattern_t * const * pats, int npat, const char * host_text, size_t nbytes,
                         int options, int want, seeqdev_counts_t * counts);
int seeqdevScanMultiRecords(const seeqdev_scan_t * scan, int k, const seeqdev_hit_t ** rec, size_t * nrec);
int seeqdevScanLastMulti(const seeqdev_scan_t * scan);     /* 1: one walk for all patterns; 0: a scan per pattern */

/* DEMULTIPLEXING: which pattern of a set does each line belong to -- on the device, without the per-pattern records crossing
 * to the host.  The set is scanned as by seeqdevScanRunMulti (one walk when it can be, else a scan per pattern; SQ_BEST is
 * implied), and per line the pattern of smallest distance wins, the lowest index on a tie (device.py:assign_best's rule).
 * The result is one record per ASSIGNED line (a line on which at least one pattern has a record), in ascending line order,
 * kept on the device: seeqdevScanDemuxDevice (valid until the context's next scan) / seeqdevScanCopyDemux.  The bytes are
 * the same whichever way the set was scanned.  `margin` = the smallest distance among the OTHER patterns with a record on
 * the line minus the winner's, saturating at 255; 255 also means that no other pattern matched; 0 means the line is
 * ambiguous (two patterns tie at the best distance).  `options`: non-DNA mode, MASK_INPUT, SEEQDEV_FASTA, SEEQDEV_SINGLELINE
 * as in seeqdevScanRunMulti; SQ_ALL / SQ_COUNT, npat < 1 or > 255, NULL pats / pats[k] / sum give EINVAL.  Synchronous.
 * per_pattern (may be NULL): [npat] lines each pattern won.  Device memory of its own (allocated by a context's first demux,
 * freed with it): 8 bytes per line of the text and 16 per record; a set scanned pattern by pattern also orders its records
 * through the context's record workspace.  (The reference has no demultiplexer: an addition of this boundary.) */
typedef struct {
   uint32_t line;      /* 1-based, the same numbering as seeqdev_hit_t.line */
   uint32_t start;
   uint32_t end;
   uint16_t dist;      /* the winner's distance */
   uint8_t  pattern;   /* index of the winner in pats[] */
   uint8_t  margin;    /* runner-up distance - dist, saturating; 255 = none; 0 = ambiguous */
} seeqdev_demux_t;     /* 16 bytes */

typedef struct {
   uint64_t nlines;      /* counted lines, as seeqdev_counts_t.nlines */
   uint64_t nassigned;   /* records produced */
   uint64_t nambiguous;  /* of them, margin == 0 */
} seeqdev_demux_counts_t;

/* BOTH ORIENTATIONS of a barcode set: pass seeqdevPatternRevComp() members in the set beside the barcodes -- the winner's index then names
 * the strand as well as the barcode (no strand bit in seeqdev_demux_t). */
int seeqdevScanRunDemux (seeqdev_scan_t * scan, const seeqdev_pattern_t * const * pats, int npat, const void * d_text, size_t nbytes,
                         int options, seeqdev_demux_counts_t * sum, uint64_t * per_pattern);
int seeqdevScanHostDemux(seeqdev_scan_t * scan, const seeqdev_pattern_t * const * pats, int npat, const char * host_text, size_t nbytes,
                         int options, seeqdev_demux_counts_t * sum, uint64_t * per_pattern);
const seeqdev_demux_t * seeqdevScanDemuxDevice(const seeqdev_scan_t * scan);
int seeqdevScanCopyDemux(seeqdev_scan_t * scan, seeqdev_demux_t * host_out, size_t first, size_t n);

/* BOTH STRANDS IN ONE CALL.  Reads come off either strand: an adapter, primer or barcode occurs in a read as its reverse complement as
 * often as forwards.  seeqdevPatternRevComp: the reverse complement of a compiled pattern -- the positions reversed, every class
 * complemented member by member (A <-> T/U, C <-> G; N stays N) -- as a new caller-owned pattern on the same device with the same
 * distance (seeqdevPatternFree).
 * seeqdevScanRunStrands / seeqdevScanHostStrands: the text is scanned with `pat` (the PLUS strand) and with its reverse complement (MINUS;
 * built by the pattern's first such call, kept in the handle and freed with it), each scan bit-exact with the reference as every scan
 * here is, and the two record sets are merged ON THE DEVICE (seeq_strand.h):
 *   SQ_ALL               every record of both, ordered by the 64-bit key line << 32 | end, plus before minus on a tie (`end` and not
 *                        `start`: the records of a line have strictly increasing ends within a strand, while starts repeat);
 *   SQ_BEST / SQ_FIRST   one record per matching line, the winner: the smaller dist / the smaller end, plus on a tie.
 * A minus record has SEEQDEV_HIT_MINUS set in `dist` (SEEQDEV_HIT_DIST / SEEQDEV_HIT_STRAND); its start / end are positions in the line as
 * scanned.  A self-complementary pattern (GAATTC) reports every SQ_ALL hit twice, plus then minus, and wins its ties as plus.
 * counts: nlines / nheaders as either scan; nmatchlines = lines with a hit on either strand; nhits = merged hits; nrecords = merged
 * records (SEEQDEV_WANT_RECORDS), else 0.  SEEQDEV_WANT_COUNTLINES / COUNTMATCH have nothing to merge: as under SEEQDEV_FASTQ they are
 * scanned for records (SQ_FIRST / SQ_ALL; record workspace for every hit) and report nrecords = 0.  per_strand (may be NULL): [0] plus,
 * [1] minus records of the result.  Synchronous.  Afterwards seeqdevScanRecordsDevice / CopyRecords / CopyOffsets serve the merged
 * arrays, seeqdevScanFetch fails (EINVAL) until the next scan, and the context's next plain scan answers as on a fresh context.
 * `options`: match mode, non-DNA mode, SEEQDEV_FASTA, SEEQDEV_FASTQ (the two scans run unflagged and the merged records go once through
 * the filter: record numbering, nlines and offsets in the original buffer as documented above).  EINVAL, before any device call:
 * SEEQDEV_SINGLELINE, an input-mode bit (SQ_STREAM), NULL scan / pat / counts, NULL text with bytes, `want` outside 0 .. 2, a pattern on
 * another device.  E2BIG: more than 2^32 - 1 records to merge.
 * How: the pair {pat, twin} in ONE walk over the text when the pattern is barcode-sized (8 .. 12 positions at distance <= 1) and the
 * pair has a union automaton (as seeqdevScanRunMulti: read-length lines, SQ_FAIL / SQ_CONVERT), else -- and under SEEQ_MULTI=sequential -- two scans, the first one's records and offsets
 * copied aside on the device (24 bytes per record); seeqdevScanLastMulti tells which.  The bytes are the same either way.  Device memory
 * of its own (allocated by a context's first such call, freed with it): 24 bytes per record kept aside and per merged record.
 * (The reference searches one orientation per run: an addition of this boundary.) */
seeqdev_pattern_t * seeqdevPatternRevComp(const seeqdev_pattern_t * pat);
int seeqdevScanRunStrands (seeqdev_scan_t * scan, const seeqdev_pattern_t * pat, const void * d_text,    size_t nbytes, int options, int want,
                           seeqdev_counts_t * counts, uint64_t per_strand[2]);
int seeqdevScanHostStrands(seeqdev_scan_t * scan, const seeqdev_pattern_t * pat, const char * host_text, size_t nbytes, int options, int want,
                           seeqdev_counts_t * counts, uint64_t per_strand[2]);

/* Device time (ms) of the last both-strands call's merge -- its kernels and device copies, between two HIP events on the context's stream
 * (profiling on; 0 otherwise, and when there was nothing to merge). */
int seeqdevScanLastStrandsMs(const seeqdev_scan_t * scan, float * merge_ms);

/* THE INSERT BETWEEN TWO FLANKS.  What a constant sequence is most often searched for in reads: to cut out what lies next to it -- a
 * barcode, a guide, a UMI between two constant flanks (the reference's Python module ships the one-string form as matchPrefix /
 * matchSuffix).  seeqdevScanRunInserts / seeqdevScanHostInserts: the text is scanned with `right` under SQ_ALL (every occurrence; its
 * records and offsets are copied aside on the device) and with `left` under the call's match mode (SQ_BEST, what matchPrefix / matchSuffix
 * use, or SQ_FIRST: one record per matching line), each scan bit-exact with the reference as every scan here is, and the two record sets
 * are joined line by line ON THE DEVICE (seeq_insert.h):
 *   admissible           a right record R of the line of a left record L with R.start >= L.end + min_len and, when max_len != 0,
 *                        R.start <= L.end + max_len (sums in 64 bits; max_len == 0: no upper bound);
 *   chosen               SQ_BEST: the admissible record of smallest dist, the smaller end on a tie; SQ_FIRST: the one of smallest end;
 *   result               one seeqdev_insert_t per line with a left record and a chosen right record, in ascending line order, and beside
 *                        each its line's byte offset in the scanned buffer (as seeqdevScanCopyOffsets).  The insert is bytes
 *                        [start, end) of the line; start == end is an empty insert.
 * The two flanks are patterns of their own (length, distance); the same handle for both is legal.  Synchronous.  The result lives in
 * arrays of its own -- seeqdevScanInsertsDevice / seeqdevScanCopyInserts / seeqdevScanCopyInsertOffsets -- and stays valid until the
 * context's next inserts call or seeqdevScanFree.  Afterwards the context is as after a both-strands call: seeqdevScanFetch fails
 * (EINVAL) until the next scan, the next plain scan answers as on a fresh context, seeqdevScanLastRuns gives the runs of the call's
 * last scan (the left one).
 * `options`: the match mode (SQ_BEST / SQ_FIRST), the non-DNA mode, SEEQDEV_FASTA, SEEQDEV_FASTQ -- the flags go to both scans unchanged,
 * so under SEEQDEV_FASTQ only sequence lines have records, `line` is the record number and the offsets are those of the sequence lines in
 * the original buffer.  EINVAL, before any device call: SQ_ALL or SQ_COUNT as the mode, SEEQDEV_SINGLELINE, an input-mode bit
 * (SQ_STREAM), NULL scan / left / right / counts, NULL text with bytes, max_len != 0 && min_len > max_len, a pattern on another device,
 * SEEQDEV_FASTA together with SEEQDEV_FASTQ.  E2BIG: more than 2^32 - 1 records in either list.
 * ONE orientation per call: for reads off the other strand call again with left = seeqdevPatternRevComp(right) and
 * right = seeqdevPatternRevComp(left).  One-sided cuts (what lies before a right flank alone, after a left flank alone, fixed
 * columns of a line) need line lengths, which the records do not carry: seeqdevScanAnchor (CUTS AT FIXED OFFSETS below) finds them.
 * seeqdevScanInsertText: the inserts cut out of the text, on the device -- every insert's bytes followed by '\n', in record order (output
 * line k is record k; an empty insert is an empty line), ready for the next stage (a second scan, seeqdevScanRunDemux).  d_text / nbytes:
 * the text the call scanned; d_text == NULL: the context's staged text of the last seeqdevScanHostInserts (EINVAL when another host call
 * has staged over it since).  *out_bytes is always set to counts.text_bytes; out_cap < text_bytes: ERANGE, nothing is written;
 * d_out == NULL with out_cap == 0: the size query.  A record that reaches beyond nbytes: EIO.  Synchronous.
 * Device memory of its own (allocated by a context's first such call, freed with it): 24 bytes per right record kept aside (the
 * both-strands call's side copy: one owner), 16 per left record, 32 per insert.  (The reference cuts one string per call: an addition
 * of this boundary.) */
typedef struct {
   uint32_t line;    /* 1-based, numbered as seeqdev_hit_t.line */
   uint32_t start;   /* = the left record's end: first byte of the insert within the line */
   uint32_t end;     /* = the chosen right record's start, exclusive; start == end is an empty insert */
   uint16_t ldist;   /* distance of the left flank's match */
   uint16_t rdist;   /* distance of the right flank's */
} seeqdev_insert_t;  /* 16 bytes */

typedef struct {
   uint64_t nlines;      /* counted lines, as seeqdev_counts_t.nlines */
   uint64_t nleft;       /* lines with a left record */
   uint64_t nright;      /* lines with at least one right record */
   uint64_t nboth;       /* lines with both */
   uint64_t ninserts;    /* records produced; nboth - ninserts: both flanks there, in the wrong order or the wrong distance apart */
   uint64_t text_bytes;  /* sum over the records of end - start + 1: the size of the insert text */
} seeqdev_insert_counts_t;

int seeqdevScanRunInserts (seeqdev_scan_t * scan, const seeqdev_pattern_t * left, const seeqdev_pattern_t * right, const void * d_text,    size_t nbytes,
                           int options, uint32_t min_len, uint32_t max_len, seeqdev_insert_counts_t * counts);
int seeqdevScanHostInserts(seeqdev_scan_t * scan, const seeqdev_pattern_t * left, const seeqdev_pattern_t * right, const char * host_text, size_t nbytes,
                           int options, uint32_t min_len, uint32_t max_len, seeqdev_insert_counts_t * counts);
const seeqdev_insert_t * seeqdevScanInsertsDevice(const seeqdev_scan_t * scan);
int seeqdevScanCopyInserts(seeqdev_scan_t * scan, seeqdev_insert_t * host_out, size_t first, size_t n);
int seeqdevScanCopyInsertOffsets(seeqdev_scan_t * scan, uint64_t * host_out, size_t first, size_t n);
int seeqdevScanInsertText(seeqdev_scan_t * scan, const void * d_text, size_t nbytes, void * d_out, size_t out_cap, uint64_t * out_bytes);
/* Device time (ms) of the last inserts call's join -- its four launches, between two HIP events on the context's stream (profiling on; 0
 * otherwise, and when there was nothing to join). */
int seeqdevScanLastInsertsMs(const seeqdev_scan_t * scan, float * join_ms);

/* THE TALLY OF DISTINCT SPANS.  Inserts are cut in order to count them -- guide counts of a screen, barcode abundance, UMI families --
 * and the demultiplexer names the best of a few patterns per line, not how often each distinct sequence occurs.  seeqdevScanTally counts
 * the distinct sequences among the spans of a record array ON THE DEVICE (seeq_tally.h), where they lie in the resident text: no insert
 * text is gathered, nothing but the table goes to the host.
 *   source               SEEQDEV_TALLY_INSERTS: bytes [start, end) of the records of the context's last inserts call;
 *                        SEEQDEV_TALLY_HITS: bytes [start, end) of the records seeqdevScanCopyRecords serves now -- those of a plain scan
 *                        fetched with SEEQDEV_WANT_RECORDS, or of a both-strands call.  A minus-strand hit is tallied as the bytes of
 *                        the text, NOT reverse-complemented.
 *                        SEEQDEV_TALLY_GATED: the records the context's last quality gate passed (THE BASE-QUALITY GATE below).
 *                        SEEQDEV_TALLY_ANCHORED: the spans the context's last anchor call cut (CUTS AT FIXED OFFSETS below).
 *   key                  of a span of L <= SEEQDEV_TALLY_MAX_LEN bases, every byte one of ACGTUacgtu:
 *                        (1 << 2L) | sum of code(b_i) << 2(L - 1 - i), code = (ASCII >> 1) & 3 as in the packed batches below
 *                        (A 0, C 1, T/U 2, G 3).  The leading 1 carries the length: the empty span has key 1; bit 63 is never set;
 *                        no key is 0.  Lower case is tallied as its base, U as T.
 *   THE TABLE'S ORDER    one seeqdev_tally_t per distinct key, keys ascending: by length first, then base by base with A < C < T < G.
 *                        (Ordering by count is a stable argsort of the copied counts on the host.)
 *   not tallied          a span of more than 31 bases is LONG, one with another byte (N included) is FOREIGN; each kind is counted,
 *                        a span that is both counts as long.  nspans = ntallied + nlong + nforeign, and the table's counts sum to
 *                        ntallied.
 * d_text / nbytes: the text the records were found in.  d_text == NULL is legal for SEEQDEV_TALLY_INSERTS only: the context's staged
 * text of the last seeqdevScanHostInserts, as seeqdevScanInsertText (EINVAL when another host call has staged over it since).
 * Under SEEQDEV_FASTQ and after a both-strands call nothing special applies: the offsets are those of the sequence lines in the
 * original buffer.  Synchronous.  The call reads the record arrays and writes arrays of its own: the inserts result
 * (seeqdevScanInsertText included), the record arrays and the context's fetch state are afterwards what they were.  The table --
 * seeqdevScanTallyDevice / seeqdevScanCopyTally -- is valid until the context's next tally or seeqdevScanFree.
 * EINVAL, before any device call: NULL scan / counts, an unknown source, NULL text with bytes, SEEQDEV_TALLY_INSERTS without a completed
 * inserts call, SEEQDEV_TALLY_HITS without text, on a context with nothing fetched (fresh, or after a multi, demux or inserts call,
 * which leave nothing to fetch) or after a packed scan (its offsets are no offsets into a text).  EIO: a span with end < start or one
 * that reaches beyond nbytes (checked before any byte of it is loaded; the context stays usable), or an internal inconsistency.
 * E2BIG: more than 2^32 - 1 spans.
 * Device memory of its own (allocated by a context's first tally, freed with it): 17 bytes per span (two 8-byte key arrays, a
 * 1 KiB digit matrix per tile of 1 024 spans) plus 41 bytes per tile, and 16 bytes per distinct key.
 * seeqdevTallyKey / seeqdevTallyDecode: the rule's two directions on the host, no GPU needed.  Key: -1 / EINVAL for a long or foreign
 * sequence.  Decode: writes the bases in upper case by code (A C T G) and a terminating 0, returns L; -1 / EINVAL for a value that
 * is no key (0, bit 63 set, a leading 1 at an odd bit).  (The reference counts nothing: an addition of this boundary.) */
#define SEEQDEV_TALLY_INSERTS 0   /* the spans of the context's last inserts call */
#define SEEQDEV_TALLY_HITS    1   /* [start, end) of the records seeqdevScanCopyRecords would serve now */
#define SEEQDEV_TALLY_MAX_LEN 31
typedef struct {
   uint64_t key;
   uint64_t count;
} seeqdev_tally_t;   /* 16 bytes */

typedef struct {
   uint64_t nspans;      /* records of the source */
   uint64_t ntallied;    /* spans with a key: the sum of the table's counts */
   uint64_t nlong;       /* spans of more than SEEQDEV_TALLY_MAX_LEN bytes */
   uint64_t nforeign;    /* spans of at most that many with a byte that is no base */
   uint64_t ndistinct;   /* entries of the table */
   uint32_t max_len;     /* the largest tallied length */
   uint32_t passes;      /* passes of the sort: ceil((2 * max_len + 1) / 8); 0: nothing was tallied */
} seeqdev_tally_counts_t;

int seeqdevScanTally(seeqdev_scan_t * scan, int source, const void * d_text, size_t nbytes, seeqdev_tally_counts_t * counts);
const seeqdev_tally_t * seeqdevScanTallyDevice(const seeqdev_scan_t * scan);
int seeqdevScanCopyTally(seeqdev_scan_t * scan, seeqdev_tally_t * host_out, size_t first, size_t n);
/* Device time (ms) of the last tally -- its launches and counter copies, between two HIP events on the context's stream (profiling on;
 * 0 otherwise, and when there was no span). */
int seeqdevScanLastTallyMs(const seeqdev_scan_t * scan, float * ms);
int seeqdevTallyKey(const char * seq, size_t len, uint64_t * key);
int seeqdevTallyDecode(uint64_t key, char out[32]);

/* THE GROUPED TALLY: COUNTS PER (GROUP, MEMBER) PAIR.  A UMI family is a pair -- this guide seen with this UMI -- and a pooled screen is a
 * count matrix of sample x guide: every line carries TWO keys, a group and a member, and what is asked for is the count of each distinct
 * pair and, per group, its reads and its distinct members.  Two calls, both ON THE DEVICE (seeq_tally_group.h):
 *   seeqdevScanTallyHold     keeps the keys of one record array as the context's HELD COLUMN: per record its line number and its key
 *                            (0: no key).  Sources: SEEQDEV_TALLY_INSERTS and SEEQDEV_TALLY_HITS exactly as in seeqdevScanTally (the same
 *                            preconditions, the same staged text for a NULL text, the same EINVAL cases; the key is seeqdevScanTally's),
 *                            and SEEQDEV_TALLY_DEMUX: the records seeqdevScanDemuxDevice serves now -- EINVAL without a completed demux
 *                            call on the context or after a later plain or packed scan on it; the text is ignored and may be NULL; the
 *                            key is pattern + 1 (1 .. 255: key_bits <= 8, one pass of the sort); a record with margin == 0 is held
 *                            without a key and counted in nambiguous.  nspans = nheld + nlong + nforeign + nambiguous.  The column
 *                            belongs to the context: it survives scans, inserts calls, demux calls and plain tallies, and the next hold
 *                            replaces it (a failed hold leaves none).  A hold over zero records is a valid, empty column.
 *   seeqdevScanTallyGrouped  pairs the spans of SEEQDEV_TALLY_INSERTS or SEEQDEV_TALLY_HITS (anything else: EINVAL) -- the MEMBERS -- with
 *                            the held column by line and counts the distinct pairs.  EINVAL without a completed hold, before any device
 *                            call.  THE CALLER KEEPS THE LINE NUMBERING OF THE CALLS THE SAME: SEEQDEV_FASTQ in every scan or in none,
 *                            over buffers whose lines (records) number alike.  Each call takes its own text, so the held column, an
 *                            appended column (below) and the members may each come from a different buffer -- read 1 and read 2 of a
 *                            paired run, both under SEEQDEV_FASTQ: record k of one is record k of the other.
 *   group of a line          the key of the FIRST held record with that line number (a lower-bound search: several hits of a line under
 *                            SQ_ALL, the first one decides); 0 when the line has no held record or that record has no key.
 *   pair                     a member span with key m on a line of group g != 0 is the pair (g, m).  Every other span is counted in
 *                            exactly one of nlong, nforeign (decided on the member as in the plain tally, long first) and nungrouped (the
 *                            member has a key, its line has no group): nspans = npaired + nlong + nforeign + nungrouped.
 *   THE PAIR TABLE           one seeqdev_tally_pair_t per distinct pair, ordered by group, then by member, both as unsigned 64-bit
 *                            numbers (each in the plain table's order); the counts sum to npaired.  The sparse matrix in row order.
 *   THE GROUP TABLE          one seeqdev_tally_group_t per distinct group, ascending: count = its reads (the sum of its pairs' counts),
 *                            first = the rank of its first pair in the pair table, ndistinct = its distinct members -- its pairs are
 *                            entries [first, first + ndistinct).  The matrix's row index.
 *   passes                   the plain tally's sort carrying both words: ceil((2 * max_len + 1) / 8) passes over the member word (max_len:
 *                            the largest PAIRED member length), then ceil(key_bits / 8) over the group word (key_bits: the bit length of
 *                            the largest held key, which the hold reports); 0 when nothing paired.
 * Synchronous.  The grouped call reads the record arrays and the held column and writes arrays of its own (it shares the plain tally's
 * key scratch, not its table): the plain tally's table, the inserts result, the record arrays, the fetch state and the held column are
 * afterwards what they were.  Its tables -- seeqdevScanTallyPairsDevice / seeqdevScanCopyTallyPairs, seeqdevScanTallyGroupsDevice /
 * seeqdevScanCopyTallyGroups -- are valid until the context's next grouped call or seeqdevScanFree.  EIO: a span with end < start or one
 * that reaches beyond nbytes, in either call (checked before any byte of it is loaded; the context stays usable), or an internal
 * inconsistency (the message names the numbers).  E2BIG: more than 2^32 - 1 records.
 * Device memory of its own (allocated by a context's first such call, freed with it): 12 bytes per held record (line, key) plus 32 per
 * tile of 1 024; per member span 16 bytes (the two group-word arrays) beside the plain tally's 17, plus 44 per tile; 24 bytes per
 * distinct pair and 24 per distinct group.  (The reference counts nothing: an addition of this boundary.) */
#define SEEQDEV_TALLY_DEMUX 2   /* seeqdevScanTallyHold only: the records seeqdevScanDemuxDevice serves now */
typedef struct {
   uint64_t group;
   uint64_t member;
   uint64_t count;
} seeqdev_tally_pair_t;   /* 24 bytes */

typedef struct {
   uint64_t group;
   uint64_t count;       /* the group's reads */
   uint32_t first;       /* rank of its first pair in the pair table */
   uint32_t ndistinct;   /* its distinct members */
} seeqdev_tally_group_t;   /* 24 bytes */

typedef struct {
   uint64_t nspans;      /* records of the source */
   uint64_t nheld;       /* of them, held with a key */
   uint64_t nlong;       /* spans of more than SEEQDEV_TALLY_MAX_LEN bytes */
   uint64_t nforeign;    /* spans of at most that many with a byte that is no base */
   uint64_t nambiguous;  /* SEEQDEV_TALLY_DEMUX: records with margin == 0 */
   uint32_t max_len;     /* the largest held length (0 for demux records) */
   uint32_t key_bits;    /* the bit length of the largest held key */
} seeqdev_tally_hold_counts_t;   /* 48 bytes */

typedef struct {
   uint64_t nspans;      /* records of the member source */
   uint64_t npaired;     /* spans with a key on a line with a group: the sum of the pair table's counts */
   uint64_t nlong;
   uint64_t nforeign;
   uint64_t nungrouped;  /* spans with a key on a line without a group */
   uint64_t npairs;      /* entries of the pair table */
   uint64_t ngroups;     /* entries of the group table */
   uint32_t max_len;     /* the largest paired member length */
   uint32_t passes;      /* passes of the sort; 0: nothing paired */
} seeqdev_tally_grouped_counts_t;   /* 64 bytes */

int seeqdevScanTallyHold   (seeqdev_scan_t * scan, int source, const void * d_text, size_t nbytes, seeqdev_tally_hold_counts_t * counts);
int seeqdevScanTallyGrouped(seeqdev_scan_t * scan, int source, const void * d_text, size_t nbytes, seeqdev_tally_grouped_counts_t * counts);
const seeqdev_tally_pair_t  * seeqdevScanTallyPairsDevice (const seeqdev_scan_t * scan);
const seeqdev_tally_group_t * seeqdevScanTallyGroupsDevice(const seeqdev_scan_t * scan);
int seeqdevScanCopyTallyPairs (seeqdev_scan_t * scan, seeqdev_tally_pair_t  * host_out, size_t first, size_t n);
int seeqdevScanCopyTallyGroups(seeqdev_scan_t * scan, seeqdev_tally_group_t * host_out, size_t first, size_t n);
/* Device time (ms) of the last grouped call -- its launches and counter copies, between two HIP events on the context's stream (profiling
 * on; 0 otherwise, and when there was no span). */
int seeqdevScanLastTallyGroupedMs(const seeqdev_scan_t * scan, float * ms);

/* COLLAPSING UMI ERRORS IN THE GROUPED TALLY.  A UMI is random: it has no library to be counted against, so a group's ndistinct counts
 * every sequencing error in a UMI as a molecule of its own.  seeqdevScanTallyCollapse stands behind seeqdevScanTallyGrouped and says, ON
 * THE DEVICE (seeq_tally_collapse.h), per pair of the pair table whether it is a molecule of its own or an erroneous copy of another pair
 * of its group, and per group how many molecules remain.  Pair i is (g_i, m_i, c_i), m_i a tally key of length L_i:
 *   neighbour                the library's: another base at one position, the same length; a member of length 0 has none.
 *   precedes                 pair j precedes pair i iff c_j > c_i, or c_j == c_i and m_j < m_i: within a group a strict total order.
 *   candidate                of i: a pair j of the same group whose member is a neighbour of m_i, that precedes i and, under
 *                            SEEQDEV_COLLAPSE_DIRECTIONAL, has c_j >= 2 c_i - 1 (evaluated without wrap-around);
 *                            SEEQDEV_COLLAPSE_ANY drops the count threshold.
 *   parent                   i has no candidate: a ROOT, parent[i] = i.  Else ABSORBED, parent[i] = the candidate that precedes all the
 *                            others (the highest count, then the smallest member).  A parent precedes its child: the parents form a
 *                            forest.  A parent may itself be absorbed (100 - 10 - 1): THE DEVICE DOES NOT FOLLOW CHAINS, a caller who
 *                            wants family sizes does (seeq_amd.device.collapse_fold).  Of two neighbours with tied counts the smaller
 *                            member is the root: the directional rule with a deterministic tie-break, which can differ from a
 *                            breadth-first network in chains of tied pairs.
 *   THE PARENTS              one uint32_t per entry of the pair table, an index into it.
 *   THE COLLAPSE ROWS        one seeqdev_tally_collapse_t per row of the group table, row r for group row r: nroots = its molecules,
 *                            nabsorbed = its pairs that are no root, absorbed_reads = the sum of their counts;
 *                            nroots + nabsorbed == ndistinct of the group's row, and nroots >= 1.
 * Synchronous.  EINVAL, before any device call: a NULL scan or counts, an unknown rule, a context without a completed grouped call (one
 * that paired nothing is completed: the collapse of it is a valid empty result -- npairs, ngroups and every number 0, nothing launched).
 * The collapse reads the pair and group tables and writes arrays of its own: both tables, the held column, the plain tally's table, the
 * inserts result, the record arrays, the fetch state and the library are afterwards what they were.  Its result --
 * seeqdevScanTallyParentsDevice / seeqdevScanCopyTallyParents, seeqdevScanTallyCollapseDevice / seeqdevScanCopyTallyCollapse -- is valid
 * until the context's next grouped call (which clears it), the next collapse or seeqdevScanFree.  EIO: an internal inconsistency (the
 * message names the numbers; the counts are filled in).
 * Device memory of its own: 16 bytes per pair (parent, two prefixes), 16 per group, 12 per tile of 1 024 pairs, 24 per 64 pairs and 16
 * per 256 groups.  (The reference counts nothing: an addition of this boundary.) */
#define SEEQDEV_COLLAPSE_DIRECTIONAL 0
#define SEEQDEV_COLLAPSE_ANY         1

typedef struct {
   uint32_t nroots, nabsorbed;
   uint64_t absorbed_reads;
} seeqdev_tally_collapse_t;   /* 16 bytes, row r belongs to group-table row r */

typedef struct {
   uint64_t npairs, ngroups;                    /* of the grouped call */
   uint64_t nroots, nabsorbed, absorbed_reads;
   uint32_t rule, max_len;                      /* the rule applied; the grouped call's largest paired member length */
} seeqdev_tally_collapse_counts_t;   /* 48 bytes */

int seeqdevScanTallyCollapse(seeqdev_scan_t * scan, int rule, seeqdev_tally_collapse_counts_t * counts);
const uint32_t * seeqdevScanTallyParentsDevice(const seeqdev_scan_t * scan);
const seeqdev_tally_collapse_t * seeqdevScanTallyCollapseDevice(const seeqdev_scan_t * scan);
int seeqdevScanCopyTallyParents (seeqdev_scan_t * scan, uint32_t * host_out, size_t first, size_t n);
int seeqdevScanCopyTallyCollapse(seeqdev_scan_t * scan, seeqdev_tally_collapse_t * host_out, size_t first, size_t n);
/* Device time (ms) of the last collapse -- its launches and its counters copy, between two HIP events on the context's stream (profiling
 * on; 0 otherwise, and when there was no pair). */
int seeqdevScanLastTallyCollapseMs(const seeqdev_scan_t * scan, float * ms);

/* COUNTING AGAINST A KNOWN LIBRARY: EXACT, ONE MISMATCH, OR ONE EDIT.  The sequences of a screen or a barcode run are known in advance -- a guide
 * library, a whitelist -- and what is asked for is one count per library ENTRY, a read with one sequencing error counted for the entry it
 * came from.  seeqdevScanTally counts distinct OBSERVED sequences: every erroneous copy is a row of its own.  With a library set on the
 * context, a span's key is replaced ON THE DEVICE (seeq_tally_library.h) by its entry's id before the tally's sort, which then runs
 * ceil(bitlen(N) / 8) passes over ids instead of ceil((2 * max_len + 1) / 8) over sequences.
 *   seeqdevScanSetLibrary    keys[0 .. n): values of seeqdevTallyKey, pairwise distinct, lengths mixed freely.  THE ID of keys[i] is i + 1;
 *                            id 0 is "no entry".  Validated on the host before any device call: EINVAL for a NULL scan, NULL keys with
 *                            n > 0, max_mismatch outside {0, 1}, a value that is no key or a duplicate (seeqdevLastError names the
 *                            index); E2BIG for n > 2^24 - 1.  The library belongs to the context: it survives scans, inserts calls, demux
 *                            calls, plain and grouped tallies and holds; the next set call replaces it, a failed one leaves none, n == 0
 *                            clears it, seeqdevScanFree frees it.
 *   neighbour                of a key k of length L: k ^ (s << 2(L - 1 - p)), 0 <= p < L, s in {1, 2, 3} -- another base at position p.
 *                            Substitutions only: an insertion or deletion changes the length and makes no neighbour.
 *   assignment               of a span's key k: k is in the library -> its id, EXACT (even when neighbours of k are entries too).  Else,
 *                            under max_mismatch 1, with H the entries that are neighbours of k: |H| == 1 -> that id, CORRECTED;
 *                            |H| >= 2 -> 0, AMBIGUOUS; |H| == 0 -> 0, UNKNOWN.  Else, under max_mismatch 0 -> 0, UNKNOWN.  Long and
 *                            foreign spans are decided first, exactly as in seeqdevScanTally; the library never sees them.
 *                            nspans = nexact + ncorrected + nambiguous + nunknown + nlong + nforeign; nassigned = nexact + ncorrected.
 *   seeqdevScanSetLibraryMode  the same call with a MODE in place of max_mismatch: SEEQDEV_LIBRARY_EXACT (0) and SEEQDEV_LIBRARY_SUBST (1) are
 *                            max_mismatch 0 and 1, exactly; SEEQDEV_LIBRARY_EDIT (2) is ONE EDIT -- a substitution, an insertion or a deletion
 *                            (Levenshtein distance 1).  Validation, errors, lifetime and "a failed call leaves none" are
 *                            seeqdevScanSetLibrary's; a mode outside {0, 1, 2} is EINVAL before anything is read.  seeqdevScanSetLibrary
 *                            itself keeps refusing a max_mismatch other than 0 and 1.
 *   neighbours under SEEQDEV_LIBRARY_EDIT  of a key k of length L, in three classes that are disjoint because their lengths differ:
 *                            the 3 L substitutions above; the DELETIONS, length L - 1 (the read carries one base too many): base p of k
 *                            removed, taken once per run of equal bases (p == 0 or base[p] != base[p - 1]); the INSERTIONS, length L + 1
 *                            (the read lost a base): base c put in front of position p, 0 <= p <= L, taken where p == 0 or
 *                            c != base[p - 1] -- 3 L + 4 of them, and only for L <= 30.  The conditions make the neighbours of a class
 *                            pairwise distinct keys (AAAA finds the entry AAA once, not four times); the three classes together are
 *                            exactly the sequences at Levenshtein distance 1.  The assignment is the one above with H taken over all
 *                            three classes: an entry one substitution away and another one deletion away are two, AMBIGUOUS.  A corrected
 *                            span is SUBSTITUTED, INSERTED or DELETED by the class of the neighbour that was the entry: ncorrected =
 *                            nsubstituted + ninserted + ndeleted.  A 31-base entry whose read GAINED a base is a span of 32 bytes: LONG,
 *                            decided before the library sees it, and stays lost.
 *   seeqdevScanLastLibraryEdits  that split for the context's last completed assignment, of any of the three library entries
 *                            (seeqdevScanTallyLibrary, seeqdevScanTallyHoldLibrary, seeqdevScanTallyHoldAppendLibrary); all zero after a
 *                            set call, after a failed call and before any assignment; ninserted = ndeleted = 0 under modes 0 and 1.
 *                            EINVAL for a NULL argument.
 *   seeqdevScanTallyLibrary  sources, preconditions, staged text, EINVAL / EIO / E2BIG cases: seeqdevScanTally's, unchanged; EINVAL
 *                            without a library, before any device call.  THE TABLE is the context's tally table -- one seeqdev_tally_t
 *                            {key = id, count} per id that occurs, ids ascending, the counts summing to nassigned, entries without a read
 *                            absent -- served by seeqdevScanTallyDevice / seeqdevScanCopyTally and replaced by the next tally of either
 *                            kind; seeqdevScanLastTallyMs reports its time.  passes = ceil(bitlen(N) / 8), 0 when nothing was assigned.
 *   seeqdevScanTallyHoldLibrary  holds the column as seeqdevScanTallyHold does for SEEQDEV_TALLY_INSERTS / SEEQDEV_TALLY_HITS
 *                            (SEEQDEV_TALLY_DEMUX: EINVAL), then assigns it: the held key of a record is its entry's id, or 0.
 *                            key_bits = bitlen(N); ndistinct and passes are 0.  A following seeqdevScanTallyGrouped runs unchanged: its
 *                            group table has one row per library entry seen, erroneous guides folded into their entry.
 * Synchronous.  Device memory of its own: 12 bytes per library entry (key, id), 8 bytes per tile of 1 024 spans and 16 per 64 misses (24
 * under SEEQDEV_LIBRARY_EDIT);
 * the miss indices (4 bytes per miss) lie in the tally's second key array, which the sort has not touched yet (the hold call allocates
 * the plain tally's key scratch for them).  (The reference counts nothing: an addition of this boundary.) */
typedef struct {
   uint64_t nspans;      /* records of the source */
   uint64_t nassigned;   /* nexact + ncorrected: the sum of the table's counts */
   uint64_t nexact;      /* spans whose key is a library entry */
   uint64_t ncorrected;  /* spans one substitution (SEEQDEV_LIBRARY_EDIT: one edit) away from exactly one entry */
   uint64_t nambiguous;  /* ... from two or more */
   uint64_t nunknown;    /* spans with a key that is neither */
   uint64_t nlong;       /* spans of more than SEEQDEV_TALLY_MAX_LEN bytes */
   uint64_t nforeign;    /* spans of at most that many with a byte that is no base */
   uint64_t ndistinct;   /* entries of the table (the hold: 0) */
   uint32_t key_bits;    /* bitlen(N) */
   uint32_t passes;      /* passes of the sort: ceil(key_bits / 8); 0: nothing was assigned (the hold: 0) */
} seeqdev_tally_library_counts_t;   /* 80 bytes */

#define SEEQDEV_LIBRARY_EXACT 0
#define SEEQDEV_LIBRARY_SUBST 1
#define SEEQDEV_LIBRARY_EDIT  2

typedef struct {
   uint64_t nsubstituted;   /* corrected spans whose entry has their length */
   uint64_t ninserted;      /* ... is one base longer: the read lost a base */
   uint64_t ndeleted;       /* ... is one base shorter: the read carries one base too many */
   uint64_t reserved;       /* 0 */
} seeqdev_tally_library_edits_t;   /* 32 bytes */

int seeqdevScanSetLibrary(seeqdev_scan_t * scan, const uint64_t * keys, size_t n, int max_mismatch);
int seeqdevScanSetLibraryMode(seeqdev_scan_t * scan, const uint64_t * keys, size_t n, int mode);
int seeqdevScanLastLibraryEdits(const seeqdev_scan_t * scan, seeqdev_tally_library_edits_t * out);
int seeqdevScanTallyLibrary    (seeqdev_scan_t * scan, int source, const void * d_text, size_t nbytes, seeqdev_tally_library_counts_t * counts);
int seeqdevScanTallyHoldLibrary(seeqdev_scan_t * scan, int source, const void * d_text, size_t nbytes, seeqdev_tally_library_counts_t * counts);

/* KEY COLUMNS APPENDED TO THE HELD COLUMN: (CELL, GUIDE) x UMI.  Counting pipelines carry three or more keys per read -- cell barcode x
 * guide x UMI, sample x guide x UMI -- and everything behind the hold works on ONE 64-bit group word.  An append composes that word from
 * several columns ON THE DEVICE (seeq_tally_append.h); seeqdevScanTallyGrouped, seeqdevScanTallyCollapse, SEEQDEV_TALLY_GATED and the library
 * then apply unchanged: the groups are the tuples.
 *   seeqdevScanTallyHoldAppend  builds a second column N from `source` exactly as seeqdevScanTallyHold would (SEEQDEV_TALLY_INSERTS, _HITS,
 *                            _GATED, _DEMUX: the same per-record line and key, kinds, counts and EINVAL / EIO / E2BIG cases; *column is
 *                            what that hold returns) in arrays of its own.  Its WIDTH w = column->key_bits: the bit length of its largest
 *                            key, 0 when no record has one.  Then every held record i is rewritten in place:
 *                            k = the key of the FIRST record of N on the line of i (0: the line has none, or that record has no key);
 *                            key[i] = key[i] != 0 && k != 0 ? (key[i] << w) | k : 0.  Lines, record count and order do not change.  A
 *                            held record that had a key and loses it is DROPPED: nbefore = nheld + ndropped.
 *   seeqdevScanTallyHoldAppendLibrary  the same with the new column assigned to the context's library as seeqdevScanTallyHoldLibrary
 *                            assigns (sources SEEQDEV_TALLY_INSERTS, _HITS, _GATED; SEEQDEV_TALLY_DEMUX and a context without a library:
 *                            EINVAL): k is the entry's id, w = bitlen(N) of the library; *column is what that hold returns.
 *   key_bits                 afterwards the bit length of the largest composed key, computed on the device (0: nothing is left): what a
 *                            following seeqdevScanTallyGrouped takes its group passes from.
 *   THE WORD                 is injective over its columns (k < 2^w: the shift loses nothing) and COLUMN-MAJOR: in the group table's
 *                            order column 0 -- the hold's -- is most significant, then column 1, and so on.  seeqdevScanTallyHoldColumns
 *                            serves the widths, seeqdevTallySplit takes a group word apart with them (host only, no GPU).
 *   limits                   the widths sum to at most 63 bits: key_bits + w > 63 is E2BIG (the message names both numbers), decided
 *                            after N is built and before the held column is touched -- it is what it was.  A 16-base barcode (33 bits)
 *                            and a guide id (17) fit; two raw 20-base columns (41 + 41) do not: that is what the library ids are for.
 *                            At most 8 columns: a ninth append is EINVAL.  Column 0's width is the hold's key_bits at the time of the hold.
 *   w == 0                   is a valid result: every key becomes 0, nheld = 0, a following grouped call pairs nothing.
 * EINVAL, before any device call: a NULL scan, column or counts, an unknown source, a context without a completed hold (or library), a
 * ninth column, and the source's own cases.  Those, E2BIG and an EIO while N is built (a span outside its text) leave the held column and
 * its columns as they were; a device failure during the join leaves no column, as a failed hold does.  EIO after the join: an internal
 * inconsistency (the message names the numbers).  A new hold resets to one column.  Synchronous.
 * seeqdevScanCopyHeld copies records [first, first + n) of the held column -- line numbers and keys, either pointer may be NULL -- with the
 * bounds of every seeqdevScanCopy* entry (EINVAL beyond the held records; a context without a column has none).
 * Device memory of its own: 12 bytes per appended record (line, key) plus 32 per tile of 1 024, one group, freed with the context; the
 * library variant's miss indices lie where seeqdevScanTallyHoldLibrary's do.  (The reference counts nothing: an addition of this boundary.) */
typedef struct {
   uint64_t nrecords;   /* records of the held column (unchanged by the call) */
   uint64_t nbefore;    /* of them, with a key before the call */
   uint64_t nheld;      /* with a key after it */
   uint64_t ndropped;   /* nbefore - nheld */
   uint32_t width;      /* bits the appended column took */
   uint32_t key_bits;   /* bit length of the largest composed key; 0: none */
   uint32_t ncolumns;   /* columns of the held key now */
   uint32_t reserved;   /* 0 */
} seeqdev_tally_append_counts_t;   /* 48 bytes */

int seeqdevScanTallyHoldAppend       (seeqdev_scan_t * scan, int source, const void * d_text, size_t nbytes,
                                      seeqdev_tally_hold_counts_t * column, seeqdev_tally_append_counts_t * counts);
int seeqdevScanTallyHoldAppendLibrary(seeqdev_scan_t * scan, int source, const void * d_text, size_t nbytes,
                                      seeqdev_tally_library_counts_t * column, seeqdev_tally_append_counts_t * counts);
/* the widths of the held key's columns, column 0 first: returns their number (0: no column) and fills min(cap, ncolumns) of them */
int seeqdevScanTallyHoldColumns(const seeqdev_scan_t * scan, uint32_t * widths, int cap);
int seeqdevScanCopyHeld(seeqdev_scan_t * scan, uint32_t * lines_out, uint64_t * keys_out, size_t first, size_t n);
/* out[c], c < ncolumns: the key of column c in a group word.  -1 / EINVAL: 0 columns or more than 8, widths that sum to more than 63, a key
 * with bits above them, a NULL pointer. */
int seeqdevTallySplit(uint64_t key, const uint32_t * widths, int ncolumns, uint64_t * out);

/* THE TALLY OF THE HELD COLUMN ITSELF: SAMPLE x GUIDE WITH NO UMI.  The bulk pooled screen counts reads per (sample barcode, guide) and has
 * no member column: the held word a hold and its appends composed IS the key.  seeqdevScanTallyHeld counts the distinct held words, one per
 * line, ON THE DEVICE (seeq_tally_held.h), and seeqdevScanTallyHeldDense scatters the result into the dense matrix a screen wants.  It covers
 * (cell, guide) and (sample, whitelist id, guide) alike.
 *   kind of a held record    record i OPENS its line iff i == 0 or the record before it has another line number.  REPEAT: it does not open
 *                            its line.  KEYLESS: it opens its line and has key 0.  COUNTED: it opens its line and has a key.  A line is
 *                            counted at most once and its FIRST held record decides (the grouped call's rule): a line whose first record
 *                            has no key is not counted, even when a later record of it has one.  nrecords = ncounted + nkeyless + nrepeat.
 *   member_columns m         0 <= m < the held key's columns: shift = the sum of the widths of the LAST m columns
 *                            (seeqdevScanTallyHoldColumns); the row of a key is key >> shift, its column part key & ((1 << shift) - 1).
 *                            m == 0: shift 0 and no row table.
 *   THE KEY TABLE            is the context's tally table, exactly as seeqdevScanTallyLibrary's: one seeqdev_tally_t {key = the held word,
 *                            count} per distinct counted word, ascending, the counts summing to ncounted -- served by
 *                            seeqdevScanTallyDevice / seeqdevScanCopyTally and replaced by the next tally of any kind.  The sparse matrix
 *                            in row order.
 *   THE ROW TABLE            (m >= 1) one seeqdev_tally_group_t per distinct row, ascending: group = key >> shift, count = its reads,
 *                            first = the rank of its first entry in the key table, ndistinct = its entries -- [first, first + ndistinct).
 *                            Served by seeqdevScanTallyHeldRowsDevice / seeqdevScanCopyTallyHeldRows, valid until the next held tally.
 *   passes                   ceil(key_bits / 8) of the tally's single-word sort, key_bits the bit length of the largest held key (what the
 *                            hold or the last append reported); 0 when nothing is counted.  counts->key_bits: of the largest COUNTED key.
 *   seeqdevScanTallyHeldDense  d_out: nrows * ncols uint64_t of device memory, row-major, ALL of them written: zero-filled, then for every
 *                            entry of the key table with r = key >> shift and c = the column part: inside iff 1 <= r <= nrows and
 *                            1 <= c <= ncols, cell (r - 1) * ncols + (c - 1) = count.  Demux keys (pattern + 1) and library ids are
 *                            1-based: that is what the matrix is for; raw sequence columns fall outside and the sparse tables serve them.
 *                            ninside + noutside = ndistinct, inside_reads + outside_reads = ncounted.  It runs on the context's stream.
 *                            seeqdevTallyHeldCell is the same rule on the host (no GPU): 1 and *cell, 0 for a key outside, -1 / EINVAL for
 *                            a NULL cell or a shift beyond 63.
 * Both calls are synchronous.  seeqdevScanTallyHeld: EINVAL, before any device call, for a NULL scan or counts, a context without a
 * completed hold, member_columns < 0 or >= the columns of the held key.  A hold of zero records, or one with nothing counted, is a valid
 * empty result: the tables are empty and nothing is launched beyond the pack.  EIO: an internal inconsistency (seeqdevLastError names the
 * numbers).  seeqdevScanTallyHeldDense, the arguments first: EINVAL for a NULL argument and for nrows == 0 or ncols == 0, E2BIG for more than
 * SEEQDEV_TALLY_DENSE_MAX (2^28) cells; then EINVAL for a context whose tally table is not (or no longer: a plain or library tally since)
 * that of a completed held tally, and for a held tally with member_columns 0 -- all before any device call.
 * The held tally reads the held column and writes the tally's key scratch and table and arrays of its own: the held column and its columns,
 * the grouped call's two tables, the collapse's result, the inserts result, the record arrays, the fetch state, the library and the gate's
 * and the anchor's arrays are afterwards what they were.
 * Device memory of its own: 12 bytes per tile of 1 024 held records, 24 per distinct row, 12 per 256 entries of the key table (the dense
 * call), beside the plain tally's scratch and table.  (The reference counts nothing: an addition of this boundary.) */
#define SEEQDEV_TALLY_DENSE_MAX ((uint64_t)1 << 28)   /* cells of a dense matrix: 2 GiB */
typedef struct {
   uint64_t nrecords;         /* records of the held column */
   uint64_t ncounted;         /* of them: the first of their line, with a key -- the sum of the key table's counts */
   uint64_t nkeyless;         /* the first of their line, without a key */
   uint64_t nrepeat;          /* not the first of their line */
   uint64_t ndistinct;        /* entries of the key table */
   uint64_t nrows;            /* entries of the row table; 0 for member_columns 0 */
   uint32_t key_bits;         /* the bit length of the largest counted key */
   uint32_t shift;            /* bits of the column part */
   uint32_t passes;           /* passes of the sort; 0: nothing counted */
   uint32_t member_columns;
} seeqdev_tally_held_counts_t;   /* 64 bytes */

typedef struct {
   uint64_t ninside;          /* entries of the key table inside the matrix */
   uint64_t noutside;
   uint64_t inside_reads;     /* the sum of the matrix */
   uint64_t outside_reads;
} seeqdev_tally_dense_counts_t;   /* 32 bytes */

int seeqdevScanTallyHeld(seeqdev_scan_t * scan, int member_columns, seeqdev_tally_held_counts_t * counts);
const seeqdev_tally_group_t * seeqdevScanTallyHeldRowsDevice(const seeqdev_scan_t * scan);
int seeqdevScanCopyTallyHeldRows(seeqdev_scan_t * scan, seeqdev_tally_group_t * host_out, size_t first, size_t n);
int seeqdevScanTallyHeldDense(seeqdev_scan_t * scan, void * d_out, uint32_t nrows, uint32_t ncols, seeqdev_tally_dense_counts_t * counts);
/* Device time (ms) of the last held tally or dense call, whichever came last -- its launches and counter copies, between two HIP events on
 * the context's stream (profiling on; 0 otherwise, and when there was no record). */
int seeqdevScanLastTallyHeldMs(const seeqdev_scan_t * scan, float * ms);
int seeqdevTallyHeldCell(uint64_t key, uint32_t shift, uint32_t nrows, uint32_t ncols, uint64_t * cell);

/* THE BASE-QUALITY GATE -- every FASTQ counting pipeline puts a bar on the base qualities of what it counts ("drop the UMI if any base is
 * below Q", "at most k bases below Q in the barcode"): an uncertain base is what makes the spurious distinct keys, the corrected library
 * hits and the absorbed UMI pairs.  seeqdevScanQualityGate reads, ON THE DEVICE, the quality bytes under every span of a record array --
 * the fourth line of the span's FASTQ record -- and keeps the records whose span passes in arrays of its own, which
 * SEEQDEV_TALLY_GATED names as the source of seeqdevScanTally, seeqdevScanTallyLibrary, seeqdevScanTallyHold,
 * seeqdevScanTallyHoldLibrary and seeqdevScanTallyGrouped: they run unchanged over the gated records.
 *   source               SEEQDEV_TALLY_INSERTS or SEEQDEV_TALLY_HITS, with the preconditions and the NULL-text rule of seeqdevScanTally,
 *                        or SEEQDEV_TALLY_ANCHORED (CUTS AT FIXED OFFSETS below: a barcode or UMI cut by position is gated before it is
 *                        counted; the text is the one the anchored records were found in, NULL only where the anchor's own source was the
 *                        inserts, and a tally over the gated records then keeps that rule);
 *                        anything else (SEEQDEV_TALLY_GATED and SEEQDEV_TALLY_DEMUX included): EINVAL.
 *   the rule             positional, like SEEQDEV_FASTQ: nothing looks for '@' or '+'.  A span is bytes [start, end) of the line at its
 *                        offset `off`.  Its kind, decided in this order:
 *                          bad     end < start, or it reaches beyond nbytes: no byte is loaded, the call fails with EIO (the context
 *                                  stays usable);
 *                          long    more than SEEQDEV_TALLY_MAX_LEN bytes: nothing is read, it is not passed (no tally would count it);
 *                          far / misfit  with p = off + end, e1 the first '\n' at or behind p and e2 the first one behind e1, both
 *                                  searched in [p, min(nbytes, p + reach)) only: without an e2 there the span is FAR when p + reach <
 *                                  nbytes (the text goes on beyond the reach), MISFIT otherwise (the text ends first);
 *                          misfit  with q0 = e2 + 1 and seqlen = e1 - off: unless q0 + seqlen <= nbytes, and unless q0 + seqlen ==
 *                                  nbytes or text[q0 + seqlen] == '\n' (the line two below ends where a quality line of the sequence
 *                                  line's length ends: one byte probe that catches truncated and misaligned records, no validator);
 *                          low     more than max_low of the quality bytes text[q0 + start .. q0 + end) are below base + min_qual
 *                                  (unsigned bytes; '\n' and '\r' like any other);
 *                          pass    otherwise; an empty span that fits passes.
 *                        Nothing outside [0, nbytes) is read.
 *   counts               nspans == npassed + nlow + nlong + nfar + nmisfit; low_bases: the low bytes seen in passed and low spans.
 * EINVAL, before any device call: NULL scan / counts, an unknown source, NULL text with bytes, base + min_qual > 255, reach outside
 * 1 .. 65536, and seeqdevScanTally's cases for the source.  E2BIG: more than 2^32 - 1 spans.  EIO: a bad span, or an internal
 * inconsistency (the kinds must sum to nspans, the compaction must have placed npassed records).
 * Synchronous.  The call reads the source arrays and writes only its own: the record arrays, what there is to fetch, the inserts result,
 * the held column, every tally table and the library are afterwards what they were.  The gated arrays -- seeqdevScanGatedDevice /
 * seeqdevScanCopyGated (the 16-byte records unchanged: line, dist with SEEQDEV_HIT_MINUS, both distances of an insert record) /
 * seeqdevScanCopyGatedOffsets, and seeqdevScanCopyGateKinds (one kind per SOURCE record) -- are COPIES: valid across later scans and
 * inserts calls, until the context's next gate or seeqdevScanFree.  A gate that passed nothing is a result (a tally over it launches
 * nothing); without a completed gate SEEQDEV_TALLY_GATED is EINVAL.  A tally over SEEQDEV_TALLY_GATED is given the text the gated records
 * were found in; NULL is legal only when the gate's own source was the inserts: the staged text, as there.
 * Device memory of its own: 1 byte per source record, 28 bytes per tile of 1 024, 24 bytes per passed record.  (The reference reads no
 * quality line: an addition of this boundary.) */
#define SEEQDEV_TALLY_GATED 4   /* the spans the context's last quality gate passed */
#define SEEQDEV_QGATE_PASS   0  /* the kinds seeqdevScanCopyGateKinds serves */
#define SEEQDEV_QGATE_LOW    1
#define SEEQDEV_QGATE_LONG   2
#define SEEQDEV_QGATE_FAR    3
#define SEEQDEV_QGATE_MISFIT 4
typedef struct { uint64_t nspans, npassed, nlow, nlong, nfar, nmisfit, low_bases; } seeqdev_qgate_counts_t;   /* 56 bytes */
int seeqdevScanQualityGate(seeqdev_scan_t * scan, int source, const void * d_text, size_t nbytes,
                           uint32_t min_qual, uint32_t base, uint32_t max_low, uint32_t reach, seeqdev_qgate_counts_t * counts);
const seeqdev_hit_t * seeqdevScanGatedDevice(const seeqdev_scan_t * scan);
int seeqdevScanCopyGated       (seeqdev_scan_t * scan, void * host_out /* 16-byte records */, size_t first, size_t n);
int seeqdevScanCopyGatedOffsets(seeqdev_scan_t * scan, uint64_t * host_out, size_t first, size_t n);
int seeqdevScanCopyGateKinds   (seeqdev_scan_t * scan, uint8_t * host_out, size_t first, size_t n);   /* one kind per SOURCE record */
int seeqdevScanLastQualityGateMs(const seeqdev_scan_t * scan, float * ms);

/* CUTS AT FIXED OFFSETS -- most read layouts have no two flanks: a cell barcode in columns 0 .. 16 and a UMI in columns 16 .. 28 of read 1
 * have none, "the 20 bases in front of the scaffold" and "the 12 bases behind the sample barcode" have one (the reference's Python module
 * calls them matchPrefix / matchSuffix).  seeqdevScanAnchor REWRITES, ON THE DEVICE, the span of every record of a record array to a cut
 * measured from the record or from the line's start, finds the line's end where the cut needs it, and keeps the records whose cut fits in
 * arrays of its own, which SEEQDEV_TALLY_ANCHORED names as the source of seeqdevScanTally, seeqdevScanTallyLibrary, seeqdevScanTallyHold,
 * seeqdevScanTallyHoldLibrary, seeqdevScanTallyGrouped, seeqdevScanTallyHoldAppend, seeqdevScanTallyHoldAppendLibrary and
 * seeqdevScanQualityGate: they run unchanged over the anchored records.
 *   source               SEEQDEV_TALLY_INSERTS or SEEQDEV_TALLY_HITS, with the preconditions and the NULL-text rule of seeqdevScanTally;
 *                        anything else (SEEQDEV_TALLY_GATED, SEEQDEV_TALLY_DEMUX and SEEQDEV_TALLY_ANCHORED included): EINVAL.
 *   anchor, skip, len    SEEQDEV_ANCHOR_AFTER: len bytes from `skip` bytes behind the record's end; SEEQDEV_ANCHOR_BEFORE: len bytes that end
 *                        `skip` bytes in front of the record's start; SEEQDEV_ANCHOR_LINE: columns [skip, skip + len) of the line.
 *                        len == 0: as far as the line goes -- to its end (AFTER, LINE), from its start (BEFORE).
 *   the rule             positional.  The source record is (line, start, end, w) with its line offset `off`, n = nbytes, all sums in 64
 *                        bits.  Its kind:
 *                          bad     end < start, or off > n, or end > n - off: no byte is loaded, the call fails with EIO (the context
 *                                  stays usable);
 *                          BEFORE  skip > start: short.  e = start - skip; s = 0 for len == 0, else short for len > e, else e - len: kept
 *                                  (s, e).  No text byte is ever loaded in this mode.
 *                          AFTER / LINE  s = (end for AFTER, 0 for LINE) + skip, e = s + len.  len > 0 and e <= end: kept (s, e) -- the
 *                                  record vouches for [0, end) of its line, no byte is loaded.  Else p = off + end, lim = min(n, p + reach),
 *                                  i = the first '\n' in text[p, lim).  No such i and lim < n (the text goes on beyond the reach): kept
 *                                  (s, e) for len > 0, FAR for len == 0.  No such i and lim == n: L = n - off, the text's end is the
 *                                  line's end.  Else L = i - off.  len == 0: short for s > L, else e = L (s == L: an empty span, kept);
 *                                  len > 0: short for e > L.
 *                          e > 2^32 - 1: short, wherever a span would be kept.
 *                        A kept record goes out as (line, s, e, w): words 0 and 3 are the source's, untouched -- dist with
 *                        SEEQDEV_HIT_MINUS, both distances of an insert record --, its 8-byte offset beside it.  Positions are the
 *                        text's: the strand bit is carried, not interpreted.  A '\r' belongs to the line (the tally calls it foreign).
 *                        Nothing outside [0, nbytes) is read.
 *   counts               nspans == nkept + nshort + nfar; span_bytes: the sum of e - s over the kept records.  The check skip + len <=
 *                        reach guarantees that a call with len > 0 never returns FAR.
 * EINVAL, before any device call: NULL scan / counts, an unknown source or anchor, NULL text with bytes, reach outside 1 .. 65536,
 * anchor != SEEQDEV_ANCHOR_BEFORE && len > 0 && skip + len > reach, and seeqdevScanTally's cases for the source.  E2BIG: more than
 * 2^32 - 1 records.  EIO: a bad record, or an internal inconsistency (the kinds must sum to nspans, the compaction must have placed nkept
 * records).
 * Synchronous.  The call reads the source arrays and writes only its own: the record arrays, what there is to fetch, the inserts result,
 * the gated arrays, the held column, every tally table and the library are afterwards what they were -- so two anchors over the same source
 * compose: the barcode, then a hold; the UMI, then the grouped tally.  The anchored arrays -- seeqdevScanAnchoredDevice /
 * seeqdevScanCopyAnchored / seeqdevScanCopyAnchoredOffsets, and seeqdevScanCopyAnchorKinds (one kind per SOURCE record) -- are COPIES: valid
 * across later scans and inserts calls, until the context's next anchor call or seeqdevScanFree.  An anchor that kept nothing is a result;
 * without a completed anchor SEEQDEV_TALLY_ANCHORED is EINVAL.  A call over SEEQDEV_TALLY_ANCHORED is given the text the anchored records
 * were found in; NULL is legal only when the anchor's own source was the inserts: the staged text, as there.
 * LINES WITHOUT A FLANK: the pattern "N" at distance 0, fetched with records, gives the record (line, 0, 1, 0) for every line whose first
 * byte is a base (an empty line, or one that starts with another byte, has none); SEEQDEV_ANCHOR_LINE over those records cuts columns
 * [skip, skip + len) of every read.
 * Device memory of its own: 5 bytes per source record, 24 bytes per tile of 1 024, 24 bytes per kept record.  (An addition of this
 * boundary.) */
#define SEEQDEV_TALLY_ANCHORED 5   /* the spans of the context's last anchor call */
#define SEEQDEV_ANCHOR_AFTER   0   /* behind the record's end */
#define SEEQDEV_ANCHOR_BEFORE  1   /* in front of the record's start */
#define SEEQDEV_ANCHOR_LINE    2   /* from the line's first byte */
#define SEEQDEV_ANCHOR_KEPT    0   /* the kinds seeqdevScanCopyAnchorKinds serves */
#define SEEQDEV_ANCHOR_SHORT   1
#define SEEQDEV_ANCHOR_FAR     2
typedef struct { uint64_t nspans, nkept, nshort, nfar, span_bytes; } seeqdev_anchor_counts_t;   /* 40 bytes */
int seeqdevScanAnchor(seeqdev_scan_t * scan, int source, const void * d_text, size_t nbytes,
                      int anchor, uint32_t skip, uint32_t len, uint32_t reach, seeqdev_anchor_counts_t * counts);
const seeqdev_hit_t * seeqdevScanAnchoredDevice(const seeqdev_scan_t * scan);
int seeqdevScanCopyAnchored       (seeqdev_scan_t * scan, void * host_out /* 16-byte records */, size_t first, size_t n);
int seeqdevScanCopyAnchoredOffsets(seeqdev_scan_t * scan, uint64_t * host_out, size_t first, size_t n);
int seeqdevScanCopyAnchorKinds    (seeqdev_scan_t * scan, uint8_t * host_out, size_t first, size_t n);   /* one kind per SOURCE record */
int seeqdevScanLastAnchorMs(const seeqdev_scan_t * scan, float * ms);

/* PACKED READ BATCHES -- 2 bits per base instead of a byte: a quarter of the HBM (and PCIe) traffic of the ASCII scan for
 * read sets that are kept packed anyway (BAM, .2bit, a sequencer's own format).  Layout, all device pointers:
 *   bases : four bases per byte, the FIRST base of a byte in its bits 7-6; code = (ASCII >> 1) & 3, i.e. A 0, C 1, T/U 2, G 3;
 *           read r starts at bases + r * stride (stride >= ceil(read_len / 4); padding bits are ignored);
 *   nmask : optional (NULL: no N anywhere): one bit per base, first base of a byte in bit 7, set where the base is N (the
 *           2-bit code of such a base is ignored); read r at nmask + r * nstride (nstride >= ceil(read_len / 8));
 *   every read has read_len bases (1 .. 256).
 * The result is that of seeqdevScanRun over the same reads as ASCII text, one read per line ('line' of a record = read
 * index + 1), for every match option and every `want` -- the scan kernel walks the packed bytes (one read per lane, no warm-
 * up, seeq_packed.h), candidate reads are unpacked and verified by the exact pass.  Asynchronous: seeqdevScanFetch waits.
 * Any pattern: those of more than 62 positions, or without a pair automaton, are served by unpacking the batch on the device
 * (nreads * (read_len + 1) bytes of scratch) and scanning that text.  seeqdevScanCopyOffsets after a packed scan reports, per
 * record, the offset its read has in the ASCII form of the batch: (line - 1) * (read_len + 1).
 * What replaces what: the reference has no packed input; this is the boundary's batch entry for callers that do. */
typedef struct {
   const void * bases;
   const void * nmask;
   uint64_t     nreads;
   uint32_t     read_len;
   uint32_t     stride;
   uint32_t     nstride;
} seeqdev_packed_t;
int  seeqdevScanPacked(seeqdev_scan_t * scan, const seeqdev_pattern_t * pat, const seeqdev_packed_t * batch, int options, int want);
/* Host helper: ASCII reads (one per line, each exactly read_len bases of A C G T U N in either case) -> that layout, into
 * caller-provided host buffers (nmask_out may be NULL when the text holds no N: an N is then an error).  Returns the number
 * of reads, or -1 (errno EINVAL: another byte, a line of another length). */
long seeqdevPackReads(const char * text, size_t nbytes, uint32_t read_len, void * bases_out, void * nmask_out, uint32_t stride, uint32_t nstride);
/* The same device to device: d_text holds nreads lines of read_len bases + '\n' in HBM (a byte that is no base counts as N with
 * a mask, as A without).  Asynchronous on hip_stream (a hipStream_t; NULL = the null stream). */
int  seeqdevPackReadsDevice(const void * d_text, uint64_t nreads, uint32_t read_len, void * d_bases, void * d_nmask, uint32_t stride, uint32_t nstride,
                            void * hip_stream);

/* Time (ms) of that H2D copy for the last fetched scan (profiling on), from HIP events on the context's stream. */
int seeqdevScanLastCopyMs(const seeqdev_scan_t * scan, float * h2d_ms);

/* Device time (ms) of the last fetched scan, measured with HIP events recorded
 * on the scan's stream around each phase of each segment (no extra
 * synchronisation): [0] newline index, [1] forward scan = the k_forward
 * launches (the dominant kernel), [2] compaction + exact pass + records,
 * [3] total.  Sums over the segments; seeqdevScanLastLaunches() returns how
 * many k_forward launches [1] covers.  Only filled when profiling was enabled
 * with seeqdevScanSetProfiling(1) before the run. */
int seeqdevScanSetProfiling(seeqdev_scan_t * scan, int on);
int seeqdevScanLastTimes(const seeqdev_scan_t * scan, float ms[4]);
int seeqdevScanLastLaunches(const seeqdev_scan_t * scan);
/* The same per launch: the duration (ms) of each of the last run's forward-scan
 * launches, in launch order, up to `cap` of them; returns how many there were. */
int seeqdevScanLastLaunchTimes(const seeqdev_scan_t * scan, float * ms, int cap);
/* The core clock (MHz) the last run's scan launches actually ran at: the kernel's first wave reads the shader clock
 * and the constant 100 MHz counter before and after its tiles (k_pair, profiling on); 0 when not measured. */
float seeqdevScanLastClockMHz(const seeqdev_scan_t * scan);

/* Synthetic shape-R reads written straight into HBM (bench/test input; spec
 * in SURVEY.md section 8d, CPU twin in oracle/seeq_oracle.c): n lines of
 * `len` bases + '\n' for read indices [first, first+n). */
int seeqdevSynthReads(void * d_out, uint64_t first, uint64_t n, int len, const char * pattern_plain, int plen,
                      int tau, uint64_t seed, void * hip_stream);

#ifdef __cplusplus
}
#endif
#endif
