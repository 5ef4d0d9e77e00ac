/*
 * seeq_rerun.h -- what a scan asks for first and what follows a run that came back void: the re-run policy of seeqdev_scan
 * (seeq_device.hip) as PURE host code.
 *
 * A scan is optimistic: it launches with a guessed workspace (seeq_first_reservation*) and the fastest plan; the device says in
 * Counters.overflow (OVF_*, seeq_types.h) what was too small or which kernel could not serve the text.  seeq_rerun_decide reads
 * the counters of a run and returns the verdict, the capacities to reserve before the next run and the fall-back bits the context
 * is to remember (RerunFallback: the planner's flags of the following scans, dropped again after SEEQ_RERUN_TTL of them).  Overflows
 * surface one stage at a time -- lines, hit lines, records, then the fall-backs --, so a scan may run SEEQ_RERUN_MAX_RUNS times.
 * The caller (rerun_next in seeq_device.hip) reserves and launches; nothing else there looks at an overflow bit.  No HIP in here:
 * tests/host_harness.cpp compiles it for the CPU and tests/test_kernel_core_host.py pins its numbers without a GPU.
 */
#ifndef SEEQ_RERUN_H_
#define SEEQ_RERUN_H_

#include <stddef.h>
#include <stdint.h>
#include "seeq_types.h"

static constexpr int SEEQ_RERUN_MAX_RUNS = 8;       /* the result of the last one is checked too */
static constexpr int SEEQ_RERUN_TTL = 32;
/* hit lines a scan expects: one line in 8; several patterns in one walk: one in 2 */
static constexpr int SEEQ_HL_DIV = 8, SEEQ_HL_DIV_MULTI = 2;

/* The fall-back flags of a context: the OVF_FALLBACK bits its runs have reported, and the scans left before they are dropped and
   the fast path is tried again (one text with a long line or foreign bytes must not slow a long-lived context down for good) */
struct RerunFallback {
   uint32_t bits;
   int      ttl;
   void note(uint32_t overflow) { if (overflow & OVF_FALLBACK) { bits |= overflow & OVF_FALLBACK; ttl = SEEQ_RERUN_TTL; } }
   void age() { if (bits && --ttl <= 0) bits = 0; }      /* once per scan, before it is planned */
   bool no_stream() const    { return bits & OVF_NO_STREAM; }       /* k_stream met a line it cannot address (starts > 1 GiB before its segment): use the per-line kernels */
   bool no_stream_nd() const { return bits & OVF_NONDNA; }          /* SQ_CONVERT / SQ_IGNORE: the text has non-DNA bytes, k_stream (exact for clean text only) is off */
   bool force_ll() const     { return bits & OVF_LONG_LINES; }      /* a read-length looking buffer had hits inside very long lines: use the long-line variants */
   bool no_window() const    { return bits & OVF_SEAM; }            /* k_pair's candidates: a line had candidates on both sides of a segment seam -- whole lines are scanned */
   bool no_leaders() const   { return bits & OVF_LEADER; }          /* long lines with many hits: a leader's fresh start lay inside the walk before it -- every line stays with one lane */
};

struct RerunCaps { size_t lines, hitlines, records; };

enum RerunVerdict {
   RERUN_DONE = 0,            /* the counters are the scan's result */
   RERUN_AGAIN,               /* reserve `cap`, note `note`, run again */
   RERUN_BAD_ENTRY,           /* a hit entry points outside its segment: the scan fails */
   RERUN_NOT_ONE_WALK,        /* several patterns: not k_pair's text after all -- a scan per pattern */
   RERUN_NO_CONVERGENCE       /* the last run the policy allows came back void as well */
};

struct RerunStep { RerunVerdict verdict; RerunCaps cap; uint32_t note; };

/* The capacity a re-run asks for where a workspace overflowed: what the device reported it needs, plus an eighth */
static inline size_t seeq_rerun_grown(uint64_t need) { return (size_t)need + (size_t)(need >> 3) + 64; }

/* What follows run number `run` (0 ..) of a scan whose workspace holds `cap`, given its counters `u`.  per != NULL: one walk for npat
   patterns -- u is the walk's, per[k] pattern k's exact pass: the records (and the hit lines once more) are cut into npat regions, so the
   largest need of a pattern counts npat times; only the seam flag is remembered, and text that is not k_pair's ends the walk. */
static inline RerunStep seeq_rerun_decide(int run, const RerunCaps &cap, const Counters &u, const Counters *per = NULL, int npat = 0)
{
   RerunStep d = {RERUN_AGAIN, cap, 0};
   uint32_t povf = 0, need_hl = 0;
   uint64_t need_rec = 0;
   for (int k = 0; per && k < npat; k++) {
      povf |= per[k].overflow;
      if (per[k].need_hitlines > need_hl) need_hl = per[k].need_hitlines;
      if (per[k].need_records > need_rec) need_rec = per[k].need_records;
   }
   if (u.overflow & OVF_BAD_ENTRY) { d.verdict = RERUN_BAD_ENTRY; return d; }
   if (per && (u.overflow & (OVF_NO_STREAM | OVF_NONDNA | OVF_LONG_LINES))) { d.verdict = RERUN_NOT_ONE_WALK; return d; }
   if (!u.overflow && !povf) { d.verdict = RERUN_DONE; return d; }
   /* Grow to what the device reported (plus slack for the parts it could not see). */
   const size_t hl_div = per ? SEEQ_HL_DIV_MULTI : SEEQ_HL_DIV;
   const bool lines = (u.overflow & OVF_LINES) != 0;
   if (lines) d.cap.lines = seeq_rerun_grown(u.need_lines);
   if (u.overflow & OVF_HITLINES) d.cap.hitlines = seeq_rerun_grown(u.need_hitlines);
   if (!per && (u.overflow & OVF_RECORDS)) d.cap.records = seeq_rerun_grown(u.need_records);      /* (need_records keeps counting after the overflow: the total of this run) */
   if (povf & OVF_HITLINES) { const size_t w = seeq_rerun_grown(need_hl) * (size_t)npat; if (w > d.cap.hitlines) d.cap.hitlines = w; }
   if (povf & OVF_RECORDS) { const size_t w = seeq_rerun_grown(need_rec) * (size_t)npat; if (w > d.cap.records) d.cap.records = w; }
   if (lines && d.cap.hitlines < d.cap.lines / hl_div) d.cap.hitlines = d.cap.lines / hl_div + 64;
   d.note = u.overflow & (per ? (uint32_t)OVF_SEAM : (uint32_t)OVF_FALLBACK);
   if (run >= SEEQ_RERUN_MAX_RUNS - 1) d.verdict = RERUN_NO_CONVERGENCE;
   return d;
}

/* The optimistic first workspace of an ASCII scan over segments of seg_bytes: lines average >= 32 bytes, one line in hl_div hits,
   1 record per hit line -- never less than the context has, and nothing at all where the caller sized it (user_reserved). */
static inline RerunCaps seeq_first_reservation(size_t seg_bytes, bool singleline, int hl_div, RerunCaps cap, bool user_reserved)
{
   if (user_reserved) return cap;
   const size_t guess = singleline ? 1 : seg_bytes / 32 + 1024;
   if (guess > cap.lines) cap.lines = guess;
   if (cap.lines / (size_t)hl_div + 1024 > cap.hitlines) cap.hitlines = cap.lines / (size_t)hl_div + 1024;
   /* the one-pass kernels cut the hit-line workspace into one slice per wave (<= 8 192 of them): room for 64
      entries each, or the first scan with a hit always costs a second pass */
   if (!singleline && cap.hitlines < (size_t)8192 * 64) cap.hitlines = (size_t)8192 * 64;
   if (cap.hitlines > cap.records) cap.records = cap.hitlines;
   return cap;
}

/* ... of a packed read batch scanned in segments of seg_reads: one read in eight is a candidate (no per-line arrays) */
static inline RerunCaps seeq_first_reservation_packed(size_t seg_reads, RerunCaps cap, bool user_reserved)
{
   if (user_reserved) return cap;
   if (seg_reads / 8 + 1024 > cap.hitlines) cap.hitlines = seg_reads / 8 + 1024;
   if (cap.hitlines > cap.records) cap.records = cap.hitlines;
   return cap;
}

#endif
