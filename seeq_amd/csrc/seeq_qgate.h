/*
 * seeq_qgate.h -- the base-quality gate: which spans of a record array over FASTQ text have good enough bases to be counted, decided on
 * the device from the record's own quality line, and the records that pass compacted into arrays of the gate's own -- the one step of a
 * FASTQ counting chain that reads the fourth line of a record.  Behind it the tally family runs unchanged (SEEQDEV_TALLY_GATED).
 *
 * The rule -- plain C++ below, shared with the host driver (tests/qgate_host_driver.cpp compiles this header with g++).  It is positional,
 * like SEEQDEV_FASTQ (seeq_fastq.h): nothing looks for '@' or '+'.
 *
 *   span        bytes [start, end) of the line at `off`: words y, z of a 16-byte record and its 8-byte line offset -- the tally's span.
 *   kind        decided in this order:
 *     BAD       tally_span_kind says bad (end < start, or the span reaches beyond nbytes): no byte is loaded, the call fails (EIO).
 *     LONG      end - start > SEEQ_TALLY_LEN_MAX: nothing is read; the tally would not tally it either.
 *     FAR / MISFIT (the quality line is not found)  p = off + end; e1 = the first '\n' at or behind p, e2 = the first one behind e1, both
 *               searched in [p, min(nbytes, p + reach)) only.  Without an e2 there: FAR when p + reach < nbytes (the text goes on beyond
 *               the reach), else MISFIT (the text ends first).
 *     MISFIT    (the quality line does not fit)  q0 = e2 + 1, seqlen = e1 - off: unless q0 + seqlen <= nbytes, and unless q0 + seqlen ==
 *               nbytes or text[q0 + seqlen] == '\n' -- the line two below must end where a quality line of the sequence line's length
 *               ends.  One byte probe: it catches truncated and misaligned records; the rule is deterministic, no FASTQ validator.
 *     LOW       the quality bytes are text[q0 + start .. q0 + end); a byte b is low iff b < base + min_qual (unsigned; the sum is at most
 *               255 by the argument check; '\n' and '\r' are low like any other byte); LOW iff more than max_low of them are.
 *     PASS      otherwise; an empty span that fits passes.
 *   Nothing outside [0, nbytes) is ever read.
 *
 *   qgate_span_kind   the rule byte by byte: what the tests' restatement is compared with.
 *   qgate_span_load   the same decision as the kernel takes it (compiled for the host too, where the driver holds it against
 *                     qgate_span_kind): ONE THREAD PER RECORD walks to the two newlines in steps of 64 bytes -- four unaligned 16-byte
 *                     loads whose addresses p + 64 it, + 16, + 32, + 48 are known before any of them returns, so they are issued together
 *                     and only the decision is serial; the newlines of the 16 words through an exact zero-byte test on w ^ 0x0A0A0A0A,
 *                     gathered into one 64-bit mask (first newline: ctz; second: ctz of the mask without its lowest bit).  The loop is
 *                     bounded by the host-known ceil(reach / 64).  Then the probe byte and the span's at most 32 quality bytes in one or
 *                     two 16-byte loads issued together, tally_span_load's pattern; byte by byte where 64 (16 / 32) bytes from the first
 *                     one do not lie inside the text: the text's end.
 *
 * The kernels, in the reduce / top / apply shape of seeq_tiles.h over tiles of SEEQ_TILE records:
 *   k_qgate_reduce  per tile: each record's kind, stored as one byte AT THE RECORD'S OWN INDEX (the apply does not walk the text again);
 *                   the tile's seven numbers {passed, low, long, far, misfit, low bases seen in passed and low spans, bad} into
 *                   bsum[j * nt + tile] (tile_sums; the bad flag through a ballot).
 *   k_qgate_top     one workgroup: row 0 -> its exclusive prefix in place; the totals (the low bases in 64 bits).
 *   k_qgate_apply   the ordered compaction of the PASS records into the gate's own arrays, never in place: the 16-byte record unchanged
 *                   (line, dist with its strand bit, both distances of an insert record) and its 8-byte offset beside it.  The last tile
 *                   reports where its last record went: the host holds it against the passed count.
 * No atomics on global memory, no workgroup waits on another, one writer per output slot, every loop bounded by a host-known count, the
 * grids from host-known counts (no spans: nothing is launched).
 */
#ifndef SEEQ_QGATE_H_
#define SEEQ_QGATE_H_

#include <stdint.h>
#include <string.h>

#include "seeq_tally.h"                                     /* tally_span_kind, SEEQ_TALLY_LEN_MAX, SEEQ_ST_HD */

#define SEEQ_QGATE_TILE    1024                             /* = SEEQ_TILE, as a number: the tests read it from this file */
static_assert(SEEQ_QGATE_TILE == SEEQ_TILE, "the gate's tile is seeq_tiles.h's");

#define SEEQ_QGATE_PASS    0                                /* what a span is */
#define SEEQ_QGATE_LOW     1
#define SEEQ_QGATE_LONG    2
#define SEEQ_QGATE_FAR     3
#define SEEQ_QGATE_MISFIT  4
#define SEEQ_QGATE_BAD     5

#define SEEQ_QGATE_REACH_MAX 65536u                         /* the largest reach (seeq_amd.h) */
#define SEEQ_QGATE_STEP    64u                              /* bytes of text per step of the walk: four 16-byte loads */
#define SEEQ_QGATE_SUMS    7                                /* numbers per tile: passed, low, long, far, misfit, low bases, bad */

/* steps of the walk for a reach: the bound of its loop */
SEEQ_ST_HD uint32_t qgate_steps(uint32_t reach) { return (reach + SEEQ_QGATE_STEP - 1u) / SEEQ_QGATE_STEP; }

/* where the search for the two newlines behind p ends: min(nbytes, p + reach), p <= nbytes */
SEEQ_ST_HD uint64_t qgate_limit(uint64_t nbytes, uint64_t p, uint32_t reach) { return (uint64_t)reach < nbytes - p ? p + reach : nbytes; }

/* FAR or MISFIT for a span whose second newline was not found within the reach */
SEEQ_ST_HD int qgate_unfound(uint64_t nbytes, uint64_t p, uint32_t reach) { return (uint64_t)reach < nbytes - p ? SEEQ_QGATE_FAR : SEEQ_QGATE_MISFIT; }

/* Does the quality line at q0 fit a sequence line of seqlen bytes?  One byte probe. */
SEEQ_ST_HD int qgate_fits(const uint8_t *text, uint64_t nbytes, uint64_t q0, uint64_t seqlen)
{
   if (q0 > nbytes || seqlen > nbytes - q0) return 0;
   return q0 + seqlen == nbytes || text[q0 + seqlen] == '\n';
}

/* THE RULE, byte by byte.  *nlow: the low bytes of a span that is PASS or LOW (0 otherwise). */
SEEQ_ST_HD int qgate_span_kind(const uint8_t *text, uint64_t nbytes, uint64_t off, uint32_t start, uint32_t end, uint32_t thr, uint32_t max_low, uint32_t reach,
                               uint32_t *nlow)
{
   uint32_t len;
   *nlow = 0u;
   const int tk = tally_span_kind(nbytes, off, start, end, &len);
   if (tk == SEEQ_TALLY_BAD) return SEEQ_QGATE_BAD;
   if (tk == SEEQ_TALLY_LONG) return SEEQ_QGATE_LONG;
   const uint64_t p = off + end, lim = qgate_limit(nbytes, p, reach);
   uint64_t e1 = p, e2;
   while (e1 < lim && text[e1] != '\n') e1++;
   e2 = e1 + 1u;
   while (e2 < lim && text[e2] != '\n') e2++;
   if (e1 >= lim || e2 >= lim) return qgate_unfound(nbytes, p, reach);
   const uint64_t q0 = e2 + 1u;
   if (!qgate_fits(text, nbytes, q0, e1 - off)) return SEEQ_QGATE_MISFIT;
   uint32_t low = 0u;
   for (uint32_t i = start; i < end; i++) low += text[q0 + i] < thr;
   *nlow = low;
   return low > max_low ? SEEQ_QGATE_LOW : SEEQ_QGATE_PASS;
}

/* ---- the same decision, as the kernel takes it ---- */

/* 16 bytes at any address -> four little-endian words */
SEEQ_ST_HD void qgate_load16(const uint8_t *at, uint32_t w[4])
{
#if defined(__HIP_DEVICE_COMPILE__)
   const fused_v4u v = *(const fused_v4u_unaligned *)at;
   w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
#else
   memcpy(w, at, 16);
#endif
}

/* four packed bytes -> bits 0 .. 3: byte j == '\n' (exact: no carry runs from one byte into the next) */
SEEQ_ST_HD uint32_t qgate_nl4(uint32_t w)
{
   const uint32_t x = w ^ 0x0A0A0A0Au;
   const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);      /* 0x80 in every byte of x that is 0 */
   return (((z >> 7) * 0x00204081u) >> 21) & 15u;                                 /* bits 0, 8, 16, 24 -> bits 21 .. 24 of the product */
}

/* Bit j: text[base + j] == '\n', j < 64, for the bytes of [base, base + 64) that lie inside the text (base <= nbytes). */
SEEQ_ST_HD uint64_t qgate_nl64(const uint8_t *text, uint64_t nbytes, uint64_t base)
{
   uint64_t m = 0u;
   if (nbytes - base >= SEEQ_QGATE_STEP) {
      uint32_t w[16];
      qgate_load16(text + base, w);
      qgate_load16(text + base + 16, w + 4);
      qgate_load16(text + base + 32, w + 8);
      qgate_load16(text + base + 48, w + 12);
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int j = 0; j < 16; j++) m |= (uint64_t)qgate_nl4(w[j]) << (4 * j);
   } else {
      const uint32_t have = (uint32_t)(nbytes - base);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
      for (uint32_t j = 0; j < have; j++) m |= (uint64_t)(text[base + j] == '\n') << j;
   }
   return m;
}

/* The two newlines behind p, searched in [p, min(nbytes, p + reach)) in at most `steps` steps of 64 bytes (steps >= qgate_steps(reach)):
   1 and *e1, *e2 when both are there, else 0. */
SEEQ_ST_HD int qgate_walk(const uint8_t *text, uint64_t nbytes, uint64_t p, uint32_t reach, uint32_t steps, uint64_t *e1, uint64_t *e2)
{
   const uint64_t lim = qgate_limit(nbytes, p, reach);
   int have1 = 0;
   *e1 = *e2 = 0u;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
   for (uint32_t it = 0; it < steps; it++) {
      const uint64_t base = p + (uint64_t)SEEQ_QGATE_STEP * it;
      if (base >= lim) break;
      uint64_t m = qgate_nl64(text, nbytes, base);
      if (lim - base < SEEQ_QGATE_STEP) m &= (1ull << (lim - base)) - 1u;
      if (!have1 && m) {
         *e1 = base + (uint64_t)__builtin_ctzll(m);
         m &= m - 1u;
         have1 = 1;
      }
      if (have1 && m) {
         *e2 = base + (uint64_t)__builtin_ctzll(m);
         return 1;
      }
   }
   return 0;
}

/* two bytes in the 16-bit halves of a word, the threshold in both halves of thr2 -> bit 15 of a half: its byte is below the threshold
   (0x8000 + b - thr stays inside its half: nothing is borrowed across) */
SEEQ_ST_HD uint32_t qgate_low2(uint32_t two, uint32_t thr2) { return ~((two | 0x80008000u) - thr2) & 0x80008000u; }

/* low bytes among the first len <= 31 of the bytes held in eight little-endian words, thr <= 255: four bytes at a time, without a
   comparison per byte (31 of them keep 31 lane masks in scalar registers, and spill them) */
SEEQ_ST_HD uint32_t qgate_low_of_words(const uint32_t w[8], uint32_t len, uint32_t thr)
{
   const uint32_t thr2 = thr * 0x00010001u;
   uint32_t low = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
   for (uint32_t j = 0; j < 8u; j++) {
      const uint32_t have = len > 4u * j ? len - 4u * j : 0u;                                 /* bytes of the span in this word */
      const uint32_t x = have >= 4u ? w[j] : (w[j] | (0xFFFFFFFFu << (8u * have)));        /* the others: 0xFF, never below thr */
      low += (uint32_t)__builtin_popcount(qgate_low2(x & 0x00FF00FFu, thr2)) + (uint32_t)__builtin_popcount(qgate_low2((x >> 8) & 0x00FF00FFu, thr2));
   }
   return low;
}

/* low bytes among the len <= 31 at text[pq ..), pq + len <= nbytes: one or two 16-byte loads where they lie inside the text */
SEEQ_ST_HD uint32_t qgate_low_count(const uint8_t *text, uint64_t nbytes, uint64_t pq, uint32_t len, uint32_t thr)
{
   if (len == 0u) return 0u;
   const uint32_t nvec = len > 16u ? 2u : 1u;
   if (nbytes - pq >= 16u * nvec) {
      uint32_t w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
      qgate_load16(text + pq, w);
      if (nvec == 2u) qgate_load16(text + pq + 16, w + 4);
      return qgate_low_of_words(w, len, thr);
   }
   uint32_t low = 0u;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
   for (uint32_t i = 0; i < len; i++) low += text[pq + i] < thr;
   return low;
}

/* qgate_span_kind with the walk and the wide loads: what a thread of k_qgate_reduce does. */
SEEQ_ST_HD int qgate_span_load(const uint8_t *text, uint64_t nbytes, uint64_t off, uint32_t start, uint32_t end, uint32_t thr, uint32_t max_low, uint32_t reach,
                               uint32_t steps, uint32_t *nlow)
{
   uint32_t len;
   *nlow = 0u;
   const int tk = tally_span_kind(nbytes, off, start, end, &len);
   if (tk == SEEQ_TALLY_BAD) return SEEQ_QGATE_BAD;
   if (tk == SEEQ_TALLY_LONG) return SEEQ_QGATE_LONG;
   const uint64_t p = off + end;
   uint64_t e1, e2;
   if (!qgate_walk(text, nbytes, p, reach, steps, &e1, &e2)) return qgate_unfound(nbytes, p, reach);
   const uint64_t q0 = e2 + 1u, seqlen = e1 - off;         /* (q0 <= nbytes: e2 lies inside the text) */
   if (seqlen > nbytes - q0) return SEEQ_QGATE_MISFIT;
   /* qgate_fits' probe and the quality bytes (inside the text now: end <= seqlen) are loaded together, the probe decides afterwards */
   const uint8_t probe = q0 + seqlen == nbytes ? (uint8_t)'\n' : text[q0 + seqlen];
   const uint32_t low = qgate_low_count(text, nbytes, q0 + start, len, thr);
   if (probe != '\n') return SEEQ_QGATE_MISFIT;
   *nlow = low;
   return low > max_low ? SEEQ_QGATE_LOW : SEEQ_QGATE_PASS;
}

#if defined(__HIPCC__)

struct QGateCnt {
   uint64_t low_bases;                /* low bases seen in passed and low spans */
   uint32_t npassed, nlow, nlong, nfar, nmisfit;      /* spans by kind */
   uint32_t bad;                      /* tiles' waves that saw a span outside the text */
   uint32_t placed;                   /* k_qgate_apply: where the last tile's last record went, + 1 */
   uint32_t pad;
};

struct QGateArgs {
   const uint4    *rec;               /* [n] the source's records */
   const uint64_t *off;               /* [n] their line offsets */
   uint32_t        n;
   uint32_t        nt;                /* tiles = workgroups of the per-tile kernels */
   const uint8_t  *text;
   uint64_t        nbytes;
   uint32_t        thr;               /* base + min_qual: a byte below it is low */
   uint32_t        max_low, reach;
   uint32_t        steps;             /* qgate_steps(reach) */
   uint8_t        *kind;              /* [n] per source record */
   uint32_t       *bsum;              /* [7 * nt] the tiles' numbers; row 0 (k_qgate_top): exclusive prefix */
   uint4          *out;               /* [np] the passed records */
   uint64_t       *off_out;           /* [np] their line offsets */
   uint32_t        np;
   QGateCnt       *cnt;
};

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_qgate_reduce(QGateArgs a)
{
   __shared__ uint32_t s_sum[SEEQ_QGATE_SUMS][SEEQ_TILE_WAVES];
   /* This lane's numbers, the five counts in fields of 10 bits (a lane has at most 4 spans, a wave 256): wave-uniform accumulators beside
      the walk's divergent loop spill scalar registers, and so do four unrolled copies of that loop. */
   uint32_t c_plo = 0u, c_fm = 0u, lowb = 0u;               /* passed | low << 10 | long << 20; far | misfit << 10; low bases */
   bool bad = false;
#pragma unroll 1
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      if (i < a.n) {
         const uint4 r = a.rec[i];
         uint32_t nlow;
         const int kind = qgate_span_load(a.text, a.nbytes, a.off[i], r.y, r.z, a.thr, a.max_low, a.reach, a.steps, &nlow);
         a.kind[i] = (uint8_t)kind;
         lowb += nlow;
         c_plo += kind == SEEQ_QGATE_PASS ? 1u : kind == SEEQ_QGATE_LOW ? 1u << 10 : kind == SEEQ_QGATE_LONG ? 1u << 20 : 0u;
         c_fm += kind == SEEQ_QGATE_FAR ? 1u : kind == SEEQ_QGATE_MISFIT ? 1u << 10 : 0u;
         bad |= kind == SEEQ_QGATE_BAD;
      }
   }
   c_plo = wave_incl_scan_u32(c_plo);                       /* (the wave's sums in its last lane, the one that publishes) */
   c_fm = wave_incl_scan_u32(c_fm);
   lowb = wave_incl_scan_u32(lowb);
   const uint32_t sum[SEEQ_QGATE_SUMS] = {c_plo & 1023u, (c_plo >> 10) & 1023u, c_plo >> 20, c_fm & 1023u, c_fm >> 10, lowb,
                                          __ballot(bad) != 0ull ? 1u : 0u};
   tile_sums(sum, s_sum, a.bsum, a.nt);
}

/* One workgroup: bsum[0 .. nt) -> its exclusive prefix, in place; the totals. */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_qgate_top(QGateArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES];
   __shared__ uint64_t s_wave64[SEEQ_TILE_WAVES];
   uint32_t tot[5];
   tile_top(a.bsum, a.nt, s_wave, tot);
   uint64_t low = 0u, bad = 0u;
   for (uint32_t i = threadIdx.x; i < a.nt; i += SEEQ_TILE_WG) {
      low += a.bsum[(size_t)5 * a.nt + i];
      bad += a.bsum[(size_t)6 * a.nt + i];
   }
   uint64_t tlow, tbad;
   block_excl_scan(low, &tlow, s_wave64);
   block_excl_scan(bad, &tbad, s_wave64);
   if (threadIdx.x == 0) {
      a.cnt->npassed = tot[0]; a.cnt->nlow = tot[1]; a.cnt->nlong = tot[2]; a.cnt->nfar = tot[3]; a.cnt->nmisfit = tot[4];
      a.cnt->low_bases = tlow;
      a.cnt->bad = tbad ? 1u : 0u;
   }
}

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_qgate_apply(QGateArgs a)
{
   __shared__ uint32_t s_cnt[SEEQ_TILE_ITEMS][SEEQ_TILE_WAVES];
   bool keep[SEEQ_TILE_ITEMS];
   uint32_t within[SEEQ_TILE_ITEMS];                        /* passed records of the wave's round before this lane */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      keep[k] = i < a.n && a.kind[i] == SEEQ_QGATE_PASS;
      within[k] = tile_wave_rank(keep[k], s_cnt[k]);
   }
   __syncthreads();
   uint32_t rank0 = a.bsum[blockIdx.x];                     /* passed records before this tile, then before this round */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint32_t j = tile_place(rank0, within[k], s_cnt[k]);
      if (keep[k] && j < a.np) {                            /* (np is the sum of these very kinds: k_qgate_top) */
         const uint64_t i = tile_index(k);
         a.out[j] = a.rec[i];
         a.off_out[j] = a.off[i];
      }
   }
   if (blockIdx.x == a.nt - 1u && threadIdx.x == 0) a.cnt->placed = rank0;
}

#endif   /* __HIPCC__ */
#endif
