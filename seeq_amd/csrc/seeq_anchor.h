/*
 * seeq_anchor.h -- spans cut at fixed offsets from a hit or from the line's start: the record post-pass that REWRITES the span of every
 * record of a source (a barcode in columns 0 .. 16, "the 20 bases in front of the scaffold", "the 12 bases behind the sample barcode",
 * the whole rest of the line) and compacts the records whose cut fits into arrays of its own.  Behind it the tally family and the
 * quality gate run unchanged (SEEQDEV_TALLY_ANCHORED).
 *
 * The rule -- plain C++ below, shared with the host driver (tests/anchor_host_driver.cpp compiles this header with g++).  It is
 * positional: the source record is (line, start, end, w) with its line offset `off`, n = nbytes, all sums in 64 bits.
 *
 *   BAD      end < start or off > n or end > n - off (tally_span_kind): no byte is loaded, the call fails (EIO).
 *   BEFORE   skip > start: SHORT.  e = start - skip; s = 0 for len == 0, else SHORT for len > e, else e - len.  KEPT (s, e): no text byte
 *            is ever loaded in this mode.
 *   AFTER / LINE   s = (end for AFTER, 0 for LINE) + skip, e = s + len.
 *            len > 0 and e <= end: KEPT (s, e) -- the record vouches for [0, end) of its line, no byte is loaded.
 *            p = off + end, lim = min(n, p + reach), i = the first '\n' in text[p, lim).
 *            no such i: lim < n (the text goes on beyond the reach): KEPT (s, e) for len > 0 (skip + len <= reach, by the argument
 *                       check: the cut lies in bytes that were searched), FAR for len == 0;
 *                       lim == n: L = n - off, the text's end is the line's end.
 *            else       L = i - off.
 *            len == 0:  SHORT for s > L, else e = L (s == L: an empty span, kept).      len > 0: SHORT for e > L.
 *   e > 2^32 - 1: SHORT, wherever a span would be kept (a record's word cannot hold it).
 *   A '\r' belongs to the line.  Nothing outside [0, nbytes) is ever read.
 *
 *   anchor_span_kind  the rule byte by byte: what the tests' restatement is compared with.
 *   anchor_span_load  the same decision as the kernel takes it (compiled for the host too, where the driver holds it against
 *                     anchor_span_kind): ONE THREAD PER RECORD walks to the newline with the quality gate's walk (seeq_qgate.h: steps of
 *                     64 bytes, four unaligned 16-byte loads issued together, the exact zero-byte test on w ^ 0x0A0A0A0A gathered into a
 *                     64-bit mask, ctz; byte by byte only where 64 bytes from a step's start do not lie inside the text), the loop bounded
 *                     by the host-known ceil(reach / 64).  For len > 0 only the bytes [p, off + e) decide -- a newline among them makes
 *                     the span SHORT, none leaves it to the text's end --, so the walk stops behind them: 12 bases behind a hit are one
 *                     step, whatever the reach.
 *
 * The kernels, in the reduce / top / apply shape of seeq_tiles.h over tiles of SEEQ_TILE records:
 *   k_anchor_reduce  per tile: each record's kind, one byte AT THE RECORD'S OWN INDEX, and the end e of its cut beside it (4 bytes: the
 *                    apply never touches the text; the start follows from the record and e: anchor_start); the tile's six numbers {kept,
 *                    short, far, the kept bytes in two words (24 bits low, the rest), bad} into bsum[j * nt + tile] (tile_sums; the bad
 *                    flag through a ballot).
 *   k_anchor_top     one workgroup: row 0 -> its exclusive prefix in place; the totals (the kept bytes in 64 bits).
 *   k_anchor_apply   the ordered compaction of the KEPT records into the anchor's own arrays, never in place: (line, s, e, w) -- words 0
 *                    and 3 the source's, untouched -- and the 8-byte offset beside it.  The last tile reports where its last record went.
 * No atomics on global memory, no workgroup waits on another, one writer per output slot, every loop bounded by a host-known count, the
 * grids from host-known counts (no records: nothing is launched).
 */
#ifndef SEEQ_ANCHOR_H_
#define SEEQ_ANCHOR_H_

#include <stdint.h>

#include "seeq_qgate.h"                                     /* qgate_nl64, qgate_limit, qgate_steps; tally_span_kind, SEEQ_ST_HD */

#define SEEQ_ANCHOR_TILE   1024                             /* = SEEQ_TILE, as a number: the tests read it from this file */
static_assert(SEEQ_ANCHOR_TILE == SEEQ_TILE, "the anchor's tile is seeq_tiles.h's");

#define SEEQ_ANCHOR_AFTER  0                                /* where the cut is measured from */
#define SEEQ_ANCHOR_BEFORE 1
#define SEEQ_ANCHOR_LINE   2

#define SEEQ_ANCHOR_KEPT   0                                /* what a record's cut is */
#define SEEQ_ANCHOR_SHORT  1
#define SEEQ_ANCHOR_FAR    2
#define SEEQ_ANCHOR_BAD    3

#define SEEQ_ANCHOR_REACH_MAX SEEQ_QGATE_REACH_MAX          /* the largest reach (seeq_amd.h) */
#define SEEQ_ANCHOR_SUMS   6                                /* numbers per tile: kept, short, far, kept bytes (low 24 bits, the rest), bad */

/* KEPT (s, e), unless a record's word cannot hold e */
SEEQ_ST_HD int anchor_keep(uint64_t s, uint64_t e, uint32_t *so, uint32_t *eo)
{
   if (e > 0xFFFFFFFFull) return SEEQ_ANCHOR_SHORT;
   *so = (uint32_t)s; *eo = (uint32_t)e;
   return SEEQ_ANCHOR_KEPT;
}

/* in front of the record's start: no byte decides */
SEEQ_ST_HD int anchor_before(uint32_t start, uint32_t skip, uint32_t len, uint32_t *so, uint32_t *eo)
{
   if (skip > start) return SEEQ_ANCHOR_SHORT;
   const uint32_t e = start - skip;
   if (len > e) return SEEQ_ANCHOR_SHORT;
   return anchor_keep(len ? e - len : 0u, e, so, eo);
}

/* the cut (s, e) against a line of L bytes */
SEEQ_ST_HD int anchor_fit(uint64_t s, uint64_t e, uint32_t len, uint64_t L, uint32_t *so, uint32_t *eo)
{
   if (len == 0u) {
      if (s > L) return SEEQ_ANCHOR_SHORT;
      e = L;
   } else if (e > L) return SEEQ_ANCHOR_SHORT;
   return anchor_keep(s, e, so, eo);
}

/* the start of a kept cut from its record and its end: what k_anchor_apply writes beside e */
SEEQ_ST_HD uint32_t anchor_start(int anchor, uint32_t skip, uint32_t len, uint32_t end, uint32_t e)
{
   return anchor == SEEQ_ANCHOR_BEFORE ? (len ? e - len : 0u) : anchor == SEEQ_ANCHOR_AFTER ? end + skip : skip;
}

/* THE RULE, byte by byte.  *so, *eo: the cut of a KEPT record (0, 0 otherwise). */
SEEQ_ST_HD int anchor_span_kind(const uint8_t *text, uint64_t nbytes, uint64_t off, uint32_t start, uint32_t end, int anchor, uint32_t skip, uint32_t len,
                                uint32_t reach, uint32_t *so, uint32_t *eo)
{
   uint32_t unused;
   *so = *eo = 0u;
   if (tally_span_kind(nbytes, off, start, end, &unused) == SEEQ_TALLY_BAD) return SEEQ_ANCHOR_BAD;
   if (anchor == SEEQ_ANCHOR_BEFORE) return anchor_before(start, skip, len, so, eo);
   const uint64_t s = (anchor == SEEQ_ANCHOR_AFTER ? (uint64_t)end : 0u) + skip, e = s + len;
   if (len && e <= end) return anchor_keep(s, e, so, eo);
   const uint64_t p = off + end, lim = qgate_limit(nbytes, p, reach);
   uint64_t i = p;
   while (i < lim && text[i] != '\n') i++;
   if (i < lim) return anchor_fit(s, e, len, i - off, so, eo);
   if (lim < nbytes) return len ? anchor_keep(s, e, so, eo) : SEEQ_ANCHOR_FAR;
   return anchor_fit(s, e, len, nbytes - off, so, eo);
}

/* ---- the same decision, as the kernel takes it ---- */

/* The first newline behind p, searched in [p, min(nbytes, p + window)) in at most `steps` steps of 64 bytes (steps >= qgate_steps(window)):
   1 and *at when it is there, else 0. */
SEEQ_ST_HD int anchor_walk(const uint8_t *text, uint64_t nbytes, uint64_t p, uint32_t window, uint32_t steps, uint64_t *at)
{
   const uint64_t lim = qgate_limit(nbytes, p, window);
   *at = 0u;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
   for (uint32_t it = 0; it < steps; it++) {
      const uint64_t base = p + (uint64_t)SEEQ_QGATE_STEP * it;
      if (base >= lim) break;
      uint64_t m = qgate_nl64(text, nbytes, base);
      if (lim - base < SEEQ_QGATE_STEP) m &= (1ull << (lim - base)) - 1u;
      if (m) {
         *at = base + (uint64_t)__builtin_ctzll(m);
         return 1;
      }
   }
   return 0;
}

/* anchor_span_kind with the walk: what a thread of k_anchor_reduce does. */
SEEQ_ST_HD int anchor_span_load(const uint8_t *text, uint64_t nbytes, uint64_t off, uint32_t start, uint32_t end, int anchor, uint32_t skip, uint32_t len,
                                uint32_t reach, uint32_t steps, uint32_t *so, uint32_t *eo)
{
   uint32_t unused;
   *so = *eo = 0u;
   if (tally_span_kind(nbytes, off, start, end, &unused) == SEEQ_TALLY_BAD) return SEEQ_ANCHOR_BAD;
   if (anchor == SEEQ_ANCHOR_BEFORE) return anchor_before(start, skip, len, so, eo);
   const uint64_t s = (anchor == SEEQ_ANCHOR_AFTER ? (uint64_t)end : 0u) + skip, e = s + len;
   if (len && e <= end) return anchor_keep(s, e, so, eo);
   const uint64_t p = off + end;
   uint64_t i;
   if (len) {
      /* e - end = skip + len (less `end` from the line's start) <= reach: a newline in [p, off + e) lies inside the rule's search and is
         its first one, L < e; none there leaves the rule with a line that ends at or behind off + e, with a text that goes on beyond the
         reach (off + e <= lim < nbytes), or with the text's end */
      if (anchor_walk(text, nbytes, p, (uint32_t)(e - end), steps, &i) || e > nbytes - off) return SEEQ_ANCHOR_SHORT;
      return anchor_keep(s, e, so, eo);
   }
   if (anchor_walk(text, nbytes, p, reach, steps, &i)) return anchor_fit(s, e, 0u, i - off, so, eo);
   if ((uint64_t)reach < nbytes - p) return SEEQ_ANCHOR_FAR;
   return anchor_fit(s, e, 0u, nbytes - off, so, eo);
}

#if defined(__HIPCC__)

struct AnchorCnt {
   uint64_t span_bytes;               /* e - s over the kept records */
   uint32_t nkept, nshort, nfar;      /* records by kind */
   uint32_t bad;                      /* tiles' waves that saw a record outside the text */
   uint32_t placed;                   /* k_anchor_apply: where the last tile's last record went, + 1 */
   uint32_t pad;
};

struct AnchorArgs {
   const uint4    *rec;               /* [n] the source's records */
   const uint64_t *off;               /* [n] their line offsets */
   uint32_t        n;
   uint32_t        nt;                /* tiles = workgroups of the per-tile kernels */
   const uint8_t  *text;
   uint64_t        nbytes;
   int             anchor;
   uint32_t        skip, len, reach;
   uint32_t        steps;             /* qgate_steps(reach) */
   uint8_t        *kind;              /* [n] per source record */
   uint32_t       *end;               /* [n] per source record: the end of its cut (KEPT records) */
   uint32_t       *bsum;              /* [6 * nt] the tiles' numbers; row 0 (k_anchor_top): exclusive prefix */
   uint4          *out;               /* [nk] the kept records, rewritten */
   uint64_t       *off_out;           /* [nk] their line offsets */
   uint32_t        nk;
   AnchorCnt      *cnt;
};

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_anchor_reduce(AnchorArgs a)
{
   __shared__ uint32_t s_sum[SEEQ_ANCHOR_SUMS][SEEQ_TILE_WAVES];
   /* This lane's numbers, the three counts in fields of 10 bits (a lane has at most 4 records, a wave 256) and its kept bytes in 64 bits
      (four cuts of up to 2^32 - 1): per-lane words and one wave scan each, the four items as a loop -- the gate's shape (seeq_qgate.h),
      for the gate's reason. */
   uint32_t c_ksf = 0u;                                     /* kept | short << 10 | far << 20 */
   uint64_t bytes = 0u;
   bool bad = false;
#pragma unroll 1
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      if (i < a.n) {
         const uint4 r = a.rec[i];
         uint32_t s, e;
         const int kind = anchor_span_load(a.text, a.nbytes, a.off[i], r.y, r.z, a.anchor, a.skip, a.len, a.reach, a.steps, &s, &e);
         a.kind[i] = (uint8_t)kind;
         a.end[i] = e;
         bytes += e - s;                                    /* (0 unless kept) */
         c_ksf += kind == SEEQ_ANCHOR_KEPT ? 1u : kind == SEEQ_ANCHOR_SHORT ? 1u << 10 : kind == SEEQ_ANCHOR_FAR ? 1u << 20 : 0u;
         bad |= kind == SEEQ_ANCHOR_BAD;
      }
   }
   c_ksf = wave_incl_scan_u32(c_ksf);                       /* (the wave's sums in its last lane, the one that publishes) */
   bytes = wave_incl_scan_u64(bytes);                       /* (< 2^40: the waves' halves add up in 32 bits) */
   const uint32_t sum[SEEQ_ANCHOR_SUMS] = {c_ksf & 1023u, (c_ksf >> 10) & 1023u, c_ksf >> 20, (uint32_t)bytes & 0xFFFFFFu, (uint32_t)(bytes >> 24),
                                           __ballot(bad) != 0ull ? 1u : 0u};
   tile_sums(sum, s_sum, a.bsum, a.nt);
}

/* One workgroup: bsum[0 .. nt) -> its exclusive prefix, in place; the totals. */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_anchor_top(AnchorArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES];
   __shared__ uint64_t s_wave64[SEEQ_TILE_WAVES];
   uint32_t tot[3];
   tile_top(a.bsum, a.nt, s_wave, tot);
   uint64_t lo = 0u, hi = 0u, bad = 0u;
   for (uint32_t i = threadIdx.x; i < a.nt; i += SEEQ_TILE_WG) {
      lo += a.bsum[(size_t)3 * a.nt + i];
      hi += a.bsum[(size_t)4 * a.nt + i];
      bad += a.bsum[(size_t)5 * a.nt + i];
   }
   uint64_t tlo, thi, tbad;
   block_excl_scan(lo, &tlo, s_wave64);
   block_excl_scan(hi, &thi, s_wave64);
   block_excl_scan(bad, &tbad, s_wave64);
   if (threadIdx.x == 0) {
      a.cnt->nkept = tot[0]; a.cnt->nshort = tot[1]; a.cnt->nfar = tot[2];
      a.cnt->span_bytes = tlo + (thi << 24);
      a.cnt->bad = tbad ? 1u : 0u;
   }
}

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_anchor_apply(AnchorArgs a)
{
   __shared__ uint32_t s_cnt[SEEQ_TILE_ITEMS][SEEQ_TILE_WAVES];
   bool keep[SEEQ_TILE_ITEMS];
   uint32_t within[SEEQ_TILE_ITEMS];                        /* kept records of the wave's round before this lane */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      keep[k] = i < a.n && a.kind[i] == SEEQ_ANCHOR_KEPT;
      within[k] = tile_wave_rank(keep[k], s_cnt[k]);
   }
   __syncthreads();
   uint32_t rank0 = a.bsum[blockIdx.x];                     /* kept records before this tile, then before this round */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint32_t j = tile_place(rank0, within[k], s_cnt[k]);
      if (keep[k] && j < a.nk) {                            /* (nk is the sum of these very kinds: k_anchor_top) */
         const uint64_t i = tile_index(k);
         uint4 r = a.rec[i];
         const uint32_t e = a.end[i];
         r.y = anchor_start(a.anchor, a.skip, a.len, r.z, e);
         r.z = e;
         a.out[j] = r;
         a.off_out[j] = a.off[i];
      }
   }
   if (blockIdx.x == a.nt - 1u && threadIdx.x == 0) a.cnt->placed = rank0;
}

#endif   /* __HIPCC__ */
#endif
