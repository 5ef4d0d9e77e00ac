/*
 * seeq_strand.h -- both strands in one call: the records of a scan with a pattern (PLUS) and of a scan of the same text with
 * the pattern's reverse complement (MINUS), merged into one ordered array on the device.
 *
 * The rule -- plain C++ below, shared with the host driver (tests/strand_host_driver.cpp compiles this header with g++):
 *
 *   reverse complement   of a compiled pattern (one key byte per position, seeq_pattern.h: A 0x01, C 0x02, G 0x04, T/U 0x08,
 *                        N 0x1F): position i of the result is position wlen - 1 - i of the input with bit 0 <-> bit 3 and
 *                        bit 1 <-> bit 2 swapped, bit 4 kept.  [AC] becomes [GT], N stays N, an empty class (key 0) stays empty.
 *   order                of the merged records: the 64-bit key line << 32 | end, on a tie plus before minus.  `end` and not
 *                        `start`: within one strand the records of a line under SQ_ALL have strictly increasing ends while
 *                        their starts only do not decrease, so (line, end, strand) is a total order and (line, start) is not.
 *   winner of a line     (SQ_BEST) the smaller dist, (SQ_FIRST) the smaller end; on a tie plus.  Under these modes each
 *                        strand holds at most one record per line.
 *   strand in a record   bit 31 of `dist` (SEEQDEV_HIT_MINUS, seeq_amd.h): a distance never exceeds 511.
 *
 * Both inputs are in key order and use the same line numbering (two scans of one text), so the output index of a record is
 * its own index plus its CO-RANK in the other list -- a plus record counts the minus keys < its own, a minus record the plus
 * keys <= its own -- found by a binary search: every output slot is written exactly once, by the one thread that owns the
 * input record.  No atomics on the output, no workgroup waits on another.
 *
 *   k_strand_merge    one thread per input record of either list, in the tiles of seeq_tiles.h: the search, then one 16-byte
 *                     store of the record with its strand bit and one 8-byte store of its line offset.  SQ_BEST / SQ_FIRST:
 *                     the search ends next to the other list's record of the same line, if there is one; the loser of the two
 *                     goes out with line number 0 (free: lines are 1-based).
 *   and over the MERGED array the reduce / top / apply of seeq_tiles.h:
 *   k_strand_reduce   per tile: records kept (line != 0), kept records that open a line (nmatchlines), kept records of the
 *                     minus strand.
 *   k_strand_top      one workgroup: exclusive scan of the tiles' kept counts in place; the three totals.
 *   k_strand_apply    (SQ_BEST / SQ_FIRST) the ordered compaction that drops the losers.
 *
 * The grid comes from the host-known record counts (none: nothing is launched).
 */
#ifndef SEEQ_STRAND_H_
#define SEEQ_STRAND_H_

#include <stdint.h>

#include "seeq_tiles.h"

#define SEEQ_STRAND_WG    SEEQ_TILE_WG                      /* (the host driver prints the shape under the merge's names) */
#define SEEQ_STRAND_ITEMS SEEQ_TILE_ITEMS
#define SEEQ_STRAND_TILE  SEEQ_TILE
#define SEEQ_STRAND_MINUS 0x80000000u                       /* = SEEQDEV_HIT_MINUS (seeq_amd.h) */

#define SEEQ_STRAND_FIRST 0                                 /* = SQ_FIRST, SQ_BEST, SQ_ALL (libseeq.h) */
#define SEEQ_STRAND_BEST  1
#define SEEQ_STRAND_ALL   2

#if defined(__HIPCC__)
#define SEEQ_ST_HD __host__ __device__ __forceinline__
typedef uint4 strand_rec_t;                                 /* seeqdev_hit_t as the kernels load it: x line, y start, z end, w dist */
#else
#define SEEQ_ST_HD static inline
typedef struct { uint32_t x, y, z, w; } strand_rec_t;
#endif

/* one key byte -> its complement */
SEEQ_ST_HD uint8_t strand_rc_key(uint8_t k)
{
   return (uint8_t)((k & 0x10u) | ((k & 0x01u) << 3) | ((k & 0x08u) >> 3) | ((k & 0x02u) << 1) | ((k & 0x04u) >> 1));
}

/* the compiled pattern's reverse complement; out must not overlap keys */
SEEQ_ST_HD void strand_rc_keys(const char *keys, int wlen, char *out)
{
   for (int i = 0; i < wlen; i++) out[i] = (char)strand_rc_key((uint8_t)keys[wlen - 1 - i]);
}

SEEQ_ST_HD uint64_t strand_key(uint32_t line, uint32_t end) { return ((uint64_t)line << 32) | end; }

/* records of the sorted list rec[0 .. n) whose key is < key (or_equal: <= key) */
SEEQ_ST_HD uint32_t strand_count_below(const strand_rec_t *rec, uint32_t n, uint64_t key, int or_equal)
{
   uint32_t lo = 0, hi = n;
   while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      const uint64_t k = strand_key(rec[mid].x, rec[mid].z);
      if (k < key || (or_equal && k == key)) lo = mid + 1;
      else hi = mid;
   }
   return lo;
}

/* co-rank of a plus record in the minus list / of a minus record in the plus list: on a tie plus goes first */
SEEQ_ST_HD uint32_t strand_corank_plus(const strand_rec_t *minus, uint32_t nb, uint64_t key) { return strand_count_below(minus, nb, key, 0); }
SEEQ_ST_HD uint32_t strand_corank_minus(const strand_rec_t *plus, uint32_t na, uint64_t key) { return strand_count_below(plus, na, key, 1); }

/* SQ_BEST / SQ_FIRST: does the plus record of a line win against the minus record of the same line? */
SEEQ_ST_HD int strand_plus_wins(int mode, uint32_t plus_end, uint32_t plus_dist, uint32_t minus_end, uint32_t minus_dist)
{
   return mode == SEEQ_STRAND_BEST ? plus_dist <= minus_dist : plus_end <= minus_end;
}

/* SQ_BEST / SQ_FIRST (at most one record per line in `other`): the index of the other list's record of `line`, given the
   co-rank p of a record of that line -- it sits at p or at p - 1 -- or n when the line has none there */
SEEQ_ST_HD uint32_t strand_partner(const strand_rec_t *other, uint32_t n, uint32_t p, uint32_t line)
{
   if (p < n && other[p].x == line) return p;
   if (p > 0 && other[p - 1].x == line) return p - 1;
   return n;
}

/* Where plus record i goes, and with which line number (0: it lost its line). */
SEEQ_ST_HD uint32_t strand_place_plus(int mode, const strand_rec_t *plus, uint32_t i, const strand_rec_t *minus, uint32_t nb, uint32_t *line_out)
{
   const strand_rec_t r = plus[i];
   const uint32_t p = strand_corank_plus(minus, nb, strand_key(r.x, r.z));
   *line_out = r.x;
   if (mode != SEEQ_STRAND_ALL) {
      const uint32_t q = strand_partner(minus, nb, p, r.x);
      if (q < nb && !strand_plus_wins(mode, r.z, r.w, minus[q].z, minus[q].w)) *line_out = 0;
   }
   return i + p;
}

SEEQ_ST_HD uint32_t strand_place_minus(int mode, const strand_rec_t *minus, uint32_t j, const strand_rec_t *plus, uint32_t na, uint32_t *line_out)
{
   const strand_rec_t r = minus[j];
   const uint32_t p = strand_corank_minus(plus, na, strand_key(r.x, r.z));
   *line_out = r.x;
   if (mode != SEEQ_STRAND_ALL) {
      const uint32_t q = strand_partner(plus, na, p, r.x);
      if (q < na && strand_plus_wins(mode, plus[q].z, plus[q].w, r.z, r.w)) *line_out = 0;
   }
   return j + p;
}

#if defined(__HIPCC__)

struct StrandCnt {
   uint32_t kept;                     /* merged records with a line number: the result's records */
   uint32_t opened;                   /* of them, records that open a line: lines with a hit on either strand */
   uint32_t minus;                    /* of them, records of the minus strand */
   uint32_t bad;                      /* an index outside the output (an internal error) */
};

struct StrandArgs {
   const uint4    *a;                 /* [na] plus records, in key order */
   const uint64_t *a_off;             /* [na] their line offsets */
   const uint4    *b;                 /* [nb] minus records */
   const uint64_t *b_off;
   uint32_t        na, nb;
   uint4          *mrg;               /* [cap_mrg] merged records (k_strand_merge writes, reduce / apply read) */
   uint64_t       *mrg_off;
   uint32_t        n, cap_mrg;        /* n = na + nb */
   uint4          *out;               /* [cap_out] k_strand_apply: the kept records */
   uint64_t       *off_out;
   uint32_t        cap_out;
   uint32_t        nt;                /* tiles = workgroups */
   uint32_t       *bsum;              /* [3 * nt]: per tile kept (k_strand_top: exclusive prefix), opened, minus */
   StrandCnt      *cnt;
   int             mode;              /* SEEQ_STRAND_FIRST / BEST / ALL */
};

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_strand_merge(StrandArgs a)
{
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t t = tile_index(k);
      if (t >= a.n) continue;
      uint4 r;
      uint64_t off;
      uint32_t line, j;
      if (t < a.na) {
         const uint32_t i = (uint32_t)t;
         r = a.a[i];
         off = a.a_off[i];
         j = strand_place_plus(a.mode, a.a, i, a.b, a.nb, &line);
      } else {
         const uint32_t i = (uint32_t)(t - a.na);
         r = a.b[i];
         off = a.b_off[i];
         j = strand_place_minus(a.mode, a.b, i, a.a, a.na, &line);
         r.w |= SEEQ_STRAND_MINUS;
      }
      if (j < a.cap_mrg) {
         a.mrg[j] = make_uint4(line, r.y, r.z, r.w);
         a.mrg_off[j] = off;
      } else {
         atomicOr(&a.cnt->bad, 1u);
      }
   }
}

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_strand_reduce(StrandArgs a)
{
   __shared__ uint32_t s_sum[3][SEEQ_TILE_WAVES];
   uint32_t sum[3] = {0u, 0u, 0u};                          /* kept, opened, minus: wave-uniform */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      uint4 r = make_uint4(0u, 0u, 0u, 0u);
      if (i < a.n) r = a.mrg[i];
      const bool keep = r.x != 0u;
      /* a loser's line number is 0 and a line's other record, if any, is its neighbour: a kept record opens its line iff the record before it has another number */
      const bool opens = tile_opens_line(i, r.x, a.mrg, a.n);
      sum[0] += (uint32_t)__popcll(__ballot(keep));
      sum[1] += (uint32_t)__popcll(__ballot(keep && opens));
      sum[2] += (uint32_t)__popcll(__ballot(keep && (r.w & SEEQ_STRAND_MINUS) != 0u));
   }
   tile_sums(sum, s_sum, a.bsum, a.nt);
}

/* One workgroup: bsum[0 .. nt) -> its exclusive prefix, in place; the totals (all below 2^32: at most n). */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_strand_top(StrandArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES];
   uint32_t tot[3];
   tile_top(a.bsum, a.nt, s_wave, tot);
   if (threadIdx.x == 0) { a.cnt->kept = tot[0]; a.cnt->opened = tot[1]; a.cnt->minus = tot[2]; }
}

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_strand_apply(StrandArgs a)
{
   __shared__ uint32_t s_cnt[SEEQ_TILE_ITEMS][SEEQ_TILE_WAVES];
   uint4 r[SEEQ_TILE_ITEMS];
   uint64_t off[SEEQ_TILE_ITEMS];
   bool keep[SEEQ_TILE_ITEMS];
   uint32_t within[SEEQ_TILE_ITEMS];                        /* kept records of the wave's round before this lane */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      r[k] = make_uint4(0u, 0u, 0u, 0u);
      off[k] = 0;
      if (i < a.n) {
         r[k] = a.mrg[i];
         if (r[k].x != 0u) off[k] = a.mrg_off[i];
      }
      keep[k] = r[k].x != 0u;
      within[k] = tile_wave_rank(keep[k], s_cnt[k]);
   }
   __syncthreads();
   uint32_t rank0 = a.bsum[blockIdx.x];                     /* kept records before this tile, then before this round */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint32_t j = tile_place(rank0, within[k], s_cnt[k]);
      if (!keep[k]) continue;
      if (j < a.cap_out) {
         a.out[j] = r[k];
         a.off_out[j] = off[k];
      } else {
         atomicOr(&a.cnt->bad, 1u);
      }
   }
}

#endif   /* __HIPCC__ */
#endif
