/*
 * seeq_fastq.h -- SEEQDEV_FASTQ: the records of a scan over four-line FASTQ records, reduced to those of the SEQUENCE lines
 * and numbered by record.
 *
 * The rule is positional (nothing looks for '@' or '+'): raw line 4r + 2 (1-based) is the sequence line of record r + 1.
 * Matching is per line, so the records a plain scan leaves for the sequence lines are exactly the records a scan of the
 * sequence lines alone would leave: the scan kernels run as ever, and behind them ONE ordered (stable) compaction of the
 * 16-byte records -- with their 8-byte line offsets, where the scan made them -- keeps line numbers with
 * ((line - 1) & 3) == 1 and rewrites them to ((line - 1) >> 2) + 1.
 *
 * The tile shape of seeq_tiles.h (reduce / top / apply over tiles of SEEQ_TILE records; the ranks, the sums and the top are its blocks):
 *
 *   k_fastq_reduce   per tile: records kept, and -- independent of the compaction -- kept records that OPEN a line (the records of
 *                    one line are contiguous), whose total is nmatchlines.  DEMUX (the records are seeqdev_demux_t, one per line):
 *                    per-pattern tallies and the count of margin == 0 through an LDS histogram, flushed with one atomic per bin and
 *                    workgroup.
 *   k_fastq_top      one workgroup: exclusive scan of the tiles' kept counts in place; the two totals.
 *   k_fastq_apply    per tile again: a kept record, renumbered, is stored at its rank in the OUTPUT arrays (never in place).
 *
 * The rule itself -- predicate, renumbering, counted lines -- is plain C++ below, shared with the host driver
 * (tests/fastq_host_driver.cpp compiles this header with g++).
 */
#ifndef SEEQ_FASTQ_H_
#define SEEQ_FASTQ_H_

#include <stdint.h>

#include "seeq_tiles.h"

/* the filter's own names of the shape, as numbers: the host driver prints them and tests/test_gpu_fastq.py reads them from this file */
#define SEEQ_FASTQ_WG    256
#define SEEQ_FASTQ_ITEMS 4
#define SEEQ_FASTQ_TILE  1024
static_assert(SEEQ_FASTQ_WG == SEEQ_TILE_WG && SEEQ_FASTQ_ITEMS == SEEQ_TILE_ITEMS && SEEQ_FASTQ_TILE == SEEQ_TILE, "the filter's tile is seeq_tiles.h's");

#if defined(__HIPCC__)
#define SEEQ_FQ_HD __host__ __device__ __forceinline__
#else
#define SEEQ_FQ_HD static inline
#endif

/* raw line number (1-based) -> is it the sequence line of its record? */
SEEQ_FQ_HD int fastq_is_sequence_line(uint32_t line) { return ((line - 1u) & 3u) == 1u; }
/* raw line number of a sequence line -> 1-based record number */
SEEQ_FQ_HD uint32_t fastq_record_of_line(uint32_t line) { return ((line - 1u) >> 2) + 1u; }
/* raw lines of a buffer -> records counted: a trailing partial record counts when its sequence line is there */
SEEQ_FQ_HD uint64_t fastq_nlines(uint64_t raw_lines) { return (raw_lines + 2u) >> 2; }

#if defined(__HIPCC__)

struct FastqCnt {
   unsigned long long per_pat[256];   /* DEMUX: kept records per winning pattern */
   unsigned long long ambiguous;      /* DEMUX: kept records of margin 0 */
   uint32_t kept;                     /* records kept */
   uint32_t opened;                   /* kept records that open a line: lines with a kept record */
   uint32_t bad;                      /* a rank outside the output (an internal error) */
   uint32_t pad;
};

struct FastqArgs {
   const uint4    *in;                /* [n] records (seeqdev_hit_t / seeqdev_demux_t): word 0 = raw line number */
   const uint64_t *off_in;            /* [n] their line offsets, or NULL */
   uint4          *out;               /* [cap_out] */
   uint64_t       *off_out;
   uint32_t        n, cap_out;
   uint32_t        nb;                /* tiles = workgroups */
   uint32_t       *bsum;              /* [2 * nb]: per tile kept (k_fastq_top: exclusive prefix), then per tile opened */
   FastqCnt       *cnt;
};

template <bool DEMUX>
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_fastq_reduce(FastqArgs a)
{
   __shared__ uint32_t s_sum[2][SEEQ_TILE_WAVES];
   __shared__ uint32_t s_h[DEMUX ? 257 : 1];
   if (DEMUX) {
      for (int j = threadIdx.x; j < 257; j += SEEQ_TILE_WG) s_h[j] = 0;
      __syncthreads();
   }
   uint32_t sum[2] = {0u, 0u};                              /* kept, opened: wave-uniform */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      uint4 r = make_uint4(0u, 0u, 0u, 0u);
      bool keep = false;
      if (i < a.n) {
         r = a.in[i];
         keep = fastq_is_sequence_line(r.x) != 0;
      }
      sum[0] += (uint32_t)__popcll(__ballot(keep));
      if (DEMUX) {
         if (keep) {
            atomicAdd(&s_h[(r.w >> 16) & 255u], 1u);
            if ((r.w >> 24) == 0u) atomicAdd(&s_h[256], 1u);
         }
      } else {
         const bool opens = tile_opens_line(i, r.x, a.in, a.n);
         sum[1] += (uint32_t)__popcll(__ballot(keep && opens));
      }
   }
   tile_sums(sum, s_sum, a.bsum, a.nb);
   if (DEMUX)
      for (int j = threadIdx.x; j < 257; j += SEEQ_TILE_WG)
         if (s_h[j]) atomicAdd(j < 256 ? &a.cnt->per_pat[j] : &a.cnt->ambiguous, (unsigned long long)s_h[j]);
}

/* One workgroup: bsum[0 .. nb) -> its exclusive prefix, in place; the totals (both below 2^32: at most n). */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_fastq_top(FastqArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES];
   uint32_t tot[2];
   tile_top(a.bsum, a.nb, s_wave, tot);
   if (threadIdx.x == 0) { a.cnt->kept = tot[0]; a.cnt->opened = tot[1]; }
}

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_fastq_apply(FastqArgs a)
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
      keep[k] = false;
      if (i < a.n) {
         r[k] = a.in[i];
         keep[k] = fastq_is_sequence_line(r[k].x) != 0;
         if (keep[k] && a.off_in) off[k] = a.off_in[i];
      }
      within[k] = tile_wave_rank(keep[k], s_cnt[k]);
   }
   __syncthreads();
   uint32_t rank0 = a.bsum[blockIdx.x];                     /* kept records before this tile, then before this round */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint32_t j = tile_place(rank0, within[k], s_cnt[k]);
      if (!keep[k]) continue;
      if (j < a.cap_out) {
         a.out[j] = make_uint4(fastq_record_of_line(r[k].x), r[k].y, r[k].z, r[k].w);
         if (a.off_in) a.off_out[j] = off[k];
      } else {
         atomicOr(&a.cnt->bad, 1u);
      }
   }
}

#endif   /* __HIPCC__ */
#endif
