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
 * The three-launch scan shape of the project (k_scan_reduce / _top / _apply in seeq_scan.h), over tiles of
 * SEEQ_FASTQ_TILE records:
 *
 *   k_fastq_reduce   per tile: records kept, and -- independent of the compaction -- kept records that OPEN a line (input
 *                    record i does iff i == 0 or rec[i - 1].line != rec[i].line: the records of one line are contiguous),
 *                    whose total is nmatchlines.  DEMUX (the records are seeqdev_demux_t, one per line): per-pattern
 *                    tallies and the count of margin == 0 through an LDS histogram, flushed with one atomic per bin and
 *                    workgroup.
 *   k_fastq_top      one workgroup: exclusive scan of the tiles' kept counts in place; the two totals.
 *   k_fastq_apply    per tile again: the rank of a kept record = tile base + kept records of the rounds and waves before
 *                    it in the tile + its rank in the wave's ballot (mbcnt); renumbered, it is stored at that rank of the
 *                    OUTPUT arrays (never in place).  A thread owns records tile + k * 256 + tid, k = 0 .. 3: every wave
 *                    load is 1 KiB of consecutive records, every wave store a run of consecutive 16-byte slots.
 *
 * No workgroup waits on another; the grid comes from the host-known record count (none: nothing is launched).
 *
 * The rule itself -- predicate, renumbering, counted lines -- is plain C++ below, shared with the host driver
 * (tests/fastq_host_driver.cpp compiles this header with g++).
 */
#ifndef SEEQ_FASTQ_H_
#define SEEQ_FASTQ_H_

#include <stdint.h>

#define SEEQ_FASTQ_WG    256                                /* threads of a filter workgroup (4 waves) */
#define SEEQ_FASTQ_ITEMS 4                                  /* records per thread */
#define SEEQ_FASTQ_TILE  1024                               /* records per workgroup = SEEQ_FASTQ_WG * SEEQ_FASTQ_ITEMS */

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

static_assert(SEEQ_FASTQ_TILE == SEEQ_FASTQ_WG * SEEQ_FASTQ_ITEMS && SEEQ_FASTQ_WG == SEEQ_WG, "filter tile / workgroup");

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
__global__ __launch_bounds__(SEEQ_FASTQ_WG) void k_fastq_reduce(FastqArgs a)
{
   __shared__ uint32_t s_kept[SEEQ_FASTQ_WG / 64], s_open[SEEQ_FASTQ_WG / 64];
   __shared__ uint32_t s_h[DEMUX ? 257 : 1];
   if (DEMUX) {
      for (int j = threadIdx.x; j < 257; j += SEEQ_FASTQ_WG) s_h[j] = 0;
      __syncthreads();
   }
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   const uint64_t base = (uint64_t)blockIdx.x * SEEQ_FASTQ_TILE;
   uint32_t kept = 0, opened = 0;                           /* wave-uniform */
#pragma unroll
   for (int k = 0; k < SEEQ_FASTQ_ITEMS; k++) {
      const uint64_t i = base + (uint64_t)k * SEEQ_FASTQ_WG + threadIdx.x;
      uint4 r = make_uint4(0u, 0u, 0u, 0u);
      bool keep = false;
      if (i < a.n) {
         r = a.in[i];
         keep = fastq_is_sequence_line(r.x) != 0;
      }
      kept += (uint32_t)__popcll(__ballot(keep));
      if (DEMUX) {
         if (keep) {
            atomicAdd(&s_h[(r.w >> 16) & 255u], 1u);
            if ((r.w >> 24) == 0u) atomicAdd(&s_h[256], 1u);
         }
      } else {
         uint32_t prev = (uint32_t)__shfl_up((int)r.x, 1, 64);      /* lane - 1 holds record i - 1 */
         if (lane == 0 && i > 0 && i < a.n) prev = a.in[i - 1].x;
         opened += (uint32_t)__popcll(__ballot(keep && (i == 0 || prev != r.x)));
      }
   }
   if (lane == 0) { s_kept[wave] = kept; s_open[wave] = opened; }
   __syncthreads();
   if (threadIdx.x == 0) {
      kept = opened = 0;
      for (int w = 0; w < SEEQ_FASTQ_WG / 64; w++) { kept += s_kept[w]; opened += s_open[w]; }
      a.bsum[blockIdx.x] = kept;
      a.bsum[a.nb + blockIdx.x] = opened;
   }
   if (DEMUX)
      for (int j = threadIdx.x; j < 257; j += SEEQ_FASTQ_WG)
         if (s_h[j]) atomicAdd(j < 256 ? &a.cnt->per_pat[j] : &a.cnt->ambiguous, (unsigned long long)s_h[j]);
}

/* One workgroup: bsum[0 .. nb) -> its exclusive prefix, in place; the totals (both below 2^32: at most n). */
__global__ __launch_bounds__(SEEQ_FASTQ_WG) void k_fastq_top(FastqArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_FASTQ_WG / 64];
   uint32_t running = 0, opened = 0;
   for (uint32_t b0 = 0; b0 < a.nb; b0 += SEEQ_FASTQ_WG) {
      const uint32_t i = b0 + threadIdx.x;
      const uint32_t v = i < a.nb ? a.bsum[i] : 0u;
      uint32_t tot;
      const uint32_t ex = block_excl_scan(v, &tot, s_wave);
      if (i < a.nb) {
         a.bsum[i] = running + ex;
         opened += a.bsum[a.nb + i];
      }
      running += tot;
   }
   uint32_t tot_open;
   block_excl_scan(opened, &tot_open, s_wave);
   if (threadIdx.x == 0) { a.cnt->kept = running; a.cnt->opened = tot_open; }
}

__global__ __launch_bounds__(SEEQ_FASTQ_WG) void k_fastq_apply(FastqArgs a)
{
   __shared__ uint32_t s_cnt[SEEQ_FASTQ_ITEMS][SEEQ_FASTQ_WG / 64];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   const uint64_t base = (uint64_t)blockIdx.x * SEEQ_FASTQ_TILE;
   uint4 r[SEEQ_FASTQ_ITEMS];
   uint64_t off[SEEQ_FASTQ_ITEMS];
   bool keep[SEEQ_FASTQ_ITEMS];
   uint32_t within[SEEQ_FASTQ_ITEMS];                       /* kept records of the wave's round before this lane */
#pragma unroll
   for (int k = 0; k < SEEQ_FASTQ_ITEMS; k++) {
      const uint64_t i = base + (uint64_t)k * SEEQ_FASTQ_WG + threadIdx.x;
      r[k] = make_uint4(0u, 0u, 0u, 0u);
      off[k] = 0;
      keep[k] = false;
      if (i < a.n) {
         r[k] = a.in[i];
         keep[k] = fastq_is_sequence_line(r[k].x) != 0;
         if (keep[k] && a.off_in) off[k] = a.off_in[i];
      }
      const uint64_t b = __ballot(keep[k]);
      within[k] = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
      if (lane == 0) s_cnt[k][wave] = (uint32_t)__popcll(b);
   }
   __syncthreads();
   uint32_t rank0 = a.bsum[blockIdx.x];                     /* kept records before this tile, then before this round */
#pragma unroll
   for (int k = 0; k < SEEQ_FASTQ_ITEMS; k++) {
      uint32_t before = 0, tot = 0;
#pragma unroll
      for (int w = 0; w < SEEQ_FASTQ_WG / 64; w++) {
         const uint32_t c = s_cnt[k][w];
         if (w < wave) before += c;
         tot += c;
      }
      if (keep[k]) {
         const uint32_t j = rank0 + before + within[k];
         if (j < a.cap_out) {
            a.out[j] = make_uint4(fastq_record_of_line(r[k].x), r[k].y, r[k].z, r[k].w);
            if (a.off_in) a.off_out[j] = off[k];
         } else {
            atomicOr(&a.cnt->bad, 1u);
         }
      }
      rank0 += tot;
   }
}

#endif   /* __HIPCC__ */
#endif
