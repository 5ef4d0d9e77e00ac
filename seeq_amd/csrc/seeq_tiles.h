/*
 * seeq_tiles.h -- the tile shape of the post-passes over 16-byte records, once: the FASTQ filter (seeq_fastq.h), the both-strands merge
 * (seeq_strand.h), the insert join (seeq_insert.h) and the tally's run-length pass (seeq_tally.h) are all the three-launch scan shape of
 * the project (k_scan_reduce / _top / _apply in seeq_scan.h) over tiles of SEEQ_TILE records, and a new record post-pass starts from here.
 *
 *   reduce   per tile: N counts -- the first one of the items kept, the others tallies of the kernel's own -- summed per wave with ballots
 *            (wave-uniform values) and over the waves through LDS into bsum[j * nt + tile], j < N (tile_sums).
 *   top      one workgroup: row 0 of bsum -> its exclusive prefix in place, 256 tiles at a time; the totals of all N rows (tile_top).
 *   apply    per tile again: the kernel recomputes its keep flags, and the output index of a kept item = tile base (row 0 of bsum) + kept
 *            items of the rounds and waves before it in the tile (the waves' counts per round, through LDS) + its rank in the wave's ballot
 *            (mbcnt).  Stored at that index of the OUTPUT arrays (never in place), the items keep their order.  The ranks are two calls
 *            per round around the kernel's one barrier: tile_wave_rank in the round that loads the item, tile_place in the round that
 *            stores it (per round, so that the compiler keeps the rounds apart: all four at once cost twice the registers).
 *
 * A thread owns items tile + k * 256 + tid, k = 0 .. 3 (tile_index): every wave load of 16-byte records is 1 KiB of consecutive records,
 * every wave store a run of consecutive slots.  No workgroup waits on another; the grid comes from the host-known item count.
 *
 * The blocks know nothing of their callers: a kernel is its own predicate, its own transform of the stored record and its own extra
 * tallies around calls to them.  The LDS they work in is the caller's (as block_excl_scan's, seeq_scan_common.h).
 */
#ifndef SEEQ_TILES_H_
#define SEEQ_TILES_H_

#include <stdint.h>

#define SEEQ_TILE_WG    256                                 /* threads of a workgroup (4 waves) */
#define SEEQ_TILE_ITEMS 4                                   /* items per thread */
#define SEEQ_TILE       1024                                /* items per workgroup = SEEQ_TILE_WG * SEEQ_TILE_ITEMS */

/* tiles (= workgroups) of n items */
static inline uint64_t seeq_tiles_of(uint64_t n) { return (n + SEEQ_TILE - 1) / SEEQ_TILE; }

#if defined(__HIPCC__)

static_assert(SEEQ_TILE == SEEQ_TILE_WG * SEEQ_TILE_ITEMS && SEEQ_TILE_WG == SEEQ_WG, "tile / workgroup");

#define SEEQ_TILE_WAVES (SEEQ_TILE_WG / 64)

/* the item this thread owns in round k of its tile */
__device__ __forceinline__ uint64_t tile_index(int k) { return (uint64_t)blockIdx.x * SEEQ_TILE + (uint64_t)k * SEEQ_TILE_WG + threadIdx.x; }

/* the one lane of a wave that writes the wave's numbers to LDS: the last one, which holds the sum of an inclusive wave scan */
__device__ __forceinline__ bool tile_publishes(void) { return (threadIdx.x & 63) == 63; }

/* Tile sums: N wave-uniform counts of this tile -> bsum[j * nt + tile], summed over the waves through s_sum. */
template <int N>
__device__ __forceinline__ void tile_sums(const uint32_t (&v)[N], uint32_t (&s_sum)[N][SEEQ_TILE_WAVES], uint32_t *bsum, uint32_t nt)
{
   const int wave = threadIdx.x >> 6;
   if (tile_publishes()) {
#pragma unroll
      for (int j = 0; j < N; j++) s_sum[j][wave] = v[j];
   }
   __syncthreads();
   if (threadIdx.x == 0) {
#pragma unroll
      for (int j = 0; j < N; j++) {
         uint32_t t = 0;
         for (int w = 0; w < SEEQ_TILE_WAVES; w++) t += s_sum[j][w];
         bsum[(size_t)j * nt + blockIdx.x] = t;
      }
   }
}

/* Top, by one workgroup: sums[0 .. nt) -> its exclusive prefix, in place; tot[j]: the total of row j, sums[j * nt .. (j + 1) * nt), j < N,
   as it was (valid in thread 0; rows 1 .. N - 1 are only read). */
template <int N, typename T>
__device__ __forceinline__ void tile_top(T *sums, uint32_t nt, T *s_wave /* >= 4 */, T (&tot)[N])
{
   T running = 0, part[N] = {};
   for (uint32_t b0 = 0; b0 < nt; b0 += SEEQ_TILE_WG) {
      const uint32_t i = b0 + threadIdx.x;
      const T v = i < nt ? sums[i] : 0u;
      T t;
      const T ex = block_excl_scan(v, &t, s_wave);
      if (i < nt) {
         sums[i] = running + ex;
#pragma unroll
         for (int j = 1; j < N; j++) part[j] += sums[(size_t)j * nt + i];
      }
      running += t;
   }
   tot[0] = running;
#pragma unroll
   for (int j = 1; j < N; j++) block_excl_scan(part[j], &tot[j], s_wave);
}

/* Ranks, before the barrier, once per round: this lane's rank among the kept items of its wave in the round (the kept items in the lanes
   below); the wave's count goes to the round's row s_cnt[round]. */
__device__ __forceinline__ uint32_t tile_wave_rank(bool keep, uint32_t (&s_row)[SEEQ_TILE_WAVES])
{
   const uint64_t b = __ballot(keep);
   if (tile_publishes()) s_row[threadIdx.x >> 6] = (uint32_t)__popcll(b);
   return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

/* The same for a 64-bit value per item (0 for an item that is not kept): the sum of the values in the lanes below; the wave's sum to its row. */
__device__ __forceinline__ uint64_t tile_wave_offset(uint64_t v, uint64_t (&s_row)[SEEQ_TILE_WAVES])
{
   const uint64_t incl = wave_incl_scan_u64(v);
   if (tile_publishes()) s_row[threadIdx.x >> 6] = incl;
   return incl - v;
}

/* Ranks, behind the barrier, once per round and in the order of the rounds: base (what lies before this tile -- row 0 of bsum -- and then
   before this round) + the waves before this one in the round + within; base moves on by the round's total.  For the counts this is where
   the round's item goes if it is kept. */
template <typename T>
__device__ __forceinline__ T tile_place(T &base, T within, const T (&s_row)[SEEQ_TILE_WAVES])
{
   const int wave = threadIdx.x >> 6;
   T before = 0, tot = 0;
#pragma unroll
   for (int w = 0; w < SEEQ_TILE_WAVES; w++) {
      const T c = s_row[w];
      if (w < wave) before += c;
      tot += c;
   }
   const T at = base + before + within;
   base += tot;
   return at;
}

/* "Opens its line": is record i of in[0 .. n), whose first word (its line number) is x, the first one of its line?  The records of a line
   are contiguous, so it is iff i == 0 or record i - 1 has another number.  Lane - 1 holds record i - 1: EVERY lane of the wave calls
   this, a lane without a record (i >= n) with any x; what it gets means nothing. */
__device__ __forceinline__ bool tile_opens_line(uint64_t i, uint32_t x, const uint4 *in, uint32_t n)
{
   uint32_t prev = (uint32_t)__shfl_up((int)x, 1, 64);
   if ((threadIdx.x & 63) == 0 && i > 0 && i < n) prev = in[i - 1].x;
   return i == 0 || prev != x;
}

#endif   /* __HIPCC__ */
#endif
