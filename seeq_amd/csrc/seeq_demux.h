/*
 * seeq_demux.h -- DEMULTIPLEXING on the device (seeqdevScanRunDemux): per line of the text the best pattern of a set.
 *
 * Input: per pattern k of the set, its SQ_BEST records (at most one per line, in line order) -- either all of them at once
 * (the one walk of seeq_multi.h leaves them in the record workspace, one region per pattern) or one pattern after the other
 * (a scan per pattern overwrites the record workspace each time).  Rule (device.py:assign_best): the winner of a line is
 * the pattern of smallest distance, the lowest index on a tie; margin = runner-up's distance - winner's, 255 = none or
 * >= 255; 0 = ambiguous.  Output: one 16-byte record per assigned line, in line order.
 *
 * Per line ONE 32-bit key (0 = no pattern yet):  bit 31 | dist << 16 | pattern << 8 | margin.
 *
 *   k_demux_fold      pattern k's records, one lane each, folded into the keys of their lines.  The patterns are folded
 *                     one launch after the other in index order, and a pattern has at most one record per line, so no
 *                     two lanes of a launch touch one key: no atomics, and ties keep the lower index by construction.
 *                     STAGE (a scan per pattern): the records are gone after the next scan, so the winner so far is
 *                     kept in a staging slot per assigned line (slot in aux[line]; slots handed out per wave).
 *   k_demux_tally     per line: per-pattern assigned counts and the ambiguous count (LDS histogram); STAGE: the final
 *                     dist / pattern / margin into the line's staging record.
 *   (scan)            exclusive scan of "key != 0" over the lines (k_scan_reduce / _top / _apply<2>): the output rank.
 *   k_demux_emit      one walk: every pattern's records again; the winner's record (its pattern is the key's) is
 *                     written at its line's rank.  blockIdx.y = pattern: one launch for the set.
 *   k_demux_scatter   a scan per pattern: every staging record to its line's rank.
 *
 * Device memory: the keys and aux (8 bytes per line), the output (16 bytes per record) and DemuxCnt.
 */
#ifndef SEEQ_DEMUX_H_
#define SEEQ_DEMUX_H_

#define SEEQ_DEMUX_MAX 255
#define DEMUX_ASSIGNED 0x80000000u
#define DEMUX_WG 256

struct DemuxCnt {
   unsigned long long per_pat[256];   /* assigned lines per winning pattern */
   unsigned long long ambiguous;      /* assigned lines of margin 0 */
   uint32_t nassigned;                /* the rank scan's total */
   uint32_t slot;                     /* STAGE: staging slots handed out */
   uint32_t bad;                      /* a record outside the key array, a slot outside the staging area: internal error */
   uint32_t pad;
};

/* One pattern's records, all patterns in one launch (blockIdx.y): pattern k's region starts at rec + k * stride. */
struct DemuxSrc {
   const uint4 *rec;
   uint64_t     stride;
   uint32_t     n[SEEQ_MULTI_MAX];
};

/* The output record's last word: dist (16 bits), pattern, margin (seeqdev_demux_t). */
__device__ __forceinline__ uint32_t demux_word(uint32_t key)
{
   return ((key >> 16) & 0x7FFFu) | (((key >> 8) & 255u) << 16) | ((key & 255u) << 24);
}

/* A record of pattern k at distance d on a line whose key is c.  won: the record is the line's best so far. */
__device__ __forceinline__ uint32_t demux_fold_key(uint32_t c, uint32_t d, uint32_t k, bool &won)
{
   if (!(c & DEMUX_ASSIGNED)) { won = true; return DEMUX_ASSIGNED | d << 16 | k << 8 | 255u; }
   const uint32_t cd = (c >> 16) & 0x7FFFu, cm = c & 255u;
   if (d < cd) {                                            /* the old winner is the runner-up now (its distance <= any other's) */
      won = true;
      const uint32_t m = cd - d < 255u ? cd - d : 255u;
      return DEMUX_ASSIGNED | d << 16 | k << 8 | m;
   }
   won = false;                                             /* a tie or worse: a later pattern never takes a line */
   const uint32_t m = d - cd < 255u ? d - cd : 255u;
   return m < cm ? (c & ~255u) | m : c;
}

template <bool STAGE>
__global__ __launch_bounds__(DEMUX_WG) void k_demux_fold(const uint4 *rec, uint32_t n, uint32_t k, uint32_t *key, uint32_t *aux, uint32_t nkeys,
                                                         uint4 *stage, uint32_t cap_stage, DemuxCnt *cnt)
{
   const uint32_t i = blockIdx.x * DEMUX_WG + threadIdx.x;
   bool won = false, fresh = false;
   uint4 r = make_uint4(0, 0, 0, 0);
   uint32_t line = 0;
   if (i < n) {
      r = rec[i];
      line = r.x - 1u;
      if (line >= nkeys || r.w > 0x7FFFu) {
         atomicOr(&cnt->bad, 1u);
      } else {
         const uint32_t c = key[line];
         fresh = !(c & DEMUX_ASSIGNED);
         const uint32_t nk = demux_fold_key(c, r.w, k, won);
         if (nk != c) key[line] = nk;
      }
   }
   if (!STAGE) return;
   /* one slot per newly assigned line: one atomic per wave */
   const int lane = threadIdx.x & 63;
   const uint64_t b = __ballot(fresh);
   uint32_t base = 0;
   if (b) {
      const int leader = __ffsll((long long)b) - 1;
      if (lane == leader) base = atomicAdd(&cnt->slot, (uint32_t)__popcll(b));
      base = (uint32_t)__shfl((int)base, leader);
   }
   if (!won) return;
   const uint32_t slot = fresh ? base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull)) : aux[line];
   if (fresh) aux[line] = slot;
   if (slot < cap_stage) stage[slot] = make_uint4(r.x, r.y, r.z, r.w | k << 16 | 255u << 24);
   else atomicOr(&cnt->bad, 2u);
}

template <bool STAGE>
__global__ __launch_bounds__(DEMUX_WG) void k_demux_tally(const uint32_t *key, const uint32_t *aux, uint32_t nkeys, uint4 *stage, uint32_t cap_stage,
                                                          DemuxCnt *cnt)
{
   __shared__ uint32_t s_h[257];
   for (int j = threadIdx.x; j < 257; j += DEMUX_WG) s_h[j] = 0;
   __syncthreads();
   for (uint32_t i = blockIdx.x * DEMUX_WG + threadIdx.x; i < nkeys; i += gridDim.x * DEMUX_WG) {
      const uint32_t c = key[i];
      if (!(c & DEMUX_ASSIGNED)) continue;
      atomicAdd(&s_h[(c >> 8) & 255u], 1u);
      if (!(c & 255u)) atomicAdd(&s_h[256], 1u);
      if (STAGE) {
         const uint32_t slot = aux[i];
         if (slot < cap_stage) reinterpret_cast<uint32_t *>(stage + slot)[3] = demux_word(c);
         else atomicOr(&cnt->bad, 2u);
      }
   }
   __syncthreads();
   for (int j = threadIdx.x; j < 257; j += DEMUX_WG)
      if (s_h[j]) atomicAdd(j < 256 ? &cnt->per_pat[j] : &cnt->ambiguous, (unsigned long long)s_h[j]);
}

__global__ __launch_bounds__(DEMUX_WG) void k_demux_emit(DemuxSrc src, const uint32_t *key, const uint32_t *rank, uint32_t nkeys, uint4 *out,
                                                         uint32_t cap, DemuxCnt *cnt)
{
   const uint32_t k = blockIdx.y;
   const uint32_t i = blockIdx.x * DEMUX_WG + threadIdx.x;
   if (i >= src.n[k]) return;
   const uint4 r = src.rec[k * src.stride + i];
   const uint32_t line = r.x - 1u;
   if (line >= nkeys) return;                               /* (k_demux_fold flagged it) */
   const uint32_t c = key[line];
   if (((c >> 8) & 255u) != k) return;
   const uint32_t j = rank[line];
   if (j < cap) out[j] = make_uint4(r.x, r.y, r.z, demux_word(c));
   else atomicOr(&cnt->bad, 4u);
}

__global__ __launch_bounds__(DEMUX_WG) void k_demux_scatter(const uint4 *stage, uint32_t cap_stage, const uint32_t *rank, uint32_t nkeys, uint4 *out,
                                                            uint32_t cap, DemuxCnt *cnt)
{
   const uint32_t n = cnt->slot < cap_stage ? cnt->slot : cap_stage;
   for (uint32_t i = blockIdx.x * DEMUX_WG + threadIdx.x; i < n; i += gridDim.x * DEMUX_WG) {
      const uint4 r = stage[i];
      const uint32_t line = r.x - 1u;
      const uint32_t j = line < nkeys ? rank[line] : cap;
      if (j < cap) out[j] = r;
      else atomicOr(&cnt->bad, 4u);
   }
}

#endif
