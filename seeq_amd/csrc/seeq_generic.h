/*
 * seeq_generic.h -- the kernels of the generic path (any pattern, any option): newline index (K0), k_forward<W> (K1), k_compact (K3),
 * k_exact<W,MODE> (K4/K5), k_rec_offsets, and the one-thread kernels every path ends a segment with (k_seg_mid, k_rec_check, k_seg_end).
 * Included by seeq_device.hip alone, after seeq_types.h / seeq_scan_common.h and its WG / TILE constants; launched by its segment driver
 * (seg_index_forward, seg_post).  The ranks between the steps (K2) are seeq_scan.h's.
 */
#ifndef SEEQ_GENERIC_H_
#define SEEQ_GENERIC_H_

/* ========================================================================== */
/* Block-level helpers                                                        */
/* ========================================================================== */
/* 64-bit mask of newline positions among the 64 bytes this thread owns
 * (bytes seg_base + tile*TILE + tid*64 ...), restricted to positions q with
 * q < seg_base+seg_len and q + 1 < nbytes (a final '\n' starts no line). */
__device__ __forceinline__ uint64_t thread_nl_mask(const ScanArgs &a, uint32_t tile)
{
   const uint64_t seg_off = (uint64_t)tile * TILE + (uint64_t)threadIdx.x * 64;
   if (seg_off >= a.seg_len) return 0;
   const uint64_t q0 = a.seg_base + seg_off;
   uint64_t limit = a.seg_base + a.seg_len;                /* exclusive */
   if (a.nbytes - 1 < limit) limit = a.nbytes - 1;         /* q + 1 < nbytes  (nbytes > 0 here) */
   uint64_t mask = 0;
   if (q0 + 64 <= limit && ((uintptr_t)(a.text + q0) & 15) == 0) {
      const uint4 *p = reinterpret_cast<const uint4 *>(a.text + q0);
#pragma unroll
      for (int j = 0; j < 4; j++) {
         const uint4 v = p[j];
         const uint32_t f0 = nl_flags(v.x), f1 = nl_flags(v.y), f2 = nl_flags(v.z), f3 = nl_flags(v.w);
         /* gather bit 7 of each byte into 4 consecutive bits */
         const uint32_t b0 = ((f0 >> 7) * 0x00204081u >> 21) & 0xFu;
         const uint32_t b1 = ((f1 >> 7) * 0x00204081u >> 21) & 0xFu;
         const uint32_t b2 = ((f2 >> 7) * 0x00204081u >> 21) & 0xFu;
         const uint32_t b3 = ((f3 >> 7) * 0x00204081u >> 21) & 0xFu;
         const uint64_t m16 = b0 | (b1 << 4) | (b2 << 8) | (b3 << 12);
         mask |= m16 << (16 * j);
      }
   } else {
      for (int k = 0; k < 64; k++) {
         const uint64_t q = q0 + k;
         if (q < limit && a.text[q] == '\n') mask |= 1ull << k;
      }
   }
   return mask;
}

/* ========================================================================== */
/* K0: newline index                                                          */
/* ========================================================================== */
__global__ __launch_bounds__(WG) void k_nl_count(ScanArgs a)
{
   __shared__ uint32_t s_wave[4];
   const uint64_t m = thread_nl_mask(a, blockIdx.x);
   uint32_t tot;
   block_excl_scan((uint32_t)__popcll(m), &tot, s_wave);
   if (threadIdx.x == 0) a.tile_cnt[blockIdx.x] = tot;
}

/* After tile_cnt has been scanned in place (exclusive) and the total written
 * to cnt->seg_nlines: add the line that starts at byte 0 of the buffer. */
__global__ void k_index_finalize(ScanArgs a)
{
   Counters *c = a.cnt;
   uint32_t n = c->seg_nlines;
   if (a.first_seg && a.nbytes > 0) n += 1;
   if (n > a.cap_lines) {
      atomicOr(&c->overflow, OVF_LINES);
      if (n > c->need_lines) c->need_lines = n;
      n = 0;                       /* later kernels of this segment do nothing */
   } else if (n > c->need_lines) {
      c->need_lines = n;
   }
   c->seg_nlines = n;
   if (n && a.first_seg) a.line_start[0] = 0;
}

__global__ __launch_bounds__(WG) void k_nl_write(ScanArgs a)
{
   __shared__ uint32_t s_wave[4];
   if (a.cnt->seg_nlines == 0) return;
   uint64_t m = thread_nl_mask(a, blockIdx.x);
   uint32_t tot;
   uint32_t rank = block_excl_scan((uint32_t)__popcll(m), &tot, s_wave);
   rank += a.tile_cnt[blockIdx.x] + (a.first_seg ? 1u : 0u);
   const uint32_t off0 = blockIdx.x * TILE + threadIdx.x * 64 + 1;   /* start = newline position + 1 */
   while (m) {
      const int b = __builtin_ctzll(m);
      m &= m - 1;
      a.line_start[rank++] = off0 + (uint32_t)b;
   }
}

/* ========================================================================== */
/* K1: forward scan, one line per lane, 64 consecutive lines per wave          */
/* ========================================================================== */
template <int W>
__device__ __forceinline__ void load_tables(const ScanArgs &a, uint32_t *s_peq, uint8_t *s_lut)
{
   for (int i = threadIdx.x; i < 10 * W; i += WG) {
      /* a.peq holds [2][5][Wp] with Wp = words of the pattern; pad to W */
      const int Wp = (a.m + 31) >> 5;
      const int dir = i / (5 * W), rem = i % (5 * W), cls = rem / W, w = rem % W;
      s_peq[i] = w < Wp ? a.peq[(dir * 5 + cls) * Wp + w] : 0u;
   }
   for (int b = threadIdx.x; b < 256; b += WG) s_lut[b] = sq_class_of((uint32_t)b, a.options);
   __syncthreads();
}

template <int W>
__global__ __launch_bounds__(WG) void k_forward(ScanArgs a)
{
   __shared__ uint32_t s_peq[10 * W];
   __shared__ uint8_t s_lut[256];
   load_tables<W>(a, s_peq, s_lut);
   const uint32_t nlines = a.cnt->seg_nlines;
   const int lane = threadIdx.x & 63;
   const uint32_t wave = (blockIdx.x * WG + threadIdx.x) >> 6;
   const uint32_t nwaves = (gridDim.x * WG) >> 6;
   const bool fasta = (a.options & SEEQDEV_FASTA) != 0;
   const uint32_t nchunks = (nlines + 63) >> 6;
   for (uint32_t chunk = wave; chunk < nchunks; chunk += nwaves) {
      const uint32_t idx = chunk * 64 + lane;
      bool hit = false, hdr = false;
      if (idx < nlines) {
         const uint64_t off = a.seg_base + a.line_start[idx];
         if (fasta && a.text[off] == '>') hdr = true;   /* off < nbytes: every line has >= 1 byte */
         else
            hit = sq_scan_line<W, SQ_MODE_ANY>(a.text, a.nbytes, off, (const uint32_t *)s_peq,
                                               (const uint32_t *)(s_peq + 5 * W), (const uint8_t *)s_lut, a.m, a.tau,
                                               a.options & 3, 0, nullptr, 0) != 0;
      }
      const uint64_t hm = __ballot(hit);
      const uint64_t dm = __ballot(hdr);
      if (lane == 0) {
         a.hitmask[chunk] = hm;
         if (fasta) a.hdrmask[chunk] = dm;
      }
   }
}

__device__ __forceinline__ uint32_t counted_line_no(const ScanArgs &a, uint32_t idx, bool fasta)
{
   /* 1-based index among counted lines of the whole buffer (reference seeq.c:377) */
   uint64_t n = a.cnt->lines + idx + 1;
   if (fasta) {
      const uint32_t chunk = idx >> 6;
      n -= a.hdr_off[chunk] + (uint32_t)__popcll(a.hdrmask[chunk] & ((1ull << (idx & 63)) - 1));
   }
   return (uint32_t)n;
}

/* ========================================================================== */
/* K3: ordered compaction of hit lines                                        */
/* ========================================================================== */
__global__ __launch_bounds__(WG) void k_compact(ScanArgs a)
{
   const uint32_t nlines = a.cnt->seg_nlines;
   const uint32_t nchunks = (nlines + 63) >> 6;
   const int lane = threadIdx.x & 63;
   const uint32_t wave = (blockIdx.x * WG + threadIdx.x) >> 6;
   const uint32_t nwaves = (gridDim.x * WG) >> 6;
   const bool fasta = (a.options & SEEQDEV_FASTA) != 0;
   for (uint32_t chunk = wave; chunk < nchunks; chunk += nwaves) {
      const uint64_t hm = a.hitmask[chunk];
      if ((hm >> lane) & 1) {
         const uint32_t k = a.wave_off[chunk] + (uint32_t)__popcll(hm & ((1ull << lane) - 1));
         if (k < a.cap_hitlines) {
            const uint32_t idx = chunk * 64 + lane;
            a.hit_start[k] = a.line_start[idx];
            a.hit_line[k] = counted_line_no(a, idx, fasta);
         }
      }
   }
}

/* After compaction: overflow check of the hit-line list; for FIRST/BEST the
 * number of records of the segment is the number of hit lines. */
__global__ void k_seg_mid(ScanArgs a)
{
   Counters *c = a.cnt;
   uint32_t nhl = c->seg_nhitlines;
   if (nhl > c->need_hitlines) c->need_hitlines = nhl;
   if (nhl > a.cap_hitlines) {
      atomicOr(&c->overflow, OVF_HITLINES);
      nhl = 0;
      c->seg_nhitlines = 0;      /* totals of this run are void anyway */
   }
   c->seg_nrec = nhl;            /* overwritten by the nh scan for SQ_ALL / COUNTMATCH */
}

__global__ void k_rec_check(ScanArgs a) { rec_check_body(a); }

/* ========================================================================== */
/* K4/K5: exact pass over the hit lines                                       */
/* ========================================================================== */
template <int W, int MODE>
__global__ __launch_bounds__(WG) void k_exact(ScanArgs a)
{
   __shared__ uint32_t s_peq[10 * W];
   __shared__ uint8_t s_lut[256];
   load_tables<W>(a, s_peq, s_lut);
   const Counters *c = a.cnt;
   const uint32_t nhl = c->seg_nhitlines;
   const int match_opt = a.options & 3;
   if (MODE == SQ_MODE_EMIT && (c->overflow & OVF_RECORDS)) return;
   const uint32_t stride = gridDim.x * WG;
   for (uint32_t k = blockIdx.x * WG + threadIdx.x; k < nhl; k += stride) {
      const uint64_t off = a.seg_base + a.hit_start[k];
      if (MODE == SQ_MODE_COUNT) {
         a.nh[k] = sq_scan_line<W, SQ_MODE_COUNT>(a.text, a.nbytes, off, (const uint32_t *)s_peq,
                                                  (const uint32_t *)(s_peq + 5 * W), (const uint8_t *)s_lut, a.m,
                                                  a.tau, match_opt, 0, nullptr, 0);
      } else {
         const uint32_t line_no = a.hit_line[k];
         uint64_t dst;
         uint32_t cap;
         if (match_opt == SQ_ALL) {
            dst = c->records + a.nh[k];
            cap = 0xFFFFFFFFu;       /* exact count known from the COUNT pass */
         } else {
            dst = c->records + (a.use_nh ? a.nh[k] : k);
            cap = 1;
         }
         sq_scan_line<W, SQ_MODE_EMIT>(a.text, a.nbytes, off, (const uint32_t *)s_peq,
                                       (const uint32_t *)(s_peq + 5 * W), (const uint8_t *)s_lut, a.m, a.tau,
                                       match_opt, line_no, reinterpret_cast<sq_hit_t *>(a.records + dst), cap);
      }
   }
}

/* Per record: where its line starts in the buffer (lets the host jump from hit to hit instead of
   walking every line: the replay of seeqFileMatch, seeq.c:361-386, becomes O(hits)). */
__global__ __launch_bounds__(WG) void k_rec_offsets(ScanArgs a)
{
   const Counters *c = a.cnt;
   if (c->overflow & OVF_RECORDS) return;
   const uint32_t nhl = c->seg_nhitlines;
   const bool all = (a.options & 3) == SQ_ALL || a.use_nh;
   const uint32_t stride = gridDim.x * WG;
   for (uint32_t k = blockIdx.x * WG + threadIdx.x; k < nhl; k += stride) {
      const uint64_t off = a.seg_base + a.hit_start[k];
      if (all) {
         const uint32_t lo = a.nh[k], hi = k + 1 < nhl ? a.nh[k + 1] : c->seg_nrec;
         for (uint32_t r = lo; r < hi; r++) a.rec_off[c->records + r] = off;
      } else {
         a.rec_off[c->records + k] = off;
      }
   }
}

/* Lines with >= 1 verified hit, from the per-line counts (before they are scanned into offsets). */
__device__ __forceinline__ void count_nonzero_body(const ScanArgs &a)
{
   __shared__ uint32_t s_n[WG / 64];
   const uint32_t nhl = a.cnt->seg_nhitlines;
   const uint32_t stride = gridDim.x * WG;
   uint32_t n = 0;
   for (uint32_t k = blockIdx.x * WG + threadIdx.x; k < nhl; k += stride) n += a.nh[k] != 0;
#pragma unroll
   for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
   if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = n;
   __syncthreads();
   if (threadIdx.x == 0) {                                 /* one atomic per block: same-address atomics serialise */
      n = 0;
      for (int w = 0; w < WG / 64; w++) n += s_n[w];
      if (n) atomicAdd(&a.cnt->seg_nmatch, n);
   }
}
__global__ __launch_bounds__(WG) void k_count_nonzero(ScanArgs a) { count_nonzero_body(a); }

__global__ void k_seg_end(ScanArgs a, int flags) { seg_end_body(a, flags); }

/* SINGLELINE: the buffer is one string -> one line starting at 0. */
__global__ void k_single_line(ScanArgs a)
{
   a.cnt->seg_nlines = 1;
   if (a.cnt->need_lines < 1) a.cnt->need_lines = 1;
   a.line_start[0] = 0;
}

#endif
