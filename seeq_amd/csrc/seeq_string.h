/*
 * seeq_string.h -- k_string<W> / seeqdevStringMatch: one string per call in one launch.  Included last by seeq_device.hip (the context,
 * text_ensure, SEEQ_FOR_WORDS).
 */
#ifndef SEEQ_STRING_H_
#define SEEQ_STRING_H_

/* ========================================================================== */
/* One string, one launch: seeqStringMatch (reference libseeq.c:171-352)        */
/* ========================================================================== */
/* The per-string entry point is what the reference's Python module calls for every string (seeqmodule.c:858).  One
 * workgroup: all threads stage the string (read over the link from page-locked host memory when it is short, else
 * from HBM) and the tables into LDS; then the string's positions are shared out over the 256 threads: every thread
 * computes the capped scores of its positions from a fresh column started m + tau + 1 characters earlier (exact from
 * there on, as in k_stream), applies the acceptance rules -- which only look at the scores of a position and the two
 * before it (libseeq.c:277-331: emit = stop ? !latch : zero, latch = stop ? 1 : zero) -- and the emissions are compacted
 * in order (block scan) / reduced (first, best), starts recovered by their threads, count + records written straight
 * into page-locked host memory.  A single lane walking the string took 0.17 us per character (41 us per call at 150
 * characters, 15 of them launch + synchronisation).  Strings with skipped bytes (SQ_IGNORE, SQ_STREAM) or longer than
 * STRING_PAR_MAX keep the one-lane scan.  One launch, one stream synchronisation, no device allocation.  Long strings
 * in line mode take the batched scan instead (libseeq_api.c). */
static constexpr uint32_t STRING_LDS_MAX = 48u * 1024;      /* strings up to this are staged in LDS */
static constexpr uint32_t STRING_ZC_MAX = 4096;             /* ... and up to this read straight from host memory */
static constexpr uint32_t STRING_PAR_MAX = 32768;           /* ... and up to this scanned by all threads (positions fit 16 bits; longer strings in line mode take the batched scan) */

template <int W>
__global__ __launch_bounds__(WG) void k_string(const uint8_t *text, uint32_t n, const uint32_t *peq, int m, int tau, int options,
                                               uint32_t *out, uint32_t cap, uint32_t seq)
{
   extern __shared__ __align__(16) uint8_t s_text[];       /* n + 16 bytes when staged */
   __shared__ uint32_t s_peq[10 * W];
   __shared__ uint8_t s_lut[256];
   const int Wp = (m + 31) >> 5;
   for (int i = threadIdx.x; i < 10 * W; i += WG) {
      const int dir = i / (5 * W), rem = i % (5 * W), cls = rem / W, w = rem % W;
      s_peq[i] = w < Wp ? peq[(dir * 5 + cls) * Wp + w] : 0u;
   }
   for (int b = threadIdx.x; b < 256; b += WG) s_lut[b] = sq_class_of((uint32_t)b, options);
   const bool staged = n <= STRING_LDS_MAX;
   if (staged) {
      /* 16 bytes per thread and round, all loads of a round in flight together (the link's latency is paid once per round) */
      for (uint32_t o = threadIdx.x * 16; o < n; o += WG * 16) {
         const sq_chunk16_t c = sq_load16(text, o, n);
         *reinterpret_cast<uint4 *>(s_text + o) = make_uint4(c.w[0], c.w[1], c.w[2], c.w[3]);
      }
   }
   __shared__ uint32_t s_first, s_skip, s_key, s_wave[WG / 64];
   const bool par = n <= STRING_PAR_MAX;                  /* (=> staged) */
   if (threadIdx.x == 0) { s_first = n; s_skip = 0; s_key = 0xFFFFFFFFu; }
   __syncthreads();
   if (par) {
      /* the line ends at its first terminator (or at n: bytes beyond read as NUL); a skipped byte before it -> one lane */
      for (uint32_t j = threadIdx.x; j < n; j += WG) if (s_lut[s_text[j]] == SQC_TERM) atomicMin(&s_first, j);
      __syncthreads();
      const uint32_t len = s_first;
      for (uint32_t j = threadIdx.x; j < len; j += WG) if (s_lut[s_text[j]] == SQC_SKIP) s_skip = 1u;
      __syncthreads();
      if (!s_skip) {
         const int match_opt = options & 3;
         const uint32_t *peq_f = s_peq, *peq_r = s_peq + 5 * W;
         uint16_t *ed = reinterpret_cast<uint16_t *>(s_text + (((size_t)n + 31) & ~(size_t)15));   /* per position: emitted distance + 1, or 0 */
         const uint32_t P = len + 1;                      /* positions 0..len; the last one is the terminator's step */
         const uint32_t B = (P + WG - 1) / WG;
         const uint32_t j0 = threadIdx.x * B, j1 = j0 + B < P ? j0 + B : P;
         const uint32_t cnt = j0 < P ? sq_emit_window<W>((const uint8_t *)s_text, len, j0, j1, peq_f, (const uint8_t *)s_lut, m, tau, ed) : 0u;
         uint32_t total = 0, nh_par = 0;
         const uint32_t excl = block_excl_scan(cnt, &total, s_wave);      /* (also orders the ed[] writes: barrier inside) */
         sq_hit_t *rec = reinterpret_cast<sq_hit_t *>(out + 4);
         if (match_opt == SQK_ALL) {
            uint32_t idx = excl;
            for (uint32_t j = j0; j < j1 && cnt; j++) {
               if (!ed[j]) continue;
               if (idx < cap) {
                  sq_hit_t h;
                  h.line = 1;
                  h.start = sq_reverse_start<W>((const uint8_t *)s_text, j, (int)ed[j] - 1, peq_r, (const uint8_t *)s_lut, m, tau);
                  h.end = j;
                  h.dist = (uint32_t)ed[j] - 1u;
                  rec[idx] = h;
               }
               idx++;
            }
            nh_par = total;
         } else {
            /* SQ_BEST: smallest distance, first position; SQ_FIRST / SQ_COUNT: first position */
            for (uint32_t j = j0; j < j1 && cnt; j++)
               if (ed[j]) { atomicMin(&s_key, (match_opt == SQK_BEST ? ((uint32_t)ed[j] - 1u) << 16 : 0u) | j); if (match_opt != SQK_BEST) break; }
            __syncthreads();
            const uint32_t key = s_key;
            if (key != 0xFFFFFFFFu) {
               const uint32_t j = key & 0xFFFFu;
               if (j >= j0 && j < j1 && cap) {
                  sq_hit_t h;
                  h.line = 1;
                  h.start = sq_reverse_start<W>((const uint8_t *)s_text, j, (int)ed[j] - 1, peq_r, (const uint8_t *)s_lut, m, tau);
                  h.end = j;
                  h.dist = (uint32_t)ed[j] - 1u;
                  rec[0] = h;
               }
            }
            nh_par = key != 0xFFFFFFFFu ? 1u : 0u;
         }
         /* records first (every writer fences), then the count, then the ticket the host spins on */
         __threadfence_system();
         __syncthreads();
         if (threadIdx.x == 0) {
            out[0] = nh_par;
            __threadfence_system();
            __hip_atomic_store(&out[1], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
         }
         return;
      }
   }
   if (threadIdx.x != 0) return;
   const uint8_t *tp = staged ? (const uint8_t *)s_text : text;
   const uint32_t nh = sq_scan_line<W, SQ_MODE_EMIT>(tp, (uint64_t)n, 0, (const uint32_t *)s_peq, (const uint32_t *)(s_peq + 5 * W),
                                                     (const uint8_t *)s_lut, m, tau, options & 3, 1,
                                                     reinterpret_cast<sq_hit_t *>(out + 4), cap);
   out[0] = nh;
   __threadfence_system();
   __hip_atomic_store(&out[1], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <int W>
static void launch_string(seeqdev_scan *s, const seeqdev_pattern *pat, const uint8_t *text, uint32_t n, int options, uint32_t cap, uint32_t seq)
{
   size_t lds = n <= STRING_LDS_MAX ? (((size_t)n + 31) & ~(size_t)15) : 0;
   if (n <= STRING_PAR_MAX) lds += (2 * ((size_t)n + 2) + 15) & ~(size_t)15;        /* + per-position emissions */
   if (lds > 48u * 1024)                                    /* beyond the default limit of dynamic LDS per workgroup (set per device: every time) */
      (void)hipFuncSetAttribute((const void *)k_string<W>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
   hipLaunchKernelGGL(k_string<W>, dim3(1), dim3(WG), lds, s->stream, text, n, (const uint32_t *)pat->d_peq, pat->wlen, pat->tau,
                      options, s->h_strout, cap, seq);
}

/* data[0..n): the string (no NUL needed; a NUL inside ends it as in the reference).  On return *rec points at the
 * hit records (left to right; context-owned page-locked memory, valid until the next call) and *nrec is their number. */
extern "C" int seeqdevStringMatch(seeqdev_scan_t *s, const seeqdev_pattern_t *pat, const char *data, size_t n, int options,
                                  const seeqdev_hit_t **rec, size_t *nrec)
{
   seeqerr = 0;
   if (!s || !pat || (!data && n) || !rec || !nrec || (options & SEEQDEV_FASTQ)) { errno = EINVAL; return -1; }
   if (n > 0xFFFF0000ull) { errno = E2BIG; return -1; }
   if (use_device(s->device)) return -1;
   if (!s->h_strout) {                                      /* (ws_make: both or neither) */
      const size_t nrec0 = 256;                             /* records */
      if (ws_make(&s->ws, {{s->h_strout, 16 + nrec0 * sizeof(seeqdev_hit_t), WS_COHERENT}, {s->h_str, STRING_ZC_MAX + 16, WS_PINNED}})) return -1;
      s->cap_strout = nrec0;
   }
   const uint8_t *dtext;
   if (n <= STRING_ZC_MAX) {
      memcpy(s->h_str, data, n);
      dtext = s->h_str;                                     /* page-locked host memory is device-visible at the same address */
   } else {
      if (text_ensure(s, n)) return -1;
      HIP_TRY(hipMemcpyAsync(s->d_text, data, n, hipMemcpyHostToDevice, s->stream), EIO);
      s->avg_text = NULL;
      dtext = s->d_text;
   }
   for (int attempt = 0; attempt < 2; attempt++) {
      const uint32_t cap = (uint32_t)s->cap_strout;
      s->h_strout[0] = 0;
      const uint32_t seq = ++s->str_seq ? s->str_seq : ++s->str_seq;      /* never 0 */
      volatile uint32_t *ticket = s->h_strout + 1;
      *ticket = 0;
      SEEQ_FOR_WORDS(pat->words, launch_string, s, pat, dtext, (uint32_t)n, options, cap, seq);
      HIP_TRY(hipGetLastError(), EIO);
      /* The kernel's last store is its ticket, into fine-grained page-locked memory: spinning on it is shorter than the
         runtime's completion path (hipStreamSynchronize: ~8 us).  After 200 us (long strings, a failed launch) the runtime
         takes over. */
      {
         struct timespec t0, t1;
         clock_gettime(CLOCK_MONOTONIC, &t0);
         unsigned spins = 0;
         while (__atomic_load_n(ticket, __ATOMIC_ACQUIRE) != seq) {
            if ((++spins & 63u) == 0) {
               clock_gettime(CLOCK_MONOTONIC, &t1);
               if ((t1.tv_sec - t0.tv_sec) * 1000000000L + (t1.tv_nsec - t0.tv_nsec) > 200000L) break;
            }
         }
         if (__atomic_load_n(ticket, __ATOMIC_ACQUIRE) != seq) HIP_TRY(hipStreamSynchronize(s->stream), EIO);
      }
      const uint32_t nh = s->h_strout[0];
      if (nh <= cap) {
         *rec = reinterpret_cast<const seeqdev_hit_t *>(s->h_strout + 4);
         *nrec = nh;
         return 0;
      }
      /* SQ_ALL with more hits than the record buffer holds: grow it (nothing to carry over; a refusal leaves the buffer it had) and scan again */
      const size_t grown = (size_t)nh + (nh >> 2) + 64;
      if (ws_grow(&s->ws, &s->cap_strout, grown, {{s->h_strout, 16 + grown * sizeof(seeqdev_hit_t), WS_COHERENT}})) return -1;
   }
   errno = EIO;
   return -1;
}

#endif
