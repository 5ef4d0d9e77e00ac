/*
 * seeq_synth.h -- k_synth / seeqdevSynthReads: the synthetic reads of the benchmark, the tests and the text placement probe.
 * Included by seeq_device.hip (HIP_TRY, WG); no scan context involved.
 */
#ifndef SEEQ_SYNTH_H_
#define SEEQ_SYNTH_H_

/* ========================================================================== */
/* Synthetic reads (bench / test input; CPU twin: oracle/seeq_oracle.c)        */
/* ========================================================================== */
__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
   x += 0x9E3779B97F4A7C15ull;
   uint64_t z = x;
   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
   z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
   return z ^ (z >> 31);
}

struct SynthArgs {
   uint8_t *out;
   uint64_t first, n, seed;
   int len, plen, tau;
   char pattern[96];
};

__global__ __launch_bounds__(WG) void k_synth(SynthArgs s)
{
   const uint64_t k = (uint64_t)blockIdx.x * WG + threadIdx.x;
   if (k >= s.n) return;
   const uint64_t r = s.first + k;
   uint8_t *line = s.out + k * (uint64_t)(s.len + 1);
   const char B[4] = {'A', 'C', 'G', 'T'};
   for (int p = 0; p < s.len; p++) line[p] = B[splitmix64(s.seed ^ (r * 256 + (uint64_t)p)) >> 62];
   line[s.len] = '\n';
   const uint64_t hr = splitmix64(s.seed ^ 0xA5A5A5A5DEADBEEFull ^ (r * 0x100000001B3ull));
   if ((hr & 15) == 0 && s.plen > 0 && s.plen + s.tau + 2 <= 96 && s.plen + s.tau + 2 <= s.len) {
      char t[96];
      int cur = s.plen;
      for (int i = 0; i < s.plen; i++) t[i] = s.pattern[i];
      const int e = (int)((hr >> 4) % (uint64_t)(s.tau + 3));
      for (int q = 0; q < e; q++) {
         const uint64_t hk = splitmix64(hr + (uint64_t)q + 1);
         const int type = (int)(hk % 3);
         const int pos = (int)((hk >> 8) % (uint64_t)cur);
         const char b = B[(hk >> 40) & 3];
         if (type == 0) t[pos] = b;
         else if (type == 1) {
            for (int u = cur; u > pos; u--) t[u] = t[u - 1];
            t[pos] = b;
            cur++;
         } else if (cur > 1) {
            for (int u = pos; u < cur - 1; u++) t[u] = t[u + 1];
            cur--;
         }
      }
      const int off = (int)((hr >> 20) % (uint64_t)(s.len - cur + 1));
      for (int i = 0; i < cur; i++) line[off + i] = (uint8_t)t[i];
   }
   const uint64_t hn = splitmix64(s.seed ^ 0x5BD1E9955BD1E995ull ^ (r * 0x9E3779B1ull));
   if ((hn & 255) == 0) line[(hn >> 8) % (uint64_t)s.len] = 'N';
}

extern "C" int seeqdevSynthReads(void *d_out, uint64_t first, uint64_t n, int len, const char *pattern_plain, int plen,
                                 int tau, uint64_t seed, void *hip_stream)
{
   if (!d_out || len <= 0 || plen < 0 || plen > 96) { seeqerr = 0; errno = EINVAL; return -1; }
   if (n == 0) return 0;
   SynthArgs s;
   memset(&s, 0, sizeof s);
   s.out = (uint8_t *)d_out; s.first = first; s.n = n; s.seed = seed; s.len = len; s.plen = plen; s.tau = tau;
   memcpy(s.pattern, pattern_plain, (size_t)plen);
   const uint64_t blocks = (n + WG - 1) / WG;
   if (blocks > 0x7FFFFFFFull) { seeqerr = 0; errno = E2BIG; return -1; }
   hipLaunchKernelGGL(k_synth, dim3((unsigned)blocks), dim3(WG), 0, (hipStream_t)hip_stream, s);
   HIP_TRY(hipGetLastError(), EIO);
   return 0;
}

#endif
