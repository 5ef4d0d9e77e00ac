/*
 * seeq_scan.h -- the exclusive prefix scans of the host drivers, each three launches or one, with their launchers:
 *   k_scan_reduce / _top / _apply<XF>   u32 items with a device-side length (launch_scan)
 *   k_scanset_reduce / _top / _apply    up to three arrays of one host-known length in place (launch_scanset)
 *   k_scan_tiles                        one workgroup, host-known length (the newline index)
 * Included by seeq_device.hip after seeq_scan_common.h (block_excl_scan) and its WG constant.  The launchers take the stream and the
 * block-sum workspace (the context's scan_ws: reserve_impl sizes it); seeq_multi.h scans with SCAN_BLOCK / SCAN_ITEMS too.
 */
#ifndef SEEQ_SCAN_H_
#define SEEQ_SCAN_H_

/* ========================================================================== */
/* Generic two-level exclusive scan over u32 items with a device-side length   */
/*   XF 0: in = u32[];  XF 1: in = u64[], item = popcount;  XF 2: u32 != 0     */
/*   n = (*n_ptr + add) >> shift                                              */
/* ========================================================================== */
static constexpr int SCAN_ITEMS = 8;                     /* per thread */
static constexpr int SCAN_BLOCK = WG * SCAN_ITEMS;       /* 2048 per block */

template <int XF>
__device__ __forceinline__ uint32_t scan_item(const void *in, uint32_t i)
{
   if (XF == 0) return reinterpret_cast<const uint32_t *>(in)[i];
   if (XF == 2) return reinterpret_cast<const uint32_t *>(in)[i] != 0u ? 1u : 0u;
   return (uint32_t)__popcll(reinterpret_cast<const uint64_t *>(in)[i]);
}

template <int XF>
__global__ __launch_bounds__(WG) void k_scan_reduce(const void *in, uint32_t *bsum, const uint32_t *n_ptr, uint32_t add,
                                                    uint32_t shift)
{
   __shared__ uint32_t s_wave[4];
   const uint32_t n = n_ptr ? (*n_ptr + add) >> shift : add;
   const uint32_t base = blockIdx.x * SCAN_BLOCK;
   if (base >= n) return;
   uint32_t v = 0;
#pragma unroll
   for (int k = 0; k < SCAN_ITEMS; k++) {
      const uint32_t i = base + threadIdx.x * SCAN_ITEMS + k;
      if (i < n) v += scan_item<XF>(in, i);
   }
   uint32_t tot;
   block_excl_scan(v, &tot, s_wave);
   if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

/* One block: exclusive scan of bsum[0..nb) in place, total -> *total_out. */
__global__ __launch_bounds__(WG) void k_scan_top(uint32_t *bsum, const uint32_t *n_ptr, uint32_t add, uint32_t shift,
                                                 uint32_t *total_out)
{
   __shared__ uint32_t s_wave[4];
   const uint32_t n = n_ptr ? (*n_ptr + add) >> shift : add;
   const uint32_t nb = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
   uint32_t running = 0;
   for (uint32_t b0 = 0; b0 < nb; b0 += WG) {
      const uint32_t i = b0 + threadIdx.x;
      const uint32_t v = i < nb ? bsum[i] : 0;
      uint32_t tot;
      const uint32_t ex = block_excl_scan(v, &tot, s_wave);
      if (i < nb) bsum[i] = running + ex;
      running += tot;
   }
   if (threadIdx.x == 0) *total_out = running;
}

template <int XF>
__global__ __launch_bounds__(WG) void k_scan_apply(const void *in, uint32_t *out, const uint32_t *bsum,
                                                   const uint32_t *n_ptr, uint32_t add, uint32_t shift)
{
   __shared__ uint32_t s_wave[4];
   const uint32_t n = n_ptr ? (*n_ptr + add) >> shift : add;
   const uint32_t base = blockIdx.x * SCAN_BLOCK;
   if (base >= n) return;
   uint32_t item[SCAN_ITEMS];
   uint32_t v = 0;
#pragma unroll
   for (int k = 0; k < SCAN_ITEMS; k++) {
      const uint32_t i = base + threadIdx.x * SCAN_ITEMS + k;
      item[k] = i < n ? scan_item<XF>(in, i) : 0;
      v += item[k];
   }
   uint32_t tot;
   uint32_t ex = block_excl_scan(v, &tot, s_wave) + bsum[blockIdx.x];
#pragma unroll
   for (int k = 0; k < SCAN_ITEMS; k++) {
      const uint32_t i = base + threadIdx.x * SCAN_ITEMS + k;
      if (i < n) out[i] = ex;
      ex += item[k];
   }
}

/* Up to three u32 arrays of the same host-known length scanned in place by ONE set of three launches (the per-tile
 * arrays of the one-pass kernels): blockIdx.y selects the array, bsum has one region of `nb` partial sums per array. */
struct ScanSet { uint32_t *arr[3]; uint32_t *total[3]; };

__global__ __launch_bounds__(WG) void k_scanset_reduce(ScanSet ss, uint32_t *bsum, uint32_t n, uint32_t nb)
{
   __shared__ uint32_t s_wave[4];
   const uint32_t *in = ss.arr[blockIdx.y];
   const uint32_t base = blockIdx.x * SCAN_BLOCK;
   uint32_t v = 0;
#pragma unroll
   for (int k = 0; k < SCAN_ITEMS; k++) {
      const uint32_t i = base + threadIdx.x * SCAN_ITEMS + k;
      if (i < n) v += in[i];
   }
   uint32_t tot;
   block_excl_scan(v, &tot, s_wave);
   if (threadIdx.x == 0) bsum[blockIdx.y * nb + blockIdx.x] = tot;
}

__global__ __launch_bounds__(WG) void k_scanset_top(ScanSet ss, uint32_t *bsum, uint32_t nb)
{
   __shared__ uint32_t s_wave[4];
   uint32_t *b = bsum + blockIdx.x * nb;
   uint32_t running = 0;
   for (uint32_t b0 = 0; b0 < nb; b0 += WG) {
      const uint32_t i = b0 + threadIdx.x;
      const uint32_t v = i < nb ? b[i] : 0;
      uint32_t tot;
      const uint32_t ex = block_excl_scan(v, &tot, s_wave);
      if (i < nb) b[i] = running + ex;
      running += tot;
      __syncthreads();
   }
   if (threadIdx.x == 0 && ss.total[blockIdx.x]) *ss.total[blockIdx.x] = running;
}

__global__ __launch_bounds__(WG) void k_scanset_apply(ScanSet ss, const uint32_t *bsum, uint32_t n, uint32_t nb)
{
   __shared__ uint32_t s_wave[4];
   uint32_t *arr = ss.arr[blockIdx.y];
   const uint32_t base = blockIdx.x * SCAN_BLOCK;
   uint32_t item[SCAN_ITEMS];
   uint32_t v = 0;
#pragma unroll
   for (int k = 0; k < SCAN_ITEMS; k++) {
      const uint32_t i = base + threadIdx.x * SCAN_ITEMS + k;
      item[k] = i < n ? arr[i] : 0;
      v += item[k];
   }
   uint32_t tot;
   uint32_t ex = block_excl_scan(v, &tot, s_wave) + bsum[blockIdx.y * nb + blockIdx.x];
#pragma unroll
   for (int k = 0; k < SCAN_ITEMS; k++) {
      const uint32_t i = base + threadIdx.x * SCAN_ITEMS + k;
      if (i < n) arr[i] = ex;
      ex += item[k];
   }
}

/* The tile_cnt scan has a host-known length (ntiles); a dedicated small kernel
 * avoids routing a host constant through device memory. */
__global__ __launch_bounds__(WG) void k_scan_tiles(uint32_t *tile_cnt, uint32_t ntiles, uint32_t *total_out)
{
   __shared__ uint32_t s_wave[4];
   uint32_t running = 0;
   for (uint32_t b0 = 0; b0 < ntiles; b0 += WG * SCAN_ITEMS) {
      uint32_t item[SCAN_ITEMS];
      uint32_t v = 0;
#pragma unroll
      for (int k = 0; k < SCAN_ITEMS; k++) {
         const uint32_t i = b0 + threadIdx.x * SCAN_ITEMS + k;
         item[k] = i < ntiles ? tile_cnt[i] : 0;
         v += item[k];
      }
      uint32_t tot;
      uint32_t ex = running + block_excl_scan(v, &tot, s_wave);
#pragma unroll
      for (int k = 0; k < SCAN_ITEMS; k++) {
         const uint32_t i = b0 + threadIdx.x * SCAN_ITEMS + k;
         if (i < ntiles) tile_cnt[i] = ex;
         ex += item[k];
      }
      running += tot;
   }
   if (threadIdx.x == 0) *total_out = running;
}

/* ---- launch helpers (bsum: room for the block sums -- one per SCAN_BLOCK items, per array of a set) ---- */
template <int XF>
static void launch_scan(hipStream_t st, uint32_t *bsum, const void *in, uint32_t *out, size_t cap_items, const uint32_t *n_ptr,
                        uint32_t add, uint32_t shift, uint32_t *total_out)
{
   const unsigned nb = (unsigned)((cap_items + SCAN_BLOCK - 1) / SCAN_BLOCK);
   if (nb == 0) return;
   hipLaunchKernelGGL(k_scan_reduce<XF>, dim3(nb), dim3(WG), 0, st, in, bsum, n_ptr, add, shift);
   hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(WG), 0, st, bsum, n_ptr, add, shift, total_out);
   hipLaunchKernelGGL(k_scan_apply<XF>, dim3(nb), dim3(WG), 0, st, in, out, (const uint32_t *)bsum,
                      n_ptr, add, shift);
}

static void launch_scanset(hipStream_t st, uint32_t *bsum, uint32_t *a0, uint32_t *a1, uint32_t *a2, uint32_t n, uint32_t *t0, uint32_t *t1, uint32_t *t2)
{
   const unsigned nb = (unsigned)((n + SCAN_BLOCK - 1) / SCAN_BLOCK);
   if (nb == 0) return;
   ScanSet ss = {{a0, a1, a2}, {t0, t1, t2}};
   const unsigned na = a2 ? 3 : a1 ? 2 : 1;
   hipLaunchKernelGGL(k_scanset_reduce, dim3(nb, na), dim3(WG), 0, st, ss, bsum, n, nb);
   hipLaunchKernelGGL(k_scanset_top, dim3(na), dim3(WG), 0, st, ss, bsum, nb);
   hipLaunchKernelGGL(k_scanset_apply, dim3(nb, na), dim3(WG), 0, st, ss, (const uint32_t *)bsum, n, nb);
}

#endif
