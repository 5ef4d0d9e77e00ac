/*
 * seeq_tally.h -- how often each distinct sequence occurs among the spans of a record array: the inserts of an inserts call, or the
 * matches of a scan, packed into 64-bit keys where they lie in the resident text, sorted, and run-length counted -- all on the device.
 * No insert text is gathered and nothing but the table goes to the host.
 *
 * The rule -- plain C++ below, shared with the host driver (tests/tally_host_driver.cpp compiles this header with g++):
 *
 *   span        bytes [start, end) of a line whose first byte lies at `offset` in the text: words y, z of a 16-byte record (hit records
 *               and insert records alike) and the record's 8-byte line offset.
 *   key         of a span of L <= 31 bases, every byte one of ACGTUacgtu:  (1 << 2L) | sum of code(b_i) << 2(L - 1 - i),
 *               code = (ASCII >> 1) & 3 -- the packed path's code (seeq_amd.h, PACKED READ BATCHES): A 0, C 1, T/U 2, G 3.  The leading 1
 *               carries the length: the empty span has key 1, 31 x G has bits 0 .. 62 set, bit 63 is never set, and no key is 0.
 *   order       THE TABLE'S ORDER: keys ascending, which is by length first, then base by base with A < C < T < G.
 *   long        a span with L > 31; foreign: one with another byte (N included).  Neither is tallied, each kind is counted; a span that
 *               is both counts as long (the length is decided first, its bytes are not read).  Their key is 0, "not tallied".
 *   bad         a span with end < start, or one that reaches beyond the text's nbytes: no byte of it is loaded, the call fails (EIO).
 *   table       one {key, count} per distinct key, ascending.
 *   run head    a sorted key is a head iff it is nonzero and differs from its predecessor; an entry's count is the distance from its
 *               head to the next head, or to n.
 *   passes      an LSD radix sort by 8-bit digits needs ceil((2 * max_len + 1) / 8) of them, max_len the largest tallied length.
 *
 *   tally_span_load     (device) tally_span_key with the span's at most 32 text bytes in one or two 16-byte loads issued together (a loop
 *                       of byte loads waits for each in turn: 1.55 ms for 9 M spans, the whole tally 2.03 ms against 0.82 with the wide
 *                       loads): the one loader of the pack, the grouped tally's hold and its pair pack (seeq_tally_group.h).
 *   tally_tile_stat / tally_stat_top    (device) a tile's eight words {long, foreign, largest L, bad, a third count, key bits, sort flag, 0}
 *                       from the waves' numbers, and one workgroup's totals over the tiles: the one reducer of the same three kernels and
 *                       of k_tally_pack_top / k_tally_group_top.
 *   k_tally_pack        one thread per span, in the tiles of seeq_tiles.h (the sort's tile too): the key stored AT THE SPAN'S OWN INDEX
 *                       (0: not tallied); per tile its eight words (third count and key bits 0).
 *   k_tally_pack_top    one workgroup: the tiles' words -> the totals (one counters copy tells the host max_len).
 *   THE SORT, of items of one or two 64-bit words (TallySortArgs; the grouped tally's pairs are the two-word items): stable, least
 *   significant digit first, two arrays per word that swap roles; the hist and the scatter are templates on the word count, instantiated
 *   under four kernel names.  Per pass (the host's tally_sort_run, seeq_tally_host.h):
 *   k_tally_hist / k_tally_pair_hist    per tile the populations of the 256 values of the digit of the word the pass sorts by (LDS
 *                       counters) -> the digit-major matrix mat[digit][tile].
 *   k_tally_scan_reduce / _top / _apply    the exclusive scan of that matrix read as one array of 256 * tiles numbers, in the
 *                       three-launch shape: per chunk of 1 024 its sum, one workgroup scans the chunk sums, per chunk the scan with
 *                       its base.  mat[d][t] is then where tile t's first item of digit d goes.
 *   k_tally_scatter / k_tally_pair_scatter    a tile's items again: an item's rank among the tile's items of its digit is (items of the
 *                       digit in earlier rounds and waves, from LDS: a wave's count per digit is written by the lowest lane that holds the
 *                       digit) + (lanes below it in its wave that hold the digit: eight ballots on the digit's bits); a tile's order is
 *                       round, wave, lane = ascending index, so the sort is stable; every word of the item is moved.  Every pass is done
 *                       properly: its histogram is taken from the arrays it permutes (an earlier pass moves items between tiles, so only
 *                       pass 0's per-tile populations could be had from the unsorted keys).  A tile whose index left the array sets its
 *                       flag word (pointer and stride in the arguments), which the *_rle_top kernel ors in.
 *   and over the sorted keys the reduce / top / apply of seeq_tiles.h:
 *   k_tally_rle_reduce  per tile: heads, nonzero keys.
 *   k_tally_rle_top     one workgroup: exclusive scan of the tiles' heads in place; ndistinct, the nonzero keys, the tiles' flags.
 *   k_tally_rle_apply   the ordered compaction of the heads: head j's index in the sorted array -> pos[j] (in the key array the last
 *                       pass left free).
 *   k_tally_table       one thread per entry: {key, pos[j + 1] (or n) - pos[j]}, one 16-byte store.
 *
 * Every output slot is written by exactly one thread; no atomics on global memory at all (flags are per tile), no workgroup waits on
 * another, every loop is bounded by a count the host knows, the grids come from host-known counts (no spans: nothing is launched).
 */
#ifndef SEEQ_TALLY_H_
#define SEEQ_TALLY_H_

#include <stdint.h>

#include "seeq_strand.h"                                    /* SEEQ_ST_HD, strand_rec_t */

#define SEEQ_TALLY_WG      SEEQ_TILE_WG                     /* (the host driver prints the shape under the tally's names) */
#define SEEQ_TALLY_ITEMS   SEEQ_TILE_ITEMS
#define SEEQ_TALLY_TILE    1024                             /* the sort's tile = SEEQ_TILE, as a number: the tests read it from this file */
static_assert(SEEQ_TALLY_TILE == SEEQ_TILE, "the tally's tile is seeq_tiles.h's");
#define SEEQ_TALLY_RADIX   256                             /* values of an 8-bit digit = SEEQ_TILE_WG: a thread per digit value */
#define SEEQ_TALLY_CHUNK   1024                             /* matrix entries per workgroup of the offsets scan = SEEQ_TILE */
#define SEEQ_TALLY_LEN_MAX 31                               /* = SEEQDEV_TALLY_MAX_LEN (seeq_amd.h) */

#define SEEQ_TALLY_OK      0                                /* what a span is */
#define SEEQ_TALLY_LONG    1
#define SEEQ_TALLY_FOREIGN 2
#define SEEQ_TALLY_BAD     3

/* is the byte one of ACGTUacgtu? */
SEEQ_ST_HD int tally_is_base(uint8_t c)
{
   const uint8_t up = (uint8_t)(c & 0xDFu);
   return up == 'A' || up == 'C' || up == 'G' || up == 'T' || up == 'U';
}

SEEQ_ST_HD uint64_t tally_code(uint8_t c) { return (uint64_t)((c >> 1) & 3u); }

/* The key of the len <= SEEQ_TALLY_LEN_MAX bytes at seq; 0 (no key is): one of them is no base. */
SEEQ_ST_HD uint64_t tally_key_of(const uint8_t *seq, uint32_t len)
{
   uint64_t key = 1u;
   int foreign = 0;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
   for (uint32_t i = 0; i < SEEQ_TALLY_LEN_MAX; i++) {
      if (i >= len) break;
      const uint8_t c = seq[i];
      foreign |= !tally_is_base(c);
      key = (key << 2) | tally_code(c);
   }
   return foreign ? 0u : key;
}

/* The same for bytes held in eight little-endian words (byte i in word i / 4): what a thread of k_tally_pack has after its two 16-byte loads. */
SEEQ_ST_HD uint64_t tally_key_of_words(const uint32_t w[8], uint32_t len)
{
   uint64_t key = 1u;
   int foreign = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
   for (uint32_t i = 0; i < SEEQ_TALLY_LEN_MAX; i++) {
      if (i >= len) continue;
      const uint8_t c = (uint8_t)(w[i >> 2] >> (8u * (i & 3u)));
      foreign |= !tally_is_base(c);
      key = (key << 2) | tally_code(c);
   }
   return foreign ? 0u : key;
}

/* What the span [start, end) of the line at `off` in a text of nbytes is before any byte of it is read: SEEQ_TALLY_BAD, SEEQ_TALLY_LONG, or
   SEEQ_TALLY_OK for one whose bytes decide; *len: its length (0 when bad). */
SEEQ_ST_HD int tally_span_kind(uint64_t nbytes, uint64_t off, uint32_t start, uint32_t end, uint32_t *len)
{
   *len = 0u;
   if (end < start || off > nbytes || (uint64_t)end > nbytes - off) return SEEQ_TALLY_BAD;
   *len = end - start;
   return *len > SEEQ_TALLY_LEN_MAX ? SEEQ_TALLY_LONG : SEEQ_TALLY_OK;
}

/* What the span is, and *key: its key (0 unless SEEQ_TALLY_OK).  Nothing outside [0, nbytes) is read, and nothing at all of a long or
   bad span. */
SEEQ_ST_HD int tally_span_key(const uint8_t *text, uint64_t nbytes, uint64_t off, uint32_t start, uint32_t end, uint64_t *key, uint32_t *len)
{
   *key = 0u;
   const int kind = tally_span_kind(nbytes, off, start, end, len);
   if (kind != SEEQ_TALLY_OK) return kind;
   *key = tally_key_of(text + off + start, *len);
   return *key ? SEEQ_TALLY_OK : SEEQ_TALLY_FOREIGN;
}

/* The length a key carries: the position of its leading 1, halved; -1: no key (0, bit 63 set, or a leading 1 at an odd position). */
SEEQ_ST_HD int tally_key_len(uint64_t key)
{
   if (key == 0u || (key >> 63)) return -1;
   const int top = 63 - __builtin_clzll(key);
   return (top & 1) ? -1 : top / 2;
}

/* key -> its bases, upper case by code (A C T G), out[len] = 0; returns the length, -1: no key. */
SEEQ_ST_HD int tally_decode(uint64_t key, char out[32])
{
   const int len = tally_key_len(key);
   if (len < 0) return -1;
   for (int i = 0; i < len; i++) out[i] = "ACTG"[(key >> (2 * (len - 1 - i))) & 3u];
   out[len] = 0;
   return len;
}

/* passes of the sort for keys of at most max_len bases: their 2 * max_len + 1 bits in digits of 8 */
SEEQ_ST_HD uint32_t tally_passes(uint32_t max_len) { return (2u * max_len + 1u + 7u) / 8u; }

/* the digit pass number `pass` sorts by */
SEEQ_ST_HD uint32_t tally_digit(uint64_t key, uint32_t pass) { return (uint32_t)(key >> (8u * pass)) & 255u; }

/* does a run begin at a sorted key?  (first: the key has no predecessor) */
SEEQ_ST_HD int tally_is_head(uint64_t key, uint64_t prev, int first) { return key != 0u && (first || key != prev); }

/* tiles of n keys; entries of their digit matrix; chunks of its scan */
SEEQ_ST_HD uint64_t tally_tiles(uint64_t n) { return (n + SEEQ_TILE - 1) / SEEQ_TILE; }
SEEQ_ST_HD uint64_t tally_matrix(uint64_t n) { return tally_tiles(n) * SEEQ_TALLY_RADIX; }
SEEQ_ST_HD uint64_t tally_chunks(uint64_t n) { return (tally_matrix(n) + SEEQ_TALLY_CHUNK - 1) / SEEQ_TALLY_CHUNK; }

#if defined(__HIPCC__)

static_assert(SEEQ_TALLY_RADIX == SEEQ_TILE_WG && SEEQ_TALLY_CHUNK == SEEQ_TILE, "tally radix / chunk");

struct TallyCnt {
   uint32_t nlong, nforeign;          /* spans not tallied, by kind */
   uint32_t max_len;                  /* the largest tallied length */
   uint32_t bad;                      /* 1: a span outside the text; 2: an index outside an array (an internal error) */
   uint32_t ndistinct;                /* heads of the sorted keys */
   uint32_t nonzero;                  /* nonzero keys among them: the tallied spans */
   uint32_t first;                    /* index of the first head: the keys that are 0 */
   uint32_t pad;
};

#define SEEQ_TALLY_STAT 8                                   /* words per tile: {long, foreign, largest L, bad, third count, key bits, sort flag, 0} */
#define SEEQ_TALLY_STAT_FLAG 6                              /* the word a scatter sets when an index left its array */

struct TallyArgs {
   const uint4    *rec;               /* [n] the records whose spans are tallied */
   const uint64_t *off;               /* [n] their line offsets */
   uint32_t        n;
   uint32_t        nt;                /* tiles = workgroups of the per-tile kernels */
   const uint8_t  *text;
   uint64_t        nbytes;
   uint64_t       *src, *dst;         /* [n] the keys: the pack writes src, the sort leaves them in src and dst free */
   uint32_t       *tstat;             /* [8 * nt] the tiles' words (tally_tile_stat) */
   uint32_t       *rsum;              /* [2 * nt] per tile heads (k_tally_rle_top: exclusive prefix), nonzero keys */
   uint32_t        nd;                /* entries of the table */
   uint32_t       *pos;               /* [nd] the heads' indices */
   uint4          *tab;               /* [cap_tab] the table */
   uint32_t        cap_tab;
   TallyCnt       *cnt;
};

/* What the sort's kernels take: items of one or two 64-bit words (the template argument of the hist and scatter bodies), moved together. */
struct TallySortArgs {
   uint32_t        n;
   uint32_t        nt;                /* tiles = workgroups of the hist and the scatter */
   uint64_t       *src[2], *dst[2];   /* per word: [n] what a pass reads / writes; they swap roles after every pass */
   uint32_t        word, pass;        /* the word a pass sorts by and the digit of it */
   uint32_t       *mat;               /* [nmat] digit-major: mat[d * nt + t] */
   uint32_t        nmat, nb;          /* 256 * nt entries; chunks of the scan = its workgroups */
   uint32_t       *bsum;              /* [nb] the chunks' sums (k_tally_scan_top: exclusive prefix) */
   uint32_t       *flag;              /* flag[fstride * tile] = 2 by a scatter whose index left its array: a word the *_rle_top kernel ors in */
   uint32_t        fstride;
};

__device__ __forceinline__ uint32_t tally_wave_max(uint32_t v)
{
#pragma unroll
   for (int d = 32; d >= 1; d >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64);
      v = o > v ? o : v;
   }
   return v;
}

/* What the span [start, end) of the line at `off` is, and its key (0 unless SEEQ_TALLY_OK): tally_span_key with the span's bytes in one or
   two unaligned 16-byte loads where 16 / 32 bytes from its first one lie inside the text (all but the last spans of a text), byte by byte
   elsewhere; nothing of a long or bad span. */
__device__ __forceinline__ int tally_span_load(const uint8_t *text, uint64_t nbytes, uint64_t off, uint32_t start, uint32_t end, uint64_t *key, uint32_t *len)
{
   *key = 0u;
   const int kind = tally_span_kind(nbytes, off, start, end, len);
   if (kind != SEEQ_TALLY_OK) return kind;
   const uint64_t p = off + start;
   const uint32_t nvec = *len > 16u ? 2u : 1u;
   if (*len == 0u) {
      *key = 1u;
   } else if (p + 16u * nvec <= nbytes) {
      const fused_v4u v0 = *(const fused_v4u_unaligned *)(text + p);
      fused_v4u v1 = {0u, 0u, 0u, 0u};
      if (nvec == 2u) v1 = *(const fused_v4u_unaligned *)(text + p + 16);
      const uint32_t w[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
      *key = tally_key_of_words(w, *len);
   } else {
      *key = tally_key_of(text + p, *len);
   }
   return *key ? SEEQ_TALLY_OK : SEEQ_TALLY_FOREIGN;
}

/* A tile's words: three wave-uniform counts, three values of this lane (two maxima, a flag) -> tstat[8 * tile ..], by thread 0. */
__device__ __forceinline__ void tally_tile_stat(uint32_t nlong, uint32_t nfor, uint32_t third, uint32_t maxl, uint32_t bits, uint32_t bad,
                                                uint32_t (&s_st)[6][SEEQ_TILE_WAVES], uint32_t *tstat)
{
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   maxl = tally_wave_max(maxl);
   bits = tally_wave_max(bits);
   bad = __ballot(bad != 0u) != 0ull ? 1u : 0u;
   if (lane == 0) { s_st[0][wave] = nlong; s_st[1][wave] = nfor; s_st[2][wave] = maxl; s_st[3][wave] = bad; s_st[4][wave] = third; s_st[5][wave] = bits; }
   __syncthreads();
   if (threadIdx.x == 0) {
      uint32_t t[SEEQ_TALLY_STAT] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
      for (int w = 0; w < SEEQ_TILE_WAVES; w++) {
         t[0] += s_st[0][w]; t[1] += s_st[1][w]; t[4] += s_st[4][w];
         t[2] = s_st[2][w] > t[2] ? s_st[2][w] : t[2];
         t[5] = s_st[5][w] > t[5] ? s_st[5][w] : t[5];
         t[3] |= s_st[3][w];
      }
      uint4 *out = (uint4 *)(tstat + (size_t)SEEQ_TALLY_STAT * blockIdx.x);
      out[0] = make_uint4(t[0], t[1], t[2], t[3]);
      out[1] = make_uint4(t[4], t[5], 0u, 0u);
   }
}

/* One workgroup: the nt tiles' words -> t[0 .. 6), in the words' order: sums of words 0, 1, 4; maxima of 2, 5; word 3 or-ed (valid in
   thread 0). */
__device__ __forceinline__ void tally_stat_top(const uint32_t *tstat, uint32_t nt, uint32_t *s_wave /* >= 4 */, uint32_t (&s_st)[3][SEEQ_TILE_WAVES], uint32_t (&t)[6])
{
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   uint32_t nlong = 0, nfor = 0, third = 0, maxl = 0, bits = 0, bad = 0;
   for (uint32_t b0 = 0; b0 < nt; b0 += SEEQ_TILE_WG) {
      const uint32_t i = b0 + threadIdx.x;
      if (i < nt) {
         const uint4 *row = (const uint4 *)(tstat + (size_t)SEEQ_TALLY_STAT * i);
         const uint4 t0 = row[0], t1 = row[1];
         nlong += t0.x; nfor += t0.y; maxl = t0.z > maxl ? t0.z : maxl; bad |= t0.w;
         third += t1.x; bits = t1.y > bits ? t1.y : bits;
      }
   }
   block_excl_scan(nlong, &t[0], s_wave);
   block_excl_scan(nfor, &t[1], s_wave);
   block_excl_scan(third, &t[4], s_wave);
   maxl = tally_wave_max(maxl);
   bits = tally_wave_max(bits);
   bad = __ballot(bad != 0u) != 0ull ? 1u : 0u;
   if (lane == 0) { s_st[0][wave] = maxl; s_st[1][wave] = bits; s_st[2][wave] = bad; }
   __syncthreads();
   if (threadIdx.x == 0) {
      for (int w = 0; w < SEEQ_TILE_WAVES; w++) { maxl = s_st[0][w] > maxl ? s_st[0][w] : maxl; bits = s_st[1][w] > bits ? s_st[1][w] : bits; bad |= s_st[2][w]; }
      t[2] = maxl; t[3] = bad; t[5] = bits;
   }
}

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_pack(TallyArgs a)
{
   __shared__ uint32_t s_st[6][SEEQ_TILE_WAVES];
   uint32_t nlong = 0, nfor = 0;                            /* wave-uniform */
   uint32_t maxl = 0, bad = 0;                              /* this lane's */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      int kind = -1;
      if (i < a.n) {
         const uint4 r = a.rec[i];
         uint64_t key;
         uint32_t len;
         kind = tally_span_load(a.text, a.nbytes, a.off[i], r.y, r.z, &key, &len);
         a.src[i] = key;
         if (kind == SEEQ_TALLY_OK && len > maxl) maxl = len;
         if (kind == SEEQ_TALLY_BAD) bad = 1u;
      }
      nlong += (uint32_t)__popcll(__ballot(kind == SEEQ_TALLY_LONG));
      nfor += (uint32_t)__popcll(__ballot(kind == SEEQ_TALLY_FOREIGN));
   }
   tally_tile_stat(nlong, nfor, 0u, maxl, 0u, bad, s_st, a.tstat);
}

/* One workgroup: the tiles' {long, foreign, largest L, bad} -> the totals. */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_pack_top(TallyArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES], s_st[3][SEEQ_TILE_WAVES];
   uint32_t t[6];
   tally_stat_top(a.tstat, a.nt, s_wave, s_st, t);
   if (threadIdx.x == 0) { a.cnt->nlong = t[0]; a.cnt->nforeign = t[1]; a.cnt->max_len = t[2]; a.cnt->bad = t[3]; }
}

/* THE SORT'S KERNELS.  The hist and the scatter are written once, for items of W words; their four instantiations keep the names the
   profiles know: k_tally_hist / k_tally_scatter (W = 1), k_tally_pair_hist / k_tally_pair_scatter (W = 2). */
template <int W>
__device__ __forceinline__ void tally_hist_tile(const TallySortArgs &a)
{
   __shared__ uint32_t s_h[SEEQ_TALLY_RADIX];
   const uint64_t *src = W > 1 && a.word ? a.src[1] : a.src[0];
   s_h[threadIdx.x] = 0u;
   __syncthreads();
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      if (i < a.n) atomicAdd(&s_h[tally_digit(src[i], a.pass)], 1u);      /* (LDS) */
   }
   __syncthreads();
   a.mat[(uint64_t)threadIdx.x * a.nt + blockIdx.x] = s_h[threadIdx.x];
}

template <int W>
__device__ __forceinline__ void tally_scatter_tile(const TallySortArgs &a)
{
   __shared__ uint32_t s_cnt[SEEQ_TILE_ITEMS * SEEQ_TILE_WAVES][SEEQ_TALLY_RADIX];      /* [round][wave] per digit: count, then destination */
   __shared__ uint32_t s_bad;
   constexpr int ROWS = SEEQ_TILE_ITEMS * SEEQ_TILE_WAVES;
   const int wave = threadIdx.x >> 6;
#pragma unroll
   for (int r = 0; r < ROWS; r++) s_cnt[r][threadIdx.x] = 0u;
   if (threadIdx.x == 0) s_bad = 0u;
   __syncthreads();
   uint64_t key[W][SEEQ_TILE_ITEMS];
   uint32_t dg[SEEQ_TILE_ITEMS], within[SEEQ_TILE_ITEMS];
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      const bool act = i < a.n;
#pragma unroll
      for (int w = 0; w < W; w++) key[w][k] = act ? a.src[w][i] : 0u;
      dg[k] = tally_digit(W > 1 && a.word ? key[W - 1][k] : key[0][k], a.pass);
      uint64_t same = __ballot(act);                        /* the wave's lanes that hold an item of this lane's digit */
#pragma unroll
      for (int b = 0; b < 8; b++) {
         const bool bit = (dg[k] >> b) & 1u;
         const uint64_t bal = __ballot(bit);
         same &= bit ? bal : ~bal;
      }
      within[k] = __builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0u));
      if (act && within[k] == 0u) s_cnt[k * SEEQ_TILE_WAVES + wave][dg[k]] = (uint32_t)__popcll(same);
   }
   __syncthreads();
   {
      uint32_t run = a.mat[(uint64_t)threadIdx.x * a.nt + blockIdx.x];      /* where the tile's first item of digit tid goes */
#pragma unroll
      for (int r = 0; r < ROWS; r++) {
         const uint32_t c = s_cnt[r][threadIdx.x];
         s_cnt[r][threadIdx.x] = run;
         run += c;
      }
   }
   __syncthreads();
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      if (i >= a.n) continue;
      const uint32_t j = s_cnt[k * SEEQ_TILE_WAVES + wave][dg[k]] + within[k];
      if (j < a.n) {
#pragma unroll
         for (int w = 0; w < W; w++) a.dst[w][j] = key[w][k];
      } else {
         s_bad = 1u;
      }
   }
   __syncthreads();
   if (threadIdx.x == 0 && s_bad) a.flag[(size_t)a.fstride * blockIdx.x] = 2u;
}

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_hist(TallySortArgs a) { tally_hist_tile<1>(a); }
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_pair_hist(TallySortArgs a) { tally_hist_tile<2>(a); }
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_scatter(TallySortArgs a) { tally_scatter_tile<1>(a); }
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_pair_scatter(TallySortArgs a) { tally_scatter_tile<2>(a); }

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_scan_reduce(TallySortArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES];
   const uint64_t base = (uint64_t)blockIdx.x * SEEQ_TALLY_CHUNK;
   uint32_t v = 0;
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = base + (uint64_t)k * SEEQ_TILE_WG + threadIdx.x;
      if (i < a.nmat) v += a.mat[i];
   }
   uint32_t tot;
   block_excl_scan(v, &tot, s_wave);
   if (threadIdx.x == 0) a.bsum[blockIdx.x] = tot;
}

/* One workgroup: bsum[0 .. nb) -> its exclusive prefix, in place. */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_scan_top(TallySortArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES];
   uint32_t tot[1];
   tile_top(a.bsum, a.nb, s_wave, tot);
}

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_scan_apply(TallySortArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES];
   const uint64_t base = (uint64_t)blockIdx.x * SEEQ_TALLY_CHUNK;
   uint32_t running = a.bsum[blockIdx.x];
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = base + (uint64_t)k * SEEQ_TILE_WG + threadIdx.x;
      const uint32_t v = i < a.nmat ? a.mat[i] : 0u;
      uint32_t tot;
      const uint32_t ex = block_excl_scan(v, &tot, s_wave);
      if (i < a.nmat) a.mat[i] = running + ex;
      running += tot;
   }
}

/* the run-length pass: the reduce / top / apply of seeq_tiles.h over the sorted keys */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_rle_reduce(TallyArgs a)
{
   __shared__ uint32_t s_sum[2][SEEQ_TILE_WAVES];
   uint32_t sum[2] = {0u, 0u};                              /* heads, nonzero keys: wave-uniform */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      bool head = false, nonzero = false;
      if (i < a.n) {
         const uint64_t key = a.src[i];
         nonzero = key != 0u;
         head = tally_is_head(key, i ? a.src[i - 1] : 0u, i == 0);
      }
      sum[0] += (uint32_t)__popcll(__ballot(head));
      sum[1] += (uint32_t)__popcll(__ballot(nonzero));
   }
   tile_sums(sum, s_sum, a.rsum, a.nt);
}

/* One workgroup: rsum[0 .. nt) -> its exclusive prefix, in place; ndistinct, the nonzero keys, the tiles' flags since the pack. */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_rle_top(TallyArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES], s_bad[SEEQ_TILE_WAVES];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   uint32_t tot[2], bad = 0;
   tile_top(a.rsum, a.nt, s_wave, tot);
   for (uint32_t i = threadIdx.x; i < a.nt; i += SEEQ_TILE_WG) bad |= a.tstat[(size_t)SEEQ_TALLY_STAT * i + SEEQ_TALLY_STAT_FLAG];
   bad = __ballot(bad != 0u) != 0ull ? 2u : 0u;
   if (lane == 0) s_bad[wave] = bad;
   __syncthreads();
   if (threadIdx.x == 0) {
      for (int w = 0; w < SEEQ_TILE_WAVES; w++) bad |= s_bad[w];
      a.cnt->ndistinct = tot[0]; a.cnt->nonzero = tot[1]; a.cnt->bad = bad;
   }
}

/* the ordered compaction of the heads: a head's index goes to its rank in pos */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_rle_apply(TallyArgs a)
{
   __shared__ uint32_t s_cnt[SEEQ_TILE_ITEMS][SEEQ_TILE_WAVES];
   bool head[SEEQ_TILE_ITEMS];
   uint32_t within[SEEQ_TILE_ITEMS];                        /* heads of the wave's round before this lane */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      head[k] = i < a.n && tally_is_head(a.src[i], i ? a.src[i - 1] : 0u, i == 0);
      within[k] = tile_wave_rank(head[k], s_cnt[k]);
   }
   __syncthreads();
   uint32_t rank0 = a.rsum[blockIdx.x];                     /* heads before this tile, then before this round */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint32_t j = tile_place(rank0, within[k], s_cnt[k]);
      if (head[k] && j < a.nd) a.pos[j] = (uint32_t)tile_index(k);      /* (nd is the sum of these very heads: k_tally_rle_top) */
   }
}

/* One thread per entry of the table; the first head's index goes to the counters (the host checks it against the tallied spans). */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_table(TallyArgs a)
{
   const uint64_t j = (uint64_t)blockIdx.x * SEEQ_TILE_WG + threadIdx.x;
   if (j >= a.nd || j >= a.cap_tab) return;
   const uint32_t p = a.pos[j];
   const uint32_t next = j + 1 < a.nd ? a.pos[j + 1] : a.n;
   if (j == 0) a.cnt->first = p;
   if (p >= a.n || next <= p || next > a.n) { a.tab[j] = make_uint4(0u, 0u, 0u, 0u); return; }
   const uint64_t key = a.src[p];
   const uint64_t count = (uint64_t)(next - p);
   a.tab[j] = make_uint4((uint32_t)key, (uint32_t)(key >> 32), (uint32_t)count, (uint32_t)(count >> 32));
}

#endif   /* __HIPCC__ */
#endif
