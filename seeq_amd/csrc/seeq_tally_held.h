/*
 * seeq_tally_held.h -- the tally of the HELD column itself: how often each distinct held word occurs, one count per line, with no member
 * column at all.  The bulk pooled screen -- sample barcode x guide, no UMI -- composes (sample << w) | guide_id with a hold and an append
 * (seeq_tally_append.h); the composed word is exactly its key, and this entry sorts and run-length counts it on the device.  The key table
 * is a sparse matrix in row order (rows: the leading columns of the word, columns: its last member_columns columns), the row table its row
 * index, and k_tally_held_dense scatters the key table into the dense sample x guide matrix a screen wants.
 *
 * The rule -- plain C++ below, shared with the host driver (tests/tally_held_host_driver.cpp compiles this header with g++):
 *
 *   held column  line[i], key[i] for i < n, in record order (seeq_tally_group.h); lines do not decrease.
 *   kind         record i OPENS its line iff i == 0 or line[i - 1] != line[i].  A record that does not is a REPEAT; one that does and has
 *                key 0 is KEYLESS; one that does and has a key is COUNTED.  A line is counted at most once and its FIRST held record
 *                decides (tally_group_of's rule): a line whose first record has no key is not counted, whatever follows on it.
 *                n = ncounted + nkeyless + nrepeat.
 *   split        member_columns = m, 0 <= m < ncolumns: shift = the sum of the widths of the LAST m columns; the row of a key is
 *                key >> shift, its column part key & ((1 << shift) - 1).  m == 0: shift 0, every key is a row of its own and no row table
 *                is made.
 *   sort         the counted keys as they are, every other record as key 0, by the tally's stable single-word LSD sort:
 *                ceil(key_bits / 8) passes, key_bits the bit length of the largest held key; 0 passes when nothing is counted.
 *   heads        a sorted item is a KEY head iff key != 0 and it is the first item or differs from its predecessor (tally_is_head); a ROW
 *                head iff key != 0 and it is the first item or key >> shift differs from its predecessor's.  Every row head is a key head.
 *   key table    one {key, count} per key head, keys ascending; count = the distance to the next key head, or to n.
 *   row table    (m >= 1) one {group = key >> shift, count, first, ndistinct} per row head, ascending: count = the distance to the next
 *                row head or to n, first = the rank of its first entry in the key table, ndistinct = the next row's first (or the key
 *                table's size) minus its own.
 *   dense cell   an entry with r = key >> shift and c = key & mask lies inside an nrows x ncols matrix iff 1 <= r <= nrows and
 *                1 <= c <= ncols; its cell is (r - 1) * ncols + (c - 1).  Demux keys (pattern + 1) and library ids are 1-based: that is
 *                what the matrix is for.  Raw sequence columns fall outside, and the sparse tables serve them.
 *
 *   k_tally_held_pack     one thread per held record, in the tiles of seeq_tiles.h: line[i], line[i - 1] (the predecessor of a tile's first
 *                         record lies in the tile before it: it is read from the array) and key[i]; the key or 0 AT THE RECORD'S OWN INDEX in
 *                         the tally's first key array; per tile the words of tally_tile_stat {keyless, repeat, 0, 0, 0, bits of the largest
 *                         counted key, sort flag, 0}.
 *   k_tally_held_top      one workgroup: the tiles' words -> the totals (tally_stat_top).
 *   the sort              seeq_tally.h's, of one-word items, unchanged (tally_sort_run).
 *   k_tally_held_rle_reduce / _top / _apply    per tile: key heads, row heads, nonzero items; one workgroup: the exclusive prefix of BOTH head
 *                         rows (tile_top once per row), the totals, the tiles' flags; the ordered compaction: key head j's index -> kpos[j],
 *                         and for a row head of rank r its key rank j -> rrank[r] (a row head is a key head: both ranks are known in the same
 *                         thread) -- 4 + 4 bytes per item in the key array the last pass left free.  A row head's index is kpos[rrank[r]].
 *   k_tally_held_table / k_tally_held_rows     one thread per entry: an entry is written by that one thread.
 *   k_tally_held_dense / _dense_top            one thread per key-table entry over an output the host zero-filled: distinct keys give distinct
 *                         cells, so a cell has one writer; the entries outside the matrix and their reads are summed per workgroup, and one
 *                         workgroup sums those.
 *
 * Every output slot is written by exactly one thread; no atomics on global memory, no workgroup waits on another, every loop is bounded by
 * a count the host knows, the grids come from host-known counts (no records: nothing is launched), every index is checked against its array.
 */
#ifndef SEEQ_TALLY_HELD_H_
#define SEEQ_TALLY_HELD_H_

#include <stdint.h>

#include "seeq_tally_append.h"                              /* SEEQ_TALLY_COLUMNS, SEEQ_TALLY_WORD_BITS; seeq_tally_group.h, seeq_tally.h */

#define SEEQ_HELD_REPEAT  0                                 /* what a held record is */
#define SEEQ_HELD_KEYLESS 1
#define SEEQ_HELD_COUNTED 2

/* does record i of line[0 .. n) open its line? */
SEEQ_ST_HD int tally_held_opens(const uint32_t *line, uint64_t i) { return i == 0u || line[i - 1] != line[i]; }

SEEQ_ST_HD int tally_held_kind(int opens, uint64_t key) { return !opens ? SEEQ_HELD_REPEAT : key ? SEEQ_HELD_COUNTED : SEEQ_HELD_KEYLESS; }

/* the word a record is sorted as: its key when it is counted, 0 otherwise */
SEEQ_ST_HD uint64_t tally_held_word(int kind, uint64_t key) { return kind == SEEQ_HELD_COUNTED ? key : 0u; }

/* *shift: the bits of the last m of ncolumns columns; -1: m outside [0, ncolumns), more than SEEQ_TALLY_COLUMNS columns, widths beyond 63 bits */
SEEQ_ST_HD int tally_held_shift(const uint32_t *widths, int ncolumns, int m, uint32_t *shift)
{
   if (ncolumns < 1 || ncolumns > SEEQ_TALLY_COLUMNS || m < 0 || m >= ncolumns) return -1;
   uint32_t total = 0;
   for (int c = ncolumns - m; c < ncolumns; c++) {
      if (widths[c] > SEEQ_TALLY_WORD_BITS - total) return -1;
      total += widths[c];
   }
   *shift = total;
   return 0;
}

/* the two parts of a key (shift <= 63) */
SEEQ_ST_HD uint64_t tally_held_row(uint64_t key, uint32_t shift) { return key >> shift; }
SEEQ_ST_HD uint64_t tally_held_col(uint64_t key, uint32_t shift) { return key & (((uint64_t)1 << shift) - 1u); }

/* passes of the sort: the key_bits bits of the largest held key in digits of 8; 0 when nothing is counted */
SEEQ_ST_HD uint32_t tally_held_passes(uint64_t ncounted, uint32_t key_bits) { return ncounted ? tally_group_passes(key_bits) : 0u; }

/* does a row begin at a sorted key?  (first: the key has no predecessor; a key head is tally_is_head) */
SEEQ_ST_HD int tally_held_is_row_head(uint64_t key, uint64_t prev, uint32_t shift, int first)
{
   return key != 0u && (first || tally_held_row(key, shift) != tally_held_row(prev, shift));
}

/* 1 and *cell: the key lies inside the nrows x ncols matrix; 0: it does not */
SEEQ_ST_HD int tally_held_cell(uint64_t key, uint32_t shift, uint32_t nrows, uint32_t ncols, uint64_t *cell)
{
   const uint64_t r = tally_held_row(key, shift), c = tally_held_col(key, shift);
   if (r < 1u || r > nrows || c < 1u || c > ncols) return 0;
   *cell = (r - 1u) * (uint64_t)ncols + (c - 1u);
   return 1;
}

#if defined(__HIPCC__)

struct TallyHeldCnt {
   uint32_t nkeyless, nrepeat;        /* held records that are not counted, by kind */
   uint32_t key_bits;                 /* bits of the largest counted key */
   uint32_t bad;                      /* 2: an index outside an array (an internal error) */
   uint32_t nkeys, nrows;             /* key heads, row heads of the sorted items */
   uint32_t nonzero;                  /* nonzero items: the counted records */
   uint32_t key_first, key_last;      /* index of the first / the last key head */
   uint32_t row_first, rank_first;    /* index of the first row head and its key rank: 0 */
   uint32_t noutside;                 /* the dense call: entries outside the matrix ... */
   uint64_t outside_reads;            /* ... and the sum of their counts */
};

struct TallyHeldArgs {
   const uint32_t *line;              /* [n] the held column: read only */
   const uint64_t *key;
   uint32_t        n;
   uint32_t        nt;                /* tiles = workgroups of the per-tile kernels */
   uint32_t        shift;             /* bits of the column part */
   uint64_t       *src;               /* [n] the words: the pack writes them, the sort leaves them here */
   uint32_t       *tstat;             /* [8 * nt] the tiles' words (tally_tile_stat) */
   uint32_t       *rsum;              /* [3 * nt] per tile key heads, row heads (k_tally_held_rle_top: exclusive prefixes), nonzero items */
   uint32_t        nk, nr;            /* entries of the two tables (nr == 0: no row table) */
   uint32_t       *kpos;              /* [nk] the key heads' indices */
   uint32_t       *rrank;             /* [nr] the row heads' key ranks */
   uint4          *tab;               /* the key table: seeqdev_tally_t */
   uint64_t       *rtab;              /* the row table: three words per entry */
   uint32_t        cap_tab, cap_rtab;
   uint64_t       *out;               /* the dense call: [nrows * ncols] */
   uint32_t        nrows, ncols;
   uint32_t       *dn;                /* [nd] per workgroup of the dense kernel: entries outside ... */
   uint64_t       *dr;                /* ... and their reads */
   uint32_t        nd;
   TallyHeldCnt   *cnt;
};

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_held_pack(TallyHeldArgs a)
{
   __shared__ uint32_t s_st[6][SEEQ_TILE_WAVES];
   uint32_t nkeyless = 0, nrepeat = 0;                      /* wave-uniform */
   uint32_t bits = 0;                                       /* this lane's */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      int kind = -1;
      if (i < a.n) {
         const uint64_t key = a.key[i];
         kind = tally_held_kind(tally_held_opens(a.line, i), key);
         const uint64_t w = tally_held_word(kind, key);
         a.src[i] = w;
         const uint32_t b = tally_key_bits(w);
         bits = b > bits ? b : bits;
      }
      nkeyless += (uint32_t)__popcll(__ballot(kind == SEEQ_HELD_KEYLESS));
      nrepeat += (uint32_t)__popcll(__ballot(kind == SEEQ_HELD_REPEAT));
   }
   tally_tile_stat(nkeyless, nrepeat, 0u, 0u, bits, 0u, s_st, a.tstat);
}

/* One workgroup: the tiles' words -> the totals. */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_held_top(TallyHeldArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES], s_st[3][SEEQ_TILE_WAVES];
   uint32_t t[6];
   tally_stat_top(a.tstat, a.nt, s_wave, s_st, t);
   if (threadIdx.x == 0) { a.cnt->nkeyless = t[0]; a.cnt->nrepeat = t[1]; a.cnt->bad = t[3]; a.cnt->key_bits = t[5]; }
}

/* the two head predicates of sorted item i < n (its predecessor is read from the array: it may lie in another tile) */
__device__ __forceinline__ void tally_held_heads(const TallyHeldArgs &a, uint64_t i, bool *khead, bool *rhead, bool *nonzero)
{
   const uint64_t key = a.src[i], prev = i ? a.src[i - 1] : 0u;
   *khead = tally_is_head(key, prev, i == 0);
   *rhead = tally_held_is_row_head(key, prev, a.shift, i == 0);
   *nonzero = key != 0u;
}

/* the run-length pass: the reduce / top / apply of seeq_tiles.h over the sorted words, two head predicates at once */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_held_rle_reduce(TallyHeldArgs a)
{
   __shared__ uint32_t s_sum[3][SEEQ_TILE_WAVES];
   uint32_t sum[3] = {0u, 0u, 0u};                          /* key heads, row heads, nonzero items: wave-uniform */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      bool khead = false, rhead = false, nonzero = false;
      if (i < a.n) tally_held_heads(a, i, &khead, &rhead, &nonzero);
      sum[0] += (uint32_t)__popcll(__ballot(khead));
      sum[1] += (uint32_t)__popcll(__ballot(rhead));
      sum[2] += (uint32_t)__popcll(__ballot(nonzero));
   }
   tile_sums(sum, s_sum, a.rsum, a.nt);
}

/* One workgroup: rows 0 and 1 of rsum -> their exclusive prefixes, in place (tile_top scans one row: once per row); the two head totals, the
   nonzero items, the tiles' flags since the pack. */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_held_rle_top(TallyHeldArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES], s_bad[SEEQ_TILE_WAVES];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   uint32_t tot[3], rtot[1], bad = 0;
   tile_top(a.rsum, a.nt, s_wave, tot);                     /* (rows 1 and 2 are read as the reduce left them ...) */
   tile_top(a.rsum + a.nt, a.nt, s_wave, rtot);             /* (... before row 1 is scanned: every entry by the thread that read it) */
   for (uint32_t i = threadIdx.x; i < a.nt; i += SEEQ_TILE_WG) bad |= a.tstat[(size_t)SEEQ_TALLY_STAT * i + SEEQ_TALLY_STAT_FLAG];
   bad = __ballot(bad != 0u) != 0ull ? 2u : 0u;
   if (lane == 0) s_bad[wave] = bad;
   __syncthreads();
   if (threadIdx.x == 0) {
      for (int w = 0; w < SEEQ_TILE_WAVES; w++) bad |= s_bad[w];
      if (rtot[0] != tot[1]) bad |= 2u;
      a.cnt->nkeys = tot[0]; a.cnt->nrows = tot[1]; a.cnt->nonzero = tot[2]; a.cnt->bad = bad;
   }
}

/* the ordered compaction of both kinds of head: a key head's index goes to its rank; a row head's key rank to its own rank */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_held_rle_apply(TallyHeldArgs a)
{
   __shared__ uint32_t s_kc[SEEQ_TILE_ITEMS][SEEQ_TILE_WAVES], s_rc[SEEQ_TILE_ITEMS][SEEQ_TILE_WAVES];
   bool khead[SEEQ_TILE_ITEMS], rhead[SEEQ_TILE_ITEMS];
   uint32_t kwithin[SEEQ_TILE_ITEMS], rwithin[SEEQ_TILE_ITEMS];
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      bool nonzero;
      khead[k] = rhead[k] = false;
      if (i < a.n) tally_held_heads(a, i, &khead[k], &rhead[k], &nonzero);
      kwithin[k] = tile_wave_rank(khead[k], s_kc[k]);
      rwithin[k] = tile_wave_rank(rhead[k], s_rc[k]);
   }
   __syncthreads();
   uint32_t krank0 = a.rsum[blockIdx.x], rrank0 = a.rsum[a.nt + blockIdx.x];      /* heads before this tile, then before this round */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint32_t j = tile_place(krank0, kwithin[k], s_kc[k]);
      const uint32_t r = tile_place(rrank0, rwithin[k], s_rc[k]);
      if (khead[k] && j < a.nk) a.kpos[j] = (uint32_t)tile_index(k);      /* (nk, nr are the sums of these very heads: k_tally_held_rle_top) */
      if (rhead[k] && r < a.nr) a.rrank[r] = j;                           /* (nr == 0 without a row table: nothing is stored) */
   }
}

/* One thread per entry of the key table; the first and the last key head's index go to the counters (the host checks them). */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_held_table(TallyHeldArgs a)
{
   const uint64_t j = (uint64_t)blockIdx.x * SEEQ_TILE_WG + threadIdx.x;
   if (j >= a.nk || j >= a.cap_tab) return;
   const uint32_t p = a.kpos[j];
   const uint32_t next = j + 1 < a.nk ? a.kpos[j + 1] : a.n;
   if (j == 0) a.cnt->key_first = p;
   if (j + 1 == a.nk) a.cnt->key_last = p;
   if (p >= a.n || next <= p || next > a.n) { a.tab[j] = make_uint4(0u, 0u, 0u, 0u); return; }
   const uint64_t key = a.src[p];
   const uint64_t count = (uint64_t)(next - p);
   a.tab[j] = make_uint4((uint32_t)key, (uint32_t)(key >> 32), (uint32_t)count, (uint32_t)(count >> 32));
}

/* One thread per entry of the row table; the first row head's index and key rank go to the counters. */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_held_rows(TallyHeldArgs a)
{
   const uint64_t r = (uint64_t)blockIdx.x * SEEQ_TILE_WG + threadIdx.x;
   if (r >= a.nr || r >= a.cap_rtab) return;
   const uint32_t first = a.rrank[r];
   const uint32_t nfirst = r + 1 < a.nr ? a.rrank[r + 1] : a.nk;
   uint64_t *e = a.rtab + 3 * r;
   if (first >= a.nk || nfirst <= first || nfirst > a.nk) {
      if (r == 0) { a.cnt->row_first = a.n; a.cnt->rank_first = first; }
      e[0] = 0u; e[1] = 0u; e[2] = 0u;
      return;
   }
   const uint32_t p = a.kpos[first];
   const uint32_t next = nfirst < a.nk ? a.kpos[nfirst] : a.n;
   if (r == 0) { a.cnt->row_first = p; a.cnt->rank_first = first; }
   if (p >= a.n || next <= p || next > a.n) { e[0] = 0u; e[1] = 0u; e[2] = 0u; return; }
   e[0] = tally_held_row(a.src[p], a.shift); e[1] = (uint64_t)(next - p); e[2] = (uint64_t)first | ((uint64_t)(nfirst - first) << 32);
}

/* One thread per entry of the key table: its count to its cell of the zero-filled matrix; per workgroup the entries outside and their reads. */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_held_dense(TallyHeldArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES];
   __shared__ uint64_t s_wave64[SEEQ_TILE_WAVES];
   const uint64_t j = (uint64_t)blockIdx.x * SEEQ_TILE_WG + threadIdx.x;
   uint32_t outside = 0u;
   uint64_t reads = 0u;
   if (j < a.nk && j < a.cap_tab) {
      const uint4 e = a.tab[j];
      const uint64_t key = (uint64_t)e.x | ((uint64_t)e.y << 32), count = (uint64_t)e.z | ((uint64_t)e.w << 32);
      uint64_t cell = 0u;
      if (tally_held_cell(key, a.shift, a.nrows, a.ncols, &cell) && cell < (uint64_t)a.nrows * a.ncols) a.out[cell] = count;
      else { outside = 1u; reads = count; }
   }
   uint32_t n;
   uint64_t r;
   block_excl_scan(outside, &n, s_wave);
   block_excl_scan(reads, &r, s_wave64);
   if (threadIdx.x == 0 && blockIdx.x < a.nd) { a.dn[blockIdx.x] = n; a.dr[blockIdx.x] = r; }
}

/* One workgroup: the dense kernel's per-workgroup numbers -> the totals. */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_held_dense_top(TallyHeldArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES];
   __shared__ uint64_t s_wave64[SEEQ_TILE_WAVES];
   uint32_t n = 0u, ntot;
   uint64_t r = 0u, rtot;
   for (uint32_t i = threadIdx.x; i < a.nd; i += SEEQ_TILE_WG) { n += a.dn[i]; r += a.dr[i]; }
   block_excl_scan(n, &ntot, s_wave);
   block_excl_scan(r, &rtot, s_wave64);
   if (threadIdx.x == 0) { a.cnt->noutside = ntot; a.cnt->outside_reads = rtot; }
}

#endif   /* __HIPCC__ */
#endif
