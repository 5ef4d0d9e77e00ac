/*
 * seeq_tally_group.h -- the grouped tally: how often each distinct (group, member) PAIR occurs, where every line carries two keys -- a
 * guide and its UMI, a sample and its guide.  One call HOLDS the keys of one record array (the group column), a later call pairs the
 * spans of another record array (the members) with them by line, sorts the pairs and run-length counts them -- all on the device.  The
 * pair table is a sparse matrix in row order (groups x members), the group table its row index.
 *
 * The rule -- plain C++ below, shared with the host driver (tests/tally_group_host_driver.cpp compiles this header with g++):
 *
 *   key          a span's key is seeq_tally.h's, unchanged (tally_span_kind / tally_key_of): long is decided before any byte is read,
 *                then foreign; a span with end < start or one that reaches beyond nbytes is bad (EIO) and no byte of it is loaded.
 *   held column  for record i of the held source, in record order: hold_line[i] (the record's line number) and hold_key[i] (0: no
 *                key -- the span is long or foreign, or, for demux records, the line is ambiguous).  Lines do not decrease.
 *                Demux records give the key pattern + 1 (1 .. 255).
 *   group        of a line (tally_group_of): j = the number of held records with a smaller line (a lower bound); the group is
 *                hold_key[j] if j < nh and hold_line[j] == line, else 0.  Of several held records on a line the FIRST decides.
 *   pair         a member span with key m != 0 on a line of group g != 0 is the pair (g, m); every other span is stored as (0, 0) and
 *                counted in exactly one of long, foreign (decided on the member, as in the plain tally) and ungrouped (the member has a
 *                key, the line has no held record or one without a key).
 *   order        by group, then by member, both as unsigned 64-bit numbers; (0, 0) sorts first, nothing is compacted before the sort.
 *   passes       the tally's stable LSD radix sort carrying both words: tally_passes(max_len) passes over the member word's digits
 *                (max_len: the largest PAIRED member length), then ceil(key_bits / 8) over the group word's (key_bits: the bit length
 *                of the largest held key); 0 when nothing paired.
 *   heads        a sorted item is a pair head iff g != 0 and it is the first item or (g, m) differs from its predecessor; a group head
 *                iff g != 0 and it is the first item or g differs from its predecessor's.  Every group head is a pair head.
 *   pair table   one {group, member, count} per pair head, in order; count = the distance to the next pair head, or to n.
 *   group table  one {group, count, first, ndistinct} per group head, in order: count = the distance to the next group head or to n (the
 *                group's reads), first = the rank of its first pair in the pair table, ndistinct = the next group's first (or npairs)
 *                minus its own.
 *
 *   k_tally_hold          one thread per held record, in the tiles of seeq_tiles.h: hold_line / hold_key AT THE RECORD'S OWN INDEX; span
 *                         bytes by tally_span_load; per tile the eight words of tally_tile_stat (seeq_tally.h) {long, foreign, largest L,
 *                         bad, ambiguous, largest key's bits, 0, 0}.
 *   k_tally_group_top     one workgroup: the tiles' words -> the totals (tally_stat_top; after the hold and after the pair pack alike).
 *   k_tally_pair_pack     one thread per member span: the member key by tally_span_load, the tally_group_of search (at most 32 probes),
 *                         g and m stored AT THE SPAN'S OWN INDEX in two key arrays; per tile {long, foreign, largest paired L, bad,
 *                         ungrouped, 0, 0, 0}.
 *   the sort              seeq_tally.h's, of two-word items: word 0 the member, word 1 the group; k_tally_pair_hist and
 *                         k_tally_pair_scatter are its two-word instantiations.
 *   k_tally_pair_rle_reduce / _top / _apply    per tile: pair heads, group heads, nonzero items; one workgroup: the exclusive prefix of
 *                         BOTH head rows (tile_top scans one row: it is called once per row), the totals, the tiles' flags; the ordered
 *                         compaction: pair head j's index -> ppos[j]; group head r's index -> gpos[r] and its pair rank -> grank[r]
 *                         (both known in the same thread: a group head is a pair head), in the key arrays the last pass left free.
 *   k_tally_pair_table / k_tally_group_table   one thread per entry: a 24-byte entry is written by that one thread.
 *
 * Every output slot is written by exactly one thread; no atomics on global memory at all (flags are per tile), no workgroup waits on
 * another, every loop is bounded by a count the host knows, the grids come from host-known counts (no spans: nothing is launched).
 */
#ifndef SEEQ_TALLY_GROUP_H_
#define SEEQ_TALLY_GROUP_H_

#include <stdint.h>

#include "seeq_tally.h"

#define SEEQ_TALLY_UNGROUPED 4                              /* beside SEEQ_TALLY_OK (paired) / _LONG / _FOREIGN / _BAD: what a member span is */
#define SEEQ_TALLY_PROBES    32                             /* steps of the lower-bound search over at most 2^32 - 1 held records */

/* the group of a line: the key of the first held record of that line, 0 when it has none */
SEEQ_ST_HD uint64_t tally_group_of(const uint32_t *hold_line, const uint64_t *hold_key, uint32_t nh, uint32_t line)
{
   uint32_t lo = 0, hi = nh;
   for (int it = 0; it < SEEQ_TALLY_PROBES && lo < hi; it++) {
      const uint32_t mid = lo + (hi - lo) / 2u;
      if (hold_line[mid] < line) lo = mid + 1u;
      else hi = mid;
   }
   return lo < nh && hold_line[lo] == line ? hold_key[lo] : 0u;
}

/* What a member span is, from what its own bytes made of it (tally_span_key's verdict) and its line's group: long, foreign and bad are
   decided on the member first; then a span whose line has no group is ungrouped. */
SEEQ_ST_HD int tally_pair_kind(int member_kind, uint64_t group)
{
   if (member_kind != SEEQ_TALLY_OK) return member_kind;
   return group ? SEEQ_TALLY_OK : SEEQ_TALLY_UNGROUPED;
}

/* the group a demux record holds, from its last word {dist : 16, pattern : 8, margin : 8}: pattern + 1, 0 for an ambiguous line (margin 0) */
SEEQ_ST_HD uint64_t tally_demux_group(uint32_t w) { return (w >> 24) ? (uint64_t)((w >> 16) & 255u) + 1u : 0u; }

/* the bit length of a key (0: no key) */
SEEQ_ST_HD uint32_t tally_key_bits(uint64_t key) { return key ? 64u - (uint32_t)__builtin_clzll(key) : 0u; }

/* passes over the group word: its key_bits bits in digits of 8 */
SEEQ_ST_HD uint32_t tally_group_passes(uint32_t key_bits) { return (key_bits + 7u) / 8u; }

/* passes of the pair sort: the member word's, then the group word's; 0 when nothing paired */
SEEQ_ST_HD uint32_t tally_pair_passes(uint64_t npaired, uint32_t max_len, uint32_t key_bits)
{
   return npaired ? tally_passes(max_len) + tally_group_passes(key_bits) : 0u;
}

/* the digit pass number `pass` of the pair sort sorts by, of mpasses member passes */
SEEQ_ST_HD uint32_t tally_pair_digit(uint64_t g, uint64_t m, uint32_t pass, uint32_t mpasses)
{
   return pass < mpasses ? tally_digit(m, pass) : tally_digit(g, pass - mpasses);
}

/* does a pair / a group begin at a sorted item?  (first: the item has no predecessor) */
SEEQ_ST_HD int tally_is_pair_head(uint64_t g, uint64_t m, uint64_t pg, uint64_t pm, int first) { return g != 0u && (first || g != pg || m != pm); }
SEEQ_ST_HD int tally_is_group_head(uint64_t g, uint64_t pg, int first) { return g != 0u && (first || g != pg); }

#if defined(__HIPCC__)

struct TallyGroupCnt {
   uint32_t nlong, nforeign;          /* spans without a key, by kind */
   uint32_t nthird;                   /* the hold: ambiguous demux records; the pair pack: ungrouped spans */
   uint32_t max_len;                  /* the largest length with a key (the pair pack: of a PAIRED member) */
   uint32_t bad;                      /* 1: a span outside the text; 2: an index outside an array (an internal error) */
   uint32_t key_bits;                 /* the hold: bits of the largest held key */
   uint32_t npairs, ngroups;          /* pair heads, group heads of the sorted items */
   uint32_t nonzero;                  /* items with a group: the paired spans */
   uint32_t pair_first, group_first;  /* index of the first pair head / group head: the items that are (0, 0) */
   uint32_t rank_first;               /* pair rank of the first group head: 0 */
};

struct TallyGroupArgs {
   const uint4    *rec;               /* [n] the records: the held source's, or the members' */
   const uint64_t *off;               /* [n] their line offsets (NULL: demux records, which need none) */
   uint32_t        n;
   uint32_t        nt;                /* tiles = workgroups of the per-tile kernels */
   const uint8_t  *text;
   uint64_t        nbytes;
   uint32_t        demux;             /* k_tally_hold: the records are seeqdev_demux_t */
   uint32_t       *hold_line;         /* [nh] the held column: k_tally_hold writes it, k_tally_pair_pack searches it */
   uint64_t       *hold_key;
   uint32_t        nh;
   uint64_t       *msrc, *gsrc;       /* [n] member words, group words: the pair pack writes them, the sort leaves them here */
   uint32_t       *tstat;             /* [8 * nt] the tiles' words (tally_tile_stat: the third count is ambiguous | ungrouped) */
   uint32_t       *rsum;              /* [3 * nt] per tile pair heads, group heads (k_tally_pair_rle_top: exclusive prefixes), nonzero items */
   uint32_t        np, ng;            /* entries of the two tables */
   uint32_t       *ppos;              /* [np] the pair heads' indices */
   uint32_t       *gpos, *grank;      /* [ng] the group heads' indices and pair ranks */
   uint64_t       *ptab, *gtab;       /* the tables: three words per entry */
   uint32_t        cap_ptab, cap_gtab;
   TallyGroupCnt  *cnt;
};

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_hold(TallyGroupArgs a)
{
   __shared__ uint32_t s_st[6][SEEQ_TILE_WAVES];
   uint32_t nlong = 0, nfor = 0, namb = 0;                  /* wave-uniform */
   uint32_t maxl = 0, bits = 0, bad = 0;                    /* this lane's */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      int kind = -1;
      bool amb = false;
      if (i < a.n) {
         const uint4 r = a.rec[i];
         uint64_t key = 0u;
         uint32_t len = 0u;
         if (a.demux) {
            key = tally_demux_group(r.w);
            amb = key == 0u;
            kind = SEEQ_TALLY_OK;
         } else {
            kind = tally_span_load(a.text, a.nbytes, a.off[i], r.y, r.z, &key, &len);
         }
         a.hold_line[i] = r.x;
         a.hold_key[i] = key;
         if (key) {
            maxl = len > maxl ? len : maxl;
            const uint32_t b = tally_key_bits(key);
            bits = b > bits ? b : bits;
         }
         if (kind == SEEQ_TALLY_BAD) bad = 1u;
      }
      nlong += (uint32_t)__popcll(__ballot(kind == SEEQ_TALLY_LONG));
      nfor += (uint32_t)__popcll(__ballot(kind == SEEQ_TALLY_FOREIGN));
      namb += (uint32_t)__popcll(__ballot(amb));
   }
   tally_tile_stat(nlong, nfor, namb, maxl, bits, bad, s_st, a.tstat);
}

/* One workgroup: the tiles' words -> the totals (after the hold and after the pair pack alike). */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_group_top(TallyGroupArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES], s_st[3][SEEQ_TILE_WAVES];
   uint32_t t[6];
   tally_stat_top(a.tstat, a.nt, s_wave, s_st, t);
   if (threadIdx.x == 0) {
      a.cnt->nlong = t[0]; a.cnt->nforeign = t[1]; a.cnt->max_len = t[2]; a.cnt->bad = t[3];
      a.cnt->nthird = t[4]; a.cnt->key_bits = t[5];
   }
}

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_pair_pack(TallyGroupArgs a)
{
   __shared__ uint32_t s_st[6][SEEQ_TILE_WAVES];
   uint32_t nlong = 0, nfor = 0, nung = 0;                  /* wave-uniform */
   uint32_t maxl = 0, bad = 0;                              /* this lane's */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      int kind = -1;
      if (i < a.n) {
         const uint4 r = a.rec[i];
         uint64_t m, g = 0u;
         uint32_t len;
         kind = tally_span_load(a.text, a.nbytes, a.off[i], r.y, r.z, &m, &len);
         if (kind == SEEQ_TALLY_OK) g = tally_group_of(a.hold_line, a.hold_key, a.nh, r.x);
         kind = tally_pair_kind(kind, g);
         const bool paired = kind == SEEQ_TALLY_OK;
         a.gsrc[i] = paired ? g : 0u;
         a.msrc[i] = paired ? m : 0u;
         if (paired && len > maxl) maxl = len;
         if (kind == SEEQ_TALLY_BAD) bad = 1u;
      }
      nlong += (uint32_t)__popcll(__ballot(kind == SEEQ_TALLY_LONG));
      nfor += (uint32_t)__popcll(__ballot(kind == SEEQ_TALLY_FOREIGN));
      nung += (uint32_t)__popcll(__ballot(kind == SEEQ_TALLY_UNGROUPED));
   }
   tally_tile_stat(nlong, nfor, nung, maxl, 0u, bad, s_st, a.tstat);
}

/* the two head predicates of sorted item i < n (its predecessor is read from the arrays: it may lie in another tile) */
__device__ __forceinline__ void tally_pair_heads(const TallyGroupArgs &a, uint64_t i, bool *phead, bool *ghead, bool *nonzero)
{
   const uint64_t g = a.gsrc[i], m = a.msrc[i];
   const uint64_t pg = i ? a.gsrc[i - 1] : 0u, pm = i ? a.msrc[i - 1] : 0u;
   *phead = tally_is_pair_head(g, m, pg, pm, i == 0);
   *ghead = tally_is_group_head(g, pg, i == 0);
   *nonzero = g != 0u;
}

/* the run-length pass: the reduce / top / apply of seeq_tiles.h over the sorted items, two head predicates at once */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_pair_rle_reduce(TallyGroupArgs a)
{
   __shared__ uint32_t s_sum[3][SEEQ_TILE_WAVES];
   uint32_t sum[3] = {0u, 0u, 0u};                          /* pair heads, group heads, nonzero items: wave-uniform */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      bool phead = false, ghead = false, nonzero = false;
      if (i < a.n) tally_pair_heads(a, i, &phead, &ghead, &nonzero);
      sum[0] += (uint32_t)__popcll(__ballot(phead));
      sum[1] += (uint32_t)__popcll(__ballot(ghead));
      sum[2] += (uint32_t)__popcll(__ballot(nonzero));
   }
   tile_sums(sum, s_sum, a.rsum, a.nt);
}

/* One workgroup: rows 0 and 1 of rsum -> their exclusive prefixes, in place (tile_top scans one row: once per row); npairs, ngroups, the
   nonzero items, the tiles' flags since the pack. */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_pair_rle_top(TallyGroupArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES], s_bad[SEEQ_TILE_WAVES];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   uint32_t tot[3], gtot[1], bad = 0;
   tile_top(a.rsum, a.nt, s_wave, tot);                     /* (rows 1 and 2 are read as the reduce left them ...) */
   tile_top(a.rsum + a.nt, a.nt, s_wave, gtot);             /* (... before row 1 is scanned: every entry by the thread that read it) */
   for (uint32_t i = threadIdx.x; i < a.nt; i += SEEQ_TILE_WG) bad |= a.tstat[(size_t)SEEQ_TALLY_STAT * i + SEEQ_TALLY_STAT_FLAG];
   bad = __ballot(bad != 0u) != 0ull ? 2u : 0u;
   if (lane == 0) s_bad[wave] = bad;
   __syncthreads();
   if (threadIdx.x == 0) {
      for (int w = 0; w < SEEQ_TILE_WAVES; w++) bad |= s_bad[w];
      if (gtot[0] != tot[1]) bad |= 2u;
      a.cnt->npairs = tot[0]; a.cnt->ngroups = tot[1]; a.cnt->nonzero = tot[2]; a.cnt->bad = bad;
   }
}

/* the ordered compaction of both kinds of head: a head's index goes to its rank; a group head's pair rank beside it */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_pair_rle_apply(TallyGroupArgs a)
{
   __shared__ uint32_t s_pc[SEEQ_TILE_ITEMS][SEEQ_TILE_WAVES], s_gc[SEEQ_TILE_ITEMS][SEEQ_TILE_WAVES];
   bool phead[SEEQ_TILE_ITEMS], ghead[SEEQ_TILE_ITEMS];
   uint32_t pwithin[SEEQ_TILE_ITEMS], gwithin[SEEQ_TILE_ITEMS];
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      bool nonzero;
      phead[k] = ghead[k] = false;
      if (i < a.n) tally_pair_heads(a, i, &phead[k], &ghead[k], &nonzero);
      pwithin[k] = tile_wave_rank(phead[k], s_pc[k]);
      gwithin[k] = tile_wave_rank(ghead[k], s_gc[k]);
   }
   __syncthreads();
   uint32_t prank0 = a.rsum[blockIdx.x], grank0 = a.rsum[a.nt + blockIdx.x];      /* heads before this tile, then before this round */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint32_t j = tile_place(prank0, pwithin[k], s_pc[k]);
      const uint32_t r = tile_place(grank0, gwithin[k], s_gc[k]);
      if (phead[k] && j < a.np) a.ppos[j] = (uint32_t)tile_index(k);      /* (np, ng are the sums of these very heads: k_tally_pair_rle_top) */
      if (ghead[k] && r < a.ng) { a.gpos[r] = (uint32_t)tile_index(k); a.grank[r] = j; }
   }
}

/* One thread per entry of the pair table; the first pair head's index goes to the counters (the host checks it against the paired spans). */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_pair_table(TallyGroupArgs a)
{
   const uint64_t j = (uint64_t)blockIdx.x * SEEQ_TILE_WG + threadIdx.x;
   if (j >= a.np || j >= a.cap_ptab) return;
   const uint32_t p = a.ppos[j];
   const uint32_t next = j + 1 < a.np ? a.ppos[j + 1] : a.n;
   if (j == 0) a.cnt->pair_first = p;
   uint64_t *e = a.ptab + 3 * j;
   if (p >= a.n || next <= p || next > a.n) { e[0] = 0u; e[1] = 0u; e[2] = 0u; return; }
   e[0] = a.gsrc[p]; e[1] = a.msrc[p]; e[2] = (uint64_t)(next - p);
}

/* One thread per entry of the group table; the first group head's index and pair rank go to the counters. */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_group_table(TallyGroupArgs a)
{
   const uint64_t r = (uint64_t)blockIdx.x * SEEQ_TILE_WG + threadIdx.x;
   if (r >= a.ng || r >= a.cap_gtab) return;
   const uint32_t p = a.gpos[r], first = a.grank[r];
   const uint32_t next = r + 1 < a.ng ? a.gpos[r + 1] : a.n;
   const uint32_t nfirst = r + 1 < a.ng ? a.grank[r + 1] : a.np;
   if (r == 0) { a.cnt->group_first = p; a.cnt->rank_first = first; }
   uint64_t *e = a.gtab + 3 * r;
   if (p >= a.n || next <= p || next > a.n || nfirst <= first || nfirst > a.np) { e[0] = 0u; e[1] = 0u; e[2] = 0u; return; }
   e[0] = a.gsrc[p]; e[1] = (uint64_t)(next - p); e[2] = (uint64_t)first | ((uint64_t)(nfirst - first) << 32);
}

#endif   /* __HIPCC__ */
#endif
