/*
 * seeq_insert.h -- the insert between two flanking patterns: the records of a scan with a LEFT flank (SQ_BEST or SQ_FIRST: one record per
 * matching line) joined, line by line, with the records of a scan of the same text with a RIGHT flank (SQ_ALL: every occurrence), and the
 * bytes between the two cut out of the text -- all on the device, on the 16-byte records behind the scans.
 *
 * The rule -- plain C++ below, shared with the host driver (tests/insert_host_driver.cpp compiles this header with g++):
 *
 *   left record          of a line: the one record of the left scan (x line, y start, z end, w dist).
 *   admissible           a right record R of the same line with R.start >= L.end + min_len and, when max_len != 0,
 *                        R.start <= L.end + max_len; both sums in 64 bits (max_len == 0: no upper bound).
 *   chosen               SQ_BEST: the admissible record of smallest dist, the smaller end on a tie; SQ_FIRST: the one of smallest end.
 *   insert record        {line, start = L.end, end = R.start (exclusive), ldist, rdist}: 16 bytes, `line` first like every record here;
 *                        a line without an admissible right record gives none.
 *   where a walk starts  an admissible record has end > start >= L.end + min_len, so the first candidate is the count of right records
 *                        whose key line << 32 | end is <= line << 32 | sat32(L.end + min_len): strand_count_below (seeq_strand.h).
 *   where it stops       at another line number, or at a start beyond the upper bound: within a line the starts of SQ_ALL records do
 *                        not decrease, the ends increase -- so under SQ_BEST the first record of the smallest dist has the smaller end.
 *   insert text          every insert's bytes followed by '\n', in record order: record k's bytes begin at pos[k], the exclusive
 *                        prefix of end - start + 1.  Output byte b belongs to the last record whose pos is <= b (positions increase
 *                        strictly: an empty insert still has its newline).
 *
 *   k_insert_join     one thread per left record, in the tiles of seeq_tiles.h: the search and the walk, one 16-byte store of the insert
 *                     record AT THE LEFT RECORD'S OWN INDEX; line number 0 (free: lines are 1-based) when nothing is admissible, and
 *                     then `start` tells whether the line has a right record at all.
 *   and over the joined array the reduce / top / apply of seeq_tiles.h:
 *   k_insert_reduce   per tile: records kept (line != 0), lines with both flanks; the kept records' text bytes (64 bits, a sum of its own).
 *   k_insert_top      one workgroup: exclusive scans of the tiles' kept counts (32 bits) and text bytes (64 bits) in place; the totals.
 *   k_insert_apply    the ordered compaction that drops line 0: record, line offset, and the record's byte position in the insert
 *                     text (the exclusive prefix of the text bytes, carried with the ranks).
 *   k_insert_text     the gather, balanced by OUTPUT BYTES: a thread owns SEEQ_INSERT_RUN consecutive output bytes, finds the record of
 *                     its first byte by one binary search over the positions and walks forward; one aligned 16-byte store where the
 *                     output buffer allows.  It checks offset + end <= nbytes against the text it was given (`bad` otherwise).
 *                     Why 16: one 16-byte store per lane is the widest the hardware has (a wave writes 1 KiB of consecutive bytes), and
 *                     with inserts of about that size (a barcode, a UMI, a guide) a run crosses one or two records, so the search is
 *                     paid once per 16 bytes and no lane serialises a long insert.  8 or 32 bytes per thread are not measured.
 *
 * Every output slot is written by exactly one thread; no atomics on outputs, no workgroup waits on another; the grids come from the
 * host-known counts (none: nothing is launched).  Lines with a right record (nright) are the right scan's own nmatchlines: no launch.
 */
#ifndef SEEQ_INSERT_H_
#define SEEQ_INSERT_H_

#include <stdint.h>

#include "seeq_strand.h"                                    /* strand_rec_t, strand_key, strand_count_below, strand_partner */

#define SEEQ_INSERT_WG    SEEQ_TILE_WG                      /* (the host driver prints the shape under the join's names) */
#define SEEQ_INSERT_ITEMS SEEQ_TILE_ITEMS
#define SEEQ_INSERT_TILE  SEEQ_TILE
#define SEEQ_INSERT_RUN   16                               /* output bytes per thread of k_insert_text */

#define SEEQ_INSERT_FIRST 0                                 /* = SQ_FIRST, SQ_BEST (libseeq.h) */
#define SEEQ_INSERT_BEST  1

SEEQ_ST_HD uint32_t insert_sat32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

/* index of the first right record that can be admissible for a left record of `line` that ends at lend */
SEEQ_ST_HD uint32_t insert_first_candidate(const strand_rec_t *right, uint32_t nr, uint32_t line, uint32_t lend, uint32_t min_len)
{
   return strand_count_below(right, nr, strand_key(line, insert_sat32((uint64_t)lend + min_len)), 1);
}

/* does `line` have a right record?  The record at the co-rank of line << 32, or the one before it, carries the number then. */
SEEQ_ST_HD int insert_line_has_right(const strand_rec_t *right, uint32_t nr, uint32_t line)
{
   return strand_partner(right, nr, strand_count_below(right, nr, strand_key(line, 0u), 0), line) < nr;
}

/* the two distances of an insert record in its fourth word: ldist in the low half, rdist in the high one (seeqdev_insert_t) */
SEEQ_ST_HD uint32_t insert_dists(uint32_t ldist, uint32_t rdist) { return (ldist & 0xFFFFu) | (rdist << 16); }

/* The insert record of left record l; x = 0: the line has none, and y tells whether it has a right record (1) or not (0). */
SEEQ_ST_HD strand_rec_t insert_join_one(int mode, strand_rec_t l, const strand_rec_t *right, uint32_t nr, uint32_t min_len, uint32_t max_len)
{
   const uint64_t lo = (uint64_t)l.z + min_len, hi = (uint64_t)l.z + max_len;
   strand_rec_t out;
   out.x = 0u; out.y = 0u; out.z = 0u; out.w = 0u;
   uint32_t best = 0xFFFFFFFFu;
   for (uint32_t i = insert_first_candidate(right, nr, l.x, l.z, min_len); i < nr && right[i].x == l.x; i++) {
      const strand_rec_t r = right[i];
      if (max_len != 0u && (uint64_t)r.y > hi) break;       /* starts do not decrease: nothing further on is admissible */
      if ((uint64_t)r.y < lo || r.w >= best) continue;      /* (ends increase: an equal dist further on has the larger end) */
      best = r.w;
      out.x = l.x; out.y = l.z; out.z = r.y; out.w = insert_dists(l.w, r.w);
      if (mode == SEEQ_INSERT_FIRST) break;
   }
   if (out.x == 0u) out.y = insert_line_has_right(right, nr, l.x) ? 1u : 0u;
   return out;
}

/* bytes of a record in the insert text: the insert and its newline */
SEEQ_ST_HD uint64_t insert_text_len(strand_rec_t r) { return (uint64_t)(r.z - r.y) + 1u; }

/* the record output byte b belongs to: the last k with pos[k] <= b (pos[0] = 0); n when there is none */
SEEQ_ST_HD uint32_t insert_text_record(const uint64_t *pos, uint32_t n, uint64_t b)
{
   uint32_t lo = 0, hi = n;
   while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (pos[mid] <= b) lo = mid + 1;
      else hi = mid;
   }
   return lo ? lo - 1 : n;
}

/* Output bytes [b0, b0 + cnt), cnt <= SEEQ_INSERT_RUN, of the insert text into w (little-endian, byte i in word i / 4; the rest 0).
   != 0: a record outside the text [0, nbytes), or no record for a byte -- those bytes are 0. */
SEEQ_ST_HD int insert_text_fill(const strand_rec_t *rec, const uint64_t *off, const uint64_t *pos, uint32_t n, const uint8_t *text, uint64_t nbytes,
                                uint64_t b0, int cnt, uint32_t w[SEEQ_INSERT_RUN / 4])
{
   for (int i = 0; i < SEEQ_INSERT_RUN / 4; i++) w[i] = 0u;
   uint32_t k = insert_text_record(pos, n, b0);
   if (k >= n) return 1;
   int bad = 0;
   strand_rec_t r = rec[k];
   uint64_t o = off[k], within = b0 - pos[k];
   uint64_t len = r.z >= r.y ? (uint64_t)(r.z - r.y) : 0u;
   int ok = r.z >= r.y && o <= nbytes && (uint64_t)r.z <= nbytes - o;
#if defined(__HIPCC__)
#pragma unroll
#endif
   for (int i = 0; i < SEEQ_INSERT_RUN; i++) {
      if (i >= cnt) continue;
      uint32_t c = 0u;
      if (within < len) {
         if (ok) c = text[o + r.y + within];
         else bad = 1;
         within++;
      } else {
         c = (uint32_t)'\n';
         if (k >= n) { bad = 1; c = 0u; }
         k++;
         within = 0;
         len = 0;
         ok = 0;
         if (k < n) {
            r = rec[k];
            o = off[k];
            len = r.z >= r.y ? (uint64_t)(r.z - r.y) : 0u;
            ok = r.z >= r.y && o <= nbytes && (uint64_t)r.z <= nbytes - o;
            if (!ok) bad = 1;
         }
      }
      w[i >> 2] |= c << (8 * (i & 3));
   }
   return bad;
}

#if defined(__HIPCC__)

static_assert(SEEQ_INSERT_RUN == 16, "k_insert_text stores a run as one uint4");

struct InsertCnt {
   uint64_t bytes;                    /* the insert text: sum over the kept records of end - start + 1 */
   uint32_t kept;                     /* joined records with a line number: the result's records */
   uint32_t both;                     /* left records whose line has a right record */
   uint32_t bad;                      /* an index outside an array, a record outside the text (an internal error) */
   uint32_t pad;
};

struct InsertArgs {
   const uint4    *left;              /* [nl] the left scan's records, in line order */
   const uint64_t *left_off;          /* [nl] their line offsets */
   const uint4    *right;             /* [nr] the right scan's records (SQ_ALL), in key order */
   uint32_t        nl, nr;
   uint32_t        min_len, max_len;
   int             mode;              /* SEEQ_INSERT_FIRST / BEST */
   uint4          *jn;                /* [cap_jn] joined records (k_insert_join writes, reduce / apply read) */
   uint32_t        cap_jn;
   uint32_t        nt;                /* tiles = workgroups */
   uint32_t       *bsum;              /* [2 * nt]: per tile kept (k_insert_top: exclusive prefix), both */
   uint64_t       *bbytes;            /* [nt]: per tile text bytes (k_insert_top: exclusive prefix) */
   uint4          *out;               /* [cap_out] k_insert_apply: the kept records, */
   uint64_t       *off_out;           /*           their line offsets, */
   uint64_t       *pos_out;           /*           their byte positions in the insert text */
   uint32_t        cap_out;
   InsertCnt      *cnt;
};

struct InsertTextArgs {
   const uint4    *rec;               /* [n] insert records */
   const uint64_t *off, *pos;         /* [n] line offsets in the text, byte positions in the output */
   uint32_t        n;
   uint64_t        total;             /* bytes of the output */
   const uint8_t  *text;
   uint64_t        nbytes;
   uint8_t        *out;
   InsertCnt      *cnt;
};

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_insert_join(InsertArgs a)
{
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t t = tile_index(k);
      if (t >= a.nl) continue;
      const uint4 r = insert_join_one(a.mode, a.left[t], a.right, a.nr, a.min_len, a.max_len);
      if (t < a.cap_jn) a.jn[t] = r;
      else atomicOr(&a.cnt->bad, 1u);
   }
}

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_insert_reduce(InsertArgs a)
{
   __shared__ uint32_t s_sum[2][SEEQ_TILE_WAVES];
   __shared__ uint64_t s_bytes[SEEQ_TILE_WAVES];
   uint32_t sum[2] = {0u, 0u};                              /* kept, both: wave-uniform */
   uint64_t bytes = 0;                                      /* this lane's */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      uint4 r = make_uint4(0u, 0u, 0u, 0u);
      if (i < a.nl) r = a.jn[i];
      const bool keep = r.x != 0u;
      sum[0] += (uint32_t)__popcll(__ballot(keep));
      sum[1] += (uint32_t)__popcll(__ballot(keep || r.y != 0u));    /* (no record: y is the line's "has a right record") */
      if (keep) bytes += insert_text_len(r);
   }
   bytes = wave_incl_scan_u64(bytes);                       /* the publishing lane, the last one: the wave's sum */
   if (tile_publishes()) s_bytes[threadIdx.x >> 6] = bytes;
   tile_sums(sum, s_sum, a.bsum, a.nt);                     /* (its barrier is s_bytes' too) */
   if (threadIdx.x == 0) {
      bytes = 0;
      for (int w = 0; w < SEEQ_TILE_WAVES; w++) bytes += s_bytes[w];
      a.bbytes[blockIdx.x] = bytes;
   }
}

/* One workgroup: bsum[0 .. nt) and bbytes[0 .. nt) -> their exclusive prefixes, in place; the totals (kept, both: at most nl). */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_insert_top(InsertArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES];
   __shared__ uint64_t s_wave64[SEEQ_TILE_WAVES];
   uint32_t tot[2];
   uint64_t tot_bytes[1];
   tile_top(a.bsum, a.nt, s_wave, tot);
   tile_top(a.bbytes, a.nt, s_wave64, tot_bytes);
   if (threadIdx.x == 0) { a.cnt->kept = tot[0]; a.cnt->both = tot[1]; a.cnt->bytes = tot_bytes[0]; }
}

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_insert_apply(InsertArgs a)
{
   __shared__ uint32_t s_cnt[SEEQ_TILE_ITEMS][SEEQ_TILE_WAVES];
   __shared__ uint64_t s_bytes[SEEQ_TILE_ITEMS][SEEQ_TILE_WAVES];
   uint4 r[SEEQ_TILE_ITEMS];
   uint64_t off[SEEQ_TILE_ITEMS];
   uint32_t within[SEEQ_TILE_ITEMS];                        /* kept records of the wave's round before this lane */
   uint64_t bytes_within[SEEQ_TILE_ITEMS];                  /* their text bytes */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      r[k] = make_uint4(0u, 0u, 0u, 0u);
      off[k] = 0;
      if (i < a.nl) {
         r[k] = a.jn[i];
         if (r[k].x != 0u) off[k] = a.left_off[i];
      }
      const bool keep = r[k].x != 0u;
      bytes_within[k] = tile_wave_offset(keep ? insert_text_len(r[k]) : 0u, s_bytes[k]);
      within[k] = tile_wave_rank(keep, s_cnt[k]);           /* (behind the scan: 64 VGPRs, two fewer than before it, and 66 are a wave less per SIMD) */
   }
   __syncthreads();
   uint32_t rank0 = a.bsum[blockIdx.x];                     /* kept records before this tile, then before this round */
   uint64_t byte0 = a.bbytes[blockIdx.x];                   /* their text bytes */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint32_t j = tile_place(rank0, within[k], s_cnt[k]);
      const uint64_t pos = tile_place(byte0, bytes_within[k], s_bytes[k]);
      if (r[k].x == 0u) continue;
      if (j < a.cap_out) {
         a.out[j] = r[k];
         a.off_out[j] = off[k];
         a.pos_out[j] = pos;
      } else {
         atomicOr(&a.cnt->bad, 1u);
      }
   }
}

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_insert_text(InsertTextArgs a)
{
   const uint64_t b0 = ((uint64_t)blockIdx.x * SEEQ_TILE_WG + threadIdx.x) * SEEQ_INSERT_RUN;
   if (b0 >= a.total) return;
   const int cnt = a.total - b0 < SEEQ_INSERT_RUN ? (int)(a.total - b0) : SEEQ_INSERT_RUN;
   uint32_t w[SEEQ_INSERT_RUN / 4];
   if (insert_text_fill(a.rec, a.off, a.pos, a.n, a.text, a.nbytes, b0, cnt, w)) atomicOr(&a.cnt->bad, 1u);
   if (cnt == SEEQ_INSERT_RUN && ((uintptr_t)a.out & 15u) == 0u) {
      *(uint4 *)(a.out + b0) = make_uint4(w[0], w[1], w[2], w[3]);
   } else {
#pragma unroll
      for (int i = 0; i < SEEQ_INSERT_RUN; i++)
         if (i < cnt) a.out[b0 + i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
   }
}

#endif   /* __HIPCC__ */
#endif
