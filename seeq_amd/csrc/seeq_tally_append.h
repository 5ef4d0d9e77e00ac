/*
 * seeq_tally_append.h -- key columns appended to the held column: the grouped tally's group word composed of SEVERAL keys per line -- a cell
 * barcode and a guide, a sample, a whitelist id and a guide -- on the device.  The grouped tally, its collapse, the quality gate and the
 * library all work on one 64-bit group word (seeq_tally_group.h); an append rewrites that word in place, so they apply to reads of three
 * and more keys unchanged.
 *
 * The rule -- plain C++ below, shared with the host driver (tests/tally_append_host_driver.cpp compiles this header with g++):
 *
 *   held column  H: hold_line[i], hold_key[i], i < nh, of key_bits B (a completed hold, or an earlier append).
 *   new column   N: col_line[j], col_key[j], j < nc, built from its source exactly as a hold builds its column (k_tally_hold; under a
 *                library the assignment behind it); its WIDTH w is the bit length of its largest key (0: no record has a key), for a
 *                library column bitlen(library entries).
 *   join         for every held record i (tally_append_of): k = tally_group_of(col_line, col_key, nc, hold_line[i]) -- the FIRST record
 *                of N on that line decides, 0 when the line has none or that record has no key --, and
 *                hold_key[i] = hold_key[i] != 0 && k != 0 ? (hold_key[i] << w) | k : 0.  Lines, record count and record order stay.
 *   dropped      a held record that had a key and has none afterwards: nbefore = nheld + ndropped.
 *   key_bits     afterwards the bit length of the largest composed key, COMPUTED (at most B + w, 0 when nothing is left): what the
 *                grouped call takes its group passes from.
 *   overflow     B + w > 63: the append is refused before H is touched (bit 63 stays clear in every group word, as in every key).
 *   injective    k < 2^w, so the shift loses nothing and the low w bits are k: (h, k) -> (h << w) | k is one-to-one, and by induction so
 *                is the word over all its columns (tally_split takes it apart again, from the widths the context keeps).
 *   column-major the word orders as the tuple of its columns: column 0 is most significant, then column 1, and so on -- h1 < h2 gives
 *                (h1 << w) | k1 < (h2 << w) | k2 whatever k1, k2 < 2^w are.  The group table's order is that order.
 *   columns      at most SEEQ_TALLY_COLUMNS; column 0's width is the hold's key_bits at the time of the hold.
 *
 *   k_tally_hold_join     one thread per HELD record, in the tiles of seeq_tiles.h: its line and key; for a nonzero key the at most 32
 *                         probes of tally_group_of over N; the composed key AT THE RECORD'S OWN INDEX; per tile the eight words of
 *                         tally_tile_stat (seeq_tally.h) {0, 0, 0, bad, dropped, largest composed key's bits, 0, 0} -- bad: a key wider
 *                         than its column (an internal error) --, which k_tally_group_top (seeq_tally_group.h) reduces to the totals.
 *
 * Every output slot is written by exactly one thread (a thread reads hold_key[i] and writes hold_key[i], nobody else touches it; N is only
 * read); no atomics on global memory, no workgroup waits on another, every loop is bounded by a count the host knows, nothing is launched
 * for zero held records.
 */
#ifndef SEEQ_TALLY_APPEND_H_
#define SEEQ_TALLY_APPEND_H_

#include <stdint.h>

#include "seeq_tally_group.h"

#define SEEQ_TALLY_COLUMNS   8                              /* columns of a held key, the hold's own included */
#define SEEQ_TALLY_WORD_BITS 63                             /* bits of a group word: the columns' widths sum to at most this */

/* may a column of w bits follow key_bits bits? */
SEEQ_ST_HD int tally_append_fits(uint32_t key_bits, uint32_t w) { return key_bits <= SEEQ_TALLY_WORD_BITS && w <= SEEQ_TALLY_WORD_BITS - key_bits; }

/* the composed key of a held key and its line's key of the new column, w bits wide (0 < w <= 63 wherever k != 0) */
SEEQ_ST_HD uint64_t tally_append_key(uint64_t held, uint64_t k, uint32_t w) { return held != 0u && k != 0u ? (held << w) | k : 0u; }

/* the join of one held record: its new key */
SEEQ_ST_HD uint64_t tally_append_of(const uint32_t *col_line, const uint64_t *col_key, uint32_t nc, uint32_t w, uint32_t line, uint64_t held)
{
   return held ? tally_append_key(held, tally_group_of(col_line, col_key, nc, line), w) : 0u;
}

/* A composed key -> out[c], c < ncolumns, the keys of its columns (column 0 first); -1: no columns or more than SEEQ_TALLY_COLUMNS, widths that
   sum to more than 63, or a key with bits above them. */
SEEQ_ST_HD int tally_split(uint64_t key, const uint32_t *widths, int ncolumns, uint64_t *out)
{
   if (ncolumns < 1 || ncolumns > SEEQ_TALLY_COLUMNS) return -1;
   uint32_t total = 0;
   for (int c = 0; c < ncolumns; c++) {
      if (widths[c] > SEEQ_TALLY_WORD_BITS - total) return -1;
      total += widths[c];
   }
   if (key >> total) return -1;
   for (int c = ncolumns - 1; c >= 0; c--) {
      out[c] = key & (((uint64_t)1 << widths[c]) - 1u);
      key >>= widths[c];
   }
   return 0;
}

#if defined(__HIPCC__)

struct TallyAppendArgs {
   uint32_t       *hold_line;         /* [nh] the held column: its keys are rewritten in place */
   uint64_t       *hold_key;
   uint32_t        nh;
   uint32_t        nt;                /* tiles of the held records = workgroups */
   const uint32_t *col_line;          /* [nc] the new column (nc == 0: never read) */
   const uint64_t *col_key;
   uint32_t        nc;
   uint32_t        key_bits, width;   /* B and w: B + w <= 63 */
   uint32_t       *tstat;             /* [8 * nt] the tiles' words (tally_tile_stat: the third count is dropped) */
};

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_hold_join(TallyAppendArgs a)
{
   __shared__ uint32_t s_st[6][SEEQ_TILE_WAVES];
   uint32_t ndrop = 0;                                      /* wave-uniform */
   uint32_t bits = 0, bad = 0;                              /* this lane's */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      bool drop = false;
      if (i < a.nh) {
         const uint64_t held = a.hold_key[i];
         uint64_t key = 0u;
         if (held) {
            const uint64_t c = tally_group_of(a.col_line, a.col_key, a.nc, a.hold_line[i]);
            if (tally_key_bits(held) > a.key_bits || tally_key_bits(c) > a.width) bad = 1u;
            else key = tally_append_key(held, c, a.width);
            drop = key == 0u;
         }
         a.hold_key[i] = key;
         const uint32_t b = tally_key_bits(key);
         bits = b > bits ? b : bits;
      }
      ndrop += (uint32_t)__popcll(__ballot(drop));
   }
   tally_tile_stat(0u, 0u, ndrop, 0u, bits, bad, s_st, a.tstat);
}

#endif   /* __HIPCC__ */
#endif
