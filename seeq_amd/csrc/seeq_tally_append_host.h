/*
 * seeq_tally_append_host.h -- the host driver of the appended key columns (rule and kernel: seeq_tally_append.h): the new column built by
 * the hold's own driver in arrays of its own (tally_hold_run with another target; under a library the assignment behind it), the width
 * check, the join into the held column, and the seeqdevScanTallyHoldAppend / seeqdevScanTallyHoldAppendLibrary /
 * seeqdevScanTallyHoldColumns / seeqdevScanCopyHeld / seeqdevTallySplit entries.  Included by seeq_device.hip behind
 * seeq_tally_library_host.h.
 */
#ifndef SEEQ_TALLY_APPEND_HOST_H_
#define SEEQ_TALLY_APPEND_HOST_H_

static TallyHoldTarget tally_append_target(seeqdev_scan *s) { return {s->ta_line, s->ta_key, s->ta_stat, s->cap_ta}; }

/* what an append lacks on this context, in the order it is looked for (NULL: nothing) */
static const char *tally_append_missing(const seeqdev_scan *s, bool library)
{
   if (!s) return NULL;
   if (library && !s->lb_n) return tally_library_missing(s);
   if (!s->th_done) return "tally append: the context holds no held column (seeqdevScanTallyHold)";
   if (s->th_ncol >= SEEQ_TALLY_COLUMNS) return "tally append: the held key has 8 columns already";
   return NULL;
}

static int tally_append_fail(const char *what, const TallyGroupCnt &h, size_t nh, uint64_t nbefore, uint32_t key_bits, uint32_t width)
{
   snprintf(g_last_error, sizeof g_last_error,
            "internal inconsistency in the tally append (%s: flags %u, %zu held records, %llu with a key, %u dropped, %u + %u bits before, %u after)",
            what, h.bad, nh, (unsigned long long)nbefore, h.nthird, key_bits, width, h.key_bits);
   errno = EIO;
   return -1;
}

/* The new column (ta_line / ta_key: nc records, `width` bits) joined into the held column; *counts is filled.  A failure leaves no column.  Waits. */
static int tally_append_join(seeqdev_scan *s, uint32_t nc, uint32_t width, seeqdev_tally_append_counts_t *counts)
{
   const hipStream_t st = s->stream;
   const uint32_t key_bits = s->th_key_bits;
   const uint64_t nbefore = s->th_nkeyed;
   const size_t nh = s->th_n;
   s->th_done = false;                                     /* (the keys are rewritten in place: a failure from here on leaves no column) */
   TallyGroupCnt h = {};
   if (nh) {                                               /* no held record: nothing is launched */
      if (tally_group_ws_cnt(s)) return -1;
      TallyAppendArgs a;
      memset(&a, 0, sizeof a);
      a.hold_line = s->th_line; a.hold_key = s->th_key; a.nh = (uint32_t)nh;
      a.nt = (uint32_t)tally_tiles(nh);
      a.col_line = s->ta_line; a.col_key = s->ta_key; a.nc = nc;
      a.key_bits = key_bits; a.width = width;
      a.tstat = s->th_stat;
      TallyGroupArgs top;                                  /* (k_tally_group_top reads the tiles' words and writes the totals, nothing else) */
      memset(&top, 0, sizeof top);
      top.nt = a.nt; top.tstat = a.tstat; top.cnt = s->d_tgcnt;
      if (nh > s->cap_th || nh > 0xFFFFFFFFull || tally_tiles(s->cap_th) < a.nt || (size_t)nc > s->cap_ta || !tally_append_fits(key_bits, width)) {
         snprintf(g_last_error, sizeof g_last_error, "tally append: %zu held records, arrays for %zu; %u appended, arrays for %zu; %u + %u bits", nh, s->cap_th, nc,
                  s->cap_ta, key_bits, width);
         errno = EIO;
         return -1;
      }
      HIP_TRY(hipMemsetAsync(s->d_tgcnt, 0, sizeof(TallyGroupCnt), st), EIO);
      hipLaunchKernelGGL(k_tally_hold_join, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
      hipLaunchKernelGGL(k_tally_group_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, top);
      if (counters_fetch(s, s->h_tgcnt, s->d_tgcnt, sizeof(TallyGroupCnt))) return -1;
      h = *s->h_tgcnt;
      if (h.bad) return tally_append_fail("a key wider than its column", h, nh, nbefore, key_bits, width);
      if (h.nthird > nbefore || h.key_bits > key_bits + width || (h.key_bits > 0u) != (nbefore - h.nthird > 0u))
         return tally_append_fail("join", h, nh, nbefore, key_bits, width);
   } else if (nbefore) {
      return tally_append_fail("no records", h, nh, nbefore, key_bits, width);
   }
   s->th_key_bits = h.key_bits;
   s->th_nkeyed = nbefore - h.nthird;
   s->th_width[s->th_ncol++] = width;
   s->th_done = true;
   counts->nrecords = nh; counts->nbefore = nbefore; counts->nheld = s->th_nkeyed; counts->ndropped = h.nthird;
   counts->width = width; counts->key_bits = h.key_bits; counts->ncolumns = s->th_ncol;
   return 0;
}

/* E2BIG, the held column untouched: a column of `width` bits does not fit behind the held key's */
static int tally_append_wide(const seeqdev_scan *s, uint32_t width)
{
   snprintf(g_last_error, sizeof g_last_error, "tally append: the held key has %u bits and the new column %u: more than %d together", s->th_key_bits, width,
            SEEQ_TALLY_WORD_BITS);
   errno = E2BIG;
   return -1;
}

extern "C" int seeqdevScanTallyHoldAppend(seeqdev_scan_t *s, int source, const void *d_text, size_t nbytes, seeqdev_tally_hold_counts_t *column,
                                          seeqdev_tally_append_counts_t *counts)
{
   const uint4 *rec;
   const uint64_t *off;
   uint64_t n;
   if (!counts) { seeqerr = 0; errno = EINVAL; return -1; }
   if (tally_hold_enter(s, column, source, tally_append_missing(s, false), &d_text, &nbytes, &rec, &off, &n)) return -1;
   memset(counts, 0, sizeof *counts);
   if (tally_hold_run(s, rec, off, (uint32_t)n, source == SEEQDEV_TALLY_DEMUX, d_text, nbytes, column, tally_append_target(s))) return -1;
   if (!tally_append_fits(s->th_key_bits, column->key_bits)) return tally_append_wide(s, column->key_bits);
   return tally_append_join(s, (uint32_t)n, column->key_bits, counts);
}

extern "C" int seeqdevScanTallyHoldAppendLibrary(seeqdev_scan_t *s, int source, const void *d_text, size_t nbytes, seeqdev_tally_library_counts_t *column,
                                                 seeqdev_tally_append_counts_t *counts)
{
   const uint4 *rec;
   const uint64_t *off;
   uint64_t n;
   if (!counts) { seeqerr = 0; errno = EINVAL; return -1; }
   if (tally_enter(s, column, source, tally_append_missing(s, true), &d_text, &nbytes, &rec, &off, &n)) return -1;
   memset(&s->lb_edits, 0, sizeof s->lb_edits);             /* (no span with a key: no assignment, and no split of one before) */
   memset(counts, 0, sizeof *counts);
   seeqdev_tally_hold_counts_t held;
   if (tally_hold_run(s, rec, off, (uint32_t)n, false, d_text, nbytes, &held, tally_append_target(s))) return -1;
   memset(column, 0, sizeof *column);
   column->nspans = n;
   column->key_bits = tally_lib_bitlen(s->lb_n);
   column->nlong = held.nlong; column->nforeign = held.nforeign;
   TallyLibCnt l = {};
   if (held.nheld) {
      /* the miss indices go where the plain tally's second key array lies, as in seeqdevScanTallyHoldLibrary */
      if (tally_ws_keys(s, (size_t)n)) return -1;
      if ((size_t)n > s->cap_tl || (size_t)n > s->cap_ta) {
         snprintf(g_last_error, sizeof g_last_error, "library append: %llu records, arrays for %zu and %zu", (unsigned long long)n, s->cap_ta, s->cap_tl);
         errno = EIO;
         return -1;
      }
      if (tally_library_assign(s, s->ta_key, (uint32_t *)s->tl_key1, (uint32_t)n, held.nheld, &l)) return -1;
   }
   tally_library_counts(column, l);
   if (column->nexact + column->ncorrected + column->nambiguous + column->nunknown + column->nlong + column->nforeign != n)
      return tally_library_fail("append", l, TallyCnt{}, (uint32_t)n, held.nheld, column->nassigned, s->lb_n);
   if (!tally_append_fits(s->th_key_bits, column->key_bits)) return tally_append_wide(s, column->key_bits);
   return tally_append_join(s, (uint32_t)n, column->key_bits, counts);
}

extern "C" int seeqdevScanTallyHoldColumns(const seeqdev_scan_t *s, uint32_t *widths, int cap)
{
   if (!s || cap < 0 || (!widths && cap)) { errno = EINVAL; return -1; }
   const int ncol = s->th_done ? (int)s->th_ncol : 0;
   for (int c = 0; c < ncol && c < cap; c++) widths[c] = s->th_width[c];
   return ncol;
}

extern "C" int seeqdevScanCopyHeld(seeqdev_scan_t *s, uint32_t *lines_out, uint64_t *keys_out, size_t first, size_t n)
{
   const size_t have = s && s->th_done ? s->th_n : 0;
   if (copy_out(s, NULL, NULL, 0, have, first, 0)) return -1;      /* (the bounds of first alone: either array may be left out) */
   if (n > have - first) { errno = EINVAL; return -1; }
   if (lines_out && copy_out(s, lines_out, s->th_line, sizeof(uint32_t), have, first, n)) return -1;
   if (keys_out && copy_out(s, keys_out, s->th_key, sizeof(uint64_t), have, first, n)) return -1;
   return 0;
}

extern "C" int seeqdevTallySplit(uint64_t key, const uint32_t *widths, int ncolumns, uint64_t *out)
{
   if (!widths || !out || tally_split(key, widths, ncolumns, out)) { errno = EINVAL; return -1; }
   return 0;
}

#endif
