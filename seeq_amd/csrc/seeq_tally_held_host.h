/*
 * seeq_tally_held_host.h -- the host driver of the tally of the held column itself (rule and kernels: seeq_tally_held.h): the pack of the
 * held words, as many passes of the single-word sort as the largest held key asks for, the run-length pass with its two tables, the dense
 * matrix, and the seeqdevScanTallyHeld / seeqdevScanTallyHeldRows* / seeqdevScanTallyHeldDense / seeqdevTallyHeldCell entries.  THE KEY
 * TABLE is the context's tally table (tl_tab, tl_n), as the library tally's is; the row table is a group of this call's own.  Included by
 * seeq_device.hip behind seeq_tally_collapse_host.h.
 */
#ifndef SEEQ_TALLY_HELD_HOST_H_
#define SEEQ_TALLY_HELD_HOST_H_

static int tally_held_fail(const char *what, const TallyHeldCnt &h, uint32_t n, uint64_t ncounted)
{
   snprintf(g_last_error, sizeof g_last_error,
            "internal inconsistency in the held tally (%s: flags %u, %u records, %u keyless, %u repeats, %llu counted, %u bits, %u nonzero items, %u keys, %u rows, "
            "key heads %u .. %u, first row head %u of rank %u, %u entries outside with %llu reads)",
            what, h.bad, n, h.nkeyless, h.nrepeat, (unsigned long long)ncounted, h.key_bits, h.nonzero, h.nkeys, h.nrows, h.key_first, h.key_last, h.row_first,
            h.rank_first, h.noutside, (unsigned long long)h.outside_reads);
   errno = EIO;
   return -1;
}

static int tally_held_ws_cnt(seeqdev_scan *s)
{
   return ws_make(&s->ws, {{s->d_thdcnt, sizeof(TallyHeldCnt)}, {s->h_thdcnt, sizeof(TallyHeldCnt), WS_PINNED}});
}

/* The two tables of the held column under a column part of `shift` bits (rows: with a row table); the context's tally table (tl_tab: tl_n)
   and thd_rows (thd_nrows) are the result.  Waits. */
static int tally_held_run(seeqdev_scan *s, uint32_t shift, bool rows, seeqdev_tally_held_counts_t *counts)
{
   const hipStream_t st = s->stream;
   const uint32_t n = (uint32_t)s->th_n;
   if (!n) return 0;                                       /* no records: nothing is launched, the tables are empty */
   const size_t nt = (size_t)tally_tiles(n);
   if (tally_ws_keys(s, n) || tally_held_ws_cnt(s)) return -1;
   if (ws_grow(&s->ws, &s->cap_thd, n, {{s->thd_sum, 3 * (nt + 1) * sizeof(uint32_t)}})) return -1;
   TallyHeldArgs a;
   memset(&a, 0, sizeof a);
   a.line = s->th_line; a.key = s->th_key; a.n = n; a.nt = (uint32_t)nt;
   a.shift = shift;
   a.tstat = s->tl_stat;
   a.rsum = s->thd_sum;
   a.cnt = s->d_thdcnt;
   TallySortArgs sa = tally_sort_args(s, n, s->tl_stat);
   a.src = sa.src[0];
   if ((size_t)n > s->cap_tl || (size_t)n > s->cap_thd || (size_t)n > s->cap_th || tally_tiles(s->cap_tl) < nt || tally_tiles(s->cap_thd) < nt ||
       tally_chunks(s->cap_tl) < sa.nb || shift > SEEQ_TALLY_WORD_BITS) {
      snprintf(g_last_error, sizeof g_last_error, "held tally: %u held records, arrays for %zu, %zu and %zu; a column part of %u bits", n, s->cap_th, s->cap_tl,
               s->cap_thd, shift);
      errno = EIO;
      return -1;
   }
   if (s->tm_thd.begin(s->prof, st)) return -1;
   HIP_TRY(hipMemsetAsync(s->d_thdcnt, 0, sizeof(TallyHeldCnt), st), EIO);
   hipLaunchKernelGGL(k_tally_held_pack, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_tally_held_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
   if (counters_fetch(s, s->h_thdcnt, s->d_thdcnt, sizeof(TallyHeldCnt))) return -1;
   TallyHeldCnt h = *s->h_thdcnt;
   if (h.bad || (uint64_t)h.nkeyless + h.nrepeat > n || h.key_bits > s->th_key_bits || s->th_key_bits > SEEQ_TALLY_WORD_BITS)
      return tally_held_fail("pack", h, n, 0);
   const uint64_t ncounted = (uint64_t)n - h.nkeyless - h.nrepeat;
   if ((ncounted > 0u) != (h.key_bits > 0u) || ncounted > s->th_nkeyed) return tally_held_fail("kinds", h, n, ncounted);
   const TallyHeldCnt packed = h;
   const uint32_t passes = tally_held_passes(ncounted, s->th_key_bits);
   if (ncounted) {
      TallyPass list[SEEQ_TALLY_PASS_MAX];
      tally_sort_run(st, &sa, 1, list, tally_pass_list(list, passes, 0u));
      a.src = sa.src[0];
      hipLaunchKernelGGL(k_tally_held_rle_reduce, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
      hipLaunchKernelGGL(k_tally_held_rle_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
      if (counters_fetch(s, s->h_thdcnt, s->d_thdcnt, sizeof(TallyHeldCnt))) return -1;
      h = *s->h_thdcnt;
      if (h.bad || h.nonzero != ncounted || h.nrows == 0 || h.nrows > h.nkeys || h.nkeys > ncounted) return tally_held_fail("sort", h, n, ncounted);
      /* the tables: the tally's own table, and a group of this call's, grown now that their sizes are known */
      const size_t nk = h.nkeys, nr = rows ? h.nrows : 0;
      if (ws_grow(&s->ws, &s->cap_tl_tab, nk, {{s->tl_tab, nk * sizeof(seeqdev_tally_t)}})) return -1;
      if (ws_grow(&s->ws, &s->cap_thd_rows, nr, {{s->thd_rows, nr * sizeof(seeqdev_tally_group_t)}})) return -1;
      a.nk = (uint32_t)nk; a.nr = (uint32_t)nr;
      a.kpos = (uint32_t *)sa.dst[0];                      /* (4 bytes per key head and 4 per row head in the 8 bytes per record the last pass left free) */
      a.rrank = a.kpos + n;
      a.tab = (uint4 *)s->tl_tab; a.rtab = (uint64_t *)s->thd_rows;
      a.cap_tab = cap_u32(s->cap_tl_tab); a.cap_rtab = cap_u32(s->cap_thd_rows);
      hipLaunchKernelGGL(k_tally_held_rle_apply, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
      hipLaunchKernelGGL(k_tally_held_table, dim3((unsigned)((nk + SEEQ_TILE_WG - 1) / SEEQ_TILE_WG)), dim3(SEEQ_TILE_WG), 0, st, a);
      if (nr) hipLaunchKernelGGL(k_tally_held_rows, dim3((unsigned)((nr + SEEQ_TILE_WG - 1) / SEEQ_TILE_WG)), dim3(SEEQ_TILE_WG), 0, st, a);
      if (counters_copy(s, s->h_thdcnt, s->d_thdcnt, sizeof(TallyHeldCnt))) return -1;
   }
   if (s->tm_thd.end(s->prof, st)) return -1;
   HIP_TRY(hipStreamSynchronize(st), EIO);
   s->tm_thd.read(s->prof);
   if (ncounted) {
      h = *s->h_thdcnt;
      /* what the apply placed: the counts of either table telescope to n - its first head's index (the items that are 0 lie before it), the
         last key head lies behind the first one unless it is the same, the rows' ndistinct telescope to nkeys - the first row's rank */
      if (h.bad || (uint64_t)n - h.key_first != ncounted || h.key_last >= n || h.key_last < h.key_first || (h.key_last == h.key_first) != (h.nkeys == 1u) ||
          (rows && ((uint64_t)n - h.row_first != ncounted || h.rank_first != 0u)))
         return tally_held_fail("tables", h, n, ncounted);
      s->tl_n = h.nkeys;
      s->thd_nrows = rows ? h.nrows : 0;
      counts->ndistinct = h.nkeys; counts->nrows = s->thd_nrows;
   }
   counts->ncounted = ncounted; counts->nkeyless = packed.nkeyless; counts->nrepeat = packed.nrepeat;
   counts->key_bits = packed.key_bits; counts->passes = passes;
   return 0;
}

extern "C" int seeqdevScanTallyHeld(seeqdev_scan_t *s, int member_columns, seeqdev_tally_held_counts_t *counts)
{
   seeqerr = 0;
   if (!s || !counts) { errno = EINVAL; return -1; }
   uint32_t shift = 0;
   if (!s->th_done || tally_held_shift(s->th_width, (int)s->th_ncol, member_columns, &shift)) {
      if (!s->th_done) snprintf(g_last_error, sizeof g_last_error, "held tally: the context holds no held column (seeqdevScanTallyHold)");
      else snprintf(g_last_error, sizeof g_last_error, "held tally: %d member columns of a held key of %u columns", member_columns, s->th_ncol);
      errno = EINVAL;
      return -1;
   }
   if (s->th_n > 0xFFFFFFFFull) { errno = E2BIG; return -1; }
   if (use_device(s->device)) return -1;
   s->tl_n = 0;                                            /* (the table of the tally before, of any kind, is gone, whatever comes of this one) */
   s->thd_live = false;
   s->thd_nrows = 0;
   s->tm_thd.ms = 0.f;
   memset(counts, 0, sizeof *counts);
   counts->nrecords = s->th_n;
   counts->shift = shift; counts->member_columns = (uint32_t)member_columns;
   if (tally_held_run(s, shift, member_columns > 0, counts)) return -1;
   s->thd_shift = shift; s->thd_members = (uint32_t)member_columns; s->thd_ncounted = counts->ncounted;
   s->thd_live = true;                                     /* (a tally that counted nothing included) */
   return 0;
}

extern "C" const seeqdev_tally_group_t *seeqdevScanTallyHeldRowsDevice(const seeqdev_scan_t *s) { return s ? s->thd_rows : NULL; }

extern "C" int seeqdevScanCopyTallyHeldRows(seeqdev_scan_t *s, seeqdev_tally_group_t *host_out, size_t first, size_t n)
{
   return copy_out(s, host_out, s ? s->thd_rows : NULL, sizeof(seeqdev_tally_group_t), s ? s->thd_nrows : 0, first, n);
}

extern "C" int seeqdevScanTallyHeldDense(seeqdev_scan_t *s, void *d_out, uint32_t nrows, uint32_t ncols, seeqdev_tally_dense_counts_t *counts)
{
   seeqerr = 0;
   /* the arguments first, then what the context must hold */
   if (!s || !d_out || !counts) { errno = EINVAL; return -1; }
   const uint64_t ncells = (uint64_t)nrows * ncols;
   if (!ncells || ncells > SEEQDEV_TALLY_DENSE_MAX) {
      snprintf(g_last_error, sizeof g_last_error, "held matrix: %u x %u cells: at least one and at most %llu", nrows, ncols, (unsigned long long)SEEQDEV_TALLY_DENSE_MAX);
      errno = ncells ? E2BIG : EINVAL;
      return -1;
   }
   if (!s->thd_live || !s->thd_members) {
      snprintf(g_last_error, sizeof g_last_error, "held matrix: %s", !s->thd_live ? "the context's tally table is not that of a held tally (seeqdevScanTallyHeld)"
                                                                                  : "the held tally had no member columns: its keys have no column part");
      errno = EINVAL;
      return -1;
   }
   if (use_device(s->device)) return -1;
   const hipStream_t st = s->stream;
   const size_t nk = s->tl_n;
   const size_t nd = (nk + SEEQ_TILE_WG - 1) / SEEQ_TILE_WG;
   memset(counts, 0, sizeof *counts);
   s->tm_thd.ms = 0.f;
   if (nk > s->cap_tl_tab || nk > 0xFFFFFFFFull) {
      snprintf(g_last_error, sizeof g_last_error, "held matrix: %zu entries, a table for %zu", nk, s->cap_tl_tab);
      errno = EIO;
      return -1;
   }
   if (nk && (tally_held_ws_cnt(s) || ws_grow(&s->ws, &s->cap_thd_dense, nd, {{s->thd_dn, nd * sizeof(uint32_t)}, {s->thd_dr, nd * sizeof(uint64_t)}}))) return -1;
   if (s->tm_thd.begin(s->prof, st)) return -1;
   HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)ncells * sizeof(uint64_t), st), EIO);
   if (nk) {                                               /* an empty table: the zero matrix, nothing is launched */
      TallyHeldArgs a;
      memset(&a, 0, sizeof a);
      a.shift = s->thd_shift;
      a.nk = (uint32_t)nk; a.tab = (uint4 *)s->tl_tab; a.cap_tab = cap_u32(s->cap_tl_tab);
      a.out = (uint64_t *)d_out; a.nrows = nrows; a.ncols = ncols;
      a.dn = s->thd_dn; a.dr = s->thd_dr; a.nd = (uint32_t)nd;
      a.cnt = s->d_thdcnt;
      hipLaunchKernelGGL(k_tally_held_dense, dim3(a.nd), dim3(SEEQ_TILE_WG), 0, st, a);
      hipLaunchKernelGGL(k_tally_held_dense_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
      if (counters_copy(s, s->h_thdcnt, s->d_thdcnt, sizeof(TallyHeldCnt))) return -1;
   }
   if (s->tm_thd.end(s->prof, st)) return -1;
   HIP_TRY(hipStreamSynchronize(st), EIO);
   s->tm_thd.read(s->prof);
   uint64_t noutside = 0, outside_reads = 0;
   if (nk) {
      const TallyHeldCnt h = *s->h_thdcnt;
      if (h.noutside > nk || h.outside_reads > s->thd_ncounted || (h.noutside == 0u) != (h.outside_reads == 0u)) return tally_held_fail("matrix", h, (uint32_t)s->th_n, s->thd_ncounted);
      noutside = h.noutside; outside_reads = h.outside_reads;
   }
   counts->noutside = noutside; counts->ninside = nk - noutside;
   counts->outside_reads = outside_reads; counts->inside_reads = s->thd_ncounted - outside_reads;
   return 0;
}

extern "C" int seeqdevScanLastTallyHeldMs(const seeqdev_scan_t *s, float *ms)
{
   if (!s || !ms) { errno = EINVAL; return -1; }
   *ms = s->tm_thd.ms;
   return 0;
}

extern "C" int seeqdevTallyHeldCell(uint64_t key, uint32_t shift, uint32_t nrows, uint32_t ncols, uint64_t *cell)
{
   if (!cell || shift > SEEQ_TALLY_WORD_BITS) { errno = EINVAL; return -1; }
   return tally_held_cell(key, shift, nrows, ncols, cell);
}

#endif
