/*
 * seeq_insert_host.h -- the host driver of the insert between two flanks (rule and kernels: seeq_insert.h): the right flank's scan under
 * SQ_ALL with its records kept aside (side_keep), the left flank's scan under the call's mode, the join and the
 * compaction on the device, the gather of the insert text, and the seeqdevScan*Insert* entries.  Included by seeq_device.hip behind
 * seeq_strand_host.h.
 */
#ifndef SEEQ_INSERT_HOST_H_
#define SEEQ_INSERT_HOST_H_

/* the reduction's per-tile sums for n left records (seeq_insert.h: kept and both per tile; text bytes per tile) */
static size_t insert_tiles(size_t n) { return n / SEEQ_TILE + 2; }

/* Room for n joined records and their tiles' sums.  Nothing on the stream reads the old blocks: every inserts call ends synchronised. */
static int inserts_ws_join(seeqdev_scan *s, size_t n)
{
   if (ws_make(&s->ws, {{s->d_inscnt, sizeof(InsertCnt)}, {s->h_inscnt, sizeof(InsertCnt), WS_PINNED}})) return -1;
   return ws_grow(&s->ws, &s->cap_ins_jn, n, {{s->ins_jn, n * sizeof(uint4)}, {s->ins_bsum, 2 * insert_tiles(n) * sizeof(uint32_t)},
                                              {s->ins_bbytes, insert_tiles(n) * sizeof(uint64_t)}});
}

/* Room for n insert records: the result's arrays. */
static int inserts_ws_result(seeqdev_scan *s, size_t n)
{
   return ws_grow(&s->ws, &s->cap_ins, n, {{s->ins_rec, n * sizeof(uint4)}, {s->ins_off, n * sizeof(uint64_t)}, {s->ins_pos, n * sizeof(uint64_t)}});
}

static int inserts_args_ok(const seeqdev_scan_t *s, const seeqdev_pattern_t *left, const seeqdev_pattern_t *right, const void *text, size_t nbytes,
                           int options, uint32_t min_len, uint32_t max_len, const seeqdev_insert_counts_t *counts)
{
   if (!s || !left || !right || !counts || (!text && nbytes)) return 0;
   if (options & (SEEQDEV_SINGLELINE | MASK_INPUT)) return 0;
   if ((options & MASK_MATCH) == SQ_ALL || (options & MASK_MATCH) == SQ_COUNT) return 0;
   if (max_len != 0 && min_len > max_len) return 0;
   const seeqdev_pattern_t *pair[2] = {left, right};
   return scan_args_ok(s, pair, 2, options, SEEQDEV_WANT_RECORDS);
}

/* Join the nl left records the context's record workspace holds (s->records / s->rec_off) with the nr right records kept aside, by the
   rule of seeq_insert.h; the result goes to ins_rec / ins_off / ins_pos, its totals to *counts (nboth, ninserts, text_bytes).  Waits. */
static int inserts_join(seeqdev_scan *s, uint32_t nl, uint32_t nr, int mode, uint32_t min_len, uint32_t max_len, seeqdev_insert_counts_t *counts)
{
   const hipStream_t st = s->stream;
   counts->nboth = counts->ninserts = counts->text_bytes = 0;
   if (!nl || !nr) return 0;                               /* no line has both: nothing is launched */
   if (inserts_ws_join(s, nl)) return -1;
   InsertArgs a;
   memset(&a, 0, sizeof a);
   a.left = (const uint4 *)s->records; a.left_off = s->rec_off; a.nl = nl;
   a.right = (const uint4 *)s->side_rec; a.nr = nr;
   a.min_len = min_len; a.max_len = max_len; a.mode = mode;
   a.jn = s->ins_jn; a.cap_jn = cap_u32(s->cap_ins_jn);
   a.nt = (uint32_t)seeq_tiles_of(nl);
   a.bsum = s->ins_bsum; a.bbytes = s->ins_bbytes;
   a.cnt = s->d_inscnt;
   if (insert_tiles(s->cap_ins_jn) < (size_t)a.nt || (size_t)nr > s->cap_side) {
      snprintf(g_last_error, sizeof g_last_error, "inserts: %u left and %u right records, tile sums for %zu, side copy for %zu", nl, nr, s->cap_ins_jn, s->cap_side);
      errno = EIO;
      return -1;
   }
   if (s->tm_ins.begin(s->prof, st)) return -1;
   HIP_TRY(hipMemsetAsync(s->d_inscnt, 0, sizeof(InsertCnt), st), EIO);
   hipLaunchKernelGGL(k_insert_join, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_insert_reduce, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_insert_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
   if (counters_fetch(s, s->h_inscnt, s->d_inscnt, sizeof(InsertCnt))) return -1;
   const InsertCnt h = *s->h_inscnt;
   if (h.bad || h.kept > h.both || h.both > nl || h.bytes < h.kept) {
      snprintf(g_last_error, sizeof g_last_error, "internal inconsistency in the insert join (flags %u, %u inserts, %u of %u lines with both flanks, %llu bytes)", h.bad,
               h.kept, h.both, nl, (unsigned long long)h.bytes);
      errno = EIO;
      return -1;
   }
   if (h.kept) {
      if (inserts_ws_result(s, h.kept)) return -1;
      a.out = s->ins_rec; a.off_out = s->ins_off; a.pos_out = s->ins_pos;
      a.cap_out = cap_u32(s->cap_ins);
      hipLaunchKernelGGL(k_insert_apply, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
      if (counters_copy(s, s->h_inscnt, s->d_inscnt, sizeof(InsertCnt))) return -1;
   }
   if (s->tm_ins.end(s->prof, st)) return -1;
   HIP_TRY(hipStreamSynchronize(st), EIO);
   s->tm_ins.read(s->prof);
   if (s->h_inscnt->bad) {
      snprintf(g_last_error, sizeof g_last_error, "internal inconsistency in the insert join (an index outside the output)");
      errno = EIO;
      return -1;
   }
   counts->nboth = h.both; counts->ninserts = h.kept; counts->text_bytes = h.bytes;
   return 0;
}

/* The two scans and the join.  The context is left with nothing to fetch whatever the outcome (the caller forgets the scans). */
static int inserts_run(seeqdev_scan_t *s, const seeqdev_pattern_t *left, const seeqdev_pattern_t *right, const void *d_text, size_t nbytes, int options,
                       uint32_t min_len, uint32_t max_len, seeqdev_insert_counts_t *counts)
{
   const int mode = options & MASK_MATCH, rest = options & ~MASK_MATCH;
   seeqdev_counts_t cr, cl;
   /* the right flank first: every occurrence, kept aside while the left flank is scanned */
   if (seeqdevScanRun(s, right, d_text, nbytes, rest | SQ_ALL, SEEQDEV_WANT_RECORDS)) return -1;
   if (seeqdevScanFetch(s, &cr)) return -1;
   if (cr.nrecords > 0xFFFFFFFFull) {
      snprintf(g_last_error, sizeof g_last_error, "inserts: more than 2^32 - 1 right records");
      errno = E2BIG;
      return -1;
   }
   if (side_keep(s, (size_t)cr.nrecords)) return -1;
   if (seeqdevScanRun(s, left, d_text, nbytes, rest | mode, SEEQDEV_WANT_RECORDS)) return -1;
   if (seeqdevScanFetch(s, &cl)) return -1;
   if (cl.nrecords > 0xFFFFFFFFull) {
      snprintf(g_last_error, sizeof g_last_error, "inserts: more than 2^32 - 1 left records");
      errno = E2BIG;
      return -1;
   }
   if (cl.nlines != cr.nlines) {
      snprintf(g_last_error, sizeof g_last_error, "inserts: the left flank counted %llu lines, the right flank %llu", (unsigned long long)cl.nlines,
               (unsigned long long)cr.nlines);
      errno = EIO;
      return -1;
   }
   memset(counts, 0, sizeof *counts);
   counts->nlines = cl.nlines;
   counts->nleft = cl.nrecords;                            /* (SQ_BEST / SQ_FIRST: one record per matching line) */
   counts->nright = cr.nmatchlines;                        /* (the right scan's own count of the records that open a line) */
   if (inserts_join(s, (uint32_t)cl.nrecords, (uint32_t)cr.nrecords, mode == SQ_BEST ? SEEQ_INSERT_BEST : SEEQ_INSERT_FIRST, min_len, max_len, counts)) return -1;
   if (counts->nboth > counts->nright) {
      snprintf(g_last_error, sizeof g_last_error, "internal inconsistency in the insert join (%llu lines with both flanks, %llu with a right one)",
               (unsigned long long)counts->nboth, (unsigned long long)counts->nright);
      errno = EIO;
      return -1;
   }
   return 0;
}

static int inserts_entry(seeqdev_scan_t *s, const seeqdev_pattern_t *left, const seeqdev_pattern_t *right, const void *d_text, size_t nbytes, int options,
                         uint32_t min_len, uint32_t max_len, seeqdev_insert_counts_t *counts, bool staged)
{
   s->ins_n = 0;                                           /* (the result of the call before is gone, whatever comes of this one) */
   s->ins_text_bytes = 0;
   s->ins_staged = false;
   s->ins_done = false;
   s->tm_ins.ms = 0.f;
   seeqdev_insert_counts_t c;
   const int rc = inserts_run(s, left, right, d_text, nbytes, options, min_len, max_len, &c);
   scan_forget(s);                                         /* (seeqdevScanFetch has nothing to fetch: the call is complete) */
   if (rc) return -1;
   s->ins_n = (size_t)c.ninserts;
   s->ins_text_bytes = c.text_bytes;
   s->ins_staged = staged;
   s->ins_staged_nbytes = nbytes;
   s->ins_done = true;
   *counts = c;
   return 0;
}

extern "C" int seeqdevScanRunInserts(seeqdev_scan_t *s, const seeqdev_pattern_t *left, const seeqdev_pattern_t *right, const void *d_text, size_t nbytes,
                                     int options, uint32_t min_len, uint32_t max_len, seeqdev_insert_counts_t *counts)
{
   seeqerr = 0;
   if (!inserts_args_ok(s, left, right, d_text, nbytes, options, min_len, max_len, counts)) { errno = EINVAL; return -1; }
   if (use_device(s->device)) return -1;
   return inserts_entry(s, left, right, d_text, nbytes, options, min_len, max_len, counts, false);
}

extern "C" int seeqdevScanHostInserts(seeqdev_scan_t *s, const seeqdev_pattern_t *left, const seeqdev_pattern_t *right, const char *host_text, size_t nbytes,
                                      int options, uint32_t min_len, uint32_t max_len, seeqdev_insert_counts_t *counts)
{
   seeqerr = 0;
   if (!inserts_args_ok(s, left, right, host_text, nbytes, options, min_len, max_len, counts)) { errno = EINVAL; return -1; }
   if (use_device(s->device)) return -1;
   if (text_upload(s, host_text, nbytes, false)) return -1;
   return inserts_entry(s, left, right, s->d_text, nbytes, options, min_len, max_len, counts, true);
}

extern "C" const seeqdev_insert_t *seeqdevScanInsertsDevice(const seeqdev_scan_t *s) { return s ? (const seeqdev_insert_t *)s->ins_rec : NULL; }

extern "C" int seeqdevScanCopyInserts(seeqdev_scan_t *s, seeqdev_insert_t *host_out, size_t first, size_t n)
{
   return copy_out(s, host_out, s ? s->ins_rec : NULL, sizeof(seeqdev_insert_t), s ? s->ins_n : 0, first, n);
}

extern "C" int seeqdevScanCopyInsertOffsets(seeqdev_scan_t *s, uint64_t *host_out, size_t first, size_t n)
{
   return copy_out(s, host_out, s ? s->ins_off : NULL, sizeof(uint64_t), s ? s->ins_n : 0, first, n);
}

extern "C" int seeqdevScanInsertText(seeqdev_scan_t *s, const void *d_text, size_t nbytes, void *d_out, size_t out_cap, uint64_t *out_bytes)
{
   seeqerr = 0;
   if (!s || !out_bytes) { errno = EINVAL; return -1; }
   const uint64_t total = s->ins_text_bytes;
   *out_bytes = total;
   if (!d_out && out_cap == 0) return 0;                   /* the size query */
   if ((uint64_t)out_cap < total) { errno = ERANGE; return -1; }
   if (!d_out) { errno = EINVAL; return -1; }
   if (staged_text(s, "insert text", &d_text, &nbytes)) return -1;
   if (total == 0) return 0;
   const uint64_t blocks = (total + (uint64_t)SEEQ_INSERT_RUN * SEEQ_TILE_WG - 1) / ((uint64_t)SEEQ_INSERT_RUN * SEEQ_TILE_WG);
   if (blocks > 0x7FFFFFFFull) { errno = E2BIG; return -1; }
   if (use_device(s->device)) return -1;
   const hipStream_t st = s->stream;
   InsertTextArgs a;
   memset(&a, 0, sizeof a);
   a.rec = s->ins_rec; a.off = s->ins_off; a.pos = s->ins_pos; a.n = (uint32_t)s->ins_n;
   a.total = total;
   a.text = (const uint8_t *)d_text; a.nbytes = nbytes;
   a.out = (uint8_t *)d_out;
   a.cnt = s->d_inscnt;
   HIP_TRY(hipMemsetAsync(&s->d_inscnt->bad, 0, sizeof(uint32_t), st), EIO);
   hipLaunchKernelGGL(k_insert_text, dim3((unsigned)blocks), dim3(SEEQ_TILE_WG), 0, st, a);
   if (counters_fetch(s, s->h_inscnt, s->d_inscnt, sizeof(InsertCnt))) return -1;
   if (s->h_inscnt->bad) {
      snprintf(g_last_error, sizeof g_last_error, "insert text: a record lies outside the %zu bytes of text it was given", nbytes);
      errno = EIO;
      return -1;
   }
   return 0;
}

extern "C" int seeqdevScanLastInsertsMs(const seeqdev_scan_t *s, float *join_ms)
{
   if (!s || !join_ms) { errno = EINVAL; return -1; }
   *join_ms = s->tm_ins.ms;
   return 0;
}

#endif
