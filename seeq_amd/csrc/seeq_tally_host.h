/*
 * seeq_tally_host.h -- the host driver of the tally of distinct spans (rule and kernels: seeq_tally.h): which record array a source
 * names, the pack, as many passes of the sort as the largest tallied length asks for, the run-length pass, and the seeqdevScan*Tally*
 * and seeqdevTally* entries.  Included by seeq_device.hip behind seeq_insert_host.h.
 */
#ifndef SEEQ_TALLY_HOST_H_
#define SEEQ_TALLY_HOST_H_

/* Room for n spans: the two key arrays, the digit matrix, the tiles' sums -- one group.  Nothing on the stream reads the old blocks:
   every tally ends synchronised. */
static int tally_ws_keys(seeqdev_scan *s, size_t n)
{
   if (ws_make(&s->ws, {{s->d_tlcnt, sizeof(TallyCnt)}, {s->h_tlcnt, sizeof(TallyCnt), WS_PINNED}})) return -1;
   const size_t nt = (size_t)tally_tiles(n) + 1;
   return ws_grow(&s->ws, &s->cap_tl, n, {{s->tl_key0, n * sizeof(uint64_t)}, {s->tl_key1, n * sizeof(uint64_t)},
                                          {s->tl_mat, nt * SEEQ_TALLY_RADIX * sizeof(uint32_t)},
                                          {s->tl_sum, (2 * nt + (size_t)tally_chunks(n) + 1) * sizeof(uint32_t)}, {s->tl_stat, nt * sizeof(uint4)}});
}

static int tally_fail(const char *what, const TallyCnt &h, uint32_t n, uint64_t ntallied)
{
   snprintf(g_last_error, sizeof g_last_error, "internal inconsistency in the tally (%s: flags %u, %u spans, %llu tallied, %u nonzero keys, %u distinct, first head %u)",
            what, h.bad, n, (unsigned long long)ntallied, h.nonzero, h.ndistinct, h.first);
   errno = EIO;
   return -1;
}

/* The table of the n spans rec / off of text[0 .. nbytes); the context's table (tl_tab, tl_n) is the result.  Waits. */
static int tally_run(seeqdev_scan *s, const uint4 *rec, const uint64_t *off, uint32_t n, const void *d_text, size_t nbytes, seeqdev_tally_counts_t *counts)
{
   const hipStream_t st = s->stream;
   memset(counts, 0, sizeof *counts);
   counts->nspans = n;
   if (!n) return 0;                                       /* no spans: nothing is launched */
   if (tally_ws_keys(s, n)) return -1;
   TallyArgs a;
   memset(&a, 0, sizeof a);
   a.rec = rec; a.off = off; a.n = n;
   a.nt = (uint32_t)tally_tiles(n);
   a.text = (const uint8_t *)d_text; a.nbytes = nbytes;
   a.src = s->tl_key0; a.dst = s->tl_key1;
   a.mat = s->tl_mat; a.nmat = (uint32_t)tally_matrix(n); a.nb = (uint32_t)tally_chunks(n);
   a.rsum = s->tl_sum; a.bsum = s->tl_sum + 2 * (size_t)a.nt;
   a.tstat = s->tl_stat;
   a.cnt = s->d_tlcnt;
   if ((size_t)n > s->cap_tl || tally_tiles(s->cap_tl) < a.nt || tally_chunks(s->cap_tl) < a.nb) {
      snprintf(g_last_error, sizeof g_last_error, "tally: %u spans, arrays for %zu", n, s->cap_tl);
      errno = EIO;
      return -1;
   }
   if (s->tm_tl.begin(s->prof, st)) return -1;
   HIP_TRY(hipMemsetAsync(s->d_tlcnt, 0, sizeof(TallyCnt), st), EIO);
   hipLaunchKernelGGL(k_tally_pack, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_tally_pack_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
   if (counters_fetch(s, s->h_tlcnt, s->d_tlcnt, sizeof(TallyCnt))) return -1;
   TallyCnt h = *s->h_tlcnt;
   if (h.bad) {
      snprintf(g_last_error, sizeof g_last_error, "tally: a span lies outside the %zu bytes of text it was given", nbytes);
      errno = EIO;
      return -1;
   }
   if ((uint64_t)h.nlong + h.nforeign > n || h.max_len > SEEQ_TALLY_LEN_MAX) return tally_fail("pack", h, n, 0);
   const uint64_t ntallied = (uint64_t)n - h.nlong - h.nforeign;
   const TallyCnt packed = h;
   uint32_t passes = 0;
   if (ntallied) {
      passes = tally_passes(h.max_len);
      for (uint32_t p = 0; p < passes; p++) {
         a.pass = p;
         hipLaunchKernelGGL(k_tally_hist, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
         hipLaunchKernelGGL(k_tally_scan_reduce, dim3(a.nb), dim3(SEEQ_TILE_WG), 0, st, a);
         hipLaunchKernelGGL(k_tally_scan_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
         hipLaunchKernelGGL(k_tally_scan_apply, dim3(a.nb), dim3(SEEQ_TILE_WG), 0, st, a);
         hipLaunchKernelGGL(k_tally_scatter, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
         uint64_t *t = a.src; a.src = a.dst; a.dst = t;     /* (the pass's output is the next one's input) */
      }
      hipLaunchKernelGGL(k_tally_rle_reduce, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
      hipLaunchKernelGGL(k_tally_rle_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
      if (counters_fetch(s, s->h_tlcnt, s->d_tlcnt, sizeof(TallyCnt))) return -1;
      h = *s->h_tlcnt;
      if (h.bad || h.nonzero != ntallied || h.ndistinct > h.nonzero || h.ndistinct == 0) return tally_fail("sort", h, n, ntallied);
      /* the table: a group of its own, grown now that ndistinct is known */
      const size_t nd = h.ndistinct;
      if (ws_grow(&s->ws, &s->cap_tl_tab, nd, {{s->tl_tab, nd * sizeof(seeqdev_tally_t)}})) return -1;
      a.nd = h.ndistinct;
      a.pos = (uint32_t *)a.dst;                           /* (4 bytes per head in the 8 bytes per span the last pass left free) */
      a.tab = (uint4 *)s->tl_tab;
      a.cap_tab = cap_u32(s->cap_tl_tab);
      hipLaunchKernelGGL(k_tally_rle_apply, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
      hipLaunchKernelGGL(k_tally_table, dim3((unsigned)((nd + SEEQ_TILE_WG - 1) / SEEQ_TILE_WG)), dim3(SEEQ_TILE_WG), 0, st, a);
      if (counters_copy(s, s->h_tlcnt, s->d_tlcnt, sizeof(TallyCnt))) return -1;
   }
   if (s->tm_tl.end(s->prof, st)) return -1;
   HIP_TRY(hipStreamSynchronize(st), EIO);
   s->tm_tl.read(s->prof);
   if (ntallied) {
      h = *s->h_tlcnt;
      /* the counts of the table telescope to n - the first head's index: the keys that are 0 lie before it */
      if (h.bad || (uint64_t)n - h.first != ntallied) return tally_fail("table", h, n, ntallied);
      s->tl_n = h.ndistinct;
      counts->ndistinct = h.ndistinct;
   }
   counts->ntallied = ntallied; counts->nlong = packed.nlong; counts->nforeign = packed.nforeign;
   counts->max_len = packed.max_len; counts->passes = passes;
   return 0;
}

/* Which record array a source names: SEEQDEV_TALLY_INSERTS or SEEQDEV_TALLY_HITS, with the preconditions of each (EINVAL; the staged text
   for a NULL text of the inserts) -- shared by seeqdevScanTally and the grouped tally's two calls (seeq_tally_group_host.h). */
static int tally_source(seeqdev_scan *s, int source, const void **d_text, size_t *nbytes, const uint4 **rec, const uint64_t **off, uint64_t *n)
{
   if (source == SEEQDEV_TALLY_INSERTS) {
      if (!s->ins_done) {
         snprintf(g_last_error, sizeof g_last_error, "tally: the context holds no result of an inserts call");
         errno = EINVAL;
         return -1;
      }
      if (staged_text(s, "tally", d_text, nbytes)) return -1;
      *rec = s->ins_rec; *off = s->ins_off; *n = s->ins_n;
   } else {
      /* what seeqdevScanCopyRecords serves: the records of a fetched scan or of a both-strands call.  A context with nothing to fetch
         (fresh, or after a multi, demux or inserts call: scan_forget) has none; a packed scan's offsets are no offsets into a text */
      const bool nothing = !s->ran && !s->pat && !s->counts.nlines && !s->counts.nrecords;
      const bool packed = s->is_packed || (s->d_unpack && s->text == (const void *)s->d_unpack);
      if (nothing || packed || !*d_text) {
         snprintf(g_last_error, sizeof g_last_error, "tally: %s", nothing ? "the context holds no fetched records" : packed ? "the records of a packed scan carry no text offsets"
                                                                                                                       : "the hits need the text they were found in");
         errno = EINVAL;
         return -1;
      }
      *rec = (const uint4 *)s->records; *off = s->rec_off; *n = s->counts.nrecords;
   }
   return 0;
}

extern "C" int seeqdevScanTally(seeqdev_scan_t *s, int source, const void *d_text, size_t nbytes, seeqdev_tally_counts_t *counts)
{
   seeqerr = 0;
   if (!s || !counts || (source != SEEQDEV_TALLY_INSERTS && source != SEEQDEV_TALLY_HITS) || (!d_text && nbytes)) { errno = EINVAL; return -1; }
   const uint4 *rec;
   const uint64_t *off;
   uint64_t n;
   if (tally_source(s, source, &d_text, &nbytes, &rec, &off, &n)) return -1;
   if (n > 0xFFFFFFFFull) { errno = E2BIG; return -1; }
   if (use_device(s->device)) return -1;
   s->tl_n = 0;                                            /* (the table of the call before is gone, whatever comes of this one) */
   s->tm_tl.ms = 0.f;
   return tally_run(s, rec, off, (uint32_t)n, d_text, nbytes, counts);
}

extern "C" const seeqdev_tally_t *seeqdevScanTallyDevice(const seeqdev_scan_t *s) { return s ? s->tl_tab : NULL; }

extern "C" int seeqdevScanCopyTally(seeqdev_scan_t *s, seeqdev_tally_t *host_out, size_t first, size_t n)
{
   return copy_out(s, host_out, s ? s->tl_tab : NULL, sizeof(seeqdev_tally_t), s ? s->tl_n : 0, first, n);
}

extern "C" int seeqdevScanLastTallyMs(const seeqdev_scan_t *s, float *ms)
{
   if (!s || !ms) { errno = EINVAL; return -1; }
   *ms = s->tm_tl.ms;
   return 0;
}

extern "C" int seeqdevTallyKey(const char *seq, size_t len, uint64_t *key)
{
   if ((!seq && len) || !key) { errno = EINVAL; return -1; }
   const uint64_t k = len <= SEEQ_TALLY_LEN_MAX ? tally_key_of((const uint8_t *)seq, (uint32_t)len) : 0u;
   if (!k) { errno = EINVAL; return -1; }                  /* long or foreign */
   *key = k;
   return 0;
}

extern "C" int seeqdevTallyDecode(uint64_t key, char out[32])
{
   if (!out) { errno = EINVAL; return -1; }
   const int len = tally_decode(key, out);
   if (len < 0) errno = EINVAL;
   return len;
}

#endif
