/*
 * seeq_demux_host.h -- the host driver of the demultiplexer (kernels: seeq_demux.h): per line the best pattern of a set, from one walk
 * (multi_one_pass) or from a scan per pattern folded on the device.  Included by seeq_device.hip behind seeq_multi_host.h.
 */
#ifndef SEEQ_DEMUX_HOST_H_
#define SEEQ_DEMUX_HOST_H_

/* ========================================================================== */
/* Demultiplexing: per line the best pattern of a set, on the device (seeq_demux.h)  */
/* ========================================================================== */
/* Per-line workspace for nkeys lines (8 bytes per line; allocated by the first demux of a context), keys cleared. */
static int demux_ws_lines(seeqdev_scan *s, size_t nkeys)
{
   if (ws_make(&s->ws, {{s->d_dmcnt, sizeof(DemuxCnt)}, {s->h_dmcnt, sizeof(DemuxCnt), WS_PINNED}})) return -1;
   if (ws_grow(&s->ws, &s->cap_dm_lines, nkeys, {{s->dm_key, nkeys * sizeof(uint32_t)}, {s->dm_aux, nkeys * sizeof(uint32_t)}})) return -1;
   if (ensure_scan_ws(s, nkeys / SCAN_BLOCK + 2)) return -1;      /* block sums of the rank scan: the context's scan workspace */
   if (nkeys) HIP_TRY(hipMemsetAsync(s->dm_key, 0, nkeys * sizeof(uint32_t), s->stream), EIO);
   HIP_TRY(hipMemsetAsync(s->d_dmcnt, 0, sizeof(DemuxCnt), s->stream), EIO);
   return 0;
}

/* Room for n output records; the first `keep` of the old area are carried over (the staging area of a scan per pattern grows). */
static int demux_ws_out(seeqdev_scan *s, size_t n, size_t keep)
{
   if (n < 1) n = 1;
   if (keep > s->cap_dm_out) keep = s->cap_dm_out;
   return ws_grow_keep(&s->ws, &s->cap_dm_out, n, {s->dm_out, n * sizeof(uint4)}, keep * sizeof(uint4));
}

static void demux_fold(seeqdev_scan *s, const seeqdev_hit_t *rec, size_t n, int k, bool stage, uint32_t nkeys)
{
   const unsigned grid = (unsigned)((n + DEMUX_WG - 1) / DEMUX_WG);
   if (stage)
      hipLaunchKernelGGL(k_demux_fold<true>, dim3(grid), dim3(DEMUX_WG), 0, s->stream, (const uint4 *)rec, (uint32_t)n, (uint32_t)k, s->dm_key,
                         s->dm_aux, nkeys, s->dm_out, (uint32_t)s->cap_dm_out, s->d_dmcnt);
   else
      hipLaunchKernelGGL(k_demux_fold<false>, dim3(grid), dim3(DEMUX_WG), 0, s->stream, (const uint4 *)rec, (uint32_t)n, (uint32_t)k, s->dm_key,
                         s->dm_aux, nkeys, s->dm_out, (uint32_t)s->cap_dm_out, s->d_dmcnt);
}

/* After the folds: counts, ranks, the records in line order (src: the one walk's records; NULL: the staging area of a scan per
   pattern), the counters to the host. */
static int demux_finish(seeqdev_scan *s, uint32_t nkeys, int npat, const DemuxSrc *src, uint32_t nmax)
{
   const hipStream_t st = s->stream;
   const bool stage = src == NULL;
   if (nkeys) {
      unsigned grid = (unsigned)((nkeys + DEMUX_WG * 8 - 1) / (DEMUX_WG * 8));
      if (grid > (unsigned)s->ncu * 8) grid = (unsigned)s->ncu * 8;
      if (stage) {
         hipLaunchKernelGGL(k_demux_tally<true>, dim3(grid), dim3(DEMUX_WG), 0, st, (const uint32_t *)s->dm_key, (const uint32_t *)s->dm_aux, nkeys,
                            s->dm_out, (uint32_t)s->cap_dm_out, s->d_dmcnt);
         /* ranks in place of the keys; the records go to the record workspace (free: the last scan's records are folded) */
         launch_scan<2>(st, s->scan_ws, s->dm_key, s->dm_key, nkeys, nullptr, nkeys, 0, &s->d_dmcnt->nassigned);
         if (s->cap_records < s->cap_dm_out) {
            HIP_TRY(hipStreamSynchronize(st), EIO);
            if (reserve_impl(s, 0, 0, 0, s->cap_dm_out)) return -1;
         }
         hipLaunchKernelGGL(k_demux_scatter, dim3(grid), dim3(DEMUX_WG), 0, st, (const uint4 *)s->dm_out, (uint32_t)s->cap_dm_out,
                            (const uint32_t *)s->dm_key, nkeys, (uint4 *)s->records, (uint32_t)s->cap_records, s->d_dmcnt);
      } else {
         hipLaunchKernelGGL(k_demux_tally<false>, dim3(grid), dim3(DEMUX_WG), 0, st, (const uint32_t *)s->dm_key, (const uint32_t *)s->dm_aux, nkeys,
                            s->dm_out, (uint32_t)s->cap_dm_out, s->d_dmcnt);
         launch_scan<2>(st, s->scan_ws, s->dm_key, s->dm_aux, nkeys, nullptr, nkeys, 0, &s->d_dmcnt->nassigned);
         if (nmax)
            hipLaunchKernelGGL(k_demux_emit, dim3((nmax + DEMUX_WG - 1) / DEMUX_WG, (unsigned)npat), dim3(DEMUX_WG), 0, st, *src,
                               (const uint32_t *)s->dm_key, (const uint32_t *)s->dm_aux, nkeys, s->dm_out, (uint32_t)s->cap_dm_out, s->d_dmcnt);
      }
   }
   if (counters_fetch(s, s->h_dmcnt, s->d_dmcnt, sizeof(DemuxCnt))) return -1;
   const DemuxCnt &h = *s->h_dmcnt;
   if (h.bad || h.nassigned > s->cap_dm_out || (stage && h.slot != h.nassigned)) {
      snprintf(g_last_error, sizeof g_last_error, "internal inconsistency in the demultiplexer (flags %u, %u assigned, %u staged)", h.bad, h.nassigned, h.slot);
      errno = EIO;
      return -1;
   }
   if (stage && h.nassigned) {
      HIP_TRY(hipMemcpyAsync(s->dm_out, s->records, (size_t)h.nassigned * sizeof(uint4), hipMemcpyDeviceToDevice, st), EIO);
      HIP_TRY(hipStreamSynchronize(st), EIO);
   }
   s->dm_nrec = h.nassigned;
   return 0;
}

/* The one walk is done: pattern k's h_mcnt[k].records records are at records + k * capR, in line order. */
static int demux_one_walk(seeqdev_scan_t *s, int npat, uint64_t capR)
{
   const uint64_t nl = s->h_mcnt[0].lines;
   if (nl > 0xFFFFFFFFull) { errno = E2BIG; return -1; }
   const uint32_t nkeys = (uint32_t)nl;
   s->dm_nlines = nl;
   if (demux_ws_lines(s, nkeys)) return -1;
   DemuxSrc src;
   memset(&src, 0, sizeof src);
   src.rec = (const uint4 *)s->records;
   src.stride = capR;
   size_t total = 0;
   uint32_t nmax = 0;
   for (int k = 0; k < npat; k++) {
      const uint32_t n = (uint32_t)s->h_mcnt[k].records;
      src.n[k] = n;
      total += n;
      if (n > nmax) nmax = n;
   }
   if (demux_ws_out(s, total < nkeys ? total : nkeys, 0)) return -1;
   for (int k = 0; k < npat; k++)
      if (src.n[k]) demux_fold(s, s->records + (uint64_t)k * capR, src.n[k], k, false, nkeys);
   return demux_finish(s, nkeys, npat, &src, nmax);
}

/* A scan per pattern: each pattern's records are folded on the device before the next scan overwrites them. */
static int demux_per_pattern(seeqdev_scan_t *s, const seeqdev_pattern_t *const *pats, int npat, const void *d_text, size_t nbytes, int options)
{
   uint32_t nkeys = 0;
   size_t sumrec = 0;
   for (int k = 0; k < npat; k++) {
      seeqdev_counts_t c;
      if (seeqdevScanRun(s, pats[k], d_text, nbytes, options, SEEQDEV_WANT_RECORDS)) return -1;
      if (seeqdevScanFetch(s, &c)) return -1;
      if (k == 0) {
         if (c.nlines > 0xFFFFFFFFull) { errno = E2BIG; return -1; }
         nkeys = (uint32_t)c.nlines;
         s->dm_nlines = c.nlines;
         if (demux_ws_lines(s, nkeys)) return -1;
      } else if (c.nlines != nkeys) {
         snprintf(g_last_error, sizeof g_last_error, "demultiplexer: pattern %d counted %llu lines, pattern 0 %u", k, (unsigned long long)c.nlines, nkeys);
         errno = EIO;
         return -1;
      }
      if (!c.nrecords) continue;
      const size_t staged = sumrec < nkeys ? sumrec : nkeys;       /* at most this many slots are handed out so far */
      sumrec += (size_t)c.nrecords;
      if (demux_ws_out(s, sumrec < nkeys ? sumrec : nkeys, staged)) return -1;
      demux_fold(s, s->records, (size_t)c.nrecords, k, true, nkeys);
      HIP_TRY(hipGetLastError(), EIO);
      HIP_TRY(hipStreamSynchronize(s->stream), EIO);          /* the next scan may reallocate the records the fold reads */
   }
   return demux_finish(s, nkeys, npat, nullptr, 0);
}

/* SEEQDEV_FASTQ: the demultiplexer's records (one per assigned raw line, in line order) reduced to those of the sequence lines and
   numbered by record -- the filter of seeq_fastq.h in its demux mode, whose tallies replace the counters of demux_finish.  The filter
   never writes in place: its output comes back from the scratch with one device copy (dm_out has a capacity of its own and carries its
   contents over when it grows, so it cannot be swapped with the scratch as the record arrays are). */
static int demux_fastq(seeqdev_scan *s)
{
   s->dm_nlines = fastq_nlines(s->dm_nlines);
   DemuxCnt &h = *s->h_dmcnt;
   const size_t n = s->dm_nrec;
   uint32_t kept = 0;
   memset(h.per_pat, 0, sizeof h.per_pat);
   h.ambiguous = 0;
   if (n) {
      if (n > 0xFFFFFFFFull) { errno = E2BIG; return -1; }
      if (reserve_impl(s, 0, 0, 0, n)) return -1;
      FastqCnt f;
      if (fastq_filter(s, s->dm_out, nullptr, (uint32_t)n, true, &f)) return -1;
      kept = f.kept;
      if (kept) {
         HIP_TRY(hipMemcpyAsync(s->dm_out, s->fq_rec, (size_t)kept * sizeof(uint4), hipMemcpyDeviceToDevice, s->stream), EIO);
         HIP_TRY(hipStreamSynchronize(s->stream), EIO);
      }
      for (int k = 0; k < 256; k++) h.per_pat[k] = f.per_pat[k];
      h.ambiguous = f.ambiguous;
   }
   h.nassigned = kept;
   s->dm_nrec = kept;
   return 0;
}

static int demux_args_ok(const seeqdev_scan_t *s, const seeqdev_pattern_t *const *pats, int npat, const void *text, size_t nbytes, int options,
                         const seeqdev_demux_counts_t *sum)
{
   return scan_args_ok(s, pats, npat, options, SEEQDEV_WANT_RECORDS) && npat <= SEEQ_DEMUX_MAX && !(!text && nbytes) && sum && (options & MASK_MATCH) < SQ_ALL;
}

extern "C" int seeqdevScanRunDemux(seeqdev_scan_t *s, const seeqdev_pattern_t *const *pats, int npat, const void *d_text, size_t nbytes,
                                   int options, seeqdev_demux_counts_t *sum, uint64_t *per_pattern)
{
   seeqerr = 0;
   if (!demux_args_ok(s, pats, npat, d_text, nbytes, options, sum)) { errno = EINVAL; return -1; }
   if (use_device(s->device)) return -1;
   const bool fastq = (options & SEEQDEV_FASTQ) != 0;
   const int opts = (options & ~(MASK_MATCH | SEEQDEV_FASTQ)) | SQ_BEST;      /* (the set's scans run unflagged: demux_fastq filters their result) */
   if (fastq) s->fq_ws = true;
   s->dm_nrec = 0;
   s->dm_done = false;
   s->dm_nlines = 0;
   s->multi_n = 0;                                         /* (no multi results on the host: seeqdevScanMultiRecords refuses) */
   s->multi_nrec = 0;
   s->last_multi = 0;
   int rc = multi_one_pass(s, pats, npat, d_text, nbytes, opts, SEEQDEV_WANT_RECORDS, nullptr, true);
   if (rc == 1) rc = demux_per_pattern(s, pats, npat, d_text, nbytes, opts);
   scan_forget(s);                                         /* (the patterns are the caller's) */
   if (rc == 0 && fastq) rc = demux_fastq(s);
   if (rc) { s->dm_nrec = 0; return -1; }
   s->dm_done = true;                                      /* (seeqdevScanTallyHold: the records are a result, none included) */
   const DemuxCnt &h = *s->h_dmcnt;
   sum->nlines = s->dm_nlines;
   sum->nassigned = h.nassigned;
   sum->nambiguous = h.ambiguous;
   if (per_pattern) for (int k = 0; k < npat; k++) per_pattern[k] = h.per_pat[k];
   return 0;
}

extern "C" int seeqdevScanHostDemux(seeqdev_scan_t *s, const seeqdev_pattern_t *const *pats, int npat, const char *host_text, size_t nbytes,
                                    int options, seeqdev_demux_counts_t *sum, uint64_t *per_pattern)
{
   seeqerr = 0;
   if (!demux_args_ok(s, pats, npat, host_text, nbytes, options, sum)) { errno = EINVAL; return -1; }
   if (use_device(s->device)) return -1;
   if (text_upload(s, host_text, nbytes, false)) return -1;
   return seeqdevScanRunDemux(s, pats, npat, s->d_text, nbytes, options, sum, per_pattern);
}

extern "C" const seeqdev_demux_t *seeqdevScanDemuxDevice(const seeqdev_scan_t *s) { return s ? (const seeqdev_demux_t *)s->dm_out : NULL; }

extern "C" int seeqdevScanCopyDemux(seeqdev_scan_t *s, seeqdev_demux_t *host_out, size_t first, size_t n)
{
   return copy_out(s, host_out, s ? s->dm_out : NULL, sizeof(seeqdev_demux_t), s ? s->dm_nrec : 0, first, n);
}

#endif
