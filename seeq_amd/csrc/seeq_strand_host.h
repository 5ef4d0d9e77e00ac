/*
 * seeq_strand_host.h -- the host driver of the both-strands search (rule and kernels: seeq_strand.h): the pattern's reverse-complement
 * twin, one walk for the pair {P, rc(P)} (multi_one_pass) or two scans with the first one's records kept aside, the merge on the device,
 * and the seeqdevScan*Strands entries.  Included by seeq_device.hip behind seeq_demux_host.h.
 */
#ifndef SEEQ_STRAND_HOST_H_
#define SEEQ_STRAND_HOST_H_

/* A new pattern on pat's device: its reverse complement at the same distance. */
static seeqdev_pattern *strand_revcomp_new(const seeqdev_pattern *pat)
{
   if (!pat->keys) { errno = EINVAL; return NULL; }
   char *rk = (char *)malloc((size_t)pat->wlen);
   if (!rk) { errno = ENOMEM; return NULL; }
   strand_rc_keys(pat->keys, pat->wlen, rk);
   seeqdev_pattern *t = use_device(pat->device) ? NULL : seeqdevPatternNew(rk, pat->wlen, pat->tau);
   free(rk);
   return t;
}

extern "C" seeqdev_pattern_t *seeqdevPatternRevComp(const seeqdev_pattern_t *pat)
{
   seeqerr = 0;
   if (!pat) { errno = EINVAL; return NULL; }
   return strand_revcomp_new(pat);
}

/* The twin of a pattern is built on first use, once, under the pattern's lock (scan contexts on several threads may share a
   pattern); it lives in the handle and goes with it (seeqdevPatternFree). */
static const seeqdev_pattern *pattern_twin(const seeqdev_pattern *pat)
{
   seeqdev_pattern *p = (seeqdev_pattern *)pat;
   pthread_mutex_lock(&p->plan_lock);
   if (!p->twin) p->twin = strand_revcomp_new(p);
   const seeqdev_pattern *t = p->twin;
   pthread_mutex_unlock(&p->plan_lock);
   return t;
}

/* the reduction's per-tile sums for n merged records (seeq_strand.h: kept, opened, minus per tile) */
static size_t strand_bsum_words(size_t n) { return 3 * (n / SEEQ_TILE + 2); }

/* Room for n merged records.  Nothing on the stream reads the old blocks: every strands call ends synchronised. */
static int strands_ws_merged(seeqdev_scan *s, size_t n)
{
   if (n < 1) n = 1;
   if (ws_make(&s->ws, {{s->d_stcnt, sizeof(StrandCnt)}, {s->h_stcnt, sizeof(StrandCnt), WS_PINNED}})) return -1;
   return ws_grow(&s->ws, &s->cap_st_mrg, n, {{s->st_mrg, n * sizeof(uint4)}, {s->st_mrg_off, n * sizeof(uint64_t)},
                                              {s->st_bsum, strand_bsum_words(n) * sizeof(uint32_t)}});
}

/* The two sorted inputs of a merge, where the scans left them. */
struct StrandSrc {
   const seeqdev_hit_t *a, *b;
   const uint64_t *a_off, *b_off;
   uint64_t na, nb;
   seeqdev_counts_t plus;             /* the plus scan's counts: nlines, nheaders */
};

/* Two scans: the plus records (with their offsets) are copied aside on the device (side_keep) before the twin's scan overwrites them. */
static int strands_two_scans(seeqdev_scan_t *s, const seeqdev_pattern_t *pat, const seeqdev_pattern_t *twin, const void *d_text, size_t nbytes,
                             int opts, StrandSrc *src)
{
   seeqdev_counts_t cb;
   if (seeqdevScanRun(s, pat, d_text, nbytes, opts, SEEQDEV_WANT_RECORDS)) return -1;
   if (seeqdevScanFetch(s, &src->plus)) return -1;
   src->na = src->plus.nrecords;
   if (src->na > 0xFFFFFFFFull) { errno = E2BIG; return -1; }
   if (side_keep(s, (size_t)src->na)) return -1;
   if (seeqdevScanRun(s, twin, d_text, nbytes, opts, SEEQDEV_WANT_RECORDS)) return -1;
   if (seeqdevScanFetch(s, &cb)) return -1;
   if (cb.nlines != src->plus.nlines) {
      snprintf(g_last_error, sizeof g_last_error, "both strands: the twin counted %llu lines, the pattern %llu", (unsigned long long)cb.nlines,
               (unsigned long long)src->plus.nlines);
      errno = EIO;
      return -1;
   }
   src->nb = cb.nrecords;
   src->a = s->side_rec; src->a_off = s->side_off;
   src->b = s->records; src->b_off = s->rec_off;
   return 0;
}

/* The reduction of seeq_strand.h over the first n records of `rec` (kept, lines opened, minus records) -> h_stcnt; waits. */
static int strands_tally(seeqdev_scan *s, StrandArgs &a, const void *rec, uint32_t n)
{
   const hipStream_t st = s->stream;
   a.mrg = (uint4 *)rec;
   a.n = n;
   a.nt = (uint32_t)seeq_tiles_of(n);
   if (strand_bsum_words(s->cap_st_mrg) < 3 * (size_t)a.nt) {
      snprintf(g_last_error, sizeof g_last_error, "both strands: %u records, tile sums for %zu", n, s->cap_st_mrg);
      errno = EIO;
      return -1;
   }
   hipLaunchKernelGGL(k_strand_reduce, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_strand_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
   if (counters_fetch(s, s->h_stcnt, s->d_stcnt, sizeof(StrandCnt))) return -1;
   const StrandCnt &h = *s->h_stcnt;
   if (h.bad || h.kept > n || h.opened > h.kept || h.minus > h.kept) {
      snprintf(g_last_error, sizeof g_last_error, "internal inconsistency in the strand merge (flags %u, %u of %u kept, %u lines, %u minus)", h.bad, h.kept, n,
               h.opened, h.minus);
      errno = EIO;
      return -1;
   }
   return 0;
}

/* Merge the two inputs by the rule of seeq_strand.h; the result becomes the context's records (s->records / s->rec_off, s->counts):
   mode SQ_ALL every record of both, SQ_BEST / SQ_FIRST the winner of every line.  fastq: the merged records go once through the
   filter of seeq_fastq.h.  want: what the caller asked for (the count wants report no records). */
static int strands_merge(seeqdev_scan *s, const StrandSrc &src, int mode, bool fastq, int want, uint64_t per_strand[2])
{
   const hipStream_t st = s->stream;
   const uint64_t n64 = src.na + src.nb;
   if (src.na > 0xFFFFFFFFull || src.nb > 0xFFFFFFFFull || n64 > 0xFFFFFFFFull) {
      snprintf(g_last_error, sizeof g_last_error, "both strands: more than 2^32 - 1 records to merge");
      errno = E2BIG;
      return -1;
   }
   const uint32_t n = (uint32_t)n64;
   uint32_t kept = 0, opened = 0, minus = 0;
   s->tm_st.ms = 0.f;
   if (n) {
      if (strands_ws_merged(s, n)) return -1;
      StrandArgs a;
      memset(&a, 0, sizeof a);
      a.a = (const uint4 *)src.a; a.a_off = src.a_off; a.na = (uint32_t)src.na;
      a.b = (const uint4 *)src.b; a.b_off = src.b_off; a.nb = (uint32_t)src.nb;
      a.mrg = s->st_mrg; a.mrg_off = s->st_mrg_off;
      a.n = n; a.cap_mrg = cap_u32(s->cap_st_mrg);
      a.nt = (uint32_t)seeq_tiles_of(n);
      a.bsum = s->st_bsum;
      a.cnt = s->d_stcnt;
      a.mode = mode;
      if (s->tm_st.begin(s->prof, st)) return -1;
      HIP_TRY(hipMemsetAsync(s->d_stcnt, 0, sizeof(StrandCnt), st), EIO);
      hipLaunchKernelGGL(k_strand_merge, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
      if (strands_tally(s, a, s->st_mrg, n)) return -1;      /* (waits: the inputs are read, the record workspace may go) */
      kept = s->h_stcnt->kept;
      /* the result goes to the record workspace, which the inputs have left by now */
      if (reserve_impl(s, 0, 0, 0, kept)) return -1;
      if (kept && mode == SQ_ALL) {
         HIP_TRY(hipMemcpyAsync(s->records, s->st_mrg, (size_t)kept * sizeof(uint4), hipMemcpyDeviceToDevice, st), EIO);
         HIP_TRY(hipMemcpyAsync(s->rec_off, s->st_mrg_off, (size_t)kept * sizeof(uint64_t), hipMemcpyDeviceToDevice, st), EIO);
      } else if (kept) {
         a.out = (uint4 *)s->records; a.off_out = s->rec_off;
         a.cap_out = cap_u32(s->cap_records);
         hipLaunchKernelGGL(k_strand_apply, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
         if (counters_copy(s, s->h_stcnt, s->d_stcnt, sizeof(StrandCnt))) return -1;
      }
      if (s->tm_st.end(s->prof, st)) return -1;
      HIP_TRY(hipStreamSynchronize(st), EIO);
      s->tm_st.read(s->prof);
      if (s->h_stcnt->bad) {
         snprintf(g_last_error, sizeof g_last_error, "internal inconsistency in the strand merge (an index outside the output)");
         errno = EIO;
         return -1;
      }
      if (fastq && kept) {
         /* as fastq_finish: the filtered arrays become the context's records; then the tallies of what is left */
         FastqCnt f;
         if (fastq_filter_swap(s, kept, &f)) return -1;
         kept = f.kept;
         if (kept) {
            HIP_TRY(hipMemsetAsync(s->d_stcnt, 0, sizeof(StrandCnt), st), EIO);
            if (strands_tally(s, a, s->records, kept)) return -1;
            if (s->h_stcnt->kept != kept) {
               snprintf(g_last_error, sizeof g_last_error, "both strands: %u records left by the FASTQ filter, %u counted", kept, s->h_stcnt->kept);
               errno = EIO;
               return -1;
            }
         } else {
            memset(s->h_stcnt, 0, sizeof(StrandCnt));
         }
      }
      opened = s->h_stcnt->opened; minus = s->h_stcnt->minus;
   }
   scan_forget(s);                                         /* (seeqdevScanFetch has nothing to fetch: the call is complete) */
   s->counts.nlines = fastq ? fastq_nlines(src.plus.nlines) : src.plus.nlines;
   s->counts.nheaders = fastq ? 0 : src.plus.nheaders;
   s->counts.nmatchlines = opened;
   s->counts.nhits = kept;
   s->counts.nrecords = want == SEEQDEV_WANT_RECORDS ? kept : 0;
   if (per_strand) { per_strand[0] = kept - minus; per_strand[1] = minus; }
   return 0;
}

static int strands_args_ok(const seeqdev_scan_t *s, const seeqdev_pattern_t *pat, const void *text, size_t nbytes, int options, int want,
                           const seeqdev_counts_t *counts)
{
   if (!s || !pat || !counts || (!text && nbytes)) return 0;
   if (options & (SEEQDEV_SINGLELINE | MASK_INPUT)) return 0;
   return scan_args_ok(s, &pat, 1, options, want);
}

extern "C" int seeqdevScanRunStrands(seeqdev_scan_t *s, const seeqdev_pattern_t *pat, const void *d_text, size_t nbytes, int options, int want,
                                     seeqdev_counts_t *counts, uint64_t per_strand[2])
{
   seeqerr = 0;
   if (!strands_args_ok(s, pat, d_text, nbytes, options, want, counts)) { errno = EINVAL; return -1; }
   if (use_device(s->device)) return -1;
   const seeqdev_pattern_t *twin = pattern_twin(pat);
   if (!twin) return -1;
   const bool fastq = (options & SEEQDEV_FASTQ) != 0;
   /* the scans run unflagged and for records: the count wants have nothing to merge (as under SEEQDEV_FASTQ: one record per matching
      line, or every hit) */
   int opts = options & ~SEEQDEV_FASTQ;
   if (want == SEEQDEV_WANT_COUNTLINES) opts = (opts & ~MASK_MATCH) | SQ_FIRST;
   else if (want == SEEQDEV_WANT_COUNTMATCH) opts = (opts & ~MASK_MATCH) | SQ_ALL;
   int mode = opts & MASK_MATCH;
   if (mode == SQ_COUNT) mode = SQ_FIRST;                  /* (a scan for records treats SQ_COUNT as SQ_FIRST) */
   if (fastq) s->fq_ws = true;                             /* (the filter's scratch follows the record workspace from now on) */
   s->multi_n = 0;                                         /* (no multi results on the host: seeqdevScanMultiRecords refuses) */
   s->multi_nrec = 0;
   s->last_multi = 0;
   StrandSrc src;
   memset(&src, 0, sizeof src);
   const seeqdev_pattern_t *pair[2] = {pat, twin};
   /* one walk for barcode-sized patterns -- 8 .. 12 positions at distance <= 1, what the union walk was built and measured for (seeq_multi.h);
      a longer pattern has a selective automaton of its own, and two scans by its fastest kernel read the text twice but verify far fewer candidates
      than a union of two prefixes */
   const bool barcode = pat->wlen >= 8 && pat->wlen <= 12 && pat->tau <= 1;
   int rc = barcode ? multi_one_pass(s, pair, 2, d_text, nbytes, opts, SEEQDEV_WANT_RECORDS, nullptr, false, true) : 1;
   if (rc == 0) {
      /* one walk: each pattern's records and offsets lie in their region of the record workspace */
      const uint64_t capR = s->cap_records / 2;
      src.plus = counts_of(s->h_mcnt[0]);
      src.na = s->h_mcnt[0].records; src.nb = s->h_mcnt[1].records;
      src.a = s->records; src.a_off = s->rec_off;
      src.b = s->records + capR; src.b_off = s->rec_off + capR;
   } else if (rc == 1) {
      rc = strands_two_scans(s, pat, twin, d_text, nbytes, opts, &src);
   }
   if (rc == 0) rc = strands_merge(s, src, mode, fastq, want, per_strand);
   if (rc) { scan_forget(s); return -1; }
   *counts = s->counts;
   return 0;
}

extern "C" int seeqdevScanLastStrandsMs(const seeqdev_scan_t *s, float *merge_ms)
{
   if (!s || !merge_ms) { errno = EINVAL; return -1; }
   *merge_ms = s->tm_st.ms;
   return 0;
}

extern "C" int seeqdevScanHostStrands(seeqdev_scan_t *s, const seeqdev_pattern_t *pat, const char *host_text, size_t nbytes, int options, int want,
                                      seeqdev_counts_t *counts, uint64_t per_strand[2])
{
   seeqerr = 0;
   if (!strands_args_ok(s, pat, host_text, nbytes, options, want, counts)) { errno = EINVAL; return -1; }
   if (use_device(s->device)) return -1;
   if (text_upload(s, host_text, nbytes, false)) return -1;
   return seeqdevScanRunStrands(s, pat, s->d_text, nbytes, options, want, counts, per_strand);
}

#endif
