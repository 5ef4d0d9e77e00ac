/*
 * seeq_multi_host.h -- the host drivers of several patterns over one text (kernels: seeq_multi.h): the per-pattern workspace, the post-pass
 * behind the union walk (multi_post: run_segments hands over to it), the one-walk scan with its re-runs, and the seeqdevScan*Multi* entries.
 * Included by seeq_device.hip behind its entry points (scan_setup, dispatch_run, rerun_next, text_upload) and before seeq_demux_host.h.
 */
#ifndef SEEQ_MULTI_HOST_H_
#define SEEQ_MULTI_HOST_H_

/* ========================================================================== */
/* Several patterns, one walk (seeq_multi.h)                                    */
/* ========================================================================== */
static int multi_ws_ensure(seeqdev_scan *s, int npat)
{
   Workspace *w = &s->ws;
   const size_t hl = s->cap_hitlines;
   if (ws_make(w, {{s->d_mcnt, SEEQ_MULTI_MAX * sizeof(Counters)}, {s->h_mcnt, SEEQ_MULTI_MAX * sizeof(Counters), WS_PINNED}})) return -1;
   if (ws_grow(w, &s->cap_ml, hl, {{s->ml_mask, hl * sizeof(uint32_t)}, {s->ml_first, hl * sizeof(uint32_t)}, {s->ml_last, hl * sizeof(uint32_t)}})) return -1;
   if (ws_grow(w, &s->cap_mp, hl, {{s->mp_idx, hl * sizeof(uint32_t)}, {s->mp_nh, hl * sizeof(uint32_t)}})) return -1;
   if (!s->d_mx) {
      const size_t slots = 64;                             /* segments whose argument arrays may be in flight (a run of more segments waits for the stream in between) */
      if (ws_make(w, {{s->d_mx, slots * SEEQ_MULTI_MAX * sizeof(MultiExact)}, {s->h_mx, slots * SEEQ_MULTI_MAX * sizeof(MultiExact), WS_PINNED}})) return -1;
      s->mx_slots = slots;
      s->mx_next = 0;
   }
   const size_t nbp = (hl / (size_t)npat) / SCAN_BLOCK + 2, nb = hl / MULTI_BLOCK + 2;
   if (ws_grow(w, &s->cap_m_scan_ws, (size_t)npat * nbp, {{s->m_scan_ws, (size_t)npat * nbp * sizeof(uint32_t)}})) return -1;
   return ws_grow(w, &s->cap_m_bsum, (size_t)npat * nb, {{s->m_bsum, (size_t)npat * nb * sizeof(uint32_t)}});
}

/* The part of a segment behind the union walk: `ua` = the union scan's arguments (hit list made, bounds done). */
static int multi_post(seeqdev_scan *s, const ScanPlan &plan, const ScanArgs &ua, hipStream_t st)
{
   const MultiPlan *mp = s->mplan;
   const int npat = mp->npat;
   const int options = s->options, want = s->want;
   const int match_opt = options & 3;
   const uint32_t capP = (uint32_t)(s->cap_hitlines / (size_t)npat);
   const uint64_t capR = s->cap_records / (uint64_t)npat;
   MultiArgs m;
   memset(&m, 0, sizeof m);
   m.text = ua.text; m.nbytes = ua.nbytes; m.seg_base = ua.seg_base;
   m.hit_start = s->hit_start; m.hit_line = s->hit_line; m.hit_col = s->hit_col; m.nh = s->nh;
   m.ucnt = s->d_cnt;
   m.res_next = mp->d_res_next; m.res_mask = mp->d_res_mask; m.res_states = mp->res_states;
   m.maxspan = (uint32_t)mp->maxspan;
   m.window_ok = ua.window_ok;
   m.options = options;
   /* whole patterns in the resolve automaton: its sets are exact -- counting lines needs no exact pass (as behind k_stream's complete automata) */
   const bool trust = mp->exact && want == SEEQDEV_WANT_COUNTLINES;
   m.trust = trust ? 1u : 0u;
   m.lmask = s->ml_mask; m.lfirst = s->ml_first; m.llast = s->ml_last;
   m.npat = (uint32_t)npat; m.capP = capP;
   m.p_idx = s->mp_idx;
   m.pcnt = s->d_mcnt;
   m.bsum = s->m_bsum;
   m.nb = (uint32_t)(s->cap_hitlines / MULTI_BLOCK + 2);
   {
      const size_t blocks = (s->cap_hitlines + MULTI_RESOLVE_WG - 1) / MULTI_RESOLVE_WG;
      const unsigned grid = (unsigned)(blocks < (size_t)s->ncu * 2 ? blocks : (size_t)s->ncu * 2);      /* persistent: the table is staged once per workgroup */
      HIP_TRY(hipMemsetAsync(s->ml_mask, 0, s->cap_hitlines * sizeof(uint32_t), st), EIO);      /* the lanes of a line's entries OR / MAX into them */
      HIP_TRY(hipMemsetAsync(s->ml_last, 0, s->cap_hitlines * sizeof(uint32_t), st), EIO);
      /* the automaton in LDS when it fits what a workgroup may ask for beside the kernel's static arrays (the device's limit, not a literal) */
      const size_t lds2 = (size_t)mp->res_states * 20, lds1 = (size_t)mp->res_states * 16;
      const size_t lds_room = s->lds_per_wg > 1024 ? s->lds_per_wg - 1024 : 0;
      HIP_TRY(hipGetLastError(), EIO);                       /* (an error of an EARLIER launch of this segment is a failure, not a reason for the per-pattern fall-back) */
      if (lds2 <= lds_room && lds2 <= 65536) hipLaunchKernelGGL(k_multi_resolve<2>, dim3(grid ? grid : 1), dim3(MULTI_RESOLVE_WG), lds2, st, m);
      else if (lds1 <= lds_room && lds1 <= 65536) hipLaunchKernelGGL(k_multi_resolve<1>, dim3(grid ? grid : 1), dim3(MULTI_RESOLVE_WG), lds1, st, m);
      else hipLaunchKernelGGL(k_multi_resolve<0>, dim3(grid ? grid : 1), dim3(MULTI_RESOLVE_WG), 0, st, m);
      {
         const hipError_t le = hipGetLastError();            /* this launch refused for its resources: a scan per pattern (seeqdevScanRunMulti); anything else fails */
         if (le == hipErrorInvalidValue || le == hipErrorLaunchOutOfResources || le == hipErrorInvalidConfiguration) return 1;
         if (le != hipSuccess) return hip_fail(le, "k_multi_resolve", EIO);
      }
      hipLaunchKernelGGL(k_multi_reduce, dim3(m.nb), dim3(256), 0, st, m);
      hipLaunchKernelGGL(k_multi_top, dim3((unsigned)npat), dim3(256), 0, st, m);
      if (trust) { HIP_TRY(hipGetLastError(), EIO); return 0; }
      hipLaunchKernelGGL(k_multi_apply, dim3(m.nb), dim3(256), 0, st, m);
   }
   /* The exact pass, every pattern in one launch per step (blockIdx.y = pattern; one-word patterns first, then the two-word
      ones): the patterns' arguments go to HBM through a page-locked ring, one slot per segment. */
   const unsigned grid_hits = capped_grid(s, capP, 4);      /* (x npat workgroups per launch) */
   if (s->mx_next == s->mx_slots) { HIP_TRY(hipStreamSynchronize(st), EIO); s->mx_next = 0; }
   MultiExact *hx = s->h_mx + s->mx_next * SEEQ_MULTI_MAX, *dx = s->d_mx + s->mx_next * SEEQ_MULTI_MAX;
   s->mx_next++;
   const uint32_t nbp = (uint32_t)((size_t)capP / SCAN_BLOCK + 2);
   int order[SEEQ_MULTI_MAX], n1 = 0, n2 = 0;
   for (int k = 0; k < npat; k++) if (mp->fw[k] == 1) order[n1++] = k;
   for (int k = 0; k < npat; k++) if (mp->fw[k] != 1) order[n1 + n2++] = k;
   for (int q = 0; q < npat; q++) {
      const int k = order[q];
      MultiExact &x = hx[q];
      ScanArgs &a = x.a;
      a = ua;
      a.m = mp->m[k]; a.tau = mp->tau[k];
      a.hit_start = s->hit_start; a.hit_line = s->hit_line; a.cap_hitlines = capP;      /* the union's lines, through this pattern's index list */
      a.hit_idx = s->mp_idx + (size_t)k * capP;
      a.nh = s->mp_nh + (size_t)k * capP;
      a.records = s->records + (uint64_t)k * capR; a.cap_records = capR; a.rec_off = s->rec_off + (uint64_t)k * capR;
      a.use_nh = 3u; a.filter = 1u;
      a.skip_back = (uint32_t)mp->maxspan;
      a.hit_last = s->ml_last;
      a.window_ok = 1u;
      a.tile_dirty = nullptr; a.tile_dmask = nullptr; a.stream_ntiles = 0; a.stream_ch = 0;
      a.cnt = s->d_mcnt + k;
      x.eq = mp->d_eq + (size_t)k * 1536;
      x.hcol = s->ml_first;
      x.cache = want == SEEQDEV_WANT_RECORDS ? s->ow.tmp + (size_t)k * capP : nullptr;
      x.scan_ws = s->m_scan_ws + (size_t)k * nbp;
      x.nb = nbp;
      x.seg_end_flags = seg_end_flags(plan.need_nh, plan.superset, plan.nh_is_count);
   }
   HIP_TRY(hipMemcpyAsync(dx, hx, (size_t)npat * sizeof(MultiExact), hipMemcpyHostToDevice, st), EIO);
   const int mo = match_opt == SQ_COUNT ? SQ_FIRST : match_opt;
   if (n1) hipLaunchKernelGGL((k_exact1m<SQ_MODE_COUNT, 1, -1>), dim3(grid_hits, (unsigned)n1), dim3(WG), 0, st, (const MultiExact *)dx);
   if (n2) hipLaunchKernelGGL((k_exact1m<SQ_MODE_COUNT, 2, -1>), dim3(grid_hits, (unsigned)n2), dim3(WG), 0, st, (const MultiExact *)(dx + n1));
   if (plan.nh_is_count) hipLaunchKernelGGL(k_multi_count_nonzero, dim3(grid_hits < 128 ? grid_hits : 128, (unsigned)npat), dim3(WG), 0, st, (const MultiExact *)dx);
   hipLaunchKernelGGL(k_multi_scan_reduce, dim3(nbp, (unsigned)npat), dim3(WG), 0, st, (const MultiExact *)dx);
   hipLaunchKernelGGL(k_multi_scan_top, dim3((unsigned)npat), dim3(WG), 0, st, (const MultiExact *)dx, want == SEEQDEV_WANT_RECORDS ? 1 : 0);
   hipLaunchKernelGGL(k_multi_scan_apply, dim3(nbp, (unsigned)npat), dim3(WG), 0, st, (const MultiExact *)dx);
   if (want == SEEQDEV_WANT_RECORDS) {
      if (mo == SQ_BEST) {
         if (n1) hipLaunchKernelGGL((k_exact1m<SQ_MODE_EMIT, 1, SQ_BEST>), dim3(grid_hits, (unsigned)n1), dim3(WG), 0, st, (const MultiExact *)dx);
         if (n2) hipLaunchKernelGGL((k_exact1m<SQ_MODE_EMIT, 2, SQ_BEST>), dim3(grid_hits, (unsigned)n2), dim3(WG), 0, st, (const MultiExact *)(dx + n1));
      } else {
         if (n1) hipLaunchKernelGGL((k_exact1m<SQ_MODE_EMIT, 1, -1>), dim3(grid_hits, (unsigned)n1), dim3(WG), 0, st, (const MultiExact *)dx);
         if (n2) hipLaunchKernelGGL((k_exact1m<SQ_MODE_EMIT, 2, -1>), dim3(grid_hits, (unsigned)n2), dim3(WG), 0, st, (const MultiExact *)(dx + n1));
      }
   }
   hipLaunchKernelGGL(k_multi_seg_end, dim3((unsigned)npat), dim3(1), 0, st, (const MultiExact *)dx);
   HIP_TRY(hipGetLastError(), EIO);
   return 0;
}

/* ========================================================================== */
/* Several patterns, one text (barcode demultiplexing: reference doc/response.tex:358-360)  */
/* ========================================================================== */
/* Several patterns over one text.  ONE walk for all of them when the set has a union automaton and the text is k_pair's
 * (read-length lines, SQ_FAIL / SQ_CONVERT; seeq_multi.h) -- else, and under SEEQ_MULTI=sequential, a scan per pattern over
 * the resident text, back to back on the context's stream.  Per pattern: counts, and for SEEQDEV_WANT_RECORDS its ordered
 * records, kept on the host until the next multi scan.  Either way the results are those of a scan of each pattern alone. */
static int multi_grow_host(seeqdev_scan_t *s, size_t n)
{
   if (s->multi_nrec + n <= s->cap_multi_rec) return 0;
   /* page-locked: the records of a barcode set are hundreds of MB, and a pageable copy runs at a fifth of the link */
   const size_t cap = (s->multi_nrec + n) + ((s->multi_nrec + n) >> 1) + 1024;
   return ws_grow_keep(&s->ws, &s->cap_multi_rec, cap, {s->multi_rec, cap * sizeof(seeqdev_hit_t), WS_PINNED}, s->multi_nrec * sizeof(seeqdev_hit_t));
}

/* Pattern k of a multi scan: its counts, and its n records -- at d_rec on the device -- appended to the host results (the copy is left on the
   context's stream); multi_gather_end closes the set of npat patterns. */
static int multi_gather(seeqdev_scan_t *s, int k, const seeqdev_counts_t &c, const seeqdev_hit_t *d_rec, size_t n, seeqdev_counts_t *counts)
{
   s->multi_cnt[k] = c;
   s->multi_first[k] = s->multi_nrec;
   if (n) {
      if (multi_grow_host(s, n)) return -1;
      HIP_TRY(hipMemcpyAsync(s->multi_rec + s->multi_nrec, d_rec, n * sizeof(seeqdev_hit_t), hipMemcpyDeviceToHost, s->stream), EIO);
      s->multi_nrec += n;
   }
   if (counts) counts[k] = c;
   return 0;
}

static void multi_gather_end(seeqdev_scan_t *s, int npat) { s->multi_first[npat] = s->multi_nrec; s->multi_n = npat; }

static int demux_one_walk(seeqdev_scan_t *s, int npat, uint64_t capR);

/* 0: done; 1: not for this set / text / options (the caller scans pattern by pattern); -1: error.  demux: the records stay on
   the device and are demultiplexed there (seeqdevScanRunDemux) instead of going to the host.  stay: the records stay on the device,
   in their regions of the record workspace, and that is all (seeqdevScanRunStrands merges them there). */
static int multi_one_pass(seeqdev_scan_t *s, const seeqdev_pattern_t *const *pats, int npat, const void *d_text, size_t nbytes,
                          int options, int want, seeqdev_counts_t *counts, bool demux = false, bool stay = false)
{
   const char *env = getenv("SEEQ_MULTI");
   if (env && !strcmp(env, "sequential")) return 1;
   if (npat < 2 || npat > SEEQ_MULTI_MAX || nbytes == 0) return 1;
   const int nd = options & MASK_NONDNA;
   if ((options & (MASK_INPUT | SEEQDEV_SINGLELINE)) || !(nd == SQ_FAIL || nd == SQ_CONVERT)) return 1;
   for (int k = 0; k < npat; k++) if (!pats[k] || pats[k]->device != s->device) return 1;
   if (use_device(s->device)) return -1;
   MultiPlan *mp = multi_plan_for(&s->mplan, pats, npat);
   if (!mp) { errno = ENOMEM; return -1; }
   if (mp->state != 1) return 1;
   /* the patterns' EQ tables of the exact pass (as run_segments makes the one of a single pattern) */
   if (mp->eq_options != options) {
      uint32_t *h = (uint32_t *)calloc((size_t)npat * 1536, sizeof(uint32_t));
      if (!h) { errno = ENOMEM; return -1; }
      for (int k = 0; k < npat; k++) eq_fill(h + (size_t)k * 1536, pats[k], options, mp->fw[k]);
      const hipError_t e = hipMemcpy(mp->d_eq, h, (size_t)npat * 1536 * sizeof(uint32_t), hipMemcpyHostToDevice);
      free(h);
      if (e != hipSuccess) return hip_fail(e, "hipMemcpy(EQ tables)", EIO);
      mp->eq_options = options;
   }
   if (scan_setup(s, &mp->upat, d_text, nbytes, options, want, SEEQ_HL_DIV_MULTI)) return -1;
   s->multi_active = true;
   int rc = -1;
   for (int run = 0;; run++) {
      if (multi_ws_ensure(s, npat)) break;
      if (hipMemsetAsync(s->d_mcnt, 0, SEEQ_MULTI_MAX * sizeof(Counters), s->stream) != hipSuccess) { errno = EIO; break; }
      const int r = dispatch_run(s);
      if (r == -2) { rc = 1; break; }
      if (r) break;
      if (hipMemcpyAsync(s->h_mcnt, s->d_mcnt, (size_t)npat * sizeof(Counters), hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
          hipStreamSynchronize(s->stream) != hipSuccess) { errno = EIO; break; }
      const int next = rerun_next(s, run, *s->h_cnt, s->h_mcnt, npat);
      if (next == 1) continue;
      s->last_runs = run + 1;
      if (next == 2) rc = 1;                               /* not k_pair's text after all: a scan per pattern */
      if (next == 0) {
         /* results: counts, then every pattern's records from its region */
         const uint64_t capR = s->cap_records / (uint64_t)npat;
         if (demux) {
            rc = demux_one_walk(s, npat, capR) ? -1 : 0;
            if (rc == 0) s->last_multi = 1;
            break;
         }
         if (stay) { rc = 0; s->last_multi = 1; break; }
         s->multi_nrec = 0;
         rc = 0;
         if (want == SEEQDEV_WANT_RECORDS) {
            size_t total = 0;
            for (int k = 0; k < npat; k++) total += (size_t)s->h_mcnt[k].records;
            if (multi_grow_host(s, total)) { rc = -1; break; }
         }
         for (int k = 0; k < npat && rc == 0; k++) {
            const Counters &h = s->h_mcnt[k];
            rc = multi_gather(s, k, counts_of(h), s->records + (uint64_t)k * capR, want == SEEQDEV_WANT_RECORDS ? (size_t)h.records : 0, counts);
         }
         if (rc == 0 && hipStreamSynchronize(s->stream) != hipSuccess) { errno = EIO; rc = -1; }
         if (rc == 0) { multi_gather_end(s, npat); s->last_multi = 1; }
      }
      break;
   }
   s->multi_active = false;
   s->ran = false;                                         /* (seeqdevScanFetch has nothing to fetch: the multi scan is complete) */
   return rc;
}

extern "C" int seeqdevScanRunMulti(seeqdev_scan_t *s, const seeqdev_pattern_t *const *pats, int npat, const void *d_text, size_t nbytes,
                                   int options, int want, seeqdev_counts_t *counts)
{
   seeqerr = 0;
   if (!scan_args_ok(s, pats, npat, options, want) || (!d_text && nbytes) || (options & SEEQDEV_FASTQ)) { errno = EINVAL; return -1; }
   if (npat > s->cap_multi_n) {
      seeqdev_counts_t *c = (seeqdev_counts_t *)realloc(s->multi_cnt, (size_t)npat * sizeof *c);
      if (c) s->multi_cnt = c;
      size_t *f = (size_t *)realloc(s->multi_first, ((size_t)npat + 1) * sizeof *f);
      if (f) s->multi_first = f;
      if (!c || !f) { errno = ENOMEM; return -1; }
      s->cap_multi_n = npat;
   }
   s->multi_n = 0;
   s->multi_nrec = 0;
   s->last_multi = 0;
   {
      const int r = multi_one_pass(s, pats, npat, d_text, nbytes, options, want, counts);
      if (r <= 0) return r;
   }
   s->multi_nrec = 0;
   for (int k = 0; k < npat; k++) {
      seeqdev_counts_t c;
      if (seeqdevScanRun(s, pats[k], d_text, nbytes, options, want)) return -1;
      if (seeqdevScanFetch(s, &c)) return -1;
      if (multi_gather(s, k, c, s->records, want == SEEQDEV_WANT_RECORDS ? (size_t)c.nrecords : 0, counts)) return -1;
      HIP_TRY(hipStreamSynchronize(s->stream), EIO);         /* the next scan overwrites the records */
   }
   multi_gather_end(s, npat);
   return 0;
}

/* 1: the last multi scan walked the text once for all its patterns; 0: a scan per pattern. */
extern "C" int seeqdevScanLastMulti(const seeqdev_scan_t *s) { return s ? s->last_multi : 0; }

extern "C" int seeqdevScanHostMulti(seeqdev_scan_t *s, const seeqdev_pattern_t *const *pats, int npat, const char *host_text, size_t nbytes,
                                    int options, int want, seeqdev_counts_t *counts)
{
   seeqerr = 0;
   if (!s || !pats || npat < 1 || (!host_text && nbytes) || (options & SEEQDEV_FASTQ)) { errno = EINVAL; return -1; }
   if (use_device(s->device)) return -1;
   if (text_upload(s, host_text, nbytes, false)) return -1;      /* once, for all patterns */
   return seeqdevScanRunMulti(s, pats, npat, s->d_text, nbytes, options, want, counts);
}

extern "C" int seeqdevScanMultiRecords(const seeqdev_scan_t *s, int k, const seeqdev_hit_t **rec, size_t *nrec)
{
   if (!s || !rec || !nrec || k < 0 || k >= s->multi_n) { errno = EINVAL; return -1; }
   *rec = s->multi_rec + s->multi_first[k];
   *nrec = s->multi_first[k + 1] - s->multi_first[k];
   return 0;
}

#endif
