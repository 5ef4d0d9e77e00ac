/*
 * seeq_tally_host.h -- the host driver of the tally of distinct spans (rule and kernels: seeq_tally.h), and what the whole tally family
 * shares on the host: the sort over a list of (word, digit) passes (tally_sort_run: the plain, the library and the grouped tally), the
 * one driver of the single-column tally with its optional step between pack and sort (tally_run, TallyStep: the library's assignment),
 * which record array a source names (tally_source) and what every entry over a record array does first (tally_enter); then the
 * seeqdevScanTally* and seeqdevTally* entries of the plain tally.  Included by seeq_device.hip behind seeq_insert_host.h.
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
                                          {s->tl_sum, (2 * nt + (size_t)tally_chunks(n) + 1) * sizeof(uint32_t)},
                                          {s->tl_stat, nt * SEEQ_TALLY_STAT * sizeof(uint32_t)}});
}

/* The sort's arguments for n items in the plain tally's scratch (tally_ws_keys): word 0 in its two key arrays, the digit matrix, the scan's
   chunk sums; the flag of a scatter in the tiles' words tstat.  A second word is the caller's to add. */
static TallySortArgs tally_sort_args(seeqdev_scan *s, uint32_t n, uint32_t *tstat)
{
   TallySortArgs a;
   memset(&a, 0, sizeof a);
   a.n = n; a.nt = (uint32_t)tally_tiles(n);
   a.src[0] = s->tl_key0; a.dst[0] = s->tl_key1;
   a.mat = s->tl_mat; a.nmat = (uint32_t)tally_matrix(n); a.nb = (uint32_t)tally_chunks(n);
   a.bsum = s->tl_sum + 2 * (size_t)a.nt;
   a.flag = tstat + SEEQ_TALLY_STAT_FLAG; a.fstride = SEEQ_TALLY_STAT;
   return a;
}

struct TallyPass { uint32_t word, digit; };                /* a pass of the sort: the word it sorts by and the 8-bit digit of it */
#define SEEQ_TALLY_PASS_MAX 16                              /* the eight digits of two words */

/* The passes of an LSD sort by word 1, then word 0: n0 digits of word 0 first, then n1 of word 1 -> list; their number. */
static uint32_t tally_pass_list(TallyPass list[SEEQ_TALLY_PASS_MAX], uint32_t n0, uint32_t n1)
{
   uint32_t np = 0;
   for (uint32_t d = 0; d < n0 && np < SEEQ_TALLY_PASS_MAX; d++) list[np++] = {0u, d};
   for (uint32_t d = 0; d < n1 && np < SEEQ_TALLY_PASS_MAX; d++) list[np++] = {1u, d};
   return np;
}

/* The stable sort of items of `words` 64-bit words by the np passes of `list`, in their order.  Five launches per pass; a pass's output is the
   next one's input, so the sorted items are in a->src when this returns and a->dst is free. */
static void tally_sort_run(hipStream_t st, TallySortArgs *a, int words, const TallyPass *list, uint32_t np)
{
   for (uint32_t p = 0; p < np; p++) {
      a->word = list[p].word; a->pass = list[p].digit;
      hipLaunchKernelGGL(words == 2 ? k_tally_pair_hist : k_tally_hist, dim3(a->nt), dim3(SEEQ_TILE_WG), 0, st, *a);
      hipLaunchKernelGGL(k_tally_scan_reduce, dim3(a->nb), dim3(SEEQ_TILE_WG), 0, st, *a);
      hipLaunchKernelGGL(k_tally_scan_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, *a);
      hipLaunchKernelGGL(k_tally_scan_apply, dim3(a->nb), dim3(SEEQ_TILE_WG), 0, st, *a);
      hipLaunchKernelGGL(words == 2 ? k_tally_pair_scatter : k_tally_scatter, dim3(a->nt), dim3(SEEQ_TILE_WG), 0, st, *a);
      for (int w = 0; w < words; w++) { uint64_t *t = a->src[w]; a->src[w] = a->dst[w]; a->dst[w] = t; }
   }
}

/* An optional step between tally_run's pack and its sort (the library's assignment: seeq_tally_library_host.h). */
struct TallyStep {
   const char *who;                   /* the prefix of the call's error texts */
   size_t      max_distinct;          /* the table can have no more entries than this */
   /* key[0 .. n) is rewritten in place, nkeyed of them nonzero; scratch: 4 bytes per span that nothing else uses until it returns.
      -> *nleft: the nonzero keys left to sort, *passes: the passes of the sort over them */
   int (*rewrite)(seeqdev_scan *s, TallyStep *step, uint64_t *key, uint32_t *scratch, uint32_t n, uint64_t nkeyed, const TallyCnt &packed, uint64_t *nleft,
                  uint32_t *passes);
   /* the text of an internal inconsistency, with the step's own numbers beside the tally's */
   int (*fail)(const TallyStep *step, const char *what, const TallyCnt &h, uint32_t n, uint64_t ntallied);
};

static int tally_fail(const TallyStep *step, const char *what, const TallyCnt &h, uint32_t n, uint64_t ntallied)
{
   if (step) return step->fail(step, what, h, n, ntallied);
   snprintf(g_last_error, sizeof g_last_error, "internal inconsistency in the tally (%s: flags %u, %u spans, %llu tallied, %u nonzero keys, %u distinct, first head %u)",
            what, h.bad, n, (unsigned long long)ntallied, h.nonzero, h.ndistinct, h.first);
   errno = EIO;
   return -1;
}

/* The table of the n spans rec / off of text[0 .. nbytes), their keys rewritten by `step` (NULL: as they are) before the sort; the context's
   table (tl_tab, tl_n) is the result.  counts->ntallied: the keys that were sorted.  Waits. */
static int tally_run(seeqdev_scan *s, const uint4 *rec, const uint64_t *off, uint32_t n, const void *d_text, size_t nbytes, seeqdev_tally_counts_t *counts,
                     TallyStep *step = NULL)
{
   const hipStream_t st = s->stream;
   const char *who = step ? step->who : "tally";
   memset(counts, 0, sizeof *counts);
   counts->nspans = n;
   if (!n) return 0;                                       /* no spans: nothing is launched */
   if (tally_ws_keys(s, n)) return -1;
   TallyArgs a;
   memset(&a, 0, sizeof a);
   a.rec = rec; a.off = off; a.n = n;
   a.nt = (uint32_t)tally_tiles(n);
   a.text = (const uint8_t *)d_text; a.nbytes = nbytes;
   a.rsum = s->tl_sum;
   a.tstat = s->tl_stat;
   a.cnt = s->d_tlcnt;
   TallySortArgs sa = tally_sort_args(s, n, s->tl_stat);
   a.src = sa.src[0]; a.dst = sa.dst[0];
   if ((size_t)n > s->cap_tl || tally_tiles(s->cap_tl) < a.nt || tally_chunks(s->cap_tl) < sa.nb) {
      snprintf(g_last_error, sizeof g_last_error, "%s: %u spans, arrays for %zu", who, n, s->cap_tl);
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
      snprintf(g_last_error, sizeof g_last_error, "%s: a span lies outside the %zu bytes of text it was given", who, nbytes);
      errno = EIO;
      return -1;
   }
   if ((uint64_t)h.nlong + h.nforeign > n || h.max_len > SEEQ_TALLY_LEN_MAX) return tally_fail(step, "pack", h, n, 0);
   uint64_t ntallied = (uint64_t)n - h.nlong - h.nforeign;
   const TallyCnt packed = h;
   uint32_t passes = ntallied ? tally_passes(h.max_len) : 0u;
   if (step && step->rewrite(s, step, a.src, (uint32_t *)a.dst, n, ntallied, packed, &ntallied, &passes)) return -1;
   if (ntallied) {
      TallyPass list[SEEQ_TALLY_PASS_MAX];
      tally_sort_run(st, &sa, 1, list, tally_pass_list(list, passes, 0u));
      a.src = sa.src[0]; a.dst = sa.dst[0];
      hipLaunchKernelGGL(k_tally_rle_reduce, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
      hipLaunchKernelGGL(k_tally_rle_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
      if (counters_fetch(s, s->h_tlcnt, s->d_tlcnt, sizeof(TallyCnt))) return -1;
      h = *s->h_tlcnt;
      if (h.bad || h.nonzero != ntallied || h.ndistinct > ntallied || h.ndistinct == 0 || (step && h.ndistinct > step->max_distinct))
         return tally_fail(step, "sort", h, n, ntallied);
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
      if (h.bad || (uint64_t)n - h.first != ntallied) return tally_fail(step, "table", h, n, ntallied);
      s->tl_n = h.ndistinct;
      counts->ndistinct = h.ndistinct;
   }
   counts->ntallied = ntallied; counts->nlong = packed.nlong; counts->nforeign = packed.nforeign;
   counts->max_len = packed.max_len; counts->passes = passes;
   return 0;
}

/* Which record array a source names: SEEQDEV_TALLY_INSERTS, SEEQDEV_TALLY_HITS, SEEQDEV_TALLY_GATED (the spans the last quality gate
   passed: seeq_qgate_host.h) or SEEQDEV_TALLY_ANCHORED (the spans the last anchor call cut: seeq_anchor_host.h), with the preconditions
   of each (EINVAL; the staged text for a NULL text of the inserts). */
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
   } else if (source == SEEQDEV_TALLY_GATED) {
      /* what seeqdevScanGatedDevice serves: the gate's own copies, whatever the context has scanned since; the text is the one the gated
         records were found in -- NULL: the staged one, where the gate's own source was the inserts */
      if (!s->qg_done || (!*d_text && !s->qg_from_inserts)) {
         snprintf(g_last_error, sizeof g_last_error, "tally: %s", !s->qg_done ? "the context holds no result of a quality gate" : "the gated hits need the text they were found in");
         errno = EINVAL;
         return -1;
      }
      if (staged_text(s, "tally", d_text, nbytes)) return -1;
      *rec = s->qg_rec; *off = s->qg_off; *n = s->qg_n;
   } else if (source == SEEQDEV_TALLY_ANCHORED) {
      /* what seeqdevScanAnchoredDevice serves: the anchor's own copies, under the gated records' text rule */
      if (!s->an_done || (!*d_text && !s->an_from_inserts)) {
         snprintf(g_last_error, sizeof g_last_error, "tally: %s", !s->an_done ? "the context holds no result of an anchor call" : "the anchored hits need the text they were found in");
         errno = EINVAL;
         return -1;
      }
      if (staged_text(s, "tally", d_text, nbytes)) return -1;
      *rec = s->an_rec; *off = s->an_off; *n = s->an_n;
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

/* What every tally entry over the spans of a record array does first, in this order: the arguments (EINVAL), what the context must hold for
   this call -- `missing`: NULL, or the text that says what it lacks (EINVAL) --, the record array of the source (tally_source), its size
   (E2BIG beyond 2^32 - 1 spans), the device. */
static int tally_enter(seeqdev_scan *s, const void *counts, int source, const char *missing, const void **d_text, size_t *nbytes, const uint4 **rec,
                       const uint64_t **off, uint64_t *n)
{
   seeqerr = 0;
   if (!s || !counts || (source != SEEQDEV_TALLY_INSERTS && source != SEEQDEV_TALLY_HITS && source != SEEQDEV_TALLY_GATED && source != SEEQDEV_TALLY_ANCHORED) || (!*d_text && *nbytes)) { errno = EINVAL; return -1; }
   if (missing) {
      snprintf(g_last_error, sizeof g_last_error, "%s", missing);
      errno = EINVAL;
      return -1;
   }
   if (tally_source(s, source, d_text, nbytes, rec, off, n)) return -1;
   if (*n > 0xFFFFFFFFull) { errno = E2BIG; return -1; }
   return use_device(s->device);
}

extern "C" int seeqdevScanTally(seeqdev_scan_t *s, int source, const void *d_text, size_t nbytes, seeqdev_tally_counts_t *counts)
{
   const uint4 *rec;
   const uint64_t *off;
   uint64_t n;
   if (tally_enter(s, counts, source, NULL, &d_text, &nbytes, &rec, &off, &n)) return -1;
   s->tl_n = 0;                                            /* (the table of the call before is gone, whatever comes of this one) */
   s->thd_live = false;                                    /* (... and it is no held tally's key table any more: seeq_tally_held_host.h) */
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
