/*
 * seeq_tally_group_host.h -- the host driver of the grouped tally (rule and kernels: seeq_tally_group.h): the hold of one record array's
 * keys, the pairing of another's spans with them, as many passes of the two-word sort as the largest paired member and the largest held
 * key ask for, the run-length pass with its two tables, and the seeqdevScanTallyHold / seeqdevScanTallyGrouped / seeqdevScan*TallyPairs* /
 * *TallyGroups* entries.  Included by seeq_device.hip behind seeq_tally_host.h.
 */
#ifndef SEEQ_TALLY_GROUP_HOST_H_
#define SEEQ_TALLY_GROUP_HOST_H_

static int tally_group_ws_cnt(seeqdev_scan *s)
{
   return ws_make(&s->ws, {{s->d_tgcnt, sizeof(TallyGroupCnt)}, {s->h_tgcnt, sizeof(TallyGroupCnt), WS_PINNED}});
}

static int tally_group_fail(const char *what, const TallyGroupCnt &h, uint32_t n, uint64_t npaired)
{
   snprintf(g_last_error, sizeof g_last_error,
            "internal inconsistency in the grouped tally (%s: flags %u, %u spans, %u long, %u foreign, %u ungrouped or ambiguous, %llu paired, %u nonzero items, "
            "%u pairs, %u groups, first pair head %u, first group head %u of rank %u)",
            what, h.bad, n, h.nlong, h.nforeign, h.nthird, (unsigned long long)npaired, h.nonzero, h.npairs, h.ngroups, h.pair_first, h.group_first, h.rank_first);
   errno = EIO;
   return -1;
}

static int tally_group_outside(const char *who, size_t nbytes)
{
   snprintf(g_last_error, sizeof g_last_error, "%s: a span lies outside the %zu bytes of text it was given", who, nbytes);
   errno = EIO;
   return -1;
}

/* The arrays a hold writes: the context's held column (th_line / th_key / th_stat), or the column an append builds beside it
   (seeq_tally_append_host.h) -- one capacity group either way. */
struct TallyHoldTarget {
   uint32_t *&line; uint64_t *&key; uint32_t *&stat; size_t &cap;
};

static TallyHoldTarget tally_hold_target(seeqdev_scan *s) { return {s->th_line, s->th_key, s->th_stat, s->cap_th}; }

/* The column of the n records rec / off (demux: seeqdev_demux_t records, no offsets, no text) in the arrays of `to`.  Waits. */
static int tally_hold_run(seeqdev_scan *s, const uint4 *rec, const uint64_t *off, uint32_t n, bool demux, const void *d_text, size_t nbytes,
                          seeqdev_tally_hold_counts_t *counts, const TallyHoldTarget &to)
{
   const hipStream_t st = s->stream;
   memset(counts, 0, sizeof *counts);
   counts->nspans = n;
   if (!n) return 0;                                       /* no records: nothing is launched, the column is empty */
   const size_t nt = (size_t)tally_tiles(n);
   if (tally_group_ws_cnt(s)) return -1;
   if (ws_grow(&s->ws, &to.cap, n, {{to.line, n * sizeof(uint32_t)}, {to.key, n * sizeof(uint64_t)},
                                    {to.stat, nt * SEEQ_TALLY_STAT * sizeof(uint32_t)}})) return -1;
   TallyGroupArgs a;
   memset(&a, 0, sizeof a);
   a.rec = rec; a.off = off; a.n = n; a.nt = (uint32_t)nt;
   a.text = (const uint8_t *)d_text; a.nbytes = nbytes;
   a.demux = demux ? 1u : 0u;
   a.hold_line = to.line; a.hold_key = to.key;
   a.tstat = to.stat;
   a.cnt = s->d_tgcnt;
   if ((size_t)n > to.cap || tally_tiles(to.cap) < nt) {
      snprintf(g_last_error, sizeof g_last_error, "tally hold: %u records, arrays for %zu", n, to.cap);
      errno = EIO;
      return -1;
   }
   HIP_TRY(hipMemsetAsync(s->d_tgcnt, 0, sizeof(TallyGroupCnt), st), EIO);
   hipLaunchKernelGGL(k_tally_hold, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_tally_group_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
   if (counters_fetch(s, s->h_tgcnt, s->d_tgcnt, sizeof(TallyGroupCnt))) return -1;
   const TallyGroupCnt h = *s->h_tgcnt;
   if (h.bad) return tally_group_outside("tally hold", nbytes);
   if ((uint64_t)h.nlong + h.nforeign + h.nthird > n || h.max_len > SEEQ_TALLY_LEN_MAX || h.key_bits > 63u || (demux && h.key_bits > 8u))
      return tally_group_fail("hold", h, n, 0);
   counts->nlong = h.nlong; counts->nforeign = h.nforeign; counts->nambiguous = h.nthird;
   counts->nheld = (uint64_t)n - h.nlong - h.nforeign - h.nthird;
   counts->max_len = h.max_len; counts->key_bits = h.key_bits;
   return 0;
}

/* What a hold over `source` does first: SEEQDEV_TALLY_DEMUX names the records seeqdevScanDemuxDevice serves now (no text, no offsets), every
   other source is tally_enter's; `missing` as there. */
static int tally_hold_enter(seeqdev_scan *s, const void *counts, int source, const char *missing, const void **d_text, size_t *nbytes, const uint4 **rec,
                            const uint64_t **off, uint64_t *n)
{
   if (source != SEEQDEV_TALLY_DEMUX) return tally_enter(s, counts, source, missing, d_text, nbytes, rec, off, n);
   seeqerr = 0;
   if (!s || !counts) { errno = EINVAL; return -1; }
   if (missing) {
      snprintf(g_last_error, sizeof g_last_error, "%s", missing);
      errno = EINVAL;
      return -1;
   }
   /* what seeqdevScanDemuxDevice serves: valid until the context's next scan -- a demux leaves nothing to fetch (scan_forget), a plain or
      packed scan after it leaves its pattern */
   if (!s->dm_done || s->pat || s->ran) {
      snprintf(g_last_error, sizeof g_last_error, "tally hold: %s", !s->dm_done ? "the context holds no result of a demux call" : "a later scan has invalidated the demux records");
      errno = EINVAL;
      return -1;
   }
   *rec = s->dm_out; *off = NULL; *n = s->dm_nrec;
   *d_text = NULL; *nbytes = 0;
   if (*n > 0xFFFFFFFFull) { errno = E2BIG; return -1; }
   return use_device(s->device);
}

/* the column of the hold before is gone, whatever comes of the one that begins */
static void tally_hold_reset(seeqdev_scan *s)
{
   s->th_done = false;
   s->th_n = 0;
   s->th_key_bits = 0;
   s->th_nkeyed = 0;
   s->th_ncol = 0;
}

/* a hold has completed: n records, nkeyed of them with a key, the largest of key_bits bits -- one column of that width */
static void tally_hold_done(seeqdev_scan *s, uint64_t n, uint64_t nkeyed, uint32_t key_bits)
{
   s->th_n = (size_t)n;
   s->th_key_bits = key_bits;
   s->th_nkeyed = nkeyed;
   s->th_ncol = 1;
   s->th_width[0] = key_bits;
   s->th_done = true;
}

extern "C" int seeqdevScanTallyHold(seeqdev_scan_t *s, int source, const void *d_text, size_t nbytes, seeqdev_tally_hold_counts_t *counts)
{
   const uint4 *rec;
   const uint64_t *off;
   uint64_t n;
   if (tally_hold_enter(s, counts, source, NULL, &d_text, &nbytes, &rec, &off, &n)) return -1;
   tally_hold_reset(s);
   if (tally_hold_run(s, rec, off, (uint32_t)n, source == SEEQDEV_TALLY_DEMUX, d_text, nbytes, counts, tally_hold_target(s))) return -1;
   tally_hold_done(s, n, counts->nheld, counts->key_bits);
   return 0;
}

/* Room for n member spans: the plain tally's key scratch (the member words, the digit matrix, the scan's chunk sums) and beside it the two
   group-word arrays, the head sums and the tiles' words -- one group. */
static int tally_group_ws_keys(seeqdev_scan *s, size_t n)
{
   if (tally_ws_keys(s, n) || tally_group_ws_cnt(s)) return -1;
   const size_t nt = (size_t)tally_tiles(n) + 1;
   return ws_grow(&s->ws, &s->cap_tg, n, {{s->tg_g0, n * sizeof(uint64_t)}, {s->tg_g1, n * sizeof(uint64_t)}, {s->tg_sum, 3 * nt * sizeof(uint32_t)},
                                          {s->tg_stat, nt * SEEQ_TALLY_STAT * sizeof(uint32_t)}});
}

/* The two tables of the n member spans rec / off of text[0 .. nbytes) against the held column; the context's tables (tg_pairs: tg_np,
   tg_groups: tg_ng) are the result.  Waits. */
static int tally_grouped_run(seeqdev_scan *s, const uint4 *rec, const uint64_t *off, uint32_t n, const void *d_text, size_t nbytes,
                             seeqdev_tally_grouped_counts_t *counts)
{
   const hipStream_t st = s->stream;
   memset(counts, 0, sizeof *counts);
   counts->nspans = n;
   if (!n) return 0;                                       /* no spans: nothing is launched */
   if (tally_group_ws_keys(s, n)) return -1;
   TallyGroupArgs a;
   memset(&a, 0, sizeof a);
   a.rec = rec; a.off = off; a.n = n;
   a.nt = (uint32_t)tally_tiles(n);
   a.text = (const uint8_t *)d_text; a.nbytes = nbytes;
   a.hold_line = s->th_line; a.hold_key = s->th_key; a.nh = (uint32_t)s->th_n;
   a.tstat = s->tg_stat;
   a.rsum = s->tg_sum;
   a.cnt = s->d_tgcnt;
   TallySortArgs sa = tally_sort_args(s, n, s->tg_stat);   /* word 0: the members, in the plain tally's key arrays; word 1: the groups */
   sa.src[1] = s->tg_g0; sa.dst[1] = s->tg_g1;
   a.msrc = sa.src[0]; a.gsrc = sa.src[1];
   if ((size_t)n > s->cap_tl || (size_t)n > s->cap_tg || tally_tiles(s->cap_tl) < a.nt || tally_tiles(s->cap_tg) < a.nt || tally_chunks(s->cap_tl) < sa.nb ||
       s->th_n > s->cap_th) {
      snprintf(g_last_error, sizeof g_last_error, "grouped tally: %u spans, arrays for %zu and %zu; %zu held records, arrays for %zu", n, s->cap_tl, s->cap_tg,
               s->th_n, s->cap_th);
      errno = EIO;
      return -1;
   }
   if (s->tm_tg.begin(s->prof, st)) return -1;
   HIP_TRY(hipMemsetAsync(s->d_tgcnt, 0, sizeof(TallyGroupCnt), st), EIO);
   hipLaunchKernelGGL(k_tally_pair_pack, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_tally_group_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
   if (counters_fetch(s, s->h_tgcnt, s->d_tgcnt, sizeof(TallyGroupCnt))) return -1;
   TallyGroupCnt h = *s->h_tgcnt;
   if (h.bad) return tally_group_outside("grouped tally", nbytes);
   if ((uint64_t)h.nlong + h.nforeign + h.nthird > n || h.max_len > SEEQ_TALLY_LEN_MAX) return tally_group_fail("pack", h, n, 0);
   const uint64_t npaired = (uint64_t)n - h.nlong - h.nforeign - h.nthird;
   const TallyGroupCnt packed = h;
   const uint32_t passes = tally_pair_passes(npaired, h.max_len, s->th_key_bits);
   if (npaired) {
      TallyPass list[SEEQ_TALLY_PASS_MAX];
      tally_sort_run(st, &sa, 2, list, tally_pass_list(list, tally_passes(h.max_len), tally_group_passes(s->th_key_bits)));
      a.msrc = sa.src[0]; a.gsrc = sa.src[1];
      hipLaunchKernelGGL(k_tally_pair_rle_reduce, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
      hipLaunchKernelGGL(k_tally_pair_rle_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
      if (counters_fetch(s, s->h_tgcnt, s->d_tgcnt, sizeof(TallyGroupCnt))) return -1;
      h = *s->h_tgcnt;
      if (h.bad || h.nonzero != npaired || h.ngroups == 0 || h.ngroups > h.npairs || h.npairs > h.nonzero) return tally_group_fail("sort", h, n, npaired);
      /* the tables: groups of their own, grown now that their sizes are known */
      const size_t np = h.npairs, ng = h.ngroups;
      if (ws_grow(&s->ws, &s->cap_tg_pairs, np, {{s->tg_pairs, np * sizeof(seeqdev_tally_pair_t)}})) return -1;
      if (ws_grow(&s->ws, &s->cap_tg_groups, ng, {{s->tg_groups, ng * sizeof(seeqdev_tally_group_t)}})) return -1;
      a.np = h.npairs; a.ng = h.ngroups;
      a.ppos = (uint32_t *)sa.dst[0];                      /* (4 bytes per pair head in the 8 bytes per span the last pass left free ...) */
      a.gpos = (uint32_t *)sa.dst[1];                      /* (... and 4 + 4 per group head in the group words') */
      a.grank = a.gpos + n;
      a.ptab = (uint64_t *)s->tg_pairs; a.gtab = (uint64_t *)s->tg_groups;
      a.cap_ptab = cap_u32(s->cap_tg_pairs); a.cap_gtab = cap_u32(s->cap_tg_groups);
      hipLaunchKernelGGL(k_tally_pair_rle_apply, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
      hipLaunchKernelGGL(k_tally_pair_table, dim3((unsigned)((np + SEEQ_TILE_WG - 1) / SEEQ_TILE_WG)), dim3(SEEQ_TILE_WG), 0, st, a);
      hipLaunchKernelGGL(k_tally_group_table, dim3((unsigned)((ng + SEEQ_TILE_WG - 1) / SEEQ_TILE_WG)), dim3(SEEQ_TILE_WG), 0, st, a);
      if (counters_copy(s, s->h_tgcnt, s->d_tgcnt, sizeof(TallyGroupCnt))) return -1;
   }
   if (s->tm_tg.end(s->prof, st)) return -1;
   HIP_TRY(hipStreamSynchronize(st), EIO);
   s->tm_tg.read(s->prof);
   if (npaired) {
      h = *s->h_tgcnt;
      /* the counts of either table telescope to n - its first head's index (the (0, 0) items lie before it), the groups' ndistinct to
         npairs - the first group's rank */
      if (h.bad || (uint64_t)n - h.pair_first != npaired || (uint64_t)n - h.group_first != npaired || h.rank_first != 0u)
         return tally_group_fail("tables", h, n, npaired);
      s->tg_np = h.npairs; s->tg_ng = h.ngroups;
      counts->npairs = h.npairs; counts->ngroups = h.ngroups;
   }
   counts->npaired = npaired; counts->nlong = packed.nlong; counts->nforeign = packed.nforeign; counts->nungrouped = packed.nthird;
   counts->max_len = npaired ? packed.max_len : 0u; counts->passes = passes;
   return 0;
}

extern "C" int seeqdevScanTallyGrouped(seeqdev_scan_t *s, int source, const void *d_text, size_t nbytes, seeqdev_tally_grouped_counts_t *counts)
{
   const uint4 *rec;
   const uint64_t *off;
   uint64_t n;
   const char *missing = s && !s->th_done ? "grouped tally: the context holds no held column (seeqdevScanTallyHold)" : NULL;
   if (tally_enter(s, counts, source, missing, &d_text, &nbytes, &rec, &off, &n)) return -1;
   s->tg_np = s->tg_ng = 0;                                /* (the tables of the call before are gone, whatever comes of this one) */
   s->tg_done = false;
   s->tc_np = s->tc_ng = 0;                                /* (... and with them what a collapse made of them: seeq_tally_collapse_host.h) */
   s->tm_tg.ms = 0.f;
   if (tally_grouped_run(s, rec, off, (uint32_t)n, d_text, nbytes, counts)) return -1;
   s->tg_npaired = counts->npaired; s->tg_max_len = counts->max_len;
   s->tg_done = true;                                      /* (a call that paired nothing included) */
   return 0;
}

extern "C" const seeqdev_tally_pair_t *seeqdevScanTallyPairsDevice(const seeqdev_scan_t *s) { return s ? s->tg_pairs : NULL; }

extern "C" const seeqdev_tally_group_t *seeqdevScanTallyGroupsDevice(const seeqdev_scan_t *s) { return s ? s->tg_groups : NULL; }

extern "C" int seeqdevScanCopyTallyPairs(seeqdev_scan_t *s, seeqdev_tally_pair_t *host_out, size_t first, size_t n)
{
   return copy_out(s, host_out, s ? s->tg_pairs : NULL, sizeof(seeqdev_tally_pair_t), s ? s->tg_np : 0, first, n);
}

extern "C" int seeqdevScanCopyTallyGroups(seeqdev_scan_t *s, seeqdev_tally_group_t *host_out, size_t first, size_t n)
{
   return copy_out(s, host_out, s ? s->tg_groups : NULL, sizeof(seeqdev_tally_group_t), s ? s->tg_ng : 0, first, n);
}

extern "C" int seeqdevScanLastTallyGroupedMs(const seeqdev_scan_t *s, float *ms)
{
   if (!s || !ms) { errno = EINVAL; return -1; }
   *ms = s->tm_tg.ms;
   return 0;
}

#endif
