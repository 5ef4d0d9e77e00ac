/*
 * seeq_tally_library_host.h -- the host driver of the tally against a known library (rule and kernels: seeq_tally_library.h): the set
 * call's validation, sort and upload, the assignment of a key array in place -- the exact pass, and under max_mismatch 1 the compaction of
 * the misses and the near pass -- as the step of tally_run (seeq_tally_host.h) between its pack and its sort, or behind the grouped
 * tally's hold, and the seeqdevScanSetLibrary / seeqdevScanSetLibraryMode / seeqdevScanLastLibraryEdits / seeqdevScanTallyLibrary /
 * seeqdevScanTallyHoldLibrary entries.  Under the edit mode (SEEQDEV_LIBRARY_EDIT) the near pass is its second instance, and the split of
 * the corrected spans is kept on the context.  Included by seeq_device.hip behind seeq_tally_group_host.h.
 */
#ifndef SEEQ_TALLY_LIBRARY_HOST_H_
#define SEEQ_TALLY_LIBRARY_HOST_H_

#include <vector>

static int tally_library_fail(const char *what, const TallyLibCnt &l, const TallyCnt &h, uint32_t n, uint64_t nkeyed, uint64_t nassigned, size_t nlib)
{
   snprintf(g_last_error, sizeof g_last_error,
            "internal inconsistency in the library tally (%s: flags %u / %u, %u spans, %llu with a key, %u exact, %u misses, %u corrected, %u ambiguous, %u unknown, "
            "%u inserted, %u deleted, %llu assigned, %u nonzero ids, %u distinct of %zu entries, first head %u)",
            what, l.bad, h.bad, n, (unsigned long long)nkeyed, l.nexact, l.nmiss, l.ncorrected, l.nambiguous, l.nunknown, l.ninserted, l.ndeleted,
            (unsigned long long)nassigned, h.nonzero, h.ndistinct, nlib, h.first);
   errno = EIO;
   return -1;
}

extern "C" int seeqdevScanSetLibraryMode(seeqdev_scan_t *s, const uint64_t *keys, size_t n, int mode)
{
   seeqerr = 0;
   if (!s) { errno = EINVAL; return -1; }
   s->lb_n = 0;                                            /* (the library of before is gone, whatever comes of this call) */
   s->lb_mismatch = 0;
   s->lb_mode = SEEQDEV_LIBRARY_EXACT;
   memset(&s->lb_edits, 0, sizeof s->lb_edits);
   if ((!keys && n) || (mode != SEEQDEV_LIBRARY_EXACT && mode != SEEQDEV_LIBRARY_SUBST && mode != SEEQDEV_LIBRARY_EDIT)) { errno = EINVAL; return -1; }
   if (!n) return 0;
   if (n > SEEQ_TLIB_MAX) {
      snprintf(g_last_error, sizeof g_last_error, "library: %zu entries, at most %u", n, SEEQ_TLIB_MAX);
      errno = E2BIG;
      return -1;
   }
   std::vector<uint64_t> skey(n);
   std::vector<uint32_t> sid(n);
   size_t at;
   const int bad = tally_lib_prepare(keys, n, skey.data(), sid.data(), &at);
   if (bad) {
      snprintf(g_last_error, sizeof g_last_error, bad == SEEQ_TLIB_E_NOKEY ? "library: entry %zu (%#llx) is no tally key" : "library: entry %zu (%#llx) repeats an earlier entry",
               at, (unsigned long long)keys[at]);
      errno = EINVAL;
      return -1;
   }
   if (use_device(s->device)) return -1;
   if (ws_grow(&s->ws, &s->cap_lb, n, {{s->lb_key, n * sizeof(uint64_t)}, {s->lb_id, n * sizeof(uint32_t)}})) return -1;
   HIP_TRY(hipMemcpyAsync(s->lb_key, skey.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream), EIO);
   HIP_TRY(hipMemcpyAsync(s->lb_id, sid.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream), EIO);
   HIP_TRY(hipStreamSynchronize(s->stream), EIO);            /* (the host copies go with this call) */
   s->lb_n = n;
   s->lb_mismatch = mode != SEEQDEV_LIBRARY_EXACT;
   s->lb_mode = mode;
   return 0;
}

/* (max_mismatch 0 and 1 ARE the modes SEEQDEV_LIBRARY_EXACT and _SUBST; any other value is no mode) */
extern "C" int seeqdevScanSetLibrary(seeqdev_scan_t *s, const uint64_t *keys, size_t n, int max_mismatch)
{
   return seeqdevScanSetLibraryMode(s, keys, n, max_mismatch == 0 || max_mismatch == 1 ? max_mismatch : -1);
}

extern "C" int seeqdevScanLastLibraryEdits(const seeqdev_scan_t *s, seeqdev_tally_library_edits_t *out)
{
   if (!s || !out) { errno = EINVAL; return -1; }
   *out = s->lb_edits;
   return 0;
}

/* key[0 .. n), n > 0, the spans' keys -> their ids against the context's library, in place; miss: room for 4 bytes per span that nothing
   else uses until this returns.  *l: the five counts, checked against nkeyed, the nonzero keys.  Waits. */
static int tally_library_assign(seeqdev_scan *s, uint64_t *key, uint32_t *miss, uint32_t n, uint64_t nkeyed, TallyLibCnt *l)
{
   const hipStream_t st = s->stream;
   const bool edit = s->lb_mode == SEEQDEV_LIBRARY_EDIT;
   memset(&s->lb_edits, 0, sizeof s->lb_edits);             /* (a failed assignment leaves no split) */
   const size_t nt = (size_t)tally_tiles(n);
   if (ws_make(&s->ws, {{s->d_lbcnt, sizeof(TallyLibCnt)}, {s->h_lbcnt, sizeof(TallyLibCnt), WS_PINNED}})) return -1;
   if (ws_grow(&s->ws, &s->cap_lb_sum, nt, {{s->lb_sum, 2 * nt * sizeof(uint32_t)}})) return -1;
   TallyLibArgs a;
   memset(&a, 0, sizeof a);
   a.key = key; a.n = n; a.nt = (uint32_t)nt;
   a.lkey = s->lb_key; a.lid = s->lb_id; a.nlib = (uint32_t)s->lb_n;
   a.stride = tally_lib_stride(a.nlib); a.probes = tally_lib_probes(a.stride);
   a.near = s->lb_mismatch ? 1u : 0u;
   a.esum = s->lb_sum;
   a.miss = miss;
   a.cnt = s->d_lbcnt;
   const TallyCnt none = {};
   if (!s->lb_n || s->lb_n > s->cap_lb || s->lb_n > SEEQ_TLIB_MAX || nt > s->cap_lb_sum) {
      snprintf(g_last_error, sizeof g_last_error, "library tally: %zu entries, arrays for %zu; %zu tiles, sums for %zu", s->lb_n, s->cap_lb, nt, s->cap_lb_sum);
      errno = EIO;
      return -1;
   }
   HIP_TRY(hipMemsetAsync(s->d_lbcnt, 0, sizeof(TallyLibCnt), st), EIO);
   hipLaunchKernelGGL(k_tally_assign_exact, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_tally_assign_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
   if (counters_fetch(s, s->h_lbcnt, s->d_lbcnt, sizeof(TallyLibCnt))) return -1;
   *l = *s->h_lbcnt;
   if ((uint64_t)l->nexact + l->nmiss != nkeyed) return tally_library_fail("exact", *l, none, n, nkeyed, 0, s->lb_n);
   if (!a.near) { l->nunknown = l->nmiss; return 0; }      /* max_mismatch 0: a miss is unknown, and 0 stands at its index already */
   if (!l->nmiss) return 0;                                /* no miss: the near pass is not launched */
   a.nmiss = l->nmiss;
   a.nwg = (uint32_t)(((uint64_t)a.nmiss + SEEQ_TLIB_NEAR_WG * SEEQ_TLIB_NEAR_ROUNDS - 1) / (SEEQ_TLIB_NEAR_WG * SEEQ_TLIB_NEAR_ROUNDS));
   if (ws_grow(&s->ws, &s->cap_lb_near, a.nwg, {{s->lb_nstat, (size_t)a.nwg * sizeof(uint4)}})) return -1;
   a.nstat = s->lb_nstat;
   if (edit) {                                             /* the edit instance's two further counts per workgroup */
      if (ws_grow(&s->ws, &s->cap_lb_edit, a.nwg, {{s->lb_nedit, (size_t)a.nwg * sizeof(uint2)}})) return -1;
      a.nedit = s->lb_nedit;
   }
   if ((size_t)a.nwg > s->cap_lb_near || (edit && (size_t)a.nwg > s->cap_lb_edit)) {
      snprintf(g_last_error, sizeof g_last_error, "library tally: %u workgroups of the near pass, room for %zu%s", a.nwg, edit ? s->cap_lb_edit : s->cap_lb_near,
               edit ? " (the edit counts)" : "");
      errno = EIO;
      return -1;
   }
   hipLaunchKernelGGL(k_tally_miss_apply, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
   if (edit) hipLaunchKernelGGL(k_tally_assign_near_edit, dim3(a.nwg), dim3(SEEQ_TILE_WG), 0, st, a);
   else hipLaunchKernelGGL(k_tally_assign_near, dim3(a.nwg), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_tally_near_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
   if (counters_fetch(s, s->h_lbcnt, s->d_lbcnt, sizeof(TallyLibCnt))) return -1;
   *l = *s->h_lbcnt;
   if (l->bad || (uint64_t)l->nexact + l->nmiss != nkeyed || (uint64_t)l->ncorrected + l->nambiguous + l->nunknown != l->nmiss)
      return tally_library_fail("near", *l, none, n, nkeyed, 0, s->lb_n);
   if ((uint64_t)l->ninserted + l->ndeleted > l->ncorrected || (!edit && (l->ninserted || l->ndeleted)))      /* (nsubstituted is the rest of ncorrected) */
      return tally_library_fail("edits", *l, none, n, nkeyed, 0, s->lb_n);
   s->lb_edits.nsubstituted = (uint64_t)l->ncorrected - l->ninserted - l->ndeleted;
   s->lb_edits.ninserted = l->ninserted;
   s->lb_edits.ndeleted = l->ndeleted;
   return 0;
}

static void tally_library_counts(seeqdev_tally_library_counts_t *counts, const TallyLibCnt &l)
{
   counts->nexact = l.nexact; counts->ncorrected = l.ncorrected; counts->nambiguous = l.nambiguous; counts->nunknown = l.nunknown;
   counts->nassigned = (uint64_t)l.nexact + l.ncorrected;
}

/* THE LIBRARY AS tally_run's STEP between its pack and its sort: the assignment of the key array in place, the sort's passes from the
   library's size, and the library's numbers beside the tally's in the text of an inconsistency. */
struct TallyLibStep : TallyStep {
   TallyLibCnt l;                     /* the assignment's five counts */
   uint64_t    nkeyed;                /* the spans with a key it saw */
};

static int tally_library_step_fail(const TallyStep *step, const char *what, const TallyCnt &h, uint32_t n, uint64_t nassigned)
{
   const TallyLibStep *ls = (const TallyLibStep *)step;
   return tally_library_fail(what, ls->l, h, n, ls->nkeyed, nassigned, ls->max_distinct);
}

static int tally_library_step(seeqdev_scan *s, TallyStep *step, uint64_t *key, uint32_t *scratch, uint32_t n, uint64_t nkeyed, const TallyCnt &packed, uint64_t *nleft,
                              uint32_t *passes)
{
   TallyLibStep *ls = (TallyLibStep *)step;
   ls->nkeyed = nkeyed;
   if (nkeyed && tally_library_assign(s, key, scratch, n, nkeyed, &ls->l)) return -1;      /* (4 bytes per miss in the 8 per span the sort has not touched yet) */
   const TallyLibCnt &l = ls->l;
   *nleft = (uint64_t)l.nexact + l.ncorrected;
   if ((uint64_t)l.nexact + l.ncorrected + l.nambiguous + l.nunknown + packed.nlong + packed.nforeign != n) return tally_library_step_fail(step, "kinds", packed, n, *nleft);
   *passes = tally_lib_passes(*nleft, (uint32_t)s->lb_n);
   return 0;
}

/* The table of the n spans rec / off of text[0 .. nbytes) against the library; the context's table (tl_tab, tl_n) is the result: tally_run
   with the step above, and its counts beside the assignment's.  Waits. */
static int tally_library_run(seeqdev_scan *s, const uint4 *rec, const uint64_t *off, uint32_t n, const void *d_text, size_t nbytes,
                             seeqdev_tally_library_counts_t *counts)
{
   memset(counts, 0, sizeof *counts);
   counts->nspans = n;
   counts->key_bits = tally_lib_bitlen(s->lb_n);
   TallyLibStep step = {};
   step.who = "library tally"; step.max_distinct = s->lb_n;
   step.rewrite = tally_library_step; step.fail = tally_library_step_fail;
   seeqdev_tally_counts_t t;
   if (tally_run(s, rec, off, n, d_text, nbytes, &t, &step)) return -1;
   tally_library_counts(counts, step.l);
   counts->nlong = t.nlong; counts->nforeign = t.nforeign;
   counts->ndistinct = t.ndistinct; counts->passes = t.passes;
   return 0;
}

static const char *tally_library_missing(const seeqdev_scan *s)
{
   return s && !s->lb_n ? "library tally: the context holds no library (seeqdevScanSetLibrary)" : NULL;
}

extern "C" int seeqdevScanTallyLibrary(seeqdev_scan_t *s, int source, const void *d_text, size_t nbytes, seeqdev_tally_library_counts_t *counts)
{
   const uint4 *rec;
   const uint64_t *off;
   uint64_t n;
   if (tally_enter(s, counts, source, tally_library_missing(s), &d_text, &nbytes, &rec, &off, &n)) return -1;
   memset(&s->lb_edits, 0, sizeof s->lb_edits);             /* (no span with a key: no assignment, and no split of one before) */
   s->tl_n = 0;                                            /* (the table of the tally before, of either kind, is gone, whatever comes of this one) */
   s->thd_live = false;                                    /* (... and it is no held tally's key table any more: seeq_tally_held_host.h) */
   s->tm_tl.ms = 0.f;
   return tally_library_run(s, rec, off, (uint32_t)n, d_text, nbytes, counts);
}

extern "C" int seeqdevScanTallyHoldLibrary(seeqdev_scan_t *s, int source, const void *d_text, size_t nbytes, seeqdev_tally_library_counts_t *counts)
{
   const uint4 *rec;
   const uint64_t *off;
   uint64_t n;
   if (tally_enter(s, counts, source, tally_library_missing(s), &d_text, &nbytes, &rec, &off, &n)) return -1;
   memset(&s->lb_edits, 0, sizeof s->lb_edits);             /* (no span with a key: no assignment, and no split of one before) */
   tally_hold_reset(s);
   seeqdev_tally_hold_counts_t held;
   if (tally_hold_run(s, rec, off, (uint32_t)n, false, d_text, nbytes, &held, tally_hold_target(s))) return -1;
   memset(counts, 0, sizeof *counts);
   counts->nspans = n;
   counts->key_bits = tally_lib_bitlen(s->lb_n);
   counts->nlong = held.nlong; counts->nforeign = held.nforeign;
   TallyLibCnt l = {};
   if (held.nheld) {
      /* the miss indices go where the plain tally's second key array lies: the scratch a following grouped call allocates anyway */
      if (tally_ws_keys(s, (size_t)n)) return -1;
      if ((size_t)n > s->cap_tl || (size_t)n > s->cap_th) {
         snprintf(g_last_error, sizeof g_last_error, "library hold: %llu records, arrays for %zu and %zu", (unsigned long long)n, s->cap_th, s->cap_tl);
         errno = EIO;
         return -1;
      }
      if (tally_library_assign(s, s->th_key, (uint32_t *)s->tl_key1, (uint32_t)n, held.nheld, &l)) return -1;
   }
   tally_library_counts(counts, l);
   if (counts->nexact + counts->ncorrected + counts->nambiguous + counts->nunknown + counts->nlong + counts->nforeign != n)
      return tally_library_fail("hold", l, TallyCnt{}, (uint32_t)n, held.nheld, counts->nassigned, s->lb_n);
   tally_hold_done(s, n, counts->nassigned, counts->key_bits);
   return 0;
}

#include "seeq_tally_append_host.h"

#endif
