/*
 * seeq_anchor_host.h -- the host driver of the anchored cut (rule and kernels: seeq_anchor.h): seeqdevScanAnchor and the entries that serve
 * its arrays.  The anchor reads the record array of a tally source (tally_source, seeq_tally_host.h) and writes arrays of its own -- the
 * kinds of the source's records and the ends of their cuts, the kept records with their rewritten spans and their offsets -- which
 * SEEQDEV_TALLY_ANCHORED then names to the tally entries and to the quality gate.  Included by seeq_device.hip behind seeq_tally_host.h.
 */
#ifndef SEEQ_ANCHOR_HOST_H_
#define SEEQ_ANCHOR_HOST_H_

static int anchor_fail(const char *what, const AnchorCnt &h, uint32_t n)
{
   snprintf(g_last_error, sizeof g_last_error, "internal inconsistency in the anchor (%s: %u records, %u kept, %u short, %u far, %u placed)", what, n, h.nkept,
            h.nshort, h.nfar, h.placed);
   errno = EIO;
   return -1;
}

/* The cut of the n records rec / off of text[0 .. nbytes): the kinds in an_kind, the kept records in an_rec / an_off.  Waits. */
static int anchor_run(seeqdev_scan *s, const uint4 *rec, const uint64_t *off, uint32_t n, const void *d_text, size_t nbytes, int anchor, uint32_t skip,
                      uint32_t len, uint32_t reach, seeqdev_anchor_counts_t *counts)
{
   const hipStream_t st = s->stream;
   memset(counts, 0, sizeof *counts);
   counts->nspans = n;
   if (!n) return 0;                                       /* no records: nothing is launched */
   if (ws_make(&s->ws, {{s->d_ancnt, sizeof(AnchorCnt)}, {s->h_ancnt, sizeof(AnchorCnt), WS_PINNED}})) return -1;
   const size_t nt = (size_t)seeq_tiles_of(n);
   if (ws_grow(&s->ws, &s->cap_an, n, {{s->an_kind, (size_t)n}, {s->an_end, (size_t)n * sizeof(uint32_t)}, {s->an_bsum, (nt + 1) * SEEQ_ANCHOR_SUMS * sizeof(uint32_t)}}))
      return -1;
   AnchorArgs a;
   memset(&a, 0, sizeof a);
   a.rec = rec; a.off = off; a.n = n; a.nt = (uint32_t)nt;
   a.text = (const uint8_t *)d_text; a.nbytes = nbytes;
   a.anchor = anchor; a.skip = skip; a.len = len; a.reach = reach; a.steps = qgate_steps(reach);
   a.kind = s->an_kind; a.end = s->an_end; a.bsum = s->an_bsum;
   a.cnt = s->d_ancnt;
   if ((size_t)n > s->cap_an || seeq_tiles_of(s->cap_an) < nt) {
      snprintf(g_last_error, sizeof g_last_error, "anchor: %u records, arrays for %zu", n, s->cap_an);
      errno = EIO;
      return -1;
   }
   if (s->tm_an.begin(s->prof, st)) return -1;
   HIP_TRY(hipMemsetAsync(s->d_ancnt, 0, sizeof(AnchorCnt), st), EIO);
   hipLaunchKernelGGL(k_anchor_reduce, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_anchor_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
   if (counters_fetch(s, s->h_ancnt, s->d_ancnt, sizeof(AnchorCnt))) return -1;
   AnchorCnt h = *s->h_ancnt;
   if (h.bad) {
      snprintf(g_last_error, sizeof g_last_error, "anchor: a record lies outside the %zu bytes of text it was given", nbytes);
      errno = EIO;
      return -1;
   }
   if ((uint64_t)h.nkept + h.nshort + h.nfar != n) return anchor_fail("kinds", h, n);
   if (h.nkept) {
      /* the kept records: a group of its own, grown now that their number is known */
      const size_t nk = h.nkept;
      if (ws_grow(&s->ws, &s->cap_an_out, nk, {{s->an_rec, nk * sizeof(uint4)}, {s->an_off, nk * sizeof(uint64_t)}})) return -1;
      a.out = s->an_rec; a.off_out = s->an_off; a.nk = h.nkept;
      hipLaunchKernelGGL(k_anchor_apply, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
      if (counters_copy(s, s->h_ancnt, s->d_ancnt, sizeof(AnchorCnt))) return -1;
   }
   if (s->tm_an.end(s->prof, st)) return -1;
   HIP_TRY(hipStreamSynchronize(st), EIO);
   s->tm_an.read(s->prof);
   if (h.nkept) {
      h = *s->h_ancnt;
      if (h.placed != h.nkept) return anchor_fail("apply", h, n);
   }
   counts->nkept = h.nkept; counts->nshort = h.nshort; counts->nfar = h.nfar;
   counts->span_bytes = h.span_bytes;
   return 0;
}

extern "C" int seeqdevScanAnchor(seeqdev_scan_t *s, int source, const void *d_text, size_t nbytes, int anchor, uint32_t skip, uint32_t len, uint32_t reach,
                                 seeqdev_anchor_counts_t *counts)
{
   const uint4 *rec;
   const uint64_t *off;
   uint64_t n;
   seeqerr = 0;
   if ((source != SEEQDEV_TALLY_INSERTS && source != SEEQDEV_TALLY_HITS) || (anchor != SEEQDEV_ANCHOR_AFTER && anchor != SEEQDEV_ANCHOR_BEFORE && anchor != SEEQDEV_ANCHOR_LINE) ||
       reach < 1u || reach > SEEQ_ANCHOR_REACH_MAX || (anchor != SEEQDEV_ANCHOR_BEFORE && len > 0u && (uint64_t)skip + len > reach)) {
      errno = EINVAL;
      return -1;
   }
   if (tally_enter(s, counts, source, NULL, &d_text, &nbytes, &rec, &off, &n)) return -1;
   s->an_done = false;                                     /* (the arrays of the anchor before are gone, whatever comes of this one) */
   s->an_n = s->an_nsrc = 0;
   s->tm_an.ms = 0.f;
   if (anchor_run(s, rec, off, (uint32_t)n, d_text, nbytes, anchor, skip, len, reach, counts)) return -1;
   s->an_n = (size_t)counts->nkept;
   s->an_nsrc = (size_t)n;
   s->an_from_inserts = source == SEEQDEV_TALLY_INSERTS;
   s->an_done = true;                                      /* (an anchor that kept nothing included) */
   return 0;
}

extern "C" const seeqdev_hit_t *seeqdevScanAnchoredDevice(const seeqdev_scan_t *s) { return s && s->an_done && s->an_n ? (const seeqdev_hit_t *)s->an_rec : NULL; }

extern "C" int seeqdevScanCopyAnchored(seeqdev_scan_t *s, void *host_out, size_t first, size_t n)
{
   return copy_out(s, host_out, s ? s->an_rec : NULL, sizeof(uint4), s && s->an_done ? s->an_n : 0, first, n);
}

extern "C" int seeqdevScanCopyAnchoredOffsets(seeqdev_scan_t *s, uint64_t *host_out, size_t first, size_t n)
{
   return copy_out(s, host_out, s ? s->an_off : NULL, sizeof(uint64_t), s && s->an_done ? s->an_n : 0, first, n);
}

extern "C" int seeqdevScanCopyAnchorKinds(seeqdev_scan_t *s, uint8_t *host_out, size_t first, size_t n)
{
   return copy_out(s, host_out, s ? s->an_kind : NULL, sizeof(uint8_t), s && s->an_done ? s->an_nsrc : 0, first, n);
}

extern "C" int seeqdevScanLastAnchorMs(const seeqdev_scan_t *s, float *ms)
{
   if (!s || !ms) { errno = EINVAL; return -1; }
   *ms = s->tm_an.ms;
   return 0;
}

#endif
