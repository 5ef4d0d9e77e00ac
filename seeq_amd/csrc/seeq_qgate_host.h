/*
 * seeq_qgate_host.h -- the host driver of the base-quality gate (rule and kernels: seeq_qgate.h): seeqdevScanQualityGate and the entries
 * that serve its arrays.  The gate reads the record array of a tally source (tally_source, seeq_tally_host.h) and writes arrays of its
 * own -- the kinds of the source's records, the passed records and their offsets -- which SEEQDEV_TALLY_GATED then names to the five tally
 * entries.  Included by seeq_device.hip behind seeq_tally_host.h.
 */
#ifndef SEEQ_QGATE_HOST_H_
#define SEEQ_QGATE_HOST_H_

static int qgate_fail(const char *what, const QGateCnt &h, uint32_t n)
{
   snprintf(g_last_error, sizeof g_last_error,
            "internal inconsistency in the quality gate (%s: %u spans, %u passed, %u low, %u long, %u far, %u misfit, %u placed)", what, n, h.npassed, h.nlow,
            h.nlong, h.nfar, h.nmisfit, h.placed);
   errno = EIO;
   return -1;
}

/* The gate over the n spans rec / off of text[0 .. nbytes): the kinds in qg_kind, the passed records in qg_rec / qg_off.  Waits. */
static int qgate_run(seeqdev_scan *s, const uint4 *rec, const uint64_t *off, uint32_t n, const void *d_text, size_t nbytes, uint32_t thr, uint32_t max_low,
                     uint32_t reach, seeqdev_qgate_counts_t *counts)
{
   const hipStream_t st = s->stream;
   memset(counts, 0, sizeof *counts);
   counts->nspans = n;
   if (!n) return 0;                                       /* no spans: nothing is launched */
   if (ws_make(&s->ws, {{s->d_qgcnt, sizeof(QGateCnt)}, {s->h_qgcnt, sizeof(QGateCnt), WS_PINNED}})) return -1;
   const size_t nt = (size_t)seeq_tiles_of(n);
   if (ws_grow(&s->ws, &s->cap_qg, n, {{s->qg_kind, (size_t)n}, {s->qg_bsum, (nt + 1) * SEEQ_QGATE_SUMS * sizeof(uint32_t)}})) return -1;
   QGateArgs a;
   memset(&a, 0, sizeof a);
   a.rec = rec; a.off = off; a.n = n; a.nt = (uint32_t)nt;
   a.text = (const uint8_t *)d_text; a.nbytes = nbytes;
   a.thr = thr; a.max_low = max_low; a.reach = reach; a.steps = qgate_steps(reach);
   a.kind = s->qg_kind; a.bsum = s->qg_bsum;
   a.cnt = s->d_qgcnt;
   if ((size_t)n > s->cap_qg || seeq_tiles_of(s->cap_qg) < nt) {
      snprintf(g_last_error, sizeof g_last_error, "quality gate: %u spans, arrays for %zu", n, s->cap_qg);
      errno = EIO;
      return -1;
   }
   if (s->tm_qg.begin(s->prof, st)) return -1;
   HIP_TRY(hipMemsetAsync(s->d_qgcnt, 0, sizeof(QGateCnt), st), EIO);
   hipLaunchKernelGGL(k_qgate_reduce, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_qgate_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
   if (counters_fetch(s, s->h_qgcnt, s->d_qgcnt, sizeof(QGateCnt))) return -1;
   QGateCnt h = *s->h_qgcnt;
   if (h.bad) {
      snprintf(g_last_error, sizeof g_last_error, "quality gate: a span lies outside the %zu bytes of text it was given", nbytes);
      errno = EIO;
      return -1;
   }
   if ((uint64_t)h.npassed + h.nlow + h.nlong + h.nfar + h.nmisfit != n) return qgate_fail("kinds", h, n);
   if (h.npassed) {
      /* the passed records: a group of its own, grown now that their number is known */
      const size_t np = h.npassed;
      if (ws_grow(&s->ws, &s->cap_qg_out, np, {{s->qg_rec, np * sizeof(uint4)}, {s->qg_off, np * sizeof(uint64_t)}})) return -1;
      a.out = s->qg_rec; a.off_out = s->qg_off; a.np = h.npassed;
      hipLaunchKernelGGL(k_qgate_apply, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
      if (counters_copy(s, s->h_qgcnt, s->d_qgcnt, sizeof(QGateCnt))) return -1;
   }
   if (s->tm_qg.end(s->prof, st)) return -1;
   HIP_TRY(hipStreamSynchronize(st), EIO);
   s->tm_qg.read(s->prof);
   if (h.npassed) {
      h = *s->h_qgcnt;
      if (h.placed != h.npassed) return qgate_fail("apply", h, n);
   }
   counts->npassed = h.npassed; counts->nlow = h.nlow; counts->nlong = h.nlong; counts->nfar = h.nfar; counts->nmisfit = h.nmisfit;
   counts->low_bases = h.low_bases;
   return 0;
}

extern "C" int seeqdevScanQualityGate(seeqdev_scan_t *s, int source, const void *d_text, size_t nbytes, uint32_t min_qual, uint32_t base, uint32_t max_low,
                                      uint32_t reach, seeqdev_qgate_counts_t *counts)
{
   const uint4 *rec;
   const uint64_t *off;
   uint64_t n;
   seeqerr = 0;
   if ((source != SEEQDEV_TALLY_INSERTS && source != SEEQDEV_TALLY_HITS && source != SEEQDEV_TALLY_ANCHORED) || (uint64_t)base + min_qual > 255u || reach < 1u || reach > SEEQ_QGATE_REACH_MAX) {
      errno = EINVAL;
      return -1;
   }
   if (tally_enter(s, counts, source, NULL, &d_text, &nbytes, &rec, &off, &n)) return -1;
   s->qg_done = false;                                     /* (the arrays of the gate before are gone, whatever comes of this one) */
   s->qg_n = s->qg_nsrc = 0;
   s->tm_qg.ms = 0.f;
   if (qgate_run(s, rec, off, (uint32_t)n, d_text, nbytes, base + min_qual, max_low, reach, counts)) return -1;
   s->qg_n = (size_t)counts->npassed;
   s->qg_nsrc = (size_t)n;
   s->qg_from_inserts = source == SEEQDEV_TALLY_INSERTS || (source == SEEQDEV_TALLY_ANCHORED && s->an_from_inserts);      /* (cut from inserts: still theirs) */
   s->qg_done = true;                                      /* (a gate that passed nothing included) */
   return 0;
}

extern "C" const seeqdev_hit_t *seeqdevScanGatedDevice(const seeqdev_scan_t *s) { return s && s->qg_done && s->qg_n ? (const seeqdev_hit_t *)s->qg_rec : NULL; }

extern "C" int seeqdevScanCopyGated(seeqdev_scan_t *s, void *host_out, size_t first, size_t n)
{
   return copy_out(s, host_out, s ? s->qg_rec : NULL, sizeof(uint4), s && s->qg_done ? s->qg_n : 0, first, n);
}

extern "C" int seeqdevScanCopyGatedOffsets(seeqdev_scan_t *s, uint64_t *host_out, size_t first, size_t n)
{
   return copy_out(s, host_out, s ? s->qg_off : NULL, sizeof(uint64_t), s && s->qg_done ? s->qg_n : 0, first, n);
}

extern "C" int seeqdevScanCopyGateKinds(seeqdev_scan_t *s, uint8_t *host_out, size_t first, size_t n)
{
   return copy_out(s, host_out, s ? s->qg_kind : NULL, sizeof(uint8_t), s && s->qg_done ? s->qg_nsrc : 0, first, n);
}

extern "C" int seeqdevScanLastQualityGateMs(const seeqdev_scan_t *s, float *ms)
{
   if (!s || !ms) { errno = EINVAL; return -1; }
   *ms = s->tm_qg.ms;
   return 0;
}

#endif
