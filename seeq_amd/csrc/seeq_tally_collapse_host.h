/*
 * seeq_tally_collapse_host.h -- the host driver of the collapse behind the grouped tally (rule and kernels: seeq_tally_collapse.h): the
 * parents of the pairs of the context's last grouped call, the prefix over them, the group rows, one counters copy with its checks, and the
 * seeqdevScanTallyCollapse / seeqdevScanTallyParentsDevice / seeqdevScanTallyCollapseDevice / seeqdevScanCopyTallyParents /
 * seeqdevScanCopyTallyCollapse / seeqdevScanLastTallyCollapseMs entries.  Included by seeq_device.hip behind seeq_tally_library_host.h.
 */
#ifndef SEEQ_TALLY_COLLAPSE_HOST_H_
#define SEEQ_TALLY_COLLAPSE_HOST_H_

static int tally_collapse_fail(const char *what, const CollapseCnt &h, size_t np, size_t ng, uint64_t npaired)
{
   snprintf(g_last_error, sizeof g_last_error,
            "internal inconsistency in the collapse (%s: flags %u, %zu pairs, %zu groups, %llu paired, %u roots, %u absorbed, %llu absorbed reads, "
            "%u roots and %llu absorbed reads by the tiles, %u roots by the group rows, %u groups without a root)",
            what, h.bad, np, ng, (unsigned long long)npaired, h.nroots, h.nabsorbed, (unsigned long long)h.reads, h.sroots, (unsigned long long)h.sreads,
            h.groots, h.noroot);
   errno = EIO;
   return -1;
}

/* The parents and the group rows of the np > 0 pairs and ng > 0 groups of the context's tables (tc_parent: tc_np, tc_groups: tc_ng are the
   result).  Waits. */
static int tally_collapse_run(seeqdev_scan *s, int rule, seeqdev_tally_collapse_counts_t *counts)
{
   const hipStream_t st = s->stream;
   const size_t np = s->tg_np, ng = s->tg_ng;
   const size_t nt = (size_t)seeq_tiles_of(np), nwg = (size_t)collapse_workgroups(np), ngwg = (ng + SEEQ_TILE_WG - 1) / SEEQ_TILE_WG;
   if (ws_make(&s->ws, {{s->d_tccnt, sizeof(CollapseCnt)}, {s->h_tccnt, sizeof(CollapseCnt), WS_PINNED}})) return -1;
   if (ws_grow(&s->ws, &s->cap_tc, np, {{s->tc_parent, np * sizeof(uint32_t)}, {s->tc_proot, np * sizeof(uint32_t)}, {s->tc_pread, np * sizeof(uint64_t)},
                                        {s->tc_rsum, nt * sizeof(uint32_t)}, {s->tc_qsum, nt * sizeof(uint64_t)}, {s->tc_wst, nwg * sizeof(CollapseWg)}})) return -1;
   if (ws_grow(&s->ws, &s->cap_tc_groups, ng, {{s->tc_groups, ng * sizeof(seeqdev_tally_collapse_t)}, {s->tc_gst, ngwg * sizeof(uint4)}})) return -1;
   if (np > 0xFFFFFFFFull || ng > np || np > s->cap_tc || ng > s->cap_tc_groups || np > s->cap_tg_pairs || ng > s->cap_tg_groups) {
      snprintf(g_last_error, sizeof g_last_error, "collapse: %zu pairs, arrays for %zu, a table of %zu; %zu groups, arrays for %zu, a table of %zu", np, s->cap_tc,
               s->cap_tg_pairs, ng, s->cap_tc_groups, s->cap_tg_groups);
      errno = EIO;
      return -1;
   }
   CollapseArgs a;
   memset(&a, 0, sizeof a);
   a.ptab = (const uint64_t *)s->tg_pairs; a.gtab = (const uint64_t *)s->tg_groups;
   a.np = (uint32_t)np; a.ng = (uint32_t)ng;
   a.rule = (uint32_t)rule;
   a.gstride = tally_lib_stride(a.ng); a.gprobes = tally_lib_probes(a.gstride);
   a.probes = tally_lib_probes(a.np);
   a.nwg = (uint32_t)nwg; a.nt = (uint32_t)nt; a.ngwg = (uint32_t)ngwg;
   a.parent = s->tc_parent; a.proot = s->tc_proot; a.pread = s->tc_pread;
   a.rsum = s->tc_rsum; a.qsum = s->tc_qsum;
   a.wst = s->tc_wst; a.gst = s->tc_gst;
   a.groups = (uint4 *)s->tc_groups;
   a.cnt = s->d_tccnt;
   if (s->tm_tc.begin(s->prof, st)) return -1;
   HIP_TRY(hipMemsetAsync(s->d_tccnt, 0, sizeof(CollapseCnt), st), EIO);
   hipLaunchKernelGGL(k_collapse_parent, dim3(a.nwg), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_collapse_prefix_reduce, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_collapse_prefix_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_collapse_prefix_apply, dim3(a.nt), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_collapse_groups, dim3(a.ngwg), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_collapse_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
   if (counters_copy(s, s->h_tccnt, s->d_tccnt, sizeof(CollapseCnt))) return -1;
   if (s->tm_tc.end(s->prof, st)) return -1;
   HIP_TRY(hipStreamSynchronize(st), EIO);
   s->tm_tc.read(s->prof);
   const CollapseCnt h = *s->h_tccnt;
   counts->nroots = h.nroots; counts->nabsorbed = h.nabsorbed; counts->absorbed_reads = h.reads;
   /* every pair is one of the two; the tiles' prefix and the group rows saw the same roots and reads as the parents' workgroups; an
      absorbed read is a paired one; every group keeps its first pair in the order */
   if (h.bad || (uint64_t)h.nroots + h.nabsorbed != np || h.sroots != h.nroots || h.sreads != h.reads || h.groots != h.nroots || h.reads > s->tg_npaired ||
       h.noroot || h.nroots < ng)
      return tally_collapse_fail("totals", h, np, ng, s->tg_npaired);
   s->tc_np = np; s->tc_ng = ng;
   return 0;
}

extern "C" int seeqdevScanTallyCollapse(seeqdev_scan_t *s, int rule, seeqdev_tally_collapse_counts_t *counts)
{
   seeqerr = 0;
   if (!s || !counts || (rule != SEEQDEV_COLLAPSE_DIRECTIONAL && rule != SEEQDEV_COLLAPSE_ANY)) { errno = EINVAL; return -1; }
   if (!s->tg_done) {
      snprintf(g_last_error, sizeof g_last_error, "collapse: the context holds no completed grouped call (seeqdevScanTallyGrouped)");
      errno = EINVAL;
      return -1;
   }
   s->tc_np = s->tc_ng = 0;                                /* (the result of the collapse before is gone, whatever comes of this one) */
   s->tm_tc.ms = 0.f;
   memset(counts, 0, sizeof *counts);
   counts->npairs = s->tg_np; counts->ngroups = s->tg_ng;
   counts->rule = (uint32_t)rule; counts->max_len = s->tg_max_len;
   if (!s->tg_np) return 0;                                /* nothing paired: nothing is launched, the result is empty */
   if (use_device(s->device)) return -1;
   return tally_collapse_run(s, rule, counts);
}

extern "C" const uint32_t *seeqdevScanTallyParentsDevice(const seeqdev_scan_t *s) { return s ? s->tc_parent : NULL; }

extern "C" const seeqdev_tally_collapse_t *seeqdevScanTallyCollapseDevice(const seeqdev_scan_t *s) { return s ? s->tc_groups : NULL; }

extern "C" int seeqdevScanCopyTallyParents(seeqdev_scan_t *s, uint32_t *host_out, size_t first, size_t n)
{
   return copy_out(s, host_out, s ? s->tc_parent : NULL, sizeof(uint32_t), s ? s->tc_np : 0, first, n);
}

extern "C" int seeqdevScanCopyTallyCollapse(seeqdev_scan_t *s, seeqdev_tally_collapse_t *host_out, size_t first, size_t n)
{
   return copy_out(s, host_out, s ? s->tc_groups : NULL, sizeof(seeqdev_tally_collapse_t), s ? s->tc_ng : 0, first, n);
}

extern "C" int seeqdevScanLastTallyCollapseMs(const seeqdev_scan_t *s, float *ms)
{
   if (!s || !ms) { errno = EINVAL; return -1; }
   *ms = s->tm_tc.ms;
   return 0;
}

#endif
