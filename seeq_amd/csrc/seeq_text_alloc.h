/*
 * seeq_text_alloc.h -- memory for a caller's text: page-locked staging buffers (seeqdevHostAlloc) and device memory for resident text chosen
 * by a placement probe (seeqdevTextAllocFor).  Included by seeq_device.hip behind its entry points: the probe scans through the public
 * entries and reaches into the context (struct seeqdev_scan) only to hand a borrowed one back (scan_forget: the demultiplexer's too).
 */
#ifndef SEEQ_TEXT_ALLOC_H_
#define SEEQ_TEXT_ALLOC_H_

/* Page-locked host memory for staging buffers (H2D at link speed instead of through a bounce buffer). */
extern "C" void *seeqdevHostAlloc(size_t bytes)
{
   /* Called from seeqFileMatch's READER THREAD (seeq_file.c slot_reserve): seeqerr is the reference's plain global (libseeq.h:38) and belongs to the
      caller's thread -- this entry reports through errno (thread-local) alone; seeq_file.c clears seeqerr where it hands the failure to the caller. */
   void *p = NULL;
   hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable);      /* every device may copy from it */
   if (e != hipSuccess) { snprintf(g_last_error, sizeof g_last_error, "hipHostMalloc: %s", hipGetErrorString(e)); errno = ENOMEM; return NULL; }
   return p;
}

extern "C" void seeqdevHostFree(void *p)
{
   if (p) (void)hipHostFree(p);
}

/* A context borrowed for scans of patterns it does not own: nothing of them is left to fetch, re-run or copy */
static void scan_forget(seeqdev_scan *s)
{
   s->pat = nullptr;
   s->ran = false;
   memset(&s->counts, 0, sizeof s->counts);
}

/* Device memory for RESIDENT TEXT, chosen by measurement.  The scan kernel's time follows the physical pages a buffer gets from the driver
 * (0.77 / 0.87 / 0.92 ms per 3.75 GiB for the same text, stable for the life of the allocation; power-of-two blocks are fast far more often
 * than requests of an odd size: DESIGN.md section 5 (i)-(l)), so a caller that keeps text resident chooses its buffer once: up to twelve
 * candidate allocations (the plain one, then blocks of p bytes, p = the power of two >= bytes), each filled with synthetic reads and
 * scanned twice with the benchmark pattern; the one whose scan kernel was fastest is returned, the
 * others are freed.  probe_ms (may be NULL): the candidates' scan-kernel times, *nprobed of them.  The buffer's contents are undefined. */
extern "C" void *seeqdevTextAllocFor(seeqdev_scan_t *scan, size_t bytes, int candidates, seeqdev_textinfo_t *info)
{
   seeqerr = 0;
   if (info) memset(info, 0, sizeof *info);
   if (bytes == 0) bytes = 1;
   void *blk[12] = {nullptr};
   size_t blk_bytes[12] = {0};
   float ms[12] = {0};
   int n = 0;
   if (candidates > 12) candidates = 12;
   if (candidates < 2 || bytes < ((size_t)64 << 20)) candidates = 1;      /* (nothing to tell apart on a scan of microseconds) */
   size_t p2 = 1;
   while (p2 < bytes) p2 <<= 1;
   /* what the probing scan context allocates beside the candidates (reserve_impl for one segment of `bytes`: per-line, per-hit-line, per-tile arrays
      and the records: about 0.46 bytes per text byte of a segment), kept free while the candidates are taken */
   seeqdev_scan_t *sc = nullptr;
   const size_t seg = bytes < (size_t)0xF0000000u ? bytes : (size_t)0xF0000000u;
   const size_t headroom = seg / 2 + ((size_t)256 << 20);
   size_t peak = 0;
   for (int i = 0; i < candidates; i++) {
      size_t want = bytes;
      if (i > 0) {
         want = p2;
         size_t freeb = 0, total = 0;
         if (hipMemGetInfo(&freeb, &total) != hipSuccess) break;
         if (want + headroom > freeb) { want = bytes; if (want + headroom > freeb) break; }
      }
      if (hipMalloc(&blk[n], want) != hipSuccess) { (void)hipGetLastError(); blk[n] = nullptr; break; }
      blk_bytes[n] = want;
      peak += want;
      n++;
   }
   if (n == 0) { hip_fail(hipErrorOutOfMemory, "seeqdevTextAlloc", ENOMEM); return NULL; }
   int best = 0;
   if (n > 1) {
      static const char plain[] = "GATGTAGCGCGATTAGCCTG";
      char keys[20];
      for (int i = 0; i < 20; i++) keys[i] = plain[i] == 'A' ? 1 : plain[i] == 'C' ? 2 : plain[i] == 'G' ? 4 : 8;
      seeqdev_pattern_t *pat = seeqdevPatternNew(keys, 20, 3);
      /* Round 5: the launch time is a property of the PAIR (text buffer, scan context's workspace) -- the same text runs at 0.72 or 0.84 ms with
         two contexts of one process, reproducibly (profiles/r05/workspace_probe.txt) -- so a caller that scans the text with a context of its own
         (`scan`: reserve it first, so that its workspace is the one that stays) has the candidates probed with THAT context, and is left with no scan to fetch;
         NULL: a context made here. */
      sc = pat ? (scan ? scan : seeqdevScanNew(NULL)) : NULL;
      const bool own_sc = scan == nullptr;
      const bool prof_was = sc ? sc->prof : false;
      const uint64_t nreads = bytes / 151;
      bool ok = pat && sc && nreads > 0 && seeqdevScanSetProfiling(sc, 1) == 0;
      for (int i = 0; ok && i < n; i++) {
         ok = seeqdevSynthReads(blk[i], 0, nreads, 150, plain, 20, 3, 0x5EE92025ull, NULL) == 0 && hipStreamSynchronize(NULL) == hipSuccess;
         for (int rep = 0; ok && rep < 2; rep++) {
            seeqdev_counts_t cnt;
            ok = seeqdevScanRun(sc, pat, blk[i], (size_t)nreads * 151, SQ_BEST, SEEQDEV_WANT_COUNTLINES) == 0 && seeqdevScanFetch(sc, &cnt) == 0;
         }
         float t[4] = {0, 0, 0, 0};
         if (ok) ok = seeqdevScanLastTimes(sc, t) == 0;
         ms[i] = t[1];
      }
      if (sc && own_sc) seeqdevScanFree(sc);
      else if (sc) { (void)seeqdevScanSetProfiling(sc, prof_was ? 1 : 0); scan_forget(sc); }
      if (pat) seeqdevPatternFree(pat);
      if (ok) {
         for (int i = 1; i < n; i++) if (ms[i] < ms[best]) best = i;
         if (info) { for (int i = 0; i < n; i++) info->probe_ms[i] = ms[i]; info->nprobed = n; }
      }                                                     /* (a failed probe: the plain allocation, nprobed = 0) */
      for (int i = 0; i < n; i++) if (i != best) (void)hipFree(blk[i]);
      seeqerr = 0;
   }
   if (info) { info->chosen = best; info->allocated_bytes = blk_bytes[best]; info->probe_peak_bytes = n > 1 ? peak + headroom : peak; }
   return blk[best];
}

extern "C" void *seeqdevTextAllocInfo(size_t bytes, int candidates, seeqdev_textinfo_t *info) { return seeqdevTextAllocFor(NULL, bytes, candidates, info); }

extern "C" void *seeqdevTextAlloc(size_t bytes, int candidates, float *probe_ms, int *nprobed)
{
   seeqdev_textinfo_t info;
   void *p = seeqdevTextAllocInfo(bytes, candidates, &info);
   if (nprobed) *nprobed = p ? info.nprobed : 0;
   if (p && probe_ms) for (int i = 0; i < info.nprobed; i++) probe_ms[i] = info.probe_ms[i];
   return p;
}

extern "C" void seeqdevTextFree(void *d_text)
{
   if (d_text) (void)hipFree(d_text);
}

#endif
