/*
 * seeq_device.hip -- the device-level C-ABI (include/seeq_amd.h) of seeq-mi355x: ONE
 * translation unit, the kernels and the drivers of the side entries in headers.  Written for gfx950 (MI355X, CDNA4): 64-wide wavefronts,
 * one text line per lane, wave ballots for per-line flags, LDS for the Peq and
 * class tables.  Integer/bitwise work only -- no MFMA.
 *
 * Pipeline of one seeqdevScanRun over a text buffer resident in HBM, per
 * segment of < 4 GiB (all offsets inside a segment are u32):
 *
 *   K0  k_nl_count / k_nl_write      newline index -> line_start[]        (HBM stream)
 *   K1  k_forward<W>                 one line per lane: Myers column per character,
 *                                    acceptance rules; ballot -> hitmask[] (1 bit/line)
 *   K2  scan of popc(hitmask)        ordered ranks of hit lines
 *   K3  k_compact                    hitlines[]
 *   K4  k_exact<W,COUNT>             (SQ_ALL / COUNTMATCH) hits per hit line, then scan
 *   K5  k_exact<W,EMIT>              acceptance rules + reverse start recovery -> records[]
 *
 * (the generic path: seeq_generic.h, seeq_scan.h; the one-pass kernels that serve most
 * scans: seeq_pair.h, seeq_stream.h, seeq_direct.h) replacing the reference's per-line
 * loop seeq.c:361-387 -> libseeq.c:171-352.  There is no host-side matcher: without a
 * GPU every entry point fails.
 *
 * Here: plumbing, pattern handle, scan context, the segment and packed drivers, the scan
 * entries.  The side entries are included where they belong in that order: seeq_synth.h,
 * seeq_text_alloc.h, seeq_multi_host.h, seeq_demux_host.h, seeq_strand_host.h, seeq_insert_host.h,
 * seeq_tally_host.h, seeq_tally_group_host.h, seeq_tally_library_host.h (and behind it seeq_tally_append_host.h), seeq_tally_collapse_host.h,
 * seeq_string.h.
 */
#include <hip/hip_runtime.h>

#include <errno.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "seeq_amd.h"
#include "seeq_kernel_core.h"
extern "C" {
#include "seeq_pattern.h"
}

/* ========================================================================== */
/* Error plumbing                                                             */
/* ========================================================================== */
static thread_local char g_last_error[256] = "";

static int hip_fail(hipError_t e, const char *what, int err_no)
{
   snprintf(g_last_error, sizeof g_last_error, "%s: %s", what, hipGetErrorString(e));
   seeqerr = 0;
   errno = err_no;
   return -1;
}

#define HIP_TRY(call, err_no)                                        \
   do {                                                              \
      hipError_t e_ = (call);                                        \
      if (e_ != hipSuccess) return hip_fail(e_, #call, (err_no));    \
   } while (0)

extern "C" const char *seeqdevLastError(void) { return g_last_error; }

/* Every entry point that takes a scan context or a pattern runs on THAT object's device, whatever device the calling
 * thread used last (a caller that spreads chunks over several GPUs goes from one context to the next). */
static int use_device(int device)
{
   int cur = -1;
   if (hipGetDevice(&cur) == hipSuccess && cur == device) return 0;
   HIP_TRY(hipSetDevice(device), ENODEV);
   return 0;
}

extern "C" int seeqdevDeviceCount(void)
{
   int n = 0;
   if (hipGetDeviceCount(&n) != hipSuccess) return 0;
   return n;
}

extern "C" int seeqdevSetDevice(int device)
{
   HIP_TRY(hipSetDevice(device), ENODEV);
   return 0;
}

#include "seeq_types.h"
#include "seeq_scan_common.h"

static constexpr int WG = 256;           /* 4 waves */
static constexpr int TILE = 16384;       /* bytes per newline-index workgroup: 64 B per thread */
static constexpr size_t FUSED_MIN_TILE = 512;    /* smallest text tile / region of the one-pass kernels */
static constexpr int STREAM_NW_HOST = 16;         /* = STREAM_NW (seeq_stream.h): waves per k_stream workgroup */
static constexpr uint32_t STREAM_CH_HOST = 128;    /* bytes per lane of k_stream / k_pair */
static constexpr size_t MAX_FUSED_GRID = 16384;   /* upper bound of the waves (= hit slices) of a persistent scan grid */
static constexpr size_t SAMPLE_BYTES = 65536;     /* prefix sampled to estimate the line length */

#include "seeq_generic.h"
#include "seeq_scan.h"
#include "seeq_fused_post.h"
#include "seeq_direct.h"
#include "seeq_exact1.h"
#include "seeq_stream.h"
#include "seeq_pair.h"
#include "seeq_packed.h"
#include "seeq_multi.h"
#include "seeq_demux.h"
#include "seeq_tiles.h"
#include "seeq_fastq.h"
#include "seeq_strand.h"
#include "seeq_insert.h"
#include "seeq_tally.h"
#include "seeq_tally_group.h"
#include "seeq_tally_append.h"
#include "seeq_tally_library.h"
#include "seeq_tally_collapse.h"
#include "seeq_tally_held.h"
#include "seeq_qgate.h"
#include "seeq_anchor.h"
static_assert(SEEQ_ANCHOR_AFTER == SEEQDEV_ANCHOR_AFTER && SEEQ_ANCHOR_BEFORE == SEEQDEV_ANCHOR_BEFORE && SEEQ_ANCHOR_LINE == SEEQDEV_ANCHOR_LINE &&
              SEEQ_ANCHOR_KEPT == SEEQDEV_ANCHOR_KEPT && SEEQ_ANCHOR_SHORT == SEEQDEV_ANCHOR_SHORT && SEEQ_ANCHOR_FAR == SEEQDEV_ANCHOR_FAR, "the anchor's constants");
static_assert(sizeof(seeqdev_tally_pair_t) == 24 && sizeof(seeqdev_tally_group_t) == 24, "pair and group entries are written as three 64-bit words");
static_assert(sizeof(seeqdev_tally_collapse_t) == sizeof(uint4) && SEEQ_COLLAPSE_DIRECTIONAL == SEEQDEV_COLLAPSE_DIRECTIONAL && SEEQ_COLLAPSE_ANY == SEEQDEV_COLLAPSE_ANY,
              "collapse rows are written as uint4");
static_assert(sizeof(seeqdev_demux_t) == 16 && sizeof(seeqdev_hit_t) == sizeof(uint4), "demux records are written as uint4");
static_assert(sizeof(seeqdev_insert_t) == sizeof(uint4), "insert records are written as uint4");
static_assert(sizeof(seeqdev_tally_t) == sizeof(uint4) && SEEQ_TALLY_LEN_MAX == SEEQDEV_TALLY_MAX_LEN, "tally entries are written as uint4");
#include "seeq_post.h"
static_assert(STREAM_NW == STREAM_NW_HOST, "waves per k_stream workgroup");
extern "C" {
#include "seeq_dfa.h"
}
#include "seeq_synth.h"

/* ========================================================================== */
/* Pattern handle                                                             */
/* ========================================================================== */
static unsigned long g_pattern_ids = 0;    /* one per seeqdevPatternNew: cache key (a freed pattern's address can come back) */

struct seeqdev_pattern {
   unsigned long id;
   int       wlen, tau, words;
   int       device;
   uint32_t *d_peq;          /* [2][5][words] */
   char     *keys;           /* host copy of the key bytes (DFA construction) */
   uint32_t *h_peq;          /* host copy of d_peq */
   int       sdfa_state;     /* the streaming automaton of k_stream (seeq_dfa.h): 0 not tried, 1 built, -1 none fits */
   uint16_t *d_sdfa;         /* transition table in HBM, staged into LDS by k_stream */
   uint16_t *d_sdfa_skip;    /* its skip variant (SQ_IGNORE: column 4 maps every state onto itself) */
   uint16_t *d_sdfa_restart; /* a filter's restart variant (long lines: acceptance goes on from the root, every part occurrence is flagged) */
   uint32_t  sdfa_rows, sdfa_final_base;
   int       sdfa_parts;     /* 1: the complete automaton (exact verdicts); > 1: partition filter (candidates) */
   int       sdfa_warm;      /* bytes of warm-up a chunk walk needs */
   double    sdfa_pacc;      /* filter: probability that a random DNA character completes a candidate */
   int       pair_state;     /* the pair automaton of k_pair (seeq_dfa.h section 3): 0 not tried, 1 built, -1 none fits */
   uint16_t *d_pair;         /* its table in HBM (32-byte rows), staged into LDS by k_pair */
   uint32_t  pair_units;     /* 16-byte units of the table (2 per row) */
   uint32_t  pair_states;
   int       pair_parts, pair_mp, pair_warm;
   double    pair_pacc;      /* probability that a random DNA character completes a candidate */
   int       quad_state;     /* the quad automaton of the packed walk (seeq_dfa.h section 3b): 0 not tried, 1 built, -1 none fits */
   uint16_t *d_quad;         /* its table in HBM (512-byte rows) */
   uint32_t  quad_units;     /* 16-byte units of it */
   uint32_t  quad_states;
   int       quad_parts, quad_mp;
   double    quad_pacc;
   pthread_mutex_t plan_lock;   /* the automata are built on first use; scan contexts on several threads may share a pattern */
   struct seeqdev_pattern *twin;   /* the reverse complement (seeq_strand_host.h): built by the first both-strands scan, owned */
};

/* FN<W>(...) for the W that holds a pattern of `words` Peq words: the five instances of the kernels templated on it (k_forward, k_exact, k_string) */
#define SEEQ_FOR_WORDS(words, FN, ...) \
   ((words) <= 1 ? FN<1>(__VA_ARGS__) : (words) <= 2 ? FN<2>(__VA_ARGS__) : (words) <= 4 ? FN<4>(__VA_ARGS__) : (words) <= 8 ? FN<8>(__VA_ARGS__) : FN<16>(__VA_ARGS__))

extern "C" seeqdev_pattern_t *seeqdevPatternNew(const char *keys, int wlen, int tau)
{
   seeqerr = 0;
   if (!keys || wlen < 1 || tau < 0 || tau >= wlen) { errno = EINVAL; return NULL; }
   if (wlen > SEEQDEV_MAX_WLEN) {
      snprintf(g_last_error, sizeof g_last_error, "pattern longer than %d positions", SEEQDEV_MAX_WLEN);
      errno = E2BIG;
      return NULL;
   }
   if (seeqdevDeviceCount() < 1) {
      snprintf(g_last_error, sizeof g_last_error, "no HIP device: seeq-mi355x has no CPU matcher");
      errno = ENODEV;
      return NULL;
   }
   seeqdev_pattern *p = (seeqdev_pattern *)calloc(1, sizeof *p);
   if (!p) return NULL;
   p->id = __atomic_add_fetch(&g_pattern_ids, 1ul, __ATOMIC_RELAXED);
   pthread_mutex_init(&p->plan_lock, NULL);
   p->wlen = wlen; p->tau = tau; p->words = seeq_words_for(wlen);
   p->keys = (char *)malloc((size_t)wlen);
   if (p->keys) memcpy(p->keys, keys, (size_t)wlen);
   const size_t nw = (size_t)10 * p->words;
   uint32_t *h = (uint32_t *)malloc(nw * sizeof(uint32_t));
   char *rkeys = (char *)malloc((size_t)wlen);
   if (!h || !rkeys || !p->keys) { free(h); free(rkeys); free(p->keys); free(p); errno = ENOMEM; return NULL; }
   for (int i = 0; i < wlen; i++) rkeys[i] = keys[wlen - 1 - i];     /* reference libseeq.c:89 */
   seeq_build_peq(keys, wlen, p->words, h);
   seeq_build_peq(rkeys, wlen, p->words, h + 5 * p->words);
   hipError_t e = hipGetDevice(&p->device);
   if (e == hipSuccess) e = hipMalloc((void **)&p->d_peq, nw * sizeof(uint32_t));
   if (e == hipSuccess) e = hipMemcpy(p->d_peq, h, nw * sizeof(uint32_t), hipMemcpyHostToDevice);
   free(rkeys);
   p->h_peq = h;
   if (e != hipSuccess) {
      hip_fail(e, "seeqdevPatternNew", e == hipErrorOutOfMemory ? ENOMEM : EIO);
      if (p->d_peq) (void)hipFree(p->d_peq);
      free(p->keys);
      free(h);
      free(p);
      return NULL;
   }
   return p;
}

extern "C" int seeqdevPatternDevice(const seeqdev_pattern_t *p) { return p ? p->device : -1; }

extern "C" void seeqdevPatternFree(seeqdev_pattern_t *p)
{
   if (!p) return;
   if (p->twin) seeqdevPatternFree(p->twin);
   (void)use_device(p->device);
   if (p->d_peq) (void)hipFree(p->d_peq);
   if (p->d_sdfa) (void)hipFree(p->d_sdfa);
   if (p->d_sdfa_skip) (void)hipFree(p->d_sdfa_skip);
   if (p->d_sdfa_restart) (void)hipFree(p->d_sdfa_restart);
   if (p->d_pair) (void)hipFree(p->d_pair);
   if (p->d_quad) (void)hipFree(p->d_quad);
   pthread_mutex_destroy(&p->plan_lock);
   free(p->keys);
   free(p->h_peq);
   free(p);
}

/* The automata of a pattern are built on first use, once, under the pattern's lock (scan contexts on several threads
 * may share a pattern); a table is published -- state 1 -- only when all of it sits in HBM, and a failed upload frees
 * what it had allocated. */
static void pattern_plan_stream(seeqdev_pattern *mp, bool complete_only)
{
   pthread_mutex_lock(&mp->plan_lock);
   if (mp->sdfa_state == 0 && mp->keys) {
      int state = -1;
      seeq_dfa_t *d = seeq_dfa_plan_stream(mp->keys, mp->wlen, mp->tau, complete_only ? 1 : 0);
      if (d) {
         const size_t bytes = (size_t)d->nrows * 16;
         uint16_t *skip = seeq_dfa_skip_variant(d);
         uint16_t *rst = d->nparts > 1 ? seeq_dfa_restart_variant(d) : nullptr;
         uint16_t *t0 = nullptr, *t1 = nullptr, *t2 = nullptr;
         if (skip && (rst || d->nparts <= 1) && hipMalloc((void **)&t0, bytes) == hipSuccess && hipMemcpy(t0, d->table, bytes, hipMemcpyHostToDevice) == hipSuccess &&
             hipMalloc((void **)&t1, bytes) == hipSuccess && hipMemcpy(t1, skip, bytes, hipMemcpyHostToDevice) == hipSuccess &&
             (!rst || (hipMalloc((void **)&t2, bytes) == hipSuccess && hipMemcpy(t2, rst, bytes, hipMemcpyHostToDevice) == hipSuccess))) {
            mp->d_sdfa = t0; mp->d_sdfa_skip = t1; mp->d_sdfa_restart = t2;
            mp->sdfa_rows = d->nrows;
            mp->sdfa_final_base = d->acc_final;            /* state value of ACC_NEW */
            mp->sdfa_parts = d->nparts;
            mp->sdfa_warm = d->warm;
            mp->sdfa_pacc = d->p_accept;
            state = 1;
         } else {
            if (t0) (void)hipFree(t0);
            if (t1) (void)hipFree(t1);
            if (t2) (void)hipFree(t2);
         }
         free(skip);
         free(rst);
         seeq_dfa_free(d);
      }
      __atomic_store_n(&mp->sdfa_state, state, __ATOMIC_RELEASE);
   }
   pthread_mutex_unlock(&mp->plan_lock);
}

static void pattern_plan_pair(seeqdev_pattern *mp)
{
   pthread_mutex_lock(&mp->plan_lock);
   if (mp->pair_state == 0 && mp->keys) {
      int state = -1;
      seeq_pair_t *d = seeq_pair_plan(mp->keys, mp->wlen, mp->tau);
      if (d) {
         const size_t bytes = d->table_bytes;
         uint16_t *t0 = nullptr;
         if (hipMalloc((void **)&t0, bytes) == hipSuccess && hipMemcpy(t0, d->table, bytes, hipMemcpyHostToDevice) == hipSuccess) {
            mp->d_pair = t0;
            mp->pair_units = d->table_bytes / 16;
            mp->pair_states = d->nstates;
            mp->pair_parts = d->nparts; mp->pair_mp = d->mp; mp->pair_warm = d->warm;
            mp->pair_pacc = d->p_accept;
            state = 1;
         } else if (t0) {
            (void)hipFree(t0);
         }
         seeq_pair_free(d);
      }
      __atomic_store_n(&mp->pair_state, state, __ATOMIC_RELEASE);
   }
   pthread_mutex_unlock(&mp->plan_lock);
}

static void pattern_plan_quad(seeqdev_pattern *mp)
{
   pthread_mutex_lock(&mp->plan_lock);
   if (mp->quad_state == 0 && mp->keys) {
      int state = -1;
      seeq_quad_t *d = seeq_quad_plan(mp->keys, mp->wlen, mp->tau);
      if (d) {
         uint16_t *t0 = nullptr;
         if (hipMalloc((void **)&t0, d->table_bytes) == hipSuccess && hipMemcpy(t0, d->table, d->table_bytes, hipMemcpyHostToDevice) == hipSuccess) {
            mp->d_quad = t0;
            mp->quad_units = d->table_bytes / 16;
            mp->quad_states = d->nstates;
            mp->quad_parts = d->nparts; mp->quad_mp = d->mp;
            mp->quad_pacc = d->p_accept;
            state = 1;
         } else if (t0) {
            (void)hipFree(t0);
         }
         seeq_quad_free(d);
      }
      __atomic_store_n(&mp->quad_state, state, __ATOMIC_RELEASE);
   }
   pthread_mutex_unlock(&mp->plan_lock);
}

/* ---- one-pass multi-pattern scans: the automata of a pattern SET (seeq_dfa.h section 4, seeq_multi.h) ---- */
struct MultiPlan {
   int            npat;
   unsigned long  ids[SEEQ_MULTI_MAX];      /* generation ids of the patterns it was built for */
   int            state;                    /* 1 usable, -1 no union automaton for this set: a scan per pattern */
   seeqdev_pattern upat;                    /* the union as a pattern: what run_segments walks (wlen = maxspan, tau = 0: skip_back = maxspan) */
   uint16_t      *d_res_next;
   uint32_t      *d_res_mask;
   uint32_t       res_states;
   int            maxspan;
   int            m[SEEQ_MULTI_MAX], tau[SEEQ_MULTI_MAX], fw[SEEQ_MULTI_MAX];
   uint32_t      *d_eq;                     /* [npat][768 * 2] the patterns' EQ tables of the exact pass */
   int            eq_options;               /* the option bits d_eq was made for (-1: none yet) */
   uint32_t       pair_states, raw_states;
   int            lp_min, exact;
};

static void multi_plan_free(MultiPlan *mp)
{
   if (!mp) return;
   if (mp->d_res_next) (void)hipFree(mp->d_res_next);
   if (mp->d_res_mask) (void)hipFree(mp->d_res_mask);
   if (mp->d_eq) (void)hipFree(mp->d_eq);
   if (mp->upat.d_pair) (void)hipFree(mp->upat.d_pair);
   if (mp->upat.d_peq) (void)hipFree(mp->upat.d_peq);
   free(mp->upat.h_peq);
   free(mp);
}

/* The plan for this set (built once per set and context; a context keeps the plan of its last set). */
static MultiPlan *multi_plan_for(MultiPlan **slot, const seeqdev_pattern_t *const *pats, int npat)
{
   MultiPlan *mp = *slot;
   if (mp && mp->npat == npat) {
      bool same = true;
      for (int k = 0; k < npat; k++) same = same && mp->ids[k] == pats[k]->id;
      if (same) return mp;
   }
   multi_plan_free(mp);
   *slot = mp = (MultiPlan *)calloc(1, sizeof *mp);
   if (!mp) return NULL;
   mp->npat = npat;
   mp->state = -1;
   mp->eq_options = -1;
   for (int k = 0; k < npat; k++) mp->ids[k] = pats[k]->id;
   if (npat < 2 || npat > SEEQ_MULTI_MAX) return mp;
   const char *keys[SEEQ_MULTI_MAX];
   for (int k = 0; k < npat; k++) {
      if (!pats[k]->keys || pats[k]->wlen > FUSED_MAX_WLEN2) return mp;
      keys[k] = pats[k]->keys; mp->m[k] = pats[k]->wlen; mp->tau[k] = pats[k]->tau;
      mp->fw[k] = pats[k]->wlen <= FUSED_MAX_WLEN ? 1 : 2;
   }
   seeq_multi_t *d = seeq_multi_build(keys, mp->m, mp->tau, npat);
   if (!d) return mp;
   if (d->maxspan <= FUSED_MAX_WLEN2) {
      seeqdev_pattern &u = mp->upat;
      u.id = __atomic_add_fetch(&g_pattern_ids, 1ul, __ATOMIC_RELAXED);
      u.wlen = d->maxspan; u.tau = 0; u.words = seeq_words_for(d->maxspan);
      u.device = pats[0]->device;
      u.sdfa_state = -1;
      u.h_peq = (uint32_t *)calloc((size_t)10 * u.words, sizeof(uint32_t));
      bool ok = u.h_peq != NULL;
      ok = ok && hipMalloc((void **)&u.d_peq, (size_t)10 * u.words * sizeof(uint32_t)) == hipSuccess;
      ok = ok && hipMemset(u.d_peq, 0, (size_t)10 * u.words * sizeof(uint32_t)) == hipSuccess;
      ok = ok && hipMalloc((void **)&u.d_pair, d->pair->table_bytes) == hipSuccess;
      ok = ok && hipMemcpy(u.d_pair, d->pair->table, d->pair->table_bytes, hipMemcpyHostToDevice) == hipSuccess;
      ok = ok && hipMalloc((void **)&mp->d_res_next, (size_t)d->res_states * 16) == hipSuccess;
      ok = ok && hipMemcpy(mp->d_res_next, d->res_next, (size_t)d->res_states * 16, hipMemcpyHostToDevice) == hipSuccess;
      ok = ok && hipMalloc((void **)&mp->d_res_mask, (size_t)d->res_states * 4) == hipSuccess;
      ok = ok && hipMemcpy(mp->d_res_mask, d->res_mask, (size_t)d->res_states * 4, hipMemcpyHostToDevice) == hipSuccess;
      ok = ok && hipMalloc((void **)&mp->d_eq, (size_t)npat * 1536 * sizeof(uint32_t)) == hipSuccess;
      if (ok) {
         u.pair_state = 1;
         u.pair_units = d->pair->table_bytes / 16;
         u.pair_states = d->pair->nstates;
         u.pair_parts = npat; u.pair_mp = d->pair->mp; u.pair_warm = d->pair->warm;
         u.pair_pacc = d->pair->p_accept;
         mp->res_states = d->res_states;
         mp->maxspan = d->maxspan;
         mp->pair_states = d->pair->nstates; mp->raw_states = d->pair->nstates_raw;
         mp->exact = d->res_exact;
         mp->lp_min = d->lp[0];
         for (int k = 1; k < npat; k++) if (d->lp[k] < mp->lp_min) mp->lp_min = d->lp[k];
         mp->state = 1;
      }
   }
   seeq_multi_free(d);
   return mp;
}

/* ========================================================================== */
/* Scan context                                                               */
/* ========================================================================== */
#include "seeq_plan.h"          /* ScanKnobs, seeq_plan_scan: which kernels serve a scan (pure host code) */
#include "seeq_workspace.h"     /* Workspace: the owner of a context's buffers -- grouped growth, one free path (pure host code) */
#include "seeq_rerun.h"         /* the first reservation, what follows a run that came back void, the fall-back flags (pure host code) */

struct OccMemo { const void *fn; size_t lds; int per_cu; };

/* Two events around a stretch of a stream's work, for a context that profiles: every call is a no-op unless `on` (the context's profiling
   switch); the events are made on first use and go with the context (seeqdevScanFree). */
struct EventPair {
   hipEvent_t ev[2];
   bool       made;
   float      ms;                 /* what the last read() found; 0: nothing timed */
   int begin(bool on, hipStream_t st)
   {
      if (!on) return 0;
      if (!made) {
         HIP_TRY(hipEventCreate(&ev[0]), EIO);
         HIP_TRY(hipEventCreate(&ev[1]), EIO);
         made = true;
      }
      HIP_TRY(hipEventRecord(ev[0], st), EIO);
      return 0;
   }
   int end(bool on, hipStream_t st)
   {
      if (on) HIP_TRY(hipEventRecord(ev[1], st), EIO);
      return 0;
   }
   void read(bool on)             /* (behind a synchronise) */
   {
      ms = 0.f;
      if (on && made) (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
   }
};

/* Packed runs (seeq_packed.h), reads per segment: 64 Mi (16 Mi until the quad walk: the per-segment launches behind the walk -- the scan of the
   candidate counts, the list, k_nh_top, k_emit1 -- are latency-bound and cost as much for a quarter of the reads: 100 M reads, 2.28 ms per step
   in six segments, 2.11 in three, 2.07 in two; 8 bytes of workspace per read of a segment); SEEQ_PACKED_SEG_READS sets another size (tests) */
static constexpr size_t PACKED_SEG_READS_DEFAULT = (size_t)1 << 26;

struct seeqdev_scan {
   hipStream_t stream;
   bool        own_stream;
   int         device;            /* the HIP device this context (its stream, its workspace) lives on */
   EventPair   tm_h2d;            /* profiling: around the H2D copy of seeqdevScanHostBegin; .ms: of the last fetched scan */
   float      *launch_ms; size_t cap_launch_ms;      /* per forward-scan launch of the last fetched scan (profiling) */
   unsigned long long *clk_probe;  /* page-locked, 4 words per segment: the scan kernel's own clock readings (profiling; k_pair) */
   size_t      cap_clk_probe;
   float       clk_mhz;           /* core clock the last run's scan launches ran at (mean over the launches; 0: not measured) */
   bool        clk_valid;         /* the last run's scan kernel filled clk_probe (k_pair under profiling): else the readings are an earlier run's */
   int         ncu;               /* compute units of the device (cached) */
   size_t      lds_per_wg;        /* LDS a workgroup may allocate on it */
   size_t      lds_per_cu;        /* LDS of a compute unit (what a workgroup gets when it asks for it: hipFuncAttributeMaxDynamicSharedMemorySize) */
   ScanKnobs   knobs;
   OccMemo     occ[8]; int nocc;  /* hipOccupancyMaxActiveBlocksPerMultiprocessor results */
   bool        last_filter;       /* the last run walked a partition filter automaton */
   int         last_plan[16];     /* the last run's plan, as seeqdevScanLastPlan reports it (run_setup; a packed run: path 8 alone) */
   bool        last_packed_quad;  /* the last packed run walked the quad table */
   size_t      pk_seg_reads;      /* reads per segment of a packed run */
   Workspace   ws;                /* owns every device and page-locked buffer below: ws_grow / ws_make bring them into being, ws_free_all ends them */
   /* workspace (device) */
   uint32_t *line_start;  size_t cap_lines;
   uint32_t *tile_cnt;    size_t cap_tiles;
   uint64_t *hitmask, *hdrmask; uint32_t *wave_off, *hdr_off; size_t cap_chunks;
   uint4    *ent;                /* [cap_hitlines] k_order -> k_bounds2 (seeq_order.h) */
   uint32_t *hit_start, *hit_line, *nh, *hit_col, *nh_sum; size_t cap_hitlines;      /* nh_sum: per 256 entries (k_verify) */
   /* one-pass kernels: what the scan kernel of a segment writes and its post-pass reads */
   struct OnePassWs {
      uint32_t *tile_cl, *tile_hits, *tile_dirty; uint64_t *tile_dmask;   /* [cap_ftiles] */
      uint4    *tmp;                 /* [cap_hitlines] hit slices, then the COUNT -> EMIT cache */
      uint32_t *wg_hits;             /* [cap_slices] */
      uint32_t *wg_part;             /* [4 * cap_slices] */
      uint32_t *wg_lastnl;           /* [cap_slices] k_stream: last newline seen by each wave */
   } ow;
   size_t cap_ftiles, cap_slices;
   uint32_t *d_eqtab, *h_eqtab;   /* [256]; h_ is pinned */
   unsigned long eq_pat_id; int eq_options;   /* what d_eqtab holds (pattern generation id, option bits) */
   double avg_line;               /* average bytes per line incl. newline (hint or sampled) */
   double line_hint;              /* caller's hint; 0 = sample the buffer */
   uint8_t *h_sample;             /* pinned, SAMPLE_BYTES */
   const void *avg_text; size_t avg_nbytes;
   int force_path;                /* 0 auto, 1 generic, 2 fused (SEEQ_PATH env / tests) */
   int last_path;                 /* 1 generic, 2 fused: what the last run used */
   seeqdev_hit_t *records; uint64_t *rec_off; size_t cap_records;
   /* SEEQDEV_FASTQ (seeq_fastq.h): the filter's output arrays -- swapped with records / rec_off after a filter, so both pairs hold cap_records
      entries -- and its per-tile sums; only on contexts that were given the flag (fq_ws), grown with the record arrays */
   seeqdev_hit_t *fq_rec; uint64_t *fq_off; uint32_t *fq_bsum; size_t cap_fq;
   FastqCnt *d_fqcnt, *h_fqcnt;   /* h_ pinned */
   bool fq_ws;                    /* the context has been given SEEQDEV_FASTQ: the scratch above follows cap_records from now on */
   bool fastq;                    /* the last run was given the flag (options / want below are those of the internal, unflagged scan) */
   bool fq_done;                  /* ... and seeqdevScanFetch has filtered its records */
   int  fq_want;                  /* ... and this is the `want` its caller passed */
   uint32_t *scan_ws;           size_t cap_scan_ws;
   uint32_t *lead_fidx, *lead_flag, *lead_wend; unsigned long long *lead_key; size_t cap_lead;      /* long lines, leaders (seeq_stream.h): per hit-list entry */
   Counters *d_cnt;
   Counters *h_cnt;            /* pinned */
   /* seeqdevStringMatch: one string per call in ONE launch (pinned, device-visible) */
   uint8_t *h_str;                            /* the string (strings below STRING_ZC_MAX are read by the kernel over the link) */
   uint32_t *h_strout; size_t cap_strout;     /* {nhits, ticket, pad[2]} + records; fine-grained (coherent) page-locked memory */
   uint32_t  str_seq;                         /* ticket of the last k_string launch */
   /* staging for seeqdevScanHost */
   uint8_t *d_text; size_t cap_text;
   /* seeqdevScanRunMulti: per pattern of the last multi scan its counts and (host copy) its records */
   seeqdev_counts_t *multi_cnt; size_t *multi_first; int multi_n, cap_multi_n;
   seeqdev_hit_t *multi_rec; size_t cap_multi_rec, multi_nrec;
   /* one-pass multi-pattern scans (seeq_multi.h): the plan of the last pattern set, per-pattern workspace */
   struct MultiPlan *mplan;                               /* owned */
   bool      multi_active;                                /* run_segments: stop after the candidate list, hand over to multi_post */
   int       multi_rc;                                    /* multi_post's verdict inside run_segments */
   uint32_t *ml_mask, *ml_first, *ml_last; size_t cap_ml;            /* per candidate line */
   uint32_t *mp_idx, *mp_nh; size_t cap_mp;               /* npat regions of cap_mp / npat entries: index into the per-line arrays, hits */
   uint32_t *m_bsum; size_t cap_m_bsum;
   Counters *d_mcnt, *h_mcnt;                             /* [SEEQ_MULTI_MAX], h_ pinned */
   MultiExact *d_mx, *h_mx; size_t mx_slots, mx_next;      /* per segment the patterns' exact-pass arguments: device copy, pinned ring of mx_slots segments */
   uint32_t *m_scan_ws; size_t cap_m_scan_ws;             /* block sums of the per-pattern scans */
   int       last_multi;                                  /* the last multi scan: 1 = one walk for all patterns, 0 = a scan per pattern */
   /* seeqdevScanRunDemux (seeq_demux.h): allocated by the first demux call */
   uint32_t *dm_key, *dm_aux; size_t cap_dm_lines;        /* per line: key, then rank (one walk) or staging slot (a scan per pattern) */
   uint4    *dm_out; size_t cap_dm_out;                   /* the records (a scan per pattern: first the staging area) */
   DemuxCnt *d_dmcnt, *h_dmcnt;                           /* h_ pinned */
   size_t    dm_nrec;                                     /* records of the last demux */
   uint64_t  dm_nlines;                                   /* its counted lines */
   /* the first scan's records and offsets of a call that scans twice, aside on the device while the second scan runs (side_keep:
      the plus strand of seeqdevScanRunStrands, the right flank of seeqdevScanRunInserts) */
   seeqdev_hit_t *side_rec; uint64_t *side_off; size_t cap_side;
   /* seeqdevScanRunStrands (seeq_strand.h): allocated by the first both-strands call */
   uint4    *st_mrg; uint64_t *st_mrg_off; uint32_t *st_bsum; size_t cap_st_mrg;      /* the merged records and offsets, the reduction's per-tile sums */
   StrandCnt *d_stcnt, *h_stcnt;                          /* h_ pinned */
   EventPair tm_st;                                       /* profiling: around the merge's launches and copies (the FASTQ filter not included) */
   /* seeqdevScanRunInserts (seeq_insert.h): allocated by the first inserts call; the result (ins_rec, ins_off, ins_pos) is valid until the next one */
   uint4    *ins_jn; uint32_t *ins_bsum; uint64_t *ins_bbytes; size_t cap_ins_jn;      /* the joined records (one per left record), the reduction's per-tile sums */
   uint4    *ins_rec; uint64_t *ins_off, *ins_pos; size_t cap_ins;      /* the insert records, their line offsets, their byte positions in the insert text */
   InsertCnt *d_inscnt, *h_inscnt;                        /* h_ pinned */
   size_t    ins_n;                                       /* records of the last inserts call */
   uint64_t  ins_text_bytes;                              /* bytes of its insert text */
   bool      ins_staged; size_t ins_staged_nbytes;        /* it scanned the context's staged text (seeqdevScanHostInserts), and d_text still holds it */
   EventPair tm_ins;                                      /* profiling: around the join's launches */
   bool      ins_done;                                    /* an inserts call has completed: ins_n records (none included) are a result */
   /* seeqdevScanTally (seeq_tally.h): allocated by the first tally; the table (tl_tab, tl_n) is valid until the next one */
   uint64_t *tl_key0, *tl_key1; uint32_t *tl_mat, *tl_sum, *tl_stat; size_t cap_tl;      /* per span: the two key arrays; per tile: the digit matrix, the sums, the pack's eight words */
   seeqdev_tally_t *tl_tab; size_t cap_tl_tab;            /* the table: one entry per distinct key */
   TallyCnt *d_tlcnt, *h_tlcnt;                           /* h_ pinned */
   size_t    tl_n;                                        /* entries of the last tally's table */
   EventPair tm_tl;                                       /* profiling: around the tally's launches and counter copies */
   /* seeqdevScanTallyHold / seeqdevScanTallyGrouped (seeq_tally_group.h).  The held column (th_line, th_key: th_n records) is the context's
      from a completed hold to the next one; the grouped call's key scratch is the plain tally's (tl_key0 / tl_key1 / tl_mat: the member
      words and the digit matrix) and two group-word arrays of its own; its two tables are valid until the next grouped call */
   uint32_t *th_line; uint64_t *th_key; uint32_t *th_stat; size_t cap_th;      /* per held record: line, key; per tile: the hold's eight words */
   size_t    th_n;                                        /* held records */
   uint32_t  th_key_bits;                                 /* bits of the largest held key */
   bool      th_done;                                     /* a hold has completed: th_n records (none included) are a column */
   /* seeqdevScanTallyHoldAppend (seeq_tally_append.h): the held key's columns, and the arrays a new column is built in before it is joined */
   uint64_t  th_nkeyed;                                   /* held records with a key */
   uint32_t  th_width[SEEQ_TALLY_COLUMNS]; uint32_t th_ncol;      /* the widths of the held key's columns, column 0 (the hold's) first */
   uint32_t *ta_line; uint64_t *ta_key; uint32_t *ta_stat; size_t cap_ta;      /* per appended record: line, key; per tile: its hold's eight words */
   bool      dm_done;                                    /* a demux has completed: dm_nrec records (none included) are a result */
   uint64_t *tg_g0, *tg_g1; uint32_t *tg_sum, *tg_stat; size_t cap_tg;         /* per span: the two group-word arrays; per tile: the head sums, the pack's words */
   seeqdev_tally_pair_t *tg_pairs; size_t cap_tg_pairs;   /* the pair table: one entry per distinct (group, member) */
   seeqdev_tally_group_t *tg_groups; size_t cap_tg_groups;      /* the group table: one entry per distinct group */
   TallyGroupCnt *d_tgcnt, *h_tgcnt;                      /* h_ pinned; the hold's counters too */
   size_t    tg_np, tg_ng;                                /* entries of the last grouped call's tables */
   EventPair tm_tg;                                       /* profiling: around the grouped call's launches and counter copies */
   /* seeqdevScanSetLibrary / seeqdevScanTallyLibrary / seeqdevScanTallyHoldLibrary (seeq_tally_library.h).  The library (lb_key, lb_id: lb_n
      entries, sorted by key) is the context's from a completed set call to the next one; the assignment's scratch is allocated by the first
      library call */
   uint64_t *lb_key; uint32_t *lb_id; size_t cap_lb;      /* per entry: key, id */
   size_t    lb_n;                                        /* entries of the library; 0: the context holds none */
   int       lb_mismatch;                                 /* its max_mismatch: 0 or 1 */
   int       lb_mode;                                     /* its mode, SEEQDEV_LIBRARY_*: max_mismatch, or 2 -- one edit, indels included */
   uint32_t *lb_sum; size_t cap_lb_sum;                   /* per tile of spans: misses, exact */
   uint4    *lb_nstat; size_t cap_lb_near;                /* per workgroup of the near pass: corrected, ambiguous, unknown, bad */
   uint2    *lb_nedit; size_t cap_lb_edit;                /* per workgroup of the near pass in the edit mode: inserted, deleted */
   seeqdev_tally_library_edits_t lb_edits;                /* the split of ncorrected of the last completed assignment; zero: none since the set call */
   TallyLibCnt *d_lbcnt, *h_lbcnt;                        /* h_ pinned */
   /* seeqdevScanTallyCollapse (seeq_tally_collapse.h): reads the two tables of the last grouped call, writes arrays of its own; its result
      (tc_parent: tc_np entries, tc_groups: tc_ng rows) is valid until the next grouped call or the next collapse */
   bool      tg_done;                                     /* a grouped call has completed: tg_np pairs in tg_ng groups (none included) are a result */
   uint64_t  tg_npaired; uint32_t tg_max_len;             /* its paired spans and its largest paired member length */
   uint32_t *tc_parent, *tc_proot; uint64_t *tc_pread; uint32_t *tc_rsum; uint64_t *tc_qsum; CollapseWg *tc_wst; size_t cap_tc;      /* per pair: parent, the two prefixes; per tile: their sums; per 64 pairs: the parents' numbers */
   seeqdev_tally_collapse_t *tc_groups; uint4 *tc_gst; size_t cap_tc_groups;      /* per group: its row; per 256 groups: their numbers */
   CollapseCnt *d_tccnt, *h_tccnt;                        /* h_ pinned */
   size_t    tc_np, tc_ng;                                /* entries of the last collapse's two arrays */
   EventPair tm_tc;                                       /* profiling: around the collapse's launches and its counters copy */
   /* seeqdevScanTallyHeld / seeqdevScanTallyHeldDense (seeq_tally_held.h): the tally of the held column itself.  Its key scratch and its key
      table are the plain tally's (tl_key0 / tl_key1 / tl_mat; tl_tab: tl_n); the head sums, the row table and the dense call's sums are its own */
   uint32_t *thd_sum; size_t cap_thd;                     /* per tile: key heads, row heads, nonzero items */
   seeqdev_tally_group_t *thd_rows; size_t cap_thd_rows;  /* the row table: one entry per distinct row */
   uint32_t *thd_dn; uint64_t *thd_dr; size_t cap_thd_dense;      /* per 256 entries of the key table: those outside the matrix, their reads */
   TallyHeldCnt *d_thdcnt, *h_thdcnt;                     /* h_ pinned */
   size_t    thd_nrows;                                   /* entries of the last held tally's row table */
   bool      thd_live;                                    /* a held tally has completed and the context's tally table is still its key table */
   uint32_t  thd_shift, thd_members;                      /* ... its column part's bits and its member_columns */
   uint64_t  thd_ncounted;                                /* ... and the sum of its counts */
   EventPair tm_thd;                                      /* profiling: around the held tally's (or the dense call's) launches and counter copies */
   /* seeqdevScanQualityGate (seeq_qgate.h): allocated by the first gate.  It reads a source's record arrays and writes these; the kinds
      (qg_kind: qg_nsrc source records) and the passed records (qg_rec, qg_off: qg_n) are copies, valid until the next gate */
   uint8_t  *qg_kind; uint32_t *qg_bsum; size_t cap_qg;   /* per source record: its kind; per tile: the seven numbers */
   uint4    *qg_rec; uint64_t *qg_off; size_t cap_qg_out; /* the passed records and their line offsets */
   QGateCnt *d_qgcnt, *h_qgcnt;                           /* h_ pinned */
   size_t    qg_n, qg_nsrc;                               /* passed records; source records of the last gate */
   bool      qg_done;                                     /* a gate has completed: qg_n records (none included) are a result */
   bool      qg_from_inserts;                             /* ... and its source was the inserts: a NULL text is the staged one */
   EventPair tm_qg;                                       /* profiling: around the gate's launches and counter copies */
   /* seeqdevScanAnchor (seeq_anchor.h): allocated by the first anchor call.  It reads a source's record arrays and writes these; the kinds
      and cut ends (an_kind, an_end: an_nsrc source records) and the kept records (an_rec, an_off: an_n) are copies, valid until the next anchor */
   uint8_t  *an_kind; uint32_t *an_end; uint32_t *an_bsum; size_t cap_an;      /* per source record: its kind, the end of its cut; per tile: the six numbers */
   uint4    *an_rec; uint64_t *an_off; size_t cap_an_out; /* the kept records, rewritten, and their line offsets */
   AnchorCnt *d_ancnt, *h_ancnt;                          /* h_ pinned */
   size_t    an_n, an_nsrc;                               /* kept records; source records of the last anchor */
   bool      an_done;                                     /* an anchor has completed: an_n records (none included) are a result */
   bool      an_from_inserts;                             /* ... and its source was the inserts: a NULL text is the staged one */
   EventPair tm_an;                                       /* profiling: around the anchor's launches and counter copies */
   /* packed read batches (seeqdevScanPacked) */
   uint32_t *pk_cand, *pk_slot, *pk_coff; uint64_t *pk_bmask; size_t cap_pk_reads;      /* candidate columns per read of a segment; per block of 64 reads: candidates before it, their mask */
   uint8_t  *pk_stage; size_t cap_pk_stage;               /* ASCII lines of the candidate reads */
   uint8_t  *d_unpack; size_t cap_unpack;                 /* the whole batch as ASCII text: patterns the packed walk does not serve */
   uint32_t *pk_last; size_t cap_pk_last;                 /* per candidate: column of its last candidate */
   bool      is_packed; seeqdev_packed_t packed;          /* the last run was a packed one (re-run on overflow) */
   /* last run (for the transparent re-run on overflow) */
   const seeqdev_pattern *pat; const void *text; size_t nbytes; int options, want;
   bool ran;
   int  last_runs;             /* runs the last completed scan (or one walk) took: 1 = no re-run */
   seeqdev_counts_t counts;
   /* profiling */
   bool prof;
   hipEvent_t *ev;             /* 4 events per segment: index start, forward start, forward end, segment end */
   size_t nev_seg;             /* segments that have events */
   size_t prof_segs;           /* segments of the last run */
   float acc_ms[4];
   float fwd_ms_avg;           /* mean k_forward launch duration of the last run */
   size_t seg_bytes;           /* segment size */
   bool user_reserved;         /* caller sized the per-line workspace: trust it */
   RerunFallback fallback;     /* what earlier runs reported of the text: kernels the planner stays off for the next scans (seeq_rerun.h) */
   bool sample_dirty;          /* the sampled prefix holds more than one byte outside the alphabet per 4 KB: FASTA input stays off k_pair */
   unsigned sample_age;        /* runs since the line-length sample was taken (a reused buffer may hold other text by now) */
};

/* the CPU argument-check tests pass a zeroed stand-in of this many bytes for a context: what a check reads before its first device call lies inside */
static_assert(sizeof(seeqdev_scan) <= 8192, "seeqdev_scan has outgrown the tests' stand-in context");

/* The workspace's hooks (seeq_workspace.h).  A refused allocation (ENOMEM) leaves the array, and with it the capacity its group was sized
   for, as it was: the context stays usable (tests/test_gpu_parity.py::test_a_refused_reserve_leaves_the_context_usable). */
static void *ws_hip_alloc(void *, int kind, size_t bytes)
{
   void *g = NULL;
   const hipError_t e = kind == WS_DEVICE ? hipMalloc(&g, bytes ? bytes : 16)
                      : hipHostMalloc(&g, bytes ? bytes : 16, kind == WS_COHERENT ? hipHostMallocCoherent : hipHostMallocDefault);
   if (e == hipSuccess) return g;
   (void)hipGetLastError();
   hip_fail(e, kind == WS_DEVICE ? "hipMalloc(workspace)" : "hipHostMalloc(workspace)", ENOMEM);
   return NULL;
}

static void ws_hip_release(void *, int kind, void *p)
{
   if (kind == WS_DEVICE) (void)hipFree(p);
   else (void)hipHostFree(p);
}

/* ws_grow_keep: work on the context's stream may still write the old block -- wait for it, then device to device (and wait), or memcpy */
static int ws_hip_copy(void *ctx, int kind, void *dst, const void *src, size_t bytes)
{
   const hipStream_t st = ((seeqdev_scan *)ctx)->stream;
   HIP_TRY(hipStreamSynchronize(st), EIO);
   if (kind != WS_DEVICE) { memcpy(dst, src, bytes); return 0; }
   HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st), EIO);
   HIP_TRY(hipStreamSynchronize(st), EIO);
   return 0;
}

extern "C" seeqdev_scan_t *seeqdevScanNew(void *hip_stream)
{
   seeqerr = 0;
   if (seeqdevDeviceCount() < 1) {
      snprintf(g_last_error, sizeof g_last_error, "no HIP device: seeq-mi355x has no CPU matcher");
      errno = ENODEV;
      return NULL;
   }
   seeqdev_scan *s = (seeqdev_scan *)calloc(1, sizeof *s);
   if (!s) return NULL;
   if (hipGetDevice(&s->device) != hipSuccess) s->device = 0;
   s->ws.hooks = {ws_hip_alloc, ws_hip_release, s, ws_hip_copy};
   s->seg_bytes = (size_t)0xF0000000u;      /* 3.75 GiB segments: u32 offsets with room for k_stream's bias; multiple of every tile size */
   const char *env = getenv("SEEQ_SEGMENT_BYTES");
   if (env && atoll(env) >= 65536) s->seg_bytes = ((size_t)atoll(env) + 15) & ~(size_t)15;
   if (s->seg_bytes > 0xFFFF0000ull) s->seg_bytes = 0xFFFF0000ull;
   hipError_t e = hipSuccess;
   if (hip_stream) s->stream = (hipStream_t)hip_stream;
   else {
      /* a private stream of the default ("blocking") kind: work a caller queued on the legacy null stream -- torch's
         default stream has handle 0, which arrives here as NULL -- is ordered before ours and ours before theirs */
      e = hipStreamCreateWithFlags(&s->stream, hipStreamDefault);
      s->own_stream = true;
   }
   if (e == hipSuccess && ws_make(&s->ws, {{s->d_cnt, sizeof(Counters)}, {s->h_cnt, sizeof(Counters), WS_PINNED}, {s->h_eqtab, 2048 * sizeof(uint32_t), WS_PINNED},
                                           {s->d_eqtab, 2048 * sizeof(uint32_t)}, {s->h_sample, SAMPLE_BYTES, WS_PINNED}}))
      e = hipErrorOutOfMemory;
   {
      const char *pe = getenv("SEEQ_PATH");
      s->force_path = pe ? (!strcmp(pe, "generic") ? 1 : !strcmp(pe, "fused") ? 2 : 0) : 0;
      ScanKnobs &kn = s->knobs;
      const char *v;
      v = getenv("SEEQ_FUSED_KERNEL"); kn.kernel = v ? (!strcmp(v, "stream") ? 1 : !strcmp(v, "direct") ? 2 : !strcmp(v, "pair") ? 3 : 0) : 0;
      v = getenv("SEEQ_NO_LEADERS");   kn.no_leaders = v && atoi(v) == 1;
      v = getenv("SEEQ_TILE_BYTES");   kn.tile_bytes = v ? atoi(v) : 0;
      v = getenv("SEEQ_NO_FILTER");    kn.no_filter = v && atoi(v) == 1;
      v = getenv("SEEQ_STREAM_SUB");   kn.no_sub = v && atoi(v) == 0;
      v = getenv("SEEQ_STREAM_WU");    kn.min_wu = v ? atoi(v) : 0;
      v = getenv("SEEQ_NO_MYERS");     kn.no_myers = v && atoi(v) == 1;
      v = getenv("SEEQ_NO_WINDOW");    kn.no_window = v && atoi(v) == 1;
      v = getenv("SEEQ_EXPLAIN");      kn.explain = v && atoi(v) == 1;
      v = getenv("SEEQ_PACKED_QUAD");  kn.no_packed_quad = v && atoi(v) == 0;
      v = getenv("SEEQ_PACKED_SEG_READS");
      s->pk_seg_reads = v && atol(v) >= 64 && (size_t)atol(v) <= ((size_t)1 << 26) ? (size_t)atol(v) & ~(size_t)63 : PACKED_SEG_READS_DEFAULT;
      s->ncu = 256;
      s->lds_per_wg = 65536;
      s->lds_per_cu = 65536;
      int dev = 0;
      hipDeviceProp_t prop;
      if (e == hipSuccess && hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
      { s->ncu = prop.multiProcessorCount; s->lds_per_wg = prop.sharedMemPerBlock; s->lds_per_cu = prop.maxSharedMemoryPerMultiProcessor; }
   }
   if (e != hipSuccess) {
      hip_fail(e, "seeqdevScanNew", EIO);
      seeqdevScanFree(s);
      return NULL;
   }
   return s;
}

extern "C" void seeqdevScanFree(seeqdev_scan_t *s)
{
   if (!s) return;
   (void)use_device(s->device);
   for (EventPair *t : {&s->tm_h2d, &s->tm_st, &s->tm_ins, &s->tm_tl, &s->tm_tg, &s->tm_tc, &s->tm_thd, &s->tm_qg, &s->tm_an})
      if (t->made) { (void)hipEventDestroy(t->ev[0]); (void)hipEventDestroy(t->ev[1]); }
   (void)hipStreamSynchronize(s->stream);
   ws_free_all(&s->ws);
   multi_plan_free(s->mplan);
   for (size_t i = 0; i < 4 * s->nev_seg; i++) (void)hipEventDestroy(s->ev[i]);
   free(s->ev);
   free(s->launch_ms);
   free(s->multi_cnt); free(s->multi_first);
   if (s->own_stream && s->stream) (void)hipStreamDestroy(s->stream);
   free(s);
}

/* block sums of the two-level scans (launch_scan, launch_scanset, the packed and demux rank scans): room for nblocks of them */
static int ensure_scan_ws(seeqdev_scan *s, size_t nblocks)
{
   return ws_grow(&s->ws, &s->cap_scan_ws, nblocks, {{s->scan_ws, nblocks * sizeof(uint32_t)}});
}

/* the filter's per-tile sums for n records (seeq_fastq.h: kept and opened per tile) */
static size_t fastq_bsum_words(size_t n) { return 2 * (n / SEEQ_TILE + 2); }

static int reserve_impl(seeqdev_scan *s, size_t max_bytes, size_t max_lines, size_t max_hitlines, size_t max_records)
{
   seeqerr = 0;
   if (!s) { errno = EINVAL; return -1; }
   Workspace *w = &s->ws;
   /* Everything per-line is per SEGMENT; only records span the whole buffer. */
   if (max_bytes) {
      const size_t seg = max_bytes < s->seg_bytes ? max_bytes : s->seg_bytes;
      const size_t tiles = (seg + TILE - 1) / TILE + 1;
      if (ws_grow(w, &s->cap_tiles, tiles, {{s->tile_cnt, tiles * sizeof(uint32_t)}})) return -1;
      const size_t ftiles = seg / FUSED_MIN_TILE + 2;
      const size_t slices = MAX_FUSED_GRID;               /* hit slices: one per wave of a persistent grid */
      if (ws_grow(w, &s->cap_ftiles, ftiles, {{s->ow.tile_cl, ftiles * sizeof(uint32_t)}, {s->ow.tile_dirty, ftiles * sizeof(uint32_t)},
                                              {s->ow.tile_dmask, ftiles * sizeof(uint64_t)}, {s->ow.tile_hits, ftiles * sizeof(uint32_t)}})) return -1;
      if (ws_grow(w, &s->cap_slices, slices, {{s->ow.wg_hits, slices * sizeof(uint32_t)}, {s->ow.wg_part, 4 * slices * sizeof(uint32_t)},
                                              {s->ow.wg_lastnl, slices * sizeof(uint32_t)}})) return -1;
   }
   if (max_lines > s->cap_lines) {
      const size_t chunks = (max_lines + 63) / 64 + 1;
      if (ws_grow(w, &s->cap_lines, max_lines, {{s->line_start, (max_lines + 1) * sizeof(uint32_t)}, {s->hitmask, chunks * sizeof(uint64_t)},
                                                {s->hdrmask, chunks * sizeof(uint64_t)}, {s->wave_off, chunks * sizeof(uint32_t)},
                                                {s->hdr_off, chunks * sizeof(uint32_t)}})) return -1;
      s->cap_chunks = chunks;
   }
   if (ws_grow(w, &s->cap_hitlines, max_hitlines, {{s->hit_start, max_hitlines * sizeof(uint32_t)}, {s->hit_line, max_hitlines * sizeof(uint32_t)},
                                                   {s->ow.tmp, max_hitlines * sizeof(uint4)}, {s->nh, max_hitlines * sizeof(uint32_t)},
                                                   {s->hit_col, max_hitlines * sizeof(uint32_t)}, {s->ent, max_hitlines * sizeof(uint4)},
                                                   {s->nh_sum, 2 * (max_hitlines / 256 + 2) * sizeof(uint32_t)}})) return -1;      /* (nh_sum: + the chunks' entries with a hit) */
   if (s->fq_ws && max_records > s->cap_records) {
      /* the filter's scratch grows with the record arrays, as one group */
      if (ws_grow(w, &s->cap_records, max_records, {{s->records, max_records * sizeof(seeqdev_hit_t)}, {s->rec_off, max_records * sizeof(uint64_t)},
                                                    {s->fq_rec, max_records * sizeof(seeqdev_hit_t)}, {s->fq_off, max_records * sizeof(uint64_t)},
                                                    {s->fq_bsum, fastq_bsum_words(max_records) * sizeof(uint32_t)}})) return -1;
      s->cap_fq = s->cap_records;
   } else if (ws_grow(w, &s->cap_records, max_records, {{s->records, max_records * sizeof(seeqdev_hit_t)}, {s->rec_off, max_records * sizeof(uint64_t)}})) return -1;
   if (s->fq_ws) {
      /* (record arrays from before the context's first flagged scan: the scratch catches up) */
      const size_t n = s->cap_records;
      if (ws_grow(w, &s->cap_fq, n, {{s->fq_rec, n * sizeof(seeqdev_hit_t)}, {s->fq_off, n * sizeof(uint64_t)}, {s->fq_bsum, fastq_bsum_words(n) * sizeof(uint32_t)}})) return -1;
      if (ws_make(w, {{s->d_fqcnt, sizeof(FastqCnt)}, {s->h_fqcnt, sizeof(FastqCnt), WS_PINNED}})) return -1;
   }
   /* block sums for the two-level scans: the largest scanned array */
   size_t largest = s->cap_tiles;
   if (s->cap_chunks > largest) largest = s->cap_chunks;
   if (s->cap_hitlines > largest) largest = s->cap_hitlines;
   if (s->cap_ftiles > largest) largest = s->cap_ftiles;
   size_t nb = largest / SCAN_BLOCK + 2;
   if (3 * (s->cap_ftiles / SCAN_BLOCK + 2) > nb) nb = 3 * (s->cap_ftiles / SCAN_BLOCK + 2);   /* launch_scanset: three tile arrays at once */
   return ensure_scan_ws(s, nb);
}

extern "C" int seeqdevScanReserve(seeqdev_scan_t *s, size_t max_bytes, size_t max_lines, size_t max_hitlines,
                                  size_t max_records)
{
   if (reserve_impl(s, max_bytes, max_lines, max_hitlines, max_records)) return -1;
   if (max_lines) s->user_reserved = true;
   return 0;
}

extern "C" int seeqdevScanSetLineHint(seeqdev_scan_t *s, double avg_bytes_per_line)
{
   if (!s || avg_bytes_per_line < 0) { errno = EINVAL; return -1; }
   s->line_hint = avg_bytes_per_line;
   return 0;
}

extern "C" int seeqdevScanLastPath(const seeqdev_scan_t *s) { return s ? s->last_path : 0; }
extern "C" int seeqdevScanLastFilter(const seeqdev_scan_t *s) { return s && s->last_filter ? 1 : 0; }
extern "C" int seeqdevScanLastPlan(const seeqdev_scan_t *s, int out[16])
{
   if (!s || !out) { errno = EINVAL; return -1; }
   memcpy(out, s->last_plan, sizeof s->last_plan);
   return 0;
}
extern "C" int seeqdevScanLastPackedQuad(const seeqdev_scan_t *s) { return s && s->last_packed_quad ? 1 : 0; }
extern "C" int seeqdevScanLastRuns(const seeqdev_scan_t *s) { return s ? s->last_runs : 0; }

extern "C" int seeqdevScanFallback(const seeqdev_scan_t *s, unsigned *bits, int *scans_left)
{
   if (!s) { errno = EINVAL; return -1; }
   if (bits) *bits = s->fallback.bits;
   if (scans_left) *scans_left = s->fallback.bits ? s->fallback.ttl : 0;
   return 0;
}

extern "C" int seeqdevScanSetProfiling(seeqdev_scan_t *s, int on)
{
   if (!s) { errno = EINVAL; return -1; }
   s->prof = on != 0;
   return 0;
}

extern "C" int seeqdevScanLastTimes(const seeqdev_scan_t *s, float ms[4])
{
   if (!s || !ms) { errno = EINVAL; return -1; }
   for (int i = 0; i < 4; i++) ms[i] = s->acc_ms[i];
   return 0;
}

/* Workgroups of `fn` (threads per workgroup, dynamic LDS) that fit one CU; asked once per kernel and LDS size.
 * Also raises the kernel's dynamic-LDS limit.  -1 (errno set) when HIP refuses. */
static int occupancy_of(seeqdev_scan *s, const void *fn, int threads, size_t lds)
{
   for (int i = 0; i < s->nocc; i++)
      if (s->occ[i].fn == fn && s->occ[i].lds == lds) return s->occ[i].per_cu;
   if (lds) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), EIO);
   int per_cu = 0;
   if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds) != hipSuccess || per_cu < 1) per_cu = 1;
   OccMemo &m = s->occ[s->nocc < 8 ? s->nocc++ : 7];
   m.fn = fn; m.lds = lds; m.per_cu = per_cu;
   return per_cu;
}

static int multi_post(seeqdev_scan *s, const ScanPlan &plan, const ScanArgs &ua, hipStream_t st);

/* what the planner (seeq_plan.h) needs to know of the pattern's automata, and how it asks for one that has not been tried yet */
static void pattern_automata(const seeqdev_pattern *p, PlanAutomata *au)
{
   au->sdfa_state = __atomic_load_n(&p->sdfa_state, __ATOMIC_ACQUIRE);
   au->sdfa_parts = p->sdfa_parts; au->sdfa_warm = p->sdfa_warm; au->sdfa_pacc = p->sdfa_pacc;
   au->pair_state = __atomic_load_n(&p->pair_state, __ATOMIC_ACQUIRE);
   au->pair_warm = p->pair_warm; au->pair_pacc = p->pair_pacc;
}

static void plan_ensure(void *ctx, int which, int complete_only, PlanAutomata *au)
{
   seeqdev_pattern *mp = (seeqdev_pattern *)ctx;
   if (which == 0) pattern_plan_stream(mp, complete_only != 0);
   else pattern_plan_pair(mp);
   pattern_automata(mp, au);
}

/* ---- a run of seeqdevScanRun, in pieces (round 5: run_segments was one function of 385 lines; the decisions had moved to seeq_plan.h in round 4,
        what is left executes the plan):  run_setup -- the plan, the kernel instance and its grid, the EQ tables, the profiling events;
        seg_onepass -- a segment's one-pass scan kernel (k_pair / k_stream / k_direct) and the ordering of its hit slices;
        seg_index_forward<W> -- the generic path's newline index and k_forward<W>;  seg_post<W> -- the exact pass and the records.
        They read the scan from the context (s->pat, s->options, ...), its plan from r.plan; SegRun holds what run_setup derives beside it ---- */
struct SegRun {
   ScanPlan  plan;
   int       nw;                      /* waves per workgroup of the scan kernel: one hit slice per wave of the grid */
   uint32_t  tile_bytes;
   unsigned  fused_grid, grid_lines;
   const void *stream_fn;             /* the k_stream / k_pair instance of this run */
   size_t    dfa_lds, seg_bytes, nseg;
};

/* Workgroups of WG threads over n entries, at most per_cu per CU (the grids of the per-line and hit-list kernels) */
static unsigned capped_grid(const seeqdev_scan *s, size_t n, size_t per_cu)
{
   const size_t blocks = (n + WG - 1) / WG, cap = (size_t)s->ncu * per_cu;
   const unsigned g = (unsigned)(blocks < cap ? blocks : cap);
   return g ? g : 1;
}

/* Profiling: four events for each of nseg segments (s->prof_segs: the segments of this run that record them) */
static int prof_events(seeqdev_scan *s, size_t nseg)
{
   s->prof_segs = 0;
   if (!s->prof) return 0;
   if (nseg > s->nev_seg) {
      hipEvent_t *g = (hipEvent_t *)realloc(s->ev, 4 * nseg * sizeof(hipEvent_t));
      if (!g) { seeqerr = 0; errno = ENOMEM; return -1; }
      s->ev = g;
      while (s->nev_seg < nseg) {                          /* a segment counts once its four events exist: seeqdevScanFree destroys those and no others */
         hipEvent_t *e4 = s->ev + 4 * s->nev_seg;
         for (int i = 0; i < 4; i++) {
            const hipError_t e = hipEventCreate(&e4[i]);
            if (e != hipSuccess) { while (i--) (void)hipEventDestroy(e4[i]); return hip_fail(e, "hipEventCreate", EIO); }
         }
         s->nev_seg++;
      }
   }
   s->prof_segs = nseg;
   return 0;
}

/* The flags of seg_end_body: 1 = the hits come from nh[], 2 = nh[] holds 0/1 verdicts (a superset's lines, hits not counted per line) */
static int seg_end_flags(bool need_nh, bool superset, bool nh_is_count) { return (need_nh ? 1 : 0) | (superset && !nh_is_count ? 2 : 0); }

/* k_verify's variant (seeq_verify.h) and a.fin: k_nh_top ends the segment with `seg_flags` unless k_exact1's EMIT pass follows (SQ_ALL
   records: k_emit1 works from what k_nh_top saved) */
static int verify_variant(int want, int options, bool nh_is_count, int seg_flags, uint32_t *fin)
{
   const int var = (want == SEEQDEV_WANT_RECORDS && (options & 3) == SQ_BEST) ? VERIFY_BEST : nh_is_count ? VERIFY_ALL : VERIFY_ANY;
   *fin = (want == SEEQDEV_WANT_RECORDS && var == VERIFY_ALL) ? 0u : 1u + (uint32_t)seg_flags;
   return var;
}

/* EQ[dir][byte][fw] of one pattern (512 x fw words): the top-aligned Peq column of the byte's class, or a flag (reference seeqcore.h:89-111
   folded with the non-DNA option, libseeq.c:223-228,265-270) */
static void eq_fill(uint32_t *tab, const seeqdev_pattern *pat, int options, int fw)
{
   const int Wp = pat->words;
   for (int dir = 0; dir < 2; dir++)
      for (int b = 0; b < 256; b++) {
         const uint8_t cls = sq_class_of((uint32_t)b, options);
         uint64_t v;
         if (cls < 5) {
            const uint32_t *q = pat->h_peq + (dir * 5 + cls) * Wp;
            const uint64_t col = (uint64_t)q[0] | (Wp > 1 ? (uint64_t)q[1] << 32 : 0);
            v = col << (32 * fw - pat->wlen);                /* row m lands on the top bit */
         } else {
            v = cls == SQC_TERM ? FUSED_FLAG_TERM : FUSED_FLAG_SKIP;
         }
         uint32_t *dst = tab + (size_t)(dir * 256 + b) * fw;
         dst[0] = (uint32_t)v;
         if (fw == 2) dst[1] = (uint32_t)(v >> 32);
      }
}

/* The context's EQ tables: uploaded when the pattern or the options changed since its last scan */
static int eq_tables_upload(seeqdev_scan *s, const seeqdev_pattern *pat, int options, int fw)
{
   if (s->eq_pat_id == pat->id && s->eq_options == options) return 0;
   eq_fill(s->h_eqtab, pat, options, fw);
   /* third table, k_stream's Myers mode: the forward table with the newline marked (flag bits 0-1 = 3) */
   memcpy(s->h_eqtab + (size_t)512 * fw, s->h_eqtab, (size_t)256 * fw * sizeof(uint32_t));
   s->h_eqtab[(size_t)512 * fw + (size_t)'\n' * fw] |= 3u;
   /* the pinned staging table may still be read by an earlier copy on this stream: wait before the next rewrite */
   HIP_TRY(hipMemcpyAsync(s->d_eqtab, s->h_eqtab, (size_t)768 * fw * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream), EIO);
   HIP_TRY(hipStreamSynchronize(s->stream), EIO);
   s->eq_pat_id = pat->id;
   s->eq_options = options;
   return 0;
}

static int run_setup(seeqdev_scan *s, SegRun &r)
{
   const seeqdev_pattern *pat = s->pat;
   const bool fasta = (s->options & SEEQDEV_FASTA) != 0, single = (s->options & SEEQDEV_SINGLELINE) != 0;
   r.grid_lines = capped_grid(s, s->cap_lines, 16);

   /* ---- the plan (seeq_plan.h: a pure function of the pattern, the options, the text's line length and this context's fall-back
           flags); the rest of this function executes it ---- */
   PlanIn pin;
   memset(&pin, 0, sizeof pin);
   pin.wlen = pat->wlen; pin.tau = pat->tau; pin.options = s->options; pin.want = s->want;
   pin.avg_line = s->avg_line; pin.line_hint = s->line_hint; pin.force_path = s->force_path;
   const RerunFallback &fb = s->fallback;
   pin.no_stream = fb.no_stream(); pin.force_ll = fb.force_ll(); pin.no_stream_nd = fb.no_stream_nd(); pin.no_window = fb.no_window();
   pin.no_leaders = fb.no_leaders(); pin.sample_dirty = s->sample_dirty; pin.multi_active = s->multi_active;
   pin.seg_bytes = s->seg_bytes; pin.kn = &s->knobs;
   PlanAutomata au;
   pattern_automata(pat, &au);
   r.plan = seeq_plan_scan(pin, au, plan_ensure, const_cast<seeqdev_pattern *>(pat));
   const ScanPlan &plan = r.plan;
   if (s->knobs.explain) seeq_plan_print(stderr, pin, au, plan);
   if (plan.rc) return plan.rc;
   const int fw = plan.fw, stream_wu = plan.stream_wu;
   if (plan.use_fused) {
      if (plan.use_stream) {
         r.nw = STREAM_NW;
         r.tile_bytes = 64u * STREAM_CH_HOST;
         /* the k_stream instance of this scan: <warm-up dwords, FASTA, long lines, SUB> (stream_sub 0, 1: SQ_CONVERT ('N' for non-DNA bytes),
            2: SQ_IGNORE (skip bytes)) */
#define SEEQ_STREAM_FN(...) (stream_wu == 4 ? (const void *)k_stream<4, __VA_ARGS__> : stream_wu == 6 ? (const void *)k_stream<6, __VA_ARGS__> \
                                                                                                      : (const void *)k_stream<8, __VA_ARGS__>)
         r.stream_fn = plan.stream_sub == 2 ? SEEQ_STREAM_FN(false, false, 2)
                     : plan.stream_sub ? (plan.stream_ll ? SEEQ_STREAM_FN(false, true, 1) : SEEQ_STREAM_FN(false, false, 1))
                     : plan.stream_ll ? (fasta ? SEEQ_STREAM_FN(true, true) : SEEQ_STREAM_FN(false, true))
                     : fasta ? SEEQ_STREAM_FN(true, false) : SEEQ_STREAM_FN(false, false);
#undef SEEQ_STREAM_FN
         r.dfa_lds = ((size_t)pat->sdfa_rows * 16 + 15) & ~(size_t)15;
         if (plan.use_myers) {
#define SEEQ_MYERS_FN(FA, MY) (stream_wu == 16 ? (const void *)k_stream<16, FA, true, 0, MY> : (const void *)k_stream<32, FA, true, 0, MY>)
            r.stream_fn = fw == 1 ? (fasta ? SEEQ_MYERS_FN(true, 1) : SEEQ_MYERS_FN(false, 1)) : (fasta ? SEEQ_MYERS_FN(true, 2) : SEEQ_MYERS_FN(false, 2));
#undef SEEQ_MYERS_FN
            r.dfa_lds = (size_t)256 * fw * sizeof(uint32_t);
         }
         if (plan.use_pair) {
#define SEEQ_PAIR_FN(...) (stream_wu == 4 ? (const void *)k_pair<4, __VA_ARGS__> : stream_wu == 5 ? (const void *)k_pair<5, __VA_ARGS__> : stream_wu == 6 ? (const void *)k_pair<6, __VA_ARGS__> \
                          : stream_wu == 7 ? (const void *)k_pair<7, __VA_ARGS__> : (const void *)k_pair<8, __VA_ARGS__>)
            r.stream_fn = fasta ? SEEQ_PAIR_FN(true) : plan.ig ? SEEQ_PAIR_FN(false, true) : plan.pair_ll ? SEEQ_PAIR_FN(false, false, true) : SEEQ_PAIR_FN(false);
            r.dfa_lds = (size_t)pat->pair_units * 16;
#undef SEEQ_PAIR_FN
         }
      } else {
         r.nw = 4;
         double want = s->avg_line * 63.5;                /* <= 64 lines per region: one per lane */
         if (want < 512) want = 512;
         if (want > DIRECT_MAXRR * 1024) want = DIRECT_MAXRR * 1024;      /* (k_direct reads a region in at most DIRECT_MAXRR rounds of 1 KiB: lines that average more than 258 bytes
                                                                              once made regions of 16 KiB + 48 bytes, whose last 48 bytes no round looked at -- profiles/ignore_fuzz.py) */
         r.tile_bytes = ((uint32_t)want) & ~15u;
         if (s->knobs.tile_bytes >= 512 && s->knobs.tile_bytes <= DIRECT_MAXRR * 1024) r.tile_bytes = (uint32_t)s->knobs.tile_bytes & ~15u;
      }
      const void *fn = plan.use_stream ? r.stream_fn : fw == 1 ? (const void *)k_direct<4, 1> : (const void *)k_direct<4, 2>;
      const int per_cu = occupancy_of(s, fn, 64 * r.nw, r.dfa_lds);
      if (per_cu < 0) return -1;
      r.fused_grid = (unsigned)(s->ncu * per_cu);
      if ((size_t)r.fused_grid * r.nw > MAX_FUSED_GRID) r.fused_grid = (unsigned)(MAX_FUSED_GRID / r.nw);
      if (eq_tables_upload(s, pat, s->options, fw)) return -1;
   }
   s->last_path = plan.path;
   s->last_filter = plan.filter;
   {  /* (the numbers and the order of tests/host_harness.cpp: harness_plan) */
      const int v[16] = {plan.rc, plan.path, plan.fw, plan.use_stream, plan.use_pair, plan.use_myers, plan.filter, plan.stream_ll, plan.stream_sub, plan.stream_wu,
                         plan.verify, plan.order2, plan.leaders, plan.window_ok, plan.ll_restart ? 2 : (plan.ll_filter ? 1 : 0), (int)plan.skip_back};
      memcpy(s->last_plan, v, sizeof v);
   }

   const size_t nbytes = s->nbytes;
   r.seg_bytes = single ? (nbytes ? nbytes : 1) : s->seg_bytes;
   if (single && nbytes > 0xFFFF0000ull) { seeqerr = 0; errno = E2BIG; return -1; }
   r.nseg = nbytes ? (nbytes + r.seg_bytes - 1) / r.seg_bytes : 0;
   if (prof_events(s, r.nseg)) return -1;
   if (s->prof && r.nseg > s->cap_clk_probe) {
      ws_release(&s->ws, s->clk_probe);                    /* (nothing to carry over: the old block goes first; a refusal leaves profiling without the clock) */
      s->cap_clk_probe = 0;
      if (ws_make(&s->ws, {{s->clk_probe, r.nseg * 4 * sizeof(unsigned long long), WS_PINNED}}) == 0) s->cap_clk_probe = r.nseg;
   }
   if (s->prof && s->clk_probe) memset(s->clk_probe, 0, r.nseg * 4 * sizeof(unsigned long long));
   s->clk_valid = s->prof && s->clk_probe && plan.use_pair && plan.use_fused;
   /* (Tried: the post-pass of segment k on a second stream under k_pair of segment k + 1, k_pair on one workgroup per CU --
      it is as fast there.  The post-pass kernels do run beside it, and take 3 to 14 times as long as alone: they are
      made of scattered loads and the memory system is what k_pair saturates.  Net: +2 % .. -3 % per step.  Not kept;
      tag r03-experiment-overlap-postpass, profiles/r03/overlap_trace.txt.) */
   return 0;
}

/* a segment's one-pass scan kernel + the ordering of its hit slices: newline handling, forward scan and per-tile compaction in ONE kernel */
static int seg_onepass(seeqdev_scan *s, const SegRun &r, ScanArgs &a, size_t sg, hipEvent_t *ev, bool &order2, uint32_t &stream_ntiles)
{
   const ScanPlan &plan = r.plan;
   const seeqdev_pattern *pat = s->pat;
   const seeqdev_scan::OnePassWs &ow = s->ow;
   hipStream_t st = s->stream;

   FusedArgs f;
   memset(&f, 0, sizeof f);
   f.text = a.text; f.nbytes = s->nbytes; f.seg_base = a.seg_base; f.seg_len = a.seg_len; f.first_seg = a.first_seg;
   f.tile_bytes = r.tile_bytes;
   f.ntiles = (uint32_t)(((uint64_t)a.seg_len + r.tile_bytes - 1) / r.tile_bytes);
   stream_ntiles = f.ntiles;
   f.eqtab = s->d_eqtab; f.peq = pat->d_peq;
   f.m = pat->wlen; f.tau = pat->tau; f.options = s->options; f.want = s->want;
   f.tile_cl = ow.tile_cl; f.tile_hits = ow.tile_hits; f.tmp = ow.tmp; f.cap_tmp = (uint32_t)s->cap_hitlines;
   f.wg_hits = ow.wg_hits; f.wg_part = ow.wg_part; f.wg_lastnl = plan.stream_ll ? ow.wg_lastnl : nullptr;   /* only the window walk (long lines) needs it */
   f.tile_dirty = f.wg_lastnl ? ow.tile_dirty : nullptr;
   f.tile_dmask = f.wg_lastnl ? ow.tile_dmask : nullptr;
   f.cnt = s->d_cnt;
   f.clk_probe = (s->prof && s->clk_probe && plan.use_pair) ? s->clk_probe + 4 * sg : nullptr;
   uint32_t pos_bias = 0;
   if (plan.use_stream) {
      f.dfa = plan.stream_sub == 2 ? pat->d_sdfa_skip : plan.ll_restart ? pat->d_sdfa_restart : pat->d_sdfa; f.dfa_rows = pat->sdfa_rows; f.dfa_final_base = pat->sdfa_final_base;
      f.ll_filter = plan.ll_restart ? 2u : plan.ll_filter ? 1u : 0u;      /* (2: the restart table -- a chain that accepted inside its warm-up window names its first byte) */
      f.skip_thr = plan.skip_thr;
      if (plan.use_pair) { f.dfa = pat->d_pair; f.dfa_rows = pat->pair_units; f.dfa_final_base = 0; f.pair = 1; f.ig_thr = plan.ig ? (uint32_t)(pat->wlen - pat->tau) : 0u; }
      if (plan.use_myers) { f.dfa = (const uint16_t *)(s->d_eqtab + (size_t)512 * plan.fw); f.dfa_rows = (uint32_t)(64 * plan.fw); f.dfa_final_base = 0; f.pair = 2; }
      /* A hit line can start before the segment: hit offsets of this segment are relative to seg_base - pos_bias */
      uint64_t room = 0xFFFFFFF0ull - a.seg_len;
      if (room > ((uint64_t)1 << 30)) room = (uint64_t)1 << 30;
      pos_bias = (uint32_t)(a.seg_base < room ? a.seg_base : room) & ~127u;     /* chunk boundaries stay multiples of the chunk */
      f.pos_bias = pos_bias;
   }
   if (ev) { HIP_TRY(hipEventRecord(ev[0], st), EIO); HIP_TRY(hipEventRecord(ev[1], st), EIO); }
   /* persistent grid (workgroups without a tile just publish zeros), one hit slice per wave */
   const unsigned nsl = r.fused_grid * r.nw;
   f.slice_cap = f.cap_tmp / nsl;
   if (plan.use_stream) {
      void *kargs[] = {&f};
      HIP_TRY(hipLaunchKernel(r.stream_fn, dim3(r.fused_grid), dim3(64 * (unsigned)r.nw), kargs, r.dfa_lds, st), EIO);
   }
   else if (plan.use_direct && plan.fw == 2) hipLaunchKernelGGL((k_direct<4, 2>), dim3(r.fused_grid), dim3(256), 0, st, f);
   else hipLaunchKernelGGL((k_direct<4, 1>), dim3(r.fused_grid), dim3(256), 0, st, f);
   if (ev) HIP_TRY(hipEventRecord(ev[2], st), EIO);
   /* read-length lines behind k_pair / k_stream: the three launches of seeq_order.h; else (long lines, k_direct) the seven of before */
   const uint32_t order_nb = (f.ntiles + SEEQ_ORDER_BLOCK - 1) / SEEQ_ORDER_BLOCK;
   order2 = plan.order2 && order_nb <= SEEQ_ORDER_MAX_BLOCKS && 2 * (size_t)order_nb <= s->cap_scan_ws;
   if (plan.ig) {
      /* SQ_IGNORE behind k_pair: the line markers travel in the ordered entries (seeq_order.h) -- the older ordering kernels know nothing of them */
      if (!order2) { snprintf(g_last_error, sizeof g_last_error, "SQ_IGNORE on k_pair needs the three-launch ordering (segment too large for its block sums)"); seeqerr = 0; errno = EIO; return -1; }
      a.ig_thr = f.ig_thr; a.ig_ent = (const uint4 *)s->ent;
      {  /* the base the pattern's plain positions hold most often (ties: T first -- the rarest byte of FASTQ quality lines): an occurrence keeps all but tau copies */
         static const char base_of_key[9] = {0, 'A', 'C', 0, 'G', 0, 0, 0, 'T'};
         int cnt[4] = {0, 0, 0, 0}, best = 3;
         for (int i = 0; i < pat->wlen; i++) { const int kb = pat->keys[i] & 0x1F; if (kb == 1) cnt[0]++; else if (kb == 2) cnt[1]++; else if (kb == 4) cnt[2]++; else if (kb == 8) cnt[3]++; }
         for (int b = 2; b >= 0; b--) if (cnt[b] > cnt[best]) best = b;
         const int need = cnt[best] - pat->tau;
         a.ig_need = need > 0 ? (uint32_t)need : 0u;
         a.ig_bval = (uint32_t)(unsigned char)base_of_key[1 << best];
         a.ig_bmask = best == 3 ? 0xDEu : 0xDFu;           /* T: U and either case too */
      }
   }
   const unsigned rgrid = nsl / 4 + 1 < 2048 ? nsl / 4 + 1 : 2048;       /* one wave per slice, strided */
   if (order2) {
      seeq_launch_tiles_post(st, f, (uint32_t)nsl, s->scan_ws, order_nb);
      seeq_launch_order(rgrid, st, f, (uint32_t)nsl, (const uint32_t *)s->scan_ws, order_nb, s->ent);
   }
   else hipLaunchKernelGGL(k_fused_post, dim3(1), dim3(256), 0, st, f, (uint32_t)nsl);
   if (!order2 && (s->want != SEEQDEV_WANT_COUNTLINES || plan.superset)) {
      launch_scanset(st, s->scan_ws, f.tile_hits, f.tile_cl, f.tile_dirty, f.ntiles, nullptr, nullptr, f.tile_dirty ? &s->d_cnt->seg_dirty_tiles : nullptr);
      if (plan.use_stream) hipLaunchKernelGGL(k_stream_reorder, dim3(rgrid), dim3(256), 0, st, f, (uint32_t)nsl, s->hit_start, s->hit_line, s->nh, s->hit_col);
      else hipLaunchKernelGGL(k_fused_reorder, dim3(rgrid), dim3(256), 0, st, f, (uint32_t)nsl, s->hit_start, s->hit_line);
   }
   a.seg_base -= pos_bias;                           /* the exact pass addresses lines through hit_start */
   a.pos_bias = pos_bias;
   a.tile_dirty = f.tile_dirty; a.tile_dmask = f.tile_dmask; a.stream_ntiles = f.ntiles; a.stream_tile_bytes = r.tile_bytes;
   /* the exact pass walks candidate windows instead of whole lines where lines are long (sampled average);
      read-length lines are scanned whole -- the bookkeeping of the walk costs more than it saves there */
   a.stream_ch = plan.stream_ll ? STREAM_CH_HOST : 0u;
   a.walk_ext = plan.walk_ext; a.ll_restart = plan.ll_restart ? 1u : 0u;
   return 0;
}

/* the generic path's segment: newline index (K0), k_forward<W> (K1), ranks of the hit lines and of the FASTA headers (K2) */
template <int W>
static int seg_index_forward(seeqdev_scan *s, const SegRun &r, ScanArgs &a, hipEvent_t *ev)
{
   Counters *c = s->d_cnt;
   hipStream_t st = s->stream;
   /* ---- K0: newline index ---- */
   if (ev) HIP_TRY(hipEventRecord(ev[0], st), EIO);
   if (s->options & SEEQDEV_SINGLELINE) {
      hipLaunchKernelGGL(k_single_line, dim3(1), dim3(1), 0, st, a);
   } else {
      hipLaunchKernelGGL(k_nl_count, dim3(a.ntiles), dim3(WG), 0, st, a);
      hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(WG), 0, st, a.tile_cnt, a.ntiles, &c->seg_nlines);
      hipLaunchKernelGGL(k_index_finalize, dim3(1), dim3(1), 0, st, a);
      hipLaunchKernelGGL(k_nl_write, dim3(a.ntiles), dim3(WG), 0, st, a);
   }
   /* ---- K1: forward scan ---- */
   if (ev) HIP_TRY(hipEventRecord(ev[1], st), EIO);
   hipLaunchKernelGGL(k_forward<W>, dim3(r.grid_lines), dim3(WG), 0, st, a);
   if (ev) HIP_TRY(hipEventRecord(ev[2], st), EIO);
   /* ---- K2: ranks of hit lines (and FASTA headers) ---- */
   launch_scan<1>(st, s->scan_ws, a.hitmask, a.wave_off, s->cap_chunks, &c->seg_nlines, 63u, 6u, &c->seg_nhitlines);
   if (s->options & SEEQDEV_FASTA) launch_scan<1>(st, s->scan_ws, a.hdrmask, a.hdr_off, s->cap_chunks, &c->seg_nlines, 63u, 6u, &c->seg_nheaders);
   return 0;
}

/* behind a segment's scan: hit list -> (multi-pattern hand-over | leaders) -> the exact pass (K4) -> the records (K5).  Returns 1 when the segment
   is finished here (several patterns: multi_post ended it), 0 to go on, < 0 on failure */
template <int W>
static int seg_post(seeqdev_scan *s, const SegRun &r, ScanArgs &a, hipEvent_t *ev, bool order2, uint32_t stream_ntiles)
{
   const ScanPlan &plan = r.plan;
   const int want = s->want, fw = plan.fw;
   Counters *c = s->d_cnt;
   hipStream_t st = s->stream;

   /* ---- K3: compaction ---- */
   if (!plan.use_fused) hipLaunchKernelGGL(k_compact, dim3(r.grid_lines), dim3(WG), 0, st, a);
   if (!plan.use_fused) hipLaunchKernelGGL(k_seg_mid, dim3(1), dim3(1), 0, st, a);   /* the fused paths: done by k_fused_post */
   const unsigned grid_hits = capped_grid(s, s->cap_hitlines, 16);
   if (order2) seeq_launch_bounds2(grid_hits, st, a, s->ent, s->hit_col);
   else if (plan.use_stream) hipLaunchKernelGGL(k_stream_bounds, dim3(grid_hits), dim3(256), 0, st, a, s->hit_col,
                                           (const uint32_t *)s->ow.tile_cl, stream_ntiles, r.tile_bytes);   /* hit position -> line start; repeats dropped */
   if (s->multi_active) {
      /* several patterns: the candidate list is the union's -- pattern sets per line, a list per pattern, the exact pass per pattern */
      { const int mr = multi_post(s, plan, a, st); if (mr > 0) return -2; if (mr) return -1; }      /* (1: a launch was refused -- a scan per pattern) */
      hipLaunchKernelGGL(k_seg_end, dim3(1), dim3(1), 0, st, a, 3);
      if (ev) HIP_TRY(hipEventRecord(ev[3], st), EIO);
      HIP_TRY(hipGetLastError(), EIO);
      return 1;
   }
   /* long lines, every hit counted: candidates far behind the one before them get a lane of their own (seeq_stream.h, leaders) */
   const uint32_t lead_wback = a.skip_back > 32u ? a.skip_back : 32u;
   if (plan.leaders) {
      if (ws_grow(&s->ws, &s->cap_lead, s->cap_hitlines, {{s->lead_fidx, s->cap_hitlines * sizeof(uint32_t)}, {s->lead_flag, s->cap_hitlines * sizeof(uint32_t)},
                                                          {s->lead_wend, s->cap_hitlines * sizeof(uint32_t)},
                                                          {s->lead_key, s->cap_hitlines * sizeof(unsigned long long)}})) return -1;
      const unsigned nbl = (unsigned)(s->cap_hitlines / LEAD_BLOCK + 1);
      hipLaunchKernelGGL(k_lead_reduce, dim3(nbl), dim3(256), 0, st, a, s->scan_ws);
      hipLaunchKernelGGL(k_lead_top, dim3(1), dim3(256), 0, st, a, s->scan_ws);
      hipLaunchKernelGGL(k_lead_apply, dim3(nbl), dim3(256), 0, st, a, (const uint32_t *)s->hit_col, (const uint32_t *)s->scan_ws, s->lead_fidx, s->lead_flag, s->ow.tmp, lead_wback, plan.lead_best ? s->lead_key : (unsigned long long *)nullptr);
      a.walk_end = s->lead_wend;
      /* SQ_BEST: COUNT has to walk every group itself (and leave each group's best hit in the cache) instead of trusting the hit
         list and leaving the scan to EMIT, one lane per line */
      if (plan.lead_best) a.filter = 1u;
      hipLaunchKernelGGL(k_lead_commit, dim3(grid_hits), dim3(256), 0, st, a, s->hit_col, (const uint4 *)s->ow.tmp);
   }
   const uint32_t *hcol = plan.use_stream ? s->hit_col : nullptr;      /* first-hit columns: the exact pass may skip ahead */
   uint4 *ecache = (plan.use_fused && plan.need_nh && want == SEEQDEV_WANT_RECORDS) ? s->ow.tmp : nullptr;   /* COUNT -> EMIT */
   const uint32_t *eqp = (const uint32_t *)s->d_eqtab;
   /* (Tried behind k_pair: a lane-queue kernel -- a wave owns 256 .. 512 hit-list entries staged in LDS and a lane that has
      finished its line takes the next entry at the next 64-byte block -- 22 % fewer instructions than k_exact1 COUNT, and
      slower, 296 against 257 us per segment: at 4 waves per SIMD the per-block loads of a lane are not hidden.  Not kept;
      tag r03-experiment-overlap-postpass holds it, profiles/r03/verify_ab.txt the numbers.) */
   /* ---- K4: hits per hit line ---- */
   /* behind the filters (every hit line is a candidate) on text where no byte is skipped: k_verify (seeq_verify.h) -- the lean
      two-phase exact pass with the scan of its counts inside; the EMIT pass behind it ends the segment */
   bool emitted = false;                                /* the records are out (k_emit1) */
   if (plan.verify) {
      const int var = verify_variant(want, s->options, plan.nh_is_count, seg_end_flags(plan.need_nh, plan.superset, plan.nh_is_count), &a.fin);
      a.nh_sum = s->nh_sum;
      a.nz_sum = plan.superset && plan.nh_is_count ? s->nh_sum + (s->cap_hitlines / 256 + 2) : nullptr;
      /* behind a partition filter every part of an occurrence reports: more than half of the entries are repeats of their line, and
         k_verify packs them away, 512 entries per workgroup (seeq_verify.h); behind a prefix automaton it does not pay */
      a.vrange = (plan.use_pair ? s->pat->pair_parts > 1 : s->pat->sdfa_parts > 1) ? 512u : 0u;
      seeq_launch_verify(fw, var, grid_hits, st, a, eqp, hcol, ecache);
      if (want == SEEQDEV_WANT_RECORDS && var != VERIFY_ALL) seeq_launch_emit1(grid_hits, st, a, ecache);
      else if (want == SEEQDEV_WANT_RECORDS && ecache)      /* SQ_ALL: the first records from the cache, the others from the overflow lists */
         seeq_launch_emit_all(fw, grid_hits, grid_hits, st, a, eqp, hcol, ecache);
      emitted = want == SEEQDEV_WANT_RECORDS && (var != VERIFY_ALL || ecache);
   }
   else if (plan.need_nh) {
      if (plan.use_fused) {
   #define SEEQ_COUNT1(WW, WK) hipLaunchKernelGGL((k_exact1<SQ_MODE_COUNT, WW, -1, WK>), dim3(grid_hits), dim3(WG), 0, st, a, eqp, hcol, ecache)
         if (fw == 2) { if (a.stream_ch) SEEQ_COUNT1(2, true); else SEEQ_COUNT1(2, false); }
         else { if (a.stream_ch) SEEQ_COUNT1(1, true); else SEEQ_COUNT1(1, false); }
   #undef SEEQ_COUNT1
      }
      else hipLaunchKernelGGL((k_exact<W, SQ_MODE_COUNT>), dim3(grid_hits), dim3(WG), 0, st, a);
      /* lines with >= 1 verified hit: with 0/1 verdicts that is the scan total (seg_nrec) -- no extra pass */
      if (plan.leaders) {
         hipLaunchKernelGGL(k_lead_check, dim3(grid_hits), dim3(256), 0, st, a, (const uint32_t *)s->hit_col, (const uint32_t *)s->lead_flag, lead_wback);
         if (plan.lead_best) {
            hipLaunchKernelGGL(k_lead_best, dim3(grid_hits), dim3(256), 0, st, a, (const uint32_t *)s->lead_fidx, s->lead_key, (const uint4 *)ecache, 0);
            hipLaunchKernelGGL(k_lead_best, dim3(grid_hits), dim3(256), 0, st, a, (const uint32_t *)s->lead_fidx, s->lead_key, (const uint4 *)ecache, 1);
         }
         else hipLaunchKernelGGL(k_lead_lines, dim3(grid_hits < 512 ? grid_hits : 512), dim3(256), 0, st, a, (const uint32_t *)s->lead_fidx, s->lead_flag);
      }
      else if (plan.superset && plan.nh_is_count) hipLaunchKernelGGL(k_count_nonzero, dim3(grid_hits < 512 ? grid_hits : 512), dim3(WG), 0, st, a);
      launch_scan<0>(st, s->scan_ws, a.nh, a.nh, s->cap_hitlines, &c->seg_nhitlines, 0u, 0u, &c->seg_nrec);
   }
   /* ---- K5: records ---- */
   if (want == SEEQDEV_WANT_RECORDS && !emitted) {
      if (!plan.verify) hipLaunchKernelGGL(k_rec_check, dim3(1), dim3(1), 0, st, a);      /* (k_verify's last workgroup did) */
      if (plan.use_fused) {
         const int mo = (s->options & 3) == SQ_COUNT ? SQ_FIRST : (s->options & 3);
   #define SEEQ_EMIT1(WW, OO, WK) hipLaunchKernelGGL((k_exact1<SQ_MODE_EMIT, WW, OO, WK>), dim3(grid_hits), dim3(WG), 0, st, a, eqp, hcol, ecache)
         if (a.stream_ch) {
            if (fw == 2) { if (mo == SQ_BEST) SEEQ_EMIT1(2, SQ_BEST, true); else SEEQ_EMIT1(2, -1, true); }
            else { if (mo == SQ_BEST) SEEQ_EMIT1(1, SQ_BEST, true); else SEEQ_EMIT1(1, -1, true); }
         } else {
            if (fw == 2) { if (mo == SQ_BEST) SEEQ_EMIT1(2, SQ_BEST, false); else SEEQ_EMIT1(2, -1, false); }
            else { if (mo == SQ_BEST) SEEQ_EMIT1(1, SQ_BEST, false); else SEEQ_EMIT1(1, -1, false); }
         }
   #undef SEEQ_EMIT1
      }
      else {
         hipLaunchKernelGGL((k_exact<W, SQ_MODE_EMIT>), dim3(grid_hits), dim3(WG), 0, st, a);
         hipLaunchKernelGGL(k_rec_offsets, dim3(grid_hits), dim3(WG), 0, st, a);    /* k_exact1 writes them itself */
      }
   }
   return 0;
}

template <int W>
static int run_segments(seeqdev_scan *s)
{
   Counters *c = s->d_cnt;
   hipStream_t st = s->stream;
   HIP_TRY(hipMemsetAsync(c, 0, sizeof(Counters), st), EIO);
   SegRun r;
   memset(&r, 0, sizeof r);
   { const int rc = run_setup(s, r); if (rc) return rc; }
   const ScanPlan &plan = r.plan;
   const seeqdev_pattern *pat = s->pat;
   const size_t nbytes = s->nbytes;
   for (size_t sg = 0; sg < r.nseg; sg++) {
      hipEvent_t *ev = s->prof ? s->ev + 4 * sg : NULL;
      uint32_t stream_ntiles = 0;
      bool order2 = false;                                /* the hit list is made by seeq_order.h's kernels */
      ScanArgs a;
      memset(&a, 0, sizeof a);
      a.text = (const uint8_t *)s->text;
      a.nbytes = nbytes;
      a.seg_base = (uint64_t)sg * r.seg_bytes;
      a.seg_len = (uint32_t)((nbytes - a.seg_base) < r.seg_bytes ? (nbytes - a.seg_base) : r.seg_bytes);
      a.first_seg = sg == 0;
      a.peq = pat->d_peq;
      a.m = pat->wlen; a.tau = pat->tau; a.options = s->options; a.want = s->want;
      a.line_start = s->line_start; a.cap_lines = (uint32_t)s->cap_lines;
      a.tile_cnt = s->tile_cnt; a.ntiles = (a.seg_len + TILE - 1) / TILE;
      a.hitmask = s->hitmask; a.hdrmask = s->hdrmask; a.wave_off = s->wave_off; a.hdr_off = s->hdr_off;
      a.hit_start = s->hit_start; a.hit_line = s->hit_line; a.cap_hitlines = (uint32_t)s->cap_hitlines; a.nh = s->nh;
      a.records = s->records; a.cap_records = s->cap_records; a.rec_off = s->rec_off;
      a.use_nh = plan.need_nh ? (plan.use_stream ? 3u : 1u) : 0u;
      a.filter = plan.filter ? 1u : 0u;
      a.skip_back = plan.skip_back;
      a.window_ok = plan.window_ok ? 1u : 0u;
      a.cnt = c;

      if (plan.use_fused) { if (seg_onepass(s, r, a, sg, ev, order2, stream_ntiles)) return -1; }
      else if (seg_index_forward<W>(s, r, a, ev)) return -1;
      if (s->want != SEEQDEV_WANT_COUNTLINES || plan.superset) {
         const int pr = seg_post<W>(s, r, a, ev, order2, stream_ntiles);
         if (pr < 0) return pr;
         if (pr > 0) continue;
      }
      if (!a.fin) hipLaunchKernelGGL(k_seg_end, dim3(1), dim3(1), 0, st, a, seg_end_flags(plan.need_nh, plan.superset, plan.nh_is_count));      /* (a.fin: the segment's last launch ended it) */
      if (ev) HIP_TRY(hipEventRecord(ev[3], st), EIO);
      HIP_TRY(hipGetLastError(), EIO);
   }
   HIP_TRY(hipMemcpyAsync(s->h_cnt, c, sizeof(Counters), hipMemcpyDeviceToHost, st), EIO);
   return 0;
}

/* ========================================================================== */
/* Packed read batches (seeq_packed.h)                                        */
/* ========================================================================== */
/* (reads per segment: seeqdev_scan.pk_seg_reads) */

static int run_packed(seeqdev_scan *s)
{
   const seeqdev_pattern *pat = s->pat;
   const seeqdev_packed_t &b = s->packed;
   const int options = s->options, want = s->want;
   const int match_opt = options & 3;
   const bool nh_is_count = want == SEEQDEV_WANT_COUNTMATCH || (want == SEEQDEV_WANT_RECORDS && match_opt == SQ_ALL);
   const int seg_flags = seg_end_flags(true, true, nh_is_count);      /* (every hit line is a candidate: nh[] decides) */
   const int fw = pat->wlen <= FUSED_MAX_WLEN ? 1 : 2;
   Counters *c = s->d_cnt;
   hipStream_t st = s->stream;
   const uint32_t L = b.read_len;
   /* the exact pass reads the candidates' windows from the batch itself (seeq_verify_packed.h) -- no staging text -- unless SQ_ALL records are
      wanted (k_emit_all recovers their starts from text) or the round-3 exact pass is asked for */
   const bool direct = !(want == SEEQDEV_WANT_RECORDS && match_opt == SQ_ALL);
   const uint32_t pitch = (L + 1u + 15u) & ~15u;            /* bytes per line of the staging text (L <= 256: the newline's word exists for every lane count up to 17; 16 lanes serve L <= 255, L = 256 below) */
   /* workspace: per read of a segment, per candidate */
   size_t PACKED_SEG_READS = s->pk_seg_reads;
   /* the staging text is addressed with 32-bit offsets: where it is used a segment holds no more reads than it has lines for (every wave fills its own
      share of it and a share never sees more candidates than its wave has reads) -- smaller segments, not E2BIG (round 4 refused above 26.8 M hit-list
      entries at read_len 150, whether or not the staging text was used at all) */
   const size_t stage_lines_max = (size_t)(0xFFFF0000ull / pitch);
   if (!direct && PACKED_SEG_READS + 64u * MAX_FUSED_GRID > stage_lines_max)
      PACKED_SEG_READS = (stage_lines_max - 64u * MAX_FUSED_GRID) & ~(size_t)63;
   const size_t seg_reads = b.nreads < PACKED_SEG_READS ? (size_t)b.nreads : PACKED_SEG_READS;
   const size_t cap_use = (!direct && s->cap_hitlines > stage_lines_max) ? stage_lines_max : s->cap_hitlines;      /* hit-list entries a segment may make */
   if (ws_grow(&s->ws, &s->cap_pk_reads, seg_reads, {{s->pk_cand, seg_reads * sizeof(uint32_t)}, {s->pk_slot, seg_reads * sizeof(uint32_t)},
                                                     {s->pk_coff, (seg_reads / 64 + 1) * sizeof(uint32_t)},
                                                     {s->pk_bmask, (seg_reads / 64 + 1) * sizeof(uint64_t)}})) return -1;
   if (!direct && ws_grow(&s->ws, &s->cap_pk_stage, cap_use * (size_t)pitch, {{s->pk_stage, cap_use * (size_t)pitch + 64}})) return -1;
   if (ws_grow(&s->ws, &s->cap_pk_last, s->cap_hitlines, {{s->pk_last, s->cap_hitlines * sizeof(uint32_t)}})) return -1;
   if (ensure_scan_ws(s, seg_reads / SCAN_BLOCK + 2)) return -1;      /* block sums of the scans over per-read arrays */
   /* EQ tables of the exact pass (as run_segments makes them) */
   if (eq_tables_upload(s, pat, options, fw)) return -1;
   HIP_TRY(hipMemsetAsync(c, 0, sizeof(Counters), st), EIO);
   s->clk_valid = false;                                    /* (the packed walk reads no clock) */
   /* four bases per gather over the quad table (seeq_dfa.h section 3b) when the pattern has one and the false candidates it adds
      -- each an exact-pass window, ~13 walks' worth -- stay below the gathers it saves: 4 % of the reads */
   const bool quad = pat->quad_state == 1 && !s->knobs.no_packed_quad && (pat->quad_pacc - pat->pair_pacc) * (double)L <= 0.04;
   s->last_packed_quad = quad;
   const size_t dfa_lds = quad ? (size_t)pat->quad_units * 16 : (size_t)pat->pair_units * 16;
   const void *walk_fn = quad ? (const void *)k_packed_walk<true> : (const void *)k_packed_walk<false>;
   int per_cu = occupancy_of(s, walk_fn, 64 * STREAM_NW, dfa_lds);
   if (per_cu < 0) return -1;
   /* persistent grid, but no more waves than blocks of 64 reads: every wave owns cap / waves lines of the staging text */
   unsigned wgrid = (unsigned)(s->ncu * per_cu);
   {
      const size_t nblocks = (seg_reads + 63) / 64, need = (nblocks + STREAM_NW_HOST - 1) / STREAM_NW_HOST;
      if (need < wgrid) wgrid = (unsigned)(need ? need : 1);
   }
   const unsigned grid_hits = capped_grid(s, s->cap_hitlines, 16);
   const size_t nseg = (size_t)((b.nreads + PACKED_SEG_READS - 1) / PACKED_SEG_READS);
   if (prof_events(s, nseg)) return -1;
   for (size_t sg = 0; sg < nseg; sg++) {
      hipEvent_t *ev = s->prof ? s->ev + 4 * sg : NULL;
      PackedArgs p;
      memset(&p, 0, sizeof p);
      p.bases = (const uint8_t *)b.bases; p.nmask = (const uint8_t *)b.nmask;
      p.first = (uint64_t)sg * PACKED_SEG_READS;
      p.nreads = (uint32_t)(b.nreads - p.first < PACKED_SEG_READS ? b.nreads - p.first : PACKED_SEG_READS);
      p.read_len = L; p.stride = b.stride; p.nstride = b.nstride;
      p.total_bytes = b.nreads * (uint64_t)b.stride;
      p.dfa = quad ? pat->d_quad : pat->d_pair; p.dfa_units = quad ? pat->quad_units : pat->pair_units;
      p.cand = s->pk_cand; p.cslot = s->pk_slot; p.boff = s->pk_coff; p.bmask = s->pk_bmask; p.stage = direct ? nullptr : s->pk_stage;
      p.wave_cap = (uint32_t)(cap_use / ((size_t)wgrid * STREAM_NW_HOST));
      p.pitch = pitch;
      p.hit_start = s->hit_start; p.hit_line = s->hit_line; p.hit_col = s->hit_col; p.hit_last = s->pk_last; p.nh = s->nh;
      p.cap = (uint32_t)cap_use;
      p.line_base = p.first;
      p.cnt = c;
      if (ev) { HIP_TRY(hipEventRecord(ev[0], st), EIO); HIP_TRY(hipEventRecord(ev[1], st), EIO); }
      {
         void *kargs[] = {&p};
         HIP_TRY(hipLaunchKernel(walk_fn, dim3(wgrid), dim3(64 * STREAM_NW), kargs, dfa_lds, st), EIO);
      }
      if (ev) HIP_TRY(hipEventRecord(ev[2], st), EIO);
      /* candidates before every block of 64 reads, their number */
      launch_scanset(st, s->scan_ws, s->pk_coff, nullptr, nullptr, (p.nreads + 63u) >> 6, &c->seg_nhitlines, nullptr, nullptr);
      hipLaunchKernelGGL(k_packed_counts, dim3(1), dim3(1), 0, st, p);
      hipLaunchKernelGGL(k_packed_list, dim3((unsigned)(((size_t)p.nreads / 1024 + 4) / 4)), dim3(256), 0, st, p);      /* a wave per 16 blocks of 64 reads */
      /* from here: the exact pass over the staging text, as behind k_pair */
      ScanArgs a;
      memset(&a, 0, sizeof a);
      a.text = direct ? nullptr : s->pk_stage;              /* (direct: nothing reads text -- the windows come from the batch) */
      a.nbytes = direct ? 0 : cap_use * (uint64_t)pitch;
      a.seg_base = 0; a.seg_len = (uint32_t)a.nbytes; a.first_seg = sg == 0;
      a.peq = pat->d_peq;
      a.m = pat->wlen; a.tau = pat->tau; a.options = options & ~(MASK_NONDNA | MASK_INPUT); a.want = want;
      a.hit_start = s->hit_start; a.hit_line = s->hit_line; a.cap_hitlines = (uint32_t)s->cap_hitlines; a.nh = s->nh;
      a.records = s->records; a.cap_records = s->cap_records; a.rec_off = s->rec_off;
      a.use_nh = 3u; a.filter = 1u;
      a.skip_back = (uint32_t)(pat->wlen + pat->tau);
      a.hit_last = s->pk_last;
      a.window_ok = 1u;
      a.cnt = c;
      a.rec_pitch = L + 1u;                                 /* seeqdevScanCopyOffsets: the read's offset in the ASCII form of the batch */
      const uint32_t *eqp = (const uint32_t *)s->d_eqtab;
      const uint32_t *hcol = s->hit_col;
      uint4 *ecache = want == SEEQDEV_WANT_RECORDS ? s->ow.tmp : nullptr;
      {
         /* the exact pass of the candidates: k_verify_packed on the batch itself, or (SQ_ALL records) k_verify over the staging text -- ASCII lines,
            no byte of them is skipped (seeq_verify.h) */
         const int var = verify_variant(want, options, nh_is_count, seg_flags, &a.fin);
         a.nh_sum = s->nh_sum;
         a.nz_sum = nh_is_count ? s->nh_sum + (s->cap_hitlines / 256 + 2) : nullptr;
         if (direct) seeq_launch_verify_packed(fw, var, grid_hits, st, a, b.bases, b.nmask, b.stride, b.nstride, L, p.total_bytes,
                                               b.nmask ? b.nreads * (uint64_t)b.nstride : 0ull, eqp, hcol, ecache);
         else seeq_launch_verify(fw, var, grid_hits, st, a, eqp, hcol, ecache);
         if (want == SEEQDEV_WANT_RECORDS && var != VERIFY_ALL) seeq_launch_emit1(grid_hits, st, a, ecache);
         else if (want == SEEQDEV_WANT_RECORDS) {
            seeq_launch_emit_all(fw, grid_hits, grid_hits, st, a, eqp, hcol, ecache);
            hipLaunchKernelGGL(k_seg_end, dim3(1), dim3(1), 0, st, a, seg_flags);
         }
      }
      if (ev) HIP_TRY(hipEventRecord(ev[3], st), EIO);
      HIP_TRY(hipGetLastError(), EIO);
   }
   HIP_TRY(hipMemcpyAsync(s->h_cnt, c, sizeof(Counters), hipMemcpyDeviceToHost, st), EIO);
   s->last_path = 8;
   s->last_filter = true;
   memset(s->last_plan, 0, sizeof s->last_plan);
   s->last_plan[1] = 8; s->last_plan[6] = 1;                /* (no ScanPlan behind a packed run: its path and the filter flag) */
   return 0;
}


static int dispatch_run(seeqdev_scan *s)
{
   if (s->is_packed) return run_packed(s);
   return SEEQ_FOR_WORDS(s->pat->words, run_segments, s);
}

/* The argument rules the scan entries share: a context, `want` in range, every pattern there and on the context's device, SEEQDEV_FASTQ not
   beside FASTA / SINGLELINE / input-mask bits.  0: one is broken (the entry's EINVAL; a foreign device is named in the error text). */
static int scan_args_ok(const seeqdev_scan_t *s, const seeqdev_pattern_t *const *pats, int npat, int options, int want)
{
   if (!s || !pats || npat < 1 || want < 0 || want > 2) return 0;
   for (int k = 0; k < npat; k++) {
      if (!pats[k]) return 0;
      if (pats[k]->device != s->device) {
         snprintf(g_last_error, sizeof g_last_error, "pattern lives on device %d, scan context on device %d", pats[k]->device, s->device);
         return 0;
      }
   }
   return !((options & SEEQDEV_FASTQ) && (options & (SEEQDEV_FASTA | SEEQDEV_SINGLELINE | MASK_INPUT)));
}

/* Everything of a run before its launches: arguments, fall-back flags, the optimistic workspace (hit lines: one line in
   `hl_div`), the line-length sample. */
static int scan_setup(seeqdev_scan_t *s, const seeqdev_pattern_t *pat, const void *d_text, size_t nbytes, int options, int want, int hl_div)
{
   seeqerr = 0;
   if (!scan_args_ok(s, &pat, 1, options, want) || (!d_text && nbytes)) { errno = EINVAL; return -1; }
   const bool fastq = (options & SEEQDEV_FASTQ) != 0;
   if (use_device(s->device)) return -1;
   s->fastq = fastq; s->fq_done = false; s->fq_want = want;
   if (fastq) {
      /* the scan itself runs unflagged (a re-run of seeqdevScanFetch too: it reads s->options / s->want); the count wants have
         no records to filter, so under the flag they are scanned for records: one per matching line, or every hit */
      s->fq_ws = true;
      options &= ~SEEQDEV_FASTQ;
      if (want != SEEQDEV_WANT_RECORDS) {
         options = (options & ~MASK_MATCH) | (want == SEEQDEV_WANT_COUNTLINES ? SQ_FIRST : SQ_ALL);
         want = SEEQDEV_WANT_RECORDS;
      }
   }
   s->pat = pat; s->text = d_text; s->nbytes = nbytes; s->options = options; s->want = want;
   s->ran = false;
   s->is_packed = false;
   s->fallback.age();
   /* The optimistic workspace: what is too small is detected on the device and fixed by a re-run (rerun_next). */
   const RerunCaps w = seeq_first_reservation(nbytes < s->seg_bytes ? nbytes : s->seg_bytes, (options & SEEQDEV_SINGLELINE) != 0, hl_div,
                                              {s->cap_lines, s->cap_hitlines, s->cap_records}, s->user_reserved);
   if (reserve_impl(s, nbytes ? nbytes : 1, w.lines, w.hitlines, w.records)) return -1;
   /* Average line length (tile sizing of the fused kernel): caller's hint, else a 64 KiB sample. */
   if (s->line_hint > 0) {
      s->avg_line = s->line_hint;
   } else if (!(options & SEEQDEV_SINGLELINE) && nbytes && (s->avg_text != d_text || s->avg_nbytes != nbytes || ++s->sample_age >= 64)) {
      s->sample_age = 0;
      const size_t n = nbytes < SAMPLE_BYTES ? nbytes : SAMPLE_BYTES;
      HIP_TRY(hipMemcpyAsync(s->h_sample, d_text, n, hipMemcpyDeviceToHost, s->stream), EIO);
      HIP_TRY(hipStreamSynchronize(s->stream), EIO);
      size_t nl = 0;
      size_t foreign = 0;                                  /* bytes outside A C G T N (either case) and newline -- FASTA header lines included: their tiles take k_pair's slow path like any other (2-line FASTA records: 5.1 against 11.3 G lines/s on k_stream) */
      for (size_t i = 0; i < n; i++) {
         const uint8_t b = s->h_sample[i];
         nl += b == '\n';
         foreign += b != '\n' && sq_class_of(b, 0) >= 5;
      }
      s->avg_line = nl ? (double)n / (double)nl : 1e9;
      /* more than one foreign byte per 4 KB (FASTQ: every quality line; FASTA: a header per read): FASTA input of that kind stays
         with k_stream, FASTQ with k_pair (seeq_plan.h) */
      s->sample_dirty = foreign * 4096 > n;
      s->avg_text = d_text;
      s->avg_nbytes = nbytes;
   }
   return 0;
}

extern "C" int seeqdevScanRun(seeqdev_scan_t *s, const seeqdev_pattern_t *pat, const void *d_text, size_t nbytes,
                              int options, int want)
{
   if (scan_setup(s, pat, d_text, nbytes, options, want, SEEQ_HL_DIV)) return -1;
   if (dispatch_run(s)) return -1;
   s->ran = true;
   return 0;
}

/* What follows run number `run` of the context's scan, given its counters (per, npat: those of the patterns of a one-walk multi scan) --
   the policy is seeq_rerun.h's.  0: the counters are the result; 1: run again -- the fall-back flags are set, the workspace is reserved;
   2: not one walk after all (multi only); -1: error. */
static int rerun_next(seeqdev_scan *s, int run, const Counters &u, const Counters *per = NULL, int npat = 0)
{
   const RerunStep d = seeq_rerun_decide(run, {s->cap_lines, s->cap_hitlines, s->cap_records}, u, per, npat);
   s->fallback.note(d.note);
   if (d.verdict == RERUN_DONE) return 0;
   if (d.verdict == RERUN_NOT_ONE_WALK) return 2;
   if (d.verdict == RERUN_AGAIN) return reserve_impl(s, s->nbytes, d.cap.lines, d.cap.hitlines, d.cap.records) ? -1 : 1;
   const bool bad = d.verdict == RERUN_BAD_ENTRY;      /* (else: the last run the policy allows came back void too) */
   snprintf(g_last_error, sizeof g_last_error, "%s", bad ? "internal inconsistency in the hit list (k_stream_bounds)" : "workspace did not converge");
   errno = bad ? EIO : ENOMEM;
   return -1;
}

static seeqdev_counts_t counts_of(const Counters &h) { return {h.lines, h.matchlines, h.hits, h.records, h.headers}; }

/* ---- plumbing of the entries behind a scan (the FASTQ filter, demux, both strands, inserts, the tally) ---- */
/* a capacity as the kernels take it */
static uint32_t cap_u32(size_t cap) { return (uint32_t)(cap < 0xFFFFFFFFull ? cap : 0xFFFFFFFFull); }

/* Behind a run of launches: did they go out, and their counter block on its way to the (pinned) host copy. */
static int counters_copy(seeqdev_scan *s, void *h, const void *d, size_t bytes)
{
   HIP_TRY(hipGetLastError(), EIO);
   HIP_TRY(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s->stream), EIO);
   return 0;
}

/* ... and there: waits. */
static int counters_fetch(seeqdev_scan *s, void *h, const void *d, size_t bytes)
{
   if (counters_copy(s, h, d, bytes)) return -1;
   HIP_TRY(hipStreamSynchronize(s->stream), EIO);
   return 0;
}

/* Elements [first, first + n) of the `have` elements of `elem` bytes at the device address `base` -> host_out: the body of every
   seeqdevScanCopy* entry.  Waits. */
static int copy_out(seeqdev_scan *s, void *host_out, const void *base, size_t elem, size_t have, size_t first, size_t n)
{
   seeqerr = 0;
   if (!s || (!host_out && n) || first > have || n > have - first) { errno = EINVAL; return -1; }
   if (n == 0) return 0;
   if (use_device(s->device)) return -1;
   HIP_TRY(hipMemcpyAsync(host_out, (const char *)base + first * elem, n * elem, hipMemcpyDeviceToHost, s->stream), EIO);
   HIP_TRY(hipStreamSynchronize(s->stream), EIO);
   return 0;
}

/* SEEQDEV_FASTQ: the filter of seeq_fastq.h over the first n > 0 records of `in` (with their line offsets, or NULL) into the context's
   scratch arrays fq_rec / fq_off; *cnt: its counters, checked (demux: the tallies per pattern, and no lines are counted).  Waits. */
static int fastq_filter(seeqdev_scan *s, const void *in, const uint64_t *off_in, uint32_t n, bool demux, FastqCnt *cnt)
{
   const hipStream_t st = s->stream;
   FastqArgs a;
   memset(&a, 0, sizeof a);
   a.in = (const uint4 *)in; a.off_in = off_in;
   a.out = (uint4 *)s->fq_rec; a.off_out = s->fq_off;
   a.n = n; a.cap_out = cap_u32(s->cap_fq);
   a.nb = (uint32_t)seeq_tiles_of(n);
   a.bsum = s->fq_bsum;
   a.cnt = s->d_fqcnt;
   if (!s->fq_rec || !s->d_fqcnt || n > s->cap_fq || fastq_bsum_words(s->cap_fq) < 2 * (size_t)a.nb) {
      snprintf(g_last_error, sizeof g_last_error, "FASTQ filter: %u records, scratch for %zu", n, s->cap_fq);
      errno = EIO;
      return -1;
   }
   HIP_TRY(hipMemsetAsync(s->d_fqcnt, 0, sizeof(FastqCnt), st), EIO);
   if (demux) hipLaunchKernelGGL(k_fastq_reduce<true>, dim3(a.nb), dim3(SEEQ_TILE_WG), 0, st, a);
   else hipLaunchKernelGGL(k_fastq_reduce<false>, dim3(a.nb), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_fastq_top, dim3(1), dim3(SEEQ_TILE_WG), 0, st, a);
   hipLaunchKernelGGL(k_fastq_apply, dim3(a.nb), dim3(SEEQ_TILE_WG), 0, st, a);
   if (counters_fetch(s, s->h_fqcnt, s->d_fqcnt, sizeof(FastqCnt))) return -1;
   *cnt = *s->h_fqcnt;
   if (cnt->bad || cnt->kept > n || cnt->opened > cnt->kept) {
      snprintf(g_last_error, sizeof g_last_error, "internal inconsistency in the FASTQ filter (flags %u, %u of %u kept, %u lines)", cnt->bad, cnt->kept, n, cnt->opened);
      errno = EIO;
      return -1;
   }
   return 0;
}

/* The filter over the context's first n > 0 records; the filtered arrays become the context's records, and what was scanned into is the
   next filter's scratch (no copy back). */
static int fastq_filter_swap(seeqdev_scan *s, uint32_t n, FastqCnt *cnt)
{
   if (s->cap_fq != s->cap_records) {
      snprintf(g_last_error, sizeof g_last_error, "FASTQ filter: scratch for %zu records, record workspace for %zu", s->cap_fq, s->cap_records);
      errno = EIO;
      return -1;
   }
   if (fastq_filter(s, s->records, s->rec_off, n, false, cnt)) return -1;
   seeqdev_hit_t *r = s->records; s->records = s->fq_rec; s->fq_rec = r;
   uint64_t *o = s->rec_off; s->rec_off = s->fq_off; s->fq_off = o;
   return 0;
}

/* The flagged scan has converged with the counters h: filter its records, swap the filtered arrays in, fill s->counts. */
static int fastq_finish(seeqdev_scan *s, const Counters &h)
{
   if (h.records > 0xFFFFFFFFull) {
      snprintf(g_last_error, sizeof g_last_error, "SEEQDEV_FASTQ: more than 2^32 - 1 records to filter");
      errno = E2BIG;
      return -1;
   }
   FastqCnt f;
   f.kept = f.opened = 0;
   if (h.records && fastq_filter_swap(s, (uint32_t)h.records, &f)) return -1;
   s->counts.nlines = fastq_nlines(h.lines);
   s->counts.nmatchlines = f.opened;
   s->counts.nhits = s->fq_want == SEEQDEV_WANT_COUNTLINES ? f.opened : f.kept;
   s->counts.nrecords = s->fq_want == SEEQDEV_WANT_RECORDS ? f.kept : 0;
   s->counts.nheaders = 0;
   return 0;
}

extern "C" int seeqdevScanFetch(seeqdev_scan_t *s, seeqdev_counts_t *counts)
{
   seeqerr = 0;
   if (!s || !s->ran) { errno = EINVAL; return -1; }
   if (use_device(s->device)) return -1;
   for (int run = 0;; run++) {
      HIP_TRY(hipStreamSynchronize(s->stream), EIO);
      const Counters h = *s->h_cnt;
      const int next = rerun_next(s, run, h);
      if (next < 0) return -1;
      if (next == 0) {
         s->last_runs = run + 1;
         if (s->fastq) {
            if (!s->fq_done && fastq_finish(s, h)) return -1;
            s->fq_done = true;
         } else s->counts = counts_of(h);
         if (counts) *counts = s->counts;
         for (int i = 0; i < 4; i++) s->acc_ms[i] = 0.f;
         s->fwd_ms_avg = 0.f;
         for (size_t sg = 0; sg < s->prof_segs; sg++) {
            hipEvent_t *ev = s->ev + 4 * sg;
            float t01 = 0, t12 = 0, t23 = 0;
            if (sg == 0 && s->prof_segs > s->cap_launch_ms) {
               float *g = (float *)realloc(s->launch_ms, s->prof_segs * sizeof(float));
               if (g) { s->launch_ms = g; s->cap_launch_ms = s->prof_segs; }
            }
            (void)hipEventElapsedTime(&t01, ev[0], ev[1]);
            (void)hipEventElapsedTime(&t12, ev[1], ev[2]);
            (void)hipEventElapsedTime(&t23, ev[2], ev[3]);
            s->acc_ms[0] += t01; s->acc_ms[1] += t12; s->acc_ms[2] += t23; s->acc_ms[3] += t01 + t12 + t23;
            if (sg < s->cap_launch_ms) s->launch_ms[sg] = t12;
         }
         s->clk_mhz = 0.f;
         if (s->clk_valid && s->prof_segs && s->clk_probe && s->cap_clk_probe >= s->prof_segs) {
            double sum = 0; size_t nn = 0;
            for (size_t sg = 0; sg < s->prof_segs; sg++) {
               const unsigned long long *q = s->clk_probe + 4 * sg;
               if (q[3] > q[1] && q[2] > q[0]) { sum += (double)(q[2] - q[0]) / (double)(q[3] - q[1]) * 100.0; nn++; }      /* s_memrealtime: 100 MHz */
            }
            if (nn) s->clk_mhz = (float)(sum / (double)nn);
         }
         if (s->prof_segs) s->fwd_ms_avg = s->acc_ms[1] / (float)s->prof_segs;
         s->tm_h2d.read(s->prof);
         return 0;
      }
      if (dispatch_run(s)) return -1;
   }
}

extern "C" const seeqdev_hit_t *seeqdevScanRecordsDevice(const seeqdev_scan_t *s) { return s ? s->records : NULL; }

extern "C" int seeqdevScanCopyRecords(seeqdev_scan_t *s, seeqdev_hit_t *host_out, size_t first, size_t n)
{
   return copy_out(s, host_out, s ? s->records : NULL, sizeof(seeqdev_hit_t), s ? (size_t)s->counts.nrecords : 0, first, n);
}

/* A packed read batch resident in HBM (seeq_amd.h: seeqdev_packed_t, seeq_packed.h): asynchronous, seeqdevScanFetch waits. */
extern "C" int seeqdevScanPacked(seeqdev_scan_t *s, const seeqdev_pattern_t *pat, const seeqdev_packed_t *batch, int options, int want)
{
   seeqerr = 0;
   if (!scan_args_ok(s, &pat, 1, options, want) || !batch || (batch->nreads && !batch->bases)) { errno = EINVAL; return -1; }
   if (batch->read_len < 1 || batch->read_len > 256 || batch->stride < (batch->read_len + 3) / 4 ||
       (batch->nmask && batch->nstride < (batch->read_len + 7) / 8) || (options & (MASK_INPUT | SEEQDEV_FASTA | SEEQDEV_SINGLELINE | SEEQDEV_FASTQ))) { errno = EINVAL; return -1; }
   if (use_device(s->device)) return -1;
   s->fastq = false;
   seeqdev_pattern *mp = const_cast<seeqdev_pattern *>(pat);
   if (pat->wlen <= FUSED_MAX_WLEN2 && __atomic_load_n(&mp->pair_state, __ATOMIC_ACQUIRE) == 0) pattern_plan_pair(mp);
   if (pat->wlen <= FUSED_MAX_WLEN2 && mp->pair_state == 1 && __atomic_load_n(&mp->quad_state, __ATOMIC_ACQUIRE) == 0) pattern_plan_quad(mp);
   if (pat->wlen > FUSED_MAX_WLEN2 || mp->pair_state != 1) {
      /* not the packed walk's pattern (more than 62 positions, or no pair automaton): the batch is unpacked on the device and the
         ASCII scan runs over it -- the reference takes any pattern (libseeq.c:43-138), so does this entry */
      const size_t tbytes = (size_t)batch->nreads * (batch->read_len + 1u);
      if (ws_grow(&s->ws, &s->cap_unpack, tbytes, {{s->d_unpack, tbytes + 64}})) return -1;
      if (batch->nreads) {
         const uint64_t threads = batch->nreads * (uint64_t)(batch->read_len / 16u + 1u), blocks = (threads + 255) / 256;
         if (blocks > 0x7FFFFFFFull) { errno = E2BIG; return -1; }
         hipLaunchKernelGGL(k_unpack_ascii, dim3((unsigned)blocks), dim3(256), 0, s->stream, (const uint8_t *)batch->bases, (const uint8_t *)batch->nmask,
                            batch->nreads, batch->read_len, batch->stride, batch->nstride, s->d_unpack);
         HIP_TRY(hipGetLastError(), EIO);
      }
      s->avg_text = NULL;                                   /* (new contents behind the same pointer: sample again) */
      return seeqdevScanRun(s, pat, s->d_unpack, tbytes, options, want);
   }
   s->pat = pat; s->text = NULL; s->nbytes = 0; s->options = options; s->want = want;
   s->ran = false;
   s->is_packed = true;
   s->packed = *batch;
   const RerunCaps w = seeq_first_reservation_packed(batch->nreads < s->pk_seg_reads ? (size_t)batch->nreads : s->pk_seg_reads,
                                                     {s->cap_lines, s->cap_hitlines, s->cap_records}, s->user_reserved);
   if (reserve_impl(s, 1, w.lines, w.hitlines, w.records)) return -1;
   if (dispatch_run(s)) return -1;
   s->ran = true;
   return 0;
}

/* The same for ASCII reads resident in HBM (one per line, each read_len bases + '\n'): device to device, asynchronous on `hip_stream`. */
extern "C" int seeqdevPackReadsDevice(const void *d_text, uint64_t nreads, uint32_t read_len, void *d_bases, void *d_nmask, uint32_t stride, uint32_t nstride,
                                      void *hip_stream)
{
   seeqerr = 0;
   if ((!d_text || !d_bases) && nreads) { errno = EINVAL; return -1; }
   if (read_len < 1 || read_len > 256 || stride < (read_len + 3) / 4 || (d_nmask && nstride < (read_len + 7) / 8)) { errno = EINVAL; return -1; }
   if (nreads == 0) return 0;
   const uint64_t blocks = (nreads + 255) / 256;
   if (blocks > 0x7FFFFFFFull) { errno = E2BIG; return -1; }
   hipLaunchKernelGGL(k_pack_ascii, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, (const uint8_t *)d_text, nreads, read_len,
                      (uint8_t *)d_bases, (uint8_t *)d_nmask, stride, nstride);
   HIP_TRY(hipGetLastError(), EIO);
   return 0;
}

/* ASCII reads, one per line, every line exactly read_len bases -> the packed layout (host helper for callers that hold text:
 * a caller that holds packed reads already -- BAM, .2bit -- fills seeqdev_packed_t itself).  A C G T U N in either case; any
 * other byte, or a line of another length: -1, errno = EINVAL.  Returns the number of reads. */
extern "C" long seeqdevPackReads(const char *text, size_t nbytes, uint32_t read_len, void *bases_out, void *nmask_out, uint32_t stride, uint32_t nstride)
{
   seeqerr = 0;
   if (!text || !bases_out || read_len < 1 || read_len > 256 || stride < (read_len + 3) / 4 || (nmask_out && nstride < (read_len + 7) / 8)) { errno = EINVAL; return -1; }
   uint8_t *bo = (uint8_t *)bases_out, *no = (uint8_t *)nmask_out;
   long r = 0;
   size_t p = 0;
   while (p < nbytes) {
      if (p + read_len > nbytes) { errno = EINVAL; return -1; }
      uint8_t *b = bo + (size_t)r * stride, *n = no ? no + (size_t)r * nstride : NULL;
      memset(b, 0, stride);
      if (n) memset(n, 0, nstride);
      for (uint32_t i = 0; i < read_len; i++) {
         const unsigned char ch = (unsigned char)text[p + i];
         const unsigned char up = ch & 0xDF;
         unsigned code;
         if (up == 'A' || up == 'C' || up == 'G' || up == 'T' || up == 'U') code = (ch >> 1) & 3u;
         else if (up == 'N') { code = 0; if (!n) { errno = EINVAL; return -1; } n[i >> 3] |= (uint8_t)(0x80u >> (i & 7)); }
         else { errno = EINVAL; return -1; }
         b[i >> 2] |= (uint8_t)(code << (6 - 2 * (i & 3)));
      }
      p += read_len;
      if (p < nbytes) { if (text[p] != '\n') { errno = EINVAL; return -1; } p++; }
      r++;
   }
   return r;
}

#include "seeq_text_alloc.h"

extern "C" int seeqdevScanCopyOffsets(seeqdev_scan_t *s, uint64_t *host_out, size_t first, size_t n)
{
   return copy_out(s, host_out, s ? s->rec_off : NULL, sizeof(uint64_t), s ? (size_t)s->counts.nrecords : 0, first, n);
}

/* The context's staging buffer holds nbytes (grown with a quarter to spare) */
static int text_ensure(seeqdev_scan *s, size_t nbytes)
{
   if (nbytes <= s->cap_text) return 0;
   const size_t cap = nbytes + (nbytes >> 2) + 4096;
   return ws_grow(&s->ws, &s->cap_text, cap, {{s->d_text, cap}});
}

/* Host text into the context's staging buffer, on its stream (timed: between the H2D events).  New contents behind the same pointer:
   the line length is sampled again */
static int text_upload(seeqdev_scan *s, const char *host_text, size_t nbytes, bool timed)
{
   if (text_ensure(s, nbytes)) return -1;
   if (s->tm_h2d.begin(timed, s->stream)) return -1;
   if (nbytes) HIP_TRY(hipMemcpyAsync(s->d_text, host_text, nbytes, hipMemcpyHostToDevice, s->stream), EIO);
   if (s->tm_h2d.end(timed, s->stream)) return -1;
   s->avg_text = NULL;
   s->ins_staged = false;                                  /* (staged_text: the staged text of the last inserts call is gone) */
   return 0;
}

/* An entry that was given no text (*d_text NULL) works on the staged text of the last inserts call (seeqdevScanHostInserts), or refuses
   under its own name `who`. */
static int staged_text(seeqdev_scan *s, const char *who, const void **d_text, size_t *nbytes)
{
   if (*d_text) return 0;
   if (!s->ins_staged) {
      snprintf(g_last_error, sizeof g_last_error, "%s: the context holds no staged text of an inserts call", who);
      errno = EINVAL;
      return -1;
   }
   *d_text = s->d_text;
   *nbytes = s->ins_staged_nbytes;
   return 0;
}

/* The first n records of the scan just fetched, with their offsets, copied aside on the device (16 + 8 bytes per record) before the call's
   next scan overwrites them: the one owner of the side copy (the both-strands call's plus records, the inserts call's right records).  Waits. */
static int side_keep(seeqdev_scan *s, size_t n)
{
   if (!n) return 0;
   if (ws_grow(&s->ws, &s->cap_side, n, {{s->side_rec, n * sizeof(seeqdev_hit_t)}, {s->side_off, n * sizeof(uint64_t)}})) return -1;
   HIP_TRY(hipMemcpyAsync(s->side_rec, s->records, n * sizeof(seeqdev_hit_t), hipMemcpyDeviceToDevice, s->stream), EIO);
   HIP_TRY(hipMemcpyAsync(s->side_off, s->rec_off, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s->stream), EIO);
   HIP_TRY(hipStreamSynchronize(s->stream), EIO);            /* the next scan may reallocate the records the copies read */
   return 0;
}

extern "C" int seeqdevScanHostBegin(seeqdev_scan_t *s, const seeqdev_pattern_t *pat, const char *host_text, size_t nbytes,
                                    int options, int want)
{
   seeqerr = 0;
   if (!s || !pat || (!host_text && nbytes)) { errno = EINVAL; return -1; }
   if (use_device(s->device)) return -1;
   if (text_upload(s, host_text, nbytes, s->prof)) return -1;
   /* the line-length sample (kernel selection) comes from the host copy: no round trip, nothing stale */
   if (s->line_hint <= 0 && !(options & SEEQDEV_SINGLELINE) && nbytes) {
      const size_t n = nbytes < SAMPLE_BYTES ? nbytes : SAMPLE_BYTES;
      size_t nl = 0;
      for (size_t i = 0; i < n; i++) nl += host_text[i] == '\n';
      s->avg_line = nl ? (double)n / (double)nl : 1e9;
      s->avg_text = s->d_text;
      s->avg_nbytes = nbytes;
   }
   return seeqdevScanRun(s, pat, s->d_text, nbytes, options, want);
}

extern "C" int seeqdevScanHost(seeqdev_scan_t *s, const seeqdev_pattern_t *pat, const char *host_text, size_t nbytes,
                               int options, int want, seeqdev_counts_t *counts)
{
   if (seeqdevScanHostBegin(s, pat, host_text, nbytes, options, want)) return -1;
   return seeqdevScanFetch(s, counts);
}

#include "seeq_multi_host.h"
#include "seeq_demux_host.h"
#include "seeq_strand_host.h"
#include "seeq_insert_host.h"
#include "seeq_tally_host.h"
#include "seeq_tally_group_host.h"
#include "seeq_tally_library_host.h"
#include "seeq_tally_collapse_host.h"
#include "seeq_tally_held_host.h"
#include "seeq_qgate_host.h"
#include "seeq_anchor_host.h"

extern "C" int seeqdevScanLastCopyMs(const seeqdev_scan_t *s, float *h2d_ms)
{
   if (!s || !h2d_ms) { errno = EINVAL; return -1; }
   *h2d_ms = s->tm_h2d.ms;
   return 0;
}

extern "C" int seeqdevScanLastLaunches(const seeqdev_scan_t *s) { return s ? (int)s->prof_segs : 0; }

extern "C" float seeqdevScanLastClockMHz(const seeqdev_scan_t *s) { return s ? s->clk_mhz : 0.f; }

extern "C" int seeqdevScanLastLaunchTimes(const seeqdev_scan_t *s, float *ms, int cap)
{
   if (!s || (!ms && cap > 0)) { errno = EINVAL; return -1; }
   const size_t n = s->prof_segs < s->cap_launch_ms ? s->prof_segs : s->cap_launch_ms;
   for (size_t i = 0; i < n && (int)i < cap; i++) ms[i] = s->launch_ms[i];
   return (int)n;
}

#include "seeq_string.h"
