/*
 * seeq_tally_library.h -- counting spans against a KNOWN library: a guide library of a screen, a barcode whitelist.  A span's tally key
 * (seeq_tally.h) is replaced, on the device, by the number of the library entry it is -- exactly, with one substitution, or (the edit
 * mode) with one substitution, insertion or deletion -- and the tally's own sort, run-length pass and table then count entry numbers
 * instead of observed sequences: one row per library entry seen, a read with one sequencing error counted for the entry it came from,
 * and ceil(bitlen(N) / 8) passes of the sort instead of ceil((2 * max_len + 1) / 8).
 *
 * The rule -- plain C++ below, shared with the host drivers (tests/tally_library_host_driver.cpp and tests/tally_library_edit_host_driver.cpp
 * compile this header with g++):
 *
 *   library      N >= 1 tally keys in the caller's order, each a valid key (tally_key_len >= 0), pairwise distinct, lengths mixed
 *                freely; N <= SEEQ_TLIB_MAX = 2^24 - 1.  THE ID of entry i is i + 1; id 0 is "no entry".  On the device: the keys
 *                ascending with the ids beside them (tally_lib_prepare sorts and validates on the host).
 *   neighbour    of a key k of length L at position 0 <= p < L with s in {1, 2, 3}: k ^ (s << 2(L - 1 - p)), the three other bases
 *                there (tally_neighbour).  It has k's length; a key has 3 L of them, the empty key none.  Substitutions only: an
 *                insertion or deletion changes the length and makes no neighbour -- but under the edit mode, below.
 *   assignment   of a span's key k under max_mismatch 0 or 1 (tally_lib_assign):
 *                  k is in the library                          -> its id, EXACT (whatever neighbours of k are in it too);
 *                  else, max_mismatch 1, H = the library entries that are neighbours of k:
 *                     |H| == 1 -> that entry's id, CORRECTED;   |H| >= 2 -> 0, AMBIGUOUS;   |H| == 0 -> 0, UNKNOWN;
 *                  else, max_mismatch 0                         -> 0, UNKNOWN.
 *   edit mode    (SEEQ_TLIB_MODE_EDIT; tally_lib_assign_mode) three classes of neighbour, disjoint because their lengths differ:
 *                  substitution  as above, length L, 3 L of them;
 *                  deletion      (the read carries one base too many) base p of k removed, length L - 1 (tally_del_neighbour), taken only at
 *                                the canonical positions p == 0 || base[p] != base[p - 1], one per run of equal bases; L == 0 has none,
 *                                L == 1 gives the empty key;
 *                  insertion     (the read lost a base) base c put in front of position p, 0 <= p <= L, length L + 1
 *                                (tally_ins_neighbour), taken only where p == 0 || c != base[p - 1] -- 3 L + 4 of them -- and only for
 *                                L <= 30: a key of 32 bases does not exist.
 *                The canonical conditions make the neighbours of one class pairwise distinct keys, so "entries found" is a sum as in the
 *                substitution pass (without them AAAA finds the entry AAA four times and is called ambiguous); the union of the three
 *                classes is exactly the keys at Levenshtein distance 1.  Exact wins; else H = the entries among all neighbours of the
 *                three classes: |H| == 1 -> that id, CORRECTED -- substituted, inserted or deleted by the class it came from
 *                (SEEQ_TLIB_BY_*); |H| >= 2 -> 0, AMBIGUOUS (an entry one substitution away and another one deletion away are two);
 *                |H| == 0 -> 0, UNKNOWN.  ncorrected = nsubstituted + ninserted + ndeleted.
 *   long, foreign, bad spans are decided first and exactly as in the plain tally (key 0): the library never sees them.  A 31-base entry
 *                whose read GAINED a base is a span of 32 bytes: long, and it stays lost under every mode.
 *   counts       nspans = nexact + ncorrected + nambiguous + nunknown + nlong + nforeign;  nassigned = nexact + ncorrected.
 *   table        one {key = id, count} per id that occurs, ids ascending; the counts sum to nassigned.
 *   passes       of the sort over ids: ceil(bitlen(N) / 8) when anything was assigned, else 0 (tally_lib_passes).
 *
 * The kernels sit between k_tally_pack and the sort, and rewrite the key array IN PLACE (the tally's other kernels run as they are):
 *
 *   the search             a lower bound over the sorted library keys in two levels: a workgroup keeps every stride-th key, 256 samples,
 *                          in LDS (stride = ceil(N / 256)) and a search takes its first eight steps there; what is left is a range of at
 *                          most stride keys of the library itself, searched in at most bitlen(stride) + 1 steps -- a host-known count.
 *                          (A search of bitlen(N) dependent loads from the L2 cost 0.58 ms for 0.9 M misses of 20-mers.)  Every
 *                          search of the rule side is tally_lower_bound, the one halving loop -- over keys or over a column of a 24-byte
 *                          table (seeq_tally_collapse.h); tally_lib_lower_bound / _top are calls to it, and the driver checks the two
 *                          levels against the one search of the whole array.
 *   k_tally_assign_exact   one thread per span, in the tiles of seeq_tiles.h: the search of the span's key, the four searches of a
 *                          thread stepped together (four independent loads in flight).  A found key stores its id AT THE SPAN'S OWN INDEX; a
 *                          nonzero key that is not found is a MISS and stores 0 -- or, when the near pass will follow, the key with
 *                          SEEQ_TLIB_MISS (bit 63, which no key and no id has) set, so that the next two kernels know it from an id.
 *                          Per tile {misses, exact}, through ballots and LDS (tile_sums).
 *   k_tally_assign_top     one workgroup: the exclusive prefix of the tiles' misses in place, the two totals (tile_top).
 *   k_tally_miss_apply     (max_mismatch 1, misses > 0) the ordered compaction of the miss INDICES, 4 bytes per miss, into the key
 *                          array the sort has not touched yet.
 *   k_tally_assign_near    a grid sized by the host-known miss count, 64 misses per workgroup in eight rounds: half a wave (32 lanes >=
 *                          L) owns one miss, lane p < L searches the three neighbours at position p (stepped together), the half sums
 *                          (neighbours found, ids found) with __shfl_xor at distances 16 .. 1, and its lane 0 stores the id when exactly
 *                          one was found, else 0.  Per workgroup {corrected, ambiguous, unknown, bad}.
 *   k_tally_assign_near_edit  the same pass in its second instance (one template, tally_assign_near<EDIT>), for the edit mode, with the
 *                          same geometry: lane p owns its three substitutions (p < L), the deletion at p (p < L, canonical) and the
 *                          insertions in front of p (p <= L <= 30: four for lane 0, three for the others); its at most eight searches are
 *                          stepped together, eight independent loads in flight.  The half sums (entries found, ids found, the class of
 *                          what was found) in two words; per workgroup two more counts, {inserted, deleted} of the corrected.
 *   k_tally_near_top       one workgroup: their totals, the edit instance's two counts too (of a workgroup per 8 misses it took 0.12 ms
 *                          for 0.9 M misses: hence the rounds).
 *
 * Compacting first makes the near pass's work proportional to misses x L: one thread per span doing all 3 L searches would leave a
 * 64-lane wave walking 3 L dependent searches for the few lanes that missed.
 *
 * Every output slot is written by exactly one thread per launch; no atomics on global memory; no workgroup waits on another; every
 * loop is bounded by a count the host knows; the grids come from host-known counts (no span, no miss: nothing is launched).
 */
#ifndef SEEQ_TALLY_LIBRARY_H_
#define SEEQ_TALLY_LIBRARY_H_

#include <stdint.h>
#include <stddef.h>

#include "seeq_tally.h"

#define SEEQ_TLIB_MAX       0xFFFFFFu                       /* entries of a library: ids of 24 bits, three passes at the most */
#define SEEQ_TLIB_MISS      0x8000000000000000ull           /* marks a missed key between the exact and the near pass */
#define SEEQ_TLIB_NEAR_WG   8                               /* misses per round of a workgroup of k_tally_assign_near: its half-waves */
#define SEEQ_TLIB_NEAR_ROUNDS 8                             /* rounds of such a workgroup: 64 misses, one {corrected, ambiguous, unknown, bad} */
#define SEEQ_TLIB_TOP       256                             /* sampled library keys a workgroup keeps in LDS: one per thread */

#define SEEQ_TLIB_EXACT     0                               /* what a span with a key is to the library */
#define SEEQ_TLIB_CORRECTED 1
#define SEEQ_TLIB_AMBIGUOUS 2
#define SEEQ_TLIB_UNKNOWN   3

#define SEEQ_TLIB_MODE_EXACT 0                              /* the library's mode = SEEQDEV_LIBRARY_* (seeq_amd.h): exact only; */
#define SEEQ_TLIB_MODE_SUBST 1                              /* ... or one substitution (max_mismatch 1); */
#define SEEQ_TLIB_MODE_EDIT  2                              /* ... or one edit: a substitution, an insertion or a deletion */

#define SEEQ_TLIB_BY_SUBST  0                               /* the class of the neighbour a corrected span was found by: of its own length; */
#define SEEQ_TLIB_BY_INS    1                               /* ... one base longer (the read lost a base); */
#define SEEQ_TLIB_BY_DEL    2                               /* ... one base shorter (the read carries one base too many) */
#define SEEQ_TLIB_INS_LEN_MAX 30                            /* the longest key with insertion neighbours: a key of 32 bases does not exist */
#define SEEQ_TLIB_EDIT_SEARCHES 8                           /* searches of a lane of the edit pass: 3 substitutions, 1 deletion, 4 insertions */

#define SEEQ_TLIB_E_NOKEY   1                               /* tally_lib_prepare: a value that is no key; a duplicate; too many entries */
#define SEEQ_TLIB_E_DUP     2
#define SEEQ_TLIB_E_MANY    3

/* the neighbour of a key of len bases: another base, s in {1, 2, 3}, at position p < len */
SEEQ_ST_HD uint64_t tally_neighbour(uint64_t key, uint32_t len, uint32_t p, uint32_t s) { return key ^ ((uint64_t)s << (2u * (len - 1u - p))); }

/* base p < len of a key of len bases: its code (A C T G = 0 1 2 3) */
SEEQ_ST_HD uint32_t tally_key_base(uint64_t key, uint32_t len, uint32_t p) { return (uint32_t)(key >> (2u * (len - 1u - p))) & 3u; }

/* THE DELETION NEIGHBOUR of a key of len >= 1 bases: base p < len removed, len - 1 bases.  Removing any base of a run of equal bases gives
   the same key: tally_del_canonical names one position per run, its first. */
SEEQ_ST_HD uint64_t tally_del_neighbour(uint64_t key, uint32_t len, uint32_t p)
{
   const uint32_t low = 2u * (len - 1u - p);                /* bits of the bases behind p */
   return ((key >> (low + 2u)) << low) | (key & ((1ull << low) - 1ull));
}

SEEQ_ST_HD int tally_del_canonical(uint64_t key, uint32_t len, uint32_t p) { return p == 0u || tally_key_base(key, len, p) != tally_key_base(key, len, p - 1u); }

/* THE INSERTION NEIGHBOUR of a key of len <= SEEQ_TLIB_INS_LEN_MAX bases: base c in front of position p <= len, len + 1 bases.  Putting a
   base in front of or behind an equal one gives the same key: tally_ins_canonical keeps the one in front of the run, 3 len + 4 in all. */
SEEQ_ST_HD uint64_t tally_ins_neighbour(uint64_t key, uint32_t len, uint32_t p, uint32_t c)
{
   const uint32_t low = 2u * (len - p);                     /* bits of the bases from p on */
   return ((((key >> low) << 2) | (uint64_t)c) << low) | (key & ((1ull << low) - 1ull));
}

SEEQ_ST_HD int tally_ins_canonical(uint64_t key, uint32_t len, uint32_t p, uint32_t c) { return p == 0u || c != tally_key_base(key, len, p - 1u); }

SEEQ_ST_HD uint32_t tally_lib_bitlen(uint64_t n) { return n ? 64u - (uint32_t)__builtin_clzll(n) : 0u; }

/* steps that bound a lower-bound search over n sorted keys (bitlen(n) halvings empty the range; one to spare) */
SEEQ_ST_HD uint32_t tally_lib_probes(uint32_t n) { return tally_lib_bitlen(n) + 1u; }

/* passes of the sort over ids 1 .. n: their bitlen(n) bits in digits of 8; 0 when nothing was assigned */
SEEQ_ST_HD uint32_t tally_lib_passes(uint64_t nassigned, uint32_t n) { return nassigned ? (tally_lib_bitlen(n) + 7u) / 8u : 0u; }

/* One step of a lower-bound search for `key` over the ascending 64-bit keys keys[stride * i], lo <= i < hi (stride in words: 1 for an array
   of keys, 3 for a column of a 24-byte table): the range is halved; an empty one stays as it is.  The kernels that advance several
   searches in lock step call this once per search and step. */
SEEQ_ST_HD void tally_bound_step(const uint64_t *keys, uint32_t stride, uint64_t key, uint32_t *lo, uint32_t *hi)
{
   if (*lo < *hi) {
      const uint32_t mid = *lo + (*hi - *lo) / 2u;
      if (keys[(uint64_t)stride * mid] < key) *lo = mid + 1u;
      else *hi = mid;
   }
}

/* THE LOWER BOUND, the one of the rule side: lo + the keys below `key` among keys[stride * i], lo <= i < hi, ascending; at most `probes`
   steps. */
SEEQ_ST_HD uint32_t tally_lower_bound(const uint64_t *keys, uint32_t stride, uint32_t lo, uint32_t hi, uint32_t probes, uint64_t key)
{
#if defined(__HIPCC__)
#pragma unroll 1
#endif
   for (uint32_t it = 0; it < probes && lo < hi; it++) tally_bound_step(keys, stride, key, &lo, &hi);
   return lo;
}

/* THE TOP OF THE SEARCH, kept in LDS by the kernels: every stride-th key of the library, SEEQ_TLIB_TOP samples with the largest 64-bit
   value (no key has bit 63) behind the last one.  The first eight steps of every search run over it; what is left for the library
   itself is a range of at most stride keys. */
SEEQ_ST_HD uint32_t tally_lib_stride(uint32_t n) { return n ? (n + SEEQ_TLIB_TOP - 1u) / SEEQ_TLIB_TOP : 1u; }

SEEQ_ST_HD uint64_t tally_lib_sample(const uint64_t *lkey, uint32_t n, uint32_t stride, uint32_t i)
{
   const uint64_t at = (uint64_t)i * stride;
   return at < n ? lkey[at] : ~0ull;
}

/* [*lo, *hi]: where the lower bound of `key` (bit 63 clear) lies, from the samples top[0 .. SEEQ_TLIB_TOP): with c samples below the key,
   lkey[(c - 1) * stride] < key <= lkey[c * stride] (or the end). */
SEEQ_ST_HD void tally_lib_top_range(const uint64_t *top, uint32_t n, uint32_t stride, uint64_t key, uint32_t *lo, uint32_t *hi)
{
   uint32_t c = 0;                                          /* samples below the key among the first SEEQ_TLIB_TOP - 1, then the last one */
   for (uint32_t step = SEEQ_TLIB_TOP / 2u; step; step >>= 1) c += top[c + step - 1u] < key ? step : 0u;
   c += top[c] < key ? 1u : 0u;
   const uint64_t end = (uint64_t)c * stride;
   *lo = c ? (c - 1u) * stride + 1u : 0u;
   *hi = end < n ? (uint32_t)end : n;
}

/* library keys below `key` among lkey[0 .. n), ascending: by one search of the whole array, and by both levels -- the samples, then at most
   `probes` = tally_lib_probes(stride) steps over the range they leave (what the kernels do, and what the host driver checks against the
   first) */
SEEQ_ST_HD uint32_t tally_lib_lower_bound(const uint64_t *lkey, uint32_t n, uint32_t probes, uint64_t key) { return tally_lower_bound(lkey, 1u, 0u, n, probes, key); }

SEEQ_ST_HD uint32_t tally_lib_lower_bound_top(const uint64_t *top, const uint64_t *lkey, uint32_t n, uint32_t stride, uint32_t probes, uint64_t key)
{
   uint32_t lo, hi;
   tally_lib_top_range(top, n, stride, key, &lo, &hi);
   return tally_lower_bound(lkey, 1u, lo, hi, probes, key);
}

/* the id of `key` in the library, 0: it is no entry */
SEEQ_ST_HD uint32_t tally_lib_find(const uint64_t *lkey, const uint32_t *lid, uint32_t n, uint32_t probes, uint64_t key)
{
   const uint32_t at = tally_lib_lower_bound(lkey, n, probes, key);
   return at < n && lkey[at] == key ? lid[at] : 0u;
}

/* The assignment of a span's key (a valid one): its id or 0, and *kind: SEEQ_TLIB_EXACT / _CORRECTED / _AMBIGUOUS / _UNKNOWN. */
SEEQ_ST_HD uint32_t tally_lib_assign(const uint64_t *lkey, const uint32_t *lid, uint32_t n, uint32_t probes, uint64_t key, int max_mismatch, int *kind)
{
   const uint32_t id = tally_lib_find(lkey, lid, n, probes, key);
   if (id) { *kind = SEEQ_TLIB_EXACT; return id; }
   *kind = SEEQ_TLIB_UNKNOWN;
   if (max_mismatch < 1) return 0u;
   const int len = tally_key_len(key);
   uint32_t nfound = 0, found = 0;
   for (int p = 0; p < len; p++)
      for (uint32_t s = 1; s <= 3u; s++) {
         const uint32_t h = tally_lib_find(lkey, lid, n, probes, tally_neighbour(key, (uint32_t)len, (uint32_t)p, s));
         if (h) { nfound++; found = h; }
      }
   if (nfound == 1u) { *kind = SEEQ_TLIB_CORRECTED; return found; }
   if (nfound >= 2u) *kind = SEEQ_TLIB_AMBIGUOUS;
   return 0u;
}

/* The assignment under a MODE (SEEQ_TLIB_MODE_*): modes 0 and 1 are tally_lib_assign with that max_mismatch; mode 2 counts the entries
   among the neighbours of all three classes.  *by: the class of the one neighbour found (SEEQ_TLIB_BY_*) of a corrected span, else -1. */
SEEQ_ST_HD uint32_t tally_lib_assign_mode(const uint64_t *lkey, const uint32_t *lid, uint32_t n, uint32_t probes, uint64_t key, int mode, int *kind, int *by)
{
   *by = -1;
   if (mode != SEEQ_TLIB_MODE_EDIT) {
      const uint32_t id = tally_lib_assign(lkey, lid, n, probes, key, mode, kind);
      if (*kind == SEEQ_TLIB_CORRECTED) *by = SEEQ_TLIB_BY_SUBST;
      return id;
   }
   const uint32_t id = tally_lib_find(lkey, lid, n, probes, key);
   if (id) { *kind = SEEQ_TLIB_EXACT; return id; }
   const uint32_t len = (uint32_t)tally_key_len(key);
   uint32_t nfound = 0, found = 0;
   for (uint32_t p = 0; p < len; p++) {
      for (uint32_t s = 1; s <= 3u; s++) {
         const uint32_t h = tally_lib_find(lkey, lid, n, probes, tally_neighbour(key, len, p, s));
         if (h) { nfound++; found = h; *by = SEEQ_TLIB_BY_SUBST; }
      }
      if (tally_del_canonical(key, len, p)) {
         const uint32_t h = tally_lib_find(lkey, lid, n, probes, tally_del_neighbour(key, len, p));
         if (h) { nfound++; found = h; *by = SEEQ_TLIB_BY_DEL; }
      }
   }
   for (uint32_t p = 0; p <= len && len <= SEEQ_TLIB_INS_LEN_MAX; p++)
      for (uint32_t c = 0; c <= 3u; c++) {
         if (!tally_ins_canonical(key, len, p, c)) continue;
         const uint32_t h = tally_lib_find(lkey, lid, n, probes, tally_ins_neighbour(key, len, p, c));
         if (h) { nfound++; found = h; *by = SEEQ_TLIB_BY_INS; }
      }
   *kind = nfound == 1u ? SEEQ_TLIB_CORRECTED : nfound >= 2u ? SEEQ_TLIB_AMBIGUOUS : SEEQ_TLIB_UNKNOWN;
   if (nfound == 1u) return found;
   *by = -1;
   return 0u;
}

#include <algorithm>

/* The library as the device holds it: skey[0 .. n) the keys ascending, sid[0 .. n) their ids (position in `keys` + 1).  0: done;
   SEEQ_TLIB_E_MANY: n > SEEQ_TLIB_MAX (nothing is read); SEEQ_TLIB_E_NOKEY: keys[*at] is no key; SEEQ_TLIB_E_DUP: keys[*at] repeats an
   earlier entry.  Of several faults the one at the smallest index is reported, a value that is no key before a duplicate. */
static inline int tally_lib_prepare(const uint64_t *keys, size_t n, uint64_t *skey, uint32_t *sid, size_t *at)
{
   *at = 0;
   if (n > SEEQ_TLIB_MAX) return SEEQ_TLIB_E_MANY;
   for (size_t i = 0; i < n; i++)
      if (tally_key_len(keys[i]) < 0) { *at = i; return SEEQ_TLIB_E_NOKEY; }
   for (size_t i = 0; i < n; i++) sid[i] = (uint32_t)i + 1u;
   std::sort(sid, sid + n, [keys](uint32_t a, uint32_t b) { return keys[a - 1u] != keys[b - 1u] ? keys[a - 1u] < keys[b - 1u] : a < b; });
   size_t dup = n;
   for (size_t i = 0; i < n; i++) {
      skey[i] = keys[sid[i] - 1u];
      if (i && skey[i] == skey[i - 1] && (size_t)sid[i] - 1u < dup) dup = (size_t)sid[i] - 1u;      /* (equal keys lie in id order: sid[i] is the repeat) */
   }
   if (dup < n) { *at = dup; return SEEQ_TLIB_E_DUP; }
   return 0;
}

#if defined(__HIPCC__)

static_assert(SEEQ_TLIB_TOP == SEEQ_TILE_WG, "a thread per sample of the top");

struct TallyLibCnt {
   uint32_t nexact, nmiss;            /* k_tally_assign_top: spans found in the library; nonzero keys that were not */
   uint32_t ncorrected, nambiguous, nunknown;      /* k_tally_near_top: what the misses were */
   uint32_t bad;                      /* 2: an index outside an array (an internal error) */
   uint32_t ninserted, ndeleted;      /* k_tally_near_top, the edit mode: the corrected that were found by an insertion, by a deletion */
};

struct TallyLibArgs {
   uint64_t       *key;               /* [n] in: the spans' keys (0: not tallied); out: their ids (0: not assigned) */
   uint32_t        n;
   uint32_t        nt;                /* tiles = workgroups of the per-tile kernels */
   const uint64_t *lkey;              /* [nlib] the library's keys, ascending */
   const uint32_t *lid;               /* [nlib] their ids */
   uint32_t        nlib, stride;      /* entries; entries per sample of the top (tally_lib_stride) */
   uint32_t        probes;            /* steps over the library behind the top: tally_lib_probes(stride) */
   uint32_t        near;              /* the near pass follows: a miss keeps its key, marked */
   uint32_t       *esum;              /* [2 * nt] per tile misses (k_tally_assign_top: exclusive prefix), exact */
   uint32_t       *miss;              /* [nmiss] the misses' indices, ascending */
   uint32_t        nmiss;
   uint32_t        nwg;               /* workgroups of k_tally_assign_near: one per SEEQ_TLIB_NEAR_WG * SEEQ_TLIB_NEAR_ROUNDS misses */
   uint4          *nstat;             /* [nwg] {corrected, ambiguous, unknown, bad} */
   uint2          *nedit;             /* [nwg] the edit mode: {inserted, deleted} of the corrected; NULL otherwise */
   TallyLibCnt    *cnt;
};

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_assign_exact(TallyLibArgs a)
{
   __shared__ uint32_t s_sum[2][SEEQ_TILE_WAVES];
   __shared__ uint64_t s_top[SEEQ_TLIB_TOP];
   uint64_t key[SEEQ_TILE_ITEMS];
   uint32_t lo[SEEQ_TILE_ITEMS], hi[SEEQ_TILE_ITEMS];
   s_top[threadIdx.x] = tally_lib_sample(a.lkey, a.nlib, a.stride, threadIdx.x);
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      key[k] = i < a.n ? a.key[i] : 0u;
   }
   __syncthreads();
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      tally_lib_top_range(s_top, a.nlib, a.stride, key[k], &lo[k], &hi[k]);
      if (!key[k]) lo[k] = hi[k] = 0u;                      /* (a span without a key searches nothing) */
   }
#pragma unroll 1
   for (uint32_t it = 0; it < a.probes; it++) {
#pragma unroll
      for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
         tally_bound_step(a.lkey, 1u, key[k], &lo[k], &hi[k]);      /* (mid < hi <= nlib) */
      }
   }
   uint32_t sum[2] = {0u, 0u};                              /* misses, exact: wave-uniform */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      bool found = false, miss = false;
      if (key[k]) {
         found = lo[k] < a.nlib && a.lkey[lo[k]] == key[k];
         miss = !found;
         a.key[tile_index(k)] = found ? (uint64_t)a.lid[lo[k]] : a.near ? (key[k] | SEEQ_TLIB_MISS) : 0u;
      }
      sum[0] += (uint32_t)__popcll(__ballot(miss));
      sum[1] += (uint32_t)__popcll(__ballot(found));
   }
   tile_sums(sum, s_sum, a.esum, a.nt);
}

/* One workgroup: esum[0 .. nt) -> its exclusive prefix, in place; the misses and the exact spans. */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_assign_top(TallyLibArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES];
   uint32_t tot[2];
   tile_top(a.esum, a.nt, s_wave, tot);
   if (threadIdx.x == 0) { a.cnt->nmiss = tot[0]; a.cnt->nexact = tot[1]; }
}

/* the ordered compaction of the misses: a marked key's index goes to its rank in miss */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_miss_apply(TallyLibArgs a)
{
   __shared__ uint32_t s_cnt[SEEQ_TILE_ITEMS][SEEQ_TILE_WAVES];
   bool miss[SEEQ_TILE_ITEMS];
   uint32_t within[SEEQ_TILE_ITEMS];
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      miss[k] = i < a.n && (a.key[i] & SEEQ_TLIB_MISS) != 0u;
      within[k] = tile_wave_rank(miss[k], s_cnt[k]);
   }
   __syncthreads();
   uint32_t rank0 = a.esum[blockIdx.x];                     /* misses before this tile, then before this round */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint32_t j = tile_place(rank0, within[k], s_cnt[k]);
      if (miss[k] && j < a.nmiss) a.miss[j] = (uint32_t)tile_index(k);      /* (nmiss is the sum of these very misses: k_tally_assign_top) */
   }
}

/* THE NEAR PASS, in its two instances: EDIT false -- the substitutions of max_mismatch 1; EDIT true -- the three classes of one edit.
   Lane p of a half-wave owns what happens AT position p of its miss: the three substitutions (p < L); under EDIT the deletion of base p
   (p < L, canonical) and the insertions in front of p (p <= L <= 30, canonical: four for lane 0, three for the others) as well -- at
   most SEEQ_TLIB_EDIT_SEARCHES searches, stepped together.  Under EDIT a found neighbour adds 1 + (its class << 16) to nfound: the half's
   sum holds the entries found below, and above them the class of the one that was found alone. */
template <bool EDIT>
__device__ __forceinline__ void tally_assign_near(const TallyLibArgs &a)
{
   constexpr int NS = EDIT ? SEEQ_TLIB_EDIT_SEARCHES : 3;
   constexpr int NST = EDIT ? 6 : 4;
   __shared__ uint32_t s_st[NST][SEEQ_TILE_WAVES];
   __shared__ uint64_t s_top[SEEQ_TLIB_TOP];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   const uint32_t p = threadIdx.x & 31u;                    /* the position this lane varies */
   s_top[threadIdx.x] = tally_lib_sample(a.lkey, a.nlib, a.stride, threadIdx.x);
   __syncthreads();
   uint32_t ncor = 0, namb = 0, nunk = 0, nins = 0, ndel = 0;      /* wave-uniform */
   bool bad = false;
#pragma unroll 1
   for (int r = 0; r < SEEQ_TLIB_NEAR_ROUNDS; r++) {
      const uint64_t j = ((uint64_t)blockIdx.x * SEEQ_TLIB_NEAR_ROUNDS + r) * SEEQ_TLIB_NEAR_WG + (threadIdx.x >> 5);
      const bool act = j < a.nmiss;
      uint32_t idx = 0;
      uint64_t key = 0;
      int len = -1;
      bool here = false;                                    /* this round's index lies in the array */
      if (act) {
         idx = a.miss[j];
         here = idx < a.n;
         if (here) {
            key = a.key[idx] & ~SEEQ_TLIB_MISS;
            len = tally_key_len(key);
         } else {
            bad = true;
         }
      }
      const bool mine = len > 0 && p < (uint32_t)len;
      uint64_t nb[NS];
      uint32_t lo[NS], hi[NS];
#pragma unroll
      for (int s = 0; s < 3; s++) {
         nb[s] = mine ? tally_neighbour(key, (uint32_t)len, p, (uint32_t)s + 1u) : 0u;
         tally_lib_top_range(s_top, a.nlib, a.stride, nb[s], &lo[s], &hi[s]);
         if (!mine) lo[s] = hi[s] = 0u;
      }
      uint32_t on = mine ? 7u : 0u;                         /* the searches of this lane that are neighbours, by slot */
      if constexpr (EDIT) {
         const bool grows = len >= 0 && len <= SEEQ_TLIB_INS_LEN_MAX && p <= (uint32_t)len;
         const uint32_t prev = p && (mine || grows) ? tally_key_base(key, (uint32_t)len, p - 1u) : 4u;      /* the base in front of p; 4: none */
         if (mine && tally_key_base(key, (uint32_t)len, p) != prev) on |= 8u;
#pragma unroll
         for (uint32_t c = 0; c < 4u; c++) on |= grows && c != prev ? 16u << c : 0u;
#pragma unroll
         for (int s = 3; s < NS; s++) {
            const bool use = (on >> s) & 1u;
            nb[s] = !use ? 0u : s == 3 ? tally_del_neighbour(key, (uint32_t)len, p) : tally_ins_neighbour(key, (uint32_t)len, p, (uint32_t)s - 4u);
            tally_lib_top_range(s_top, a.nlib, a.stride, nb[s], &lo[s], &hi[s]);
            if (!use) lo[s] = hi[s] = 0u;
         }
      }
#pragma unroll 1
      for (uint32_t it = 0; it < a.probes; it++) {
#pragma unroll
         for (int s = 0; s < NS; s++) {
            tally_bound_step(a.lkey, 1u, nb[s], &lo[s], &hi[s]);      /* (mid < hi <= nlib) */
         }
      }
      uint32_t nfound = 0, idsum = 0;                       /* (one neighbour found: the sum of the ids found is its id) */
#pragma unroll
      for (int s = 0; s < 3; s++) {
         if (mine && lo[s] < a.nlib && a.lkey[lo[s]] == nb[s]) { nfound++; idsum += a.lid[lo[s]]; }
      }
      if constexpr (EDIT) {
#pragma unroll
         for (int s = 3; s < NS; s++) {
            if (((on >> s) & 1u) && lo[s] < a.nlib && a.lkey[lo[s]] == nb[s]) {
               nfound += 1u + ((uint32_t)(s == 3 ? SEEQ_TLIB_BY_DEL : SEEQ_TLIB_BY_INS) << 16);      /* (at most 256 found in a half) */
               idsum += a.lid[lo[s]];
            }
         }
      }
#pragma unroll
      for (int d = 16; d >= 1; d >>= 1) {                   /* (distances below 32 stay inside the half) */
         nfound += (uint32_t)__shfl_xor((int)nfound, d, 64);
         idsum += (uint32_t)__shfl_xor((int)idsum, d, 64);
      }
      const uint32_t by = EDIT ? nfound >> 16 : 0u;
      if constexpr (EDIT) nfound &= 0xFFFFu;
      int kind = -1;
      if (here && p == 0u) {
         kind = nfound == 1u ? SEEQ_TLIB_CORRECTED : nfound >= 2u ? SEEQ_TLIB_AMBIGUOUS : SEEQ_TLIB_UNKNOWN;
         a.key[idx] = nfound == 1u ? (uint64_t)idsum : 0u;
      }
      ncor += (uint32_t)__popcll(__ballot(kind == SEEQ_TLIB_CORRECTED));
      namb += (uint32_t)__popcll(__ballot(kind == SEEQ_TLIB_AMBIGUOUS));
      nunk += (uint32_t)__popcll(__ballot(kind == SEEQ_TLIB_UNKNOWN));
      if constexpr (EDIT) {
         nins += (uint32_t)__popcll(__ballot(kind == SEEQ_TLIB_CORRECTED && by == SEEQ_TLIB_BY_INS));
         ndel += (uint32_t)__popcll(__ballot(kind == SEEQ_TLIB_CORRECTED && by == SEEQ_TLIB_BY_DEL));
      }
   }
   const uint32_t nbad = __ballot(bad) != 0ull ? 2u : 0u;
   if (lane == 0) {
      s_st[0][wave] = ncor; s_st[1][wave] = namb; s_st[2][wave] = nunk; s_st[3][wave] = nbad;
      if constexpr (EDIT) { s_st[4][wave] = nins; s_st[5][wave] = ndel; }
   }
   __syncthreads();
   if (threadIdx.x == 0) {
      uint4 t = make_uint4(0u, 0u, 0u, 0u);
      for (int w = 0; w < SEEQ_TILE_WAVES; w++) { t.x += s_st[0][w]; t.y += s_st[1][w]; t.z += s_st[2][w]; t.w |= s_st[3][w]; }
      a.nstat[blockIdx.x] = t;
      if constexpr (EDIT) {
         uint2 e = make_uint2(0u, 0u);
         for (int w = 0; w < SEEQ_TILE_WAVES; w++) { e.x += s_st[4][w]; e.y += s_st[5][w]; }
         a.nedit[blockIdx.x] = e;
      }
   }
}

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_assign_near(TallyLibArgs a) { tally_assign_near<false>(a); }

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_assign_near_edit(TallyLibArgs a) { tally_assign_near<true>(a); }

/* One workgroup: the near workgroups' {corrected, ambiguous, unknown, bad}, and {inserted, deleted} under the edit mode -> the totals. */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_tally_near_top(TallyLibArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES], s_bad[SEEQ_TILE_WAVES];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   uint32_t ncor = 0, namb = 0, nunk = 0, nins = 0, ndel = 0, bad = 0;
   for (uint32_t b0 = 0; b0 < a.nwg; b0 += SEEQ_TILE_WG) {
      const uint32_t i = b0 + threadIdx.x;
      if (i < a.nwg) {
         const uint4 t = a.nstat[i];
         ncor += t.x; namb += t.y; nunk += t.z; bad |= t.w;
         if (a.nedit) { const uint2 e = a.nedit[i]; nins += e.x; ndel += e.y; }
      }
   }
   uint32_t tot_cor, tot_amb, tot_unk, tot_ins, tot_del;
   block_excl_scan(ncor, &tot_cor, s_wave);
   block_excl_scan(namb, &tot_amb, s_wave);
   block_excl_scan(nunk, &tot_unk, s_wave);
   block_excl_scan(nins, &tot_ins, s_wave);
   block_excl_scan(ndel, &tot_del, s_wave);
   bad = __ballot(bad != 0u) != 0ull ? 2u : 0u;
   if (lane == 0) s_bad[wave] = bad;
   __syncthreads();
   if (threadIdx.x == 0) {
      for (int w = 0; w < SEEQ_TILE_WAVES; w++) bad |= s_bad[w];
      a.cnt->ncorrected = tot_cor; a.cnt->nambiguous = tot_amb; a.cnt->nunknown = tot_unk; a.cnt->bad = bad;
      a.cnt->ninserted = tot_ins; a.cnt->ndeleted = tot_del;
   }
}

#endif   /* __HIPCC__ */
#endif
