/*
 * seeq_tally_collapse.h -- collapsing UMI errors in the grouped tally: per pair of the pair table (seeq_tally_group.h), is it a molecule of
 * its own or an erroneous copy -- one substitution away -- of another pair OF ITS GROUP, and per group, how many molecules remain.  A UMI
 * is random: it has no library to be corrected against (seeq_tally_library.h), only its neighbours in the same group and their counts.
 * The step stands behind seeqdevScanTallyGrouped, reads its two tables where they lie on the device and writes arrays of its own.
 *
 * The rule -- plain C++ below, shared with the host driver (tests/tally_collapse_host_driver.cpp compiles this header with g++).  Pair i of
 * the pair table is (g_i, m_i, c_i); m_i is a tally key of length L_i (tally_key_len):
 *
 *   neighbour    tally_neighbour of seeq_tally_library.h, unchanged: another base at one position, the same length.  A member of length 0
 *                has none; neither has a member that is no tally key.
 *   precedes     pair j precedes pair i iff c_j > c_i, or c_j == c_i and m_j < m_i (collapse_precedes): within a group a strict total
 *                order, the members of a group being pairwise distinct.
 *   candidate    of i: a pair j of the same group whose member is a neighbour of m_i, that precedes i and -- under
 *                SEEQ_COLLAPSE_DIRECTIONAL -- has c_j >= 2 c_i - 1, evaluated without wrap-around as c_j - c_i >= c_i - 1 (j precedes i:
 *                c_j >= c_i >= 1; collapse_admits).  SEEQ_COLLAPSE_ANY drops the count threshold.
 *   parent       i has no candidate: it is a ROOT, parent[i] = i.  Else it is ABSORBED and parent[i] is the candidate that precedes all
 *                the others: the highest count, then the smallest member.  A parent precedes its child, so the parents form a forest; a
 *                parent may itself be absorbed (the chain 100 - 10 - 1).  THE CHAINS ARE NOT FOLLOWED here: the host does that in
 *                O(log depth) gathers (seeq_amd.device.collapse_fold).
 *   per group    nroots (its molecules), nabsorbed (its pairs that are no root), absorbed_reads (the sum of their counts);
 *                nroots + nabsorbed = the ndistinct of the group's row, and every group has a root: its first pair in the order.
 *   tied counts  of two neighbouring members with EQUAL counts -- mostly count 1 beside count 1 -- the smaller member is the root and
 *                absorbs the other (under the directional rule only where c - c >= c - 1, that is c = 1; under ANY always).  This is
 *                the directional rule with its tie-break made deterministic.  It can differ from a breadth-first network, which starts
 *                at the highest count and takes a whole component: in a chain of tied pairs a - b - c (a < b < c, neighbours a - b and
 *                b - c only) b is absorbed by a and c by b here, one family after the fold, where a network visiting in another order
 *                could split it; and a pair between two roots goes to the one that precedes, not to the one visited first.
 *
 * The kernels read the pair table (24 bytes per entry, ascending by (group, member)) and the group table (24 bytes per row: its key, its
 * reads, first | ndistinct << 32):
 *
 *   the group row          of pair i: a lower bound of g_i over the group table in two levels, as the library's search: a workgroup keeps
 *                          every stride-th group key, 256 samples, in LDS (tally_lib_top_range), the rest is at most
 *                          tally_lib_probes(stride) steps over the table.  (The alternative -- writing each pair's group rank once, by a
 *                          kernel of its own -- costs 4 bytes per pair and a launch; the search was chosen: the lanes of a half wave
 *                          share its loads.)  The row gives the segment [first, first + ndistinct) of the pair's group.
 *   k_collapse_parent      k_tally_assign_near's shape, a grid sized by the host-known pair count, 64 pairs per workgroup in eight rounds:
 *                          half a wave (32 lanes >= L) owns one pair, lane p < L searches the three neighbours at position p among
 *                          the members of the segment (stepped together; at most tally_lib_probes(npairs) steps, left early when no
 *                          lane of the wave has a range left), keeps the best candidate it found under "precedes", the half reduces to
 *                          the best of all with __shfl_xor at distances 16 .. 1, and its lane 0 stores parent[i].  Work by the pair,
 *                          not by the group: sixteen demux groups of 500 k pairs stand against 2 000 guides of 450.  Per workgroup
 *                          {roots, absorbed, absorbed reads, bad}.
 *   k_collapse_prefix_reduce / _top / _apply    the reduce / top / apply of seeq_tiles.h over the pair table: per tile the roots and
 *                          the absorbed reads (64-bit), one workgroup scans both rows (tile_top, once per row), per pair the INCLUSIVE
 *                          count of roots and sum of absorbed reads up to it: proot[i], pread[i].
 *   k_collapse_groups      one thread per group row: the differences of both prefixes between the segment's end and its start, one
 *                          16-byte {nroots, nabsorbed, absorbed_reads}; per workgroup {roots, groups without a root, bad}.
 *   k_collapse_top         one workgroup: the totals of both kinds of per-workgroup numbers, for the host's one counters copy.
 *
 * Every output slot is written by exactly one thread per launch; no atomics on global memory; no workgroup waits on another; every loop
 * is bounded by a count the host knows; the grids come from host-known counts (no pair: nothing is launched); every index is clamped
 * into its table before it is used.
 */
#ifndef SEEQ_TALLY_COLLAPSE_H_
#define SEEQ_TALLY_COLLAPSE_H_

#include <stdint.h>

#include "seeq_tally_library.h"

#define SEEQ_COLLAPSE_DIRECTIONAL 0                         /* = SEEQDEV_COLLAPSE_DIRECTIONAL / _ANY (seeq_amd.h) */
#define SEEQ_COLLAPSE_ANY         1
#define SEEQ_COLLAPSE_HALVES      8                         /* pairs per round of a workgroup of k_collapse_parent: its half-waves */
#define SEEQ_COLLAPSE_ROUNDS      8                         /* rounds of such a workgroup: 64 pairs, one {roots, absorbed, absorbed reads, bad} */
#define SEEQ_COLLAPSE_NONE        0xFFFFFFFFu               /* "no candidate" where an index of the pair table is expected */

/* does the pair (count cj, member mj) precede the pair (ci, mi) of its group? */
SEEQ_ST_HD int collapse_precedes(uint64_t cj, uint64_t mj, uint64_t ci, uint64_t mi) { return cj > ci || (cj == ci && mj < mi); }

/* the count threshold of a pair of count cj that PRECEDES one of count ci (cj >= ci): cj >= 2 ci - 1 without wrap-around */
SEEQ_ST_HD int collapse_admits(int rule, uint64_t cj, uint64_t ci) { return rule == SEEQ_COLLAPSE_ANY || (ci != 0u && cj - ci >= ci - 1u); }

/* the three words of a pair-table entry; first and ndistinct of a group-table row */
SEEQ_ST_HD uint64_t collapse_group(const uint64_t *ptab, uint64_t i) { return ptab[3u * i]; }
SEEQ_ST_HD uint64_t collapse_member(const uint64_t *ptab, uint64_t i) { return ptab[3u * i + 1u]; }
SEEQ_ST_HD uint64_t collapse_count(const uint64_t *ptab, uint64_t i) { return ptab[3u * i + 2u]; }

/* The segment [*first, *end) of group row r, CLAMPED into a pair table of np entries; 0: the row is inconsistent with np (the segment is
   then what of it lies inside the table). */
SEEQ_ST_HD int collapse_segment(const uint64_t *gtab, uint64_t r, uint32_t np, uint32_t *first, uint32_t *end)
{
   const uint64_t w = gtab[3u * r + 2u];
   uint32_t f = (uint32_t)w, nd = (uint32_t)(w >> 32);
   int ok = nd != 0u;
   if (f > np) { f = np; ok = 0; }
   if (nd > np - f) { nd = np - f; ok = 0; }
   *first = f;
   *end = f + nd;
   return ok;
}

/* pairs with a member below `key` among the pairs before `end`, searched from `first` on (a group's segment, ascending by member), and group
   rows with a key below g among gtab's ng rows: tally_lower_bound over a column of a table, every third word; at most `probes` steps */
SEEQ_ST_HD uint32_t collapse_lower_bound(const uint64_t *ptab, uint32_t first, uint32_t end, uint32_t probes, uint64_t key)
{
   return tally_lower_bound(ptab + 1, 3u, first, end, probes, key);
}

SEEQ_ST_HD uint32_t collapse_group_lower_bound(const uint64_t *gtab, uint32_t ng, uint32_t probes, uint64_t g) { return tally_lower_bound(gtab, 3u, 0u, ng, probes, g); }

/* THE TOP OF THE GROUP SEARCH, kept in LDS by k_collapse_parent: every stride-th group key (stride = tally_lib_stride(ng)), SEEQ_TLIB_TOP
   samples with the largest 64-bit value behind the last one: tally_lib_top_range over them gives the range of at most stride rows that
   holds the lower bound. */
SEEQ_ST_HD uint64_t collapse_group_sample(const uint64_t *gtab, uint32_t ng, uint32_t stride, uint32_t i)
{
   const uint64_t at = (uint64_t)i * stride;
   return at < ng ? gtab[3u * at] : ~0ull;
}

/* the group row by both levels: the samples, then at most `probes` = tally_lib_probes(stride) steps over the range they leave */
SEEQ_ST_HD uint32_t collapse_group_lower_bound_top(const uint64_t *top, const uint64_t *gtab, uint32_t ng, uint32_t stride, uint32_t probes, uint64_t g)
{
   uint32_t lo, hi;
   tally_lib_top_range(top, ng, stride, g, &lo, &hi);
   return tally_lower_bound(gtab, 3u, lo, hi, probes, g);
}

/* THE RULE: the parent of pair i < np (i itself: a root).  *bad is set when the tables contradict each other: the pair's group has no row,
   or its row's segment does not hold the pair (it is then a root). */
SEEQ_ST_HD uint32_t collapse_parent(const uint64_t *ptab, uint32_t np, const uint64_t *gtab, uint32_t ng, uint32_t i, int rule, int *bad)
{
   const uint64_t g = collapse_group(ptab, i), m = collapse_member(ptab, i), c = collapse_count(ptab, i);
   const uint32_t r = collapse_group_lower_bound(gtab, ng, tally_lib_probes(ng), g);
   uint32_t first, end;
   if (r >= ng || gtab[3u * (uint64_t)r] != g || !collapse_segment(gtab, r, np, &first, &end) || i < first || i >= end) { *bad = 1; return i; }
   const int len = tally_key_len(m);
   const uint32_t probes = tally_lib_probes(np);
   uint64_t bc = 0u, bm = 0u;
   uint32_t bj = SEEQ_COLLAPSE_NONE;
   for (int p = 0; p < len; p++)
      for (uint32_t s = 1; s <= 3u; s++) {
         const uint64_t nb = tally_neighbour(m, (uint32_t)len, (uint32_t)p, s);
         const uint32_t j = collapse_lower_bound(ptab, first, end, probes, nb);
         if (j >= end || collapse_member(ptab, j) != nb) continue;
         const uint64_t cj = collapse_count(ptab, j);
         if (!collapse_precedes(cj, nb, c, m) || !collapse_admits(rule, cj, c)) continue;
         if (bj == SEEQ_COLLAPSE_NONE || collapse_precedes(cj, nb, bc, bm)) { bc = cj; bm = nb; bj = j; }
      }
   return bj == SEEQ_COLLAPSE_NONE ? i : bj;
}

/* workgroups of k_collapse_parent for np pairs */
SEEQ_ST_HD uint64_t collapse_workgroups(uint64_t np) { return (np + SEEQ_COLLAPSE_HALVES * SEEQ_COLLAPSE_ROUNDS - 1u) / (SEEQ_COLLAPSE_HALVES * SEEQ_COLLAPSE_ROUNDS); }

#if defined(__HIPCC__)

static_assert(SEEQ_COLLAPSE_HALVES * 32 == SEEQ_TILE_WG && SEEQ_TLIB_TOP == SEEQ_TILE_WG, "half a wave per pair; a thread per sample of the top");

struct CollapseCnt {
   uint64_t reads;                    /* k_collapse_top: the absorbed pairs' counts */
   uint64_t sreads;                   /* k_collapse_prefix_top: the same, from the tiles */
   uint32_t nroots, nabsorbed;        /* k_collapse_top: from the workgroups of k_collapse_parent */
   uint32_t sroots;                   /* k_collapse_prefix_top: the roots, from the tiles */
   uint32_t groots;                   /* k_collapse_top: the group rows' nroots, summed */
   uint32_t noroot;                   /* groups without a root (an internal error) */
   uint32_t bad;                      /* 2: an index outside its table, tables that contradict each other (an internal error) */
};

struct CollapseWg {                   /* what a workgroup of k_collapse_parent found */
   uint64_t reads;
   uint32_t roots, absorbed;
   uint32_t bad, pad;
};

struct CollapseArgs {
   const uint64_t *ptab;              /* [np] the pair table: {group, member, count} */
   const uint64_t *gtab;              /* [ng] the group table: {group, reads, first | ndistinct << 32} */
   uint32_t        np, ng;
   uint32_t        rule;
   uint32_t        gstride, gprobes;  /* group rows per sample of the top; steps over the table behind it: tally_lib_probes(gstride) */
   uint32_t        probes;            /* steps of a search inside a segment: tally_lib_probes(np) */
   uint32_t        nwg;               /* workgroups of k_collapse_parent */
   uint32_t        nt;                /* tiles of the prefix over the pairs */
   uint32_t        ngwg;              /* workgroups of k_collapse_groups */
   uint32_t       *parent;            /* [np] */
   uint32_t       *proot;             /* [np] roots among pairs 0 .. i */
   uint64_t       *pread;             /* [np] absorbed reads among pairs 0 .. i */
   uint32_t       *rsum;              /* [nt] per tile roots (k_collapse_prefix_top: exclusive prefix) */
   uint64_t       *qsum;              /* [nt] per tile absorbed reads (the same) */
   CollapseWg     *wst;               /* [nwg] */
   uint4          *gst;               /* [ngwg] {roots, groups without a root, bad, 0} */
   uint4          *groups;            /* [ng] seeqdev_tally_collapse_t: {nroots, nabsorbed, absorbed_reads (two words)} */
   CollapseCnt    *cnt;
};

__device__ __forceinline__ uint64_t collapse_shfl_xor_u64(uint64_t v, int d)
{
   const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
   return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_collapse_parent(CollapseArgs a)
{
   __shared__ uint64_t s_top[SEEQ_TLIB_TOP];
   __shared__ uint64_t s_reads[SEEQ_TILE_WAVES];
   __shared__ uint32_t s_st[3][SEEQ_TILE_WAVES];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   const uint32_t p = threadIdx.x & 31u;                    /* the position this lane varies */
   s_top[threadIdx.x] = collapse_group_sample(a.gtab, a.ng, a.gstride, threadIdx.x);
   __syncthreads();
   uint32_t nroot = 0, nabs = 0;                            /* wave-uniform */
   uint64_t reads = 0;                                      /* this lane's */
   bool bad = false;
#pragma unroll 1
   for (int r = 0; r < SEEQ_COLLAPSE_ROUNDS; r++) {
      const uint64_t i = ((uint64_t)blockIdx.x * SEEQ_COLLAPSE_ROUNDS + r) * SEEQ_COLLAPSE_HALVES + (threadIdx.x >> 5);
      const bool act = i < a.np;
      uint64_t m = 0, c = 0;
      uint32_t first = 0, end = 0;
      int len = -1;
      if (act) {
         const uint64_t g = collapse_group(a.ptab, i);
         m = collapse_member(a.ptab, i);
         c = collapse_count(a.ptab, i);
         uint32_t lo, hi;                                   /* the pair's group row: the same search in every lane of the half */
         tally_lib_top_range(s_top, a.ng, a.gstride, g, &lo, &hi);
         lo = tally_lower_bound(a.gtab, 3u, lo, hi, a.gprobes, g);      /* (hi <= ng) */
         if (lo < a.ng && a.gtab[3u * (uint64_t)lo] == g && collapse_segment(a.gtab, lo, a.np, &first, &end) && i >= first && i < end) {
            len = tally_key_len(m);
         } else {
            bad = true;                                     /* (the pair searches nothing and is a root) */
            first = end = 0u;
         }
      }
      const bool mine = len > 0 && p < (uint32_t)len;
      uint64_t nb[3];
      uint32_t lo[3], hi[3];
#pragma unroll
      for (int s = 0; s < 3; s++) {
         nb[s] = mine ? tally_neighbour(m, (uint32_t)len, p, (uint32_t)s + 1u) : 0u;
         lo[s] = mine ? first : 0u;
         hi[s] = mine ? end : 0u;
      }
#pragma unroll 1
      for (uint32_t it = 0; it < a.probes; it++) {
         bool more = false;
#pragma unroll
         for (int s = 0; s < 3; s++) {
            tally_bound_step(a.ptab + 1, 3u, nb[s], &lo[s], &hi[s]);      /* (the members' column; mid < hi <= end <= np) */
            more |= lo[s] < hi[s];
         }
         if (__ballot(more) == 0ull) break;                 /* (no lane of the wave has a range left) */
      }
      uint64_t bc = 0u, bm = 0u;                            /* the best candidate of this lane, then of the half */
      uint32_t bj = SEEQ_COLLAPSE_NONE;
#pragma unroll
      for (int s = 0; s < 3; s++) {
         if (mine && lo[s] < end && collapse_member(a.ptab, lo[s]) == nb[s]) {
            const uint64_t cj = collapse_count(a.ptab, lo[s]);
            if (collapse_precedes(cj, nb[s], c, m) && collapse_admits((int)a.rule, cj, c) &&
                (bj == SEEQ_COLLAPSE_NONE || collapse_precedes(cj, nb[s], bc, bm))) { bc = cj; bm = nb[s]; bj = lo[s]; }
         }
      }
#pragma unroll
      for (int d = 16; d >= 1; d >>= 1) {                   /* (distances below 32 stay inside the half) */
         const uint64_t oc = collapse_shfl_xor_u64(bc, d), om = collapse_shfl_xor_u64(bm, d);
         const uint32_t oj = (uint32_t)__shfl_xor((int)bj, d, 64);
         if (oj != SEEQ_COLLAPSE_NONE && (bj == SEEQ_COLLAPSE_NONE || collapse_precedes(oc, om, bc, bm))) { bc = oc; bm = om; bj = oj; }
      }
      int kind = -1;                                        /* 0: a root; 1: absorbed */
      if (act && p == 0u) {
         kind = bj != SEEQ_COLLAPSE_NONE ? 1 : 0;
         a.parent[i] = kind ? bj : (uint32_t)i;
         if (kind) reads += c;
      }
      nroot += (uint32_t)__popcll(__ballot(kind == 0));
      nabs += (uint32_t)__popcll(__ballot(kind == 1));
   }
#pragma unroll
   for (int d = 32; d >= 1; d >>= 1) reads += collapse_shfl_xor_u64(reads, d);
   const uint32_t nbad = __ballot(bad) != 0ull ? 2u : 0u;
   if (lane == 0) { s_st[0][wave] = nroot; s_st[1][wave] = nabs; s_st[2][wave] = nbad; s_reads[wave] = reads; }
   __syncthreads();
   if (threadIdx.x == 0) {
      CollapseWg t = {0u, 0u, 0u, 0u, 0u};
      for (int w = 0; w < SEEQ_TILE_WAVES; w++) { t.roots += s_st[0][w]; t.absorbed += s_st[1][w]; t.bad |= s_st[2][w]; t.reads += s_reads[w]; }
      a.wst[blockIdx.x] = t;
   }
}

/* is pair i < np a root, and what it adds to the absorbed reads (its count if it is none) */
__device__ __forceinline__ bool collapse_is_root(const CollapseArgs &a, uint64_t i, uint64_t *reads)
{
   const bool root = a.parent[i] == (uint32_t)i;
   *reads = root ? 0u : collapse_count(a.ptab, i);
   return root;
}

__global__ __launch_bounds__(SEEQ_TILE_WG) void k_collapse_prefix_reduce(CollapseArgs a)
{
   __shared__ uint32_t s_r[SEEQ_TILE_WAVES];
   __shared__ uint64_t s_q[SEEQ_TILE_WAVES];
   uint32_t roots = 0;                                      /* wave-uniform */
   uint64_t reads = 0;                                      /* this lane's */
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      bool root = false;
      uint64_t v = 0;
      if (i < a.np) root = collapse_is_root(a, i, &v);
      roots += (uint32_t)__popcll(__ballot(root));
      reads += v;
   }
   reads = wave_incl_scan_u64(reads);                       /* the publishing lane, the last one: the wave's sum */
   if (tile_publishes()) { s_r[threadIdx.x >> 6] = roots; s_q[threadIdx.x >> 6] = reads; }
   __syncthreads();
   if (threadIdx.x == 0) {
      uint32_t tr = 0;
      uint64_t tq = 0;
      for (int w = 0; w < SEEQ_TILE_WAVES; w++) { tr += s_r[w]; tq += s_q[w]; }
      a.rsum[blockIdx.x] = tr;
      a.qsum[blockIdx.x] = tq;
   }
}

/* One workgroup: both rows of tile sums -> their exclusive prefixes, in place; their totals. */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_collapse_prefix_top(CollapseArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES];
   __shared__ uint64_t s_wave64[SEEQ_TILE_WAVES];
   uint32_t tr[1];
   uint64_t tq[1];
   tile_top(a.rsum, a.nt, s_wave, tr);
   tile_top(a.qsum, a.nt, s_wave64, tq);
   if (threadIdx.x == 0) { a.cnt->sroots = tr[0]; a.cnt->sreads = tq[0]; }
}

/* per pair: the roots and the absorbed reads among the pairs up to it, itself included */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_collapse_prefix_apply(CollapseArgs a)
{
   __shared__ uint32_t s_rc[SEEQ_TILE_ITEMS][SEEQ_TILE_WAVES];
   __shared__ uint64_t s_qc[SEEQ_TILE_ITEMS][SEEQ_TILE_WAVES];
   bool root[SEEQ_TILE_ITEMS];
   uint64_t v[SEEQ_TILE_ITEMS], qwithin[SEEQ_TILE_ITEMS];
   uint32_t rwithin[SEEQ_TILE_ITEMS];
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      root[k] = false;
      v[k] = 0u;
      if (i < a.np) root[k] = collapse_is_root(a, i, &v[k]);
      rwithin[k] = tile_wave_rank(root[k], s_rc[k]);
      qwithin[k] = tile_wave_offset(v[k], s_qc[k]);
   }
   __syncthreads();
   uint32_t rbase = a.rsum[blockIdx.x];                     /* what lies before this tile, then before this round */
   uint64_t qbase = a.qsum[blockIdx.x];
#pragma unroll
   for (int k = 0; k < SEEQ_TILE_ITEMS; k++) {
      const uint64_t i = tile_index(k);
      const uint32_t rr = tile_place(rbase, rwithin[k], s_rc[k]);
      const uint64_t qq = tile_place(qbase, qwithin[k], s_qc[k]);
      if (i < a.np) { a.proot[i] = rr + (root[k] ? 1u : 0u); a.pread[i] = qq + v[k]; }
   }
}

/* One thread per group row: both prefixes at the segment's end minus at its start. */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_collapse_groups(CollapseArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES];
   const uint64_t r = (uint64_t)blockIdx.x * SEEQ_TILE_WG + threadIdx.x;
   uint32_t nroots = 0, noroot = 0, bad = 0;
   if (r < a.ng) {
      uint32_t first, end;
      if (!collapse_segment(a.gtab, r, a.np, &first, &end)) bad = 1u;      /* (clamped: the loads below lie inside the prefixes) */
      const uint32_t r1 = end ? a.proot[end - 1u] : 0u, r0 = first ? a.proot[first - 1u] : 0u;
      const uint64_t q1 = end ? a.pread[end - 1u] : 0u, q0 = first ? a.pread[first - 1u] : 0u;
      nroots = r1 - r0;
      if (r1 < r0 || nroots > end - first || q1 < q0) { bad = 1u; nroots = 0u; }
      const uint64_t q = bad ? 0u : q1 - q0;
      if (!nroots) noroot = 1u;
      a.groups[r] = make_uint4(nroots, end - first - nroots, (uint32_t)q, (uint32_t)(q >> 32));
   }
   uint32_t tot_roots, tot_noroot, tot_bad;
   block_excl_scan(nroots, &tot_roots, s_wave);
   block_excl_scan(noroot, &tot_noroot, s_wave);
   block_excl_scan(bad, &tot_bad, s_wave);
   if (threadIdx.x == 0) a.gst[blockIdx.x] = make_uint4(tot_roots, tot_noroot, tot_bad ? 2u : 0u, 0u);
}

/* One workgroup: the workgroups' numbers of k_collapse_parent and of k_collapse_groups -> the totals. */
__global__ __launch_bounds__(SEEQ_TILE_WG) void k_collapse_top(CollapseArgs a)
{
   __shared__ uint32_t s_wave[SEEQ_TILE_WAVES];
   __shared__ uint64_t s_wave64[SEEQ_TILE_WAVES];
   uint32_t roots = 0, absorbed = 0, groots = 0, noroot = 0, bad = 0;
   uint64_t reads = 0;
   for (uint32_t b0 = 0; b0 < a.nwg; b0 += SEEQ_TILE_WG) {
      const uint32_t i = b0 + threadIdx.x;
      if (i < a.nwg) {
         const CollapseWg t = a.wst[i];
         roots += t.roots; absorbed += t.absorbed; reads += t.reads; bad |= t.bad;
      }
   }
   for (uint32_t b0 = 0; b0 < a.ngwg; b0 += SEEQ_TILE_WG) {
      const uint32_t i = b0 + threadIdx.x;
      if (i < a.ngwg) {
         const uint4 t = a.gst[i];
         groots += t.x; noroot += t.y; bad |= t.z;
      }
   }
   uint32_t tot_roots, tot_abs, tot_groots, tot_noroot, tot_bad;
   uint64_t tot_reads;
   block_excl_scan(roots, &tot_roots, s_wave);
   block_excl_scan(absorbed, &tot_abs, s_wave);
   block_excl_scan(groots, &tot_groots, s_wave);
   block_excl_scan(noroot, &tot_noroot, s_wave);
   block_excl_scan(bad ? 1u : 0u, &tot_bad, s_wave);
   block_excl_scan(reads, &tot_reads, s_wave64);
   if (threadIdx.x == 0) {
      a.cnt->nroots = tot_roots; a.cnt->nabsorbed = tot_abs; a.cnt->reads = tot_reads;
      a.cnt->groots = tot_groots; a.cnt->noroot = tot_noroot; a.cnt->bad = tot_bad ? 2u : 0u;
   }
}

#endif   /* __HIPCC__ */
#endif
