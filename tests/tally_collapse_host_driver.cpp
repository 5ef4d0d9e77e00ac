// The collapse rule of seeq_amd/csrc/seeq_tally_collapse.h (precedes, the count threshold, the segment search, the parent of a pair, the
// group rows) compiled for the host by plain g++, for tests/test_tally_collapse_host.py.
//
//   tally_collapse_host_driver collapse < cases   a case is "T np ng rule", np lines "group member count" (hex, hex, decimal) -- a pair table,
//                                                 ascending by (group, member) -- and ng lines "group reads first ndistinct" (hex, then
//                                                 decimal) -- its group table.  Out: "R nroots nabsorbed absorbed_reads bad", the np parents
//                                                 on one line ("-" for none), and per group row "nroots nabsorbed absorbed_reads", taken
//                                                 as k_collapse_groups takes them: differences of the inclusive prefixes over the pairs.
//                                                 The group row of every pair is searched by both levels (the samples a workgroup keeps
//                                                 in LDS, then the table) and must be the one-level search's, or the driver fails.  The
//                                                 tables are heap blocks of exactly 3 np and 3 ng words: a read beyond them is the
//                                                 sanitizer's to find.
//   tally_collapse_host_driver order < cases      a case is "cj mj ci mi" (decimal, hex, decimal, hex): "precedes admits(directional)
//                                                 admits(any)".
//   tally_collapse_host_driver                    the constants: the two rules, pairs per workgroup of k_collapse_parent, "no candidate".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "seeq_tally_collapse.h"

static int do_collapse()
{
   unsigned long long np, ng;
   int rule;
   while (scanf(" T %llu %llu %d", &np, &ng, &rule) == 3) {
      uint64_t *ptab = (uint64_t *)malloc(np ? 3 * np * sizeof(uint64_t) : 1);
      uint64_t *gtab = (uint64_t *)malloc(ng ? 3 * ng * sizeof(uint64_t) : 1);
      for (unsigned long long i = 0; i < np; i++)
         if (scanf("%" SCNx64 " %" SCNx64 " %" SCNu64, &ptab[3 * i], &ptab[3 * i + 1], &ptab[3 * i + 2]) != 3) { fprintf(stderr, "short pair table\n"); return 1; }
      for (unsigned long long r = 0; r < ng; r++) {
         uint64_t first, nd;
         if (scanf("%" SCNx64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &gtab[3 * r], &gtab[3 * r + 1], &first, &nd) != 4) { fprintf(stderr, "short group table\n"); return 1; }
         gtab[3 * r + 2] = first | (nd << 32);
      }
      const uint32_t stride = tally_lib_stride((uint32_t)ng), probes2 = tally_lib_probes(stride);
      uint64_t *top = (uint64_t *)malloc(SEEQ_TLIB_TOP * sizeof(uint64_t));
      for (uint32_t i = 0; i < SEEQ_TLIB_TOP; i++) top[i] = collapse_group_sample(gtab, (uint32_t)ng, stride, i);
      std::vector<uint32_t> parent(np), proot(np);
      std::vector<uint64_t> pread(np);
      uint64_t nroots = 0, nabs = 0, reads = 0;
      int bad = 0;
      for (uint32_t i = 0; i < np; i++) {
         const uint64_t g = collapse_group(ptab, i);
         const uint32_t one = collapse_group_lower_bound(gtab, (uint32_t)ng, tally_lib_probes((uint32_t)ng), g);
         if (collapse_group_lower_bound_top(top, gtab, (uint32_t)ng, stride, probes2, g) != one) {
            fprintf(stderr, "the two-level group search differs for %" PRIx64 ": %u, stride %u\n", g, one, stride);
            return 2;
         }
         parent[i] = collapse_parent(ptab, (uint32_t)np, gtab, (uint32_t)ng, i, rule, &bad);
         if (parent[i] >= np) { fprintf(stderr, "a parent outside the table at %u\n", i); return 2; }
         const bool root = parent[i] == i;
         if (!root && !collapse_precedes(collapse_count(ptab, parent[i]), collapse_member(ptab, parent[i]), collapse_count(ptab, i), collapse_member(ptab, i))) {
            fprintf(stderr, "a parent that does not precede its child at %u\n", i);
            return 2;
         }
         nroots += root; nabs += !root; reads += root ? 0u : collapse_count(ptab, i);      // (wraps as the device's sum would)
         proot[i] = (uint32_t)nroots; pread[i] = reads;
      }
      printf("R %" PRIu64 " %" PRIu64 " %" PRIu64 " %d\n", nroots, nabs, reads, bad);
      if (!np) printf("-");
      for (uint32_t i = 0; i < np; i++) printf("%s%u", i ? " " : "", parent[i]);
      printf("\n");
      for (uint32_t r = 0; r < ng; r++) {
         uint32_t first, end;
         if (!collapse_segment(gtab, r, (uint32_t)np, &first, &end)) { fprintf(stderr, "group row %u lies outside the pair table\n", r); return 2; }
         const uint32_t gr = (end ? proot[end - 1] : 0u) - (first ? proot[first - 1] : 0u);
         const uint64_t gq = (end ? pread[end - 1] : 0u) - (first ? pread[first - 1] : 0u);
         printf("%u %u %" PRIu64 "\n", gr, end - first - gr, gq);
      }
      free(top);
      free(gtab);
      free(ptab);
   }
   return 0;
}

static int do_order()
{
   uint64_t cj, mj, ci, mi;
   while (scanf("%" SCNu64 " %" SCNx64 " %" SCNu64 " %" SCNx64, &cj, &mj, &ci, &mi) == 4)
      printf("%d %d %d\n", collapse_precedes(cj, mj, ci, mi), collapse_admits(SEEQ_COLLAPSE_DIRECTIONAL, cj, ci), collapse_admits(SEEQ_COLLAPSE_ANY, cj, ci));
   return 0;
}

int main(int argc, char **argv)
{
   if (argc > 1 && !strcmp(argv[1], "collapse")) return do_collapse();
   if (argc > 1 && !strcmp(argv[1], "order")) return do_order();
   printf("C %d %d %d %u %" PRIu64 " %" PRIu64 "\n", SEEQ_COLLAPSE_DIRECTIONAL, SEEQ_COLLAPSE_ANY, SEEQ_COLLAPSE_HALVES * SEEQ_COLLAPSE_ROUNDS, SEEQ_COLLAPSE_NONE,
          collapse_workgroups(64), collapse_workgroups(65));
   return 0;
}
