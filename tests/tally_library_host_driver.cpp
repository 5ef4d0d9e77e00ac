// The library rule of seeq_amd/csrc/seeq_tally_library.h (neighbour, lower bound, assignment, the host-side sort and validation of a
// library) compiled for the host by plain g++, for tests/test_tally_library_host.py.
//
//   tally_library_host_driver neigh < cases    a case is "K <key in hex>": the key's 3 L neighbours in hex on one line, position by
//                                              position, s = 1, 2, 3 ("-" for the empty key).
//   tally_library_host_driver assign < cases   a case is "L n max_mismatch" and n keys in hex in the caller's order, then "Q m" and m keys
//                                              in hex.  tally_lib_prepare sorts and validates: "E <code> <index>" for a refused library
//                                              (1: no key, 2: a duplicate, 3: too many), and nothing more of the case.  Else
//                                              "P <bitlen> <probes> <passes>" and per query "id kind lower" -- tally_lib_assign's id and
//                                              kind (0 exact, 1 corrected, 2 ambiguous, 3 unknown) and tally_lib_lower_bound's result
//                                              over the sorted keys, which the kernels' two-level search (tally_lib_top_range,
//                                              tally_lib_lower_bound_top) must give too, or the driver fails.  The arrays are heap
//                                              blocks of exactly n entries: a read beyond them is the sanitizer's to find.
//   tally_library_host_driver                  the constants: largest library, misses per near workgroup, the four kinds, the error codes.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "seeq_tally_library.h"

static int do_neigh()
{
   uint64_t key;
   while (scanf(" K %" SCNx64, &key) == 1) {
      const int len = tally_key_len(key);
      if (len < 0) { fprintf(stderr, "no key: %" PRIx64 "\n", key); return 1; }
      if (!len) printf("-");
      for (int p = 0; p < len; p++)
         for (uint32_t s = 1; s <= 3; s++) printf("%s%" PRIx64, p || s > 1 ? " " : "", tally_neighbour(key, (uint32_t)len, (uint32_t)p, s));
      printf("\n");
   }
   return 0;
}

static int do_assign()
{
   unsigned long long n, m;
   int mm;
   while (scanf(" L %llu %d", &n, &mm) == 2) {
      std::vector<uint64_t> keys(n);
      for (auto &k : keys)
         if (scanf("%" SCNx64, &k) != 1) { fprintf(stderr, "short library\n"); return 1; }
      if (scanf(" Q %llu", &m) != 1) { fprintf(stderr, "no queries\n"); return 1; }
      std::vector<uint64_t> q(m);
      for (auto &k : q)
         if (scanf("%" SCNx64, &k) != 1) { fprintf(stderr, "short queries\n"); return 1; }
      uint64_t *skey = (uint64_t *)malloc(n ? n * sizeof(uint64_t) : 1);
      uint32_t *sid = (uint32_t *)malloc(n ? n * sizeof(uint32_t) : 1);
      size_t at;
      const int bad = tally_lib_prepare(keys.data(), (size_t)n, skey, sid, &at);
      if (bad) {
         printf("E %d %zu\n", bad, at);
      } else {
         for (size_t i = 0; i < n; i++)
            if (sid[i] < 1 || sid[i] > n || keys[sid[i] - 1] != skey[i] || (i && skey[i - 1] >= skey[i])) { fprintf(stderr, "the sorted library is wrong at %zu\n", i); return 2; }
         const uint32_t probes = tally_lib_probes((uint32_t)n);
         printf("P %u %u %u\n", tally_lib_bitlen(n), probes, tally_lib_passes(1, (uint32_t)n));
         // the kernels' two-level search: the samples a workgroup keeps in LDS, then the few steps left over the library
         const uint32_t stride = tally_lib_stride((uint32_t)n), probes2 = tally_lib_probes(stride);
         uint64_t *top = (uint64_t *)malloc(SEEQ_TLIB_TOP * sizeof(uint64_t));
         for (uint32_t i = 0; i < SEEQ_TLIB_TOP; i++) top[i] = tally_lib_sample(skey, (uint32_t)n, stride, i);
         for (const uint64_t k : q) {
            int kind = -1;
            const uint32_t id = tally_lib_assign(skey, sid, (uint32_t)n, probes, k, mm, &kind);
            const uint32_t lower = tally_lib_lower_bound(skey, (uint32_t)n, probes, k);
            uint32_t lo, hi;
            tally_lib_top_range(top, (uint32_t)n, stride, k, &lo, &hi);
            if (lo > lower || lower > hi || hi - lo > stride || tally_lib_lower_bound_top(top, skey, (uint32_t)n, stride, probes2, k) != lower) {
               fprintf(stderr, "the two-level search differs for %" PRIx64 ": %u, range %u .. %u, stride %u\n", k, lower, lo, hi, stride);
               return 2;
            }
            printf("%u %d %u\n", id, kind, lower);
         }
         free(top);
      }
      free(skey);
      free(sid);
   }
   return 0;
}

int main(int argc, char **argv)
{
   if (argc > 1 && !strcmp(argv[1], "neigh")) return do_neigh();
   if (argc > 1 && !strcmp(argv[1], "assign")) return do_assign();
   printf("B %u %d %d %d %d %d %d %d %d %u %u\n", SEEQ_TLIB_MAX, SEEQ_TLIB_NEAR_WG * SEEQ_TLIB_NEAR_ROUNDS, SEEQ_TLIB_EXACT, SEEQ_TLIB_CORRECTED, SEEQ_TLIB_AMBIGUOUS, SEEQ_TLIB_UNKNOWN,
          SEEQ_TLIB_E_NOKEY, SEEQ_TLIB_E_DUP, SEEQ_TLIB_E_MANY, tally_lib_passes(0, 2000), tally_lib_passes(5, 2000));
   return 0;
}
