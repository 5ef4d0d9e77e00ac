// The one-edit mode of the library rule of seeq_amd/csrc/seeq_tally_library.h (the deletion and insertion neighbours of a key, the
// assignment under a mode) compiled for the host by plain g++, for tests/test_tally_library_edit_host.py.
//
//   tally_library_edit_host_driver neigh < cases    a case is "K <key in hex>": two lines, "D" and the key's canonical deletion neighbours
//                                                   in hex, by position, then "I" and its canonical insertion neighbours, by position
//                                                   and base (none for a key of 31 bases).
//   tally_library_edit_host_driver assign < cases   a case is "L n mode" and n keys in hex in the caller's order, then "Q m" and m keys in
//                                                   hex.  Per query "id kind by": tally_lib_assign_mode's id, kind (0 exact, 1 corrected,
//                                                   2 ambiguous, 3 unknown) and the class of the neighbour found (0 substitution,
//                                                   1 insertion, 2 deletion; -1: not corrected).  Under modes 0 and 1 the driver fails
//                                                   unless tally_lib_assign with that max_mismatch gives the same id and kind.  The arrays
//                                                   are heap blocks of exactly n entries: a read beyond them is the sanitizer's to find.
//   tally_library_edit_host_driver                  the constants: the three modes, the three classes, the longest key that grows, the
//                                                   searches of a lane.
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
      const uint32_t L = (uint32_t)len;
      printf("D");
      for (uint32_t p = 0; p < L; p++)
         if (tally_del_canonical(key, L, p)) printf(" %" PRIx64, tally_del_neighbour(key, L, p));
      printf("\nI");
      for (uint32_t p = 0; p <= L && L <= SEEQ_TLIB_INS_LEN_MAX; p++)
         for (uint32_t c = 0; c <= 3; c++)
            if (tally_ins_canonical(key, L, p, c)) printf(" %" PRIx64, tally_ins_neighbour(key, L, p, c));
      printf("\n");
   }
   return 0;
}

static int do_assign()
{
   unsigned long long n, m;
   int mode;
   while (scanf(" L %llu %d", &n, &mode) == 2) {
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
      if (bad) { fprintf(stderr, "a refused library: %d at %zu\n", bad, at); return 1; }
      const uint32_t probes = tally_lib_probes((uint32_t)n);
      for (const uint64_t k : q) {
         int kind = -1, by = -2;
         const uint32_t id = tally_lib_assign_mode(skey, sid, (uint32_t)n, probes, k, mode, &kind, &by);
         if (mode != SEEQ_TLIB_MODE_EDIT) {
            int kind1 = -1;
            const uint32_t id1 = tally_lib_assign(skey, sid, (uint32_t)n, probes, k, mode, &kind1);
            if (id1 != id || kind1 != kind || by != (kind == SEEQ_TLIB_CORRECTED ? SEEQ_TLIB_BY_SUBST : -1)) {
               fprintf(stderr, "mode %d differs from max_mismatch %d for %" PRIx64 ": %u %d %d, %u %d\n", mode, mode, k, id, kind, by, id1, kind1);
               return 2;
            }
         }
         printf("%u %d %d\n", id, kind, by);
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
   printf("B %d %d %d %d %d %d %d %d\n", SEEQ_TLIB_MODE_EXACT, SEEQ_TLIB_MODE_SUBST, SEEQ_TLIB_MODE_EDIT, SEEQ_TLIB_BY_SUBST, SEEQ_TLIB_BY_INS, SEEQ_TLIB_BY_DEL,
          SEEQ_TLIB_INS_LEN_MAX, SEEQ_TLIB_EDIT_SEARCHES);
   return 0;
}
