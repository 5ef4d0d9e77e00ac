// The both-strands rule of seeq_amd/csrc/seeq_strand.h (reverse complement of key bytes, co-rank, winner of a line) compiled for the
// host by plain g++, for tests/test_strand_host.py.
//
//   strand_host_driver keys EXPR RCEXPR ...   per pair:  K <keys of EXPR> <their reverse complement> <keys of RCEXPR> <the complement twice>
//                                             (hex, "-" for no position)
//   strand_host_driver merge < cases          a case is "C mode na nb" followed by na plus and nb minus records "line start end dist", both
//                                             lists in key order; per case:  M <n>, then the n merged records in output order
//                                             "line start end dist strand" (line 0: the record lost its line).  Every output slot must be
//                                             written exactly once: anything else is an error (exit status 2).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "seeq_pattern.h"
#include "seeq_strand.h"

static std::string hex(const std::vector<char> &k)
{
   if (k.empty()) return "-";
   std::string s;
   char b[4];
   for (char c : k) { snprintf(b, sizeof b, "%02x", (unsigned)(unsigned char)c); s += b; }
   return s;
}

static int compile(const char *expr, std::vector<char> &keys)
{
   int err = 0;
   keys.assign(strlen(expr) + 1, 0);
   const int n = seeq_compile_pattern(expr, keys.data(), &err);
   if (n < 0) { fprintf(stderr, "pattern %s: error %d\n", expr, err); return -1; }
   keys.resize((size_t)n);
   return n;
}

static int do_keys(int argc, char **argv)
{
   for (int i = 2; i + 1 < argc; i += 2) {
      std::vector<char> k, r;
      if (compile(argv[i], k) < 0 || compile(argv[i + 1], r) < 0) return 1;
      std::vector<char> rc(k.size()), twice(k.size());
      strand_rc_keys(k.data(), (int)k.size(), rc.data());
      strand_rc_keys(rc.data(), (int)rc.size(), twice.data());
      printf("K %s %s %s %s\n", hex(k).c_str(), hex(rc).c_str(), hex(r).c_str(), hex(twice).c_str());
   }
   return 0;
}

static int do_merge()
{
   int mode;
   unsigned na, nb;
   while (scanf(" C %d %u %u", &mode, &na, &nb) == 3) {
      std::vector<strand_rec_t> a(na), b(nb);
      for (unsigned i = 0; i < na + nb; i++) {
         strand_rec_t &r = i < na ? a[i] : b[i - na];
         if (scanf("%u %u %u %u", &r.x, &r.y, &r.z, &r.w) != 4) { fprintf(stderr, "short case\n"); return 1; }
      }
      const unsigned n = na + nb;
      std::vector<strand_rec_t> out(n);
      std::vector<int> written(n, 0);
      // what one thread of k_strand_merge does, for every input record of either list
      for (unsigned t = 0; t < n; t++) {
         uint32_t line, j;
         strand_rec_t r;
         if (t < na) {
            r = a[t];
            j = strand_place_plus(mode, a.data(), t, b.data(), nb, &line);
         } else {
            r = b[t - na];
            j = strand_place_minus(mode, b.data(), t - na, a.data(), na, &line);
            r.w |= SEEQ_STRAND_MINUS;
         }
         if (j >= n || written[j]++) { fprintf(stderr, "record %u goes to slot %u of %u (written %d times)\n", t, j, n, j < n ? written[j] : 0); return 2; }
         r.x = line;
         out[j] = r;
      }
      printf("M %u\n", n);
      for (const strand_rec_t &r : out) printf("%u %u %u %u %u\n", r.x, r.y, r.z, r.w & ~SEEQ_STRAND_MINUS, (r.w & SEEQ_STRAND_MINUS) ? 1u : 0u);
   }
   return 0;
}

int main(int argc, char **argv)
{
   if (argc > 1 && !strcmp(argv[1], "keys")) return do_keys(argc, argv);
   if (argc > 1 && !strcmp(argv[1], "merge")) return do_merge();
   printf("T %d %d %d %u\n", SEEQ_STRAND_TILE, SEEQ_STRAND_WG, SEEQ_STRAND_ITEMS, SEEQ_STRAND_MINUS);
   return 0;
}
