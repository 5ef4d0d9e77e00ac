// The rule of the appended key columns of seeq_amd/csrc/seeq_tally_append.h (the join of a new column into the held one, the composed key,
// the width check, the split) compiled for the host by plain g++, for tests/test_tally_append_host.py.
//
//   tally_append_host_driver join < cases     a case is "W key_bits w", then "H nh" + nh rows "line key" (key in hex), then "N nc" + nc rows
//                                             "line key": the join over exactly nh and nc heap entries (0: none are allocated), in place.
//                                             Output: "F fits", and when it fits per held record its new key (hex), then
//                                             "C nbefore nheld ndropped key_bits".
//   tally_append_host_driver compose < cases  a case is "ncolumns" + ncolumns pairs "width key" (key in hex, nonzero, at most width bits):
//                                             the word composed column by column with tally_append_key (hex), and its bit length.
//   tally_append_host_driver split < cases    a case is "key ncolumns" + ncolumns widths: "rc" and, for rc 0, the columns' keys (hex), by
//                                             tally_split over exactly ncolumns heap entries.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "seeq_tally_append.h"

struct Column {
   uint32_t *line;
   uint64_t *key;
   uint32_t  n;
};

// exactly n entries on the heap: a probe beyond them is the sanitizer's to find
static bool read_column(const char *tag, Column *c)
{
   char fmt[16];
   unsigned n;
   snprintf(fmt, sizeof fmt, " %s %%u", tag);
   if (scanf(fmt, &n) != 1) return false;
   c->n = n;
   c->line = n ? (uint32_t *)malloc(n * sizeof(uint32_t)) : NULL;
   c->key = n ? (uint64_t *)malloc(n * sizeof(uint64_t)) : NULL;
   for (unsigned i = 0; i < n; i++)
      if (scanf("%u %" SCNx64, &c->line[i], &c->key[i]) != 2) { fprintf(stderr, "short column\n"); exit(1); }
   return true;
}

static void free_column(Column *c) { free(c->line); free(c->key); }

static int do_join()
{
   unsigned key_bits, w;
   while (scanf(" W %u %u", &key_bits, &w) == 2) {
      Column h, n;
      if (!read_column("H", &h) || !read_column("N", &n)) { fprintf(stderr, "short case\n"); return 1; }
      const int fits = tally_append_fits(key_bits, w);
      printf("F %d\n", fits);
      if (fits) {
         unsigned long long nbefore = 0, nheld = 0;
         uint32_t bits = 0;
         for (uint32_t i = 0; i < h.n; i++) {
            nbefore += h.key[i] != 0;
            h.key[i] = tally_append_of(n.line, n.key, n.n, w, h.line[i], h.key[i]);
            nheld += h.key[i] != 0;
            const uint32_t b = tally_key_bits(h.key[i]);
            if (b > bits) bits = b;
            printf("%" PRIx64 "\n", h.key[i]);
         }
         printf("C %llu %llu %llu %u\n", nbefore, nheld, nbefore - nheld, bits);
      }
      free_column(&h);
      free_column(&n);
   }
   return 0;
}

static int do_compose()
{
   int ncol;
   while (scanf("%d", &ncol) == 1) {
      uint64_t word = 0;
      for (int c = 0; c < ncol; c++) {
         unsigned w;
         uint64_t k;
         if (scanf("%u %" SCNx64, &w, &k) != 2) { fprintf(stderr, "short case\n"); return 1; }
         word = c ? tally_append_key(word, k, w) : k;
      }
      printf("%" PRIx64 " %u\n", word, tally_key_bits(word));
   }
   return 0;
}

static int do_split()
{
   uint64_t key;
   int ncol;
   while (scanf("%" SCNx64 " %d", &key, &ncol) == 2) {
      const int n = ncol > 0 ? ncol : 0;
      uint32_t *w = n ? (uint32_t *)malloc(n * sizeof(uint32_t)) : NULL;
      uint64_t *out = n ? (uint64_t *)malloc(n * sizeof(uint64_t)) : NULL;
      for (int c = 0; c < n; c++)
         if (scanf("%u", &w[c]) != 1) { fprintf(stderr, "short widths\n"); return 1; }
      // (more than SEEQ_TALLY_COLUMNS widths are refused before any of them is read: exactly ncol entries are enough)
      const int rc = tally_split(key, w, ncol, out);
      printf("%d", rc);
      for (int c = 0; rc == 0 && c < n; c++) printf(" %" PRIx64, out[c]);
      printf("\n");
      free(w);
      free(out);
   }
   return 0;
}

int main(int argc, char **argv)
{
   if (argc > 1 && !strcmp(argv[1], "join")) return do_join();
   if (argc > 1 && !strcmp(argv[1], "compose")) return do_compose();
   if (argc > 1 && !strcmp(argv[1], "split")) return do_split();
   printf("A %d %d %d\n", SEEQ_TALLY_COLUMNS, SEEQ_TALLY_WORD_BITS, SEEQ_TALLY_PROBES);
   return 0;
}
