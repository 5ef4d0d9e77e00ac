// The rule of the tally of the held column itself, seeq_amd/csrc/seeq_tally_held.h (the kinds of the held records, the shift of the member
// columns, the two head rows and both tables over a sorted array, the dense cell), compiled for the host by plain g++, for
// tests/test_tally_held_host.py.
//
//   tally_held_host_driver kinds < cases    a case is "M ncolumns m" + ncolumns widths, then "H n" + n rows "line key" (key in hex): "S rc shift"
//                                           (tally_held_shift over exactly ncolumns heap entries), then per record "kind word" (word in hex:
//                                           what the record is sorted as), then "C ncounted nkeyless nrepeat key_bits passes" -- key_bits
//                                           of the largest counted key, passes from the largest held one.
//   tally_held_host_driver tables < cases   a case is "T shift n" + n words (hex) ALREADY SORTED: the heads as the device compacts them
//                                           (kpos, rrank over exactly as many heap entries as there are heads), then "K nk" + nk rows
//                                           "key count" and "R nr" + nr rows "group count first ndistinct" (keys and groups in hex).
//   tally_held_host_driver dense < cases    a case is "key shift nrows ncols" (key in hex): "inside cell".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "seeq_tally_held.h"

template <class T> static T *heap(size_t n) { return n ? (T *)malloc(n * sizeof(T)) : NULL; }      // exactly n entries: a step beyond them is the sanitizer's to find

static int do_kinds()
{
   int ncol, m;
   while (scanf(" M %d %d", &ncol, &m) == 2) {
      const int nw = ncol > 0 ? ncol : 0;
      uint32_t *w = heap<uint32_t>(nw);
      for (int c = 0; c < nw; c++)
         if (scanf("%u", &w[c]) != 1) { fprintf(stderr, "short widths\n"); return 1; }
      unsigned n;
      if (scanf(" H %u", &n) != 1) { fprintf(stderr, "short case\n"); return 1; }
      uint32_t *line = heap<uint32_t>(n);
      uint64_t *key = heap<uint64_t>(n);
      for (unsigned i = 0; i < n; i++)
         if (scanf("%u %" SCNx64, &line[i], &key[i]) != 2) { fprintf(stderr, "short column\n"); return 1; }
      uint32_t shift = 0;
      // (a shape tally_held_shift refuses is refused before any width is read: exactly ncol entries are enough)
      const int rc = tally_held_shift(w, ncol, m, &shift);
      printf("S %d %u\n", rc, rc ? 0u : shift);
      unsigned long long cnt[3] = {0, 0, 0};
      uint32_t bits = 0, held_bits = 0;
      for (unsigned i = 0; i < n; i++) {
         const int kind = tally_held_kind(tally_held_opens(line, i), key[i]);
         const uint64_t word = tally_held_word(kind, key[i]);
         cnt[kind]++;
         if (tally_key_bits(word) > bits) bits = tally_key_bits(word);
         if (tally_key_bits(key[i]) > held_bits) held_bits = tally_key_bits(key[i]);
         printf("%d %" PRIx64 "\n", kind, word);
      }
      printf("C %llu %llu %llu %u %u\n", cnt[SEEQ_HELD_COUNTED], cnt[SEEQ_HELD_KEYLESS], cnt[SEEQ_HELD_REPEAT], bits, tally_held_passes(cnt[SEEQ_HELD_COUNTED], held_bits));
      free(w); free(line); free(key);
   }
   return 0;
}

static int do_tables()
{
   unsigned shift, n;
   while (scanf(" T %u %u", &shift, &n) == 2) {
      uint64_t *src = heap<uint64_t>(n);
      for (unsigned i = 0; i < n; i++)
         if (scanf("%" SCNx64, &src[i]) != 1) { fprintf(stderr, "short words\n"); return 1; }
      // the reduce: the heads' numbers
      uint32_t nk = 0, nr = 0;
      for (unsigned i = 0; i < n; i++) {
         const uint64_t prev = i ? src[i - 1] : 0u;
         nk += tally_is_head(src[i], prev, i == 0);
         nr += tally_held_is_row_head(src[i], prev, shift, i == 0);
      }
      // the apply: a key head's index to its rank, a row head's key rank to its own
      uint32_t *kpos = heap<uint32_t>(nk), *rrank = heap<uint32_t>(nr);
      uint32_t j = 0, r = 0;
      for (unsigned i = 0; i < n; i++) {
         const uint64_t prev = i ? src[i - 1] : 0u;
         const int khead = tally_is_head(src[i], prev, i == 0), rhead = tally_held_is_row_head(src[i], prev, shift, i == 0);
         if (rhead && !khead) { fprintf(stderr, "a row head that is no key head at %u\n", i); return 1; }
         if (rhead) rrank[r++] = j;
         if (khead) kpos[j++] = i;
      }
      // the tables: one entry per head
      printf("K %u\n", nk);
      for (uint32_t e = 0; e < nk; e++) {
         const uint32_t p = kpos[e], next = e + 1 < nk ? kpos[e + 1] : n;
         printf("%" PRIx64 " %u\n", src[p], next - p);
      }
      printf("R %u\n", nr);
      for (uint32_t e = 0; e < nr; e++) {
         const uint32_t first = rrank[e], nfirst = e + 1 < nr ? rrank[e + 1] : nk;
         const uint32_t p = kpos[first], next = nfirst < nk ? kpos[nfirst] : n;
         printf("%" PRIx64 " %u %u %u\n", tally_held_row(src[p], shift), next - p, first, nfirst - first);
      }
      free(src); free(kpos); free(rrank);
   }
   return 0;
}

static int do_dense()
{
   uint64_t key;
   unsigned shift, nrows, ncols;
   while (scanf("%" SCNx64 " %u %u %u", &key, &shift, &nrows, &ncols) == 4) {
      uint64_t cell = 0;
      const int inside = tally_held_cell(key, shift, nrows, ncols, &cell);
      printf("%d %" PRIu64 "\n", inside, inside ? cell : 0u);
   }
   return 0;
}

int main(int argc, char **argv)
{
   if (argc > 1 && !strcmp(argv[1], "kinds")) return do_kinds();
   if (argc > 1 && !strcmp(argv[1], "tables")) return do_tables();
   if (argc > 1 && !strcmp(argv[1], "dense")) return do_dense();
   printf("H %d %d %d %d %d\n", SEEQ_HELD_REPEAT, SEEQ_HELD_KEYLESS, SEEQ_HELD_COUNTED, SEEQ_TALLY_COLUMNS, SEEQ_TALLY_WORD_BITS);
   return 0;
}
