// The tally rule of seeq_amd/csrc/seeq_tally.h (span -> key, key -> bases, digit of a pass, pass count, run heads) compiled for the host by
// plain g++, for tests/test_tally_host.py.
//
//   tally_host_driver span < cases    a case is "S <text as hex, - for none> nbytes off start end": what one thread of k_tally_pack makes of
//                                     the span -- "kind key len" (key in hex), and for a key its decoding and the key of that:
//                                     "kind key len bases rekey" (bases - for the empty span).  nbytes may be smaller than the text given.
//   tally_host_driver table < cases   a case is "N n" followed by n keys in hex (0: not tallied): the sort as the host drives it -- the
//                                     pass count from the largest length, per pass a stable counting sort by tally_digit -- and the
//                                     run-length pass by tally_is_head; per case:  P <passes>, T <entries>, then "key count" per entry.
//   tally_host_driver                 the constants: tile, workgroup, items, radix, chunk, longest key, then tiles / matrix / chunks of
//                                     1, 1024, 1025 and 4 100 spans.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "seeq_tally.h"

static int do_span()
{
   char hex[4096];
   unsigned long long nbytes, off;
   unsigned start, end;
   while (scanf(" S %4095s %llu %llu %u %u", hex, &nbytes, &off, &start, &end) == 5) {
      std::vector<uint8_t> text;
      if (strcmp(hex, "-"))
         for (size_t i = 0; hex[i] && hex[i + 1]; i += 2) {
            unsigned b;
            if (sscanf(hex + i, "%2x", &b) != 1) { fprintf(stderr, "bad hex\n"); return 1; }
            text.push_back((uint8_t)b);
         }
      if (nbytes > text.size()) { fprintf(stderr, "nbytes beyond the text given\n"); return 1; }
      // exactly nbytes on the heap: a read beyond them is the sanitizer's to find
      uint8_t *t = (uint8_t *)malloc(nbytes ? nbytes : 1);
      if (nbytes) memcpy(t, text.data(), nbytes);
      uint64_t key;
      uint32_t len;
      const int kind = tally_span_key(t, nbytes, off, start, end, &key, &len);
      if (kind == SEEQ_TALLY_OK || kind == SEEQ_TALLY_FOREIGN) {
         // the same bytes as a thread of k_tally_pack holds them after its 16-byte loads: eight words, the rest 0
         uint32_t w[8] = {0};
         uint32_t len2;
         for (uint32_t i = 0; i < len; i++) w[i >> 2] |= (uint32_t)t[off + start + i] << (8 * (i & 3));
         if (tally_span_kind(nbytes, off, start, end, &len2) != SEEQ_TALLY_OK || len2 != len || tally_key_of_words(w, len) != key) {
            fprintf(stderr, "the key from words differs\n");
            return 2;
         }
      }
      free(t);
      if (kind != SEEQ_TALLY_OK) { printf("%d %" PRIx64 " %u\n", kind, key, len); continue; }
      char out[32];
      const int n = tally_decode(key, out);
      if (n < 0 || (uint32_t)n != len || (int)strlen(out) != n) { fprintf(stderr, "decode of %" PRIx64 " gives %d\n", key, n); return 2; }
      printf("%d %" PRIx64 " %u %s %" PRIx64 "\n", kind, key, len, n ? out : "-", tally_key_of((const uint8_t *)out, (uint32_t)n));
   }
   return 0;
}

static int do_table()
{
   unsigned n;
   while (scanf(" N %u", &n) == 1) {
      std::vector<uint64_t> a(n), b(n);
      uint32_t max_len = 0;
      for (unsigned i = 0; i < n; i++) {
         if (scanf("%" SCNx64, &a[i]) != 1) { fprintf(stderr, "short case\n"); return 1; }
         const int len = tally_key_len(a[i]);
         if (a[i] && len < 0) { fprintf(stderr, "no key: %" PRIx64 "\n", a[i]); return 1; }
         if (len > (int)max_len) max_len = (uint32_t)len;
      }
      const uint32_t passes = tally_passes(max_len);
      for (uint32_t p = 0; p < passes; p++) {
         size_t count[SEEQ_TALLY_RADIX + 1] = {0};
         for (unsigned i = 0; i < n; i++) count[tally_digit(a[i], p) + 1]++;
         for (int d = 0; d < SEEQ_TALLY_RADIX; d++) count[d + 1] += count[d];
         for (unsigned i = 0; i < n; i++) b[count[tally_digit(a[i], p)]++] = a[i];
         a.swap(b);
      }
      std::vector<unsigned> heads;
      for (unsigned i = 0; i < n; i++)
         if (tally_is_head(a[i], i ? a[i - 1] : 0, i == 0)) heads.push_back(i);
      printf("P %u\nT %zu\n", passes, heads.size());
      for (size_t j = 0; j < heads.size(); j++) printf("%" PRIx64 " %u\n", a[heads[j]], (j + 1 < heads.size() ? heads[j + 1] : n) - heads[j]);
   }
   return 0;
}

int main(int argc, char **argv)
{
   if (argc > 1 && !strcmp(argv[1], "span")) return do_span();
   if (argc > 1 && !strcmp(argv[1], "table")) return do_table();
   printf("T %d %d %d %d %d %d", SEEQ_TALLY_TILE, SEEQ_TALLY_WG, SEEQ_TALLY_ITEMS, SEEQ_TALLY_RADIX, SEEQ_TALLY_CHUNK, SEEQ_TALLY_LEN_MAX);
   const uint64_t ns[4] = {1, 1024, 1025, 4100};
   for (int i = 0; i < 4; i++) printf(" %" PRIu64 " %" PRIu64 " %" PRIu64, tally_tiles(ns[i]), tally_matrix(ns[i]), tally_chunks(ns[i]));
   printf("\n");
   return 0;
}
