// The insert rule of seeq_amd/csrc/seeq_insert.h (first candidate, walk, chosen right record; output byte -> record of the insert text)
// compiled for the host by plain g++, for tests/test_insert_host.py.
//
//   insert_host_driver join < cases   a case is "C mode min_len max_len nl nr" followed by nl left and nr right records
//                                     "line start end dist", the left list one per line in line order, the right list in key order; per
//                                     case:  J <nl>, then per left record what one thread of k_insert_join stores at its index:
//                                     "line start end ldist rdist" (line 0: no insert; start then tells whether the line has a right record)
//   insert_host_driver text < cases   a case is "T n nbytes" followed by the text (nbytes characters, '|' for a newline) and n insert records
//                                     "start end offset"; per case:  X <total>, then per output byte "record within" (within -1: the
//                                     record's newline) by insert_text_record, then "B <bad>" and the text as the threads of k_insert_text
//                                     fill it, SEEQ_INSERT_RUN bytes each ('|' for a newline, '?' for a byte that was not filled)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "seeq_insert.h"

static int do_join()
{
   int mode;
   unsigned min_len, max_len, nl, nr;
   while (scanf(" C %d %u %u %u %u", &mode, &min_len, &max_len, &nl, &nr) == 5) {
      std::vector<strand_rec_t> l(nl), r(nr);
      for (unsigned i = 0; i < nl + nr; i++) {
         strand_rec_t &q = i < nl ? l[i] : r[i - nl];
         if (scanf("%u %u %u %u", &q.x, &q.y, &q.z, &q.w) != 4) { fprintf(stderr, "short case\n"); return 1; }
      }
      printf("J %u\n", nl);
      for (unsigned i = 0; i < nl; i++) {
         const strand_rec_t o = insert_join_one(mode, l[i], r.data(), nr, min_len, max_len);
         printf("%u %u %u %u %u\n", o.x, o.y, o.z, o.w & 0xFFFFu, o.w >> 16);
      }
   }
   return 0;
}

static int do_text()
{
   unsigned n;
   unsigned long long nbytes;
   while (scanf(" T %u %llu", &n, &nbytes) == 2) {
      std::string text(nbytes, ' ');
      for (unsigned long long i = 0; i < nbytes; i++) {
         int c;
         do c = getchar(); while (c == '\n' || c == ' ');
         if (c == EOF) { fprintf(stderr, "short text\n"); return 1; }
         text[i] = c == '|' ? '\n' : (char)c;
      }
      std::vector<strand_rec_t> rec(n);
      std::vector<uint64_t> off(n), pos(n);
      uint64_t total = 0;
      for (unsigned k = 0; k < n; k++) {
         unsigned long long o;
         rec[k].x = k + 1; rec[k].w = 0;
         if (scanf("%u %u %llu", &rec[k].y, &rec[k].z, &o) != 3) { fprintf(stderr, "short case\n"); return 1; }
         off[k] = o;
         pos[k] = total;                                    // what k_insert_apply writes: the exclusive prefix
         total += insert_text_len(rec[k]);
      }
      printf("X %llu\n", (unsigned long long)total);
      for (uint64_t b = 0; b < total; b++) {
         const uint32_t k = insert_text_record(pos.data(), n, b);
         if (k >= n) { fprintf(stderr, "byte %llu has no record\n", (unsigned long long)b); return 2; }
         const uint64_t within = b - pos[k];
         printf("%u %lld\n", k, within == (uint64_t)(rec[k].z - rec[k].y) ? -1ll : (long long)within);
      }
      // what the threads of k_insert_text do, one run each
      std::string out(total, '?');
      int bad = 0;
      for (uint64_t b0 = 0; b0 < total; b0 += SEEQ_INSERT_RUN) {
         const int cnt = total - b0 < SEEQ_INSERT_RUN ? (int)(total - b0) : SEEQ_INSERT_RUN;
         uint32_t w[SEEQ_INSERT_RUN / 4];
         bad |= insert_text_fill(rec.data(), off.data(), pos.data(), n, (const uint8_t *)text.data(), nbytes, b0, cnt, w);
         for (int i = 0; i < cnt; i++) {
            const char c = (char)(w[i >> 2] >> (8 * (i & 3)));
            out[b0 + i] = c == '\n' ? '|' : c ? c : '?';
         }
      }
      printf("B %d\n%s\n", bad, out.c_str());
   }
   return 0;
}

int main(int argc, char **argv)
{
   if (argc > 1 && !strcmp(argv[1], "join")) return do_join();
   if (argc > 1 && !strcmp(argv[1], "text")) return do_text();
   printf("T %d %d %d %d %u\n", SEEQ_INSERT_TILE, SEEQ_INSERT_WG, SEEQ_INSERT_ITEMS, SEEQ_INSERT_RUN, (unsigned)sizeof(strand_rec_t));
   return 0;
}
