// The anchored cut of seeq_amd/csrc/seeq_anchor.h compiled for the host by plain g++, for tests/test_anchor_host.py.
//
//   anchor_host_driver cut < cases    a case is "T <nbytes> <text in hex>" and then any number of
//                                     "S off start end anchor skip len reach": per record one line "kind s e" by anchor_span_kind, the rule
//                                     byte by byte.  The same record goes through anchor_span_load, the decision as the kernel takes it (the
//                                     walk in steps of 64 bytes), and the driver fails where the two differ -- and where anchor_start does
//                                     not give a kept cut's start back from its end, as k_anchor_apply relies on.  The text is a heap block
//                                     of exactly nbytes bytes: a read beyond it is the sanitizer's to find.
//   anchor_host_driver                the constants: tile, the three anchors, the four kinds, the largest reach, the tile's numbers.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "seeq_anchor.h"

static int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

static int do_cut()
{
   uint8_t *text = NULL;
   unsigned long long nbytes = 0;
   char tag;
   while (scanf(" %c", &tag) == 1) {
      if (tag == 'T') {
         if (scanf("%llu", &nbytes) != 1) { fprintf(stderr, "no size\n"); return 1; }
         free(text);
         text = (uint8_t *)malloc(nbytes ? nbytes : 1);
         int c;
         while ((c = getchar()) == ' ') {}
         ungetc(c, stdin);
         for (unsigned long long i = 0; i < nbytes; i++) {
            const int hi = hexval(getchar()), lo = hexval(getchar());
            if (hi < 0 || lo < 0) { fprintf(stderr, "short text\n"); return 1; }
            text[i] = (uint8_t)(hi * 16 + lo);
         }
      } else if (tag == 'S') {
         unsigned long long off;
         unsigned start, end, skip, len, reach;
         int anchor;
         if (scanf("%llu %u %u %d %u %u %u", &off, &start, &end, &anchor, &skip, &len, &reach) != 7) { fprintf(stderr, "short record\n"); return 1; }
         uint32_t s, e, s2, e2;
         const int kind = anchor_span_kind(text, nbytes, off, start, end, anchor, skip, len, reach, &s, &e);
         const int kind2 = anchor_span_load(text, nbytes, off, start, end, anchor, skip, len, reach, qgate_steps(reach), &s2, &e2);
         if (kind != kind2 || s != s2 || e != e2) {
            fprintf(stderr, "the walk differs from the rule for off %llu [%u, %u) anchor %d skip %u len %u reach %u: %d %u %u vs %d %u %u\n", off, start, end, anchor,
                    skip, len, reach, kind2, s2, e2, kind, s, e);
            return 2;
         }
         if (kind == SEEQ_ANCHOR_KEPT && anchor_start(anchor, skip, len, end, e) != s) {
            fprintf(stderr, "anchor_start differs for off %llu [%u, %u) anchor %d skip %u len %u: %u vs %u\n", off, start, end, anchor, skip, len,
                    anchor_start(anchor, skip, len, end, e), s);
            return 2;
         }
         printf("%d %u %u\n", kind, s, e);
      } else {
         fprintf(stderr, "unknown case %c\n", tag);
         return 1;
      }
   }
   free(text);
   return 0;
}

int main(int argc, char **argv)
{
   if (argc > 1 && !strcmp(argv[1], "cut")) return do_cut();
   printf("B %d %d %d %d %d %d %d %d %u %d\n", SEEQ_ANCHOR_TILE, SEEQ_ANCHOR_AFTER, SEEQ_ANCHOR_BEFORE, SEEQ_ANCHOR_LINE, SEEQ_ANCHOR_KEPT, SEEQ_ANCHOR_SHORT,
          SEEQ_ANCHOR_FAR, SEEQ_ANCHOR_BAD, SEEQ_ANCHOR_REACH_MAX, SEEQ_ANCHOR_SUMS);
   return 0;
}
