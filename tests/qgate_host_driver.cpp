// The base-quality rule of seeq_amd/csrc/seeq_qgate.h compiled for the host by plain g++, for tests/test_qgate_host.py.
//
//   qgate_host_driver gate < cases    a case is "T <nbytes> <text in hex>" and then any number of
//                                     "S off start end thr max_low reach": per span one line "kind nlow" by qgate_span_kind, the rule byte
//                                     by byte.  The same span goes through qgate_span_load, the decision as the kernel takes it (the walk
//                                     in steps of 64 bytes, the wide loads), and the driver fails where the two differ.  The text is a
//                                     heap block of exactly nbytes bytes: a read beyond it is the sanitizer's to find.
//   qgate_host_driver nl < words      a word in hex per line: qgate_nl4's four bits.
//   qgate_host_driver                 the constants: tile, the six kinds, the largest reach, the walk's step, the longest span.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "seeq_qgate.h"

static int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

static int do_gate()
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
         unsigned start, end, thr, max_low, reach;
         if (scanf("%llu %u %u %u %u %u", &off, &start, &end, &thr, &max_low, &reach) != 6) { fprintf(stderr, "short span\n"); return 1; }
         uint32_t nlow, nlow2;
         const int kind = qgate_span_kind(text, nbytes, off, start, end, thr, max_low, reach, &nlow);
         const int kind2 = qgate_span_load(text, nbytes, off, start, end, thr, max_low, reach, qgate_steps(reach), &nlow2);
         if (kind != kind2 || nlow != nlow2) {
            fprintf(stderr, "the walk differs from the rule for off %llu [%u, %u) reach %u: %d %u vs %d %u\n", off, start, end, reach, kind2, nlow2, kind, nlow);
            return 2;
         }
         printf("%d %u\n", kind, nlow);
      } else {
         fprintf(stderr, "unknown case %c\n", tag);
         return 1;
      }
   }
   free(text);
   return 0;
}

static int do_nl()
{
   uint32_t w;
   while (scanf("%" SCNx32, &w) == 1) printf("%u\n", qgate_nl4(w));
   return 0;
}

int main(int argc, char **argv)
{
   if (argc > 1 && !strcmp(argv[1], "gate")) return do_gate();
   if (argc > 1 && !strcmp(argv[1], "nl")) return do_nl();
   printf("B %d %d %d %d %d %d %d %u %u %d\n", SEEQ_QGATE_TILE, SEEQ_QGATE_PASS, SEEQ_QGATE_LOW, SEEQ_QGATE_LONG, SEEQ_QGATE_FAR, SEEQ_QGATE_MISFIT, SEEQ_QGATE_BAD,
          SEEQ_QGATE_REACH_MAX, SEEQ_QGATE_STEP, SEEQ_TALLY_LEN_MAX);
   return 0;
}
