// The FASTQ rule of seeq_amd/csrc/seeq_fastq.h (predicate, renumbering, counted lines) compiled for the host by plain g++ and
// printed for tests/test_fastq_host.py:   L <raw line> <is sequence line> <record number>     N <raw lines> <records counted>
#include <cstdio>
#include <cstdlib>

#include "seeq_fastq.h"

int main(int argc, char **argv)
{
   const unsigned nl = argc > 1 ? (unsigned)atoi(argv[1]) : 41u, nn = argc > 2 ? (unsigned)atoi(argv[2]) : 13u;
   for (uint32_t line = 1; line <= nl; line++)
      printf("L %u %d %u\n", line, fastq_is_sequence_line(line), fastq_is_sequence_line(line) ? fastq_record_of_line(line) : 0u);
   for (uint64_t raw = 0; raw <= nn; raw++) printf("N %llu %llu\n", (unsigned long long)raw, (unsigned long long)fastq_nlines(raw));
   printf("T %d %d %d\n", SEEQ_FASTQ_TILE, SEEQ_FASTQ_WG, SEEQ_FASTQ_ITEMS);
   return 0;
}
