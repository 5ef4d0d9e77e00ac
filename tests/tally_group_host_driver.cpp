// The grouped tally's rule of seeq_amd/csrc/seeq_tally_group.h (the group of a line, what a member span is, the pass count, the digit of a
// pass, the two head predicates, the two tables) compiled for the host by plain g++, for tests/test_tally_group_host.py.
//
//   tally_group_host_driver group < cases   a case is "H nh" + nh rows "line key" (key in hex), then "Q nq" + nq lines: per query line its
//                                           group (hex), by tally_group_of over exactly nh heap entries (nh = 0: none are allocated).
//   tally_group_host_driver passes < cases  a case is "npaired max_len key_bits": tally_pair_passes, and the member passes of it.
//   tally_group_host_driver demux < words   per demux record's last word (hex): its group (tally_demux_group) and the group's bits.
//   tally_group_host_driver table < cases   a case is "N n" + n rows "g m" (hex), SORTED: per item "ph gh" (the head predicates), then the
//                                           tables as below.
//   tally_group_host_driver pairs < cases   the whole rule as the host drives it.  A case is "H nh" + nh rows "line key", then "M nm" + nm
//                                           rows "line seq" (seq in hex, - for the empty span, ! for a span with end < start): the member
//                                           key by tally_span_key, the group by tally_group_of, the kind by tally_pair_kind, (g, m) or
//                                           (0, 0) stored at the span's index, the stable counting sort by tally_pair_digit, the heads.
//                                           Output: "C npaired nlong nforeign nungrouped nbad max_len key_bits passes", then the tables.
//   the tables                              "P np" + np rows "g m count", "G ng" + ng rows "g count first ndistinct".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "seeq_tally_group.h"

struct Held {
   uint32_t *line;
   uint64_t *key;
   uint32_t  nh;
   uint32_t  key_bits;
};

// exactly nh entries on the heap: a probe beyond them is the sanitizer's to find
static bool read_held(Held *h)
{
   unsigned nh;
   if (scanf(" H %u", &nh) != 1) return false;
   h->nh = nh; h->key_bits = 0;
   h->line = nh ? (uint32_t *)malloc(nh * sizeof(uint32_t)) : NULL;
   h->key = nh ? (uint64_t *)malloc(nh * sizeof(uint64_t)) : NULL;
   for (unsigned i = 0; i < nh; i++) {
      if (scanf("%u %" SCNx64, &h->line[i], &h->key[i]) != 2) { fprintf(stderr, "short held column\n"); exit(1); }
      const uint32_t b = tally_key_bits(h->key[i]);
      if (b > h->key_bits) h->key_bits = b;
   }
   return true;
}

static void free_held(Held *h) { free(h->line); free(h->key); }

static void print_tables(const std::vector<uint64_t> &g, const std::vector<uint64_t> &m)
{
   const size_t n = g.size();
   std::vector<size_t> ppos, gpos, grank;
   for (size_t i = 0; i < n; i++) {
      const uint64_t pg = i ? g[i - 1] : 0, pm = i ? m[i - 1] : 0;
      const int ph = tally_is_pair_head(g[i], m[i], pg, pm, i == 0), gh = tally_is_group_head(g[i], pg, i == 0);
      if (gh && !ph) { fprintf(stderr, "a group head that is no pair head\n"); exit(2); }
      if (gh) { gpos.push_back(i); grank.push_back(ppos.size()); }
      if (ph) ppos.push_back(i);
   }
   printf("P %zu\n", ppos.size());
   for (size_t j = 0; j < ppos.size(); j++)
      printf("%" PRIx64 " %" PRIx64 " %zu\n", g[ppos[j]], m[ppos[j]], (j + 1 < ppos.size() ? ppos[j + 1] : n) - ppos[j]);
   printf("G %zu\n", gpos.size());
   for (size_t r = 0; r < gpos.size(); r++)
      printf("%" PRIx64 " %zu %zu %zu\n", g[gpos[r]], (r + 1 < gpos.size() ? gpos[r + 1] : n) - gpos[r], grank[r],
             (r + 1 < gpos.size() ? grank[r + 1] : ppos.size()) - grank[r]);
}

static int do_group()
{
   Held h;
   while (read_held(&h)) {
      unsigned nq;
      if (scanf(" Q %u", &nq) != 1) { fprintf(stderr, "no queries\n"); return 1; }
      for (unsigned i = 0; i < nq; i++) {
         unsigned line;
         if (scanf("%u", &line) != 1) { fprintf(stderr, "short queries\n"); return 1; }
         printf("%" PRIx64 "\n", tally_group_of(h.line, h.key, h.nh, line));
      }
      free_held(&h);
   }
   return 0;
}

static int do_passes()
{
   unsigned long long npaired;
   unsigned max_len, key_bits;
   while (scanf("%llu %u %u", &npaired, &max_len, &key_bits) == 3)
      printf("%u %u\n", tally_pair_passes(npaired, max_len, key_bits), tally_passes(max_len));
   return 0;
}

static int do_demux()
{
   unsigned w;
   while (scanf("%x", &w) == 1) {
      const uint64_t g = tally_demux_group(w);
      printf("%" PRIx64 " %u\n", g, tally_key_bits(g));
   }
   return 0;
}

static int do_table()
{
   unsigned n;
   while (scanf(" N %u", &n) == 1) {
      std::vector<uint64_t> g(n), m(n);
      for (unsigned i = 0; i < n; i++)
         if (scanf("%" SCNx64 " %" SCNx64, &g[i], &m[i]) != 2) { fprintf(stderr, "short case\n"); return 1; }
      for (unsigned i = 0; i < n; i++)
         printf("%d %d\n", tally_is_pair_head(g[i], m[i], i ? g[i - 1] : 0, i ? m[i - 1] : 0, i == 0), tally_is_group_head(g[i], i ? g[i - 1] : 0, i == 0));
      print_tables(g, m);
   }
   return 0;
}

static int do_pairs()
{
   Held h;
   while (read_held(&h)) {
      unsigned nm;
      if (scanf(" M %u", &nm) != 1) { fprintf(stderr, "no members\n"); return 1; }
      std::vector<uint64_t> g(nm), m(nm), g2(nm), m2(nm);
      unsigned long long count[5] = {0, 0, 0, 0, 0};
      uint32_t max_len = 0;
      for (unsigned i = 0; i < nm; i++) {
         unsigned line;
         char hex[256];
         if (scanf("%u %255s", &line, hex) != 2) { fprintf(stderr, "short members\n"); return 1; }
         std::vector<uint8_t> seq;
         const bool bad = !strcmp(hex, "!");
         if (!bad && strcmp(hex, "-"))
            for (size_t k = 0; hex[k] && hex[k + 1]; k += 2) {
               unsigned b;
               if (sscanf(hex + k, "%2x", &b) != 1) { fprintf(stderr, "bad hex\n"); return 1; }
               seq.push_back((uint8_t)b);
            }
         const size_t nbytes = seq.size();
         uint8_t *t = (uint8_t *)malloc(nbytes ? nbytes : 1);
         if (nbytes) memcpy(t, seq.data(), nbytes);
         uint64_t key;
         uint32_t len;
         const int mk = bad ? tally_span_key(t, nbytes, 0, 1, 0, &key, &len) : tally_span_key(t, nbytes, 0, 0, (uint32_t)nbytes, &key, &len);
         free(t);
         const uint64_t grp = tally_group_of(h.line, h.key, h.nh, line);
         const int kind = tally_pair_kind(mk, grp);      // (long, foreign and bad are decided on the member, whatever its line's group)
         count[kind]++;
         const bool paired = kind == SEEQ_TALLY_OK;
         g[i] = paired ? grp : 0; m[i] = paired ? key : 0;
         if (paired && len > max_len) max_len = len;
      }
      const uint32_t mpasses = tally_passes(max_len);
      const uint32_t passes = tally_pair_passes(count[SEEQ_TALLY_OK], max_len, h.key_bits);
      for (uint32_t p = 0; p < passes; p++) {
         size_t cnt[SEEQ_TALLY_RADIX + 1] = {0};
         for (unsigned i = 0; i < nm; i++) cnt[tally_pair_digit(g[i], m[i], p, mpasses) + 1]++;
         for (int d = 0; d < SEEQ_TALLY_RADIX; d++) cnt[d + 1] += cnt[d];
         for (unsigned i = 0; i < nm; i++) {
            const size_t j = cnt[tally_pair_digit(g[i], m[i], p, mpasses)]++;
            g2[j] = g[i]; m2[j] = m[i];
         }
         g.swap(g2); m.swap(m2);
      }
      printf("C %llu %llu %llu %llu %llu %u %u %u\n", count[SEEQ_TALLY_OK], count[SEEQ_TALLY_LONG], count[SEEQ_TALLY_FOREIGN], count[SEEQ_TALLY_UNGROUPED],
             count[SEEQ_TALLY_BAD], max_len, h.key_bits, passes);
      print_tables(g, m);
      free_held(&h);
   }
   return 0;
}

int main(int argc, char **argv)
{
   if (argc > 1 && !strcmp(argv[1], "group")) return do_group();
   if (argc > 1 && !strcmp(argv[1], "passes")) return do_passes();
   if (argc > 1 && !strcmp(argv[1], "demux")) return do_demux();
   if (argc > 1 && !strcmp(argv[1], "table")) return do_table();
   if (argc > 1 && !strcmp(argv[1], "pairs")) return do_pairs();
   printf("G %d %d %d %d\n", SEEQ_TALLY_TILE, SEEQ_TALLY_UNGROUPED, SEEQ_TALLY_PROBES, SEEQ_TALLY_LEN_MAX);
   return 0;
}
