// Stand-alone driver of the wave-tile plan of csrc/gram_plan.h for tests/test_gram_quads_host.py: answers the
// queries on standard input, one per line, with one line each on standard output.  mask: one character per
// 64 x 64 wave tile of the upper triangle of 2 nb column groups (row-major), '1' = dropped, or a single '-'
// for none dropped.
//   K nb mask                          ->  the blocks of one row split (gram_quads_pack): I J and four wave bytes each
//   Q nb nsplit continuous mask        ->  the task table of gram_quads_table, then its wave bytes entry for entry
//   D nb ntiles slots nsplit mask      ->  gram_quads_choose_dealing
#include <cinttypes>
#include <cstdio>

#include "../outerbase_amd/csrc/gram_plan.h"

static bool read_keep(int nb, std::vector<uint8_t> &keep) {
  static char m[1 << 16];
  if (scanf("%65535s", m) != 1) return false;
  const size_t n = obhip::gram_npairs(2 * nb);
  keep.assign(n, 1);
  if (m[0] == '-') return true;
  size_t k = 0;
  for (const char *q = m; *q; ++q, ++k)
    if (k < n) keep[k] = *q != '1';
  return k == n;
}

int main() {
  char kind;
  std::vector<uint8_t> keep;
  while (scanf(" %c", &kind) == 1) {
    if (kind == 'K') {
      int nb;
      if (scanf("%d", &nb) != 1 || !read_keep(nb, keep)) return 2;
      std::vector<obhip::QuadBlock> blocks;
      obhip::gram_quads_pack(nb, keep.data(), blocks);
      for (size_t m = 0; m < blocks.size(); ++m)
        printf("%s%d %d %d %d %d %d", m ? " " : "", blocks[m].I, blocks[m].J, blocks[m].w[0], blocks[m].w[1],
               blocks[m].w[2], blocks[m].w[3]);
      printf("\n");
    } else if (kind == 'Q') {
      int nb, nsplit, continuous;
      if (scanf("%d %d %d", &nb, &nsplit, &continuous) != 3 || !read_keep(nb, keep)) return 2;
      std::vector<uint64_t> tab;
      std::vector<uint32_t> wb;
      obhip::gram_quads_table(nb, nsplit, continuous != 0, keep.data(), tab, wb);
      if (wb.size() != tab.size()) return 3;
      for (size_t i = 0; i < tab.size(); ++i) printf(i ? " %" PRIu64 : "%" PRIu64, tab[i]);
      for (size_t i = 0; i < wb.size(); ++i) printf(" %" PRIu32, wb[i]);
      printf("\n");
    } else if (kind == 'D') {
      obhip::GramShape s;
      uint64_t nsplit;
      if (scanf("%d %" SCNu64 " %" SCNu64 " %" SCNu64, &s.nb, &s.ntiles, &s.slots, &nsplit) != 4 || !read_keep(s.nb, keep))
        return 2;
      double cost = 0.0;
      const bool c = obhip::gram_quads_choose_dealing(s, nsplit, keep.data(), &cost);
      printf("%d %.0f\n", (int)c, cost * 1000.0);
    } else {
      return 2;
    }
  }
  return 0;
}
