// Stand-alone driver of csrc/gram_plan.h for tests/test_gram_plan_host.py: answers the queries on
// standard input, one per line, with one line each on standard output.  mask: one character per slot of
// the tile-pair triangle, '1' = skipped, or a single '-' for no mask.
//   T nb nsplit diag4 continuous mask         ->  the task table of build_task_order
//   X nb nsplit diag4 continuous              ->  gram_xcd_blocks
//   R mt nt                                   ->  the task table of atb_rect_table
//   P nb ntiles slots diag4                   ->  nsplit continuous (gram_choose_split) gram_max_split
//   D nb ntiles slots diag4 nsplit mask       ->  gram_choose_dealing
//   C free_bytes bytes_per_tile ntiles forced ->  gram_chunk_tiles
//   S nb i j                                  ->  pair_slot
#include <cinttypes>
#include <cstdio>

#include "../outerbase_amd/csrc/gram_plan.h"

static void print_table(const std::vector<uint64_t> &tab) {
  for (size_t i = 0; i < tab.size(); ++i) printf(i ? " %" PRIu64 : "%" PRIu64, tab[i]);
  printf("\n");
}

static bool read_mask(std::vector<uint8_t> &mask) {
  static char m[4096];
  if (scanf("%4095s", m) != 1) return false;
  mask.clear();
  if (m[0] != '-')
    for (const char *q = m; *q; ++q) mask.push_back(*q == '1');
  return true;
}

int main() {
  char kind;
  std::vector<uint8_t> mask;
  std::vector<uint64_t> tab;
  while (scanf(" %c", &kind) == 1) {
    if (kind == 'T') {
      int nb, nsplit, diag4, continuous;
      if (scanf("%d %d %d %d", &nb, &nsplit, &diag4, &continuous) != 4 || !read_mask(mask)) return 2;
      if (!mask.empty() && mask.size() != obhip::gram_npairs(nb)) return 2;
      obhip::build_task_order(nb, nsplit, diag4 != 0, continuous != 0, mask.empty() ? nullptr : mask.data(), tab);
      print_table(tab);
    } else if (kind == 'X') {
      int nb, nsplit, diag4, continuous;
      if (scanf("%d %d %d %d", &nb, &nsplit, &diag4, &continuous) != 4) return 2;
      printf("%" PRIu64 "\n", obhip::gram_xcd_blocks(nb, nsplit, diag4 != 0, continuous != 0));
    } else if (kind == 'R') {
      uint64_t mt, nt;
      if (scanf("%" SCNu64 " %" SCNu64, &mt, &nt) != 2) return 2;
      print_table(obhip::atb_rect_table(mt, nt));
    } else if (kind == 'P' || kind == 'D') {
      obhip::GramShape s;
      int diag4;
      if (scanf("%d %" SCNu64 " %" SCNu64 " %d", &s.nb, &s.ntiles, &s.slots, &diag4) != 4) return 2;
      s.diag4 = diag4 != 0;
      if (kind == 'P') {
        const obhip::GramPlan plan = obhip::gram_choose_split(s);
        printf("%" PRIu64 " %d %" PRIu64 "\n", plan.nsplit, (int)plan.continuous, obhip::gram_max_split(s));
      } else {
        uint64_t nsplit;
        if (scanf("%" SCNu64, &nsplit) != 1 || !read_mask(mask) || mask.size() != obhip::gram_npairs(s.nb)) return 2;
        printf("%d\n", (int)obhip::gram_choose_dealing(s, nsplit, mask.data()));
      }
    } else if (kind == 'C') {
      uint64_t free_bytes, bytes_per_tile, ntiles, forced;
      if (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &free_bytes, &bytes_per_tile, &ntiles, &forced) != 4)
        return 2;
      printf("%" PRIu64 "\n", obhip::gram_chunk_tiles(free_bytes, bytes_per_tile, ntiles, forced));
    } else if (kind == 'S') {
      int nb, i, j;
      if (scanf("%d %d %d", &nb, &i, &j) != 3) return 2;
      printf("%d\n", obhip::pair_slot(nb, i, j));
    } else {
      return 2;
    }
  }
  return 0;
}
