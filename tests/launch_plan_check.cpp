// Stand-alone driver of csrc/launch_plan.h for tests/test_launch_plan_host.py: answers the queries on
// standard input, one per line, with one line each on standard output.
//   S ntiles want min_tiles      ->  nsplit tps
//   U p_pad terms_per_unit max   ->  units
//   C w2                         ->  tl_max_units tl_max_pairs predict_tl_max_units(mean) (variance)
#include <cinttypes>
#include <cstdio>

#include "../outerbase_amd/csrc/launch_plan.h"

int main() {
  char kind;
  while (scanf(" %c", &kind) == 1) {
    if (kind == 'S') {
      uint64_t ntiles, want, min_tiles;
      if (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &ntiles, &want, &min_tiles) != 3) return 2;
      const obhip::RowSplit rs = obhip::split_rows(ntiles, want, min_tiles);
      printf("%" PRIu64 " %" PRIu64 "\n", rs.nsplit, rs.tps);
    } else if (kind == 'U') {
      uint64_t p_pad, tpu;
      int mx;
      if (scanf("%" SCNu64 " %" SCNu64 " %d", &p_pad, &tpu, &mx) != 3) return 2;
      printf("%d\n", obhip::units_per_lane(p_pad, tpu, mx));
    } else if (kind == 'C') {
      int w2;
      if (scanf("%d", &w2) != 1) return 2;
      printf("%d %d %d %d\n", obhip::tl_max_units(w2), obhip::tl_max_pairs(w2),
             obhip::predict_tl_max_units(w2, false), obhip::predict_tl_max_units(w2, true));
    } else {
      return 2;
    }
  }
  return 0;
}
