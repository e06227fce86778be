// The arithmetic every product launch shares: how the row tiles are split over blocks and how many
// terms a lane takes.  Plain C++17 with nothing from HIP, so that a host compiler can check it alone
// (tests/launch_plan_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>

namespace obhip {

// Row tiles dealt to blocks: block r takes the tiles [r * tps, min(ntiles, (r + 1) * tps)).
struct RowSplit {
  uint64_t nsplit;  // blocks along the rows, none of them empty
  uint64_t tps;     // tiles per block
};
// `want` blocks if the rows allow it: at least one, and no block with fewer than min_tiles tiles
// unless a single block has them all; then as few blocks as still take ceil(ntiles / nsplit) each.
// ntiles >= 1.
inline RowSplit split_rows(uint64_t ntiles, uint64_t want, uint64_t min_tiles = 1) {
  const uint64_t cap = std::max<uint64_t>(1, ntiles / min_tiles);
  const uint64_t nsplit = std::min(std::max<uint64_t>(1, want), cap);
  const uint64_t tps = (ntiles + nsplit - 1) / nsplit;
  return {(ntiles + tps - 1) / tps, tps};
}

// Units (groups or pairs of groups of 64 terms) per lane of a term-per-lane kernel: doubled until
// one block of terms_per_unit * units terms covers p_pad or the ceiling is reached -- the fewest
// blocks along the terms that the register budget allows.
inline int units_per_lane(uint64_t p_pad, uint64_t terms_per_unit, int max_units) {
  int units = 1;
  while (units < max_units && terms_per_unit * units < p_pad) units *= 2;
  return units;
}

// The ceilings by W2 = factors of a term / 2 (rounded up), one per kernel family; the dispatch of
// a family instantiates no kernel above its ceiling.
// k_mm_tl (NG) and k_hm_tl (NU): 8 terms of 6 factors per lane spill and run at half the speed
constexpr int tl_max_units(int w2) { return w2 <= 2 ? 8 : 4; }
// k_tmm_tl and k_materialize_tl (NPAIR, two groups each): six-slot terms take 4 terms per lane at
// 123 VGPRs, 8 would spill
constexpr int tl_max_pairs(int w2) { return w2 <= 2 ? 4 : 2; }
// k_predict_tl (NG): the variance form carries twice the accumulators and coefficients, so half
// the terms per lane
constexpr int predict_tl_max_units(int w2, bool var) { return tl_max_units(w2) / (var ? 2 : 1); }

}  // namespace obhip
