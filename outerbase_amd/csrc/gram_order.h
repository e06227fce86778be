// The order in which the panel Gram stages and multiplies its columns, and the sequential pass that decides
// which 64 x 64 wave tiles of G in that order are dropped.  Plain C++17 beside gram_plan.h: nothing from HIP,
// no environment, no device query (tests/gram_order_check.cpp compiles it alone).
//
// The caller's term order stays what it is everywhere else.  Column k of the staged design matrix is term
// perm[k]: the terms in a STABLE sort by their number of factors, ascending.  An entry of G depends on the
// per-dimension unordered level pairs of its two terms only (gram_dedup.hip), and a (2-factor, 4-factor) pair
// always repeats a (3-factor, 3-factor) one when every 3-subset of the dimensions is a term: the sort makes
// the blocks of such repeats contiguous, so more wave tiles consist of repeats alone.
//
// The sequential pass, the serial definition every implementation must reproduce tile for tile
// (gram_seq_pass below; k_seq_walk of gram_dedup.hip on the device):
//   entries   the upper-triangle entries (s <= t < p) of wave tile (a <= b), s in column group a, t in b.  Two
//             entries are of one class when their d unordered level pairs are equal.  A class that holds an
//             entry of the diagonal of G (a duplicate term) is left alone: its entries are not counted and the
//             wave tiles that hold them stay (a formed sink holds e2 G + the prior there).
//   by rule   the wave tiles of the diagonal tile pairs (a / 2 == b / 2) and those that reach into the padding
//             columns ((b + 1) * 64 > p) never drop.
//   walk      the other wave tiles from the largest b - a down to 1, the smallest a first among equals.  A
//             tile drops when every one of its entries still has another occurrence in a tile not yet dropped:
//             take its entries off the per-class counts, test that none of their classes is at zero, put them
//             back on failure.
//   sources   of a dropped entry: the first occurrence of its class in a surviving tile, in the order of
//             priority of the parallel rule (smallest b - a, then smallest a, then row-major in the tile).
// Counts only fall and a tile drops only while every class it holds keeps a survivor, so every dropped entry
// has a source at the end.
#pragma once
#include <numeric>

#include "gram_plan.h"

namespace obhip {

// launches of one term set the set-up of the order is spread over (a fit is a few Newton or IRLS steps, a
// hyper-parameter search many more): the one departure from the "pays within one launch" rule of the
// wave-tile plan
constexpr int kGramOrderLaunches = 4;
// What the order costs a term set, once, in host wall time: permutation, analysis in Gram coordinates with the
// sequential pass, packing and the two dealings priced.  11.1 ms measured at the headline set (DESIGN.md section
// 5), half as much again for the run-to-run spread, as kQuadsSetupMs takes it.
constexpr double kGramOrderSetupMs = 17.0;
// The set-up grows with the number of wave tiles (the sort and the class kernels with their entries, the
// one-workgroup walk with the tiles it visits: about four times the headline's at p = 8192), so a larger term set is
// charged in proportion; a smaller one is charged the headline's figure, which keeps short launches out.
constexpr double kGramOrderSetupTiles = 2080.0;  // wave tiles of the headline's upper triangle (p = 4096)
inline double gram_order_setup_ms(int nb) {
  return kGramOrderSetupMs * std::max(1.0, (double)gram_npairs(2 * nb) / kGramOrderSetupTiles);
}

// perm[k] = the term staged as column k: stable by the number of factors (non-zero levels), ascending
inline std::vector<uint32_t> gram_order_perm(const uint32_t *lev, uint64_t p, uint64_t d) {
  std::vector<uint32_t> nf(p, 0), perm(p);
  for (uint64_t k = 0; k < p; ++k)
    for (uint64_t j = 0; j < d; ++j) nf[k] += lev[k * d + j] != 0;
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return nf[x] < nf[y]; });
  return perm;
}
inline bool gram_perm_is_identity(const std::vector<uint32_t> &perm) {
  for (size_t k = 0; k < perm.size(); ++k)
    if (perm[k] != k) return false;
  return true;
}
inline std::vector<uint32_t> gram_perm_inverse(const std::vector<uint32_t> &perm) {
  std::vector<uint32_t> inv(perm.size());
  for (size_t k = 0; k < perm.size(); ++k) inv[perm[k]] = (uint32_t)k;
  return inv;
}
// the level table in Gram order: row k = the levels of term perm[k]
inline std::vector<uint32_t> gram_perm_levels(const uint32_t *lev, uint64_t d, const std::vector<uint32_t> &perm) {
  std::vector<uint32_t> out(perm.size() * d);
  for (size_t k = 0; k < perm.size(); ++k) std::copy(lev + perm[k] * d, lev + (perm[k] + 1) * d, out.begin() + k * d);
  return out;
}

// rank of wave tile (a <= b) in the order of priority over ng column groups: smallest b - a first, then smallest a
constexpr int wave_rank(int ng, int a, int b) {
  return (b - a) * ng - (b - a) * (b - a - 1) / 2 + a;
}

// Whether the ordered plan is taken without being forced: it saves a block per split against the plan the
// launch would otherwise run, and kGramOrderLaunches launches save more modelled time than the set-up costs.
inline bool gram_order_pays(int nb, double cost_other, int blocks_other, double cost_order, int blocks_order,
                            double block_tile_ms) {
  return blocks_order + 1 <= blocks_other &&
         kGramOrderLaunches * (cost_other - cost_order) * block_tile_ms > gram_order_setup_ms(nb);
}
// ... and a launch whose modelled time is so short that it could not pay is not even analysed
inline bool gram_order_worth_analysing(int nb, double cost_other, double block_tile_ms) {
  return kGramOrderLaunches * cost_other * block_tile_ms > gram_order_setup_ms(nb);
}

// The serial definition, on the host (tests; the library runs k_seq_walk).  lev: p x d levels in the order the
// Gram stages its columns.  keep: one byte per wave tile, slot pair_slot(ng, a, b), 0 = dropped.  src (may be
// null): per dropped wave tile in the order of `dropped` (a | b << 16) its 64 x 64 sources s' << 16 | t'.
// parallel = true: the parallel rule of gram_dedup.hip instead (a tile that holds no first occurrence drops).
inline void gram_seq_pass(const uint32_t *lev, uint64_t p, uint64_t d, bool parallel, std::vector<uint8_t> &keep,
                          std::vector<uint32_t> *dropped = nullptr, std::vector<uint32_t> *src = nullptr) {
  const int ng = (int)((p + kGramTile - 1) / kGramTile) * 2;
  const size_t ntile = gram_npairs(ng);
  constexpr uint32_t kNone = ~0u;
  // the upper entries tile by tile in the order of priority
  struct Entry { uint32_t s, t, tile; };
  std::vector<Entry> ent;
  for (int dist = 0; dist < ng; ++dist)
    for (int a = 0; a + dist < ng; ++a)
      for (uint32_t r = 0; r < 64; ++r)
        for (uint32_t c = 0; c < 64; ++c) {
          const uint32_t s = (uint32_t)a * 64 + r, t = (uint32_t)(a + dist) * 64 + c;
          if (s < p && t < p && s <= t) ent.push_back({s, t, (uint32_t)wave_rank(ng, a, a + dist)});
        }
  // classes: sort by the unordered level pairs themselves (two 64-bit mixes first, the pairs decide ties)
  auto pairs_cmp = [&](const Entry &x, const Entry &y) {
    for (uint64_t k = 0; k < d; ++k) {
      const uint32_t a = lev[x.s * d + k], b = lev[x.t * d + k], a2 = lev[y.s * d + k], b2 = lev[y.t * d + k];
      const uint64_t u = (uint64_t)std::max(a, b) << 32 | std::min(a, b), v = (uint64_t)std::max(a2, b2) << 32 | std::min(a2, b2);
      if (u != v) return u < v ? -1 : 1;
    }
    return 0;
  };
  std::vector<uint64_t> key(ent.size());
  for (size_t e = 0; e < ent.size(); ++e) {
    uint64_t h = 0x9e3779b97f4a7c15ull;
    for (uint64_t k = 0; k < d; ++k) {
      const uint32_t a = lev[ent[e].s * d + k], b = lev[ent[e].t * d + k];
      h ^= ((uint64_t)std::max(a, b) << 32 | std::min(a, b)) + k * 0x100000001b3ull;
      h = (h ^ (h >> 29)) * 0xbf58476d1ce4e5b9ull;
    }
    key[e] = h ^ (h >> 32);
  }
  std::vector<uint32_t> idx(ent.size());
  std::iota(idx.begin(), idx.end(), 0u);
  std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) {
    if (key[x] != key[y]) return key[x] < key[y];
    const int c = pairs_cmp(ent[x], ent[y]);
    return c != 0 ? c < 0 : x < y;
  });
  std::vector<uint32_t> cls(ent.size(), kNone), first;  // class of an entry; first entry (in priority) of a class
  std::vector<uint8_t> has_diag;
  for (size_t i = 0; i < idx.size(); ++i) {
    if (i == 0 || key[idx[i]] != key[idx[i - 1]] || pairs_cmp(ent[idx[i]], ent[idx[i - 1]]) != 0) {
      first.push_back(idx[i]);
      has_diag.push_back(0);
    }
    cls[idx[i]] = (uint32_t)first.size() - 1;
    if (ent[idx[i]].s == ent[idx[i]].t) has_diag.back() = 1;
  }
  auto by_rule = [&](int a, int b) { return a / 2 == b / 2 || (uint64_t)(b + 1) * 64 > p; };
  std::vector<uint8_t> gone(ntile, 0), stays(ntile, 0);  // by rank
  std::vector<uint32_t> tile0(ntile + 1, 0);             // the entries of a tile are contiguous in ent
  for (const Entry &e : ent) ++tile0[e.tile + 1];
  for (size_t r = 0; r < ntile; ++r) tile0[r + 1] += tile0[r];
  std::vector<uint32_t> cnt(first.size(), 0);
  for (size_t e = 0; e < ent.size(); ++e) {
    if (has_diag[cls[e]]) stays[ent[e].tile] = 1;
    else ++cnt[cls[e]];
  }
  if (parallel) {
    std::vector<uint8_t> holds_first(ntile, 0);
    for (uint32_t f : first) holds_first[ent[f].tile] = 1;
    for (int dist = 1; dist < ng; ++dist)
      for (int a = 0; a + dist < ng; ++a) {
        const int r = wave_rank(ng, a, a + dist);
        if (!by_rule(a, a + dist) && !stays[r] && !holds_first[r]) gone[r] = 1;
      }
  } else {
    for (int dist = ng - 1; dist >= 1; --dist)
      for (int a = 0; a + dist < ng; ++a) {
        const int r = wave_rank(ng, a, a + dist);
        if (by_rule(a, a + dist) || stays[r]) continue;
        for (uint32_t e = tile0[r]; e < tile0[r + 1]; ++e) --cnt[cls[e]];
        bool ok = true;
        for (uint32_t e = tile0[r]; e < tile0[r + 1] && ok; ++e) ok = cnt[cls[e]] >= 1;
        if (ok) gone[r] = 1;
        else
          for (uint32_t e = tile0[r]; e < tile0[r + 1]; ++e) ++cnt[cls[e]];
      }
  }
  keep.assign(ntile, 1);
  if (dropped) dropped->clear();
  if (src) src->clear();
  // the first surviving occurrence of every class (ent is in the order of priority)
  std::vector<uint32_t> survivor(first.size(), kNone);
  for (size_t e = 0; e < ent.size(); ++e)
    if (!gone[ent[e].tile] && survivor[cls[e]] == kNone) survivor[cls[e]] = (uint32_t)e;
  for (int a = 0; a < ng; ++a)
    for (int b = a; b < ng; ++b) {
      const int r = wave_rank(ng, a, b);
      if (!gone[r]) continue;
      keep[(size_t)pair_slot(ng, a, b)] = 0;
      if (dropped) dropped->push_back((uint32_t)a | (uint32_t)b << 16);
      if (src)
        for (uint32_t e = tile0[r]; e < tile0[r + 1]; ++e) {  // (a dropped tile holds all 64 x 64, row-major)
          const uint32_t f = survivor[cls[e]];
          src->push_back(f == kNone ? kNone : ent[f].s << 16 | ent[f].t);
        }
    }
}

}  // namespace obhip
