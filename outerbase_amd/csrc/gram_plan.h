// What a launch of k_atb_dma2 (kernels_gram_panel.hip) runs, decided on the host: the task encoding, the
// (tile-pair square, row split) units and their dealing to the XCDs, the row split and dealing the cost
// model picks, the key the caches of those choices share, and the size of a row chunk.  Plain C++17 with
// nothing from HIP, no environment and no device query, so that a host compiler can check it alone
// (tests/gram_plan_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <tuple>
#include <vector>

namespace obhip {

constexpr int kGramTile = 128;    // output tile edge (terms)
constexpr int kGramRowTile = 64;  // rows per row tile (kTileRows of obhip_internal.h)

// ---- task encoding ------------------------------------------------------------------------------------
// tile pair (I, J), row split y, and what the block's four waves do with the two panels (type,
// atb_wave_code); k_atb_dma2 decodes it
inline uint64_t atb_task(uint64_t I, uint64_t J, uint64_t y, uint64_t type = 0) {
  return I | (J << 24) | (y << 48) | (type << 62);
}
constexpr uint64_t kAtbNoTask = ~0ull;
// row-major slot of tile pair (i <= j) in the upper triangle of nb x nb tiles
inline int pair_slot(int nb, int i, int j) { return i * nb - i * (i - 1) / 2 + (j - i); }
inline bool pair_skipped(const uint8_t *skip, int nb, int i, int j) { return skip && skip[pair_slot(nb, i, j)]; }

// ---- units and their dealing --------------------------------------------------------------------------
// Workgroups go to the 8 XCDs round-robin by linear id, so blocks x, x + 8, x + 16, ... share
// one 4-MB L2, and an XCD keeps 64 of them resident (32 CUs x 2).  The work is cut into units
// of (8 x 8 square of the tile-pair triangle, row split): the 64 blocks of a unit read 16
// panel column blocks over the same rows, so a panel row fetched by one block is an L2 hit
// for the others.  Every XCD gets whole units, one after the other (diagonal squares hold
// 36 pairs; the next unit fills the slots they leave), and all XCDs the same number of blocks
// (padding tasks exit at once).  At p = 4096: 10 squares x 32 splits = 320 units, 2112 blocks
// per XCD = 33 rounds of 64.  (The first version dealt every XCD a 66-pair run of the sorted
// pair list per split: runs straddle squares and touch 16-24 column blocks.)
//
// When the units do not pack into the 64 slots of an XCD -- one 34-block square per split at
// p = 1024: two units are 68 blocks, and the four that do not fit wait for a whole second round --
// the units are dealt CONTINUOUSLY instead (`continuous`): the task list in unit order is cut
// into 8 equal runs, a unit may straddle two XCDs (its panels are then fetched by both).
// gram_xcd_blocks tells the row-split choice what either dealing gives an XCD.
//
// Tile pairs that hold repeats of other entries of G only (`skip`, one byte per slot of the pair
// triangle, gram_dedup.hip; may be null) get no task: their squares are smaller units, and their
// slots of the partial-tile workspace stay unwritten.
constexpr int kXcd = 8, kSq = 8;

// The eight per-XCD task sequences of a table: block m * 8 + k runs the m-th task of XCD k.
struct XcdDeal {
  std::vector<uint64_t> seq[kXcd];
  // a whole run of tasks to the XCD with the fewest blocks so far (the first of equals)
  void deal(const std::vector<uint64_t> &run) {
    int k = 0;
    for (int q = 1; q < kXcd; ++q)
      if (seq[q].size() < seq[k].size()) k = q;
    seq[k].insert(seq[k].end(), run.begin(), run.end());
  }
  // the sequences interleaved, the shorter ones padded with kAtbNoTask
  std::vector<uint64_t> table() const {
    size_t len = 0;
    for (const auto &q : seq) len = std::max(len, q.size());
    std::vector<uint64_t> tab(len * kXcd, kAtbNoTask);
    for (int k = 0; k < kXcd; ++k)
      for (size_t m = 0; m < seq[k].size(); ++m) tab[m * kXcd + k] = seq[k][m];
    return tab;
  }
};

struct GramUnit {  // square (bi <= bj) of the tile-pair triangle, row split, tasks
  int bi, bj, y, size;
};
inline void gram_units(int nb, int nsplit, bool diag4, const uint8_t *skip, std::vector<GramUnit> &units) {
  const int nsq = (nb + kSq - 1) / kSq;
  for (int y = 0; y < nsplit; ++y)
    for (int bi = 0; bi < nsq; ++bi)
      for (int bj = bi; bj < nsq; ++bj) {
        int size = 0;
        for (int i = bi * kSq; i < std::min(nb, (bi + 1) * kSq); ++i)
          for (int j = std::max(i, bj * kSq); j < std::min(nb, (bj + 1) * kSq); ++j)
            if (!(i == j && diag4 && i / 4 * 4 + 3 < nb && i % 4 == 3) && !pair_skipped(skip, nb, i, j)) ++size;
        if (size) units.push_back({bi, bj, y, size});
      }
}
// blocks of the busiest XCD
inline uint64_t gram_xcd_blocks(int nb, int nsplit, bool diag4, bool continuous) {
  std::vector<GramUnit> units;
  gram_units(nb, 1, diag4, nullptr, units);  // (every split has the same units)
  uint64_t per_split = 0;
  for (const GramUnit &u : units) per_split += (uint64_t)u.size;
  if (continuous) return (per_split * (uint64_t)nsplit + kXcd - 1) / kXcd;
  std::vector<int> sizes;
  for (int y = 0; y < nsplit; ++y)
    for (const GramUnit &u : units) sizes.push_back(u.size);
  std::stable_sort(sizes.begin(), sizes.end(), [](int a, int b) { return a > b; });
  uint64_t load[kXcd] = {0};
  for (int s : sizes) {
    int k = 0;
    for (int q = 1; q < kXcd; ++q)
      if (load[q] < load[k]) k = q;
    load[k] += (uint64_t)s;
  }
  return *std::max_element(load, load + kXcd);
}
inline void build_task_order(int nb, int nsplit, bool diag4, bool continuous, const uint8_t *skip,
                             std::vector<uint64_t> &tab) {
  std::vector<GramUnit> units;
  gram_units(nb, nsplit, diag4, skip, units);
  // the tasks of a unit in its order
  auto unit_tasks = [&](const GramUnit &u, std::vector<uint64_t> &out) {
    for (int i = u.bi * kSq; i < std::min(nb, (u.bi + 1) * kSq); ++i)
      for (int j = std::max(i, u.bj * kSq); j < std::min(nb, (u.bj + 1) * kSq); ++j) {
        if (i == j && diag4) {
          // four consecutive diagonal tiles as three blocks (atb_wave_code); squares are 8 wide,
          // so a group never straddles two of them (its three blocks may still go to different
          // XCDs where the top-up below takes single tasks of a diagonal square: they write
          // disjoint wave tiles)
          const int g0 = i / 4 * 4;
          if (g0 + 3 < nb) {
            if (i - g0 < 3) out.push_back(atb_task(i, i + 1, u.y, 1 + (i - g0)));
            continue;
          }
        }
        if (pair_skipped(skip, nb, i, j)) continue;
        out.push_back(atb_task(i, j, u.y));
      }
  };
  XcdDeal xcd;
  // whole runs of tasks, the largest first, each to the XCD with the fewest blocks so far (stable:
  // the order of equal-sized runs keeps squares of one split together)
  auto deal = [&](std::vector<std::vector<uint64_t>> &runs) {
    std::stable_sort(runs.begin(), runs.end(),
                     [](const std::vector<uint64_t> &a, const std::vector<uint64_t> &b) { return a.size() > b.size(); });
    for (const auto &r : runs) xcd.deal(r);
  };
  if (continuous) {  // the task list in unit order cut into 8 equal runs
    std::vector<uint64_t> all;
    for (const GramUnit &u : units) unit_tasks(u, all);
    const uint64_t run = (all.size() + kXcd - 1) / kXcd;
    for (size_t m = 0; m < all.size(); ++m) xcd.seq[m / run].push_back(all[m]);
  } else if (skip) {
    // An off-diagonal square that lost pairs no longer fills the 64 slots of its XCD: the next
    // unit's first blocks would start beside it and its remaining ones a round later, and sharers
    // of a panel that do not start together miss the L2 together.  Such a
    // square is topped up to 64 with tasks of the split's diagonal squares -- those of its own row
    // or column band first, whose panels it stages anyway -- and what is left of the diagonal
    // squares goes out in runs of 64.
    constexpr size_t kFull = (size_t)kSq * kSq;
    std::vector<std::vector<uint64_t>> runs;
    const int nsq = (nb + kSq - 1) / kSq;
    size_t u0 = 0;
    while (u0 < units.size()) {
      size_t u1 = u0;
      while (u1 < units.size() && units[u1].y == units[u0].y) ++u1;
      std::vector<std::vector<uint64_t>> diag((size_t)nsq);
      for (size_t m = u0; m < u1; ++m)
        if (units[m].bi == units[m].bj) unit_tasks(units[m], diag[(size_t)units[m].bi]);
      for (size_t m = u0; m < u1; ++m) {
        const GramUnit &u = units[m];
        if (u.bi == u.bj) continue;
        std::vector<uint64_t> r;
        unit_tasks(u, r);
        for (int pass = 0; pass < 2 && r.size() < kFull; ++pass)
          for (int sq = 0; sq < nsq && r.size() < kFull; ++sq) {
            if ((pass == 0) != (sq == u.bi || sq == u.bj)) continue;
            std::vector<uint64_t> &pool = diag[(size_t)sq];
            while (!pool.empty() && r.size() < kFull) {
              r.push_back(pool.back());
              pool.pop_back();
            }
          }
        runs.push_back(std::move(r));
      }
      std::vector<uint64_t> rest;
      for (auto &pool : diag) rest.insert(rest.end(), pool.begin(), pool.end());
      for (size_t m = 0; m < rest.size(); m += kFull)
        runs.emplace_back(rest.begin() + m, rest.begin() + std::min(rest.size(), m + kFull));
      u0 = u1;
    }
    deal(runs);
  } else {
    std::vector<std::vector<uint64_t>> runs(units.size());
    for (size_t m = 0; m < units.size(); ++m) unit_tasks(units[m], runs[m]);
    deal(runs);
  }
  tab = xcd.table();
}

// The table of C = A^T Bm over mt x nt output tiles (launch_atb): units of up to 8 x 8 tiles, column-tile
// squares of equal k range together, each dealt to the XCD with the fewest blocks so far.
inline std::vector<uint64_t> atb_rect_table(uint64_t mt, uint64_t nt) {
  XcdDeal xcd;
  for (uint64_t bj = 0; bj * kSq < nt; ++bj)
    for (uint64_t bi = 0; bi * kSq < mt; ++bi) {
      std::vector<uint64_t> run;
      for (uint64_t i = bi * kSq; i < std::min(mt, (bi + 1) * kSq); ++i)
        for (uint64_t j = bj * kSq; j < std::min(nt, (bj + 1) * kSq); ++j) run.push_back(atb_task(i, j, 0));
      xcd.deal(run);
    }
  return xcd.table();
}

// ---- the plan -----------------------------------------------------------------------------------------
struct GramShape {
  int nb = -1;                     // tiles of 128 terms (-1: no shape, an empty cache entry's)
  uint64_t ntiles = 0, slots = 0;  // row tiles of the launch; blocks resident at a time: 2 x CUs
  bool diag4 = false;              // four consecutive diagonal tiles take three blocks (atb_wave_code)
};
// nsplit runs of row tiles that differ by at most one tile; the task list cut into 8 equal runs, or whole units
struct GramPlan { uint64_t nsplit; bool continuous; };
// What the caches of the plan compare, each the parts its value depends on (the others stay as they are
// here): the process-wide choice of the split the shape alone; a mask's dealing (with its GramDedup) the
// shape and the split it is priced at; the uploaded table (with the basis) nb and diag4 of the shape,
// the split, the mask's serial number and the dealing -- not ntiles or slots, which change no task.
struct GramKey {
  GramShape shape;
  uint64_t nsplit = 0;
  uint64_t sig = 0;   // GramDedup::sig of the mask (0: none)
  int dealing = -1;   // 0 whole units, 1 continuous
  auto tied() const { return std::tie(shape.nb, shape.ntiles, shape.slots, shape.diag4, nsplit, sig, dealing); }
  bool operator==(const GramKey &o) const { return tied() == o.tied(); }
  bool operator<(const GramKey &o) const { return tied() < o.tied(); }
};

inline uint64_t gram_npairs(int nb) { return (uint64_t)nb * (uint64_t)(nb + 1) / 2; }
// at most 64 splits, at least 8 row tiles each, and at most 4 GiB of partial tiles
inline uint64_t gram_max_split(const GramShape &s) {
  const uint64_t by_memory = (4ull << 30) / (gram_npairs(s.nb) * kGramTile * kGramTile * 8);
  return std::max<uint64_t>(1, std::min<uint64_t>({64, s.ntiles / 8, by_memory}));
}
// Row split: two blocks per CU at a time and all blocks (nearly) equally long, so the launch
// takes ceil(blocks / slots) rounds of tiles-per-split each; the split that minimises that product is
// picked (528 pairs x 32 splits = 33 x 512 exactly on MI355X).
// (the splits differ by at most one tile and the longer ones are few and dealt out first,
// so a round costs the average length; one tile charged for a block's first chunk, its
// partial-tile store and the hand-over of the slot: ~7 us measured, OBHIP_GRAM_DBG)
// A last round that fills at most half of the slots leaves its blocks alone on their CUs,
// where they run ~1.7x as fast (0.6 of a round); and every split costs k_gram_reduce one
// more partial of every tile pair to read (128 KB at ~4 TB/s = 0.0022 of the 14.6 us a block
// takes per row tile).  Both measured at p = 4096 (16 vs 32 splits at 125 000 rows: equal
// Gram times, half the reduction).
// The rounds are those of the busiest XCD (64 of the slots each, xcd_blocks its blocks): the task table
// hands the XCDs whole units (build_task_order), and when those do not pack into 64 slots -- p = 1024: one
// 34-block unit per split, two of them = 68 -- a whole round is spent on the overhang (measured:
// 2.56 ms where the model without XCDs promised 1.5).  Both dealings are priced, the continuous
// one 3 % dearer for the panels its straddling units fetch twice.
inline double gram_cost(const GramShape &s, uint64_t nsplit, bool continuous, uint64_t xcd_blocks, uint64_t blocks) {
  const uint64_t xslots = s.slots / kXcd;
  const uint64_t full = xcd_blocks / xslots, tail = xcd_blocks % xslots;
  const double rounds = (double)full + (tail == 0 ? 0.0 : (2 * tail <= xslots ? 0.6 : 1.0));
  const double cost = rounds * ((double)s.ntiles / (double)nsplit + 1.0) + 0.0022 * (double)blocks;
  return continuous ? cost * 1.03 : cost;
}
// The split is chosen WITHOUT the skipped pairs, as if every pair had its task: the entries of the
// computed pairs are then the same sums in the same order whether or not others are skipped (bit
// for bit the run with OBHIP_GRAM_DEDUP=0).  Only the dealing to the XCDs, which changes no sum,
// is priced on the tasks that are left (gram_choose_dealing).
inline GramPlan gram_choose_split(const GramShape &s) {
  // blocks per row split: four consecutive diagonal tiles take three blocks
  const uint64_t bps = gram_npairs(s.nb) - (s.diag4 ? (uint64_t)(s.nb / 4) : 0);
  GramPlan best = {1, false};
  double bestc = 1e300;
  for (uint64_t ns = 1, max_split = gram_max_split(s); ns <= max_split; ++ns)
    for (bool continuous : {false, true}) {
      const double cost = gram_cost(s, ns, continuous, gram_xcd_blocks(s.nb, (int)ns, s.diag4, continuous), ns * bps);
      if (cost < bestc - 1e-9) {
        bestc = cost;
        best = {ns, continuous};
      }
    }
  return best;
}
// the dealing for a mask at a split, priced on the table build_task_order deals for the mask (its
// topped-up runs are not the units gram_xcd_blocks models) and on the tasks that are left
inline bool gram_choose_dealing(const GramShape &s, uint64_t nsplit, const uint8_t *skip) {
  auto price = [&](bool continuous) {
    std::vector<uint64_t> tab;
    build_task_order(s.nb, (int)nsplit, s.diag4, continuous, skip, tab);
    const uint64_t blocks = tab.size() - (uint64_t)std::count(tab.begin(), tab.end(), kAtbNoTask);
    return gram_cost(s, nsplit, continuous, tab.size() / kXcd /* the longest XCD sequence */, blocks);
  };
  return price(true) < price(false) - 1e-9;
}

// ---- the plan at wave-tile granularity ----------------------------------------------------------------
// A block's four waves each compute one 64 x 64 wave tile of G from the 256 staged columns [panel I | panel J]:
// any of the four of (I, J), the three of (I, I) and the three of (J, J).  With a keep byte per wave tile of
// the upper triangle of ng = 2 nb column groups (slot pair_slot(ng, a, b), a <= b; 0 = every entry repeats in a
// kept wave tile, gram_dedup.hip) the kept off-diagonal wave tiles stay in the block of their tile pair, the
// diagonal tiles' wave tiles (always kept) fill the waves a partial pair leaves free -- as many as a maximum
// matching places -- and what is left of the diagonal goes to neighbour blocks (i, i + 1), the way types 1-3
// of atb_wave_code pack it.  A wave without a wave tile idles (kWaveIdle): it stages, waits at the barriers
// and stores nothing.  Every kept wave tile is computed exactly once, no dropped one at all.
constexpr uint8_t kWaveIdle = 0xc0;  // the unused value of the output-tile bits
// the byte (atb_wave_code's format) of wave tile (a <= b) in a block that stages panels (I, J)
inline uint8_t wave_byte(int I, int J, int a, int b) {
  const int ta = a / 2, ra = a & 1, cb = b & 1;
  uint32_t A, B, sel;
  if (ta == b / 2) {  // of diagonal tile ta: panel I's groups are 0, 1 and panel J's 2, 3
    sel = ta == I ? 0u : 1u;
    A = 2 * sel + (uint32_t)ra;
    B = 2 * sel + (uint32_t)cb;
  } else {
    sel = 2;
    A = (uint32_t)ra;
    B = 2u + (uint32_t)cb;
  }
  (void)J;
  return (uint8_t)(A | B << 2 | (uint32_t)ra << 4 | (uint32_t)cb << 5 | sel << 6);
}
struct QuadBlock {
  int I, J;
  uint8_t w[4];
  uint32_t bytes() const { return (uint32_t)w[0] | (uint32_t)w[1] << 8 | (uint32_t)w[2] << 16 | (uint32_t)w[3] << 24; }
};
// The blocks of one row split: those of the off-diagonal tile pairs that keep a wave tile, in row-major order
// of the pairs, then the neighbour blocks of the diagonal's rest.
inline void gram_quads_pack(int nb, const uint8_t *keep, std::vector<QuadBlock> &blocks) {
  const int ng = 2 * nb;
  blocks.clear();
  struct Hole { int block, wave; };
  std::vector<Hole> holes;
  for (int I = 0; I < nb; ++I)
    for (int J = I + 1; J < nb; ++J) {
      QuadBlock q = {I, J, {kWaveIdle, kWaveIdle, kWaveIdle, kWaveIdle}};
      int k = 0;
      for (int r = 0; r < 2; ++r)
        for (int c = 0; c < 2; ++c)
          if (keep[pair_slot(ng, 2 * I + r, 2 * J + c)]) q.w[k++] = wave_byte(I, J, 2 * I + r, 2 * J + c);
      if (k == 0) continue;
      for (; k < 4; ++k) holes.push_back({(int)blocks.size(), k});
      blocks.push_back(q);
    }
  // diagonal wave tile u = 3 tile + {0: (lo, lo), 1: (lo, hi), 2: (hi, hi)}; a hole of block (I, J) takes one
  // of I's or J's: maximum bipartite matching by augmenting paths (holes and units by the hundred)
  const int nunits = 3 * nb;
  std::vector<int> hole_of(nunits, -1);
  std::vector<char> seen;
  auto try_hole = [&](auto &&self, int h) -> bool {
    for (int side = 0; side < 2; ++side) {
      const int tile = side ? blocks[holes[h].block].J : blocks[holes[h].block].I;
      for (int u = 3 * tile; u < 3 * tile + 3; ++u) {
        if (seen[u]) continue;
        seen[u] = 1;
        if (hole_of[u] < 0 || self(self, hole_of[u])) {
          hole_of[u] = h;
          return true;
        }
      }
    }
    return false;
  };
  for (int h = 0; h < (int)holes.size(); ++h) {
    seen.assign(nunits, 0);
    try_hole(try_hole, h);
  }
  auto unit_byte = [&](int I, int J, int u) {
    const int tile = u / 3, k = u % 3;
    return wave_byte(I, J, 2 * tile + (k == 2), 2 * tile + (k >= 1));
  };
  std::vector<std::vector<int>> rest(nb);
  for (int u = 0; u < nunits; ++u)
    if (hole_of[u] >= 0) {
      QuadBlock &q = blocks[holes[hole_of[u]].block];
      q.w[holes[hole_of[u]].wave] = unit_byte(q.I, q.J, u);
    } else {
      rest[u / 3].push_back(u);
    }
  // the rest, left to right: all of tile i's and as many of tile i + 1's as still fit
  for (int i = 0; i < nb; ++i) {
    if (rest[i].empty()) continue;
    QuadBlock q = {i + 1 < nb ? i : std::max(i - 1, 0), i + 1 < nb ? i + 1 : i, {kWaveIdle, kWaveIdle, kWaveIdle, kWaveIdle}};
    int k = 0;
    for (int u : rest[i]) q.w[k++] = unit_byte(q.I, q.J, u);
    rest[i].clear();
    if (i + 1 < nb)
      while (k < 4 && !rest[i + 1].empty()) {
        q.w[k++] = unit_byte(q.I, q.J, rest[i + 1].front());
        rest[i + 1].erase(rest[i + 1].begin());
      }
    blocks.push_back(q);
  }
}
// The task table of the packed blocks and, entry for entry, their four wave bytes (whatever at a padding task):
// build_task_order's dealings on the packed list -- units are the 8 x 8 squares by a block's (I, J); an
// off-diagonal square that lost blocks is topped up to 64 from the diagonal squares of its own bands first,
// what is left of those goes out in runs of 64; or the list in unit order cut into 8 equal runs.
inline void gram_quads_table(int nb, int nsplit, bool continuous, const uint8_t *keep, std::vector<uint64_t> &tab,
                             std::vector<uint32_t> &wbytes) {
  std::vector<QuadBlock> blocks;
  gram_quads_pack(nb, keep, blocks);
  const int nsq = (nb + kSq - 1) / kSq;
  // an entry while dealing: block index | split << 32
  std::vector<std::vector<uint64_t>> square((size_t)nsq * nsq);
  for (size_t m = 0; m < blocks.size(); ++m)
  {
    // (a neighbour block (i, i + 1) of the diagonal's rest belongs to the diagonal square of i, also where i + 1 is
    // the first tile of the next square: an off-diagonal square of 65 blocks would shift every later run of its
    // XCD by one slot, and the sharers of a panel would no longer start together)
    const QuadBlock &q = blocks[m];
    const bool rest = (q.w[0] >> 6) != 2;  // no wave tile of (I, J) itself: the off-diagonal blocks put theirs first
    square[(size_t)(q.I / kSq) * nsq + (rest ? q.I : q.J) / kSq].push_back(m);
  }
  XcdDeal xcd;
  constexpr size_t kFull = (size_t)kSq * kSq;
  std::vector<std::vector<uint64_t>> runs;
  std::vector<uint64_t> all;
  for (int y = 0; y < nsplit; ++y) {
    auto of_split = [&](const std::vector<uint64_t> &sq) {
      std::vector<uint64_t> r(sq);
      for (uint64_t &e : r) e |= (uint64_t)y << 32;
      return r;
    };
    if (continuous) {
      for (int bi = 0; bi < nsq; ++bi)
        for (int bj = bi; bj < nsq; ++bj) {
          const std::vector<uint64_t> r = of_split(square[(size_t)bi * nsq + bj]);
          all.insert(all.end(), r.begin(), r.end());
        }
      continue;
    }
    std::vector<std::vector<uint64_t>> diag((size_t)nsq);
    for (int sq = 0; sq < nsq; ++sq) diag[(size_t)sq] = of_split(square[(size_t)sq * nsq + sq]);
    for (int bi = 0; bi < nsq; ++bi)
      for (int bj = bi + 1; bj < nsq; ++bj) {
        std::vector<uint64_t> r = of_split(square[(size_t)bi * nsq + bj]);
        if (r.empty()) continue;
        for (int pass = 0; pass < 2 && r.size() < kFull; ++pass)
          for (int sq = 0; sq < nsq && r.size() < kFull; ++sq) {
            if ((pass == 0) != (sq == bi || sq == bj)) continue;
            std::vector<uint64_t> &pool = diag[(size_t)sq];
            while (!pool.empty() && r.size() < kFull) {
              r.push_back(pool.back());
              pool.pop_back();
            }
          }
        runs.push_back(std::move(r));
      }
    // what is left of the diagonal squares in runs of 64, the fullest squares first: two that lost nothing to
    // the top-up are 60 blocks on 16 panels, where the squares in their order put parts of all four -- 28
    // panels, whose window of 8 chunks no longer fits the L2 -- into one run
    std::stable_sort(diag.begin(), diag.end(),
                     [](const std::vector<uint64_t> &a, const std::vector<uint64_t> &b) { return a.size() > b.size(); });
    // ... and last the smallest square that still holds the whole short run at the end: the short runs of four
    // splits share a round at the tail of an XCD's sequence, 8 panels each instead of parts of two squares
    size_t total = 0;
    for (const auto &pool : diag) total += pool.size();
    for (size_t m = diag.size(); m-- > 0;)
      if (total % kFull != 0 && diag[m].size() >= total % kFull) {
        std::rotate(diag.begin() + (std::ptrdiff_t)m, diag.begin() + (std::ptrdiff_t)m + 1, diag.end());
        break;
      }
    std::vector<uint64_t> rest;
    for (auto &pool : diag) rest.insert(rest.end(), pool.begin(), pool.end());
    for (size_t m = 0; m < rest.size(); m += kFull)
      runs.emplace_back(rest.begin() + m, rest.begin() + std::min(rest.size(), m + kFull));
  }
  if (continuous) {
    const uint64_t run = (all.size() + kXcd - 1) / kXcd;
    for (size_t m = 0; m < all.size(); ++m) xcd.seq[m / run].push_back(all[m]);
  } else {
    std::stable_sort(runs.begin(), runs.end(),
                     [](const std::vector<uint64_t> &a, const std::vector<uint64_t> &b) { return a.size() > b.size(); });
    for (const auto &r : runs) xcd.deal(r);
  }
  tab = xcd.table();
  wbytes.assign(tab.size(), 0);
  for (size_t m = 0; m < tab.size(); ++m) {
    if (tab[m] == kAtbNoTask) continue;
    const QuadBlock &q = blocks[(size_t)(tab[m] & 0xffffffffu)];
    wbytes[m] = q.bytes();
    tab[m] = atb_task((uint64_t)q.I, (uint64_t)q.J, tab[m] >> 32);
  }
}
// what gram_cost says of a task table
inline double gram_table_cost(const GramShape &s, uint64_t nsplit, bool continuous, const std::vector<uint64_t> &tab) {
  const uint64_t blocks = tab.size() - (uint64_t)std::count(tab.begin(), tab.end(), kAtbNoTask);
  return gram_cost(s, nsplit, continuous, tab.size() / kXcd /* the longest XCD sequence */, blocks);
}
// the dealing of the packed blocks at a split, priced like gram_choose_dealing; *cost: that of the choice
inline bool gram_quads_choose_dealing(const GramShape &s, uint64_t nsplit, const uint8_t *keep, double *cost = nullptr) {
  std::vector<uint64_t> tab;
  std::vector<uint32_t> wb;
  double c[2];
  for (int continuous = 0; continuous < 2; ++continuous) {
    gram_quads_table(s.nb, (int)nsplit, continuous != 0, keep, tab, wb);
    c[continuous] = gram_table_cost(s, nsplit, continuous != 0, tab);
  }
  const bool pick = c[1] < c[0] - 1e-9;
  if (cost) *cost = c[pick ? 1 : 0];
  return pick;
}

// ---- row chunks ---------------------------------------------------------------------------------------
// Row tiles per staged chunk when the whole matrix does not fit: a quarter of the free HBM and at most
// 16 GB (forced_rows != 0: that many rows instead, tests), at least one tile, at most all ntiles >= 1; 0 when
// not even that chunk fits into the free memory.
inline uint64_t gram_chunk_tiles(uint64_t free_bytes, uint64_t bytes_per_tile, uint64_t ntiles, uint64_t forced_rows) {
  const uint64_t fit = std::min<uint64_t>(free_bytes / 4, 16ull << 30) / bytes_per_tile;
  const uint64_t ctiles = std::min(std::max<uint64_t>(forced_rows ? forced_rows / kGramRowTile : fit, 1), ntiles);
  return ctiles * bytes_per_tile > free_bytes ? 0 : ctiles;
}

}  // namespace obhip
