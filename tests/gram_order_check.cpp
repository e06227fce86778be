// Stand-alone host check of csrc/gram_order.h (and of gram_plan.h's packing on its mask), no GPU.  Compiled by
// tests/test_gram_order_host.py with g++ under the address and undefined-behaviour sanitizers and run as a
// program of its own:
//
//   gram_order_check LEVELS [MIN_DROPPED MAX_BLOCKS]
//
// LEVELS: a text file "p d" followed by the p x d levels of a term set in the caller's order.  Checked, with a
// message on stderr and exit status 1 at the first failure:
//   - perm is a stable sort by the number of factors and inv its inverse;
//   - the sequential pass on the levels in Gram order drops at least MIN_DROPPED wave tiles (default 0);
//   - every entry of a dropped wave tile has a source, in a kept wave tile, of the same unordered level pairs;
//   - no wave tile kept by rule is dropped;
//   - gram_quads_pack on that mask gives at most MAX_BLOCKS blocks (default: no bound) and never fewer than
//     ceil(kept / 4);
//   - for p = 4096 (the headline): the engagement rule says yes at 15 625 row tiles against the wave-tile plan of
//     the terms' own order, and no at 64.
// stdout: "identity 0|1", "dropped N", "blocks M", "as_given_parallel N", "mask <one character per wave tile, row-major in the upper triangle, 1 = dropped>",
// "as_given_mask <the same for the parallel rule in the terms' own order>", "engage_headline 0|1", "engage_64 0|1".
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../outerbase_amd/csrc/gram_order.h"

using namespace obhip;

#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
      return 1;                     \
    }                               \
  } while (0)

static int count_dropped(const std::vector<uint8_t> &keep) { return (int)std::count(keep.begin(), keep.end(), (uint8_t)0); }

static std::string mask_string(const std::vector<uint8_t> &keep) {
  std::string m;
  for (uint8_t k : keep) m.push_back(k ? '0' : '1');
  return m;
}

constexpr double kBlockTileMs = 0.0146;  // gram_dedup.hip's

// the decision of gram_order_get at a launch of ntiles row tiles on 512 slots: `other` the wave-tile mask the
// launch would otherwise pack (null: every tile pair whole, the dearest the competing plan can be)
static bool decide(int nb, uint64_t ntiles, const std::vector<uint8_t> *other, const std::vector<uint8_t> &ordered) {
  const GramShape shape = {nb, ntiles, 512, true};
  const GramPlan plan = gram_choose_split(shape);
  double cost_other = 0.0, cost = 0.0;
  int blocks_other = 0;
  std::vector<QuadBlock> blocks;
  if (other) {
    gram_quads_choose_dealing(shape, plan.nsplit, other->data(), &cost_other);
    gram_quads_pack(nb, other->data(), blocks);
    blocks_other = (int)blocks.size();
  } else {
    std::vector<uint64_t> tab;
    build_task_order(nb, (int)plan.nsplit, true, plan.continuous, nullptr, tab);
    cost_other = gram_table_cost(shape, plan.nsplit, plan.continuous, tab);
    blocks_other = (int)((tab.size() - (size_t)std::count(tab.begin(), tab.end(), kAtbNoTask)) / plan.nsplit);
  }
  if (!gram_order_worth_analysing(nb, cost_other, kBlockTileMs)) return false;
  gram_quads_choose_dealing(shape, plan.nsplit, ordered.data(), &cost);
  gram_quads_pack(nb, ordered.data(), blocks);
  return gram_order_pays(nb, cost_other, blocks_other, cost, (int)blocks.size(), kBlockTileMs);
}

int main(int argc, char **argv) {
  CHECK(argc >= 2, "usage: gram_order_check LEVELS [MIN_DROPPED MAX_BLOCKS]");
  const int min_dropped = argc >= 3 ? atoi(argv[2]) : 0;
  const int max_blocks = argc >= 4 ? atoi(argv[3]) : -1;
  FILE *f = fopen(argv[1], "r");
  CHECK(f, "cannot open %s", argv[1]);
  unsigned long long p = 0, d = 0;
  CHECK(fscanf(f, "%llu %llu", &p, &d) == 2 && p > 0 && d > 0 && p < 65536, "bad header");
  std::vector<uint32_t> lev(p * d);
  for (uint32_t &v : lev) CHECK(fscanf(f, "%u", &v) == 1, "short level table");
  fclose(f);

  // the permutation
  const std::vector<uint32_t> perm = gram_order_perm(lev.data(), p, d), inv = gram_perm_inverse(perm);
  CHECK(perm.size() == p && inv.size() == p, "perm has the wrong length");
  auto factors = [&](uint32_t k) {
    int nf = 0;
    for (uint64_t j = 0; j < d; ++j) nf += lev[k * d + j] != 0;
    return nf;
  };
  std::vector<char> seen(p, 0);
  for (uint64_t k = 0; k < p; ++k) {
    CHECK(perm[k] < p && !seen[perm[k]], "perm is no permutation at %llu", (unsigned long long)k);
    seen[perm[k]] = 1;
    CHECK(inv[perm[k]] == k, "inv is not the inverse at %llu", (unsigned long long)k);
    if (k > 0) {
      const int f0 = factors(perm[k - 1]), f1 = factors(perm[k]);
      CHECK(f0 < f1 || (f0 == f1 && perm[k - 1] < perm[k]), "perm is no stable factor-count sort at %llu", (unsigned long long)k);
    }
  }
  const bool identity = gram_perm_is_identity(perm);
  printf("identity %d\n", identity ? 1 : 0);

  // the sequential pass in Gram order
  const std::vector<uint32_t> glev = gram_perm_levels(lev.data(), d, perm);
  for (uint64_t k = 0; k < p; ++k)
    for (uint64_t j = 0; j < d; ++j) CHECK(glev[k * d + j] == lev[perm[k] * d + j], "permuted level table");
  const int nb = (int)((p + kGramTile - 1) / kGramTile), ng = 2 * nb;
  std::vector<uint8_t> keep;
  std::vector<uint32_t> dropped, src;
  gram_seq_pass(glev.data(), p, d, false, keep, &dropped, &src);
  CHECK(keep.size() == gram_npairs(ng), "one keep byte per wave tile");
  CHECK((int)dropped.size() == count_dropped(keep) && src.size() == dropped.size() * 64 * 64, "dropped list and sources");
  CHECK((int)dropped.size() >= min_dropped, "the sequential pass drops %d wave tiles, fewer than %d", (int)dropped.size(),
        min_dropped);
  for (size_t m = 0; m < dropped.size(); ++m) {
    const int a = (int)(dropped[m] & 0xffffu), b = (int)(dropped[m] >> 16);
    CHECK(a < b && b < ng && a / 2 != b / 2 && (uint64_t)(b + 1) * 64 <= p, "wave tile (%d, %d) is kept by rule", a, b);
    for (uint32_t w = 0; w < 64 * 64; ++w) {
      const uint32_t s = (uint32_t)a * 64 + w / 64, t = (uint32_t)b * 64 + w % 64, q = src[m * 64 * 64 + w];
      CHECK(q != ~0u, "entry (%u, %u) has no source", s, t);
      const uint32_t ss = q >> 16, st = q & 0xffffu;
      CHECK(ss < st && st < p, "source (%u, %u) of (%u, %u)", ss, st, s, t);
      CHECK(keep[(size_t)pair_slot(ng, (int)(ss / 64), (int)(st / 64))], "source (%u, %u) lies in a dropped wave tile", ss, st);
      for (uint64_t j = 0; j < d; ++j) {
        const uint32_t x = glev[s * d + j], y = glev[t * d + j], x2 = glev[ss * d + j], y2 = glev[st * d + j];
        CHECK(std::min(x, y) == std::min(x2, y2) && std::max(x, y) == std::max(x2, y2),
              "source (%u, %u) of (%u, %u) differs in dimension %llu", ss, st, s, t, (unsigned long long)j);
      }
    }
  }
  printf("dropped %d\n", (int)dropped.size());

  // its packing
  std::vector<QuadBlock> blocks;
  gram_quads_pack(nb, keep.data(), blocks);
  const int kept = (int)keep.size() - (int)dropped.size();
  CHECK((int)blocks.size() >= (kept + 3) / 4, "%d blocks for %d kept wave tiles", (int)blocks.size(), kept);
  CHECK(max_blocks < 0 || (int)blocks.size() <= max_blocks, "%d blocks per split, more than %d", (int)blocks.size(), max_blocks);
  printf("blocks %d\n", (int)blocks.size());

  // the plan it competes with: the parallel rule in the terms' own order
  std::vector<uint8_t> given_par;
  gram_seq_pass(lev.data(), p, d, true, given_par);
  printf("as_given_parallel %d\n", count_dropped(given_par));
  printf("mask %s\nas_given_mask %s\n", mask_string(keep).c_str(), mask_string(given_par).c_str());

  // the engagement rule
  if (p == 4096) {
    const bool yes = decide(nb, 15625, &given_par, keep), no = decide(nb, 64, nullptr, keep);
    printf("engage_headline %d\nengage_64 %d\n", yes ? 1 : 0, no ? 1 : 0);
    CHECK(yes, "the order does not engage at 15 625 row tiles");
    CHECK(!no, "the order engages at 64 row tiles");
  }
  return 0;
}
