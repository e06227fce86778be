// Stand-alone check of csrc/conditional_plan.h for tests/test_conditional_host.py: walks every case itself, prints one
// line per failed property and "ok <cases>" at the end; the exit status is the number of failures (at most 1).
//   grouping   random and structured level matrices (p in {1, 2, 15, 16, 17, 129, 300}, d in {2, 3, 8, 40}, every
//              size of E from 1 to d - 1 that the case list names) against a std::map keyed by the level tuple:
//              groups numbered in the order of their first term, group_of, first, the offsets and the order (terms by
//              group, ascending within a group, a permutation); all terms alike (G = 1) and all different (G = p)
//   chunks     n in {0, 1, 127, 128, 129, 200, 8192, 8193, 10^5} x chunk_rows in {0, 128, 256, 8192}: the chunks
//              cover the rows once, in order, each at most cmax rows and padded to 128; the workspace counts two
//              blocks of q Gp npad doubles, the moments and the padded tables, carved consecutively on 128-byte
//              boundaries (the offsets conditional.cpp allocates by)
//   edges      the default chunk keeps a block within 2^28 bytes or is one 128-row chunk; the largest sizes that
//              are let through (q = 65535, G = 16384, chunk_rows = 2^28) do not overflow 64 bits
//   refusals   dims_e null, empty, all d dimensions, unsorted, repeated, out of range; p = 0, p > 2^24, d = 0,
//              d > 255, q = 0, q > 65535, n > 2^40, chunk_rows not a multiple of 128 or above 2^28
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <vector>

#include "../outerbase_amd/csrc/conditional_plan.h"

using namespace obhip;

static int failures = 0;
static long cases = 0;

#define CHECK(cond, ...)           \
  do {                             \
    ++cases;                       \
    if (!(cond)) {                 \
      ++failures;                  \
      printf("FAIL " __VA_ARGS__); \
      printf("\n");                \
    }                              \
  } while (0)

typedef unsigned long long ull;

static void check_grouping(const std::vector<uint32_t> &lev, uint64_t p, uint64_t d, const std::vector<uint32_t> &de,
                           const char *what) {
  const CondGroups g = cond_groups(lev.data(), p, d, de.data(), de.size());
  std::map<std::vector<uint32_t>, uint32_t> ids;
  std::vector<uint32_t> want(p), first;
  for (uint64_t k = 0; k < p; ++k) {
    std::vector<uint32_t> key;
    for (uint32_t l : de) key.push_back(lev[k * d + l]);
    auto it = ids.find(key);
    if (it == ids.end()) {
      it = ids.emplace(key, (uint32_t)ids.size()).first;
      first.push_back((uint32_t)k);
    }
    want[k] = it->second;
  }
  CHECK(g.G == ids.size(), "G %s p=%llu d=%llu", what, (ull)p, (ull)d);
  CHECK(g.group_of == want, "group_of %s p=%llu d=%llu", what, (ull)p, (ull)d);
  CHECK(g.first == first, "first %s p=%llu d=%llu", what, (ull)p, (ull)d);
  CHECK(g.off.size() == g.G + 1 && g.off[0] == 0 && g.off[g.G] == p && g.order.size() == p, "offsets %s p=%llu", what,
        (ull)p);
  std::vector<int> seen(p, 0);
  bool ok = true;
  for (uint64_t gi = 0; gi < g.G && ok; ++gi) {
    ok = g.off[gi] < g.off[gi + 1] && g.order[g.off[gi]] == g.first[gi];
    for (uint64_t e = g.off[gi]; e < g.off[gi + 1] && ok; ++e) {
      const uint32_t k = g.order[e];
      ok = k < p && !seen[k] && want[k] == gi && (e == g.off[gi] || g.order[e - 1] < k);
      if (ok) seen[k] = 1;
    }
  }
  CHECK(ok, "order %s p=%llu d=%llu", what, (ull)p, (ull)d);
}

static void check_chunks(uint64_t G, uint64_t q, uint64_t n, uint64_t chunk_rows) {
  const CondPlan pl = cond_plan(G, q, n, chunk_rows);
  CHECK(pl.cmax % 128 == 0 && pl.cmax >= 128 && (chunk_rows == 0 || pl.cmax == chunk_rows), "cmax n=%llu c=%llu", (ull)n,
        (ull)chunk_rows);
  CHECK(pl.Gp() % 16 == 0 && pl.Gp() >= G && pl.Gp() < G + 16, "Gp G=%llu", (ull)G);
  if (chunk_rows == 0)
    CHECK(pl.cmax == 128 || q * pl.Gp() * pl.cmax * 8 <= kCondCapBytes, "cap G=%llu q=%llu", (ull)G, (ull)q);
  const RowChunks rc = pl.chunks();
  uint64_t next = 0, biggest = 0;
  for (uint64_t c = 0; c < rc.count(); ++c) {
    const RowChunk ch = rc.at(c);
    CHECK(ch.r0 == next && ch.nr >= 1 && ch.nr <= pl.cmax && ch.npad == pad128(ch.nr) && ch.npad <= pl.chunk_rows_max(),
          "chunk n=%llu c=%llu i=%llu", (ull)n, (ull)chunk_rows, (ull)c);
    CHECK(ch.whole == (rc.count() == 1), "whole n=%llu c=%llu", (ull)n, (ull)chunk_rows);
    next += ch.nr;
    biggest = ch.npad > biggest ? ch.npad : biggest;
  }
  CHECK(next == n && (n == 0) == (rc.count() == 0), "cover n=%llu c=%llu", (ull)n, (ull)chunk_rows);
  CHECK(n == 0 || biggest == pl.chunk_rows_max(), "largest n=%llu c=%llu", (ull)n, (ull)chunk_rows);
  const uint64_t cr = pl.chunk_rows_max();
  CHECK(pl.block_doubles() == q * pl.Gp() * cr &&
            pl.workspace_bytes() == 8 * (2 * q * pl.Gp() * cr + 2 * q * cr + pl.Gp() + pl.Gp() * pl.Gp()),
        "workspace G=%llu q=%llu n=%llu", (ull)G, (ull)q, (ull)n);
  // the carving conditional.cpp allocates by: consecutive, nothing shared, every block on a 128-byte boundary
  CHECK(pl.off_mE() == 0 && pl.off_K() == pl.Gp() && pl.off_C() == pl.off_K() + pl.Gp() * pl.Gp() &&
            pl.off_Y() == pl.off_C() + pl.block_doubles() && pl.off_M() == pl.off_Y() + pl.block_doubles() &&
            pl.off_W() == pl.off_M() + q * cr && pl.workspace_doubles() == pl.off_W() + q * cr &&
            pl.workspace_bytes() == 8 * pl.workspace_doubles(),
        "carving G=%llu q=%llu n=%llu", (ull)G, (ull)q, (ull)n);
  CHECK(pl.off_K() % 16 == 0 && pl.off_C() % 16 == 0 && pl.off_Y() % 16 == 0 && pl.off_M() % 16 == 0 &&
            pl.off_W() % 16 == 0, "alignment G=%llu q=%llu n=%llu", (ull)G, (ull)q, (ull)n);
}

int main() {
  std::mt19937 rng(12345);
  const uint64_t ps[] = {1, 2, 15, 16, 17, 129, 300};
  const uint64_t ds[] = {2, 3, 8, 40};
  for (uint64_t p : ps)
    for (uint64_t d : ds) {
      std::vector<uint32_t> lev(p * d);
      for (uint32_t maxlev : {1u, 3u, 255u}) {
        for (auto &v : lev) v = rng() % (maxlev + 1);
        std::vector<std::vector<uint32_t>> sets = {{0}, {(uint32_t)d - 1}};
        if (d > 2) {
          std::vector<uint32_t> inter, allbut;
          for (uint32_t l = 0; l < d; l += 2) inter.push_back(l);
          if (inter.size() == d) inter.pop_back();
          for (uint32_t l = 1; l < d; ++l) allbut.push_back(l);
          sets.push_back(inter);
          sets.push_back(allbut);
        }
        for (const auto &de : sets) {
          CHECK(cond_dims_refusal(de.data(), de.size(), d) == nullptr, "dims let through d=%llu", (ull)d);
          check_grouping(lev, p, d, de, "random");
        }
      }
      // all alike on E, all different on E
      std::vector<uint32_t> de = {0};
      for (uint64_t k = 0; k < p; ++k) lev[k * d] = 2;
      check_grouping(lev, p, d, de, "alike");
      for (uint64_t k = 0; k < p; ++k) lev[k * d] = (uint32_t)(p - 1 - k);
      check_grouping(lev, p, d, de, "different");
    }

  const uint64_t ns[] = {0, 1, 127, 128, 129, 200, 8192, 8193, 100000};
  const uint64_t crs[] = {0, 128, 256, 8192};
  for (uint64_t n : ns)
    for (uint64_t cr : crs)
      for (uint64_t G : {1ull, 15ull, 16ull, 17ull, 129ull, 4096ull})
        for (uint64_t q : {1ull, 3ull, 16ull}) {
          CHECK(cond_sizes_refusal(300, 8, q, n, cr) == nullptr, "sizes let through n=%llu", (ull)n);
          check_chunks(G, q, n, cr);
        }
  // the largest sizes that are let through: no product overflows 64 bits
  {
    CHECK(cond_sizes_refusal(kCondMaxP, 255, kCondMaxQ, kCondMaxRows, kCondMaxChunkRows) == nullptr, "largest sizes");
    const CondPlan pl = cond_plan(kCondMaxGroups, kCondMaxQ, kCondMaxRows, kCondMaxChunkRows);
    const long double exact = 8.0L * (2.0L * kCondMaxQ * kCondMaxGroups * kCondMaxChunkRows +
                                      2.0L * kCondMaxQ * kCondMaxChunkRows + kCondMaxGroups +
                                      (long double)kCondMaxGroups * kCondMaxGroups);
    CHECK(exact < 18446744073709551615.0L && (long double)pl.workspace_bytes() == exact, "no overflow at the limits");
    const CondPlan dflt = cond_plan(kCondMaxGroups, kCondMaxQ, kCondMaxRows, 0);
    CHECK(dflt.cmax == 128, "default chunk at the largest q G");
    CHECK(cond_plan(1, 1, 1, 0).cmax == kCondCapBytes / (16 * 8), "default chunk at the smallest q G: 2^28 bytes of 16 groups");
  }
  // refusals
  {
    const uint32_t ok[] = {0, 2}, unsorted[] = {2, 0}, twice[] = {1, 1}, far[] = {0, 3}, all[] = {0, 1, 2};
    CHECK(cond_dims_refusal(ok, 2, 3) == nullptr, "dims ok");
    CHECK(cond_dims_refusal(nullptr, 1, 3) != nullptr, "dims null");
    CHECK(cond_dims_refusal(ok, 0, 3) != nullptr, "dims empty");
    CHECK(cond_dims_refusal(all, 3, 3) != nullptr, "dims all");
    CHECK(cond_dims_refusal(unsorted, 2, 3) != nullptr, "dims unsorted");
    CHECK(cond_dims_refusal(twice, 2, 3) != nullptr, "dims repeated");
    CHECK(cond_dims_refusal(far, 2, 3) != nullptr, "dims out of range");
    CHECK(cond_dims_refusal(ok, 1, 1) != nullptr, "d = 1 has no split");
    CHECK(cond_sizes_refusal(0, 3, 1, 1, 0) != nullptr, "p = 0");
    CHECK(cond_sizes_refusal(kCondMaxP + 1, 3, 1, 1, 0) != nullptr, "p > 2^24");
    CHECK(cond_sizes_refusal(8, 0, 1, 1, 0) != nullptr, "d = 0");
    CHECK(cond_sizes_refusal(8, 256, 1, 1, 0) != nullptr, "d > 255");
    CHECK(cond_sizes_refusal(8, 3, 0, 1, 0) != nullptr, "q = 0");
    CHECK(cond_sizes_refusal(8, 3, 65536, 1, 0) != nullptr, "q > 65535");
    CHECK(cond_sizes_refusal(8, 3, 1, kCondMaxRows + 1, 0) != nullptr, "n > 2^40");
    CHECK(cond_sizes_refusal(8, 3, 1, 1, 100) != nullptr, "chunk_rows 100");
    CHECK(cond_sizes_refusal(8, 3, 1, 1, 64) != nullptr, "chunk_rows 64");
    CHECK(cond_sizes_refusal(8, 3, 1, 1, kCondMaxChunkRows + 128) != nullptr, "chunk_rows above 2^28");
    CHECK(cond_sizes_refusal(8, 3, 1, 0, 128) == nullptr, "n = 0 is not refused");
  }
  if (failures == 0) printf("ok %ld\n", cases);
  return failures ? 1 : 0;
}
