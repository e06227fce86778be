// Stand-alone check of csrc/term_path_plan.h for tests/test_term_path_host.py: walks every case itself, prints one
// line per failed property and "ok <cases>" at the end; the exit status is the number of failures (at most 1).
//   checkpoints  p in {1, 15, 16, 17, 127, 128, 129, 385, 4096, 65535} x step in {1, 7, 16, 129, 1000, 2^63, 2^64 - 1}:
//                K = ceil(p / step) (1 for step >= p), k_c = min((c + 1) step, p) strictly ascending and ending at
//                p, and the kernel's walk (next_checkpoint from 0) visits exactly k_0 .. k_{K-1} without overflow
//   layout       the (checkpoint, response, score) and sumv entries of one set of sums are a bijection onto
//                [0, K (3 q + 1)), scores first
//   tiles        n in {0, 1, 127, 128, 129, 300, 8192, 8193, 10^5}: tiles and groups cover the rows, a group is 64
//                tiles, and walking the tiles chunk after chunk (chunk_rows 128, 256, 8192, the default) gives every
//                tile the same group as the unchunked walk does: what makes the sums independent of the chunking
//   sizes        the default chunk keeps Z within 1 GiB (32768 rows at pp = 4096), scratch_bytes counts Z, the
//                chunk's tile sums and the group sums; the response block fits the staging sweep
//   refusals     p = 0, p > 65535, q = 0, q > 65534, step = 0, n > 2^40, chunk_rows not a multiple of 128 or above
//                2^30; and the cases above are not refused
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../outerbase_amd/csrc/term_path_plan.h"

using namespace obhip;

static int failures = 0;
static long cases = 0;

#define CHECK(cond, ...)          \
  do {                            \
    ++cases;                      \
    if (!(cond)) {                \
      ++failures;                 \
      printf("FAIL " __VA_ARGS__); \
      printf("\n");               \
    }                             \
  } while (0)

typedef unsigned long long ull;

static void check_checkpoints(uint64_t p, uint64_t step) {
  const TermPathPlan t = term_path_plan(p, 3, step, 0, 0);
  const uint64_t K = t.K();
  const uint64_t want = step >= p ? 1 : (p / step + (p % step ? 1 : 0));
  CHECK(K == want && K >= 1, "K p=%llu step=%llu", (ull)p, (ull)step);
  uint64_t prev = 0, walk = 0;
  for (uint64_t c = 0; c < K; ++c) {
    const uint64_t k = t.checkpoint(c);
    const uint64_t direct = (c + 1 < K) ? (c + 1) * step : p;  // min((c + 1) step, p) without overflow
    CHECK(k == direct && k > prev && k <= p, "checkpoint p=%llu step=%llu c=%llu", (ull)p, (ull)step, (ull)c);
    walk = t.next_checkpoint(walk);
    CHECK(walk == k, "walk p=%llu step=%llu c=%llu", (ull)p, (ull)step, (ull)c);
    CHECK((k - 1) / step == c || (k == p && c == K - 1), "index p=%llu step=%llu c=%llu", (ull)p, (ull)step, (ull)c);
    prev = k;
  }
  CHECK(prev == p, "last checkpoint p=%llu step=%llu", (ull)p, (ull)step);
}

static void check_layout(uint64_t p, uint64_t q, uint64_t step) {
  const TermPathPlan t = term_path_plan(p, q, step, 0, 0);
  const uint64_t K = t.K(), E = t.entries();
  CHECK(E == K * (3 * q + 1) && t.score_entries() == 3 * K * q, "entries p=%llu q=%llu", (ull)p, (ull)q);
  std::vector<int> seen(E, 0);
  for (uint64_t c = 0; c < K; ++c) {
    for (uint64_t j = 0; j < q; ++j)
      for (uint64_t s = 0; s < 3; ++s) {
        const uint64_t e = t.score_at(c, j, s);
        CHECK(e < t.score_entries(), "score entry out of range");
        if (e < E) ++seen[e];
      }
    const uint64_t e = t.sumv_at(c);
    CHECK(e >= t.score_entries() && e < E, "sumv entry out of range");
    if (e < E) ++seen[e];
  }
  bool once = true;
  for (int v : seen) once = once && v == 1;
  CHECK(once, "layout is no bijection p=%llu q=%llu step=%llu", (ull)p, (ull)q, (ull)step);
  CHECK(t.passes() == (q + kTpRespBlock - 1) / kTpRespBlock && t.passes() * kTpRespBlock >= q, "passes q=%llu", (ull)q);
}

static void check_tiles(uint64_t p, uint64_t n, uint64_t chunk_rows) {
  const TermPathPlan t = term_path_plan(p, 2, 16, n, chunk_rows);
  CHECK(t.cmax % 128 == 0 && t.cmax >= 128, "cmax p=%llu chunk_rows=%llu", (ull)p, (ull)chunk_rows);
  if (chunk_rows) CHECK(t.cmax == chunk_rows, "cmax given outright");
  CHECK(t.tiles() * kTpTileRows >= n && (n == 0 ? t.tiles() == 0 : (t.tiles() - 1) * kTpTileRows < n), "tiles n=%llu", (ull)n);
  CHECK(t.groups() * kTpGroup >= t.tiles() && (t.tiles() == 0 ? t.groups() == 0 : (t.groups() - 1) * kTpGroup < t.tiles()),
        "groups n=%llu", (ull)n);
  // the walk of term_path.cpp: chunk after chunk, a chunk's local tile lt is tile r0 / 128 + lt of the call
  const RowChunks chunks{n, t.cmax};
  uint64_t next_tile = 0;
  for (uint64_t c = 0; n && c < chunks.count(); ++c) {
    const RowChunk ch = chunks.at(c);
    CHECK(ch.r0 % kTpTileRows == 0, "a chunk starts inside a tile n=%llu cmax=%llu", (ull)n, (ull)t.cmax);
    const uint64_t tile0 = ch.r0 / kTpTileRows, ctiles = ch.npad / kTpTileRows;
    CHECK(tile0 == next_tile, "tiles out of order n=%llu cmax=%llu", (ull)n, (ull)t.cmax);
    CHECK(ch.npad <= t.chunk_rows_max(), "chunk above chunk_rows_max n=%llu cmax=%llu", (ull)n, (ull)t.cmax);
    for (uint64_t lt = 0; lt < ctiles; ++lt) {
      const uint64_t T = tile0 + lt;
      CHECK(T < t.tiles() && T / kTpGroup < t.groups(), "tile beyond the call n=%llu", (ull)n);
      CHECK(T * kTpTileRows < ch.r0 + ch.nr, "a tile without a row n=%llu", (ull)n);
    }
    next_tile = tile0 + ctiles;
  }
  CHECK(next_tile == t.tiles(), "the chunks' tiles end at %llu of %llu", (ull)next_tile, (ull)t.tiles());
  const uint64_t cr = t.chunk_rows_max();
  CHECK(t.scratch_bytes() == 8 * (cr * t.pp() + (cr / 128) * t.entries() + t.groups() * t.entries()), "scratch n=%llu", (ull)n);
  if (!chunk_rows && t.cmax > 128) CHECK(t.cmax * t.pp() * 8 <= kTpZCapBytes, "Z over its cap p=%llu", (ull)p);
}

static void check_refusals() {
  CHECK(term_path_refusal(0, 1, 1, 0, 0), "p = 0");
  CHECK(term_path_refusal(65536, 1, 1, 0, 0), "p = 65536");
  CHECK(term_path_refusal(8, 0, 1, 0, 0), "q = 0");
  CHECK(term_path_refusal(8, 65535, 1, 0, 0), "q = 65535");
  CHECK(term_path_refusal(8, 1, 0, 0, 0), "step = 0");
  CHECK(term_path_refusal(8, 1, 1, (1ull << 40) + 1, 0), "n > 2^40");
  CHECK(term_path_refusal(8, 1, 1, 10, 100), "chunk_rows = 100");
  CHECK(term_path_refusal(8, 1, 1, 10, 129), "chunk_rows = 129");
  CHECK(term_path_refusal(8, 1, 1, 10, (1ull << 30) + 128), "chunk_rows above 2^30");
  CHECK(!term_path_refusal(1, 1, 1, 0, 0), "smallest case refused");
  CHECK(!term_path_refusal(65535, 65534, ~0ull, 1ull << 40, 1ull << 30), "largest case refused");
  CHECK(!term_path_refusal(385, 3, 16, 300, 128), "plain case refused");
}

int main() {
  static_assert(kTpTileRows == 128 && kTpGroup == 64 && kTpPitch % 2 == 1, "sizes the documents state");
  const uint64_t ps[] = {1, 15, 16, 17, 127, 128, 129, 385, 4096, 65535};
  const uint64_t steps[] = {1, 7, 16, 129, 1000, 1ull << 63, ~0ull};
  for (uint64_t p : ps)
    for (uint64_t step : steps) {
      if (p / step > 5000) continue;  // (K in the tens of thousands: the same arithmetic, seconds under the sanitizers)
      check_checkpoints(p, step);
      for (uint64_t q : {1ull, 3ull, 4ull, 5ull, 9ull}) check_layout(p, q, step);
    }
  check_checkpoints(65535, 16);
  for (uint64_t p : {1ull, 129ull, 385ull, 4096ull, 65535ull})
    for (uint64_t n : {0ull, 1ull, 127ull, 128ull, 129ull, 300ull, 8192ull, 8193ull, 100000ull})
      for (uint64_t chunk_rows : {0ull, 128ull, 256ull, 8192ull}) check_tiles(p, n, chunk_rows);
  CHECK(term_path_plan(4096, 1, 16, 100000, 0).cmax == 32768, "default chunk at pp = 4096");
  CHECK(term_path_plan(4096, 16, 16, 100000, 0).K() == 256, "K at p = 4096, step 16");
  check_refusals();
  printf("ok %ld\n", cases);
  return failures ? 1 : 0;
}
