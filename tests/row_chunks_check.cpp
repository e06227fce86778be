// Stand-alone check of the arithmetic part of csrc/row_chunks.h for tests/test_row_chunks_host.py: walks every case
// itself, prints one line per failed property and "ok <cases>" at the end; the exit status is the number of failures
// (at most 1).
//   sizes:  chunk_rows_for at the caps the three callers use: the values that the formula max(128, (cap / (pp 8)) /
//           128 * 128) gives, worked out by hand
//   plans:  pp in {128, 256, 4096, 16384, 65536} x caps 1 GiB and 8 GiB, and cmax = 128, 256 given outright;
//           n in {1, 127, 128, 129, 300, cmax - 1, cmax, cmax + 1, 3 cmax + 44}: the chunks tile [0, n) in ascending
//           order without gap or overlap, all but the last have cmax rows, npad = pad128(nr) >= nr, whole exactly for
//           the one chunk that is the call, and a block of pp x npad doubles stays within the cap whenever cmax > 128
#include <cstdint>
#include <cstdio>

#include "../outerbase_amd/csrc/row_chunks.h"

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
static const uint64_t kGiB = 1ull << 30;

static void check_sizes() {
  CHECK(obhip::chunk_rows_for(128, kGiB) == 1048576, "chunk_rows_for(128, 1 GiB)");
  CHECK(obhip::chunk_rows_for(4096, kGiB) == 32768, "chunk_rows_for(4096, 1 GiB)");
  CHECK(obhip::chunk_rows_for(65536, kGiB) == 2048, "chunk_rows_for(65536, 1 GiB)");
  CHECK(obhip::chunk_rows_for(16384, 8 * kGiB) == 65536, "chunk_rows_for(16384, 8 GiB)");
  // the quotient falls below 128: 1 GiB / (2^21 * 8) = 64, 8 GiB / (2^24 * 8) = 64, and nothing at all
  CHECK(obhip::chunk_rows_for(1ull << 21, kGiB) == 128, "chunk_rows_for(2^21, 1 GiB)");
  CHECK(obhip::chunk_rows_for(1ull << 24, 8 * kGiB) == 128, "chunk_rows_for(2^24, 8 GiB)");
  CHECK(obhip::chunk_rows_for(1ull << 40, kGiB) == 128, "chunk_rows_for(2^40, 1 GiB)");
  for (uint64_t v : {0ull, 1ull, 127ull, 128ull, 129ull, 300ull})
    CHECK(obhip::pad128(v) % 128 == 0 && obhip::pad128(v) >= v && obhip::pad128(v) < v + 128, "pad128(%llu)", (ull)v);
}

// cap = 0: cmax was given outright, no block bound to hold
static void check_plan(uint64_t n, uint64_t cmax, uint64_t pp, uint64_t cap) {
  const obhip::RowChunks plan{n, cmax};
  const uint64_t count = plan.count();
  CHECK(count == (n + cmax - 1) / cmax && count >= 1, "count n=%llu cmax=%llu", (ull)n, (ull)cmax);
  uint64_t next = 0;
  for (uint64_t c = 0; c < count; ++c) {
    const obhip::RowChunk ch = plan.at(c);
    CHECK(ch.r0 == next, "gap or overlap n=%llu cmax=%llu chunk %llu", (ull)n, (ull)cmax, (ull)c);
    CHECK(ch.nr >= 1 && ch.nr <= cmax && ch.r0 + ch.nr <= n, "rows n=%llu cmax=%llu chunk %llu", (ull)n, (ull)cmax, (ull)c);
    if (c + 1 < count) CHECK(ch.nr == cmax, "short inner chunk n=%llu cmax=%llu chunk %llu", (ull)n, (ull)cmax, (ull)c);
    CHECK(ch.npad == obhip::pad128(ch.nr) && ch.npad >= ch.nr, "npad n=%llu cmax=%llu chunk %llu", (ull)n, (ull)cmax, (ull)c);
    CHECK(ch.whole == (count == 1), "whole n=%llu cmax=%llu chunk %llu", (ull)n, (ull)cmax, (ull)c);
    if (cap && cmax > 128)
      CHECK(pp * ch.npad * 8 <= cap, "block over the cap n=%llu cmax=%llu pp=%llu", (ull)n, (ull)cmax, (ull)pp);
    next = ch.r0 + ch.nr;
  }
  CHECK(next == n, "the chunks end at %llu, n=%llu cmax=%llu", (ull)next, (ull)n, (ull)cmax);
}

static void check_sizes_of(uint64_t cmax, uint64_t pp, uint64_t cap) {
  const uint64_t ns[] = {1, 127, 128, 129, 300, cmax - 1, cmax, cmax + 1, 3 * cmax + 44};
  for (uint64_t n : ns) check_plan(n, cmax, pp, cap);
}

int main() {
  check_sizes();
  for (uint64_t pp : {128ull, 256ull, 4096ull, 16384ull, 65536ull}) {
    for (uint64_t cap : {kGiB, 8 * kGiB}) check_sizes_of(obhip::chunk_rows_for(pp, cap), pp, cap);
    for (uint64_t cmax : {128ull, 256ull}) check_sizes_of(cmax, pp, 0);
  }
  printf("ok %ld\n", cases);
  return failures ? 1 : 0;
}
