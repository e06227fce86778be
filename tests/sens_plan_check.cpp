// Stand-alone check of csrc/sens_plan.h for tests/test_sens_plan_host.py: walks every case itself, prints one line
// per failed property and "ok <cases>" at the end; the exit status is the number of failures (at most 1).
//   passes:   d = 1 .. 60 at T = 5: pass_of maps every (di <= dj) to a pass whose decode gives (di / T, dj / T), the
//             passes hit are exactly 0 .. pass_count - 1, and the largest index a block of the pair kernel writes is
//             pair_part_doubles - 1
//   tiles:    tile_pair and tile_pair_lower enumerate each pair once, in the documented order, ntile = 1 .. 40
//   packed:   packed_pair with and without the diagonal is a bijection onto the pairs, in row-major order
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../outerbase_amd/csrc/sens_plan.h"

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

static void check_passes() {
  const int T = 5, RC = 2, TW = 128;
  for (int d = 1; d <= 60; ++d) {
    const int nb = obhip::dim_blocks(d, T), npass = obhip::pass_count(d, T);
    CHECK(npass == nb + nb * (nb - 1) / 2, "pass_count d=%d", d);
    std::vector<int> hit(npass, 0);
    for (int di = 0; di < d; ++di)
      for (int dj = di; dj < d; ++dj) {
        const int z = obhip::pass_of(di, dj, d, T);
        CHECK(z >= 0 && z < npass, "pass_of out of range d=%d (%d,%d) -> %d", d, di, dj, z);
        if (z < 0 || z >= npass) continue;
        ++hit[z];
        // the kernels decode a pass within its launch: the diagonal launch has passes 0 .. nb-1 at zbase 0, the
        // off-diagonal one the rest at zbase nb
        const bool diag = z < nb;
        int bi = -1, bj = -1;
        obhip::pass_blocks(diag ? z : z - nb, nb, diag, bi, bj);
        CHECK(bi == di / T && bj == dj / T, "decode d=%d (%d,%d): pass %d -> blocks (%d,%d)", d, di, dj, z, bi, bj);
        CHECK(diag == (di / T == dj / T), "diagonal pass d=%d (%d,%d)", d, di, dj);
      }
    for (int z = 0; z < npass; ++z) CHECK(hit[z] > 0, "pass %d of d=%d holds no output", z, d);
    // the last double of the last block (pass, response chunk, tile pair) that a launch writes
    for (uint64_t p : {1u, 128u, 129u, 1000u})
      for (uint64_t q : {1u, 2u, 3u}) {
        const uint64_t nrc = (q + RC - 1) / RC, nt = (p + TW - 1) / TW, npairs = nt * (nt + 1) / 2, blk = RC * T * T;
        const uint64_t last = obhip::pair_part_index(npass - 1, nrc, nrc - 1, npairs, npairs - 1, blk) + blk - 1;
        CHECK(last == obhip::pair_part_doubles(p, d, q, T, RC, TW) - 1, "part size d=%d p=%d q=%d", d, (int)p, (int)q);
      }
  }
}

static void check_tiles() {
  for (int ntile = 1; ntile <= 40; ++ntile) {
    int z = 0;
    for (int I = 0; I < ntile; ++I)
      for (int J = I; J < ntile; ++J, ++z) {  // (0,0), (0,1), .. (0,ntile-1), (1,1), ..
        int i = -1, j = -1;
        obhip::tile_pair(z, ntile, i, j);
        CHECK(i == I && j == J, "tile_pair ntile=%d z=%d -> (%d,%d), want (%d,%d)", ntile, z, i, j, I, J);
      }
    CHECK(z == ntile * (ntile + 1) / 2, "tile_pair count ntile=%d", ntile);
    z = 0;
    for (int ta = 0; ta < ntile; ++ta)
      for (int tb = 0; tb <= ta; ++tb, ++z) {  // (0,0), (1,0), (1,1), (2,0), ..
        int a = -1, b = -1;
        obhip::tile_pair_lower(z, a, b);
        CHECK(a == ta && b == tb, "tile_pair_lower z=%d -> (%d,%d), want (%d,%d)", z, a, b, ta, tb);
      }
  }
}

static void check_packed() {
  for (int d = 1; d <= 60; ++d)
    for (int with_diag = 0; with_diag < 2; ++with_diag) {
      int o = 0;
      for (int di = 0; di < d; ++di)
        for (int dj = di + 1 - with_diag; dj < d; ++dj, ++o) {
          int i = -1, j = -1;
          obhip::packed_pair(o, d, with_diag != 0, i, j);
          CHECK(i == di && j == dj, "packed_pair d=%d diag=%d o=%d -> (%d,%d), want (%d,%d)", d, with_diag, o, i, j, di,
                dj);
        }
      CHECK(o == (with_diag ? d * (d + 1) / 2 : d * (d - 1) / 2), "packed_pair count d=%d diag=%d", d, with_diag);
    }
}

int main() {
  check_passes();
  check_tiles();
  check_packed();
  if (!failures) printf("ok %ld\n", cases);
  return failures ? 1 : 0;
}
