// The index arithmetic of the sensitivity family that its kernels and its host code must agree on (pair_sum.h,
// kernels_sobol.hip, kernels_active.hip, kernels_shapley.hip): plain C++17, nothing from HIP,
// so that tests/sens_plan_check.cpp can walk every case on the host.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define OBHIP_SENS_HD __host__ __device__
#else
#define OBHIP_SENS_HD
#endif

namespace obhip {

// the z-th pair (I <= J) of ntile term tiles in the order (0,0), (0,1), .. (0,ntile-1), (1,1), ..
OBHIP_SENS_HD inline void tile_pair(int z, int ntile, int &I, int &J) {
  I = 0;
  while (z >= ntile - I) {
    z -= ntile - I;
    ++I;
  }
  J = I + z;
}

// the z-th pair (ta >= tb) of level tiles in the order (0,0), (1,0), (1,1), (2,0), ..
OBHIP_SENS_HD inline void tile_pair_lower(int z, int &ta, int &tb) {
  ta = 0;
  while (z >= ta + 1) {
    z -= ta + 1;
    ++ta;
  }
  tb = z;
}

// The d x d triangle of outputs of a block pair sum is cut into nb = ceil(d / T) blocks of T dimensions.  Passes
// 0 .. nb-1 are the diagonal blocks (bi = bj = pass); pass nb + z is the z-th pair bi < bj in the order
// (0,1), (0,2), .. (0,nb-1), (1,2), ..
OBHIP_SENS_HD inline int dim_blocks(int d, int T) { return (d + T - 1) / T; }
OBHIP_SENS_HD inline int pass_count(int d, int T) {
  const int nb = dim_blocks(d, T);
  return nb + nb * (nb - 1) / 2;
}
// z: the pass within its launch (the diagonal launch has nb of them, the off-diagonal one the rest)
OBHIP_SENS_HD inline void pass_blocks(int z, int nb, bool diag, int &bi, int &bj) {
  bi = bj = z;
  if (diag) return;
  bi = 0;
  while (z >= nb - 1 - bi) {
    z -= nb - 1 - bi;
    ++bi;
  }
  bj = bi + 1 + z;
}
// the inverse: the pass that holds output (di <= dj), at (di % T) * T + dj % T of its T x T outputs
OBHIP_SENS_HD inline int pass_of(int di, int dj, int d, int T) {
  const int nb = dim_blocks(d, T), bi = di / T, bj = dj / T;
  return bi == bj ? bi : nb + bi * (nb - 1) - bi * (bi - 1) / 2 + (bj - bi - 1);
}

// partials of a block pair sum over p terms in tiles of tw: part[((pass * nrc + rc) * npairs + pair) * RC * T * T + e]
OBHIP_SENS_HD inline uint64_t pair_part_index(uint64_t pass, uint64_t nrc, uint64_t rc, uint64_t npairs, uint64_t pair,
                                              uint64_t block_doubles) {
  return ((pass * nrc + rc) * npairs + pair) * block_doubles;
}
OBHIP_SENS_HD inline uint64_t pair_part_doubles(uint64_t p, uint64_t d, uint64_t q, int T, int RC, int tw) {
  const uint64_t nrc = (q + RC - 1) / RC, nt = (p + tw - 1) / tw;
  return pair_part_index((uint64_t)pass_count((int)d, T), nrc, 0, nt * (nt + 1) / 2, 0, (uint64_t)RC * T * T);
}

// entry o of the packed upper triangle of d dimensions, row-major: with the diagonal (0,0), (0,1), .. (1,1), ..;
// without it (0,1), (0,2), .. (0,d-1), (1,2), ..
OBHIP_SENS_HD inline void packed_pair(int o, int d, bool with_diag, int &di, int &dj) {
  const int first = with_diag ? d : d - 1;  // entries of row 0
  di = 0;
  while (o >= first - di) {
    o -= first - di;
    ++di;
  }
  dj = di + o + (with_diag ? 0 : 1);
}

}  // namespace obhip
