// Device helpers shared by kernels_sobol.hip, kernels_shapley.hip and kernels_active.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "obhip_internal.h"

namespace obhip {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the z-th pair (I <= J) of ntile term tiles in the order (0,0), (0,1), .. (0,ntile-1), (1,1), ..
__device__ __forceinline__ void tile_pair(int z, int ntile, int &I, int &J) {
  I = 0;
  while (z >= ntile - I) {
    z -= ntile - I;
    ++I;
  }
  J = I + z;
}

// the z-th pair (ta >= tb) of level tiles in the order (0,0), (1,0), (1,1), (2,0), ..
__device__ __forceinline__ void tile_pair_lower(int z, int &ta, int &tb) {
  ta = 0;
  while (z >= ta + 1) {
    z -= ta + 1;
    ++ta;
  }
  tb = z;
}

// ---- the moment kernels (k_dim_moments, k_dim_grad_moments) -------------------------------------------------
constexpr int kMomLT = 8;            // levels per accumulator tile
constexpr int kMomP1 = kMomLT + 2;   // sums of pass 1: 8 levels, the weights, the bad weights
constexpr int kMomP2 = kMomLT * kMomLT;
constexpr int kMomBlocks = 512;      // row slices at most

// the dimension's interval tables into LDS (all threads of the block call it); -> the table base
__device__ __forceinline__ const double *stage_tab(DimDesc &D, const double *__restrict__ tab, double *ltab) {
  if (D.tab < 0) return tab;
  const int sz = ((D.m + 1) & ~1) + (D.m + 1) * D.ncol * 6;
  if (sz > kIntervalTabMax) return tab;
  for (int e = threadIdx.x; e < sz; e += blockDim.x) ltab[e] = tab[D.tab + e];
  __syncthreads();
  D.tab = 0;
  return ltab;
}

__device__ __forceinline__ int mean_offset(const DimDesc *__restrict__ dims, int l) {
  int o = 0;
  for (int i = 0; i < l; ++i) o += dims[i].ncol;
  return o;
}
__device__ __forceinline__ int cov_offset(const DimDesc *__restrict__ dims, int l) {
  int o = 0;
  for (int i = 0; i < l; ++i) o += dims[i].ncol * dims[i].ncol;
  return o;
}

// part[k] = sum over the block of acc[k]: butterfly per wave, the waves in order
template <int K>
__device__ __forceinline__ void block_sums(const double (&acc)[K], double *red, double *__restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double v = wave_sum(acc[k]);
    if (lane == 0) red[wave * K + k] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < K) {
    double s = 0.0;
    for (int w = 0; w < nw; ++w) s += red[w * K + threadIdx.x];
    part[threadIdx.x] = s;
  }
}

// sum over the nblk row slices of entry k of K, every lane of the wave gets it
template <int K>
__device__ __forceinline__ double slices_sum(const double *__restrict__ base, int nblk, int k) {
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 64) s += base[(uint64_t)b * K + k];
  return wave_sum(s);
}

}  // namespace obhip
