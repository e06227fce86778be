// Device helpers shared by kernels_sobol.hip, kernels_shapley.hip, kernels_active.hip and kernels_moments.hip.
// The index arithmetic that the host shares is in sens_plan.h, the frame of the term-pair sums in pair_sum.h.
#pragma once
#include <hip/hip_runtime.h>

#include "obhip_internal.h"
#include "device_common.h"
#include "sens_plan.h"

namespace obhip {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// sum over the block's 256 threads by a tree in red[256]; every thread gets it
__device__ __forceinline__ double block_tree_256(double v, double *red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  return red[0];
}

// ---- the moment kernels (kernels_moments.hip) ---------------------------------------------------------------
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

struct StoreCol {
  double *col;  // tile + thread
  int ccol0, nt;
  __device__ __forceinline__ void operator()(int ccol, double v) const { col[(size_t)(ccol - ccol0 + 1) * nt] = v; }
};

// raw psi_{l,t}(xv), t < D.ncol, into col[t * nt]
__device__ __forceinline__ void eval_raw(const DimDesc &D, const double *ka, const double *kb, const double *kc,
                                         const double *rot, const double *tab, double xv, double *col, int nt) {
  const StoreCol st{col, D.ccol0, nt};
  const double c0 = build_dim_any(D, ka, kb, kc, rot, tab, xv, st);
  col[0] = c0;
  for (int t = 1; t < D.ncol; ++t) col[(size_t)t * nt] *= c0;
}

// threads per block and dynamic LDS of the kernels that evaluate one basis tile:
// [interval tables kIntervalTabMax][reduction 4 * 64][tile lmax * threads]
inline int eval_threads(uint64_t lmax) { return lmax <= 32 ? 256 : 64; }
inline size_t eval_lds(uint64_t lmax) {
  return (kIntervalTabMax + 4 * kMomP2 + lmax * eval_threads(lmax)) * sizeof(double);
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
