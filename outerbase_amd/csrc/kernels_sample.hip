// Kernels of the posterior draws (sample.cpp; include/obhip.h, "posterior draws").
// No reference counterpart: the reference package predicts a mean and a variance, it does not draw.
//
// With H = L L^T and X = L^-T resident in the posterior handle, Theta[:, s] = theta + X z_s is a draw from
// N(theta, inv(H)) for z_s ~ N(0, I_p), and its sample path at row i is b_i^T Theta[:, s].
//
//   k_draw            the triangular product for up to 128 draws: one workgroup per coefficient k, thread = draw,
//                     Theta_ks = theta_k + sum_{j >= k} X_kj z_js with j ascending in one fma chain and theta
//                     added last -- one order per (k, s) whatever the launch; written term-major [p][16 NQB]
//                     with zero padding columns (the B operand of the matrix-core predictors) and, for the
//                     draw entry, column-major p x S.
//   k_sample_ext      the fused pass: k_predict_multi<NQB> (kernels_multi.hip) up to and including
//                     (acc + red) * scale, so that every (row, draw) value carries the bits that kernel would
//                     store -- and then no [QW][64] staging and no store: a lane reduces its four rows, a
//                     butterfly over the four k-quarters of the wave gives the best of the 16 rows a column
//                     has there, the four row groups meet in LDS, and one (key, lowest index among equals)
//                     pair per draw and workgroup goes to part_key / part_idx [block][QW].  NQB = 8 as well:
//                     without the [QW][64] staging a 128-draw pass fits the LDS up to Mu <= 167, and it was
//                     measured faster than two 64-draw passes.
//   k_sample_colext   the same partials from paths in HBM (the unfused route), 256 rows per workgroup.
//   k_sample_pick     one workgroup per draw: the partials lane-strided in ascending block order, an LDS tree.
// key = sgn * value (sgn = -1 for the maximum: exact), so that "better" is "smaller key, then lower index":
// a total order, hence independent of the order of the comparisons.  A row that is not eligible or whose
// value is not finite never enters: NaN never wins.  No atomics, no grid-wide barrier.
#include <cmath>

#include "obhip_internal.h"
#include "device_dx.h"
#include "vec_ops.h"

namespace obhip {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int kSxThreads = 512, kSxWaves = kSxThreads / 64;
constexpr int64_t kNoIndex = INT64_MAX;

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// (key, index) a beats b: the smaller key, the lower index among equals (-0.0 == 0.0)
__device__ __forceinline__ bool better(double ka, int64_t ia, double kb, int64_t ib) {
  return ka < kb || (ka == kb && ia < ib);
}

__device__ __forceinline__ void take_better(double ok, int64_t oi, double &key, int64_t &idx) {
  if (better(ok, oi, key, idx)) {
    key = ok;
    idx = oi;
  }
}

__global__ void __launch_bounds__(128)
k_draw(int p, uint64_t pp, const double *__restrict__ X, const double *__restrict__ theta,
       const double *__restrict__ z, uint64_t ldz, int qc, int qw, double *__restrict__ tht,
       double *__restrict__ Theta) {
  const int k = blockIdx.x, s = threadIdx.x;
  double v = 0.0;
  if (s < qc) {
    const double *xr = X + (uint64_t)k * pp, *zc = z + (uint64_t)s * ldz;
    double acc = 0.0;
#pragma unroll 8
    for (int j = k; j < p; ++j) acc = fma(xr[j], zc[j], acc);
    v = theta[k] + acc;
  }
  if (tht && s < qw) tht[(size_t)k * qw + s] = v;
  if (Theta && s < qc) Theta[(uint64_t)s * p + k] = v;
}

// 8 waves per 64-row tile, as k_predict_multi<NQB>: wave = (row group of 16, half of the 4-term steps)
template <int NQB>
__global__ void __launch_bounds__(kSxThreads)
k_sample_ext(const DimDesc *__restrict__ dims, const double *__restrict__ ka, const double *__restrict__ kb,
             const double *__restrict__ kc, const double *__restrict__ rot, const double *__restrict__ tab,
             const int *__restrict__ cpos, int d, int Mu, int tile_doubles, const uint32_t *__restrict__ colsw,
             int W2, int p, const double *__restrict__ ThT /* [p][16 NQB] */, const double *__restrict__ x,
             uint64_t n, const uint8_t *__restrict__ elig, double sgn, double *__restrict__ part_key,
             int64_t *__restrict__ part_idx) {
  extern __shared__ double lds[];
  constexpr int QW = 16 * NQB;
  double *reds = lds + tile_doubles;            // [8][64] scale partials
  double *scl = reds + kSxWaves * kTileRows;    // [64] basescale of the rows
  double *red = scl + kTileRows;                // [4][NQB][256] partials of the second half
  double *wkey = red + 4 * NQB * 256;           // [4][QW] best key of a row group
  int64_t *widx = (int64_t *)(wkey + 4 * QW);   // [4][QW] and its row
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t row0 = (uint64_t)blockIdx.x * kTileRows;
  {
    const uint64_t row = row0 + lane;
    const bool valid = row < n;
    const StoreTile<kTileRows> store{lds, cpos, lane, Mu};
    build_tile<kSxWaves, false>(dims, ka, kb, kc, rot, tab, nullptr, d, x, n, row, valid, wave, store, reds);
  }
  __syncthreads();
  if (wave == 0) scl[lane] = tile_scale<kSxWaves>(reds, lane);
  const int m = lane & 15, kq = lane >> 4;
  const int rg = wave & 3, half = wave >> 2;
  const int trow = 16 * rg + m;
  d4 acc[NQB];
#pragma unroll
  for (int j = 0; j < NQB; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
  const int nsteps = (p + 3) / 4;
  for (int s = half; s < nsteps; s += 2) {
    const int k = 4 * s + kq;
    const bool ok = k < p;
    const int kk = min(k, p - 1);
    double pr = ok ? 1.0 : 0.0;
    const uint32_t *cw = colsw + (size_t)kk * W2;
    for (int w = 0; w < W2; ++w) {
      const uint32_t c = cw[w];
      pr *= lds[(c & 0xffffu) * kTileRows + trow];
      pr *= lds[(c >> 16) * kTileRows + trow];
    }
#pragma unroll
    for (int j = 0; j < NQB; ++j) acc[j] = mfma(pr, ThT[(size_t)kk * QW + 16 * j + m], acc[j]);
  }
  if (half == 1) {
#pragma unroll
    for (int j = 0; j < NQB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(rg * NQB + j) * 256 + 4 * lane + r] = acc[j][r];
  }
  __syncthreads();
  if (half == 0) {
    // the lane's four rows 16 rg + kq + 4 r, ascending in r
    bool rok[4];
    double rs[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = 16 * rg + kq + 4 * r;
      const uint64_t row = row0 + orow;
      rok[r] = row < n && elig[row < n ? row : 0] != 0;
      rs[r] = scl[orow];
    }
#pragma unroll
    for (int j = 0; j < NQB; ++j) {
      double key = INFINITY;
      int64_t idx = kNoIndex;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double v = (acc[j][r] + red[(rg * NQB + j) * 256 + 4 * lane + r]) * rs[r];
        if (rok[r] && isfinite(v)) take_better(sgn * v, (int64_t)(row0 + 16 * rg + kq + 4 * r), key, idx);
      }
      // the 16 rows column 16 j + m has in this wave: the four k-quarters
#pragma unroll
      for (int off = 16; off <= 32; off <<= 1) {
        const double okey = __shfl_xor(key, off, 64);
        const int64_t oidx = __shfl_xor((long long)idx, off, 64);
        take_better(okey, oidx, key, idx);
      }
      if (kq == 0) {
        wkey[rg * QW + 16 * j + m] = key;
        widx[rg * QW + 16 * j + m] = idx;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < QW) {
    double key = wkey[threadIdx.x];
    int64_t idx = widx[threadIdx.x];
#pragma unroll
    for (int g = 1; g < 4; ++g) take_better(wkey[g * QW + threadIdx.x], widx[g * QW + threadIdx.x], key, idx);
    part_key[(uint64_t)blockIdx.x * QW + threadIdx.x] = key;
    part_idx[(uint64_t)blockIdx.x * QW + threadIdx.x] = idx;
  }
}

// the unfused route: 256 rows of one column per workgroup
__global__ void __launch_bounds__(256)
k_sample_colext(const double *__restrict__ path, uint64_t ld, uint64_t nr, uint64_t row0,
                const uint8_t *__restrict__ elig, double sgn, uint64_t stride, double *__restrict__ part_key,
                int64_t *__restrict__ part_idx) {
  __shared__ double wk[4];
  __shared__ int64_t wi[4];
  const uint64_t rl = (uint64_t)blockIdx.x * kColextRows + threadIdx.x;
  const int s = blockIdx.y;
  double key = INFINITY;
  int64_t idx = kNoIndex;
  if (rl < nr) {
    const double v = path[(uint64_t)s * ld + rl];
    if (elig[row0 + rl] != 0 && isfinite(v)) {
      key = sgn * v;
      idx = (int64_t)(row0 + rl);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double okey = __shfl_xor(key, off, 64);
    const int64_t oidx = __shfl_xor((long long)idx, off, 64);
    take_better(okey, oidx, key, idx);
  }
  if ((threadIdx.x & 63) == 0) {
    wk[threadIdx.x >> 6] = key;
    wi[threadIdx.x >> 6] = idx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < 4; ++q) take_better(wk[q], wi[q], key, idx);
    const uint64_t b = row0 / kColextRows + blockIdx.x;
    part_key[b * stride + s] = key;
    part_idx[b * stride + s] = idx;
  }
}

__global__ void __launch_bounds__(256)
k_sample_pick(const double *__restrict__ part_key, const int64_t *__restrict__ part_idx, uint64_t nparts,
              uint64_t stride, double sgn, int64_t *__restrict__ index, double *__restrict__ value) {
  __shared__ double wk[256];
  __shared__ int64_t wi[256];
  const int s = blockIdx.x;
  double key = INFINITY;
  int64_t idx = kNoIndex;
  for (uint64_t b = threadIdx.x; b < nparts; b += 256) take_better(part_key[b * stride + s], part_idx[b * stride + s], key, idx);
  wk[threadIdx.x] = key;
  wi[threadIdx.x] = idx;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) {
      key = wk[threadIdx.x];
      idx = wi[threadIdx.x];
      take_better(wk[threadIdx.x + off], wi[threadIdx.x + off], key, idx);
      wk[threadIdx.x] = key;
      wi[threadIdx.x] = idx;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const bool none = wi[0] == kNoIndex;
    index[s] = none ? -1 : wi[0];
    value[s] = none ? NAN : sgn * wk[0];
  }
}

size_t sample_ext_lds(uint64_t Mu, int nqb, int *tile_doubles) {
  const size_t tile = Mu * kTileRows;
  *tile_doubles = (int)tile;
  return (tile + kSxWaves * kTileRows + kTileRows + (size_t)4 * nqb * 256 + (size_t)2 * 4 * 16 * nqb) * sizeof(double);
}

template <int NQB>
int run_sample_ext(const obhip_model &m, obhip_terms &t, const double *d_tht, const double *d_x, uint64_t n,
                   const uint8_t *d_elig, double sgn, double *part_key, int64_t *part_idx) {
  int tile = 0;
  const size_t lds = sample_ext_lds(t.Mu, NQB, &tile);
  OB_TRY(ensure_dyn_lds((const void *)k_sample_ext<NQB>, lds));
  launch_pred<false>(k_sample_ext<NQB>, dim3((unsigned)((n + kTileRows - 1) / kTileRows)), dim3(kSxThreads), lds,
                     pred_tabs(m, t), tile, (const uint32_t *)t.cols.p, (int)(t.W / 2), (int)t.p, d_tht, d_x, n, d_elig,
                     sgn, part_key, part_idx);
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace

// As predict_multi_supports: the padded width of the column lists is even (the kernel reads them two to a
// word), and the tile of the Mu used columns plus the scale partials, red and the reduction scratch of the
// narrowest pass (1728 doubles) fit the LDS of a workgroup: Mu <= 293 (a pass of 128 draws: Mu <= 167, of 64: 239,
// of 32: 275).  Within predict_multi_supports (Mu <= 295),
// asked for by name: the fused values are that kernel's, and sample must be able to give the same ones.
bool sample_ext_supports(const obhip_terms &t) {
  int tile = 0;
  return predict_multi_supports(t) && sample_ext_lds(t.Mu, 1, &tile) <= kLdsBudget;
}

int sample_ext_nqb_max(const obhip_terms &t) {
  int tile = 0, nqb = 8;
  while (nqb > 1 && sample_ext_lds(t.Mu, nqb, &tile) > kLdsBudget) nqb /= 2;
  return nqb;
}

int launch_draw(const PostFactor &f, const double *d_theta, const double *d_z, uint64_t ldz, int qc, uint64_t qw,
                double *d_tht, double *d_Theta) {
  ProfScope ps("draw");
  hipLaunchKernelGGL(k_draw, dim3((unsigned)f.p), dim3(qw > 64 ? 128 : 64), 0, cur_stream(), (int)f.p, f.pp, (const double *)f.X.p,
                     d_theta, d_z, ldz, qc, (int)qw, d_tht, d_Theta);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_sample_elig(const double *d_x, uint64_t n, uint64_t d, const uint8_t *d_skip, uint8_t *d_elig) {
  return vmap(n, [=] __device__(uint64_t i) {
    bool ok = !(d_skip && d_skip[i] != 0);
    for (uint64_t l = 0; l < d; ++l) ok = ok && isfinite(d_x[l * n + i]);
    d_elig[i] = ok ? 1 : 0;
  });
}

int launch_sample_ext(const obhip_model &m, obhip_terms &t, const double *d_tht, int nqb, const double *d_x,
                      uint64_t n, const uint8_t *d_elig, double sgn, double *part_key, int64_t *part_idx) {
  ProfScope ps("sample_ext");
  return pick_or<1, 2, 4, 8>(nqb, no_kernel(), [&](auto NQB) {
    return run_sample_ext<NQB()>(m, t, d_tht, d_x, n, d_elig, sgn, part_key, part_idx);
  });
}

int launch_sample_colext(const double *d_path, uint64_t ld, uint64_t nr, uint64_t row0, int qc, const uint8_t *d_elig,
                         double sgn, uint64_t stride, double *part_key, int64_t *part_idx) {
  ProfScope ps("sample_colext");
  hipLaunchKernelGGL(k_sample_colext, dim3((unsigned)((nr + kColextRows - 1) / kColextRows), (unsigned)qc), dim3(256),
                     0, cur_stream(), d_path, ld, nr, row0, d_elig, sgn, stride, part_key, part_idx);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_sample_pick(const double *part_key, const int64_t *part_idx, uint64_t nparts, uint64_t stride, int qc,
                       double sgn, int64_t *d_index, double *d_value) {
  hipLaunchKernelGGL(k_sample_pick, dim3((unsigned)qc), dim3(256), 0, cur_stream(), part_key, part_idx, nparts, stride,
                     sgn, d_index, d_value);
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace obhip
