// Kernels of the sequential design (design.cpp; include/obhip.h, "sequential design").  No reference
// counterpart: the reference package fits and predicts, it does not choose the next runs.
//
// One greedy step conditions the posterior on a run at the picked row j and scores every candidate for
// the next pick.  With S = inv(H), nu = e^{2 sigma}, s = S b_j, gamma = nu + b_j^T s, and for the
// integrated-variance criterion T = S M S, h = T b_j, tau = b_j^T h:
//     a_i = b_i^T s      c_i = b_i^T h
//     d_i   <- d_i - a_i^2 / gamma
//     num_i <- num_i - 2 a_i c_i / gamma + a_i^2 tau / gamma^2
//     score_i = w_i d_i (MAXVAR)  |  w_i num_i / (nu + d_i) (IMSE)
//
//   k_design_step    the fused step: the structure of k_predict_multi<1> (kernels_multi.hip) -- basis of a
//                    64-row tile into LDS by build_tile, the term products formed once per (row, term) and
//                    multiplied on the matrix cores with a term-major [p][16] block whose column 0 is s and
//                    column 1 is h -- with a new epilogue: a and c never reach HBM; the tile's 64 rows are
//                    downdated, scored and reduced to one (best score, lowest index) pair per workgroup.
//                    Only 2 of the 16 columns of v_mfma_f64_16x16x4_f64 carry data: the products of a
//                    (row, term) are the cost of the pass, the matrix instruction is what sums them in the
//                    order the multi-response predictor does.
//   k_design_update  the same epilogue from a and c in HBM (the unfused route: launch_predict_multi first).
//   k_design_pick    one workgroup: the partial pairs in a fixed order, the pick appended, x_j gathered.
//   k_design_matvec, k_design_scalars, k_design_rank   the p-space work between two steps on explicit S, T.
// No atomics, no grid-wide barrier: every sum and every argmax runs in a fixed order.
#include <cmath>

#include "obhip_internal.h"
#include "device_dx.h"
#include "vec_ops.h"

namespace obhip {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int kDsThreads = 512, kDsWaves = kDsThreads / 64;
constexpr int64_t kNoIndex = INT64_MAX;

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// (score, index) a beats b: the larger score, the lower index among equals
__device__ __forceinline__ bool beats(double sa, int64_t ia, double sb, int64_t ib) {
  return sa > sb || (sa == sb && ia < ib);
}

// downdate of one candidate by the previous pick and its score for the next one; -inf: not eligible
template <int CRIT>
__device__ __forceinline__ double design_row(double a, double c, double gamma, double tau, double nu, double w,
                                             bool taken, double &d, double &num) {
  const double ag = a / gamma;
  d -= a * ag;
  double score;
  if (CRIT == OBHIP_DESIGN_IMSE) {
    num += ag * (ag * tau - 2.0 * c);
    score = w * num / (nu + d);
  } else {
    score = w * d;
  }
  return (taken || !(w > 0.0) || !isfinite(score)) ? -INFINITY : score;
}

// the 64 lanes of a wave -> lane 0's pair is the wave's best
__device__ __forceinline__ void wave_best(double &score, int64_t &idx) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double os = __shfl_xor(score, off, 64);
    const int64_t oi = __shfl_xor((long long)idx, off, 64);
    if (beats(os, oi, score, idx)) {
      score = os;
      idx = oi;
    }
  }
}

// 8 waves per 64-row tile, as k_predict_multi<1>: wave = (row group of 16, half of the 4-term steps)
template <int CRIT>
__global__ void __launch_bounds__(kDsThreads)
k_design_step(const DimDesc *__restrict__ dims, const double *__restrict__ ka, const double *__restrict__ kb,
              const double *__restrict__ kc, const double *__restrict__ rot, const double *__restrict__ tab,
              const int *__restrict__ cpos, int d, int Mu, int tile_doubles, const uint32_t *__restrict__ colsw,
              int W2, int p, const double *__restrict__ sh /* [p][16] */, const double *__restrict__ x, uint64_t n,
              const double *__restrict__ scal, const double *__restrict__ w, const uint8_t *__restrict__ picked,
              double *__restrict__ dvar, double *__restrict__ num, double *__restrict__ part_score,
              int64_t *__restrict__ part_idx) {
  extern __shared__ double lds[];
  double *reds = lds + tile_doubles;            // [8][64] scale partials
  double *scl = reds + kDsWaves * kTileRows;    // [64] basescale of the rows
  double *red = scl + kTileRows;                // [4][256] partials of the second half
  double *ac = red + 4 * 256;                   // [2][64]: a and c of the tile's rows
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t row0 = (uint64_t)blockIdx.x * kTileRows;
  {
    const uint64_t row = row0 + lane;
    const bool valid = row < n;
    const StoreTile<kTileRows> store{lds, cpos, lane, Mu};
    build_tile<kDsWaves, false>(dims, ka, kb, kc, rot, tab, nullptr, d, x, n, row, valid, wave, store, reds);
  }
  __syncthreads();
  if (wave == 0) scl[lane] = tile_scale<kDsWaves>(reds, lane);
  const int m = lane & 15, kq = lane >> 4;
  const int rg = wave & 3, half = wave >> 2;
  const int trow = 16 * rg + m;
  d4 acc = d4{0.0, 0.0, 0.0, 0.0};
  const int nsteps = (p + 3) / 4;
  for (int s = half; s < nsteps; s += 2) {
    const int k = 4 * s + kq;
    const bool ok = k < p;
    const int kk = min(k, p - 1);
    double pr = ok ? 1.0 : 0.0;
    const uint32_t *cw = colsw + (size_t)kk * W2;
    for (int q = 0; q < W2; ++q) {
      const uint32_t c = cw[q];
      pr *= lds[(c & 0xffffu) * kTileRows + trow];
      pr *= lds[(c >> 16) * kTileRows + trow];
    }
    acc = mfma(pr, sh[(size_t)kk * 16 + m], acc);
  }
  if (half == 1) {
#pragma unroll
    for (int r = 0; r < 4; ++r) red[rg * 256 + 4 * lane + r] = acc[r];
  }
  __syncthreads();
  if (half == 0 && m < 2) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = 16 * rg + kq + 4 * r;
      ac[m * kTileRows + orow] = (acc[r] + red[rg * 256 + 4 * lane + r]) * scl[orow];
    }
  }
  __syncthreads();
  if (wave != 0) return;
  // the epilogue: lane = row
  const uint64_t row = row0 + lane;
  double score = -INFINITY;
  int64_t idx = kNoIndex;
  if (row < n) {
    double dv = dvar[row], nm = CRIT == OBHIP_DESIGN_IMSE ? num[row] : 0.0;
    score = design_row<CRIT>(ac[lane], ac[kTileRows + lane], scal[0], scal[1], scal[3], w ? w[row] : 1.0,
                             picked && picked[row], dv, nm);
    dvar[row] = dv;
    if (CRIT == OBHIP_DESIGN_IMSE) num[row] = nm;
    idx = (int64_t)row;
  }
  wave_best(score, idx);
  if (lane == 0) {
    part_score[blockIdx.x] = score;
    part_idx[blockIdx.x] = idx;
  }
}

// the unfused route: 256 rows per workgroup, a = ac[i], c = ac[n + i]
template <int CRIT>
__global__ void __launch_bounds__(256)
k_design_update(uint64_t n, const double *__restrict__ acv, const double *__restrict__ scal,
                const double *__restrict__ w, const uint8_t *__restrict__ picked, double *__restrict__ dvar,
                double *__restrict__ num, double *__restrict__ part_score, int64_t *__restrict__ part_idx) {
  __shared__ double ws[4];
  __shared__ int64_t wi[4];
  const uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  double score = -INFINITY;
  int64_t idx = kNoIndex;
  if (row < n) {
    double dv = dvar[row], nm = CRIT == OBHIP_DESIGN_IMSE ? num[row] : 0.0;
    score = design_row<CRIT>(acv[row], acv[n + row], scal[0], scal[1], scal[3], w ? w[row] : 1.0,
                             picked && picked[row], dv, nm);
    dvar[row] = dv;
    if (CRIT == OBHIP_DESIGN_IMSE) num[row] = nm;
    idx = (int64_t)row;
  }
  wave_best(score, idx);
  if ((threadIdx.x & 63) == 0) {
    ws[threadIdx.x >> 6] = score;
    wi[threadIdx.x >> 6] = idx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < 4; ++q)
      if (beats(ws[q], wi[q], score, idx)) {
        score = ws[q];
        idx = wi[q];
      }
    part_score[blockIdx.x] = score;
    part_idx[blockIdx.x] = idx;
  }
}

// scal: [0] gamma, [1] tau, [2] d_j, [3] nu, [4] unused, [5] 1 = no eligible candidate was left
__global__ void __launch_bounds__(256)
k_design_pick(const double *__restrict__ part_score, const int64_t *__restrict__ part_idx, uint64_t nparts,
              const double *__restrict__ x, uint64_t n, int d, uint64_t step, int64_t *__restrict__ index,
              double *__restrict__ score_out, double *__restrict__ xj, uint8_t *__restrict__ picked,
              double *__restrict__ scal) {
  __shared__ double ws[256];
  __shared__ int64_t wi[256];
  double score = -INFINITY;
  int64_t idx = kNoIndex;
  for (uint64_t b = threadIdx.x; b < nparts; b += 256) {
    const double os = part_score[b];
    const int64_t oi = part_idx[b];
    if (beats(os, oi, score, idx)) {
      score = os;
      idx = oi;
    }
  }
  ws[threadIdx.x] = score;
  wi[threadIdx.x] = idx;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off && beats(ws[threadIdx.x + off], wi[threadIdx.x + off], ws[threadIdx.x], wi[threadIdx.x])) {
      ws[threadIdx.x] = ws[threadIdx.x + off];
      wi[threadIdx.x] = wi[threadIdx.x + off];
    }
    __syncthreads();
  }
  score = ws[0];
  idx = wi[0];
  const bool none = !(score > -INFINITY) || idx < 0 || (uint64_t)idx >= n;
  if (none) {
    if (threadIdx.x == 0) scal[5] = 1.0;
    return;
  }
  if (threadIdx.x == 0) {
    index[step] = idx;
    score_out[step] = score;
    picked[idx] = 1;
  }
  for (int l = threadIdx.x; l < d; l += 256) xj[l] = x[(uint64_t)l * n + (uint64_t)idx];
}

// sv[k] = sum_l S[k][l] b[l], hv[k] = sum_l T[k][l] b[l] (T null: 0): one workgroup per row, a fixed order
__global__ void __launch_bounds__(256)
k_design_matvec(int p, uint64_t pp, const double *__restrict__ S, const double *__restrict__ T,
                const double *__restrict__ b, double *__restrict__ sv, double *__restrict__ hv) {
  __shared__ double red[2][256];
  const uint64_t k = blockIdx.x;
  double s = 0.0, h = 0.0;
  for (int l = threadIdx.x; l < p; l += 256) {
    const double bl = b[l];
    s += S[k * pp + l] * bl;
    if (T) h += T[k * pp + l] * bl;
  }
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = h;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) {
      red[0][threadIdx.x] += red[0][threadIdx.x + off];
      red[1][threadIdx.x] += red[1][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    sv[k] = red[0][0];
    hv[k] = red[1][0];
  }
}

// d_j = b . s, tau = b . h, gamma = nu + d_j into scal; trace[step + 1]; the [p][16] block's columns 0 and 1
template <int CRIT>
__global__ void __launch_bounds__(256)
k_design_scalars(int p, const double *__restrict__ b, const double *__restrict__ sv, const double *__restrict__ hv,
                 double *__restrict__ sh, double *__restrict__ scal, double *__restrict__ trace, uint64_t step) {
  __shared__ double red[2][256];
  double dj = 0.0, tau = 0.0;
  for (int k = threadIdx.x; k < p; k += 256) {
    dj += b[k] * sv[k];
    tau += b[k] * hv[k];
    sh[(size_t)k * 16] = sv[k];
    sh[(size_t)k * 16 + 1] = hv[k];
  }
  red[0][threadIdx.x] = dj;
  red[1][threadIdx.x] = tau;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) {
      red[0][threadIdx.x] += red[0][threadIdx.x + off];
      red[1][threadIdx.x] += red[1][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    dj = red[0][0];
    tau = red[1][0];
    const double nu = scal[3], gamma = nu + dj;
    scal[0] = gamma;
    scal[1] = tau;
    scal[2] = dj;
    trace[step + 1] = CRIT == OBHIP_DESIGN_IMSE ? trace[step] - tau / gamma : trace[step] + log1p(dj / nu);
  }
}

// S -= s s^T / gamma;  T -= (s h^T + h s^T) / gamma - s s^T tau / gamma^2
__global__ void __launch_bounds__(256)
k_design_rank(int p, uint64_t pp, const double *__restrict__ sv, const double *__restrict__ hv,
              const double *__restrict__ scal, double *__restrict__ S, double *__restrict__ T) {
  const int l = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  if (l >= p) return;
  const double gamma = scal[0], tau = scal[1];
  const double sk = sv[k] / gamma, sl = sv[l];
  S[(uint64_t)k * pp + l] -= sk * sl;
  if (T) T[(uint64_t)k * pp + l] -= sk * hv[l] + hv[k] / gamma * sl - sk * sl * (tau / gamma);
}

size_t design_step_lds(uint64_t Mu, int *tile_doubles) {
  const size_t tile = Mu * kTileRows;
  *tile_doubles = (int)tile;
  return (tile + kDsWaves * kTileRows + kTileRows + 4 * 256 + 2 * kTileRows) * sizeof(double);
}

template <int CRIT>
int run_design_step(const obhip_model &m, obhip_terms &t, const DesignStep &s) {
  int tile = 0;
  const size_t lds = design_step_lds(t.Mu, &tile);
  OB_TRY(ensure_dyn_lds((const void *)k_design_step<CRIT>, lds));
  launch_pred<false>(k_design_step<CRIT>, dim3((unsigned)design_step_parts(s.n, true)), dim3(kDsThreads), lds,
                     pred_tabs(m, t), tile, (const uint32_t *)t.cols.p, (int)(t.W / 2), (int)t.p, s.sh, s.x, s.n, s.scal,
                     s.w, s.replace ? nullptr : s.picked, s.dvar, s.num, s.part_score, s.part_idx);
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace

// As predict_multi_supports: the padded width of the column lists is even (the kernel reads them two to a
// word), and the tile of the Mu used columns plus the epilogue's 1728 doubles fit the LDS of a workgroup.
bool design_step_supports(const obhip_terms &t) {
  int tile = 0;
  return t.W >= 2 && t.W % 2 == 0 && design_step_lds(t.Mu, &tile) <= kLdsBudget && !getenv("OBHIP_FORCE_GENERIC");
}

uint64_t design_step_parts(uint64_t n, bool fused) {
  const uint64_t rows = fused ? kTileRows : 256;
  return (n + rows - 1) / rows;
}

int launch_design_step(const obhip_model &m, obhip_terms &t, const DesignStep &s) {
  ProfScope ps("design_step");
  if (s.crit == OBHIP_DESIGN_IMSE) return run_design_step<OBHIP_DESIGN_IMSE>(m, t, s);
  return run_design_step<OBHIP_DESIGN_MAXVAR>(m, t, s);
}

int launch_design_update(const DesignStep &s, const double *d_ac) {
  ProfScope ps("design_update");
  const dim3 grid((unsigned)design_step_parts(s.n, false));
  const uint8_t *picked = s.replace ? nullptr : s.picked;
  if (s.crit == OBHIP_DESIGN_IMSE)
    hipLaunchKernelGGL(k_design_update<OBHIP_DESIGN_IMSE>, grid, dim3(256), 0, cur_stream(), s.n, d_ac, s.scal, s.w,
                       picked, s.dvar, s.num, s.part_score, s.part_idx);
  else
    hipLaunchKernelGGL(k_design_update<OBHIP_DESIGN_MAXVAR>, grid, dim3(256), 0, cur_stream(), s.n, d_ac, s.scal, s.w,
                       picked, s.dvar, s.num, s.part_score, s.part_idx);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_design_pick(const DesignStep &s, uint64_t nparts, uint64_t d, uint64_t step, int64_t *d_index,
                       double *d_score, double *d_xj, uint8_t *d_picked, double *d_scal) {
  hipLaunchKernelGGL(k_design_pick, dim3(1), dim3(256), 0, cur_stream(), (const double *)s.part_score,
                     (const int64_t *)s.part_idx, nparts, s.x, s.n, (int)d, step, d_index, d_score, d_xj, d_picked,
                     d_scal);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_design_pspace(int crit, uint64_t p, uint64_t pp, const double *d_b, double *d_S, double *d_T, double *d_sv,
                         double *d_hv, double *d_sh, double *d_scal, double *d_trace, uint64_t step) {
  ProfScope ps("design_pspace");
  hipStream_t st = cur_stream();
  hipLaunchKernelGGL(k_design_matvec, dim3((unsigned)p), dim3(256), 0, st, (int)p, pp, (const double *)d_S,
                     (const double *)d_T, d_b, d_sv, d_hv);
  if (crit == OBHIP_DESIGN_IMSE)
    hipLaunchKernelGGL(k_design_scalars<OBHIP_DESIGN_IMSE>, dim3(1), dim3(256), 0, st, (int)p, d_b, (const double *)d_sv,
                       (const double *)d_hv, d_sh, d_scal, d_trace, step);
  else
    hipLaunchKernelGGL(k_design_scalars<OBHIP_DESIGN_MAXVAR>, dim3(1), dim3(256), 0, st, (int)p, d_b,
                       (const double *)d_sv, (const double *)d_hv, d_sh, d_scal, d_trace, step);
  hipLaunchKernelGGL(k_design_rank, dim3((unsigned)((p + 255) / 256), (unsigned)p), dim3(256), 0, st, (int)p, pp,
                     (const double *)d_sv, (const double *)d_hv, (const double *)d_scal, d_S, d_T);
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace obhip
