// Term-count path (include/obhip.h, "term-count path"; no reference counterpart).
//
//   k_term_path        one workgroup per 128-row tile of the stored Z = B X (row-major, X = L^-T upper triangular, so
//                      z_ij depends on terms 1 .. j only): 128 x 32 column tiles go through LDS -- global reads
//                      coalesced along the terms, the next tile in flight while this one is walked -- and one lane
//                      owns one row.  It walks the row's columns strictly ascending with v = sum z_j^2 and, per
//                      response of the block, m = sum z_j U_j in registers; at a checkpoint column it forms r, e, s^2
//                      and the row's (sse, spe, lpd) per response and v, which the tile sums in a fixed lane order:
//                      the butterfly of each wave, then wave 0 + wave 1.  One logarithm per (row, checkpoint): s^2
//                      does not depend on the response.
//   k_term_path_fold   a chunk's tile sums added to their groups' in ascending tile order: group g holds tiles
//                      64 g .. 64 g + 63 OF THE CALL, so a group's sum is one ascending sum whatever the chunks are
//   k_term_path_final  the group sums added in ascending order: the two-stage rule of vec_ops.h, no atomics
//   k_term_path_coef   U = X^T G, k_term_path_theta  Theta_k = X[:k,:k] U[:k]: one ascending sum per entry, both with
//                      their global reads along the rows of X
#include "obhip_internal.h"
#include "term_path_plan.h"

namespace obhip {
namespace {

constexpr int TR = (int)kTpTileRows, TC = (int)kTpTileCols, PITCH = (int)kTpPitch, RB = (int)kTpRespBlock;
constexpr int NV = 3 * RB + 1;          // values a row adds at a checkpoint
constexpr int PRE = TC;                 // doubles of the next tile a lane holds in flight: 32
static_assert(TR * TC == TR * PRE, "the lanes' PRE doubles are the tile");
constexpr double kLog2Pi = 1.8378770664093454835606594728112;

template <int LOO>
__global__ void __launch_bounds__(TR)
k_term_path(const double *__restrict__ Z, uint64_t ldz, uint64_t nr, uint64_t p, uint64_t step, uint64_t q, uint64_t K,
            const double *__restrict__ U, uint64_t j0, int nresp, const double *__restrict__ Y, uint64_t ldy,
            const double *__restrict__ meansd, double nu, uint64_t entries, double *__restrict__ part) {
  __shared__ double zt[TR * PITCH];
  __shared__ double us[RB][TC];
  __shared__ double red[2][NV];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint64_t row0 = (uint64_t)blockIdx.x * TR, row = row0 + tid;
  const bool live = row < nr;
  double y[RB], m[RB], v = 0.0;
#pragma unroll
  for (int c = 0; c < RB; ++c) {
    m[c] = 0.0;
    y[c] = 0.0;
    if (live && c < nresp) {
      const double raw = Y[(j0 + c) * ldy + row];
      y[c] = meansd ? (raw - meansd[3 * (j0 + c)]) / meansd[3 * (j0 + c) + 1] : raw;
    }
  }
  // staging: lane (lr, lc) moves column lc of rows lr, lr + 4, ...: 32 lanes read 256 contiguous bytes of a row
  const int lc = tid % TC, lr = tid / TC;
  constexpr int RSTEP = TR / TC;
  double pre[PRE];
  const double *zsrc = Z + (row0 + lr) * ldz + lc;  // (Z has pad128 rows and pad128(p) columns: every read is inside)
#pragma unroll
  for (int i = 0; i < PRE; ++i) pre[i] = zsrc[(uint64_t)(i * RSTEP) * ldz];
  double *mine = part + (uint64_t)blockIdx.x * entries;
  uint64_t next = p > step ? step : p, cidx = 0;
  int par = 0;
  for (uint64_t c0 = 0; c0 < p; c0 += TC) {
    __syncthreads();  // the walk of the tile before is over
#pragma unroll
    for (int i = 0; i < PRE; ++i) zt[(lr + i * RSTEP) * PITCH + lc] = pre[i];
    for (int e = tid; e < RB * TC; e += TR) {
      const int c = e / TC, jj = e % TC;
      us[c][jj] = (c < nresp && c0 + jj < p) ? U[(j0 + c) * p + c0 + jj] : 0.0;
    }
    __syncthreads();
    if (c0 + TC < p) {
#pragma unroll
      for (int i = 0; i < PRE; ++i) pre[i] = zsrc[(uint64_t)(i * RSTEP) * ldz + c0 + TC];
    }
    const int jend = (int)(p - c0 < (uint64_t)TC ? p - c0 : (uint64_t)TC);
    for (int jj = 0; jj < jend; ++jj) {
      const double z = zt[tid * PITCH + jj];
      v = fma(z, z, v);
#pragma unroll
      for (int c = 0; c < RB; ++c) m[c] = fma(z, us[c][jj], m[c]);
      if (c0 + jj + 1 != next) continue;  // (uniform over the workgroup)
      // ---- checkpoint k = next ----
      double val[NV];
      const double om = 1.0 - v / nu;                    // 1 - h
      const double s2 = LOO ? nu / om : nu + v;
      const double lg = -0.5 * (kLog2Pi + log(s2));
#pragma unroll
      for (int c = 0; c < RB; ++c) {
        const double r = y[c] - m[c], e = LOO ? r / om : r;
        val[3 * c] = r * r;
        val[3 * c + 1] = e * e;
        val[3 * c + 2] = lg - 0.5 * (e * e) / s2;
      }
      val[NV - 1] = v;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        double s = live ? val[i] : 0.0;  // the padding rows of the last tile are in no sum
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        val[i] = s;
      }
      if (wave == 1 && lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) red[par][i] = val[i];
      }
      __syncthreads();  // red[par] is next written two checkpoints on: wave 0 has read it before the barrier between
      if (wave == 0 && lane == 0) {
        for (int c = 0; c < nresp; ++c)
          for (int s = 0; s < 3; ++s) mine[((cidx * q) + j0 + c) * 3 + s] = val[3 * c + s] + red[par][3 * c + s];
        if (j0 == 0) mine[K * q * 3 + cidx] = val[NV - 1] + red[par][NV - 1];
      }
      par ^= 1;
      ++cidx;
      next = p - next > step ? next + step : p;
    }
  }
}

__global__ void __launch_bounds__(256)
k_term_path_fold(const double *__restrict__ part, uint64_t ctiles, uint64_t tile0, uint64_t entries,
                 double *__restrict__ groups) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  uint64_t g = tile0 / kTpGroup;
  double s = groups[g * entries + e];
  for (uint64_t t = 0; t < ctiles; ++t) {
    const uint64_t gt = (tile0 + t) / kTpGroup;
    if (gt != g) {
      groups[g * entries + e] = s;
      g = gt;
      s = groups[g * entries + e];
    }
    s += part[t * entries + e];
  }
  groups[g * entries + e] = s;
}

__global__ void __launch_bounds__(256)
k_term_path_final(const double *__restrict__ groups, uint64_t ngroups, uint64_t entries, uint64_t nscore,
                  double *__restrict__ scores, double *__restrict__ sumv) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  double s = 0.0;
  for (uint64_t g = 0; g < ngroups; ++g) s += groups[g * entries + e];
  if (e < nscore)
    scores[e] = s;
  else
    sumv[e - nscore] = s;
}

// U_jc = sum_{i <= j} X_ij G_ic: lanes along j, so a step of i reads consecutive entries of a row of X
__global__ void __launch_bounds__(256)
k_term_path_coef(const double *__restrict__ X, uint64_t p, uint64_t pp, const double *__restrict__ G, uint64_t q,
                 double *__restrict__ U) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= p * q) return;
  const uint64_t j = e % p, c = e / p;
  double s = 0.0;
  for (uint64_t i = 0; i <= j; ++i) s = fma(X[i * pp + j], G[c * p + i], s);
  U[e] = s;
}

// Theta_ic = sum_{i <= j < k} X_ij U_jc, zeros from row k on.  One wave per 64 rows i and response c (blockIdx.y): the
// sum runs along a row of X, so 64 x 64 tiles of X go through LDS -- read with the lanes along j, 512 contiguous bytes
// of a row, and walked with one lane per row i (pitch 65 doubles: no two lanes of a half wave on one bank) -- and every
// entry is still one ascending sum over j.  (X has pad128(p) rows and columns: every tile read is inside.)
constexpr int TT = 64;
__global__ void __launch_bounds__(TT)
k_term_path_theta(const double *__restrict__ X, uint64_t p, uint64_t pp, const double *__restrict__ U, uint64_t k,
                  double *__restrict__ Theta) {
  __shared__ double xt[TT * (TT + 1)];
  __shared__ double us[TT];
  const int lane = threadIdx.x;
  const uint64_t i0 = (uint64_t)blockIdx.x * TT, i = i0 + lane, c = blockIdx.y;
  double s = 0.0;
  for (uint64_t j0 = i0; j0 < k; j0 += TT) {  // (tiles left of the diagonal tile hold zeros only)
    __syncthreads();
    for (int r = 0; r < TT; ++r) xt[r * (TT + 1) + lane] = X[(i0 + r) * pp + j0 + lane];
    us[lane] = j0 + lane < k ? U[c * p + j0 + lane] : 0.0;
    __syncthreads();
    const int jend = (int)(k - j0 < (uint64_t)TT ? k - j0 : (uint64_t)TT);
    for (int jj = 0; jj < jend; ++jj)
      if (j0 + jj >= i) s = fma(xt[lane * (TT + 1) + jj], us[jj], s);
  }
  if (i < p) Theta[c * p + i] = i < k ? s : 0.0;
}

unsigned blocks256(uint64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

int launch_term_path(const TermPathPlan &plan, const double *d_Z, uint64_t nr, uint64_t npad, const double *d_U,
                     uint64_t j0, uint64_t nresp, const double *d_Y, uint64_t ldy, const double *d_meansd, double nu,
                     int loo, double *d_part) {
  if (nresp == 0 || nresp > kTpRespBlock || j0 + nresp > plan.q || nr == 0 || nr > npad || npad % kTpTileRows)
    return fail(OBHIP_ERR_INVALID, "launch_term_path: bad response block or rows");
  const dim3 grid((unsigned)(npad / kTpTileRows)), block(TR);
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, cur_stream(), d_Z, plan.pp(), nr, plan.p, plan.step, plan.q, plan.K(),
                       d_U, j0, (int)nresp, d_Y, ldy, d_meansd, nu, plan.entries(), d_part);
  };
  if (loo)
    go(k_term_path<1>);
  else
    go(k_term_path<0>);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_term_path_fold(const TermPathPlan &plan, const double *d_part, uint64_t ctiles, uint64_t tile0,
                          double *d_groups) {
  const uint64_t E = plan.entries();
  hipLaunchKernelGGL(k_term_path_fold, dim3(blocks256(E)), dim3(256), 0, cur_stream(), d_part, ctiles, tile0, E,
                     d_groups);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_term_path_final(const TermPathPlan &plan, const double *d_groups, double *d_scores, double *d_sumv) {
  const uint64_t E = plan.entries();
  hipLaunchKernelGGL(k_term_path_final, dim3(blocks256(E)), dim3(256), 0, cur_stream(), d_groups, plan.groups(), E,
                     plan.score_entries(), d_scores, d_sumv);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_term_path_coef(const double *d_X, uint64_t p, uint64_t pp, const double *d_G, uint64_t q, double *d_U) {
  hipLaunchKernelGGL(k_term_path_coef, dim3(blocks256(p * q)), dim3(256), 0, cur_stream(), d_X, p, pp, d_G, q, d_U);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_term_path_theta(const double *d_X, uint64_t p, uint64_t pp, const double *d_U, uint64_t q, uint64_t k,
                           double *d_Theta) {
  hipLaunchKernelGGL(k_term_path_theta, dim3((unsigned)((p + TT - 1) / TT), (unsigned)q), dim3(TT), 0, cur_stream(), d_X,
                     p, pp, d_U, k, d_Theta);  // (q <= 65534: within the grid's y)
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace obhip
