// Kernels of the acquisition picks (acquire.cpp; include/obhip.h, "acquisition picks").
// No reference counterpart: the reference package fits and predicts, it does not choose the next runs.
//
// One step conditions the posterior on a fantasised run at the picked row j and scores every candidate
// for the next pick.  With S = inv(H), nu = e^{2 sigma}, s = S b_j, gamma = nu + b_j^T s, a_i = b_i^T s (the
// one-response predictor's pass with s for coefficients, in HBM) and delta = y* - mu_j:
//     mu_i <- mu_i + a_i delta / gamma        d_i <- d_i - a_i^2 / gamma
//     sd = sqrt(max(d, 0)), t = best - xi - mu, u = t / sd
//     EI t Phi(u) + sd phi(u) | PI Phi(u) | LCB kappa sd - mu | STRADDLE kappa sd - |mu - level|
// scored on sgn * mu (sgn = -1: maximize; best and level come in that sign already).
//
//   k_acq_update  256 rows per workgroup, lane = row: the two downdates, the score in FP64, a wave butterfly
//                 and four LDS words -> one (best score, lowest index among equals) pair per workgroup.
//   k_acq_pick    one workgroup: the partial pairs lane-strided in ascending order, an LDS tree with the
//                 order-independent comparison, the pick appended and marked, x_j gathered, y*, delta and
//                 the new incumbent formed for the next pass.
// Every sum and every argmax runs in a fixed order; the hand-overs are kernel boundaries.
#include <cmath>

#include "obhip_internal.h"
#include "acquire_device.h"

namespace obhip {

namespace {

template <int CRIT>
__global__ void __launch_bounds__(256)
k_acq_update(uint64_t n, const double *__restrict__ a, const double *__restrict__ scal, double sgn, double xi,
             double kappa, double level, const uint8_t *__restrict__ elig, const uint8_t *__restrict__ picked,
             double *__restrict__ mu, double *__restrict__ dvar, double *__restrict__ score0,
             double *__restrict__ part_score, int64_t *__restrict__ part_idx) {
  __shared__ double ws[4];
  __shared__ int64_t wi[4];
  const uint64_t row = (uint64_t)blockIdx.x * kAcqRows + threadIdx.x;
  double score = -INFINITY;
  int64_t idx = kNoIndex;
  if (row < n) {
    const double gamma = scal[0], delta = scal[kAcqDelta], best = scal[kAcqBest];
    const double ai = a[row], ag = ai / gamma;
    const double m = mu[row] + ag * delta;
    const double d = dvar[row] - ai * ag;
    mu[row] = m;
    dvar[row] = d;
    const double sc = acq_score<CRIT>(sgn * m, d, best, xi, kappa, level);
    if (score0) score0[row] = sc;
    if (elig[row] && !picked[row] && isfinite(sc)) {
      score = sc;
      idx = (int64_t)row;
    }
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

// scal: [0] gamma, [3] nu, [5] 1 = no eligible candidate was left (the design step's block), [kAcqDelta] delta,
// [kAcqBest] the incumbent
__global__ void __launch_bounds__(256)
k_acq_pick(const double *__restrict__ part_score, const int64_t *__restrict__ part_idx, uint64_t nparts,
           const double *__restrict__ x, uint64_t n, int d, uint64_t step, const double *__restrict__ mu, int moves_best,
           int lie, double lie_value, double sgn, int64_t *__restrict__ index, double *__restrict__ score_out,
           double *__restrict__ xj, uint8_t *__restrict__ picked, double *__restrict__ scal) {
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
    const double muj = mu[idx];
    const double ystar = lie == OBHIP_LIE_CONSTANT ? lie_value : muj;
    scal[kAcqDelta] = ystar - muj;
    if (moves_best) scal[kAcqBest] = fmin(scal[kAcqBest], sgn * ystar);
  }
  for (int l = threadIdx.x; l < d; l += 256) xj[l] = x[(uint64_t)l * n + (uint64_t)idx];
}

template <int CRIT>
void run_acq_update(const AcqStep &s, double *d_score0) {
  hipLaunchKernelGGL(k_acq_update<CRIT>, dim3((unsigned)((s.n + kAcqRows - 1) / kAcqRows)), dim3(256), 0, cur_stream(),
                     s.n, s.a, (const double *)s.scal, s.sgn, s.xi, s.kappa, s.level, s.elig, (const uint8_t *)s.picked,
                     s.mu, s.dvar, d_score0, s.part_score, s.part_idx);
}

}  // namespace

int launch_acq_update(const AcqStep &s, double *d_score0) {
  ProfScope ps("acq_update");
  switch (s.crit) {
    case OBHIP_ACQ_EI: run_acq_update<OBHIP_ACQ_EI>(s, d_score0); break;
    case OBHIP_ACQ_PI: run_acq_update<OBHIP_ACQ_PI>(s, d_score0); break;
    case OBHIP_ACQ_LCB: run_acq_update<OBHIP_ACQ_LCB>(s, d_score0); break;
    case OBHIP_ACQ_STRADDLE: run_acq_update<OBHIP_ACQ_STRADDLE>(s, d_score0); break;
    default: return fail(OBHIP_ERR_INVALID, "acquire: no kernel for this criterion");
  }
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_acq_pick(const AcqStep &s, uint64_t d, uint64_t step, int64_t *d_index, double *d_score, double *d_xj) {
  ProfScope ps("acq_pick");
  const int moves_best = s.crit == OBHIP_ACQ_EI || s.crit == OBHIP_ACQ_PI;
  hipLaunchKernelGGL(k_acq_pick, dim3(1), dim3(256), 0, cur_stream(), (const double *)s.part_score,
                     (const int64_t *)s.part_idx, (s.n + kAcqRows - 1) / kAcqRows, s.x, s.n, (int)d, step,
                     (const double *)s.mu, moves_best, s.lie, s.lie_value, s.sgn, d_index, d_score, d_xj, s.picked, s.scal);
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace obhip
