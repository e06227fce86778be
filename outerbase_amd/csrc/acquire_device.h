// The acquisition criteria on the device, once (kernels_acquire.hip scores with them, kernels_acquire_dx.hip
// differentiates them; DESIGN.md sections 22, 32 and 34).  Scored on the signed mean ms = sgn * mu (sgn = -1:
// maximize; best and level come in that sign already) and the latent variance dv:
//     sd = sqrt(max(dv, 0)), t = best - xi - ms, u = t / sd
//     EI t Phi(u) + sd phi(u) | PI Phi(u) | LCB kappa sd - ms | STRADDLE kappa sd - |ms - level|
#pragma once
#include <cmath>

#include "../../include/obhip.h"

namespace obhip {

// the score, and the coefficients of its gradient: d score = A d(ms) + C d(sd)
template <int CRIT>
__device__ __forceinline__ double acq_eval(double ms, double dv, double best, double xi, double kappa, double level,
                                           double &A, double &C) {
  const double sd = sqrt(fmax(dv, 0.0));
  if (CRIT == OBHIP_ACQ_LCB) {
    A = -1.0;
    C = kappa;
    return kappa * sd - ms;
  }
  if (CRIT == OBHIP_ACQ_STRADDLE) {
    const double df = ms - level;
    A = df > 0.0 ? -1.0 : (df < 0.0 ? 1.0 : (df == 0.0 ? 0.0 : NAN));
    C = kappa;
    return kappa * sd - fabs(df);
  }
  const double t = best - xi - ms;
  if (!(sd > 0.0)) {
    C = 0.0;
    if (sd != sd || t != t) {
      A = C = NAN;
      return NAN;
    }
    if (CRIT == OBHIP_ACQ_PI) {
      A = 0.0;
      return t > 0.0 ? 1.0 : 0.0;
    }
    A = t > 0.0 ? -1.0 : 0.0;
    return fmax(t, 0.0);
  }
  const double u = t / sd;
  const double Phi = 0.5 * erfc(-u * 0.70710678118654752440);
  const double phi = exp(-0.5 * u * u) * 0.39894228040143267794;
  if (CRIT == OBHIP_ACQ_PI) {
    A = -phi / sd;
    C = -(phi * u) / sd;
    return Phi;
  }
  A = -Phi;
  C = phi;
  return t * Phi + sd * phi;
}

// the score alone
template <int CRIT>
__device__ __forceinline__ double acq_score(double ms, double dv, double best, double xi, double kappa, double level) {
  double A, C;
  return acq_eval<CRIT>(ms, dv, best, xi, kappa, level, A, C);
}

// the argmax of the pick kernels (kernels_acquire.hip, kernels_acquire_multi.hip): one comparison everywhere, so the
// result does not depend on the order in which pairs meet
constexpr int64_t kNoIndex = INT64_MAX;

// (score, index) a beats b: the larger score, the lower index among equals
__device__ __forceinline__ bool beats(double sa, int64_t ia, double sb, int64_t ib) {
  return sa > sb || (sa == sb && ia < ib);
}

// the 64 lanes of a wave -> every lane holds the wave's best pair
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

}  // namespace obhip
