// One row of the GLM row pass (kernels_glm.hip): from the linear predictor eta, the response y and the
// prior weight a to the mean, the square root of the IRLS weight, the working value u and the row's
// part of the log-likelihood.  Plain C++17 with nothing from HIP, so that a host program can check the
// formulas (tests/glm_rows_check.cpp); the kernels call the same functions.
#pragma once
#include <cmath>

#include "../../include/obhip.h"

#if defined(__HIPCC__)
#define OBHIP_GLM_HD __host__ __device__
#else
#define OBHIP_GLM_HD
#endif

namespace obhip {

// mu, d mu / d eta, and b(eta) of l = y eta - b(eta); the binomial forms are free of overflow
template <int FAMILY>
OBHIP_GLM_HD inline void glm_link(double eta, double &mu, double &dmu, double &b) {
  if constexpr (FAMILY == OBHIP_GLM_BINOMIAL) {
    const double e = std::exp(-std::fabs(eta)), d = 1.0 + e;
    mu = eta >= 0.0 ? 1.0 / d : e / d;
    dmu = e / (d * d);
    b = std::fmax(eta, 0.0) + std::log1p(e);
  } else if constexpr (FAMILY == OBHIP_GLM_POISSON) {
    mu = std::exp(eta);
    dmu = mu;
    b = mu;
  } else {
    mu = eta;
    dmu = 1.0;
    b = 0.0;
  }
}

struct GlmRow {
  double mu, sw, u;  // mean, sqrt(w) (0: the row takes no part), a (y - mu) (Gaussian: e2) / sqrt(w)
  double al, mag;    // a l and the magnitude a (|y eta| + |b|) it is summed of (Gaussian: a |l|)
  bool finite;       // both are finite: the row enters the sums, otherwise it is counted
};

// e2 = e^{-2 sigma}, read by the Gaussian family only
template <int FAMILY>
OBHIP_GLM_HD inline GlmRow glm_row(double eta, double y, double a, double e2) {
  GlmRow r;
  double dmu, b, l, w, res;
  glm_link<FAMILY>(eta, r.mu, dmu, b);
  if constexpr (FAMILY == OBHIP_GLM_GAUSSIAN) {
    const double d = y - eta;
    l = -0.5 * e2 * d * d;
    r.mag = a * std::fabs(l);
    w = a * e2;
    res = a * d * e2;
  } else {
    const double ye = y * eta;
    l = ye - b;
    r.mag = a * (std::fabs(ye) + std::fabs(b));
    w = a * dmu;
    res = a * (y - r.mu);
  }
  r.al = a * l;
  r.finite = std::isfinite(r.al) && std::isfinite(r.mag);
  // w = 0 (binomial beyond |eta| = 745, Poisson below -745) or not finite: the row takes no part
  const bool live = w > 0.0 && std::isfinite(w);
  r.sw = live ? std::sqrt(w) : 0.0;
  r.u = live ? res / r.sw : 0.0;
  return r;
}

}  // namespace obhip
