// The raw twins of build_dim_dx / build_dim_tab_dx / build_dim_dx_any (device_dx.h): one dimension of the
// basis and of its derivative by that dimension's input for one row, NOT normalised by level 0:
//   val[t * nt] = R_t  = (cov(x, knots) . rotmat)[t]
//   der[t * nt] = R'_t = ((dcov/dx) . rotmat)[t]            t = 0 .. D.ncol - 1, level 0 included
// in raw input units.  The gradient-moment tables (kernels_active.hip) are sums of w R'_a R_b and w R'_a R'_b;
// the normalised builders hand over r'_t = (R'_t - r_t R'_0) / R_0, and R'_t put together again from that adds
// back what was just subtracted.  The knot sums and the table polynomials are those of device_dx.h, through
// the same kernel_pre, kernel_value_dx, dudx_of and tab_locate; the builders there are untouched.
#pragma once
#include "device_dx.h"

namespace obhip {

// the knot loop
template <int KIND>
__device__ __forceinline__ void build_dim_raw_dx(const DimDesc &D, const double *__restrict__ ka,
                                                 const double *__restrict__ kb, const double *__restrict__ kc,
                                                 const double *__restrict__ rot, double xv, double *val, double *der,
                                                 int nt) {
  double a0, a1, a2;
  kernel_pre<KIND>(D, xv, a0, a1, a2);
  double cx = 0.0, sx = 0.0, dudx = 1.0;
  if (KIND == OBHIP_COV_MAT25ANG) {
    cx = cos(xv) / D.p0;
    sx = sin(xv) / D.p1;
  } else {
    dudx = dudx_of<KIND>(D, xv, a0 + D.p2);
  }
  for (int c0 = 0; c0 < D.ncolp; c0 += 8) {
    double acc[8], dacc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = dacc[c] = 0.0;
    const double *rp = rot + D.rotoff + c0;
#pragma unroll 2
    for (int j = 0; j < D.m; ++j) {
      double kv, dkv;
      kernel_value_dx<KIND>(ka[D.koff + j], kb[D.koff + j], kc[D.koff + j], a0, a1, a2, cx, sx, kv, dkv);
      const double *r = rp + (size_t)j * D.ncolp;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        acc[c] = fma(kv, r[c], acc[c]);
        dacc[c] = fma(dkv, r[c], dacc[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int col = c0 + c;
      if (col < D.ncol) {
        val[(size_t)col * nt] = acc[c];
        der[(size_t)col * nt] = dacc[c] * dudx;
      }
    }
  }
}

// mat25 / mat25pow from the interval tables; dtab: obhip_terms::Dx::dtab (ensure_dx_tables)
template <int KIND>
__device__ __forceinline__ void build_dim_tab_raw_dx(const DimDesc &D, const double *__restrict__ tab,
                                                     const double *__restrict__ dtab, int dtab_off, double xv,
                                                     double *val, double *der, int nt) {
  typedef double dd2 __attribute__((ext_vector_type(2)));
  const double tx = KIND == OBHIP_COV_MAT25 ? xv / D.p0 : pow(xv, D.p0) / D.p1;
  const double ux = tx - D.p2;
  const double dudx = dudx_of<KIND>(D, xv, tx);
  const double *__restrict__ us = tab + D.tab;
  int J;
  double uref;
  tab_locate(D, us, ux, J, uref);
  const double t = ux - uref;
  const double em = J == 0 ? 0.0 : exp(-t), ep = J == D.m ? 0.0 : exp(t);
  const size_t erel = ((D.m + 1) & ~1) + (size_t)J * D.ncol * 6;
  const dd2 *__restrict__ cf = (const dd2 *)(tab + D.tab + erel);
  const dd2 *__restrict__ df = (const dd2 *)(dtab + dtab_off + erel);
  for (int c = 0; c < D.ncol; ++c) {
    const dd2 e0 = cf[3 * c], e1 = cf[3 * c + 1], e2 = cf[3 * c + 2];  // A0 A1 | A2 B0 | B1 B2
    const dd2 f0 = df[3 * c], f1 = df[3 * c + 1], f2 = df[3 * c + 2];
    val[(size_t)c * nt] = em * fma(t, fma(t, e1.x, e0.y), e0.x) + ep * fma(t, fma(t, e2.y, -e2.x), e1.y);
    der[(size_t)c * nt] = (em * fma(t, fma(t, f1.x, f0.y), f0.x) + ep * fma(t, fma(t, f2.y, -f2.x), f1.y)) * dudx;
  }
}

// tab / D.tab may point at a copy of the dimension's value tables (LDS, D.tab = 0); dtab_off is the
// dimension's offset in dtab, the D.tab of the model's own descriptor
__device__ __forceinline__ void build_dim_raw_dx_any(const DimDesc &D, const double *ka, const double *kb,
                                                     const double *kc, const double *rot, const double *tab,
                                                     const double *dtab, int dtab_off, double xv, double *val,
                                                     double *der, int nt) {
  if (D.tab >= 0) {
    if (D.kind == OBHIP_COV_MAT25) return build_dim_tab_raw_dx<OBHIP_COV_MAT25>(D, tab, dtab, dtab_off, xv, val, der, nt);
    return build_dim_tab_raw_dx<OBHIP_COV_MAT25POW>(D, tab, dtab, dtab_off, xv, val, der, nt);
  }
  if (D.kind == OBHIP_COV_MAT25) return build_dim_raw_dx<OBHIP_COV_MAT25>(D, ka, kb, kc, rot, xv, val, der, nt);
  if (D.kind == OBHIP_COV_MAT25POW) return build_dim_raw_dx<OBHIP_COV_MAT25POW>(D, ka, kb, kc, rot, xv, val, der, nt);
  if (D.kind == kCovMat25Direct) return build_dim_raw_dx<kCovMat25Direct>(D, ka, kb, kc, rot, xv, val, der, nt);
  if (D.kind == kCovMat25PowDirect)
    return build_dim_raw_dx<kCovMat25PowDirect>(D, ka, kb, kc, rot, xv, val, der, nt);
  return build_dim_raw_dx<OBHIP_COV_MAT25ANG>(D, ka, kb, kc, rot, xv, val, der, nt);
}

}  // namespace obhip
