// The second-derivative twins of build_dim_dx / build_dim_tab_dx / build_dim_dx_any (device_dx.h):
// one dimension of the basis, of its derivative and of its SECOND derivative by that dimension's
// input, for one row.  No reference counterpart; the formulas are those of include/obhip.h at
// obhip_predict_hvp_multi_dev.  With R = cov . rotmat, R' = (dcov/dx) . rotmat, R'' = (d2cov/dx2) . rotmat
// a dimension hands over
//   r_t   = R_t / R_0                                   t >= 1
//   r'_t  = (R'_t - r_t R'_0) / R_0                     t >= 1
//   r''_t = (R''_t - 2 r'_t R'_0 - r_t R''_0) / R_0     t >= 1     store.put(compact column, r, r', r'')
//   R_0 (returned),  rho = R'_0 / R_0  and  kappa = R''_0 / R_0.
// The value and first-derivative sides follow build_dim_dx* operation for operation.
#pragma once
#include "device_dx.h"

namespace obhip {

// the tile of the Hessian-vector kernel, [column][PITCH], lane = row: Mu value columns (column 0 =
// ones), Mu first-derivative columns (column 0 = zeros), Mu second-derivative columns (column 0 =
// zeros), then d columns each of rho_l, kappa_l and the direction v_l
template <int PITCH>
struct StoreD2 {
  double *tile;
  const int *cpos;  // compact column -> used column or -1
  int lane, Mu, d;
  __device__ __forceinline__ void put(int ccol, double r, double dr, double d2r) const {
    const int u = cpos[ccol];
    if (u >= 0) {
      tile[u * PITCH + lane] = r;
      tile[(Mu + u) * PITCH + lane] = dr;
      tile[(2 * Mu + u) * PITCH + lane] = d2r;
    }
  }
  __device__ __forceinline__ void rho(int l, double v) const { tile[(3 * Mu + l) * PITCH + lane] = v; }
  __device__ __forceinline__ void kappa(int l, double v) const { tile[(3 * Mu + d + l) * PITCH + lane] = v; }
  __device__ __forceinline__ void dir(int l, double v) const { tile[(3 * Mu + 2 * d + l) * PITCH + lane] = v; }
};

// k(h), dk/du and d2k/du2 of one knot (kernel_value_dx with one more weight and no further exponential):
//   mat25 family  d2k/du2 = -(1/3) (1 + |h| - h^2) e^{-|h|}
//   mat25ang      d2k/dx2 = -(1/3) e^{-h} ((1 + h) q' - q^2),  q = hs cx - hc sx,
//                 q' = cx^2 + sx^2 - hs sin x / ls_s - hc cos x / ls_c      -- nothing divides by h
template <int KIND>
__device__ __forceinline__ void kernel_value_d2(double ka, double kb, double kc, double a0, double a1, double a2,
                                                double cx, double sx, double &kv, double &dkv, double &d2kv) {
  constexpr double third = 1.0 / 3.0;
  if (KIND == OBHIP_COV_MAT25ANG) {
    const double hs = a0 - ka, hc = a1 - kb;
    const double h = sqrt(hs * hs + hc * hc);
    const double eh = exp(-h);
    const double q = hs * cx - hc * sx;
    const double qp = cx * cx + sx * sx - hs * a0 - hc * a1;
    kv = (1.0 + h + h * h * third) * eh;
    dkv = -third * ((1.0 + h) * eh) * q;
    d2kv = -third * eh * ((1.0 + h) * qp - q * q);
  } else {
    const double dlt = a0 - ka;
    const double h = fabs(dlt);
    double eh;
    if (KIND == kCovMat25Direct || KIND == kCovMat25PowDirect)
      eh = exp(-h);
    else
      eh = dlt >= 0.0 ? a2 * kb : a1 * kc;
    kv = (1.0 + h + h * h * third) * eh;
    dkv = -third * (dlt * (1.0 + h) * eh);
    d2kv = -third * ((1.0 + h - h * h) * eh);
  }
}

// d2u/dx2 of the mat25 family: 0, or powv (powv - 1) x^powv / (expLS x^2)
template <int KIND>
__device__ __forceinline__ double d2udx2_of(const DimDesc &D, double xv, double tx) {
  if (KIND == OBHIP_COV_MAT25 || KIND == kCovMat25Direct) return 0.0;
  return D.p0 * (D.p0 - 1.0) * tx / (xv * xv);
}

template <int KIND, typename Store>
__device__ __forceinline__ double build_dim_d2(const DimDesc &D, const double *__restrict__ ka,
                                               const double *__restrict__ kb, const double *__restrict__ kc,
                                               const double *__restrict__ rot, double xv, const Store &store,
                                               double &rho, double &kappa) {
  double a0, a1, a2;
  kernel_pre<KIND>(D, xv, a0, a1, a2);
  double cx = 0.0, sx = 0.0, dudx = 1.0, d2udx = 0.0;
  if (KIND == OBHIP_COV_MAT25ANG) {
    cx = cos(xv) / D.p0;
    sx = sin(xv) / D.p1;
  } else {
    dudx = dudx_of<KIND>(D, xv, a0 + D.p2);
    d2udx = d2udx2_of<KIND>(D, xv, a0 + D.p2);
  }
  const double dudx2 = dudx * dudx;
  double cl = 1.0, dcl = 0.0, d2cl = 0.0;
  for (int c0 = 0; c0 < D.ncolp; c0 += 8) {
    double acc[8], dacc[8], d2acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = dacc[c] = d2acc[c] = 0.0;
    const double *rp = rot + D.rotoff + c0;
#pragma unroll 2
    for (int j = 0; j < D.m; ++j) {
      double kv, dkv, d2kv;
      kernel_value_d2<KIND>(ka[D.koff + j], kb[D.koff + j], kc[D.koff + j], a0, a1, a2, cx, sx, kv, dkv, d2kv);
      const double *r = rp + (size_t)j * D.ncolp;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        acc[c] = fma(kv, r[c], acc[c]);
        dacc[c] = fma(dkv, r[c], dacc[c]);
        d2acc[c] = fma(d2kv, r[c], d2acc[c]);
      }
    }
    if (c0 == 0) {
      cl = acc[0];
      dcl = dacc[0] * dudx;
      d2cl = fma(d2acc[0], dudx2, dacc[0] * d2udx);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int col = c0 + c;
      if (col >= 1 && col < D.ncol) {
        const double r = acc[c] / cl;
        const double dr = (dacc[c] * dudx - r * dcl) / cl;
        const double R2 = fma(d2acc[c], dudx2, dacc[c] * d2udx);
        store.put(D.ccol0 + col - 1, r, dr, (R2 - 2.0 * dr * dcl - r * d2cl) / cl);
      }
    }
  }
  rho = dcl / cl;
  kappa = d2cl / cl;
  return cl;
}

// mat25 / mat25pow from the interval tables: `d2tab` has the layout of `dtab` with the six sums of
// the SECOND derivative by u per (interval, level) (predict_hvp.cpp build_d2_tables_host: summed per
// knot in extended precision, not derived from the first-derivative polynomial),
//   d2R[c]/du2 = e^{-t} (A0'' + t (A1'' + t A2'')) + e^{+t} (B0'' + t (t B2'' - B1''));
// mat25pow applies the chain rule with both table results.
template <int KIND, typename Store>
__device__ __forceinline__ double build_dim_tab_d2(const DimDesc &D, const double *__restrict__ tab,
                                                   const double *__restrict__ dtab, const double *__restrict__ d2tab,
                                                   double xv, const Store &store, double &rho, double &kappa) {
  typedef double dd2 __attribute__((ext_vector_type(2)));
  const double tx = KIND == OBHIP_COV_MAT25 ? xv / D.p0 : pow(xv, D.p0) / D.p1;
  const double ux = tx - D.p2;
  const double dudx = dudx_of<KIND>(D, xv, tx);
  const double d2udx = d2udx2_of<KIND>(D, xv, tx);
  const double dudx2 = dudx * dudx;
  const double *__restrict__ us = tab + D.tab;
  int J;
  double uref;
  tab_locate(D, us, ux, J, uref);
  const double t = ux - uref;
  const double em = J == 0 ? 0.0 : exp(-t), ep = J == D.m ? 0.0 : exp(t);
  const size_t eoff = (size_t)D.tab + ((D.m + 1) & ~1) + (size_t)J * D.ncol * 6;
  const dd2 *__restrict__ cf = (const dd2 *)(tab + eoff);
  const dd2 *__restrict__ df = (const dd2 *)(dtab + eoff);
  const dd2 *__restrict__ sf = (const dd2 *)(d2tab + eoff);
  double cl = 1.0, icl = 1.0, dcl = 0.0, d2cl = 0.0;
  for (int c = 0; c < D.ncol; ++c) {
    const dd2 e0 = cf[3 * c], e1 = cf[3 * c + 1], e2 = cf[3 * c + 2];  // A0 A1 | A2 B0 | B1 B2
    const dd2 f0 = df[3 * c], f1 = df[3 * c + 1], f2 = df[3 * c + 2];
    const dd2 g0 = sf[3 * c], g1 = sf[3 * c + 1], g2 = sf[3 * c + 2];
    const double r = em * fma(t, fma(t, e1.x, e0.y), e0.x) + ep * fma(t, fma(t, e2.y, -e2.x), e1.y);
    const double du = em * fma(t, fma(t, f1.x, f0.y), f0.x) + ep * fma(t, fma(t, f2.y, -f2.x), f1.y);
    const double d2u = em * fma(t, fma(t, g1.x, g0.y), g0.x) + ep * fma(t, fma(t, g2.y, -g2.x), g1.y);
    const double dr = du * dudx;
    const double d2r = fma(d2u, dudx2, du * d2udx);
    if (c == 0) {
      cl = r;
      icl = 1.0 / r;
      dcl = dr;
      d2cl = d2r;
    } else {
      const double rr = r * icl;
      const double drr = (dr - rr * dcl) * icl;
      store.put(D.ccol0 + c - 1, rr, drr, (d2r - 2.0 * drr * dcl - rr * d2cl) * icl);
    }
  }
  rho = dcl * icl;
  kappa = d2cl * icl;
  return cl;
}

template <typename Store>
__device__ __forceinline__ double build_dim_d2_any(const DimDesc &D, const double *ka, const double *kb,
                                                   const double *kc, const double *rot, const double *tab,
                                                   const double *dtab, const double *d2tab, double xv,
                                                   const Store &store, double &rho, double &kappa) {
  if (D.tab >= 0) {
    if (D.kind == OBHIP_COV_MAT25)
      return build_dim_tab_d2<OBHIP_COV_MAT25>(D, tab, dtab, d2tab, xv, store, rho, kappa);
    return build_dim_tab_d2<OBHIP_COV_MAT25POW>(D, tab, dtab, d2tab, xv, store, rho, kappa);
  }
  if (D.kind == OBHIP_COV_MAT25) return build_dim_d2<OBHIP_COV_MAT25>(D, ka, kb, kc, rot, xv, store, rho, kappa);
  if (D.kind == OBHIP_COV_MAT25POW)
    return build_dim_d2<OBHIP_COV_MAT25POW>(D, ka, kb, kc, rot, xv, store, rho, kappa);
  if (D.kind == kCovMat25Direct)
    return build_dim_d2<kCovMat25Direct>(D, ka, kb, kc, rot, xv, store, rho, kappa);
  if (D.kind == kCovMat25PowDirect)
    return build_dim_d2<kCovMat25PowDirect>(D, ka, kb, kc, rot, xv, store, rho, kappa);
  return build_dim_d2<OBHIP_COV_MAT25ANG>(D, ka, kb, kc, rot, xv, store, rho, kappa);
}

}  // namespace obhip
