// What the predictors share on the device beyond device_common.h.
//
// 1. The derivative twins of build_dim / build_dim_tab / build_dim_any: one dimension of the basis
//    AND of its derivative by that dimension's input, for one row.  No reference counterpart (the
//    reference has no input gradients); the formulas are those of include/obhip.h at
//    obhip_predict_grad_dev.  With R = cov(x, knots) . rotmat and R' = (dcov/dx) . rotmat a
//    dimension hands over
//      r_t  = R_t / R_0                       t >= 1   store.val(compact column, .)
//      r'_t = (R'_t - r_t R'_0) / R_0         t >= 1   store.der(compact column, .)
//      R_0  (returned)   and   rho = R'_0 / R_0.
//    The value side follows build_dim* operation for operation; the interval search is the one
//    function both call (tab_locate).
// 2. Phase 1 of every fused predictor (build_tile, tile_scale): the basis -- with or without its
//    derivative -- at the 64 rows of a tile, written into the tile by the waves of the block.
#pragma once
#include "device_common.h"

namespace obhip {

// k(h) and dk/du of one knot, u the transformed input (mat25 family: the caller multiplies the
// knot sum by du/dx) or x itself (mat25ang; cx = cos x / ls_s, sx = sin x / ls_c):
//   mat25 family  dk/du = -(1/3) (u - u_j) (1 + |u - u_j|) e^{-|u - u_j|}
//   mat25ang      dk/dx = -(1/3) (1 + h) e^{-h} (hs cx - hc sx)      -- (k'(h) / h) (h dh/dx): no division by h
template <int KIND>
__device__ __forceinline__ void kernel_value_dx(double ka, double kb, double kc, double a0, double a1,
                                                double a2, double cx, double sx, double &kv, double &dkv) {
  constexpr double third = 1.0 / 3.0;
  if (KIND == OBHIP_COV_MAT25ANG) {
    const double hs = a0 - ka, hc = a1 - kb;
    const double h = sqrt(hs * hs + hc * hc);
    const double eh = exp(-h);
    kv = (1.0 + h + h * h * third) * eh;
    dkv = -third * ((1.0 + h) * eh) * (hs * cx - hc * sx);
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
  }
}

// du/dx of the mat25 family: 1 / expLS, or powv x^powv / (expLS x) (t = x^powv / expLS)
template <int KIND>
__device__ __forceinline__ double dudx_of(const DimDesc &D, double xv, double tx) {
  if (KIND == OBHIP_COV_MAT25 || KIND == kCovMat25Direct) return 1.0 / D.p0;
  return D.p0 * tx / xv;
}

// the knot loop: one exp per knot (direct kinds, mat25ang) or the separable pair
template <int KIND, typename Store>
__device__ __forceinline__ double build_dim_dx(const DimDesc &D, const double *__restrict__ ka,
                                               const double *__restrict__ kb, const double *__restrict__ kc,
                                               const double *__restrict__ rot, double xv, const Store &store,
                                               double &rho) {
  double a0, a1, a2;
  kernel_pre<KIND>(D, xv, a0, a1, a2);
  double cx = 0.0, sx = 0.0, dudx = 1.0;
  if (KIND == OBHIP_COV_MAT25ANG) {
    cx = cos(xv) / D.p0;
    sx = sin(xv) / D.p1;
  } else {
    dudx = dudx_of<KIND>(D, xv, a0 + D.p2);
  }
  double cl = 1.0, dcl = 0.0;
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
    if (c0 == 0) {
      cl = acc[0];
      dcl = dacc[0] * dudx;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int col = c0 + c;
      if (col >= 1 && col < D.ncol) {
        const double r = acc[c] / cl;
        store.val(D.ccol0 + col - 1, r);
        store.der(D.ccol0 + col - 1, (dacc[c] * dudx - r * dcl) / cl);
      }
    }
  }
  rho = dcl / cl;
  return cl;
}

// mat25 / mat25pow from the interval tables.  `tab` are ModelDev's; `dtab` has the same layout (its
// sorted-knot part unused) with the six sums of the DERIVATIVE by u per (interval, level):
//   dR[c]/du = e^{-t} (A0' + t (A1' + t A2')) + e^{+t} (B0' + t (t B2' - B1'))
// (csrc/predict_dx.cpp build_dx_tables: summed per knot in extended precision, so nothing cancels
// here that does not cancel in the knot sum of the derivative itself -- differentiating the value
// polynomial instead would subtract A0 from A1, sums that agree to first order in the knot distance).
template <int KIND, typename Store>
__device__ __forceinline__ double build_dim_tab_dx(const DimDesc &D, const double *__restrict__ tab,
                                                   const double *__restrict__ dtab, double xv,
                                                   const Store &store, double &rho) {
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
  const size_t eoff = (size_t)D.tab + ((D.m + 1) & ~1) + (size_t)J * D.ncol * 6;
  const dd2 *__restrict__ cf = (const dd2 *)(tab + eoff);
  const dd2 *__restrict__ df = (const dd2 *)(dtab + eoff);
  double cl = 1.0, icl = 1.0, dcl = 0.0;
  for (int c = 0; c < D.ncol; ++c) {
    const dd2 e0 = cf[3 * c], e1 = cf[3 * c + 1], e2 = cf[3 * c + 2];  // A0 A1 | A2 B0 | B1 B2
    const dd2 f0 = df[3 * c], f1 = df[3 * c + 1], f2 = df[3 * c + 2];
    const double r = em * fma(t, fma(t, e1.x, e0.y), e0.x) + ep * fma(t, fma(t, e2.y, -e2.x), e1.y);
    const double dr = (em * fma(t, fma(t, f1.x, f0.y), f0.x) + ep * fma(t, fma(t, f2.y, -f2.x), f1.y)) * dudx;
    if (c == 0) {
      cl = r;
      icl = 1.0 / r;
      dcl = dr;
    } else {
      const double rr = r * icl;
      store.val(D.ccol0 + c - 1, rr);
      store.der(D.ccol0 + c - 1, (dr - rr * dcl) * icl);
    }
  }
  rho = dcl * icl;
  return cl;
}

template <typename Store>
__device__ __forceinline__ double build_dim_dx_any(const DimDesc &D, const double *ka, const double *kb,
                                                   const double *kc, const double *rot, const double *tab,
                                                   const double *dtab, double xv, const Store &store,
                                                   double &rho) {
  if (D.tab >= 0) {
    if (D.kind == OBHIP_COV_MAT25) return build_dim_tab_dx<OBHIP_COV_MAT25>(D, tab, dtab, xv, store, rho);
    return build_dim_tab_dx<OBHIP_COV_MAT25POW>(D, tab, dtab, xv, store, rho);
  }
  if (D.kind == OBHIP_COV_MAT25) return build_dim_dx<OBHIP_COV_MAT25>(D, ka, kb, kc, rot, xv, store, rho);
  if (D.kind == OBHIP_COV_MAT25POW)
    return build_dim_dx<OBHIP_COV_MAT25POW>(D, ka, kb, kc, rot, xv, store, rho);
  if (D.kind == kCovMat25Direct) return build_dim_dx<kCovMat25Direct>(D, ka, kb, kc, rot, xv, store, rho);
  if (D.kind == kCovMat25PowDirect)
    return build_dim_dx<kCovMat25PowDirect>(D, ka, kb, kc, rot, xv, store, rho);
  return build_dim_dx<OBHIP_COV_MAT25ANG>(D, ka, kb, kc, rot, xv, store, rho);
}

// ---- phase 1 of the fused predictors: one 64-row tile of the basis -------------------------------
// lane = row; wave w of WAVES takes the dimensions w, w + WAVES, ... and writes their used columns
// through `store` (DX: also their derivative columns and the column rho_l; dtab is not read
// otherwise), wave 0 the ones column.  Rows beyond the input (valid false) are evaluated at 0.5 instead.
// The wave's share of the row scale (the product of its dimensions' level 0) goes to part[wave][64];
// after a barrier tile_scale gives the row's scale.  x is column-major with leading dimension ldx.
template <int WAVES, bool DX, int PITCH>
__device__ __forceinline__ void build_tile(const DimDesc *__restrict__ dims, const double *__restrict__ ka,
                                           const double *__restrict__ kb, const double *__restrict__ kc,
                                           const double *__restrict__ rot, const double *__restrict__ tab,
                                           const double *__restrict__ dtab, int d, const double *__restrict__ x,
                                           uint64_t ldx, uint64_t row, bool valid, int wave,
                                           const StoreTile<PITCH> &store, double *part) {
  double sc = 1.0;
  for (int l = wave; l < d; l += WAVES) {
    const DimDesc D = dims[l];
    const double xv = valid ? x[(uint64_t)l * ldx + row] : 0.5;
    if constexpr (DX) {
      double rho;
      sc *= build_dim_dx_any(D, ka, kb, kc, rot, tab, dtab, xv, store, rho);
      store.rho(l, rho);
    } else {
      sc *= build_dim_any(D, ka, kb, kc, rot, tab, xv, store);
    }
  }
  if (wave == 0) store.tile[store.lane] = 1.0;  // used column 0 = all ones
  part[wave * kTileRows + store.lane] = sc;
}

// build_tile for one side of a product of two input blocks (kernels_product.hip): the dimensions
// side[0 .. nside) instead of 0 .. d, column s of x holding dimension side[s]; the wave takes the
// entries slot, slot + WAVES, ... (slot: its place in the round the caller deals the two sides' dimensions
// in).  store.cpos maps the compact columns of the side's dimensions to the side's own used columns, so the
// row scale that lands in part[wave][64] is the product of R_l0 over this side's dimensions only.
template <int WAVES, int PITCH>
__device__ __forceinline__ void build_tile_side(const DimDesc *__restrict__ dims, const double *__restrict__ ka,
                                                const double *__restrict__ kb, const double *__restrict__ kc,
                                                const double *__restrict__ rot, const double *__restrict__ tab,
                                                const int *__restrict__ side, int nside,
                                                const double *__restrict__ x, uint64_t ldx, uint64_t row, bool valid,
                                                int wave, int slot, const StoreTile<PITCH> &store, double *part) {
  double sc = 1.0;
  for (int s = slot; s < nside; s += WAVES) {
    const DimDesc D = dims[side[s]];
    const double xv = valid ? x[(uint64_t)s * ldx + row] : 0.5;
    sc *= build_dim_any(D, ka, kb, kc, rot, tab, xv, store);
  }
  if (wave == 0) store.tile[store.lane] = 1.0;  // used column 0 = all ones
  part[wave * kTileRows + store.lane] = sc;
}

// build_tile_side with the derivatives by the side's inputs (kernels_product_dx.hip): behind the side's Mu
// value columns the derivative column of every used column >= 1 and behind those one column of rho per entry
// of side[], in that order (StoreTile::der, ::rho with l = the entry's index).  The value columns and the row
// scale are those of build_tile_side's formulas through build_dim_dx_any, as build_tile<DX = true> has them.
template <int WAVES, int PITCH>
__device__ __forceinline__ void build_tile_side_dx(const DimDesc *__restrict__ dims, const double *__restrict__ ka,
                                                   const double *__restrict__ kb, const double *__restrict__ kc,
                                                   const double *__restrict__ rot, const double *__restrict__ tab,
                                                   const double *__restrict__ dtab, const int *__restrict__ side,
                                                   int nside, const double *__restrict__ x, uint64_t ldx, uint64_t row,
                                                   bool valid, int wave, int slot, const StoreTile<PITCH> &store,
                                                   double *part) {
  double sc = 1.0;
  for (int s = slot; s < nside; s += WAVES) {
    const DimDesc D = dims[side[s]];
    const double xv = valid ? x[(uint64_t)s * ldx + row] : 0.5;
    double rho;
    sc *= build_dim_dx_any(D, ka, kb, kc, rot, tab, dtab, xv, store, rho);
    store.rho(s, rho);
  }
  if (wave == 0) store.tile[store.lane] = 1.0;  // used column 0 = all ones
  part[wave * kTileRows + store.lane] = sc;
}

// the row scale of this lane's row: the waves' shares multiplied in wave order
template <int WAVES>
__device__ __forceinline__ double tile_scale(const double *part, int lane) {
  double s = 1.0;
#pragma unroll
  for (int q = 0; q < WAVES; ++q) s *= part[q * kTileRows + lane];
  return s;
}

}  // namespace obhip
