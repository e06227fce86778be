// Input gradients of the full-covariance posterior variance and of the acquisition criteria for gfx950
// (acquire_dx.cpp; include/obhip.h, "acquisition gradients").  No reference counterpart.
//
// With S = inv(H), b_ik = s_i P_ik and the stored product Y = S B^T (term-major, pp x npad: Y[k npad + i] =
// t_ik, the row's own coefficient vector) the latent variance is d_i = b_i^T t_i and, S being symmetric,
// dd_i/dx_l = 2 (db_i/dx_l)^T t_i: the mean-gradient formula of k_predict_dx with t_i in the place of theta.
//
// Per 64-row tile (lane = row, 8 waves), as k_predict_dx:
//   1. build_tile<., true>: value columns, derivative columns and rho_l of the tile's rows;
//   2. dense pass: Sm = sum_k theta_k P_k (theta in registers behind readlane) and Sd = sum_k t_ik P_k, the lane
//      reading Y[k npad + row] -- coalesced, 512 bytes per wave and term;
//   3. for every dimension l the 8 waves split the view of l (obhip_terms::dx) evenly: gm = sum theta_k E_kl r'
//      and gd = sum t_ik E_kl r'.  The wave partials go through double-buffered LDS and are summed in wave
//      order by wave l mod 8, which forms
//        mu = s Sm    dmu/dx_l = s (rho_l Sm + gm)        d = s Sd    dd/dx_l = 2 s (rho_l Sd + gd)
//      and, in FP64, d score / dx_l = A dmu~ + C dsd with dsd = dd / (2 sd) (0 where d <= 0) and the two
//      coefficients A, C of the criterion (acq_eval), formed once per row and tile.
// Every output is column-major n x d with leading dimension ldo, 512 contiguous bytes per (tile, dimension).
// No atomics, a fixed summation order that does not depend on where a row stands: two runs give the same
// bits, a chunked call those of the unchunked one, twin rows the same results.
//
// CRIT = kAdxNone: the variance and its gradient only, theta is never read.
// HBM = false: the tile lives in LDS (predict_dx_supports).  HBM = true (W2 = 0): the tile in a per-block slice
// of pooled HBM scratch and the term tables read from memory, any number of used columns and of factors.
#include <cmath>

#include "obhip_internal.h"
#include "acquire_device.h"
#include "device_dx.h"

namespace obhip {

namespace {

constexpr int kAdxThreads = 512, kAdxWaves = kAdxThreads / 64;
constexpr int kAdxRedCols = 2 * 2 * kAdxWaves;  // [buffer][mean | variance][wave] columns of 64 partials

template <int W2, int CRIT, bool HBM>
__global__ void __launch_bounds__(kAdxThreads)
k_acquire_dx(const DimDesc *__restrict__ dims, const double *__restrict__ ka, const double *__restrict__ kb,
             const double *__restrict__ kc, const double *__restrict__ rot, const double *__restrict__ tab,
             const double *__restrict__ dtab, const int *__restrict__ cpos, int d, int Mu,
             const uint32_t *__restrict__ colsw, int W2rt, int p, const uint32_t *__restrict__ vw,
             const uint32_t *__restrict__ voff, const double *__restrict__ theta, const double *__restrict__ Y,
             uint64_t npad, const double *__restrict__ x, uint64_t ldx, uint64_t n, uint64_t ntiles,
             double *__restrict__ scratch, const AcqDxArgs a) {
  constexpr bool MEAN = CRIT != kAdxNone;
  extern __shared__ double lds[];
  const int ncols = 2 * Mu - 1 + d;
  double *tile = HBM ? scratch + (size_t)blockIdx.x * ncols * kTileRows : lds;
  double *red = HBM ? lds : lds + (size_t)ncols * kTileRows;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int stride = W2rt + 2;  // words per view entry: W2rt column words, own column, term index
  auto redp = [&](int buf, int which, int w) { return red + ((buf * 2 + which) * kAdxWaves + w) * kTileRows + lane; };

  for (uint64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const uint64_t row = tl * kTileRows + lane;  // < npad: the padded rows of Y are zeros
    const bool valid = row < n;
    // a row with a coordinate that is not finite is evaluated at 0.5 like a row beyond the input and gets NaN
    bool fin = valid;
    for (int l = 0; l < d && fin; ++l) fin = isfinite(x[(uint64_t)l * ldx + row]);
    // ---- 1. basis, derivative basis and rho at the rows of the tile ----
    const StoreTile<kTileRows> store{tile, cpos, lane, Mu};
    build_tile<kAdxWaves, true>(dims, ka, kb, kc, rot, tab, dtab, d, x, ldx, row, fin, wave, store, red);
    __syncthreads();
    const double s = tile_scale<kAdxWaves>(red, lane);  // (the partials lie where redp(0, 0, .) does)
    __syncthreads();

    // ---- 2. dense pass: Sm = sum theta_k P_k, Sd = sum t_ik P_k ----
    const double *__restrict__ yrow = Y + row;
    double am = 0.0, ad = 0.0;
    if constexpr (W2 > 0) {
      const int ngroups = (p + 63) / 64;
      uint32_t cw[W2];
      for (int g = wave; g < ngroups; g += kAdxWaves) {
        const int k0 = g * 64, cnt = min(64, p - k0);
        const int kk = min(k0 + lane, p - 1);
        load_cw(cw, colsw, kk);
        const double th = MEAN ? theta[kk] : 0.0;
        const double *__restrict__ yp = yrow + (size_t)k0 * npad;
        for (int t = 0; t < cnt; ++t) {
          const double pr = term_prod_rl<W2>(tile, cw, t, lane, 1.0);
          if (MEAN) am = fma(readlane_f64(th, t), pr, am);
          ad = fma(yp[(size_t)t * npad], pr, ad);
        }
      }
    } else {
      for (int k = wave; k < p; k += kAdxWaves) {
        const double pr = term_prod_mem(tile, colsw + (size_t)k * W2rt, W2rt, lane, 1.0);
        if (MEAN) am = fma(theta[k], pr, am);
        ad = fma(yrow[(size_t)k * npad], pr, ad);
      }
    }
    if (MEAN) *redp(0, 0, wave) = am;
    *redp(0, 1, wave) = ad;
    __syncthreads();
    double Sm = 0.0, Sd = 0.0;
#pragma unroll
    for (int q = 0; q < kAdxWaves; ++q) {
      if (MEAN) Sm += *redp(0, 0, q);
      Sd += *redp(0, 1, q);
    }
    const double mu = fin ? Sm * s : NAN, dv = fin ? Sd * s : NAN;
    double A = 0.0, C = 0.0, hsd = 0.0;  // hsd = 1 / (2 sd), 0 where d <= 0
    if constexpr (MEAN) {
      const double sc = acq_eval<CRIT>(a.sgn * mu, dv, a.best, a.xi, a.kappa, a.level, A, C);
      const double sd = sqrt(fmax(dv, 0.0));
      hsd = sd > 0.0 ? 1.0 / (2.0 * sd) : (dv != dv ? NAN : 0.0);
      if (wave == 0 && valid) {
        a.score[a.row0 + row] = sc;
        if (a.mean) a.mean[a.row0 + row] = mu;
      }
    }
    if (wave == 0 && valid && a.var) a.var[a.row0 + row] = dv + a.noise;

    // ---- 3. per dimension: the view of l split over the waves ----
    for (int l = 0; l < d; ++l) {
      const int buf = (l + 1) & 1;
      const int v0 = (int)voff[l], vcnt = (int)voff[l + 1] - v0;
      const int per = (vcnt + kAdxWaves - 1) / kAdxWaves;
      const int beg = v0 + min(wave * per, vcnt), end = v0 + min((wave + 1) * per, vcnt);
      double gm = 0.0, gd = 0.0;
      if constexpr (W2 > 0) {
        uint32_t cw[W2];
        for (int e0 = beg; e0 < end; e0 += 64) {
          const int cnt = min(64, end - e0);
          const uint32_t *ent = vw + (size_t)min(e0 + lane, end - 1) * stride;
#pragma unroll
          for (int w = 0; w < W2; ++w) cw[w] = ent[w];
          const int ownl = (int)ent[W2];
          const int kl = (int)ent[W2 + 1];
          const double th = MEAN ? theta[kl] : 0.0;
          for (int t = 0; t < cnt; ++t) {
            const double E = term_prod_rl<W2>(tile, cw, t, lane, 1.0);
            const int own = __builtin_amdgcn_readlane(ownl, t);
            const int k = __builtin_amdgcn_readlane(kl, t);
            const double Ed = E * tile[(Mu + own - 1) * kTileRows + lane];
            if (MEAN) gm = fma(readlane_f64(th, t), Ed, gm);
            gd = fma(yrow[(size_t)k * npad], Ed, gd);
          }
        }
      } else {
        for (int e = beg; e < end; ++e) {
          const uint32_t *ent = vw + (size_t)e * stride;
          const double E = term_prod_mem(tile, ent, W2rt, lane, 1.0);
          const int own = (int)ent[W2rt];
          const uint32_t k = ent[W2rt + 1];
          const double Ed = E * tile[(Mu + own - 1) * kTileRows + lane];
          if (MEAN) gm = fma(theta[k], Ed, gm);
          gd = fma(yrow[(size_t)k * npad], Ed, gd);
        }
      }
      if (MEAN) *redp(buf, 0, wave) = gm;
      *redp(buf, 1, wave) = gd;
      __syncthreads();
      if (wave == (l & (kAdxWaves - 1)) && valid) {
        double tg = 0.0, td = 0.0;
#pragma unroll
        for (int q = 0; q < kAdxWaves; ++q) {
          if (MEAN) tg += *redp(buf, 0, q);
          td += *redp(buf, 1, q);
        }
        const double rho = tile[(2 * Mu - 1 + l) * kTileRows + lane];
        const uint64_t o = (uint64_t)l * a.ldo + a.row0 + row;
        const double dd = fin ? 2.0 * s * fma(rho, Sd, td) : NAN;
        if (a.gradvar) a.gradvar[o] = dd;
        if constexpr (MEAN) {
          const double dm = fin ? s * fma(rho, Sm, tg) : NAN;
          if (a.gradmean) a.gradmean[o] = dm;
          const double dsd = hsd == 0.0 ? 0.0 : dd * hsd;
          a.gradscore[o] = A * (a.sgn * dm) + C * dsd;
        }
      }
    }
    __syncthreads();  // the tile and the partials are free for the next tile
  }
}

template <int W2, int CRIT, bool HBM>
int run_acquire_dx(const obhip_model &m, obhip_terms &t, const double *d_theta, const double *d_Y, uint64_t npad,
                   const double *d_x, uint64_t ldx, uint64_t n, const AcqDxArgs &a) {
  const uint64_t ncols = 2 * t.Mu - 1 + m.d;
  const size_t lds = ((HBM ? 0 : ncols) + kAdxRedCols) * kTileRows * sizeof(double);
  OB_TRY(ensure_dyn_lds((const void *)k_acquire_dx<W2, CRIT, HBM>, lds));
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t ntiles = (n + kTileRows - 1) / kTileRows;
  uint64_t nblk = std::min<uint64_t>(ntiles, (uint64_t)device_cus(dev) * (HBM ? 2 : 4));
  DevBuf<double> scratch;
  if (HBM) {
    nblk = hbm_tile_blocks(nblk, ncols);
    OB_TRY(scratch.alloc(nblk * ncols * kTileRows));
  }
  launch_pred<true>(k_acquire_dx<W2, CRIT, HBM>, dim3((unsigned)nblk), dim3(kAdxThreads), lds, pred_tabs(m, t),
                    (const uint32_t *)t.cols.p, (int)(t.W / 2), (int)t.p, t.dx.vw.p, t.dx.voff_dev.p, d_theta, d_Y,
                    npad, d_x, ldx, n, ntiles, scratch.p, a);
  OB_HIP(hipGetLastError());
  // (scratch goes back to the pool under this stream: handed out again to work queued behind the kernel)
  return 0;
}

template <int CRIT>
int dispatch_acquire_dx(bool fused, const obhip_model &m, obhip_terms &t, const double *d_theta, const double *d_Y,
                        uint64_t npad, const double *d_x, uint64_t ldx, uint64_t n, const AcqDxArgs &a) {
#define OB_ADX(W2_, HBM_) return run_acquire_dx<W2_, CRIT, HBM_>(m, t, d_theta, d_Y, npad, d_x, ldx, n, a)
  if (!fused) OB_ADX(0, true);
  switch (t.W / 2) {
    case 1: OB_ADX(1, false);
    case 2: OB_ADX(2, false);
    case 3: OB_ADX(3, false);
    default: OB_ADX(4, false);
  }
#undef OB_ADX
}

}  // namespace

bool acquire_dx_fused(const obhip_terms &t) { return predict_dx_supports(t) && !getenv("OBHIP_FORCE_GENERIC"); }

uint64_t acquire_dx_lds_bytes(const obhip_terms &t, uint64_t d, bool fused) {
  return ((fused ? 2 * t.Mu - 1 + d : 0) + kAdxRedCols) * kTileRows * sizeof(double);
}

int launch_acquire_dx(const obhip_model &m, obhip_terms &t, int crit, const double *d_theta, const double *d_Y,
                      uint64_t npad, const double *d_x, uint64_t ldx, uint64_t n, const AcqDxArgs &a) {
  if (n == 0) return 0;
  if (npad < (n + kTileRows - 1) / kTileRows * kTileRows)
    return fail(OBHIP_ERR_STATE, "acquire_dx: the stored product is narrower than the rows' tiles");
  ProfScope ps("acquire_dx");
  const bool fused = acquire_dx_fused(t);
  switch (crit) {
    case kAdxNone: return dispatch_acquire_dx<kAdxNone>(fused, m, t, d_theta, d_Y, npad, d_x, ldx, n, a);
    case OBHIP_ACQ_EI: return dispatch_acquire_dx<OBHIP_ACQ_EI>(fused, m, t, d_theta, d_Y, npad, d_x, ldx, n, a);
    case OBHIP_ACQ_PI: return dispatch_acquire_dx<OBHIP_ACQ_PI>(fused, m, t, d_theta, d_Y, npad, d_x, ldx, n, a);
    case OBHIP_ACQ_LCB: return dispatch_acquire_dx<OBHIP_ACQ_LCB>(fused, m, t, d_theta, d_Y, npad, d_x, ldx, n, a);
    case OBHIP_ACQ_STRADDLE:
      return dispatch_acquire_dx<OBHIP_ACQ_STRADDLE>(fused, m, t, d_theta, d_Y, npad, d_x, ldx, n, a);
    default: return fail(OBHIP_ERR_INVALID, "acquire_grad: no kernel for this criterion");
  }
}

}  // namespace obhip
