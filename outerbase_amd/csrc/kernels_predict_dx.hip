// Fused input-gradient predictor for gfx950: at new rows x the mean B theta, the variance
// B^2 coeffvar + e^{2 sigma} and their gradients by every input x_l in one kernel; neither the
// basis nor its derivative ever exists outside the tile.  No reference counterpart.
//
// Per 64-row tile (lane = row, 8 waves):
//   1. the waves evaluate the dimensions (wave w takes w, w + 8, ...; build_dim_dx_any) into the
//      tile: Mu used value columns (column 0 = ones), behind them the derivative column of every
//      used column >= 1, behind those d columns of rho_l = R'_l0 / R_l0;
//   2. dense pass, as k_predict: S = sum_k theta_k P_k (and V = sum_k c_k P_k^2), terms in groups of
//      64 with register-resident tables;
//   3. for every dimension l the 8 waves split the view of l (obhip_terms::dx: the terms that have
//      l, each with its OTHER columns, its own column and its index) evenly, in chunks of 64
//      view-terms held in registers: g = sum theta_k E_kl r'_l,t (E_kl the product of the other
//      columns), gv = sum c_k (E_kl r) (E_kl r').  The wave partials go through LDS and are summed
//      in wave order by wave l mod 8, which writes
//        dmean/dx_l = s (rho_l S + g)        dvar/dx_l = 2 s^2 (rho_l V + gv)
//      column-major, 512 contiguous bytes per (tile, dimension).  The partials are double-buffered:
//      one barrier per dimension.
// No atomics, a fixed summation order: two runs give the same bits.
//
// HBM = false: the tile lives in LDS ((2 Mu - 1 + d + 32) x 512 bytes, predict_dx_supports).
// HBM = true: the same code with the tile in a per-block slice of pooled HBM scratch and the term
// tables read from memory (any number of used columns and of factors): the fallback.
#include "obhip_internal.h"
#include "device_dx.h"

namespace obhip {

namespace {

constexpr int kDxThreads = 512, kDxWaves = kDxThreads / 64;
constexpr int kDxRedCols = 2 * 2 * kDxWaves;  // [buffer][mean | var][wave] columns of 64 partials

template <int W2, bool VAR, bool HBM>
__global__ void __launch_bounds__(kDxThreads)
k_predict_dx(const DimDesc *__restrict__ dims, const double *__restrict__ ka, const double *__restrict__ kb,
             const double *__restrict__ kc, const double *__restrict__ rot, const double *__restrict__ tab,
             const double *__restrict__ dtab, const int *__restrict__ cpos, int d, int Mu,
             const uint32_t *__restrict__ colsw, int W2rt, int p, const uint32_t *__restrict__ vw,
             const uint32_t *__restrict__ voff, const double *__restrict__ theta,
             const double *__restrict__ coeffvar, double e2sigma, const double *__restrict__ x, uint64_t n,
             uint64_t ntiles, double *__restrict__ scratch, double *__restrict__ mean,
             double *__restrict__ var, double *__restrict__ grad, double *__restrict__ gradvar) {
  extern __shared__ double lds[];
  const int ncols = 2 * Mu - 1 + d;
  double *tile = HBM ? scratch + (size_t)blockIdx.x * ncols * kTileRows : lds;
  double *red = HBM ? lds : lds + (size_t)ncols * kTileRows;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int stride = W2rt + 2;  // words per view entry: W2rt column words, own column, term index
  auto redp = [&](int buf, int which, int w) { return red + ((buf * 2 + which) * kDxWaves + w) * kTileRows + lane; };

  for (uint64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const uint64_t row = tl * kTileRows + lane;
    const bool valid = row < n;
    // ---- 1. basis, derivative basis and rho at the rows of the tile ----
    const StoreTile<kTileRows> store{tile, cpos, lane, Mu};
    build_tile<kDxWaves, true>(dims, ka, kb, kc, rot, tab, dtab, d, x, n, row, valid, wave, store, red);
    __syncthreads();
    const double s = tile_scale<kDxWaves>(red, lane);  // (the partials lie where redp(0, 0, .) does)
    __syncthreads();

    // ---- 2. dense pass: S = sum theta_k P_k, V = sum c_k P_k^2 ----
    double am = 0.0, av = 0.0;
    if constexpr (W2 > 0) {
      const int ngroups = (p + 63) / 64;
      uint32_t cw[W2];
      for (int g = wave; g < ngroups; g += kDxWaves) {
        const int k0 = g * 64, cnt = min(64, p - k0);
        const int kk = min(k0 + lane, p - 1);
        load_cw(cw, colsw, kk);
        const double th = theta[kk];
        const double cv = VAR ? coeffvar[kk] : 0.0;
        for (int t = 0; t < cnt; ++t) {
          const double pr = term_prod_rl<W2>(tile, cw, t, lane, 1.0);
          am = fma(readlane_f64(th, t), pr, am);
          if (VAR) av = fma(readlane_f64(cv, t), pr * pr, av);
        }
      }
    } else {
      for (int k = wave; k < p; k += kDxWaves) {
        const double pr = term_prod_mem(tile, colsw + (size_t)k * W2rt, W2rt, lane, 1.0);
        am = fma(theta[k], pr, am);
        if (VAR) av = fma(coeffvar[k], pr * pr, av);
      }
    }
    *redp(0, 0, wave) = am;
    if (VAR) *redp(0, 1, wave) = av;
    __syncthreads();
    double S = 0.0, V = 0.0;
#pragma unroll
    for (int q = 0; q < kDxWaves; ++q) {
      S += *redp(0, 0, q);
      if (VAR) V += *redp(0, 1, q);
    }
    if (wave == 0 && valid) {
      if (mean) mean[row] = S * s;
      if (VAR && var) var[row] = V * (s * s) + e2sigma;
    }

    // ---- 3. per dimension: the view of l split over the waves ----
    for (int l = 0; l < d; ++l) {
      const int buf = (l + 1) & 1;
      const int v0 = (int)voff[l], vcnt = (int)voff[l + 1] - v0;
      const int per = (vcnt + kDxWaves - 1) / kDxWaves;
      const int beg = v0 + min(wave * per, vcnt), end = v0 + min((wave + 1) * per, vcnt);
      double gm = 0.0, gv = 0.0;
      if constexpr (W2 > 0) {
        uint32_t cw[W2];
        for (int e0 = beg; e0 < end; e0 += 64) {
          const int cnt = min(64, end - e0);
          const uint32_t *ent = vw + (size_t)min(e0 + lane, end - 1) * stride;
#pragma unroll
          for (int w = 0; w < W2; ++w) cw[w] = ent[w];
          const int ownl = (int)ent[W2];
          const uint32_t k = ent[W2 + 1];
          const double th = theta[k];
          const double cv = VAR ? coeffvar[k] : 0.0;
          for (int t = 0; t < cnt; ++t) {
            const double E = term_prod_rl<W2>(tile, cw, t, lane, 1.0);
            const int own = __builtin_amdgcn_readlane(ownl, t);
            const double dr = tile[(Mu + own - 1) * kTileRows + lane];
            const double Ed = E * dr;
            gm = fma(readlane_f64(th, t), Ed, gm);
            if (VAR) gv = fma(readlane_f64(cv, t), (E * tile[own * kTileRows + lane]) * Ed, gv);
          }
        }
      } else {
        for (int e = beg; e < end; ++e) {
          const uint32_t *ent = vw + (size_t)e * stride;
          const double E = term_prod_mem(tile, ent, W2rt, lane, 1.0);
          const int own = (int)ent[W2rt];
          const uint32_t k = ent[W2rt + 1];
          const double Ed = E * tile[(Mu + own - 1) * kTileRows + lane];
          gm = fma(theta[k], Ed, gm);
          if (VAR) gv = fma(coeffvar[k], (E * tile[own * kTileRows + lane]) * Ed, gv);
        }
      }
      *redp(buf, 0, wave) = gm;
      if (VAR) *redp(buf, 1, wave) = gv;
      __syncthreads();
      if (wave == (l & (kDxWaves - 1)) && valid) {
        double tg = 0.0, tv = 0.0;
#pragma unroll
        for (int q = 0; q < kDxWaves; ++q) {
          tg += *redp(buf, 0, q);
          if (VAR) tv += *redp(buf, 1, q);
        }
        const double rho = tile[(2 * Mu - 1 + l) * kTileRows + lane];
        grad[(uint64_t)l * n + row] = s * fma(rho, S, tg);
        if (VAR && gradvar) gradvar[(uint64_t)l * n + row] = 2.0 * (s * s) * fma(rho, V, tv);
      }
    }
    __syncthreads();  // the tile and the partials are free for the next tile
  }
}

template <int W2, bool VAR, bool HBM>
int run_predict_dx(const obhip_model &m, obhip_terms &t, const double *d_theta, const double *d_x, uint64_t n,
                   double *d_mean, double *d_grad, const double *d_coeffvar, double e2sigma, double *d_var,
                   double *d_gradvar) {
  const uint64_t ncols = 2 * t.Mu - 1 + m.d;
  const size_t lds = ((HBM ? 0 : ncols) + kDxRedCols) * kTileRows * sizeof(double);
  OB_TRY(ensure_dyn_lds((const void *)k_predict_dx<W2, VAR, HBM>, lds));
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t ntiles = (n + kTileRows - 1) / kTileRows;
  uint64_t nblk = std::min<uint64_t>(ntiles, (uint64_t)device_cus(dev) * (HBM ? 2 : 4));
  DevBuf<double> scratch;
  if (HBM) {
    nblk = hbm_tile_blocks(nblk, ncols);
    OB_TRY(scratch.alloc(nblk * ncols * kTileRows));
  }
  launch_pred<true>(k_predict_dx<W2, VAR, HBM>, dim3((unsigned)nblk), dim3(kDxThreads), lds, pred_tabs(m, t),
                    (const uint32_t *)t.cols.p, (int)(t.W / 2), (int)t.p, t.dx.vw.p, t.dx.voff_dev.p, d_theta,
                    d_coeffvar, e2sigma, d_x, n, ntiles, scratch.p, d_mean, d_var, d_grad, d_gradvar);
  OB_HIP(hipGetLastError());
  // (scratch goes back to the pool under this stream: handed out again to work queued behind the kernel)
  return 0;
}

template <bool VAR>
int dispatch_predict_dx(bool fused, const obhip_model &m, obhip_terms &t, const double *d_theta, const double *d_x,
                        uint64_t n, double *d_mean, double *d_grad, const double *d_coeffvar, double e2sigma,
                        double *d_var, double *d_gradvar) {
#define OB_DX(W2_, HBM_) \
  return run_predict_dx<W2_, VAR, HBM_>(m, t, d_theta, d_x, n, d_mean, d_grad, d_coeffvar, e2sigma, d_var, d_gradvar)
  if (!fused) OB_DX(0, true);
  switch (t.W / 2) {
    case 1: OB_DX(1, false);
    case 2: OB_DX(2, false);
    case 3: OB_DX(3, false);
    default: OB_DX(4, false);
  }
#undef OB_DX
}

}  // namespace

// the fused kernel's domain: at most 8 factors per term and a tile that fits the LDS
bool predict_dx_supports(const obhip_terms &t) {
  const uint64_t w2 = t.W / 2;
  return w2 >= 1 && w2 <= 4 &&
         (2 * t.Mu - 1 + t.d + kDxRedCols) * kTileRows * sizeof(double) <= kLdsBudget;
}

int launch_predict_dx(const obhip_model &m, obhip_terms &t, const double *d_theta, const double *d_x, uint64_t n,
                      double *d_mean, double *d_grad, const double *d_coeffvar, double e2sigma, double *d_var,
                      double *d_gradvar) {
  OB_TRY(prepare_predict(m, t, true));
  if (n == 0) return 0;
  ProfScope ps("predict_dx");
  const bool fused = predict_dx_supports(t) && !getenv("OBHIP_FORCE_GENERIC");
  if (d_coeffvar != nullptr)
    return dispatch_predict_dx<true>(fused, m, t, d_theta, d_x, n, d_mean, d_grad, d_coeffvar, e2sigma, d_var,
                                     d_gradvar);
  return dispatch_predict_dx<false>(fused, m, t, d_theta, d_x, n, d_mean, d_grad, d_coeffvar, e2sigma, d_var,
                                    d_gradvar);
}

}  // namespace obhip
