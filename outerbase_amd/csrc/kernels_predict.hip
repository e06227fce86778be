// Fused predictor for gfx950: basis evaluation at new inputs and the B theta
// (and B^2 coeffvar) contraction in one kernel; the basis tile only ever exists
// in LDS.  Replaces predictor$update + $mean + $var of pred_gauss
// (src/lpdfs/loglik_gauss.cpp:214-227: a fresh outerbase (modandbase.cpp:547)
// followed by prodmm_ (linalg.cpp:57-131) on basemat and on basematsq).
//
// Per 64-row tile: 8 waves evaluate the dimensions (wave w takes w, w+8, ...),
// lane = row, writing only the columns the terms use into the LDS tile; after
// one barrier the 8 waves split the terms in groups of 64 with register-resident
// term tables, exactly as k_mm does.
#include "obhip_internal.h"
#include "device_dx.h"

namespace obhip {

namespace {

// 8 waves per 64-row tile (see kMmThreads in kernels_prod.hip)
constexpr int kPrThreads = 512, kPrWaves = kPrThreads / 64;

template <int W2, bool VAR>
__global__ void __launch_bounds__(kPrThreads)
k_predict(const DimDesc *__restrict__ dims, const double *__restrict__ ka,
          const double *__restrict__ kb, const double *__restrict__ kc,
          const double *__restrict__ rot, const double *__restrict__ tab, const int *__restrict__ cpos, int d, int Mu,
          const uint32_t *__restrict__ colsw, int W2rt, int p, const double *__restrict__ theta,
          const double *__restrict__ coeffvar, double e2sigma, const double *__restrict__ x,
          uint64_t n, double *__restrict__ mean, double *__restrict__ var) {
  extern __shared__ double lds[];
  double *red = lds + (size_t)Mu * kTileRows;   // [kPrWaves][64] scale partials, then mean partials
  double *redv = red + kPrWaves * kTileRows;    // [kPrWaves][64] variance partials
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t row = (uint64_t)blockIdx.x * kTileRows + lane;
  const bool valid = row < n;

  const StoreTile<kTileRows> store{lds, cpos, lane, Mu};
  build_tile<kPrWaves, false>(dims, ka, kb, kc, rot, tab, nullptr, d, x, n, row, valid, wave, store, red);
  __syncthreads();
  const double s = tile_scale<kPrWaves>(red, lane);
  __syncthreads();

  double am = 0.0, av = 0.0;
  if constexpr (W2 > 0) {
    const int ngroups = (p + 63) / 64;
    uint32_t cw[W2];
    for (int g = wave; g < ngroups; g += kPrWaves) {
      const int k0 = g * 64, cnt = min(64, p - k0);
      const int kk = min(k0 + lane, p - 1);
      load_cw(cw, colsw, k0 + lane);
      const double th = theta[kk];
      const double cv = VAR ? coeffvar[kk] : 0.0;
      if (cnt == 64) {
#pragma unroll
        for (int t = 0; t < 64; ++t) {
          const double pr = term_prod_rl<W2>(lds, cw, t, lane, 1.0);
          am = fma(readlane_f64(th, t), pr, am);
          if (VAR) av = fma(readlane_f64(cv, t), pr * pr, av);
        }
      } else {
        for (int t = 0; t < cnt; ++t) {
          const double pr = term_prod_rl<W2>(lds, cw, t, lane, 1.0);
          am = fma(readlane_f64(th, t), pr, am);
          if (VAR) av = fma(readlane_f64(cv, t), pr * pr, av);
        }
      }
    }
  } else {
    for (int k = wave; k < p; k += kPrWaves) {
      const double pr = term_prod_mem(lds, colsw + (size_t)k * W2rt, W2rt, lane, 1.0);
      am = fma(theta[k], pr, am);
      if (VAR) av = fma(coeffvar[k], pr * pr, av);
    }
  }
  red[wave * kTileRows + lane] = am;
  if (VAR) redv[wave * kTileRows + lane] = av;
  __syncthreads();
  if (wave == 0 && valid) {
    double tm = 0.0, tv = 0.0;
#pragma unroll
    for (int q = 0; q < kPrWaves; ++q) {
      tm += red[q * kTileRows + lane];
      if (VAR) tv += redv[q * kTileRows + lane];
    }
    mean[row] = tm * s;
    if (VAR) var[row] = tv * (s * s) + e2sigma;  // loglik_gauss.cpp:224-225
  }
}

// ---- term-per-lane predictor -------------------------------------------------------------------
// Default.  Persistent blocks of 8 waves; per 64-row tile the waves first evaluate the
// dimensions (lane = row) into the [column][65] LDS tile, then switch to lane = term for the
// contraction exactly as k_mm_tl does: theta_k (and coeffvar_k) and the column addresses of
// NG terms per lane stay in registers, 8 rows of accumulators per chunk, permlane-swap
// butterfly + DPP for the sum over the lanes.  More than 8 * NG * 64 terms: several passes
// over the same LDS tile with the tables reloaded.
template <int W, int NG, bool VAR>
struct PrCtx {
  uint32_t ad[NG][W];
  double th[NG];
  double cv[VAR ? NG : 1];
  double acc[8];
  double accv[VAR ? 8 : 1];
  template <int RR>
  __device__ __forceinline__ void row() {}
  template <int RR, int UNIT>
  __device__ __forceinline__ void use(double v) {
    acc[RR] = fma(v, th[UNIT], acc[RR]);
    if constexpr (VAR) accv[RR] = fma(v * v, cv[UNIT], accv[RR]);
  }
};

// 8 accumulators x 64 lanes -> tile rows rc .. rc + 7 of red[wave][.]
__device__ __forceinline__ void pr_reduce8(const double (&acc)[8], double *__restrict__ redw, int rc,
                                           int lane) {
  double s4[4], s2[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) s4[i] = swap32_sum(acc[i], acc[i + 4]);
#pragma unroll
  for (int i = 0; i < 2; ++i) s2[i] = swap16_sum(s4[i], s4[i + 2]);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    double v = row16_ror_add<8>(s2[i]);
    v = row16_ror_add<4>(v);
    v = row16_ror_add<2>(v);
    v = row16_ror_add<1>(v);
    if ((lane & 15) == 0) redw[rc + i + 2 * (lane >> 4)] = v;
  }
}

template <int W2, int NG, bool VAR>
__global__ void __launch_bounds__(kTlThreads, 4)
k_predict_tl(const DimDesc *__restrict__ dims, const double *__restrict__ ka,
             const double *__restrict__ kb, const double *__restrict__ kc,
             const double *__restrict__ rot, const double *__restrict__ tab, const int *__restrict__ cpos, int d, int Mu,
             const uint32_t *__restrict__ colsw, const uint32_t *__restrict__ sperm, int p,
             uint64_t p_pad, int npass,
             const double *__restrict__ theta, const double *__restrict__ coeffvar, double e2sigma,
             const double *__restrict__ x, uint64_t n, uint64_t ntiles, uint64_t tiles_per_split,
             double *__restrict__ mean, double *__restrict__ var) {
  extern __shared__ double lds[];
  constexpr int W = 2 * W2;
  constexpr int kInflight = NG * W >= 32 ? 8 : 12;
  double *red = lds + (size_t)Mu * kTlPitch;    // [8 waves][64 rows] mean partials
  double *redv = red + kTlWaves * kTileRows;    // [8][64] variance partials
  double *reds = redv + kTlWaves * kTileRows;   // [8][64] scale partials
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t t0 = (uint64_t)blockIdx.x * tiles_per_split;
  const uint64_t t1 = min(ntiles, t0 + tiles_per_split);

  PrCtx<W, NG, VAR> c;
  int we = W;  // column slots the terms of this wave (and pass) need
  // slots: NG * 64 consecutive ones of the sorted order per wave (tl_slot)
  auto load_terms = [&](int pass) {
    int nzmax = 1;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const uint64_t slot = tl_slot<NG>((uint64_t)pass, wave, g, lane);
      const bool ok = slot < p_pad;
      const uint64_t k = ok ? sperm[slot] : 0;
      const bool real = ok && k < (uint64_t)p;
      c.th[g] = real ? theta[k] : 0.0;
      if constexpr (VAR) c.cv[g] = real ? coeffvar[k] : 0.0;
      uint32_t cw[W2];
#pragma unroll
      for (int w = 0; w < W2; ++w) {
        cw[w] = ok ? colsw[k * W2 + w] : 0u;  // column 0 = ones
        c.ad[g][2 * w] = (cw[w] & 0xffffu) * (kTlPitch * 8);
        c.ad[g][2 * w + 1] = (cw[w] >> 16) * (kTlPitch * 8);
      }
      nzmax = max(nzmax, tl_nnz<W2>(cw));
    }
    we = tl_variant<W>(wave_max_i32(nzmax));
  };
  if (npass == 1) load_terms(0);

  double s_cur = 0.0;  // wave 0: basescale of row = lane of the tile being contracted
  auto emit = [&](uint64_t tile, double s) {  // wave 0, lane = row
    const uint64_t row = tile * kTileRows + lane;
    double tm = 0.0, tv = 0.0;
#pragma unroll
    for (int q = 0; q < kTlWaves; ++q) {
      tm += red[q * kTileRows + lane];
      if (VAR) tv += redv[q * kTileRows + lane];
    }
    if (row < n) {
      mean[row] = tm * s;
      if (VAR) var[row] = tv * (s * s) + e2sigma;  // loglik_gauss.cpp:224-225
    }
  };

  const StoreTile<kTlPitch> store{lds, cpos, lane, Mu};
  for (uint64_t tile = t0; tile < t1; ++tile) {
    __syncthreads();  // the previous tile's partials are complete, its LDS tile is free
    if (tile > t0 && wave == 0) emit(tile - 1, s_cur);
    {  // basis at the new rows, lane = row
      const uint64_t row = tile * kTileRows + lane;
      const bool valid = row < n;
      build_tile<kTlWaves, false>(dims, ka, kb, kc, rot, tab, nullptr, d, x, n, row, valid, wave, store, reds);
    }
    __syncthreads();  // tile built; wave 0 has read the previous partials
    if (wave == 0) s_cur = tile_scale<kTlWaves>(reds, lane);
#pragma unroll 1
    for (int rc = 0; rc < kTileRows; rc += 8) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        c.acc[r] = 0.0;
        if constexpr (VAR) c.accv[r] = 0.0;
      }
      for (int pass = 0; pass < npass; ++pass) {
        if (npass > 1) {
          load_terms(pass);
#pragma unroll
          for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int j = 0; j < W; ++j) c.ad[g][j] += rc * 8;
        }
        tl_run_half<W, NG, 8, kInflight, 0>(c, we);
      }
      if (npass == 1) {
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
          for (int j = 0; j < W; ++j) {
            c.ad[g][j] += (rc + 8 < kTileRows) ? 8 * 8 : -(kTileRows - 8) * 8;
            asm volatile("" : "+v"(c.ad[g][j]));
          }
      }
      pr_reduce8(c.acc, red + wave * kTileRows, rc, lane);
      if constexpr (VAR) pr_reduce8(c.accv, redv + wave * kTileRows, rc, lane);
    }
  }
  __syncthreads();
  if (t0 < t1 && wave == 0) emit(t1 - 1, s_cur);
}

size_t predict_tl_lds_bytes(const obhip_terms &t) {
  return (t.Mu * kTlPitch + 3 * kTlWaves * kTileRows) * sizeof(double);
}

// k_predict_tl: the terms in passes of 8 waves x NG groups x 64
int run_predict_tl(const obhip_model &m, obhip_terms &t, const double *d_theta, const double *d_x, uint64_t n,
                   double *d_mean, const double *d_coeffvar, double e2sigma, double *d_var) {
  const bool var = d_coeffvar != nullptr && d_var != nullptr;
  const int w2 = (int)(t.W / 2);
  const int ng = units_per_lane(t.p_pad, (uint64_t)kTlWaves * 64, predict_tl_max_units(w2, var));
  const uint64_t tpb = (uint64_t)kTlWaves * ng * 64;
  const int npass = (int)((t.p_pad + tpb - 1) / tpb);
  const size_t lds = predict_tl_lds_bytes(t);
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t ntiles = (n + kTileRows - 1) / kTileRows;
  const RowSplit rs = split_rows(ntiles, (uint64_t)device_cus(dev) * 4);
  return pick<1, 2, 3, 4>(w2, [&](auto W2) {
    return pick_bool(var, [&](auto VAR) {
      return pick<8, 4, 2, 1>(ng, [&](auto NG) {
        if constexpr (NG() > predict_tl_max_units(W2(), VAR())) return no_kernel();
        else {
          constexpr auto kernel = k_predict_tl<W2(), NG(), VAR()>;
          OB_TRY(ensure_dyn_lds((const void *)kernel, lds));
          launch_pred<false>(kernel, dim3((unsigned)rs.nsplit), dim3(kTlThreads), lds, pred_tabs(m, t),
                             (const uint32_t *)t.cols.p, t.sperm.p, (int)t.p, t.p_pad, npass, d_theta, d_coeffvar,
                             e2sigma, d_x, n, ntiles, rs.tps, d_mean, d_var);
          OB_HIP(hipGetLastError());
          return 0;
        }
      });
    });
  });
}

// k_predict: lane = row
int run_predict(const obhip_model &m, obhip_terms &t, const double *d_theta, const double *d_x, uint64_t n,
                double *d_mean, const double *d_coeffvar, double e2sigma, double *d_var) {
  const size_t lds = (t.Mu * kTileRows + 2 * kPrWaves * kTileRows) * sizeof(double);
  const int w2 = (int)(t.W / 2);
  return pick<1, 2, 3, 4, 0>(w2, [&](auto W2) {
    return pick_bool(d_coeffvar != nullptr && d_var != nullptr, [&](auto VAR) {
      constexpr auto kernel = k_predict<W2(), VAR()>;
      OB_TRY(ensure_dyn_lds((const void *)kernel, lds));
      launch_pred<false>(kernel, dim3((unsigned)((n + kTileRows - 1) / kTileRows)), dim3(kPrThreads), lds,
                         pred_tabs(m, t), (const uint32_t *)t.cols.p, w2, (int)t.p, d_theta, d_coeffvar, e2sigma, d_x, n,
                         d_mean, d_var);
      OB_HIP(hipGetLastError());
      return 0;
    });
  });
}

}  // namespace

int launch_predict(const obhip_model &m, obhip_terms &t, const double *d_theta, const double *d_x,
                   uint64_t n, double *d_mean, const double *d_coeffvar, double e2sigma,
                   double *d_var) {
  OB_TRY(prepare_predict(m, t, false));
  if (n == 0) return 0;
  ProfScope ps("predict");
  if (t.Mu > 296 || getenv("OBHIP_FORCE_GENERIC")) {
    // more used columns than the fused kernel's LDS tile holds: evaluate the basis at the new
    // rows into HBM (levels the terms use only) and take the products from there
    obhip_basis *bn = nullptr;
    OB_TRY(obhip_basis_create_dev(&bn, &m, d_x, n, t.maxlev.data()));
    int rc = launch_mm(*bn, t, d_theta, d_mean, false);
    if (!rc && d_coeffvar != nullptr && d_var != nullptr) {
      rc = launch_mm(*bn, t, d_coeffvar, d_var, true);
      if (!rc) rc = launch_affine(d_var, n, -e2sigma, 1.0);
    }
    obhip_basis_destroy(bn);  // synchronises the stream first
    return rc;
  }
  static const bool lane_row = getenv("OBHIP_PREDICT_LANE_ROW") != nullptr;
  static const bool no_star = getenv("OBHIP_HM3") && atoi(getenv("OBHIP_HM3")) == 0;
  if (!lane_row && !no_star && star_predict_supports(t))  // shared sub-products (kernels_star.hip)
    return launch_star_predict(m, t, d_theta, d_x, n, d_mean, d_coeffvar, e2sigma, d_var);
  const int w2 = (int)(t.W / 2);
  if (!lane_row && w2 >= 1 && w2 <= 4 && predict_tl_lds_bytes(t) <= kLdsTile)
    return run_predict_tl(m, t, d_theta, d_x, n, d_mean, d_coeffvar, e2sigma, d_var);
  return run_predict(m, t, d_theta, d_x, n, d_mean, d_coeffvar, e2sigma, d_var);
}

}  // namespace obhip
