// Moment tables of the 1-D bases over a product measure: the means and covariances behind the variance-based
// measures and the derivative means, cross and derivative-product tables behind the derivative-based ones
// (sobol.cpp; include/obhip.h; DESIGN.md sections 19, 31 and 33).  No reference counterpart.
//
// k_moments<V>: lane = node row, block = (row slice, dimension, tile of 8 levels or pair of such tiles).  A row's raw
//   psi_t -- and, for the derivative variants, psi'_t -- come from the library's own builders (build_dim_any,
//   build_dim_raw_dx_any: interval tables staged in LDS where the model has them, the knot loop otherwise) into
//   [level][thread] LDS tiles, never into HBM.  Rows >= n are never read.  A variant V names the builder, how
//   blockIdx.z numbers the level tiles and the two factors:
//     ValueMeans     w psi_t, w and the bad weights                          one tile
//     ValueCov       w (psi_t - m_t)(psi_t' - m_t'), the means of ValueMeans  lower triangle of tile pairs, mirrored
//     DerivMeans     w psi'_t, w and the bad weights                         one tile
//     DerivCross     w (psi'_a psi_b)                                        all ordered tile pairs (not symmetric)
//     DerivProducts  w (psi'_a psi'_b)                                       lower triangle of tile pairs, mirrored
//   The product of the two factors comes first, so that (a, b) and (b, a) get the same bits.  Sums: per thread over
//   its rows, butterfly per wave, the waves in order, then k_moments_fin<V> over the row slices (lane-strided,
//   butterfly): a fixed order.
#include "obhip_internal.h"
#include "device_common.h"
#include "device_dx_raw.h"
#include "sobol_device.h"

namespace obhip {

namespace {

enum MomTiles { kOneTile, kAllTilePairs, kLowerTilePairs };

// kScreen: a weight that is negative or not finite counts as 0 (ValueCov takes the weights as they are: by then
// ValueMeans has flagged the call)
struct ValueMeans {
  static constexpr bool kDeriv = false, kCentred = false, kScreen = true;
  static constexpr MomTiles kTiles = kOneTile;
  static __device__ __forceinline__ const double *first(const double *val, const double *) { return val; }
  static __device__ __forceinline__ const double *second(const double *val, const double *) { return val; }
};
struct ValueCov : ValueMeans {
  static constexpr bool kCentred = true, kScreen = false;
  static constexpr MomTiles kTiles = kLowerTilePairs;
};
struct DerivMeans {
  static constexpr bool kDeriv = true, kCentred = false, kScreen = true;
  static constexpr MomTiles kTiles = kOneTile;
  static __device__ __forceinline__ const double *first(const double *, const double *der) { return der; }
  static __device__ __forceinline__ const double *second(const double *, const double *der) { return der; }
};
struct DerivCross : DerivMeans {
  static constexpr MomTiles kTiles = kAllTilePairs;
  static __device__ __forceinline__ const double *second(const double *val, const double *) { return val; }
};
struct DerivProducts : DerivMeans {
  static constexpr MomTiles kTiles = kLowerTilePairs;
};

template <typename V>
constexpr int mom_sums() { return V::kTiles == kOneTile ? kMomP1 : kMomP2; }
inline int mom_tiles(MomTiles tiles, int nlt) {
  return tiles == kOneTile ? nlt : tiles == kAllTilePairs ? nlt * nlt : nlt * (nlt + 1) / 2;
}
template <MomTiles TILES>
__device__ __forceinline__ void mom_tile(int z, int nlt, int &ta, int &tb) {
  ta = z, tb = 0;
  if (TILES == kAllTilePairs) {
    ta = z / nlt;
    tb = z % nlt;
  } else if (TILES == kLowerTilePairs) {
    tile_pair_lower(z, ta, tb);
  }
}

// dynamic LDS: [interval tables kIntervalTabMax][reduction 4 * 64][values lmax * threads] and, for a derivative
// variant, [derivatives lmax * threads]
template <typename V>
__global__ void __launch_bounds__(256)
k_moments(const DimDesc *__restrict__ dims, const double *__restrict__ ka, const double *__restrict__ kb,
          const double *__restrict__ kc, const double *__restrict__ rot, const double *__restrict__ tab,
          const double *__restrict__ dtab, const double *__restrict__ x, uint64_t n, uint64_t ldx,
          const double *__restrict__ w, uint64_t ldw, int nlt, int lmax, const double *__restrict__ mean,
          double *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int l = blockIdx.y, nt = blockDim.x;
  double *ltab = smem, *red = smem + kIntervalTabMax, *val = red + 4 * kMomP2 + threadIdx.x;
  double *der = val + (size_t)lmax * nt;  // (a derivative variant only)
  DimDesc D = dims[l];
  const int L = D.ncol, dtab_off = D.tab;
  int ta, tb;
  mom_tile<V::kTiles>(blockIdx.z, nlt, ta, tb);
  if (ta * kMomLT >= L || tb * kMomLT >= L) return;  // (block-uniform, before the first barrier)
  const double *tb_ = stage_tab(D, tab, ltab);
  constexpr int K = mom_sums<V>();
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  double ma[kMomLT], mb[kMomLT];
  if (V::kCentred) {
    const int om = mean_offset(dims, l);
#pragma unroll
    for (int a = 0; a < kMomLT; ++a) {
      ma[a] = ta * kMomLT + a < L ? mean[om + ta * kMomLT + a] : 0.0;
      mb[a] = tb * kMomLT + a < L ? mean[om + tb * kMomLT + a] : 0.0;
    }
  }
  const double *fa = V::first(val, der), *fb = V::second(val, der);
  for (uint64_t i = (uint64_t)blockIdx.x * nt + threadIdx.x; i < n; i += (uint64_t)gridDim.x * nt) {
    const double xv = x[(uint64_t)l * ldx + i];
    double wv = w ? w[(uint64_t)l * ldw + i] : 1.0;
    const bool bad = V::kScreen && (!(wv >= 0.0) || wv > 1.7976931348623157e308);
    if (bad) wv = 0.0;
    if constexpr (V::kDeriv) build_dim_raw_dx_any(D, ka, kb, kc, rot, tb_, dtab, dtab_off, xv, val, der, nt);
    else eval_raw(D, ka, kb, kc, rot, tb_, xv, val, nt);
    if (V::kTiles == kOneTile) {
      if (bad) acc[kMomLT + 1] += 1.0;
      acc[kMomLT] += wv;
#pragma unroll
      for (int a = 0; a < kMomLT; ++a) {
        const int t = ta * kMomLT + a;
        if (t < L) acc[a] = fma(wv, fa[(size_t)t * nt], acc[a]);
      }
    } else {
      double da[kMomLT], db[kMomLT];
#pragma unroll
      for (int a = 0; a < kMomLT; ++a) {
        const int t = ta * kMomLT + a, u = tb * kMomLT + a;
        if (V::kCentred) {
          da[a] = t < L ? fa[(size_t)t * nt] - ma[a] : 0.0;
          db[a] = u < L ? fb[(size_t)u * nt] - mb[a] : 0.0;
        } else {
          da[a] = t < L ? fa[(size_t)t * nt] : 0.0;
          db[a] = u < L ? fb[(size_t)u * nt] : 0.0;
        }
      }
      // w (F_a F_b): the product of the two factors first, so that (a, b) and (b, a) get the same bits
#pragma unroll
      for (int a = 0; a < kMomLT; ++a)
#pragma unroll
        for (int b = 0; b < kMomLT; ++b) acc[a * kMomLT + b] = fma(wv, da[a] * db[b], acc[a * kMomLT + b]);
    }
  }
  __syncthreads();
  block_sums<K>(acc, red, part + (((uint64_t)l * gridDim.z + blockIdx.z) * gridDim.x + blockIdx.x) * K);
}

// block (dimension, level tile or pair of level tiles as k_moments<V> numbers them), one wave: one tile -- the
// means, the weight sum of the dimension and the flag; pairs -- the table over the weight sum, the lower triangle
// mirrored
template <MomTiles TILES>
__global__ void __launch_bounds__(64)
k_moments_fin(const DimDesc *__restrict__ dims, const double *__restrict__ part, int nblk, int nlt,
              double *__restrict__ wsum, int *__restrict__ flag, double *__restrict__ out) {
  constexpr int K = TILES == kOneTile ? kMomP1 : kMomP2;
  const int l = blockIdx.x, L = dims[l].ncol;
  int ta, tb;
  mom_tile<TILES>(blockIdx.y, nlt, ta, tb);
  if (ta * kMomLT >= L || tb * kMomLT >= L) return;
  const double *base = part + ((uint64_t)l * gridDim.y + blockIdx.y) * nblk * K;
  if (TILES == kOneTile) {
    const double W = slices_sum<K>(base, nblk, kMomLT), bad = slices_sum<K>(base, nblk, kMomLT + 1);
    if (ta == 0 && threadIdx.x == 0) {
      wsum[l] = W;
      if (bad > 0.0 || !(W > 0.0) || W > 1.7976931348623157e308) flag[0] = 1;
    }
    const int om = mean_offset(dims, l);
    for (int a = 0; a < kMomLT; ++a) {
      const double s = slices_sum<K>(base, nblk, a);
      const int t = ta * kMomLT + a;
      if (t < L && threadIdx.x == 0) out[om + t] = s / W;
    }
  } else {
    const double W = wsum[l];
    const int oc = cov_offset(dims, l);
    for (int k = 0; k < K; ++k) {
      const int ia = ta * kMomLT + k / kMomLT, ib = tb * kMomLT + k % kMomLT;
      if (ia >= L || ib >= L || (TILES == kLowerTilePairs && ib > ia)) continue;  // (wave-uniform)
      const double s = slices_sum<K>(base, nblk, k);
      if (threadIdx.x == 0) {
        const double c = s / W;
        out[oc + ia * L + ib] = c;
        if (TILES == kLowerTilePairs) out[oc + ib * L + ia] = c;
      }
    }
  }
}

// pass -> finish for each variant in turn, into outs[i]; outs[0] are the means (the first variant's, which a
// centred variant behind it reads); lmax: the most levels of a dimension; nth threads, lds bytes of dynamic LDS per
// block of the pass
template <typename... Vs>
int launch_moment_variants(const char *scope, const obhip_model &m, obhip_terms &t, uint64_t lmax, int nth, size_t lds,
                           const double *d_nodes, uint64_t n, uint64_t ldx, const double *d_w, uint64_t ldw,
                           double *const (&outs)[sizeof...(Vs)], int *flag_out) {
  constexpr bool deriv = (Vs::kDeriv || ...);
  OB_TRY(prepare_predict(m, t, deriv));
  const ModelDev &md = t.pred_md;
  const uint64_t d = m.d;
  const int nblk = (int)std::min<uint64_t>(kMomBlocks, (n + nth - 1) / nth);
  const int nlt = (int)((lmax + kMomLT - 1) / kMomLT);
  DevBuf<double> part, wsum;
  DevBuf<int> flag;
  OB_TRY(part.alloc(d * nblk * std::max({(uint64_t)mom_tiles(Vs::kTiles, nlt) * mom_sums<Vs>()...})));
  OB_TRY(wsum.alloc(d));
  OB_TRY(flag.alloc(1));
  OB_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), cur_stream()));
  int rc = 0;
  ((rc = rc ? rc : ensure_dyn_lds((const void *)k_moments<Vs>, lds)), ...);
  OB_TRY(rc);
  {
    ProfScope ps(scope);
    const double *dtab = deriv ? t.dx.dtab.p : nullptr;
    int i = 0;
    (([&] {
       const int ntile = mom_tiles(Vs::kTiles, nlt);
       hipLaunchKernelGGL(k_moments<Vs>, dim3(nblk, (unsigned)d, ntile), dim3(nth), lds, cur_stream(), md.dims.p, md.ka.p,
                          md.kb.p, md.kc.p, md.rot.p, md.tab.p, dtab, d_nodes, n, ldx, d_w, ldw, nlt, (int)lmax,
                          (const double *)outs[0], part.p);
       hipLaunchKernelGGL(k_moments_fin<Vs::kTiles>, dim3((unsigned)d, ntile), dim3(64), 0, cur_stream(), md.dims.p,
                          (const double *)part.p, nblk, nlt, wsum.p, flag.p, outs[i++]);
     }()),
     ...);
    OB_HIP(hipGetLastError());
  }
  return d2h(flag_out, flag.p, sizeof(int));  // (waits: the scratch above is released behind it)
}

uint64_t max_levels(const obhip_model &m, const obhip_terms &t) {
  uint64_t lmax = 1;
  for (uint64_t l = 0; l < m.d; ++l) lmax = std::max<uint64_t>(lmax, t.maxlev[l] + 1);
  return lmax;
}

}  // namespace

int active_moment_threads(uint64_t lmax) { return lmax <= 16 ? 256 : 64; }
size_t active_moments_lds(uint64_t lmax) {
  return (kIntervalTabMax + 4 * kMomP2 + 2 * lmax * active_moment_threads(lmax)) * sizeof(double);
}

int launch_dim_moments(const obhip_model &m, obhip_terms &t, const double *d_nodes, uint64_t n, uint64_t ldx,
                       const double *d_w, uint64_t ldw, double *d_mean, double *d_cov, int *flag_out) {
  const uint64_t lmax = max_levels(m, t);
  double *const outs[] = {d_mean, d_cov};
  return launch_moment_variants<ValueMeans, ValueCov>("dim_moments", m, t, lmax, eval_threads(lmax), eval_lds(lmax),
                                                      d_nodes, n, ldx, d_w, ldw, outs, flag_out);
}

int launch_dim_grad_moments(const obhip_model &m, obhip_terms &t, const double *d_nodes, uint64_t n, uint64_t ldx,
                            const double *d_w, uint64_t ldw, double *d_dmean, double *d_cross, double *d_dd,
                            int *flag_out) {
  const uint64_t lmax = max_levels(m, t);
  double *const outs[] = {d_dmean, d_cross, d_dd};
  return launch_moment_variants<DerivMeans, DerivCross, DerivProducts>(
      "dim_grad_moments", m, t, lmax, active_moment_threads(lmax), active_moments_lds(lmax), d_nodes, n, ldx, d_w, ldw,
      outs, flag_out);
}

}  // namespace obhip
