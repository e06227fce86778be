// The gradient basis of an outerbase for gfx950:
//   basemat_gradhyp        outermod::buildob, gradient form   src/modandbase.cpp:306-327
//                          outerbase::build with dograd       src/modandbase.cpp:547-626
//
// For hyper-parameter h of dimension l = hypmatch[h] the reference stores, per row,
//   basemat_gradhyp[:, gest[h] + t] = (d cov/d hyp_h . rotmat_l + cov . rotmat_gradhyp_h)[:, t] / c_l
// for EVERY level t (0 included).  ONE combined tile-blocked array holds the basemat columns, then per
// hyper-parameter these gradient columns ge[h, 0..cap], then per hyper-parameter the delta columns
// ge[h, t] - basemat[col(dim h, t)] ge[h, 0]; ensure_gradbasis_sq adds its squared store.
#include <atomic>
#include <thread>

#include "obhip_internal.h"
#include "device_common.h"

namespace obhip {

namespace {

// kernel value and its hyper-parameter derivatives at one knot (covfuncs.cpp:134-150,
// 220-243, 318-347); a0, a1 as in kernel_pre, lx = log(x) (mat25pow only)
template <int KIND>
__device__ __forceinline__ void kernel_value_grad(const DimDesc &D, double ka, double kb, double kd,
                                                  double a0, double a1, double lx, double &kv,
                                                  double &g0, double &g1) {
  constexpr double a = 2.0, b = 0.25;
  if (KIND == OBHIP_COV_MAT25ANG) {
    const double hs = a0 - ka, hc = a1 - kb;
    const double h = sqrt(hs * hs + hc * hc);
    const double e = exp(-h), w = e * (h + 1.0);
    kv = (1.0 + h + h * h * (1.0 / 3.0)) * e;
    g0 = a / 3 * hs * hs * w;
    g1 = a / 3 * hc * hc * w;
  } else {
    const double h = a0 - ka, ah = fabs(h);
    const double e = exp(-ah);
    kv = (1.0 + ah + ah * ah * (1.0 / 3.0)) * e;
    const double h2 = h * (1.0 + ah) * e;
    g0 = a / 3 * (h * h2);
    g1 = 0.0;
    if (KIND == OBHIP_COV_MAT25POW || KIND == kCovMat25PowDirect)
      // D.p0 = powv; a0 and ka are centred on D.p2 (device_common.h), t(x) itself is a0 + D.p2
      g1 = (lx * (a0 + D.p2) - kd) * (-(b * D.p0 / 3) * h2) + b / 3 * (h * h2);
  }
}

// one dimension, one row: R = cov . rot, Rt_h = dcov_h . rot + cov . rotg_h, everything
// divided by R[0]; basemat columns and gradient columns go to the combined tile
template <int KIND>
__device__ __forceinline__ double build_dim_grad(const DimDesc &D, const GradHyp *__restrict__ hy,
                                                 int nh, const double *__restrict__ ka,
                                                 const double *__restrict__ kb,
                                                 const double *__restrict__ kd,
                                                 const double *__restrict__ rot,
                                                 const double *__restrict__ rotg, double xv,
                                                 double *__restrict__ tile_out) {
  double a0, a1, a2;
  kernel_pre<KIND>(D, xv, a0, a1, a2);
  const double lx = (KIND == OBHIP_COV_MAT25POW || KIND == kCovMat25PowDirect) ? log(xv) : 0.0;
  double cl = 1.0, g00 = 0.0, g10 = 0.0;  // level-0 gradient columns of the two hyper-parameters
  for (int c0 = 0; c0 < D.ncolp; c0 += 8) {
    double r[8], t0[8], t1[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) r[c] = t0[c] = t1[c] = 0.0;
    const double *rp = rot + D.rotoff + c0;
    const double *g0p = rotg + hy[0].rotgoff + c0;
    const double *g1p = rotg + hy[nh - 1].rotgoff + c0;
    for (int j = 0; j < D.m; ++j) {
      double kv, d0, d1;
      kernel_value_grad<KIND>(D, ka[D.koff + j], kb[D.koff + j], kd[D.koff + j], a0, a1, lx, kv, d0,
                              d1);
      const size_t o = (size_t)j * D.ncolp;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const double rc = rp[o + c];
        r[c] = fma(kv, rc, r[c]);
        t0[c] = fma(d0, rc, fma(kv, g0p[o + c], t0[c]));
        if (KIND != OBHIP_COV_MAT25 && KIND != kCovMat25Direct) t1[c] = fma(d1, rc, fma(kv, g1p[o + c], t1[c]));
      }
    }
    if (c0 == 0) {
      cl = r[0];
      g00 = t0[0] / cl;
      g10 = t1[0] / cl;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int col = c0 + c;
      if (col < D.ncol) {
        const double bv = r[c] / cl, ge0 = t0[c] / cl, ge1 = t1[c] / cl;
        tile_out[(size_t)(hy[0].gecol + col) * kTileRows] = ge0;
        if (KIND != OBHIP_COV_MAT25 && KIND != kCovMat25Direct) tile_out[(size_t)(hy[1].gecol + col) * kTileRows] = ge1;
        if (col >= 1) {
          tile_out[(size_t)(D.ccol0 + col - 1) * kTileRows] = bv;
          tile_out[(size_t)(hy[0].dcol + col - 1) * kTileRows] = fma(-bv, g00, ge0);
          if (KIND != OBHIP_COV_MAT25 && KIND != kCovMat25Direct)
            tile_out[(size_t)(hy[1].dcol + col - 1) * kTileRows] = fma(-bv, g10, ge1);
        }
      }
    }
  }
  return cl;
}

// ---- interval tables of the gradient basis (mat25 / mat25pow) -------------------------------
// The same algebra as the value path's tables (device_common.h build_dim_tab, core.cpp): between
// two neighbouring knots every per-knot quantity of build_dim_grad is e^{-h} (below) or e^{-ah}
// (above) times a polynomial of degree <= 3 in h = u(x) - u_j:
//   kv = (1 + |h| + h^2 / 3) e            cov                       covfuncs.cpp:121-124
//   d0 = (a / 3) h^2 (1 + |h|) e          d cov / d hyp_0           covfuncs.cpp:134-150
//   d1 = -(b pw / 3) (L - kd_j) h (1 + |h|) e + (b / 3) h^2 (1 + |h|) e   (mat25pow, :220-243;
//        L = log(x) t(x) is a per-row scalar, kd_j = log(knot_j) t(knot_j))
// so with t = u(x) - (the largest u_j <= u(x)) the three knot sums per level are
//   r  = e^{-t} V-(t) + e^{t} V+(t)
//   t0 = e^{-t} C(t)  + e^{t} D(t)
//   t1 = e^{-t} (E(t) + L P(t)) + e^{t} (F(t) + L Q(t))
// with 6 + 8 (+ 8 + 6) host-built coefficients per (interval, level) (build_grad_tab below) -- O(1)
// per (row, level) where the knot loop spends ~45 instructions per (row, knot, 8 levels).
// A dimension's table is [mu sorted u][chunk 0][chunk 1] ...: the levels in chunks of `nck`, a chunk
// = [m + 1 intervals][nck levels][nc] -- as many levels as fit the LDS buffer beside the sorted u
// (every mat25 / mat25pow dimension of at most 127 knots gets tables: 128 intervals x 28
// coefficients are 3584 doubles per level).
struct GradTab {
  int off;      // offset (doubles) of the dimension's table in the table array, -1: knot loop
  int nc;       // coefficients per (interval, level): 14 (mat25) or 28 (mat25pow)
  int mu;       // sorted u, padded to an even length
  int nck;      // levels per chunk
  int nchunks;  // ceil(ncol / nck)
  int chunk;    // doubles per chunk = (m + 1) * nck * nc
};
constexpr int kGradTabMax = 16384;  // doubles of LDS for the sorted u + one chunk (128 KB)

// a row's place in a dimension's table: interval, local variable, the two exponentials, L
struct GradRow {
  int J;
  double t, em, ep, L;
};
template <int KIND>
__device__ __forceinline__ GradRow grad_row(const DimDesc &D, const double *__restrict__ tab, double xv) {
  constexpr bool POW = KIND == OBHIP_COV_MAT25POW;
  const double ux = (POW ? pow(xv, D.p0) / D.p1 : xv / D.p0) - D.p2;
  GradRow g;
  g.J = tab_bisect(tab, D.m, ux);
  g.t = ux - tab[max(g.J - 1, 0)];
  g.em = g.J == 0 ? 0.0 : exp(-g.t);
  g.ep = g.J == D.m ? 0.0 : exp(g.t);
  g.L = POW ? log(xv) * (ux + D.p2) : 0.0;
  return g;
}
// level 0's values, carried from the first chunk of a dimension to the later ones
struct GradLevel0 {
  double cl = 1.0, icl = 1.0, g00 = 0.0, g10 = 0.0;
};
// levels [c_lo, c_hi) of one dimension for one row; chunk: the staged chunk [m + 1][nck][NC]
template <int KIND>
__device__ __forceinline__ void build_dim_grad_tab(const DimDesc &D, const GradHyp *__restrict__ hy,
                                                   const double *__restrict__ chunk, int nck, int c_lo,
                                                   int c_hi, const GradRow &g, GradLevel0 &z,
                                                   double *__restrict__ tile_out) {
  constexpr bool POW = KIND == OBHIP_COV_MAT25POW;
  constexpr int NC = POW ? 28 : 14;
  typedef double dd2 __attribute__((ext_vector_type(2)));
  const double t = g.t, em = g.em, ep = g.ep, L = g.L;
  const dd2 *__restrict__ cf = (const dd2 *)(chunk + (size_t)g.J * nck * NC);
  double icl = z.icl, cl = z.cl, g00 = z.g00, g10 = z.g10;
#pragma unroll 1
  for (int c = c_lo; c < c_hi; ++c) {
    const dd2 *e = cf + (c - c_lo) * (NC / 2);
    const dd2 v0 = e[0], v1 = e[1], v2 = e[2];           // V-0 V-1 | V-2 V+0 | V+1 V+2
    const dd2 c0 = e[3], c1 = e[4], d0 = e[5], d1 = e[6];  // C0 C1 | C2 C3 | D0 D1 | D2 D3
    const double r = em * fma(t, fma(t, v1.x, v0.y), v0.x) + ep * fma(t, fma(t, v2.y, v2.x), v1.y);
    const double s0 = em * fma(t, fma(t, fma(t, c1.y, c1.x), c0.y), c0.x) +
                      ep * fma(t, fma(t, fma(t, d1.y, d1.x), d0.y), d0.x);
    double s1 = 0.0;
    if (POW) {
      const dd2 e0 = e[7], e1 = e[8], f0 = e[9], f1 = e[10];  // E0 E1 | E2 E3 | F0 F1 | F2 F3
      const dd2 p0 = e[11], pq = e[12], q1 = e[13];            // P0 P1 | P2 Q0 | Q1 Q2
      const double lo_ = fma(t, fma(t, fma(t, e1.y, e1.x), e0.y), e0.x) + L * fma(t, fma(t, pq.x, p0.y), p0.x);
      const double hi_ = fma(t, fma(t, fma(t, f1.y, f1.x), f0.y), f0.x) + L * fma(t, fma(t, q1.y, q1.x), pq.y);
      s1 = em * lo_ + ep * hi_;
    }
    if (c == 0) {
      cl = r;
      icl = 1.0 / r;
      g00 = s0 * icl;
      g10 = s1 * icl;
    }
    const double bv = r * icl, ge0 = s0 * icl, ge1 = s1 * icl;
    tile_out[(size_t)(hy[0].gecol + c) * kTileRows] = ge0;
    if (POW) tile_out[(size_t)(hy[1].gecol + c) * kTileRows] = ge1;
    if (c >= 1) {
      tile_out[(size_t)(D.ccol0 + c - 1) * kTileRows] = bv;
      tile_out[(size_t)(hy[0].dcol + c - 1) * kTileRows] = fma(-bv, g00, ge0);
      if (POW) tile_out[(size_t)(hy[1].dcol + c - 1) * kTileRows] = fma(-bv, g10, ge1);
    }
  }
  z.cl = cl, z.icl = icl, z.g00 = g00, z.g10 = g10;
}

// 16 waves = 16 row tiles per block; all waves walk the dimensions that have a table together,
// a dimension's sorted u and one chunk of its levels staged in LDS at a time.  Dimensions without a
// table (mat25ang, out-of-range hyper-parameters, more than 127 knots) are left to
// k_build_basis_grad, which then ran BEFORE this kernel on those dimensions alone
// (scale_has_part: scale holds their product).
__global__ void __launch_bounds__(1024)
k_build_basis_grad_tab(const DimDesc *__restrict__ dims, const GradHyp *__restrict__ hyps,
                       const int *__restrict__ hypst, const GradTab *__restrict__ gtabs,
                       const double *__restrict__ gtab, const double *__restrict__ x, uint64_t n, int d,
                       uint64_t Mtot, uint64_t ntiles, int scale_has_part, double *__restrict__ bm,
                       double *__restrict__ scale) {
  extern __shared__ double ltab[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t tile = (uint64_t)blockIdx.x * 16 + wave;
  const bool mine = tile < ntiles;  // (wave-uniform)
  const uint64_t row = tile * kTileRows + lane;
  const bool valid = mine && row < n;
  double *tile_out = bm + tile * Mtot * kTileRows + lane;
  double sc = 1.0;
  for (int l = 0; l < d; ++l) {
    const GradTab T = gtabs[l];
    if (T.off < 0) continue;  // (block-uniform)
    const DimDesc D = dims[l];
    const GradHyp *hy = hyps + hypst[l];
    const bool m25 = D.kind == OBHIP_COV_MAT25;
    GradRow g;
    GradLevel0 z;
    // per chunk: ~1800 clocks of LDS-bound evaluation per wave and 8 levels follow, so the ~1 us the
    // copy is exposed for is ~10 % (prefetching it through registers made the kernel spill)
    for (int k = 0; k < T.nchunks; ++k) {
      __syncthreads();  // everyone is done with what the buffer held
      if (k == 0)
        for (int e = threadIdx.x; e < T.mu; e += 1024) ltab[e] = gtab[T.off + e];
      const double *src = gtab + T.off + T.mu + (size_t)k * T.chunk;
      for (int e = threadIdx.x; e < T.chunk; e += 1024) ltab[T.mu + e] = src[e];
      __syncthreads();
      if (!mine) continue;
      if (k == 0) {
        const double xv = valid ? x[(uint64_t)l * n + row] : 0.5;
        g = m25 ? grad_row<OBHIP_COV_MAT25>(D, ltab, xv) : grad_row<OBHIP_COV_MAT25POW>(D, ltab, xv);
      }
      const int c_lo = k * T.nck, c_hi = min(D.ncol, c_lo + T.nck);
      if (m25)
        build_dim_grad_tab<OBHIP_COV_MAT25>(D, hy, ltab + T.mu, T.nck, c_lo, c_hi, g, z, tile_out);
      else
        build_dim_grad_tab<OBHIP_COV_MAT25POW>(D, hy, ltab + T.mu, T.nck, c_lo, c_hi, g, z, tile_out);
    }
    sc *= z.cl;
  }
  if (mine) {
    tile_out[0] = 1.0;
    if (scale_has_part) sc *= scale[row];
    scale[row] = valid ? sc : 0.0;
  }
}

__global__ void __launch_bounds__(256)
k_build_basis_grad(const DimDesc *__restrict__ dims, const GradHyp *__restrict__ hyps,
                   const int *__restrict__ hypst, const double *__restrict__ ka,
                   const double *__restrict__ kb, const double *__restrict__ kd,
                   const double *__restrict__ rot, const double *__restrict__ rotg,
                   const double *__restrict__ x, uint64_t n, int d, uint64_t Mtot,
                   const int *__restrict__ dimsel /* d dimensions to take, or null: 0 .. d - 1 */,
                   double *__restrict__ bm, double *__restrict__ scale) {
  __shared__ double part[4][kTileRows];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t tile = blockIdx.x;
  const uint64_t row = tile * kTileRows + lane;
  const bool valid = row < n;
  double *tile_out = bm + tile * Mtot * kTileRows + lane;
  double sc = 1.0;
  for (int li = wave; li < d; li += 4) {
    const int l = dimsel ? dimsel[li] : li;
    const DimDesc D = dims[l];
    const GradHyp *hy = hyps + hypst[l];
    const int nh = hypst[l + 1] - hypst[l];
    const double xv = valid ? x[(uint64_t)l * n + row] : 0.5;
    double cl;
    // (the gradient kernel takes one exp per knot anyway: the DIRECT kinds are the plain ones)
    if (D.kind == OBHIP_COV_MAT25 || D.kind == kCovMat25Direct)
      cl = build_dim_grad<kCovMat25Direct>(D, hy, nh, ka, kb, kd, rot, rotg, xv, tile_out);
    else if (D.kind == OBHIP_COV_MAT25POW || D.kind == kCovMat25PowDirect)
      cl = build_dim_grad<kCovMat25PowDirect>(D, hy, nh, ka, kb, kd, rot, rotg, xv, tile_out);
    else
      cl = build_dim_grad<OBHIP_COV_MAT25ANG>(D, hy, nh, ka, kb, kd, rot, rotg, xv, tile_out);
    sc *= cl;
  }
  part[wave][lane] = sc;
  if (wave == 0) tile_out[0] = 1.0;
  __syncthreads();
  if (wave == 0) {
    const double s = part[0][lane] * part[1][lane] * part[2][lane] * part[3][lane];
    scale[row] = valid ? s : 0.0;
  }
}

// ---- host: the interval tables of one dimension -------------------------------------------------
// Layout: [m sorted u, padded to an even length][m + 1 intervals][ncol levels][NC] with, per
// (interval J, level c), the polynomial coefficients (lowest power first) of
//   V- (3) V+ (3) | C (4) D (4) | E (4) F (4) P (3) Q (3)     (the last 14 for mat25pow only)
// in the local variable t = u(x) - ref_J, ref_J = u_(J-1) (u_(0) for J = 0): "-" sums the knots
// below (j < J, h = t + q_j, q_j = ref_J - u_j), "+" the knots above (ah = q_j - t, q_j = u_j -
// ref_J), each knot weighted by e^{-q_j} <= 1.  Built by two recurrences in extended precision,
// O(m) per level where a direct sum per interval would be O(m^2): going from interval J to J + 1
// the local variable moves by D = u_J - u_(J-1), so the "below" polynomial is shifted
// (P(t + D), a Taylor shift of a cubic) and damped by e^{-D} before knot J enters with q = 0;
// the "above" polynomials run the same way from the last interval down.  Every factor is <= 1
// and nothing is ever subtracted that the knot sum itself does not subtract.
typedef long double ld;
struct Cubic {
  ld c[4] = {0, 0, 0, 0};
  void shift(ld D) {  // P(t) -> P(t + D)
    const ld p0 = c[0], p1 = c[1], p2 = c[2], p3 = c[3];
    c[0] = p0 + D * (p1 + D * (p2 + D * p3));
    c[1] = p1 + D * (2 * p2 + 3 * D * p3);
    c[2] = p2 + 3 * D * p3;
  }
  void scale(ld f) {
    for (ld &v : c) v *= f;
  }
  void add(const Cubic &o, ld f) {
    for (int k = 0; k < 4; ++k) c[k] += f * o.c[k];
  }
  Cubic flipped() const {  // P(t) -> P(-t)
    Cubic r;
    r.c[0] = c[0], r.c[1] = -c[1], r.c[2] = c[2], r.c[3] = -c[3];
    return r;
  }
};

// us: the m centred knot positions u_j sorted ascending, ord their original indices; R, G0, G1:
// rotmat / rotmat_gradhyp columns of level c (indexed by the ORIGINAL knot index); kdv:
// log(knot_j) t(knot_j).  out: the chunks behind the sorted u, level c at chunk c / nck, entry
// ((J * nck) + c % nck) * NC of it.
void build_grad_tab(int m, int ncol, int nck, bool pw, double powv, const std::vector<double> &us,
                    const std::vector<int> &ord, const double *rot, const double *rotg0,
                    const double *rotg1, uint64_t ldr, const double *kdv, double *out) {
  const int NC = pw ? 28 : 14;
  const ld a3 = 2.0L / 3.0L, b3 = 0.25L / 3.0L, bp3 = 0.25L * (ld)powv / 3.0L;
  Cubic gkv, gcub, ghq;  // (1 + z + z^2 / 3), z^2 (1 + z), z (1 + z)
  gkv.c[0] = 1, gkv.c[1] = 1, gkv.c[2] = 1.0L / 3.0L;
  gcub.c[2] = 1, gcub.c[3] = 1;
  ghq.c[1] = 1, ghq.c[2] = 1;
  for (int c = 0; c < ncol; ++c) {
    const double *R = rot + (size_t)c * ldr, *G0 = rotg0 + (size_t)c * ldr, *G1 = pw ? rotg1 + (size_t)c * ldr : nullptr;
    // per-knot polynomials in z (z = h below, z = ah above); the sign of the z (1 + z) term flips
    // above, where h (1 + ah) = -ah (1 + ah)
    auto knot = [&](int j, bool above, Cubic (&f)[4]) {
      const int o = ord[j];
      const ld r = R[o], g0 = G0[o];
      for (Cubic &q : f) q = Cubic();
      f[0].add(gkv, r);                       // V
      f[1].add(gcub, a3 * r), f[1].add(gkv, g0);  // T0
      if (pw) {
        const ld sg = above ? -1.0L : 1.0L;
        f[2].add(ghq, sg * bp3 * (ld)kdv[o] * r), f[2].add(gcub, b3 * r), f[2].add(gkv, (ld)G1[o]);  // E / F
        f[3].add(ghq, -sg * bp3 * r);                                                                // P / Q
      }
    };
    std::vector<Cubic> below((size_t)(m + 1) * 4), above((size_t)(m + 1) * 4);
    Cubic cur[4], kn[4];
    // forward: below(J), J = 1 .. m (below(0) is empty)
    for (int J = 1; J <= m; ++J) {
      if (J >= 2) {
        const ld D = (ld)us[J - 1] - (ld)us[J - 2];
        const ld e = expl(-D);
        for (Cubic &q : cur) q.shift(D), q.scale(e);
      }
      knot(J - 1, false, kn);  // enters with q = 0: z = t
      for (int f = 0; f < 4; ++f) cur[f].add(kn[f], 1), below[(size_t)J * 4 + f] = cur[f];
    }
    // backward: above(J) for J = m - 1 .. 0 (above(m) is empty), as polynomials in t
    for (Cubic &q : cur) q = Cubic();
    for (int J = m - 1; J >= 0; --J) {
      // local variable of interval J against that of J + 1: t_J = t_(J+1) + D, D = ref_(J+1) - ref_J
      const ld refJ = us[J >= 1 ? J - 1 : 0], refJ1 = us[J];
      const ld D = refJ1 - refJ;
      const ld e = expl(-D);
      for (Cubic &q : cur) q.shift(-D), q.scale(e);
      // knot J enters with q_J = u_J - ref_J: polynomial in z = q_J - t -> in t
      knot(J, true, kn);
      const ld qJ = (ld)us[J] - refJ;
      const ld w = expl(-qJ);
      for (int f = 0; f < 4; ++f) {
        Cubic g = kn[f];
        g.shift(qJ);              // g(z = qJ + s)
        cur[f].add(g.flipped(), w);  // s = -t
        above[(size_t)J * 4 + f] = cur[f];
      }
    }
    for (int J = 0; J <= m; ++J) {
      double *e = out + (size_t)(c / nck) * ((size_t)(m + 1) * nck * NC) + ((size_t)J * nck + c % nck) * NC;
      const Cubic *lo = &below[(size_t)J * 4], *hi = &above[(size_t)J * 4];
      e[0] = (double)lo[0].c[0], e[1] = (double)lo[0].c[1], e[2] = (double)lo[0].c[2];
      e[3] = (double)hi[0].c[0], e[4] = (double)hi[0].c[1], e[5] = (double)hi[0].c[2];
      for (int k = 0; k < 4; ++k) e[6 + k] = (double)lo[1].c[k], e[10 + k] = (double)hi[1].c[k];
      if (pw) {
        for (int k = 0; k < 4; ++k) e[14 + k] = (double)lo[2].c[k], e[18 + k] = (double)hi[2].c[k];
        for (int k = 0; k < 3; ++k) e[22 + k] = (double)lo[3].c[k], e[25 + k] = (double)hi[3].c[k];
      }
    }
  }
}

}  // namespace

// (Re)build the gradient basis of b for the current model state.
int ensure_gradbasis(obhip_basis &b) {
  const obhip_model &m = *b.model;
  // like the reference's outerbase, b does not follow later changes of the model
  // (vignettes/learning.Rmd:48-54); mixing its tables with newer gradient tables would be
  // silently wrong, so ask for the rebuild instead
  if (b.md.model_version != m.version)
    return fail(OBHIP_ERR_STATE, "the model changed after this basis was built: call build() first");
  if (b.grad && b.grad->model_version == m.version) return 0;
  HostTimer ht_all("ensure_gradbasis (rebuild)");
  auto g = std::make_unique<obhip_gradbasis>();
  const uint64_t d = m.d, nh = m.nhyp();
  // tables: per hyper-parameter the rotmat_gradhyp block capped like ModelDev::rot
  std::vector<double> hrotg, hkd(m.M(), 0.0);
  std::vector<int> hhypst(d + 1);
  g->hyps_h.resize(nh);
  uint64_t gecol = b.md.Mc;
  for (uint64_t l = 0; l < d; ++l) {
    const DimDesc &D = b.md.dims_h[l];
    const uint64_t ml = m.m_of(l), o = m.knotptst[l];
    hhypst[l] = (int)m.hypst[l];
    for (uint64_t h = m.hypst[l]; h < m.hypst[l + 1]; ++h) {
      GradHyp &G = g->hyps_h[h];
      G.dim = (int)l;
      G.which = (int)(h - m.hypst[l]);
      G.rotgoff = (int)hrotg.size();
      G.gecol = (int)gecol;
      gecol += (uint64_t)D.ncol;
      hrotg.resize(hrotg.size() + ml * D.ncolp, 0.0);
      for (uint64_t j = 0; j < ml; ++j)
        for (int cc = 0; cc < D.ncol; ++cc)
          hrotg[G.rotgoff + j * D.ncolp + cc] = m.rotmat_gradhyp[(m.gest[h] + cc) * m.mmax + j];
    }
    if (m.kinds[l] == OBHIP_COV_MAT25POW)
      for (uint64_t j = 0; j < ml; ++j) {
        const double t = std::pow(m.knotpt[o + j], D.p0) / D.p1;
        hkd[o + j] = std::log(m.knotpt[o + j]) * t;  // covfuncs.cpp:234
      }
  }
  hhypst[d] = (int)m.hypst[d];
  for (uint64_t h = 0; h < nh; ++h) {  // the delta blocks behind all gradient blocks
    g->hyps_h[h].dcol = (int)gecol;
    gecol += (uint64_t)b.md.dims_h[m.hypmatch[h]].ncol - 1;
  }
  OB_TRY(g->hyps.upload(g->hyps_h.data(), nh));
  {
    std::vector<int> c0(nh);
    for (uint64_t h = 0; h < nh; ++h) c0[h] = g->hyps_h[h].gecol;
    if (nh) OB_TRY(g->ge0col.upload(c0.data(), nh));
  }
  OB_TRY(g->rotg.upload(hrotg.data(), hrotg.size()));
  OB_TRY(g->kd.upload(hkd.data(), hkd.size()));
  DevBuf<int> dhypst;
  OB_TRY(dhypst.upload(hhypst.data(), hhypst.size()));
  // interval tables of the mat25 / mat25pow dimensions (OBHIP_GRAD_KNOTLOOP=1: none, the
  // round-3 kernel -- A/B runs)
  const bool knotloop = getenv("OBHIP_GRAD_KNOTLOOP") && atoi(getenv("OBHIP_GRAD_KNOTLOOP")) != 0;
  HostTimer ht_tab("ensure_gradbasis: host tables + uploads");
  std::vector<GradTab> hgt(d);
  std::vector<int> rest;  // dimensions without a table: the knot loop
  std::vector<double> htab;
  std::vector<uint64_t> tabbed;  // dimensions with a table
  uint64_t htab_size = 0;
  bool any_tab = false;
  for (uint64_t l = 0; l < d; ++l) {
    const DimDesc &D = b.md.dims_h[l];
    const uint64_t ml = m.m_of(l);
    const bool pw = m.kinds[l] == OBHIP_COV_MAT25POW;
    const int nc = pw ? 28 : 14;
    const uint64_t mu = (ml + 1) / 2 * 2;
    const uint64_t per_level = (ml + 1) * (uint64_t)nc;
    hgt[l] = GradTab{-1, nc, (int)mu, 0, 0, 0};
    rest.push_back((int)l);
    // (D.kind differs from the model's kind when the knots spread too far for the separable
    // exponentials: those dimensions keep the per-knot exp)
    if (knotloop || (m.kinds[l] != OBHIP_COV_MAT25 && !pw) || D.kind != m.kinds[l] || ml > 127) continue;
    const uint64_t nck = std::min<uint64_t>((uint64_t)D.ncol, ((uint64_t)kGradTabMax - mu) / per_level);
    const uint64_t nchunks = ((uint64_t)D.ncol + nck - 1) / nck;
    const uint64_t size = mu + nchunks * nck * per_level;
    rest.pop_back();
    if (htab_size % 2) ++htab_size;
    hgt[l].off = (int)htab_size;
    hgt[l].nck = (int)nck;
    hgt[l].nchunks = (int)nchunks;
    hgt[l].chunk = (int)(nck * per_level);
    htab_size += size;
    tabbed.push_back(l);
    any_tab = true;
  }
  // the tables of the dimensions are independent (two extended-precision recurrences over the knots
  // per level each): filled on host threads, like the eigen-problems of obhip_model::build -- an
  // obfit function evaluation rebuilds them
  htab.assign(htab_size, 0.0);
  auto fill_dim = [&](uint64_t l) {
    const DimDesc &D = b.md.dims_h[l];
    const uint64_t ml = m.m_of(l), o = m.knotptst[l];
    const bool pw = m.kinds[l] == OBHIP_COV_MAT25POW;
    const uint64_t mu = (ml + 1) / 2 * 2;
    std::vector<int> ord(ml);
    std::vector<double> u(ml), us(ml);
    for (uint64_t j = 0; j < ml; ++j) {
      ord[j] = (int)j;
      u[j] = (pw ? std::pow(m.knotpt[o + j], D.p0) / D.p1 : m.knotpt[o + j] / D.p0) - D.p2;
    }
    std::stable_sort(ord.begin(), ord.end(), [&](int a2, int b2) { return u[a2] < u[b2]; });
    for (uint64_t j = 0; j < ml; ++j) us[j] = u[ord[j]];
    double *T = &htab[hgt[l].off];
    for (uint64_t j = 0; j < ml; ++j) T[j] = us[j];
    for (uint64_t j = ml; j < mu; ++j) T[j] = us[ml - 1];
    const uint64_t h0 = m.hypst[l];
    build_grad_tab((int)ml, D.ncol, hgt[l].nck, pw, D.p0, us, ord, &m.rotmat[o * m.mmax],
                   &m.rotmat_gradhyp[m.gest[h0] * m.mmax], pw ? &m.rotmat_gradhyp[m.gest[h0 + 1] * m.mmax] : nullptr,
                   m.mmax, &hkd[o], T + mu);
  };
  {
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const uint64_t nthr = std::min<uint64_t>({(uint64_t)tabbed.size(), (uint64_t)hw, 16});
    if (nthr <= 1) {
      for (uint64_t l : tabbed) fill_dim(l);
    } else {
      std::atomic<uint64_t> next{0};
      std::vector<std::thread> pool;
      for (uint64_t q = 0; q < nthr; ++q)
        pool.emplace_back([&] {
          for (uint64_t e = next++; e < tabbed.size(); e = next++) fill_dim(tabbed[e]);
        });
      for (std::thread &th : pool) th.join();
    }
  }
  DevBuf<GradTab> dgt;
  DevBuf<double> dtab;
  DevBuf<int> drest;
  if (any_tab) {
    OB_TRY(dgt.upload(hgt.data(), hgt.size()));
    OB_TRY(dtab.upload(htab.data(), htab.size()));
    if (!rest.empty()) OB_TRY(drest.upload(rest.data(), rest.size()));
  }

  // the combined array as an obhip_basis whose dimension table is extended by two
  // pseudo-dimensions per hyper-parameter: d + h, whose level j >= 1 is gradient level j - 1,
  // and d + nhyp + h, whose level j >= 1 is delta level j
  g->gb = std::make_unique<obhip_basis>();
  obhip_basis &gb = *g->gb;
  gb.model = b.model;
  gb.n = b.n;
  gb.n_pad = b.n_pad;
  gb.d = d + 2 * nh;
  gb.device = b.device;
  gb.md.cap = b.md.cap;
  gb.md.dims_h = b.md.dims_h;
  for (uint64_t h = 0; h < nh; ++h) {
    const DimDesc &D = b.md.dims_h[m.hypmatch[h]];
    DimDesc P = D;
    P.ccol0 = g->hyps_h[h].gecol;  // level j -> column gecol + j - 1
    P.ncol = D.ncol + 1;
    gb.md.cap.push_back((int64_t)D.ncol);
    gb.md.dims_h.push_back(P);
  }
  for (uint64_t h = 0; h < nh; ++h) {
    const DimDesc &D = b.md.dims_h[m.hypmatch[h]];
    DimDesc P = D;
    P.ccol0 = g->hyps_h[h].dcol;  // level j -> column dcol + j - 1
    gb.md.cap.push_back((int64_t)D.ncol - 1);
    gb.md.dims_h.push_back(P);
  }
  gb.md.Mc = gecol;
  gb.md.model_version = m.version;
  const uint64_t tiles = b.n_pad / kTileRows;
  OB_TRY(gb.bm.alloc(tiles * gecol * kTileRows));
  OB_TRY(gb.scale.alloc(b.n_pad));
  {
    ProfScope ps("build_basis_grad");
    if (any_tab) {
      // the dimensions without a table first (their product goes to scale), then the others
      if (!rest.empty())
        hipLaunchKernelGGL(k_build_basis_grad, dim3((unsigned)tiles), dim3(256), 0, cur_stream(),
                           b.md.dims.p, g->hyps.p, dhypst.p, b.md.ka.p, b.md.kb.p, g->kd.p, b.md.rot.p,
                           g->rotg.p, b.x.p, b.n, (int)rest.size(), gecol, drest.p, gb.bm.p, gb.scale.p);
      const size_t lds = (size_t)kGradTabMax * sizeof(double);
      OB_TRY(ensure_dyn_lds((const void *)k_build_basis_grad_tab, lds));
      hipLaunchKernelGGL(k_build_basis_grad_tab, dim3((unsigned)((tiles + 15) / 16)), dim3(1024), lds, cur_stream(),
                         b.md.dims.p, g->hyps.p, dhypst.p, dgt.p, dtab.p, b.x.p, b.n, (int)d, gecol, tiles,
                         rest.empty() ? 0 : 1, gb.bm.p, gb.scale.p);
    } else {
      hipLaunchKernelGGL(k_build_basis_grad, dim3((unsigned)tiles), dim3(256), 0, cur_stream(),
                         b.md.dims.p, g->hyps.p, dhypst.p, b.md.ka.p, b.md.kb.p, g->kd.p, b.md.rot.p,
                         g->rotg.p, b.x.p, b.n, (int)d, gecol, (const int *)nullptr, gb.bm.p, gb.scale.p);
    }
    OB_HIP(hipGetLastError());
    OB_HIP(hipStreamSynchronize(cur_stream()));  // dhypst and the tables are locals
  }
  g->model_version = m.version;
  static uint64_t next_id = 1;
  g->id = next_id++;
  b.grad = std::move(g);
  return 0;
}

namespace {

// squared store of the gradient basis (basematsq / basematsq_gradhyp, modandbase.cpp:581,
// 588-590): basemat columns squared, gradient column t of a hyper-parameter -> 2 * it *
// basemat level t of its dimension (the ones column at level 0); scale squared
__global__ void __launch_bounds__(256)
k_square_gradbasis(const double *__restrict__ src, const double *__restrict__ scale,
                   const uint32_t *__restrict__ pair, uint64_t Mc, uint64_t Mtot,
                   double *__restrict__ dst, double *__restrict__ scale_sq) {
  const uint64_t tile = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double *s = src + tile * Mtot * kTileRows + lane;
  double *o = dst + tile * Mtot * kTileRows + lane;
  for (uint64_t c = wave; c < Mtot; c += 4) {
    const double v = s[c * kTileRows];
    o[c * kTileRows] = c < Mc ? v * v : 2.0 * v * s[(uint64_t)pair[c - Mc] * kTileRows];
  }
  if (wave == 0) {
    const double sc = scale[tile * kTileRows + lane];
    scale_sq[tile * kTileRows + lane] = sc * sc;
  }
}

}  // namespace

int ensure_gradbasis_sq(obhip_basis &b) {
  OB_TRY(ensure_gradbasis(b));
  obhip_gradbasis &g = *b.grad;
  if (g.gbsq) return 0;
  const obhip_basis &gb = *g.gb;
  const uint64_t Mc = b.md.Mc, Mtot = gb.md.Mc;
  std::vector<uint32_t> pair(Mtot - Mc, 0u);
  for (size_t h = 0; h < g.hyps_h.size(); ++h) {
    const DimDesc &D = b.md.dims_h[g.hyps_h[h].dim];
    for (int t = 1; t < D.ncol; ++t) {
      pair[g.hyps_h[h].gecol - Mc + t] = (uint32_t)(D.ccol0 + t - 1);
      // delta_sq[t] = ge_sq[t] - basemat[t]^2 ge_sq[0] = 2 basemat[t] delta[t]
      pair[g.hyps_h[h].dcol - Mc + t - 1] = (uint32_t)(D.ccol0 + t - 1);
    }
  }
  DevBuf<uint32_t> dpair;
  OB_TRY(dpair.upload(pair.data(), pair.size()));
  auto sq = std::make_unique<obhip_basis>();
  sq->model = gb.model;
  sq->n = gb.n;
  sq->n_pad = gb.n_pad;
  sq->d = gb.d;
  sq->device = gb.device;
  sq->md.cap = gb.md.cap;
  sq->md.dims_h = gb.md.dims_h;
  sq->md.Mc = Mtot;
  sq->md.model_version = gb.md.model_version;
  const uint64_t tiles = gb.n_pad / kTileRows;
  OB_TRY(sq->bm.alloc(tiles * Mtot * kTileRows));
  OB_TRY(sq->scale.alloc(gb.n_pad));
  hipLaunchKernelGGL(k_square_gradbasis, dim3((unsigned)tiles), dim3(256), 0, cur_stream(), gb.bm.p,
                     gb.scale.p, dpair.p, Mc, Mtot, sq->bm.p, sq->scale.p);
  OB_HIP(hipGetLastError());
  OB_HIP(hipStreamSynchronize(cur_stream()));  // dpair is a local
  g.gbsq = std::move(sq);
  return 0;
}

}  // namespace obhip
