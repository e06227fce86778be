// Conditional moments of the fitted mean for gfx950 (conditional.cpp; include/obhip.h, "conditional moments";
// DESIGN.md section 36).  No reference counterpart.  With E the noise dimensions, S the others, g(k) the group of
// term k by its levels on E and P_ik = s^S_i prod_{l in S, t_kl > 0} r_{l,t_kl}(x_il):
//   c_ij[g] = sum_{k in g} theta_kj P_ik     M_ij = c_ij^T mE     W_ij = c_ij^T K c_ij,
//   mE[g] = prod_{l in E} m_l[.],  K[g,g'] = sum_{l in E} (prod_{i<l} A_i) C_l (prod_{i>l} m_i m_i) on the tuples.
//
// k_cond_tables   mE and K.  Lane = group of tile I, the partner of tile J >= I wave-uniform, A, C and m m^T of the
//                 noise dimensions in LDS (stage_pair_tables); the forward sweep of k_sobol_pairs over the noise
//                 dimensions alone; the entry is written where k_sobol_pairs would add it.  An unordered pair is
//                 formed once, by the lane of the lower group, and written to both places: K is symmetric to the bit.
// k_cond_coef     per 64-row tile (lane = row, 8 waves): build_tile_side over S into a tile in LDS or, HBM, in a
//                 per-block slice of pooled scratch; then a wave takes (group, block of kCondRC responses) items and
//                 adds the group's terms in ascending term order.  c is stored group-major, c[(j Gp + g) npad + i],
//                 512 contiguous bytes per store, exact zeros at the rows and groups of the padding.
// k_cond_ck       Y = c K on the matrix cores (v_mfma_f64_16x16x4_f64): a wave holds 16 groups x 64 rows of Y, the
//                 A operand 16 x 4 of K (read through its symmetry, 16 contiguous doubles), the B operand 4 groups x
//                 16 rows of c; g ascends in fours.  A column of the product is a row of the call: nothing a row gets
//                 depends on its neighbours or on where the chunk starts.
// k_cond_moments  thread = (row, response): M = sum_g c_g mE[g], W = sum_g c_g Y_g, g ascending.
// k_cond_grad     per 64-row tile: build_tile_side_dx over S; a wave takes (dimension a of S, block of responses)
//                 items and contracts the view of a (the terms with a factor there) with the per-row coefficients:
//                   dM/dx_a = rho_a M + s sum_k theta_k mE[g(k)] E_ka r'      dW/dx_a = 2 (rho_a W + s sum_k theta_k Y[g(k)] E_ka r')
//                 -- the mean-gradient contraction of k_predict_dx / k_acquire_dx with theta_k Y_i[g(k)] for theta.
// Every sum has a fixed order that does not depend on where a row stands, nothing is atomic: two calls give the
// same bits and a chunked call those of the unchunked one.  A row with a coordinate that is not finite is evaluated
// at 0.5 like a row of the padding and gets NaN.
#include "obhip_internal.h"
#include "conditional_plan.h"
#include "device_dx.h"
#include "pair_sum.h"
#include "product_tile.h"

namespace obhip {

namespace {

constexpr int kCdThreads = 512, kCdWaves = kCdThreads / 64;
constexpr int RC = (int)kCondRC;

// dynamic LDS: [A: n_cov + 1][C: n_cov + 1][m m^T: n_cov + 1] of the noise dimensions, whose compact tables mtab and
// ctab are (conditional.cpp gathers them).  meta: [L_e][offset of m_e][offset of C_e] of the ne noise dimensions, glev: G x ne levels
__global__ void __launch_bounds__(kSobolTW)
k_cond_tables(const uint8_t *__restrict__ glev, const int *__restrict__ meta, int G, int ne, int n_cov,
              const double *__restrict__ mtab, const double *__restrict__ ctab, double *__restrict__ mE,
              double *__restrict__ K, uint64_t ldk) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *tA = smem, *tC = tA + n_cov + 1, *tM = tC + n_cov + 1;
  int I, J;
  tile_pair(blockIdx.x, (G + kSobolTW - 1) / kSobolTW, I, J);
  stage_pair_tables(
      meta, ne,
      [&](int i, int ia, int ib) {
        const double c = ctab[i], mm = mtab[ia] * mtab[ib];
        tC[i] = c;
        tM[i] = mm;
        tA[i] = c + mm;
      },
      [] {});
  const int g = I * kSobolTW + threadIdx.x;
  if (g >= G) return;  // (no barrier below)
  const uint8_t *lv = glev + (uint64_t)g * ne;
  if (I == J) {
    double pr = 1.0;
    for (int l = 0; l < ne; ++l) pr *= mtab[meta[ne + l] + lv[l]];
    mE[g] = pr;
  }
  const int nj = min(kSobolTW, G - J * kSobolTW);
  for (int kk = 0; kk < nj; ++kk) {
    const int g2 = J * kSobolTW + kk;  // (wave-uniform)
    if (g2 < g) continue;              // the lane of the lower group forms the pair
    const uint8_t *lp = glev + (uint64_t)g2 * ne;
    double pa = 1.0, dd = 0.0;
    for (int l = 0; l < ne; ++l) {
      const int idx = meta[2 * ne + l] + (int)lv[l] * meta[l] + lp[l];
      dd = fma(tM[idx], dd, pa * tC[idx]);  // prod A - prod m m up to l
      pa *= tA[idx];
    }
    K[(uint64_t)g * ldk + g2] = dd;
    K[(uint64_t)g2 * ldk + g] = dd;
  }
}

// the tile's row, whether it is in the chunk and whether its coordinates are finite
struct TileRow {
  uint64_t row;
  bool valid, fin;
};
__device__ __forceinline__ TileRow tile_row(const CondChunk &a, uint64_t tl, int lane) {
  TileRow r;
  r.row = tl * kTileRows + lane;
  r.valid = r.row < a.nr;
  r.fin = r.valid;
  for (int s = 0; s < a.nside && r.fin; ++s) r.fin = isfinite(a.x[(uint64_t)s * a.ldx + r.row]);
  return r;
}

// dynamic LDS: [tile: mu x 64 unless HBM][scale partials: 8 x 64]
template <bool HBM>
__global__ void __launch_bounds__(kCdThreads) k_cond_coef(const CondChunk a) {
  extern __shared__ double lds[];
  double *tile = HBM ? a.scratch + (size_t)blockIdx.x * a.mu * kTileRows : lds;
  double *red = HBM ? lds : lds + (size_t)a.mu * kTileRows;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nrc = (a.q + RC - 1) / RC, items = a.Gp * nrc;
  for (uint64_t tl = blockIdx.x; tl < a.ntiles; tl += gridDim.x) {
    const TileRow r = tile_row(a, tl, lane);
    const StoreTile<kTileRows> store{tile, a.cpos, lane, a.mu};
    build_tile_side<kCdWaves>(a.dims, a.ka, a.kb, a.kc, a.rot, a.tab, a.side, a.nside, a.x, a.ldx, r.row, r.fin, wave,
                              wave, store, red);
    __syncthreads();
    const double s = tile_scale<kCdWaves>(red, lane);
    for (int it = wave; it < items; it += kCdWaves) {
      const int g = it / nrc, j0 = it % nrc * RC;
      double acc[RC];
#pragma unroll
      for (int c = 0; c < RC; ++c) acc[c] = 0.0;
      if (g < a.G) {
        const int e1 = (int)a.goff[g + 1];
        for (int e = (int)a.goff[g]; e < e1; ++e) {
          const int k = (int)a.order[e];  // (wave-uniform)
          const double pr = term_prod_mem(tile, a.colsw + (size_t)k * a.W2, a.W2, lane, 1.0);
#pragma unroll
          for (int c = 0; c < RC; ++c)
            if (j0 + c < a.q) acc[c] = fma(a.Theta[(uint64_t)(j0 + c) * a.p + k], pr, acc[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < RC; ++c)
        if (j0 + c < a.q)
          a.C[((uint64_t)(j0 + c) * a.Gp + g) * a.npad + r.row] =
              g < a.G && r.valid ? (r.fin ? s * acc[c] : NAN) : 0.0;
    }
    __syncthreads();  // the tile and the partials are free for the next tile
  }
}

// grid (tiles of 64 rows, blocks of 64 groups, responses); wave = 16 groups
__global__ void __launch_bounds__(256)
k_cond_ck(const double *__restrict__ C, const double *__restrict__ K, int Gp, uint64_t npad, double *__restrict__ Y) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gp0 = (blockIdx.y * 4 + wave) * 16;
  if (gp0 >= Gp) return;
  const int mn = lane & 15, kq = lane >> 4;
  const uint64_t i0 = (uint64_t)blockIdx.x * kTileRows;
  const double *__restrict__ Cj = C + (uint64_t)blockIdx.z * Gp * npad + i0 + mn;
  d4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  for (int g0 = 0; g0 < Gp; g0 += 4) {
    const double av = K[(uint64_t)(g0 + kq) * Gp + gp0 + mn];  // A[m][k] = K[gp0 + m][g0 + k], by symmetry
    const double *__restrict__ cb = Cj + (uint64_t)(g0 + kq) * npad;  // B[k][n] = c[g0 + k][row n]
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = mfma(av, cb[16 * c], acc[c]);
  }
  double *__restrict__ Yj = Y + (uint64_t)blockIdx.z * Gp * npad + i0 + mn;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) Yj[(uint64_t)(gp0 + kq + 4 * r) * npad + 16 * c] = acc[c][r];  // D[k + 4 r][n]
}

// grid (row blocks of 256, responses)
__global__ void __launch_bounds__(256)
k_cond_moments(const double *__restrict__ C, const double *__restrict__ Y, const double *__restrict__ mE, int G,
               int Gp, uint64_t npad, uint64_t nr, uint64_t row0, uint64_t n, double *__restrict__ Mw,
               double *__restrict__ Ww, double *__restrict__ mean, double *__restrict__ var) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npad) return;
  const uint64_t j = blockIdx.y;
  const double *__restrict__ c = C + j * Gp * npad + i, *__restrict__ y = Y + j * Gp * npad + i;
  double m = 0.0, w = 0.0;
  for (int g = 0; g < G; ++g) {
    const double cg = c[(uint64_t)g * npad];
    m = fma(cg, mE[g], m);
    w = fma(cg, y[(uint64_t)g * npad], w);
  }
  Mw[j * npad + i] = m;
  Ww[j * npad + i] = w;
  if (i < nr) {
    if (mean) mean[j * n + row0 + i] = m;
    if (var) var[j * n + row0 + i] = w;
  }
}

// dynamic LDS: [tile: (2 mu - 1 + nside) x 64 unless HBM][scale partials: 8 x 64]
template <bool HBM>
__global__ void __launch_bounds__(kCdThreads) k_cond_grad(const CondChunk a) {
  extern __shared__ double lds[];
  const int ncols = 2 * a.mu - 1 + a.nside;
  double *tile = HBM ? a.scratch + (size_t)blockIdx.x * ncols * kTileRows : lds;
  double *red = HBM ? lds : lds + (size_t)ncols * kTileRows;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nrc = (a.q + RC - 1) / RC, items = a.nside * nrc;
  const int stride = a.W2 + 2;
  for (uint64_t tl = blockIdx.x; tl < a.ntiles; tl += gridDim.x) {
    const TileRow r = tile_row(a, tl, lane);
    const StoreTile<kTileRows> store{tile, a.cpos, lane, a.mu};
    build_tile_side_dx<kCdWaves>(a.dims, a.ka, a.kb, a.kc, a.rot, a.tab, a.dtab, a.side, a.nside, a.x, a.ldx, r.row,
                                 r.fin, wave, wave, store, red);
    __syncthreads();
    const double s = tile_scale<kCdWaves>(red, lane);
    for (int it = wave; it < items; it += kCdWaves) {
      const int sa = it / nrc, j0 = it % nrc * RC;
      const double *__restrict__ yrow[RC];
      double gm[RC], gv[RC];
#pragma unroll
      for (int c = 0; c < RC; ++c) {
        gm[c] = gv[c] = 0.0;
        yrow[c] = a.Y + (uint64_t)min(j0 + c, a.q - 1) * a.Gp * a.npad + r.row;
      }
      const int e1 = (int)a.voff[sa + 1];
      for (int e = (int)a.voff[sa]; e < e1; ++e) {
        const uint32_t *ent = a.vw + (size_t)e * stride;  // (wave-uniform)
        const double E = term_prod_mem(tile, ent, a.W2, lane, 1.0);
        const int own = (int)ent[a.W2];
        const uint32_t k = ent[a.W2 + 1], g = a.gof[k];
        const double Ed = E * tile[(a.mu + own - 1) * kTileRows + lane];
        const double mg = a.mE[g];
#pragma unroll
        for (int c = 0; c < RC; ++c)
          if (j0 + c < a.q) {
            const double th = a.Theta[(uint64_t)(j0 + c) * a.p + k];
            gm[c] = fma(th * mg, Ed, gm[c]);
            gv[c] = fma(th * yrow[c][(uint64_t)g * a.npad], Ed, gv[c]);
          }
      }
      if (r.valid) {
        const double rho = tile[(2 * a.mu - 1 + sa) * kTileRows + lane];
#pragma unroll
        for (int c = 0; c < RC; ++c)
          if (j0 + c < a.q) {
            const uint64_t j = (uint64_t)(j0 + c);
            const uint64_t o = (j * a.nside + sa) * a.n + a.row0 + r.row;
            if (a.gradmean) a.gradmean[o] = r.fin ? fma(rho, a.Mw[j * a.npad + r.row], s * gm[c]) : NAN;
            if (a.gradvar) a.gradvar[o] = r.fin ? 2.0 * fma(rho, a.Ww[j * a.npad + r.row], s * gv[c]) : NAN;
          }
      }
    }
    __syncthreads();  // the tile and the partials are free for the next tile
  }
}

template <bool HBM, bool DX>
int run_cond_rows(CondChunk a) {
  const uint64_t ncols = DX ? 2 * (uint64_t)a.mu - 1 + a.nside : (uint64_t)a.mu;
  const size_t lds = ((HBM ? 0 : ncols) + kCdWaves) * kTileRows * sizeof(double);
  auto kernel = DX ? k_cond_grad<HBM> : k_cond_coef<HBM>;
  OB_TRY(ensure_dyn_lds((const void *)kernel, lds));
  int dev = 0;
  (void)hipGetDevice(&dev);
  uint64_t nblk = std::min<uint64_t>(a.ntiles, (uint64_t)device_cus(dev) * 2);
  DevBuf<double> scratch;
  if (HBM) {
    nblk = hbm_tile_blocks(nblk, ncols);
    OB_TRY(scratch.alloc(nblk * ncols * kTileRows));
    a.scratch = scratch.p;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(kCdThreads), lds, cur_stream(), a);
  OB_HIP(hipGetLastError());
  // (scratch goes back to the pool under this stream: handed out again to work queued behind the kernel)
  return 0;
}

}  // namespace

// the row kernels keep the tile of S in LDS: at most 8 factors per term on S, the derivative tile within kLdsBudget
bool cond_rows_supports(uint64_t mu, uint64_t nside, uint64_t w) {
  return w >= 2 && w <= 8 && (2 * mu - 1 + nside + kCdWaves) * kTileRows * sizeof(double) <= kLdsBudget;
}

int launch_cond_tables(const uint8_t *d_glev, const int *d_meta, uint64_t G, uint64_t ne, uint64_t n_cov,
                       const double *d_mtab, const double *d_ctab, double *d_mE, double *d_K, uint64_t ldk) {
  ProfScope ps("cond_tables");
  const int nt = (int)((G + kSobolTW - 1) / kSobolTW), npairs = nt * (nt + 1) / 2;
  const size_t lds = cond_tables_lds(n_cov);
  OB_TRY(ensure_dyn_lds((const void *)k_cond_tables, lds));
  hipLaunchKernelGGL(k_cond_tables, dim3(npairs), dim3(kSobolTW), lds, cur_stream(), d_glev, d_meta, (int)G, (int)ne,
                     (int)n_cov, d_mtab, d_ctab, d_mE, d_K, ldk);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_cond_chunk(CondChunk c) {
  const CondChunk &a = c;
  c.scratch = nullptr;
  {
    ProfScope ps("cond_coef");
    OB_TRY(c.fused ? (run_cond_rows<false, false>(a)) : (run_cond_rows<true, false>(a)));
  }
  {
    ProfScope ps("cond_ck");
    hipLaunchKernelGGL(k_cond_ck, dim3((unsigned)a.ntiles, (unsigned)((a.Gp + 63) / 64), (unsigned)a.q), dim3(256), 0,
                       cur_stream(), (const double *)c.C, c.K, a.Gp, c.npad, c.Y);
    OB_HIP(hipGetLastError());
  }
  {
    ProfScope ps("cond_moments");
    hipLaunchKernelGGL(k_cond_moments, dim3((unsigned)((c.npad + 255) / 256), (unsigned)a.q), dim3(256), 0, cur_stream(),
                       (const double *)c.C, (const double *)c.Y, c.mE, a.G, a.Gp, c.npad, c.nr, c.row0, c.n, c.Mw, c.Ww,
                       c.mean, c.var);
    OB_HIP(hipGetLastError());
  }
  if (c.gradmean || c.gradvar) {
    ProfScope ps("cond_grad");
    OB_TRY(c.fused ? (run_cond_rows<false, true>(a)) : (run_cond_rows<true, true>(a)));
  }
  return 0;
}

}  // namespace obhip
