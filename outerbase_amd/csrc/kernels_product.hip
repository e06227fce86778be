// The predictor on the product of two input blocks (include/obhip.h, "product of two input blocks";
// DESIGN.md section 24).  The dimensions are split into a block A, read from xa (na rows), and a block B,
// read from xb (nb rows); a design-matrix entry of the pair (i, j) separates into
//   sA_i sB_j U_ik V_jk,   U_ik = prod_{l in A, t_kl > 0} r_{l,t_kl}(xa_i),   V_jk likewise over B,
// so mean[i, j] = sA_i sB_j sum_k theta_k U_ik V_jk is a GEMM with inner dimension p whose operands are
// generated on the fly, and var[i, j] = sA_i^2 sB_j^2 sum_k c_k U_ik^2 V_jk^2 + e^{2 sigma} a second one.
//
//   k_predict_product  workgroup = 64 rows of xa x 64 rows of xb, four waves.  Phase 1: the used columns of
//                      the A dimensions at the xa rows and of the B dimensions at the xb rows go to two LDS
//                      tiles (build_tile_side, lane = row).  Phase 2: wave (ig, jg) owns the 32 x 32 block of
//                      pairs (A rows 32 ig .., B rows 32 jg ..) as 2 x 2 accumulators of
//                      v_mfma_f64_16x16x4_f64 and runs over the terms in steps of four; a lane forms the side
//                      products of its (row, term) from the tiles -- no staging of U and V; the terms' column
//                      lists and coefficients pass through LDS in chunks of 256, two barriers per chunk.  The B rows sit on the M side of the instruction and the A rows on the N side, so
//                      that the sixteen lanes of an accumulator register hold consecutive i, the fast index of
//                      the output.  Epilogue: store, or the likelihood sums over the tile's A rows.
//   k_product_expand / _scatter / _lik_rows   the row route for term sets outside the kernel's domain.
//   k_product_sum_tiles                       the A tiles' partial sums added in ascending order.
//
// The launch arguments, the staged contraction (pp_contract) and the pieces of the likelihood epilogue are in
// product_tile.h, shared with the gradient kernel of kernels_product_dx.hip.
#include "obhip_internal.h"
#include "product_tile.h"
#include "vec_ops.h"

namespace obhip {

namespace {

template <bool VAR, bool LIK>
__global__ void __launch_bounds__(kPpThreads, 2)
k_predict_product(const PpArgs a) {
  extern __shared__ double lds[];
  double *ta = lds;                              // [mu_a][64]
  double *tb = ta + (size_t)a.mu_a * kTileRows;  // [mu_b][64]
  double *pa = tb + (size_t)a.mu_b * kTileRows;  // [4][64] scale shares of the A dimensions
  double *pb = pa + kPpWaves * kTileRows;        // [4][64] of the B dimensions
  double *sa = pb + kPpWaves * kTileRows;        // [64] sA of the tile's A rows
  double *sb = sa + kTileRows;                   // [64] sB of its B rows
  double *red = sb + kTileRows;                  // [2][4][64] likelihood partials per 16-row group of A
  PpChunk ch;
  ch.th = red + 2 * 4 * kTileRows;
  ch.cv = ch.th + kPpTerms;
  ch.cw_a = (uint32_t *)(ch.cv + kPpTerms);
  ch.cw_b = ch.cw_a + kPpTerms * a.wa2;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t at = a.atile0 + (uint64_t)blockIdx.x / a.tiles_b, bt = (uint64_t)blockIdx.x % a.tiles_b;
  const uint64_t i0 = at * kTileRows, j0 = bt * kTileRows;
  {
    const StoreTile<kTileRows> st_a{ta, a.cpos_a, lane, a.mu_a};
    build_tile_side<kPpWaves>(a.dims, a.ka, a.kb, a.kc, a.rot, a.tab, a.side_a, a.nda, a.xa, a.na, i0 + lane,
                              i0 + lane < a.na, wave, wave, st_a, pa);
    // the B dimensions are dealt on from the wave behind the one that took the last A dimension
    const int slot_b = (wave + kPpWaves - a.nda % kPpWaves) % kPpWaves;
    const StoreTile<kTileRows> st_b{tb, a.cpos_b, lane, a.mu_b};
    build_tile_side<kPpWaves>(a.dims, a.ka, a.kb, a.kc, a.rot, a.tab, a.side_b, a.ndb, a.xb, a.nb, j0 + lane,
                              j0 + lane < a.nb, wave, slot_b, st_b, pb);
  }
  __syncthreads();
  if (wave == 0) sa[lane] = tile_scale<kPpWaves>(pa, lane);
  if (wave == 1) sb[lane] = tile_scale<kPpWaves>(pb, lane);
  __syncthreads();

  const int m = lane & 15, kq = lane >> 4;
  const int ig = wave & 1, jg = wave >> 1;
  const int ra = 32 * ig + m, rb = 32 * jg + m;
  for (int r = 0; r < a.qc; ++r) {
    d4 acc[2][2], accv[2][2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int c = 0; c < 2; ++c) acc[b][c] = accv[b][c] = d4{0.0, 0.0, 0.0, 0.0};
    const double *th = a.theta + (uint64_t)r * a.p;
    // the variance is the same for every response: it rides along with the first one
    if (VAR && r == 0) pp_contract<true>(a, ta, tb, th, ch, kq, ra, rb, acc, accv);
    else pp_contract<false>(a, ta, tb, th, ch, kq, ra, rb, acc, accv);

    if constexpr (!LIK) {
      double *mean = a.mean + (uint64_t)r * a.nb * a.lda;
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int jl = 32 * jg + 16 * b + kq + 4 * rr;
          const uint64_t j = j0 + jl;
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int il = 32 * ig + 16 * c + m;
            const uint64_t i = i0 + il;
            if (i < a.na && j < a.nb) {
              const double s = sa[il] * sb[jl];
              mean[j * a.lda + i] = acc[b][c][rr] * s;
              if (VAR && r == 0) a.var[j * a.lda + i] = accv[b][c][rr] * (s * s) + a.e2sigma;
            }
          }
        }
    } else {
      double yv[2], ov[2];
      bool ok[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const uint64_t i = i0 + 32 * ig + 16 * c + m;
        ok[c] = i < a.na;  // the rows beyond na leave the sums, not only the output
        yv[c] = ok[c] ? a.y[i] : 0.0;
        ov[c] = (ok[c] && a.obsvar) ? a.obsvar[i] : 0.0;
      }
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int jl = 32 * jg + 16 * b + kq + 4 * rr;
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int il = 32 * ig + 16 * c + m;
            const double s = sa[il] * sb[jl];
            const double var = VAR ? accv[b][c][rr] * (s * s) + a.e2sigma : a.e2sigma;
            double t1, t2;
            lik_terms(ok[c], yv[c], acc[b][c][rr] * s, var, ov[c], t1, t2);
            t1 = sum16(t1);
            t2 = sum16(t2);
            if (m == 0) {
              red[(0 * 4 + 2 * ig + c) * kTileRows + jl] = t1;
              red[(1 * 4 + 2 * ig + c) * kTileRows + jl] = t2;
            }
          }
        }
      __syncthreads();
      if (threadIdx.x < 2 * kTileRows) {
        const int w = threadIdx.x >> 6, jl = threadIdx.x & 63;
        const double *rw = red + (size_t)w * 4 * kTileRows + jl;
        const double sum = ((rw[0] + rw[kTileRows]) + rw[2 * kTileRows]) + rw[3 * kTileRows];
        if (j0 + jl < a.nb) a.part[((uint64_t)w * a.tiles_a + at) * a.nb + j0 + jl] = sum;
      }
    }
  }
}

// ---- the row route ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_product_expand(const int *__restrict__ dim_src, const double *__restrict__ xa, uint64_t na,
                 const double *__restrict__ xb, uint64_t nb, uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj,
                 double *__restrict__ X) {
  const uint64_t rows = ni * nj;
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows) return;
  const int l = blockIdx.y, src = dim_src[l];
  const uint64_t ii = e % ni, jj = e / ni;
  X[(uint64_t)l * rows + e] = src >= 0 ? xa[(uint64_t)src * na + i0 + ii] : xb[(uint64_t)(-src - 1) * nb + j0 + jj];
}

__global__ void __launch_bounds__(256)
k_product_scatter(const double *__restrict__ src, uint64_t nb, uint64_t lda, uint64_t i0, uint64_t ni, uint64_t j0,
                  uint64_t nj, double *__restrict__ dst) {
  const uint64_t rows = ni * nj;
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows) return;
  const uint64_t r = blockIdx.y, ii = e % ni, jj = e / ni;
  dst[(r * nb + j0 + jj) * lda + i0 + ii] = src[r * rows + e];
}

// one wave per (A tile of the chunk, B row): lane = row of the tile; the sixteen-row groups by the fused
// kernel's butterfly, then the four groups in ascending order
__global__ void __launch_bounds__(64)
k_product_lik_rows(const double *__restrict__ mean, const double *__restrict__ var, double e2sigma,
                   const double *__restrict__ y, const double *__restrict__ obsvar, uint64_t nb, uint64_t tiles_a,
                   uint64_t i0, uint64_t ni, uint64_t j0, uint64_t ctiles, double *__restrict__ part) {
  const int lane = threadIdx.x;
  const uint64_t ct = (uint64_t)blockIdx.x % ctiles, jj = (uint64_t)blockIdx.x / ctiles;
  const uint64_t ii = ct * kTileRows + lane;
  const bool ok = ii < ni;
  const uint64_t e = jj * ni + (ok ? ii : 0);
  double t1, t2;
  lik_terms(ok, ok ? y[i0 + ii] : 0.0, mean[e], var ? var[e] : e2sigma, (ok && obsvar) ? obsvar[i0 + ii] : 0.0, t1, t2);
  t1 = sum16(t1);
  t2 = sum16(t2);
  const double s1 = ((__shfl(t1, 0, 64) + __shfl(t1, 16, 64)) + __shfl(t1, 32, 64)) + __shfl(t1, 48, 64);
  const double s2 = ((__shfl(t2, 0, 64) + __shfl(t2, 16, 64)) + __shfl(t2, 32, 64)) + __shfl(t2, 48, 64);
  if (lane == 0) {
    const uint64_t at = i0 / kTileRows + ct;
    part[(0 * tiles_a + at) * nb + j0 + jj] = s1;
    part[(1 * tiles_a + at) * nb + j0 + jj] = s2;
  }
}

__global__ void __launch_bounds__(256)
k_product_sum_tiles(const double *__restrict__ part, uint64_t tiles_a, uint64_t nb, double *__restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nb) return;
  const uint64_t w = blockIdx.y;
  double s = 0.0;
  for (uint64_t at = 0; at < tiles_a; ++at) s += part[(w * tiles_a + at) * nb + j];
  out[w * nb + j] = s;
}

__global__ void __launch_bounds__(256) k_check_nonneg(const double *__restrict__ v, uint64_t n, int *__restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && !(v[i] >= 0.0 && v[i] <= 1.79769313486231570815e308)) *flag = 1;
}

// grid.x of the chunked one-dimensional launches
constexpr uint64_t kMaxGridX = 0x7fffffffull;

}  // namespace

size_t predict_product_lds(uint64_t mu_a, uint64_t mu_b, uint64_t wa, uint64_t wb) {
  return ((mu_a + mu_b) * kTileRows + kPpStage + 2 * kPpTerms) * sizeof(double) +
         kPpTerms * (wa / 2 + wb / 2) * sizeof(uint32_t);
}

bool predict_product_supports(uint64_t mu_a, uint64_t mu_b, uint64_t wa, uint64_t wb) {
  return wa >= 2 && wb >= 2 && wa % 2 == 0 && wb % 2 == 0 && predict_product_lds(mu_a, mu_b, wa, wb) <= kLdsBudget;
}

int launch_predict_product(const obhip_model &m, obhip_terms &t, const ProductCall &c) {
  ProfScope ps("predict_product");
  const obhip_terms::Product &pr = t.product;
  const ModelDev &md = t.pred_md;
  const bool lik = c.mean == nullptr;
  const bool var = c.coeffvar != nullptr && (lik || c.var != nullptr);
  PpArgs a{};
  a.dims = md.dims.p, a.ka = md.ka.p, a.kb = md.kb.p, a.kc = md.kc.p, a.rot = md.rot.p, a.tab = md.tab.p;
  a.side_a = pr.side_a.p, a.side_b = pr.side_b.p;
  a.nda = (int)(m.d - pr.dims_b.size()), a.ndb = (int)pr.dims_b.size();
  a.cpos_a = pr.cpos_a.p, a.cpos_b = pr.cpos_b.p;
  a.mu_a = (int)pr.mu_a, a.mu_b = (int)pr.mu_b;
  a.cw_a = (const uint32_t *)pr.cols_a.p, a.cw_b = (const uint32_t *)pr.cols_b.p;
  a.wa2 = (int)(pr.wa / 2), a.wb2 = (int)(pr.wb / 2), a.p = (int)t.p;
  a.coeffvar = c.coeffvar, a.e2sigma = std::exp(2.0 * c.sigma);
  a.xa = c.xa, a.xb = c.xb, a.na = c.na, a.nb = c.nb;
  a.tiles_a = (c.na + kTileRows - 1) / kTileRows, a.tiles_b = (c.nb + kTileRows - 1) / kTileRows;
  a.lda = c.lda, a.var = c.var, a.y = c.y, a.obsvar = c.obsvar, a.part = c.part;
  if (a.tiles_b > kMaxGridX) return fail(OBHIP_ERR_INVALID, "predict_product: more than 2^37 rows in xb");
  const size_t lds = predict_product_lds(pr.mu_a, pr.mu_b, pr.wa, pr.wb);
  // a launch takes as many A tiles as keep tiles_a x tiles_b within the grid's first dimension
  const uint64_t at_per = std::max<uint64_t>(1, kMaxGridX / a.tiles_b);
  constexpr uint64_t kRespBlock = 16;  // responses per pass over the tiles
  for (uint64_t r0 = 0; r0 < c.q; r0 += kRespBlock) {
    a.theta = c.theta + r0 * t.p;
    a.qc = (int)std::min(kRespBlock, c.q - r0);
    a.mean = lik ? nullptr : c.mean + r0 * c.nb * c.lda;
    const bool v = var && r0 == 0;
    for (uint64_t at0 = 0; at0 < a.tiles_a; at0 += at_per) {
      a.atile0 = at0;
      const dim3 grid((unsigned)(std::min(at_per, a.tiles_a - at0) * a.tiles_b));
      OB_TRY(pick_bool(v, [&](auto VAR) {
        return pick_bool(lik, [&](auto LIK) {
          constexpr auto kernel = k_predict_product<VAR(), LIK()>;
          OB_TRY(ensure_dyn_lds((const void *)kernel, lds));
          hipLaunchKernelGGL(kernel, grid, dim3(kPpThreads), lds, cur_stream(), a);
          OB_HIP(hipGetLastError());
          return 0;
        });
      }));
    }
  }
  return 0;
}

int launch_product_expand(const obhip_terms &t, const double *d_xa, uint64_t na, const double *d_xb, uint64_t nb,
                          uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj, double *d_X) {
  const uint64_t rows = ni * nj;
  hipLaunchKernelGGL(k_product_expand, dim3((unsigned)((rows + 255) / 256), (unsigned)t.d), dim3(256), 0, cur_stream(),
                     t.product.dim_src.p, d_xa, na, d_xb, nb, i0, ni, j0, nj, d_X);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_product_scatter(const double *d_src, uint64_t q, uint64_t nb, uint64_t lda, uint64_t i0, uint64_t ni,
                           uint64_t j0, uint64_t nj, double *d_dst) {
  const uint64_t rows = ni * nj;
  for (uint64_t r0 = 0; r0 < q; r0 += 65535) {  // grid.y
    const uint64_t qc = std::min<uint64_t>(65535, q - r0);
    hipLaunchKernelGGL(k_product_scatter, dim3((unsigned)((rows + 255) / 256), (unsigned)qc), dim3(256), 0, cur_stream(),
                       d_src + r0 * rows, nb, lda, i0, ni, j0, nj, d_dst + r0 * nb * lda);
  }
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_product_lik_rows(const double *d_mean, const double *d_var, double e2sigma, const double *d_y,
                            const double *d_obsvar, uint64_t na, uint64_t nb, uint64_t i0, uint64_t ni, uint64_t j0,
                            uint64_t nj, double *d_part) {
  const uint64_t ctiles = (ni + kTileRows - 1) / kTileRows, tiles_a = (na + kTileRows - 1) / kTileRows;
  // the chunks of the row route hold at most 2^23 rows: ctiles x nj is far below the grid limit
  hipLaunchKernelGGL(k_product_lik_rows, dim3((unsigned)(ctiles * nj)), dim3(64), 0, cur_stream(), d_mean, d_var,
                     e2sigma, d_y, d_obsvar, nb, tiles_a, i0, ni, j0, ctiles, d_part);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_product_sum_tiles(const double *d_part, uint64_t tiles_a, uint64_t nb, double *d_out) {
  hipLaunchKernelGGL(k_product_sum_tiles, dim3((unsigned)((nb + 255) / 256), 2), dim3(256), 0, cur_stream(), d_part,
                     tiles_a, nb, d_out);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_check_nonneg(const double *d_v, uint64_t n, int *bad_out) {
  DevBuf<int> flag;
  OB_TRY(flag.alloc(1));
  OB_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), cur_stream()));
  hipLaunchKernelGGL(k_check_nonneg, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cur_stream(), d_v, n, flag.p);
  OB_HIP(hipGetLastError());
  return d2h(bad_out, flag.p, sizeof(int));
}

}  // namespace obhip
