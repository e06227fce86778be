// Gradient by xb of the predictor on the product of two input blocks, and of the calibration likelihood's sums
// (include/obhip.h, "gradient by xb on the product").  Notation of kernels_product.hip;
// l runs over the L dimensions of B, rho_jl = R'_l0 / R_l0, r'_{l,t} the derivative column of level t, E_jkl =
// V_jk without dimension l's factor:
//   m'_ijl = d mean_ij / d xb_jl = s (rho_jl S_ij + D_ijl),      D_ijl = sum_{k: t_kl > 0} theta_k U_ik E_jkl r'
//   v'_ijl = d var_ij / d xb_jl = 2 s^2 (rho_jl Q_ij + F_ijl),   F_ijl = sum_{k: t_kl > 0} c_k U_ik^2 V_jk E_jkl r'
// with S, Q the dense sums of k_predict_product and s = sA_i sB_j.
//
//   k_product_grad  tile, waves and accumulators of k_predict_product.  Phase 1: the A tile as there; the B tile
//                   by build_tile_side_dx: value columns, derivative columns, L columns of rho.  Phase 2a:
//                   pp_contract, the dense sums S and Q.  Phase 2b, for l = 0 .. L - 1: D and F over the VIEW of
//                   l (the terms that have l: obhip_terms::product_grad) in steps of four view-terms on the
//                   matrix cores, the view staged through LDS like the term chunk.  Store epilogue: m' and v'.
//                   Likelihood epilogue: with r = y - mean, v = var + obsvar the pair weights
//                     a1 = -2 s r / v,   a2 = -2 s^2 r^2 / v^2,   a3 = 2 s^2 / v       (0 for a row beyond na)
//                   give d chi2_j / d xb_jl = sum_i (a1 (rho S + D) + a2 (rho Q + F)) and d logdet_j / d xb_jl =
//                   sum_i a3 (rho Q + F).  rho_jl does not depend on i, so the dense parts sum_i (a1 S + a2 Q) and
//                   sum_i a3 Q are reduced once per tile and S, Q leave the registers before phase 2b; per l only
//                   a1 D + a2 F and a3 F are reduced, by the butterfly and group order of k_predict_product.
//   k_product_lik_grad_rows   the row route's reduction of the same sums, same order, same partials.
//   k_product_sum_tile_cols   k_product_sum_tiles for 2 + 2 L columns.
// No atomics, a fixed order everywhere: two calls give the same bits.  Every output index is 64-bit.
#include "obhip_internal.h"
#include "product_tile.h"

// workgroups per CU the register allocation aims at (DESIGN.md section 28 records the comparison)
#ifndef OBHIP_PG_MIN_BLOCKS
#define OBHIP_PG_MIN_BLOCKS 2
#endif

namespace obhip {

namespace {

// The likelihood epilogue with the variance holds three weights and two accumulators per pair through phase 2b:
// within the 256 registers of two workgroups per CU it spills 72 bytes per lane, so it is built for one
constexpr int pg_min_blocks(bool var, bool lik) { return var && lik ? 1 : OBHIP_PG_MIN_BLOCKS; }

struct PgArgs {
  PpArgs a;              // theta: the one response; qc, mean, var unused
  const double *dtab;    // derivative interval tables (obhip_terms::dx)
  const uint32_t *vw;    // view entries: wa2 A words, wb2 other-B words, own B column, term index
  const uint32_t *voff;  // L + 1
  double *dmean, *dvar;  // store epilogue
};

// pp_operands for view entry 4 s + kq of the staged chunk: u = U at the A rows, v = E r' and, DOV, w = V E r' at
// the B rows (the chunk's B words are the term's other B columns)
template <bool DOV>
__device__ __forceinline__ void pg_operands(const PpArgs &a, const double *__restrict__ ta,
                                            const double *__restrict__ tb, const PpChunk &ch,
                                            const uint32_t *__restrict__ own, int s, int kq, int ra, int rb,
                                            double (&u)[2], double (&v)[2], double (&w)[2], double &thk, double &cvk) {
  double e[2];
  pp_operands<DOV>(a, ta, tb, ch, s, kq, ra, rb, u, e, thk, cvk);
  const int o = (int)own[4 * s + kq];
  const double *dr = tb + (a.mu_b + o - 1) * kTileRows + rb;
  v[0] = e[0] * dr[0];
  v[1] = e[1] * dr[16];
  if constexpr (DOV) {
    const double *rv = tb + o * kTileRows + rb;
    w[0] = (e[0] * rv[0]) * v[0];
    w[1] = (e[1] * rv[16]) * v[1];
  }
}

// accd[b][a] += (E r')_b (theta U_a)^T and, DOV, accf[b][a] += (V E r')_b (c U_a^2)^T over the view of B
// dimension l, staged in chunks of kPpTerms entries (theta = c = 0 on the padding, whose columns are the ones
// column and the first derivative column).  Called by every thread of the workgroup (barriers).
template <bool DOV>
__device__ __forceinline__ void pg_view_contract(const PgArgs &g, const double *__restrict__ ta,
                                                 const double *__restrict__ tb, const PpChunk &ch,
                                                 uint32_t *__restrict__ own, int l, int kq, int ra, int rb,
                                                 d4 (&accd)[2][2], d4 (&accf)[2][2]) {
  const PpArgs &a = g.a;
  const uint32_t v0 = g.voff[l];
  const int vcnt = (int)(g.voff[l + 1] - v0);
  const int stride = a.wa2 + a.wb2 + 2;
  for (int k0 = 0; k0 < vcnt; k0 += kPpTerms) {
    const int kc = min(kPpTerms, vcnt - k0);
    __syncthreads();  // the previous chunk is spent
    for (int e = threadIdx.x; e < kPpTerms; e += kPpThreads) {
      const bool in = e < kc;
      const uint32_t *ent = g.vw + ((size_t)v0 + k0 + (in ? e : 0)) * stride;
      for (int w = 0; w < a.wa2; ++w) ch.cw_a[e * a.wa2 + w] = in ? ent[w] : 0u;
      for (int w = 0; w < a.wb2; ++w) ch.cw_b[e * a.wb2 + w] = in ? ent[a.wa2 + w] : 0u;
      own[e] = in ? ent[a.wa2 + a.wb2] : 1u;
      const uint32_t k = ent[a.wa2 + a.wb2 + 1];
      ch.th[e] = in ? a.theta[k] : 0.0;
      if (DOV) ch.cv[e] = in ? a.coeffvar[k] : 0.0;
    }
    __syncthreads();
    const int nsteps = (kc + 3) / 4;
    double u[2], v[2], w[2], thk, cvk;
    pg_operands<DOV>(a, ta, tb, ch, own, 0, kq, ra, rb, u, v, w, thk, cvk);
    for (int s = 0; s < nsteps; ++s) {
      const double tu0 = thk * u[0], tu1 = thk * u[1];
      accd[0][0] = mfma(v[0], tu0, accd[0][0]);
      accd[0][1] = mfma(v[0], tu1, accd[0][1]);
      accd[1][0] = mfma(v[1], tu0, accd[1][0]);
      accd[1][1] = mfma(v[1], tu1, accd[1][1]);
      if constexpr (DOV) {
        const double cu0 = cvk * (u[0] * u[0]), cu1 = cvk * (u[1] * u[1]);
        accf[0][0] = mfma(w[0], cu0, accf[0][0]);
        accf[0][1] = mfma(w[0], cu1, accf[0][1]);
        accf[1][0] = mfma(w[1], cu0, accf[1][0]);
        accf[1][1] = mfma(w[1], cu1, accf[1][1]);
      }
      if (s + 1 < nsteps) pg_operands<DOV>(a, ta, tb, ch, own, s + 1, kq, ra, rb, u, v, w, thk, cvk);
    }
  }
}

__device__ __forceinline__ void zero(d4 (&x)[2][2]) {
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int c = 0; c < 2; ++c) x[b][c] = d4{0.0, 0.0, 0.0, 0.0};
}

template <bool VAR, bool LIK>
__global__ void __launch_bounds__(kPpThreads, pg_min_blocks(VAR, LIK))
k_product_grad(const PgArgs g) {
  const PpArgs &a = g.a;
  extern __shared__ double lds[];
  const int L = a.ndb, ncols_b = 2 * a.mu_b - 1 + L;
  double *ta = lds;                              // [mu_a][64]
  double *tb = ta + (size_t)a.mu_a * kTileRows;  // [mu_b values | mu_b - 1 derivatives | L rho][64]
  double *pa = tb + (size_t)ncols_b * kTileRows; // [4][64] scale shares of the A dimensions
  double *pb = pa + kPpWaves * kTileRows;        // [4][64] of the B dimensions
  double *sa = pb + kPpWaves * kTileRows;        // [64] sA of the tile's A rows
  double *sb = sa + kTileRows;                   // [64] sB of its B rows
  double *red = sb + kTileRows;                  // [2][4][64] likelihood partials per 16-row group of A
  double *gd = red + 2 * 4 * kTileRows;          // [2][64] the dense parts of the two gradient sums
  PpChunk ch;
  ch.th = gd + 2 * kTileRows;
  ch.cv = ch.th + kPpTerms;
  ch.cw_a = (uint32_t *)(ch.cv + kPpTerms);
  ch.cw_b = ch.cw_a + kPpTerms * a.wa2;
  uint32_t *own = ch.cw_b + kPpTerms * a.wb2;    // [kPpTerms] own B column of the staged view entries
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t at = a.atile0 + (uint64_t)blockIdx.x / a.tiles_b, bt = (uint64_t)blockIdx.x % a.tiles_b;
  const uint64_t i0 = at * kTileRows, j0 = bt * kTileRows;
  {
    const StoreTile<kTileRows> st_a{ta, a.cpos_a, lane, a.mu_a};
    build_tile_side<kPpWaves>(a.dims, a.ka, a.kb, a.kc, a.rot, a.tab, a.side_a, a.nda, a.xa, a.na, i0 + lane,
                              i0 + lane < a.na, wave, wave, st_a, pa);
    const int slot_b = (wave + kPpWaves - a.nda % kPpWaves) % kPpWaves;
    const StoreTile<kTileRows> st_b{tb, a.cpos_b, lane, a.mu_b};
    build_tile_side_dx<kPpWaves>(a.dims, a.ka, a.kb, a.kc, a.rot, a.tab, g.dtab, a.side_b, a.ndb, a.xb, a.nb,
                                 j0 + lane, j0 + lane < a.nb, wave, slot_b, st_b, pb);
  }
  __syncthreads();
  if (wave == 0) sa[lane] = tile_scale<kPpWaves>(pa, lane);
  if (wave == 1) sb[lane] = tile_scale<kPpWaves>(pb, lane);
  __syncthreads();

  const int m = lane & 15, kq = lane >> 4;
  const int ig = wave & 1, jg = wave >> 1;
  const int ra = 32 * ig + m, rb = 32 * jg + m;
  const double *rho = tb + (size_t)(2 * a.mu_b - 1) * kTileRows;  // [L][64]
  d4 acc[2][2], accv[2][2];
  zero(acc);
  zero(accv);
  pp_contract<VAR>(a, ta, tb, a.theta, ch, kq, ra, rb, acc, accv);

  if constexpr (!LIK) {
    for (int l = 0; l < L; ++l) {
      d4 ad[2][2], af[2][2];
      zero(ad);
      zero(af);
      pg_view_contract<VAR>(g, ta, tb, ch, own, l, kq, ra, rb, ad, af);
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int jl = 32 * jg + 16 * b + kq + 4 * rr;
          const uint64_t j = j0 + jl;
          const double rh = rho[l * kTileRows + jl];
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int il = 32 * ig + 16 * c + m;
            const uint64_t i = i0 + il;
            if (i < a.na && j < a.nb) {
              const double s = sa[il] * sb[jl];
              const uint64_t at_out = ((uint64_t)l * a.nb + j) * a.lda + i;
              g.dmean[at_out] = s * fma(rh, acc[b][c][rr], ad[b][c][rr]);
              if (VAR) g.dvar[at_out] = 2.0 * (s * s) * fma(rh, accv[b][c][rr], af[b][c][rr]);
            }
          }
        }
    }
  } else {
    // the four 16-row groups of `red` in ascending order: threads 0..127 = (which of the two sums, B row)
    auto group_sum = [&](int w, int jl) {
      const double *rw = red + (size_t)w * 4 * kTileRows + jl;
      return ((rw[0] + rw[kTileRows]) + rw[2 * kTileRows]) + rw[3 * kTileRows];
    };
    double yv[2], ov[2];
    bool ok[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const uint64_t i = i0 + 32 * ig + 16 * c + m;
      ok[c] = i < a.na;  // the rows beyond na leave the sums, not only the output
      yv[c] = ok[c] ? a.y[i] : 0.0;
      ov[c] = (ok[c] && a.obsvar) ? a.obsvar[i] : 0.0;
    }
    // the sums of obhip_product_loglik_dev, formed as k_predict_product forms them
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
      const double sum = group_sum(w, jl);
      if (j0 + jl < a.nb) a.part[((uint64_t)w * a.tiles_a + at) * a.nb + j0 + jl] = sum;
    }
    __syncthreads();
    // the pair weights, and the dense parts sum_i (a1 S + a2 Q), sum_i a3 Q of the two gradient sums
    d4 a1[2][2], a2[2][2], a3[2][2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int jl = 32 * jg + 16 * b + kq + 4 * rr;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int il = 32 * ig + 16 * c + m;
          const double s = sa[il] * sb[jl], s2 = 2.0 * (s * s);
          const double var = VAR ? accv[b][c][rr] * (s * s) + a.e2sigma : a.e2sigma;
          const double r = yv[c] - acc[b][c][rr] * s, v = var + ov[c];
          const double iv = 1.0 / v, q = r * iv;
          a1[b][c][rr] = ok[c] ? -2.0 * (s * q) : 0.0;
          a2[b][c][rr] = (VAR && ok[c]) ? -(s2 * (q * q)) : 0.0;
          a3[b][c][rr] = (VAR && ok[c]) ? s2 * iv : 0.0;
          // S and Q end here: their registers take the pair's share of the dense parts
          double x1 = a1[b][c][rr] * acc[b][c][rr], x2 = 0.0;
          if (VAR) {
            x1 += a2[b][c][rr] * accv[b][c][rr];
            x2 = a3[b][c][rr] * accv[b][c][rr];
          }
          acc[b][c][rr] = x1;
          accv[b][c][rr] = x2;
        }
      }
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int jl = 32 * jg + 16 * b + kq + 4 * rr;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const double x1 = sum16(acc[b][c][rr]), x2 = sum16(accv[b][c][rr]);
          if (m == 0) {
            red[(0 * 4 + 2 * ig + c) * kTileRows + jl] = x1;
            red[(1 * 4 + 2 * ig + c) * kTileRows + jl] = x2;
          }
        }
      }
    __syncthreads();
    if (threadIdx.x < 2 * kTileRows) gd[threadIdx.x] = group_sum(threadIdx.x >> 6, threadIdx.x & 63);
    // (the barriers of the loop below order gd and red)
    for (int l = 0; l < L; ++l) {
      d4 ad[2][2], af[2][2];
      zero(ad);
      zero(af);
      pg_view_contract<VAR>(g, ta, tb, ch, own, l, kq, ra, rb, ad, af);
      __syncthreads();  // red is free (an empty view has no barrier of its own)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int jl = 32 * jg + 16 * b + kq + 4 * rr;
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            double x1 = a1[b][c][rr] * ad[b][c][rr], x2 = 0.0;
            if (VAR) {
              x1 += a2[b][c][rr] * af[b][c][rr];
              x2 = a3[b][c][rr] * af[b][c][rr];
            }
            x1 = sum16(x1);
            x2 = sum16(x2);
            if (m == 0) {
              red[(0 * 4 + 2 * ig + c) * kTileRows + jl] = x1;
              red[(1 * 4 + 2 * ig + c) * kTileRows + jl] = x2;
            }
          }
        }
      __syncthreads();
      if (threadIdx.x < 2 * kTileRows) {
        const int w = threadIdx.x >> 6, jl = threadIdx.x & 63;
        const double sum = fma(rho[l * kTileRows + jl], gd[w * kTileRows + jl], group_sum(w, jl));
        if (j0 + jl < a.nb)
          a.part[((uint64_t)(2 + w * L + l) * a.tiles_a + at) * a.nb + j0 + jl] = sum;
      }
    }
  }
}

// one wave per (A tile of the chunk, B row), lane = row of the tile, as k_product_lik_rows: per B dimension
// the gradients of the two sums from the row predictor's gradients of the mean and the variance (the sums
// themselves are k_product_lik_rows's, so that they carry the bits of the row route's obhip_product_loglik_dev)
__global__ void __launch_bounds__(64)
k_product_lik_grad_rows(const double *__restrict__ mean, const double *__restrict__ var, double e2sigma,
                        const double *__restrict__ grad, const double *__restrict__ gradvar,
                        const int *__restrict__ side_b, int L, const double *__restrict__ y,
                        const double *__restrict__ obsvar, uint64_t nb, uint64_t tiles_a, uint64_t i0, uint64_t ni,
                        uint64_t j0, uint64_t rows, uint64_t ctiles, double *__restrict__ part) {
  const int lane = threadIdx.x;
  const uint64_t ct = (uint64_t)blockIdx.x % ctiles, jj = (uint64_t)blockIdx.x / ctiles;
  const uint64_t ii = ct * kTileRows + lane;
  const bool ok = ii < ni;
  const uint64_t e = jj * ni + (ok ? ii : 0);
  const double yv = ok ? y[i0 + ii] : 0.0, mv = mean[e], vv = var ? var[e] : e2sigma;
  const double ov = (ok && obsvar) ? obsvar[i0 + ii] : 0.0;
  auto wave_sum = [&](double t) {
    t = sum16(t);
    return ((__shfl(t, 0, 64) + __shfl(t, 16, 64)) + __shfl(t, 32, 64)) + __shfl(t, 48, 64);
  };
  const uint64_t at = i0 / kTileRows + ct, j = j0 + jj;
  const double r = yv - mv, v = vv + ov;
  const double iv = 1.0 / v, q = r * iv;
  for (int lb = 0; lb < L; ++lb) {
    const uint64_t ge = (uint64_t)side_b[lb] * rows + e;
    const double gm = grad[ge], gv = gradvar ? gradvar[ge] : 0.0;
    const double x1 = wave_sum(ok ? -2.0 * q * gm - (q * q) * gv : 0.0);
    const double x2 = wave_sum(ok ? iv * gv : 0.0);
    if (lane == 0) {
      part[((uint64_t)(2 + lb) * tiles_a + at) * nb + j] = x1;
      part[((uint64_t)(2 + L + lb) * tiles_a + at) * nb + j] = x2;
    }
  }
}

__global__ void __launch_bounds__(256)
k_product_sum_tile_cols(const double *__restrict__ part, uint64_t tiles_a, uint64_t nb, double *__restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nb) return;
  const uint64_t w = blockIdx.y;
  double s = 0.0;
  for (uint64_t at = 0; at < tiles_a; ++at) s += part[(w * tiles_a + at) * nb + j];
  out[w * nb + j] = s;
}

// grid.x of the chunked one-dimensional launches
constexpr uint64_t kMaxGridX = 0x7fffffffull;

}  // namespace

size_t product_grad_lds(uint64_t mu_a, uint64_t mu_b, uint64_t nb_dims, uint64_t wa, uint64_t wb) {
  return ((mu_a + 2 * mu_b - 1 + nb_dims) * kTileRows + kPpStage + 2 * kTileRows + 2 * kPpTerms) * sizeof(double) +
         kPpTerms * (wa / 2 + wb / 2 + 1) * sizeof(uint32_t);
}

bool product_grad_supports(uint64_t mu_a, uint64_t mu_b, uint64_t nb_dims, uint64_t wa, uint64_t wb) {
  return wa >= 2 && wb >= 2 && wa % 2 == 0 && wb % 2 == 0 &&
         product_grad_lds(mu_a, mu_b, nb_dims, wa, wb) <= kLdsBudget;
}

int launch_product_grad(const obhip_model &m, obhip_terms &t, const ProductGradCall &c) {
  ProfScope ps("product_grad");
  const obhip_terms::Product &pr = t.product;
  const ModelDev &md = t.pred_md;
  const bool lik = c.dmean == nullptr;
  const bool var = c.coeffvar != nullptr && (lik || c.dvar != nullptr);
  PgArgs g{};
  PpArgs &a = g.a;
  a.dims = md.dims.p, a.ka = md.ka.p, a.kb = md.kb.p, a.kc = md.kc.p, a.rot = md.rot.p, a.tab = md.tab.p;
  a.side_a = pr.side_a.p, a.side_b = pr.side_b.p;
  a.nda = (int)(m.d - pr.dims_b.size()), a.ndb = (int)pr.dims_b.size();
  a.cpos_a = pr.cpos_a.p, a.cpos_b = pr.cpos_b.p;
  a.mu_a = (int)pr.mu_a, a.mu_b = (int)pr.mu_b;
  a.cw_a = (const uint32_t *)pr.cols_a.p, a.cw_b = (const uint32_t *)pr.cols_b.p;
  a.wa2 = (int)(pr.wa / 2), a.wb2 = (int)(pr.wb / 2), a.p = (int)t.p;
  a.theta = c.theta, a.qc = 1;
  a.coeffvar = var ? c.coeffvar : nullptr, a.e2sigma = std::exp(2.0 * c.sigma);
  a.xa = c.xa, a.xb = c.xb, a.na = c.na, a.nb = c.nb;
  a.tiles_a = (c.na + kTileRows - 1) / kTileRows, a.tiles_b = (c.nb + kTileRows - 1) / kTileRows;
  a.lda = c.lda, a.y = c.y, a.obsvar = c.obsvar, a.part = c.part;
  g.dtab = t.dx.dtab.p, g.vw = t.product_grad.vw.p, g.voff = t.product_grad.voff.p;
  g.dmean = c.dmean, g.dvar = c.dvar;
  if (a.tiles_b > kMaxGridX) return fail(OBHIP_ERR_INVALID, "product_grad: more than 2^37 rows in xb");
  const size_t lds = product_grad_lds(pr.mu_a, pr.mu_b, pr.dims_b.size(), pr.wa, pr.wb);
  // a launch takes as many A tiles as keep tiles_a x tiles_b within the grid's first dimension
  const uint64_t at_per = std::max<uint64_t>(1, kMaxGridX / a.tiles_b);
  for (uint64_t at0 = 0; at0 < a.tiles_a; at0 += at_per) {
    a.atile0 = at0;
    const dim3 grid((unsigned)(std::min(at_per, a.tiles_a - at0) * a.tiles_b));
    OB_TRY(pick_bool(var, [&](auto VAR) {
      return pick_bool(lik, [&](auto LIK) {
        constexpr auto kernel = k_product_grad<VAR(), LIK()>;
        OB_TRY(ensure_dyn_lds((const void *)kernel, lds));
        hipLaunchKernelGGL(kernel, grid, dim3(kPpThreads), lds, cur_stream(), g);
        OB_HIP(hipGetLastError());
        return 0;
      });
    }));
  }
  return 0;
}

int launch_product_lik_grad_rows(const obhip_terms &t, const double *d_mean, const double *d_var, double e2sigma,
                                 const double *d_grad, const double *d_gradvar, const double *d_y,
                                 const double *d_obsvar, uint64_t na, uint64_t nb, uint64_t i0, uint64_t ni,
                                 uint64_t j0, uint64_t nj, double *d_part) {
  const uint64_t ctiles = (ni + kTileRows - 1) / kTileRows, tiles_a = (na + kTileRows - 1) / kTileRows;
  // the chunks of the row route hold at most 2^23 rows: ctiles x nj is far below the grid limit
  hipLaunchKernelGGL(k_product_lik_grad_rows, dim3((unsigned)(ctiles * nj)), dim3(64), 0, cur_stream(), d_mean, d_var,
                     e2sigma, d_grad, d_gradvar, t.product.side_b.p, (int)t.product.dims_b.size(), d_y, d_obsvar, nb,
                     tiles_a, i0, ni, j0, ni * nj, ctiles, d_part);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_product_sum_tile_cols(const double *d_part, uint64_t tiles_a, uint64_t nb, uint64_t ncols, double *d_out) {
  hipLaunchKernelGGL(k_product_sum_tile_cols, dim3((unsigned)((nb + 255) / 256), (unsigned)ncols), dim3(256), 0,
                     cur_stream(), d_part, tiles_a, nb, d_out);
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace obhip
