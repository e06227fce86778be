// Hessian-vector and Jacobian-vector product of the multi-response predictor for gfx950: at new rows
// x, for one direction v per row (the rows of V) and q responses,
//   jvp_ij = sum_l v_l dmean_ij/dx_l            hvp_il = sum_j W_ij sum_m v_m d2mean_ij/dx_l dx_m
// and, from the same pass, the means and the VJP sum_j W_ij dmean_ij/dx_l.  One kernel evaluates the
// basis with its first and second derivative once per tile and forms every term product and every
// view product once; neither the Jacobian nor any n x d x q or n x d x d array reaches HBM.  No
// reference counterpart.  Formulas: include/obhip.h at obhip_predict_hvp_multi_dev.
//
// Per 32-row tile, 8 waves (32 rows: three column families at 64 rows do not fit the LDS at d = 20):
//   1. the two half-waves of a wave take different dimensions of the same 32 rows (half-wave h of
//      wave w: 2 w + h, + 16, ...; build_dim_d2_any) and write the tile: Mu value, Mu first- and Mu
//      second-derivative columns (column 0: ones, zeros, zeros), d columns each of rho_l, kappa_l and
//      v_l; pitch 33.  The row scale is the product of the 16 partial scales in their order, rho.v
//      the sum over the dimensions in their order.
//   2. wave = (row group of 16, quarter of the 4-entry steps); lane (m, k) forms the A operands of its
//      (row 16 rg + m, entry 4 step + k) through products of (value, directional derivative) pairs,
//        (E, dE) <- (E a, dE a + E v_dim(c) r'_c)      for every column c of the entry,
//      and reads the B operand Theta^T[term][16 j + m] from a term-major zero-padded copy of the chunk:
//        dense pass      A = P_k | dP_k                                     -> S, Sd
//        pass of dim. l  A = (rho.v) E r' + v_l E r'' + r' dE | E r'        -> X_l, g_l
//      over the view of l (obhip_terms::dx).  The quarters' accumulators meet in LDS and are added in
//      quarter order by the first quarter's waves, which apply, element-wise in the accumulator layout,
//        mean = s S      jvp = s ((rho.v) S + Sd)
//        Hv_l = s ((rho_l (rho.v) + v_l (kappa_l - rho_l^2)) S + rho_l Sd + X_l)     G_l = s (rho_l S + g_l)
//      into the finished blocks [16 NQB responses][33].
//   3. the means and the JVP leave as runs of 32 rows per response; wave l mod 8 (lane = row; the
//      lower half-wave Hv_l, the upper G_l) contracts the finished block with the tile's rows of W in
//      response order, one fma per response, starting from 0 in the first chunk of responses and
//      from what the chunk before left otherwise.
// No atomics, a fixed summation order: two runs give the same bits, and the bits of an output do not
// depend on which other outputs are asked for (the second operand of a pass is skipped, never
// reordered).
//
// HBM = true: the same code with the tile in a per-block slice of pooled HBM scratch and the column
// -> dimension map read from memory (any number of used columns and of factors): the fallback.
#include "obhip_internal.h"
#include "device_d2.h"

namespace obhip {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int kHvThreads = 512, kHvWaves = kHvThreads / 64;
constexpr int kHvPitch = kHvpRows + 1;    // doubles per tile column and per staged response
constexpr int kHvParts = 4;               // the quarters of the steps
constexpr int kHvSlots = 2 * kHvWaves;    // scale partials per row
constexpr uint64_t kHvChunk = 32;         // responses of one launch at most (48 accumulator registers per
                                          // block of 16: a third block would spill)

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// (E, dE) of the W2 column words at ent for the row trow; E starts at e0 (1, or 0 for a lane past the end)
__device__ __forceinline__ void pair_prod(const double *__restrict__ tile, const uint32_t *__restrict__ ent, int W2,
                                          int Mu, int vcol0, const int *__restrict__ ud, int trow, double e0,
                                          double &E, double &dE) {
  E = e0;
  dE = 0.0;
  for (int w = 0; w < W2; ++w) {
    const uint32_t cw = ent[w];
#pragma unroll
    for (int hw = 0; hw < 2; ++hw) {
      const int c = hw ? (int)(cw >> 16) : (int)(cw & 0xffffu);
      const double a = tile[c * kHvPitch + trow];
      const double b = tile[(Mu + c) * kHvPitch + trow] * tile[(vcol0 + max(ud[c], 0)) * kHvPitch + trow];
      dE = fma(dE, a, E * b);
      E *= a;
    }
  }
}

template <int NQB, bool HBM>
__global__ void __launch_bounds__(kHvThreads)
k_predict_hvp(const DimDesc *__restrict__ dims, const double *__restrict__ ka, const double *__restrict__ kb,
              const double *__restrict__ kc, const double *__restrict__ rot, const double *__restrict__ tab,
              const double *__restrict__ dtab, const int *__restrict__ cpos, int d, int Mu,
              const double *__restrict__ d2tab, const int *__restrict__ udim, const uint32_t *__restrict__ colsw,
              int W2, int p, const uint32_t *__restrict__ vw, const uint32_t *__restrict__ voff,
              const double *__restrict__ ThT /* [p][16 NQB] */, int qc, const double *__restrict__ x, uint64_t n,
              uint64_t ntiles, double *__restrict__ scratch, const double *__restrict__ Wc, uint64_t ldw,
              const double *__restrict__ V, int first, double *__restrict__ mean, double *__restrict__ vjp,
              double *__restrict__ jvp, double *__restrict__ hvp) {
  extern __shared__ double lds[];
  constexpr int QW = 16 * NQB;
  const int ncols = 3 * Mu + 3 * d;
  double *tile = HBM ? scratch + (size_t)blockIdx.x * ncols * kHvPitch : lds;       // [ncols][33]
  double *parts = HBM ? lds : lds + (size_t)ncols * kHvPitch;                        // [3][2][QW][33]
  double *fin = parts + (kHvParts - 1) * 2 * QW * kHvPitch;                          // [2][QW][33]
  double *reds = fin + 2 * QW * kHvPitch;                                            // [16][32] scale partials
  double *scl = reds + kHvSlots * kHvpRows;                                          // [32] row scale
  double *rvs = scl + kHvpRows;                                                      // [32] rho . v
  int *udl = (int *)(rvs + kHvpRows);                                                // [Mu] (HBM: unused)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = lane & 15, kq = lane >> 4;
  const int rg = wave & 1, part = wave >> 1;
  const int trow = 16 * rg + m;
  const int hl = lane & 31, hf = lane >> 5;
  const int vcol0 = 3 * Mu + 2 * d;
  const bool want_vjp = vjp != nullptr, want_hvp = hvp != nullptr;

  if (!HBM)
    for (int i = threadIdx.x; i < Mu; i += kHvThreads) udl[i] = max(udim[i], 0);
  const int *ud = HBM ? udim : udl;  // (the ones column's -1 is clamped again where it is read)

  for (uint64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const uint64_t row0 = tl * kHvpRows;
    // ---- 1. basis, first and second derivative, rho, kappa and v at the rows of the tile ----
    {
      const uint64_t row = row0 + hl;
      const bool valid = row < n;
      const StoreD2<kHvPitch> store{tile, cpos, hl, Mu, d};
      double sc = 1.0;
      for (int l = 2 * wave + hf; l < d; l += kHvSlots) {
        const DimDesc D = dims[l];
        const double xv = valid ? x[(uint64_t)l * n + row] : 0.5;
        double rho, kappa;
        sc *= build_dim_d2_any(D, ka, kb, kc, rot, tab, dtab, d2tab, xv, store, rho, kappa);
        store.rho(l, rho);
        store.kappa(l, kappa);
        store.dir(l, valid ? V[(uint64_t)l * n + row] : 0.0);
      }
      if (wave == 0 && hf == 0) {
        tile[hl] = 1.0;
        tile[Mu * kHvPitch + hl] = 0.0;
        tile[2 * Mu * kHvPitch + hl] = 0.0;
      }
      reds[(2 * wave + hf) * kHvpRows + hl] = sc;
    }
    __syncthreads();
    if (wave == 0 && lane < kHvpRows) {
      double s = 1.0;
#pragma unroll
      for (int q = 0; q < kHvSlots; ++q) s *= reds[q * kHvpRows + lane];
      scl[lane] = s;
    }
    if (wave == 1 && lane < kHvpRows) {
      double a = 0.0;
      for (int l = 0; l < d; ++l)
        a = fma(tile[(vcol0 + l) * kHvPitch + lane], tile[(3 * Mu + l) * kHvPitch + lane], a);
      rvs[lane] = a;
    }

    // ---- 2. / 3. the dense pass and the d passes of the dimensions ----
    d4 S[NQB], Sd[NQB];
    const int lend = want_vjp || want_hvp ? d : 0;
    for (int l = -1; l < lend; ++l) {
      d4 acc0[NQB], acc1[NQB];
#pragma unroll
      for (int j = 0; j < NQB; ++j) acc0[j] = acc1[j] = d4{0.0, 0.0, 0.0, 0.0};
      if (l < 0) {
        const int nsteps = (p + 3) / 4;
        for (int s = part; s < nsteps; s += kHvParts) {
          const int e = 4 * s + kq;
          const int k = min(e, p - 1);
          double P, dP;
          pair_prod(tile, colsw + (size_t)k * W2, W2, Mu, vcol0, ud, trow, e < p ? 1.0 : 0.0, P, dP);
          const double *th = ThT + (size_t)k * QW + m;
#pragma unroll
          for (int j = 0; j < NQB; ++j) {
            const double b = th[16 * j];
            acc0[j] = mfma(P, b, acc0[j]);
            acc1[j] = mfma(dP, b, acc1[j]);
          }
        }
      } else {
        // (rvs, written after the first barrier of the tile, is behind the barriers of the dense pass)
        const int v0 = (int)voff[l], cnt = (int)voff[l + 1] - v0;
        const int nsteps = (cnt + 3) / 4;
        const double rvr = rvs[trow], vl = tile[(vcol0 + l) * kHvPitch + trow];
        for (int s = part; s < nsteps; s += kHvParts) {
          const int e = 4 * s + kq;
          const uint32_t *ent = vw + (size_t)(v0 + min(e, cnt - 1)) * (W2 + 2);
          double E, dE;
          pair_prod(tile, ent, W2, Mu, vcol0, ud, trow, e < cnt ? 1.0 : 0.0, E, dE);
          const int own = (int)ent[W2];
          const double r1 = tile[(Mu + own) * kHvPitch + trow], r2 = tile[(2 * Mu + own) * kHvPitch + trow];
          const double Er1 = E * r1;
          const double A = fma(rvr, Er1, fma(vl, E * r2, r1 * dE));
          const double *th = ThT + (size_t)ent[W2 + 1] * QW + m;
#pragma unroll
          for (int j = 0; j < NQB; ++j) {
            const double b = th[16 * j];
            acc0[j] = mfma(A, b, acc0[j]);
            if (want_vjp) acc1[j] = mfma(Er1, b, acc1[j]);
          }
        }
      }
      __syncthreads();  // the blocks of the pass before have left (and scl, rvs are there)
      if (part > 0) {
        double *pp = parts + (size_t)(part - 1) * 2 * QW * kHvPitch;
#pragma unroll
        for (int j = 0; j < NQB; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = (16 * j + m) * kHvPitch + 16 * rg + kq + 4 * r;
            pp[o] = acc0[j][r];
            pp[QW * kHvPitch + o] = acc1[j][r];
          }
      }
      __syncthreads();
      if (part == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int orow = 16 * rg + kq + 4 * r;
          const double s = scl[orow], rvv = rvs[orow];
          double rho = 0.0, coef = 0.0;
          if (l >= 0) {
            rho = tile[(3 * Mu + l) * kHvPitch + orow];
            const double kap = tile[(3 * Mu + d + l) * kHvPitch + orow];
            const double vl = tile[(vcol0 + l) * kHvPitch + orow];
            coef = fma(rho, rvv, vl * (kap - rho * rho));
          }
#pragma unroll
          for (int j = 0; j < NQB; ++j) {
            const int o = (16 * j + m) * kHvPitch + orow;
            double t0 = acc0[j][r], t1 = acc1[j][r];
#pragma unroll
            for (int q = 0; q < kHvParts - 1; ++q) {
              t0 += parts[(size_t)q * 2 * QW * kHvPitch + o];
              t1 += parts[(size_t)(q * 2 + 1) * QW * kHvPitch + o];
            }
            if (l < 0) {
              S[j][r] = t0;
              Sd[j][r] = t1;
              fin[o] = t0 * s;
              fin[QW * kHvPitch + o] = s * fma(rvv, t0, t1);
            } else {
              fin[o] = s * fma(coef, S[j][r], fma(rho, Sd[j][r], t0));
              fin[QW * kHvPitch + o] = s * fma(rho, S[j][r], t1);
            }
          }
        }
      }
      __syncthreads();
      if (l < 0) {
        for (int e = threadIdx.x; e < 2 * QW * kHvpRows; e += kHvThreads) {
          const int which = e / (QW * kHvpRows), j = (e >> 5) & (QW - 1), r = e & 31;
          double *dst = which ? jvp : mean;
          if (dst && j < qc && row0 + r < n)
            dst[(uint64_t)j * n + row0 + r] = fin[(which * QW + j) * kHvPitch + r];
        }
      } else if (wave == (l & (kHvWaves - 1))) {
        const uint64_t row = row0 + hl;
        double *out = hf ? vjp : hvp;
        if (out && row < n) {
          const double *blk = fin + (size_t)hf * QW * kHvPitch + hl;
          double a = first ? 0.0 : out[(uint64_t)l * n + row];
          const double *wp = Wc + row;
          // the sum is serial in the responses; the weights of a block of 16 are requested together
          for (int j0 = 0; j0 < qc; j0 += 16) {
            double wv[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) wv[u] = j0 + u < qc ? wp[(uint64_t)(j0 + u) * ldw] : 0.0;
#pragma unroll
            for (int u = 0; u < 16; ++u)
              if (j0 + u < qc) a = fma(wv[u], blk[(j0 + u) * kHvPitch], a);
          }
          out[(uint64_t)l * n + row] = a;
        }
      }
    }
    __syncthreads();  // the tile and the blocks are free for the next tile
  }
}

template <int NQB, bool HBM>
int run_predict_hvp(const obhip_model &m, obhip_terms &t, const double *d_ThT, int qc, const double *d_x, uint64_t n,
                    const double *d_W, uint64_t ldw, const double *d_V, int first, double *d_mean, double *d_vjp,
                    double *d_jvp, double *d_hvp) {
  const size_t lds = predict_hvp_lds(t.Mu, m.d, NQB, HBM);
  OB_TRY(ensure_dyn_lds((const void *)k_predict_hvp<NQB, HBM>, lds));
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t ntiles = (n + kHvpRows - 1) / kHvpRows;
  uint64_t nblk = std::min<uint64_t>(ntiles, (uint64_t)device_cus(dev) * (HBM ? 2 : 4));
  DevBuf<double> scratch;
  if (HBM) {
    const uint64_t per = (3 * t.Mu + 3 * m.d) * kHvPitch;  // doubles of one block's tile; 1 GB in all at most
    nblk = std::max<uint64_t>(1, std::min<uint64_t>(nblk, (1ull << 27) / per));
    OB_TRY(scratch.alloc(nblk * per));
  }
  launch_pred<true>(k_predict_hvp<NQB, HBM>, dim3((unsigned)nblk), dim3(kHvThreads), lds, pred_tabs(m, t),
                    (const double *)t.dx.d2tab.p, (const int *)t.dx.udim.p, (const uint32_t *)t.cols.p,
                    (int)(t.W / 2), (int)t.p, (const uint32_t *)t.dx.vw.p, (const uint32_t *)t.dx.voff_dev.p, d_ThT,
                    qc, d_x, n, ntiles, scratch.p, d_W, ldw, d_V, first, d_mean, d_vjp, d_jvp, d_hvp);
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace

// bytes of LDS of one workgroup: the tile of 3 Mu + 3 d columns (hbm: in memory instead), the three
// quarters' two partial blocks and the two finished blocks of 16 nqb responses, the scale partials,
// the row scale, rho . v and the column -> dimension map
size_t predict_hvp_lds(uint64_t Mu, uint64_t d, int nqb, bool hbm) {
  const size_t blocks = (size_t)(2 * (kHvParts - 1) + 2) * 16 * nqb * kHvPitch;
  const size_t tile = hbm ? 0 : (3 * Mu + 3 * d) * kHvPitch;
  return (tile + blocks + (kHvSlots + 2) * kHvpRows) * sizeof(double) + (hbm ? 0 : (Mu + 1) / 2 * 2 * sizeof(int));
}

// the fused kernel's domain: the tile and the blocks of one group of 16 responses within the LDS
// (any number of factors: the column lists are read from memory)
bool predict_hvp_supports(const obhip_terms &t) {
  return t.W >= 2 && t.W % 2 == 0 && predict_hvp_lds(t.Mu, t.d, 1, false) <= kLdsBudget;
}

int launch_predict_hvp(const obhip_model &m, obhip_terms &t, const double *d_Theta, uint64_t q, const double *d_x,
                       uint64_t n, const double *d_W, uint64_t ldw, const double *d_V, double *d_mean, double *d_vjp,
                       double *d_jvp, double *d_hvp) {
  OB_TRY(ensure_dx_stage(m, t));
  OB_TRY(ensure_d2_tables(m, t));
  if (n == 0) return 0;
  ProfScope ps("predict_hvp_multi");
  const uint64_t p = t.p, d = m.d;
  const bool fused = predict_hvp_supports(t) && !getenv("OBHIP_FORCE_GENERIC");
  // (the fallback keeps to one block of 16: its tile addresses take the registers of the second)
  int nqb_max = fused ? 2 : 1;
  while (nqb_max > 1 && predict_hvp_lds(t.Mu, d, nqb_max, !fused) > kLdsBudget) nqb_max /= 2;
  const uint64_t chunk = std::min<uint64_t>(kHvChunk, 16 * (uint64_t)nqb_max);
  DevBuf<double> tht;
  OB_TRY(tht.alloc(p * chunk));
  for (uint64_t q0 = 0; q0 < q; q0 += chunk) {
    const int qc = (int)std::min<uint64_t>(chunk, q - q0);
    int nqb = 1;
    while (16 * nqb < qc) nqb *= 2;
    double *T = tht.p;
    OB_TRY(launch_theta_term_major(d_Theta + q0 * p, p, qc, 16 * (uint64_t)nqb, T));
    double *mc = d_mean ? d_mean + q0 * n : nullptr;
    double *jc = d_jvp ? d_jvp + q0 * n : nullptr;
    const double *wc = d_W ? d_W + q0 * ldw : nullptr;
    const int first = q0 == 0;
#define OB_HV(NQB_)                                                                                              \
  if (nqb == NQB_) {                                                                                             \
    if (fused)                                                                                                   \
      OB_TRY((run_predict_hvp<NQB_, false>(m, t, T, qc, d_x, n, wc, ldw, d_V, first, mc, d_vjp, jc, d_hvp)));    \
    else                                                                                                         \
      OB_TRY((run_predict_hvp<NQB_, true>(m, t, T, qc, d_x, n, wc, ldw, d_V, first, mc, d_vjp, jc, d_hvp)));     \
  }
    OB_HV(1)
    if (nqb == 2) OB_TRY((run_predict_hvp<2, false>(m, t, T, qc, d_x, n, wc, ldw, d_V, first, mc, d_vjp, jc, d_hvp)));
#undef OB_HV
  }
  return 0;
}

}  // namespace obhip
