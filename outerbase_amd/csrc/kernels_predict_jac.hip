// Jacobian and vector-Jacobian product of the multi-response predictor for gfx950: at new rows x
// the means of q responses, d mean_ij / d x_l for all of them, or sum_j W_ij d mean_ij / d x_l, from
// one kernel that evaluates the basis and its derivative once and forms every term product P_k and
// every view product E_kl r'_l,t once -- they do not depend on the response; only Theta does.  No
// reference counterpart.  Formulas: include/obhip.h at obhip_predict_jac_multi_dev.
//
// The union of k_predict_dx (tile, phase 1, the per-dimension views) and k_predict_multi (the
// contraction on the matrix cores).  Per 64-row tile, 8 waves:
//   1. lane = row: the waves evaluate the dimensions (wave w takes w, w + 8, ...; build_dim_dx_any)
//      into the tile: Mu value columns (column 0 = ones), Mu - 1 derivative columns, d columns of
//      rho_l; pitch 65, so that the four columns of an MFMA step do not start on the same bank.
//      The row scale is the product of the waves' partial scales in wave order.
//   2. d + 1 passes.  wave = (row group of 16, half of the 4-entry steps); lane (m, k) forms the A
//      operand of its (row 16 rg + m, entry 4 step + k) and reads the B operand Theta^T[term][16 j + m]
//      from a term-major zero-padded copy of the chunk of at most 16 NQB responses:
//        dense pass      A = P_k                  over all p terms          -> S[row, j]
//        pass of dim. l  A = E_kl r'_l,t_kl       over the view of l        -> g_l[row, j]
//      (obhip_terms::dx; the view entry names the term, hence the row of Theta^T).  The second half's
//      accumulators go through the staging block, the first half adds its own (first + second, a
//      fixed order) and applies, element-wise in the accumulator layout S and g_l share,
//        mean = s S        jac_l = s (rho_l S + g_l)
//      into the staging block [16 NQB responses][64 rows + 1].
//   3. per pass the staged block leaves as 512-byte runs per (response, dimension, tile): the means
//      after the dense pass, jac[(j d + l) n + i] after the pass of l.
//      VJP = true: nothing of the Jacobian is written.  Wave l mod 8 (lane = row) contracts the
//      staged block with the tile's rows of W in response order, one fma per response, starting from
//      0 in the first chunk of responses and from what the chunk before left in out otherwise, and
//      writes out[l n + i]: the sum runs over all q responses in response order.
// No atomics, a fixed summation order: two runs give the same bits, and the bits of mean and jac do
// not depend on which outputs are asked for.
//
// Outside the fused domain (predict_jac_supports), under OBHIP_FORCE_GENERIC and for q = 1: one
// launch_predict_dx per response, the VJP accumulated by k_vjp_accum from an n x d pooled scratch.
#include "obhip_internal.h"
#include "device_dx.h"

namespace obhip {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int kPjThreads = 512, kPjWaves = kPjThreads / 64;
constexpr int kPjPitch = kTileRows + 1;   // doubles per tile column and per staged response
constexpr uint64_t kPjChunk = 64;         // responses of one launch at most

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// the steps of one pass that this wave's half takes, accumulated into acc (zeroed here).
// DENSE: entry = term, W2 column words at colsw.  Otherwise entry = view entry of W2 + 2 words (the
// other columns, the own column, the term) starting at ent0.
template <int NQB, bool DENSE>
__device__ __forceinline__ void jac_pass(d4 (&acc)[NQB], const double *__restrict__ tile,
                                         const uint32_t *__restrict__ ent0, int cnt, int W2, int Mu,
                                         const double *__restrict__ ThT, int trow, int m, int kq, int half) {
  constexpr int QW = 16 * NQB;
  const int stride = DENSE ? W2 : W2 + 2;
#pragma unroll
  for (int j = 0; j < NQB; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
  const int nsteps = (cnt + 3) / 4;
  for (int s = half; s < nsteps; s += 2) {
    const int e = 4 * s + kq;
    const bool ok = e < cnt;
    const uint32_t *ent = ent0 + (size_t)min(e, cnt - 1) * stride;
    double pr = ok ? 1.0 : 0.0;
    for (int w = 0; w < W2; ++w) {
      const uint32_t c = ent[w];
      pr *= tile[(c & 0xffffu) * kPjPitch + trow];
      pr *= tile[(c >> 16) * kPjPitch + trow];
    }
    uint32_t k;
    if (DENSE) {
      k = (uint32_t)min(e, cnt - 1);
    } else {
      pr *= tile[(Mu + (int)ent[W2] - 1) * kPjPitch + trow];
      k = ent[W2 + 1];
    }
    const double *th = ThT + (size_t)k * QW + m;
#pragma unroll
    for (int j = 0; j < NQB; ++j) acc[j] = mfma(pr, th[16 * j], acc[j]);
  }
}

template <int NQB, bool VJP>
__global__ void __launch_bounds__(kPjThreads)
k_predict_jac(const DimDesc *__restrict__ dims, const double *__restrict__ ka, const double *__restrict__ kb,
              const double *__restrict__ kc, const double *__restrict__ rot, const double *__restrict__ tab,
              const double *__restrict__ dtab, const int *__restrict__ cpos, int d, int Mu,
              const uint32_t *__restrict__ colsw, int W2, int p, const uint32_t *__restrict__ vw,
              const uint32_t *__restrict__ voff, const double *__restrict__ ThT /* [p][16 NQB] */, int qc,
              const double *__restrict__ x, uint64_t n, uint64_t ntiles, double *__restrict__ mean,
              double *__restrict__ jac /* of the chunk's first response */, const double *__restrict__ Wc,
              uint64_t ldw, int first, double *__restrict__ out) {
  extern __shared__ double lds[];
  constexpr int QW = 16 * NQB;
  const int ncols = 2 * Mu - 1 + d;
  double *tile = lds;                                  // [ncols][65]
  double *stage = tile + (size_t)ncols * kPjPitch;     // [QW][65]
  double *reds = stage + QW * kPjPitch;                // [8][64] scale partials
  double *scl = reds + kPjWaves * kTileRows;           // [64] row scale
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = lane & 15, kq = lane >> 4;
  const int rg = wave & 3, half = wave >> 2;
  const int trow = 16 * rg + m;

  for (uint64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const uint64_t row0 = tl * kTileRows;
    // ---- 1. basis, derivative basis and rho at the rows of the tile (as k_predict_dx) ----
    {
      const uint64_t row = row0 + lane;
      const bool valid = row < n;
      const StoreTile<kPjPitch> store{tile, cpos, lane, Mu};
      build_tile<kPjWaves, true>(dims, ka, kb, kc, rot, tab, dtab, d, x, n, row, valid, wave, store, reds);
    }
    __syncthreads();
    if (wave == 0) scl[lane] = tile_scale<kPjWaves>(reds, lane);

    // ---- 2. / 3. the d + 1 passes ----
    d4 S[NQB];
    for (int l = -1; l < d; ++l) {
      d4 acc[NQB];
      if (l < 0) {
        jac_pass<NQB, true>(acc, tile, colsw, p, W2, Mu, ThT, trow, m, kq, half);
      } else {
        const int v0 = (int)voff[l], vcnt = (int)voff[l + 1] - v0;
        jac_pass<NQB, false>(acc, tile, vw + (size_t)v0 * (W2 + 2), vcnt, W2, Mu, ThT, trow, m, kq, half);
      }
      __syncthreads();  // the staged block of the pass before has left (and scl is there)
      if (half == 1) {
#pragma unroll
        for (int j = 0; j < NQB; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) stage[(16 * j + m) * kPjPitch + 16 * rg + kq + 4 * r] = acc[j][r];
      }
      __syncthreads();
      if (half == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int orow = 16 * rg + kq + 4 * r;
          const double s = scl[orow];
          const double rho = l < 0 ? 0.0 : tile[(2 * Mu - 1 + l) * kPjPitch + orow];
#pragma unroll
          for (int j = 0; j < NQB; ++j) {
            double *sp = stage + (16 * j + m) * kPjPitch + orow;
            const double tot = acc[j][r] + *sp;
            if (l < 0) {
              S[j][r] = tot;
              *sp = tot * s;
            } else {
              *sp = s * fma(rho, S[j][r], tot);
            }
          }
        }
      }
      __syncthreads();
      if (l < 0) {
        if (mean) {
          for (int e = threadIdx.x; e < QW * kTileRows; e += kPjThreads) {
            const int j = e >> 6, r = e & 63;
            if (j < qc && row0 + r < n) mean[(uint64_t)j * n + row0 + r] = stage[j * kPjPitch + r];
          }
        }
      } else if (!VJP) {
        for (int e = threadIdx.x; e < QW * kTileRows; e += kPjThreads) {
          const int j = e >> 6, r = e & 63;
          if (j < qc && row0 + r < n) jac[((uint64_t)j * d + l) * n + row0 + r] = stage[j * kPjPitch + r];
        }
      } else if (wave == (l & (kPjWaves - 1))) {
        const uint64_t row = row0 + lane;
        if (row < n) {
          double a = first ? 0.0 : out[(uint64_t)l * n + row];
          const double *wp = Wc + row;
          // the sum is serial in the responses; the weights of a block of 16 are requested together
          for (int j0 = 0; j0 < qc; j0 += 16) {
            double wv[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) wv[u] = j0 + u < qc ? wp[(uint64_t)(j0 + u) * ldw] : 0.0;
#pragma unroll
            for (int u = 0; u < 16; ++u)
              if (j0 + u < qc) a = fma(wv[u], stage[(j0 + u) * kPjPitch + lane], a);
          }
          out[(uint64_t)l * n + row] = a;
        }
      }
    }
    __syncthreads();  // the tile and the staged block are free for the next tile
  }
}

size_t predict_jac_lds(uint64_t Mu, uint64_t d, int nqb) {
  return ((2 * Mu - 1 + d) * kPjPitch + (size_t)16 * nqb * kPjPitch + kPjWaves * kTileRows + kTileRows) *
         sizeof(double);
}

template <int NQB, bool VJP>
int run_predict_jac(const obhip_model &m, obhip_terms &t, const double *d_ThT, int qc, const double *d_x, uint64_t n,
                    double *d_mean, double *d_jac, const double *d_W, uint64_t ldw, int first, double *d_out) {
  const size_t lds = predict_jac_lds(t.Mu, m.d, NQB);
  OB_TRY(ensure_dyn_lds((const void *)k_predict_jac<NQB, VJP>, lds));
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t ntiles = (n + kTileRows - 1) / kTileRows;
  const uint64_t nblk = std::min<uint64_t>(ntiles, (uint64_t)device_cus(dev) * 8);
  launch_pred<true>(k_predict_jac<NQB, VJP>, dim3((unsigned)nblk), dim3(kPjThreads), lds, pred_tabs(m, t),
                    (const uint32_t *)t.cols.p, (int)(t.W / 2), (int)t.p, t.dx.vw.p, t.dx.voff_dev.p, d_ThT, qc, d_x,
                    n, ntiles, d_mean, d_jac, d_W, ldw, first, d_out);
  OB_HIP(hipGetLastError());
  return 0;
}

// out (n x d) = (first ? 0 : out) + w (n) o g (n x d), one fma per entry
__global__ void __launch_bounds__(256)
k_vjp_accum(const double *__restrict__ w, const double *__restrict__ g, uint64_t n, uint64_t nd, int first,
            double *__restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nd) return;
  out[i] = fma(w[i % n], g[i], first ? 0.0 : out[i]);
}

}  // namespace

// the fused kernel's domain: an even padded width (any number of factors: the column lists are read
// from memory) and the tile, one staged block of 16 responses and the scale space within the LDS
bool predict_jac_supports(const obhip_terms &t) {
  return t.W >= 2 && t.W % 2 == 0 && predict_jac_lds(t.Mu, t.d, 1) <= kLdsBudget;
}

// d_W == nullptr: the Jacobian into d_jac ((q, d, n)); otherwise the VJP with d_W into d_out (n x d).
// d_mean (n x q) may be nullptr.  q = 1, term sets outside the fused domain and OBHIP_FORCE_GENERIC
// take launch_predict_dx once per response.
int launch_predict_jac(const obhip_model &m, obhip_terms &t, const double *d_Theta, uint64_t q, const double *d_x,
                       uint64_t n, double *d_mean, double *d_jac, const double *d_W, uint64_t ldw, double *d_out) {
  OB_TRY(prepare_predict(m, t, true));
  if (n == 0) return 0;
  const uint64_t p = t.p, d = m.d;
  const bool vjp = d_W != nullptr;
  if (q == 1 || !predict_jac_supports(t) || getenv("OBHIP_FORCE_GENERIC")) {
    DevBuf<double> g;
    if (vjp) OB_TRY(g.alloc(n * d));
    for (uint64_t j = 0; j < q; ++j) {
      double *gj = vjp ? g.p : d_jac + j * d * n;
      OB_TRY(launch_predict_dx(m, t, d_Theta + j * p, d_x, n, d_mean ? d_mean + j * n : nullptr, gj, nullptr, 1.0,
                               nullptr, nullptr));
      if (vjp) {
        hipLaunchKernelGGL(k_vjp_accum, dim3((unsigned)((n * d + 255) / 256)), dim3(256), 0, cur_stream(),
                           d_W + j * ldw, (const double *)g.p, n, n * d, j == 0 ? 1 : 0, d_out);
        OB_HIP(hipGetLastError());
      }
    }
    return 0;
  }
  ProfScope ps(vjp ? "predict_vjp_multi" : "predict_jac_multi");
  int nqb_max = 4;
  while (nqb_max > 1 && predict_jac_lds(t.Mu, d, nqb_max) > kLdsBudget) nqb_max /= 2;
  const uint64_t chunk = std::min<uint64_t>(kPjChunk, 16 * (uint64_t)nqb_max);
  DevBuf<double> tht;
  OB_TRY(tht.alloc(p * chunk));
  for (uint64_t q0 = 0; q0 < q; q0 += chunk) {
    const int qc = (int)std::min<uint64_t>(chunk, q - q0);
    int nqb = 1;
    while (16 * nqb < qc) nqb *= 2;
    double *T = tht.p;
    OB_TRY(launch_theta_term_major(d_Theta + q0 * p, p, qc, 16 * (uint64_t)nqb, T));
    double *mc = d_mean ? d_mean + q0 * n : nullptr;
    double *jc = vjp ? nullptr : d_jac + q0 * d * n;
    const double *wc = vjp ? d_W + q0 * ldw : nullptr;
    const int first = q0 == 0;
#define OB_PJ(NQB_)                                                                                  \
  if (nqb == NQB_) {                                                                                 \
    if (vjp)                                                                                         \
      OB_TRY((run_predict_jac<NQB_, true>(m, t, T, qc, d_x, n, mc, jc, wc, ldw, first, d_out)));     \
    else                                                                                             \
      OB_TRY((run_predict_jac<NQB_, false>(m, t, T, qc, d_x, n, mc, jc, wc, ldw, first, d_out)));    \
  }
    OB_PJ(1)
    OB_PJ(2)
    OB_PJ(4)
#undef OB_PJ
  }
  return 0;
}

}  // namespace obhip
