// Staging kernel of the derivative design matrix for gfx950: at rows x and for a list of L
// differentiated dimensions the L row blocks sqrt(w_j) D_j, D_j[i,k] = dB[i,k] / dx_{dims[j]}, written
// row-major with a pitch -- the layout k_atb_dma2<kAtbGram> reads (kernels_gram_panel.hip), so that the
// Gram kernels form sum_j w_j D_j^T D_j from it.  No reference counterpart; the formulas are those of
// include/obhip.h at obhip_predict_grad_dev:
//   D_l[i,k] = s_i (rho_l P_k + [t_kl > 0] E_kl r'_{l,t_kl})
// P_k the term product, E_kl the product of the term's OTHER factors (a product, never a quotient).
//
// Per 64-row tile (8 waves):
//   1. lane = row: the waves evaluate the dimensions (wave w takes w, w + 8, ...; build_dim_dx_any)
//      into the tile exactly as phase 1 of k_predict_dx does: Mu value columns (column 0 = ones), the
//      derivative column of every used column >= 1, d columns of rho_l; the row scale s through a
//      wave-ordered product.  Tile pitch 65 doubles: phase 2 reads 64 DIFFERENT columns at one row.
//   2. lane = two adjacent terms, wave = 128 consecutive terms (wave w takes the groups w, w + 8, ...).
//      Per row the lane forms P and, for every factor j of its terms, G_j = E_j r'_j ONCE (prefix and
//      suffix products over the at most 8 factors); the loop over the L dimensions then only selects:
//        value = sqrt(w_l) s (rho_l P + sum_j [dimension of factor j = l] G_j)
//      -- the LDS reads do not depend on l.  One wave instruction stores 1 KB of one staged row.
//      The right-hand side rides along as WITH_Y does in k_materialize_tl: acc += value sqrt(w_l) g_l[row],
//      one partial per (tile, term), summed over the tiles in tile order by k_dx_colsum.  No atomics:
//      two calls give the same bits.
// Rows beyond n are stored as exact zeros (pad_rows) or not at all; terms beyond p likewise.
//
// HBM = false: the tile lives in LDS (materialize_dx_supports).  HBM = true (W2 = 0): the same code
// with the tile in a per-block slice of pooled HBM scratch and the column words read from memory, any
// number of used columns and of factors: the fallback, also under OBHIP_FORCE_GENERIC.
#include "obhip_internal.h"
#include "device_dx.h"

namespace obhip {

namespace {

constexpr int kMdThreads = 512, kMdWaves = kMdThreads / 64;
constexpr int kMdPitch = 65;  // doubles between the columns of the LDS tile

struct MdArgs : PredTabs {
  const uint32_t *colsw;  // p_pad x W2rt words of two used-column indices
  int W2rt;
  const int *udim;        // used column -> its dimension (-1: the ones column)
  int p;
  const double *x;        // column-major, leading dimension ldx
  uint64_t ldx, n, ntiles;
  const uint32_t *ldims;  // L differentiated dimensions
  const double *sqw;      // L: sqrt(w_j)
  int L;
  double *out;
  uint64_t pitch, blk_rows;  // out[(j * blk_rows + i) * pitch + k]
  int pcols;                 // columns written per row (>= p: the rest zeros)
  int pad_rows;              // rows n .. 64 ntiles written as zeros
  int vec;                   // 16-byte stores are aligned
  const double *g;           // optional: g[j * ldg + i], the gradient observations of one response
  uint64_t ldg;
  double *ypart;             // [ntiles][pitch]
  double *scratch;           // HBM tiles
};

// doubles of LDS behind the tile: [8][64] scale partials, [64] row scales, [d][64] sqrt(w) g, [d] sqrt(w),
// [d] dimensions (ints)
__host__ __device__ inline size_t md_aux_doubles(int d) {
  return (size_t)kMdWaves * kTileRows + kTileRows + (size_t)d * kTileRows + d + (d + 1) / 2;
}

template <int W2, bool HBM>
__global__ void __launch_bounds__(kMdThreads) k_materialize_dx(const MdArgs a) {
  extern __shared__ double lds[];
  constexpr int TP = HBM ? kTileRows : kMdPitch;
  constexpr int W = 2 * (W2 > 0 ? W2 : 1);
  const int Mu = a.Mu, d = a.d, L = a.L;
  const int ncols = 2 * Mu - 1 + d;
  double *tile = HBM ? a.scratch + (size_t)blockIdx.x * ncols * kTileRows : lds;
  double *red = HBM ? lds : lds + (size_t)ncols * TP;
  double *srow = red + kMdWaves * kTileRows;
  double *gs = srow + kTileRows;
  double *lsq = gs + (size_t)d * kTileRows;
  int *ldm = (int *)(lsq + d);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int dofs = (Mu - 1) * TP;  // from a used column >= 1 to its derivative column
  const int ngroups = (a.pcols + 127) / 128;

  for (int li = threadIdx.x; li < L; li += kMdThreads) {  // (read after the first barrier of the tile loop)
    lsq[li] = a.sqw[li];
    ldm[li] = (int)a.ldims[li];
  }

  for (uint64_t tl = blockIdx.x; tl < a.ntiles; tl += gridDim.x) {
    const uint64_t row0 = tl * kTileRows, row = row0 + lane;
    const bool valid = row < a.n;
    // ---- 1. basis, derivative basis and rho at the rows of the tile (lane = row) ----
    {
      // (build_tile's loop, kept here: through the builder the HBM instantiation takes one VGPR more, 169,
      // and with it drops below three waves per SIMD -- DESIGN §16)
      double sc = 1.0;
      const StoreTile<TP> store{tile, a.cpos, lane, Mu};
      for (int l = wave; l < d; l += kMdWaves) {
        const DimDesc D = a.dims[l];
        const double xv = valid ? a.x[(uint64_t)l * a.ldx + row] : 0.5;
        double rho;
        sc *= build_dim_dx_any(D, a.ka, a.kb, a.kc, a.rot, a.tab, a.dtab, xv, store, rho);
        store.rho(l, rho);
      }
      if (wave == 0) tile[lane] = 1.0;  // (the ones column)
      red[wave * kTileRows + lane] = sc;
      if (a.g)
        for (int li = wave; li < L; li += kMdWaves)
          gs[li * kTileRows + lane] = valid ? a.sqw[li] * a.g[(uint64_t)li * a.ldg + row] : 0.0;
    }
    __syncthreads();
    if (wave == 0) srow[lane] = valid ? tile_scale<kMdWaves>(red, lane) : 0.0;
    __syncthreads();

    // ---- 2. lane = two adjacent terms ----
    const int nvalid = (int)min((uint64_t)kTileRows, a.n - row0);  // (ntiles = ceil(n / 64): at least 1)
    const int nrows = a.pad_rows ? kTileRows : nvalid;
    for (int grp = wave; grp < ngroups; grp += kMdWaves) {
      const int k = grp * 128 + 2 * lane;
      const bool live0 = k < a.p, live1 = k + 1 < a.p;
      double acc0 = 0.0, acc1 = 0.0;
      int ca[2][W], dm[2][W];
      if constexpr (W2 > 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int w = 0; w < W2; ++w) {
            const uint32_t cw = (k + i) < a.p ? a.colsw[(size_t)(k + i) * W2 + w] : 0u;
            const int c0 = (int)(cw & 0xffffu), c1 = (int)(cw >> 16);
            ca[i][2 * w] = c0 * TP;
            ca[i][2 * w + 1] = c1 * TP;
            dm[i][2 * w] = a.udim[c0];
            dm[i][2 * w + 1] = a.udim[c1];
          }
      }
      for (int r = 0; r < nrows; ++r) {
        const bool rv = r < nvalid;
        const double sr = srow[r];
        double P[2] = {0.0, 0.0}, G[2][W];
        if constexpr (W2 > 0) {
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            double v[W], pre = 1.0;
#pragma unroll
            for (int j = 0; j < W; ++j) {
              v[j] = tile[ca[i][j] + r];
              G[i][j] = pre * tile[ca[i][j] + dofs + r];  // (prefix) r'_j; the ones slots are never selected
              pre *= v[j];
            }
            P[i] = pre;
            double suf = 1.0;
#pragma unroll
            for (int j = W - 1; j >= 0; --j) {
              G[i][j] *= suf;
              suf *= v[j];
            }
          }
        } else {
          for (int i = 0; i < 2; ++i) {
            if (k + i >= a.p) continue;
            const uint32_t *cwp = a.colsw + (size_t)(k + i) * a.W2rt;
            double pr = 1.0;
            for (int w = 0; w < a.W2rt; ++w) {
              const uint32_t c = cwp[w];
              pr *= tile[(c & 0xffffu) * TP + r];
              pr *= tile[(c >> 16) * TP + r];
            }
            P[i] = pr;
          }
        }
        for (int li = 0; li < L; ++li) {
          const int l = ldm[li];
          const double rho = tile[(2 * Mu - 1 + l) * TP + r];
          const double cf = sr * lsq[li];
          double val[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            double aa = rho * P[i];
            if constexpr (W2 > 0) {
#pragma unroll
              for (int j = 0; j < W; ++j) aa += dm[i][j] == l ? G[i][j] : 0.0;
            } else if (k + i < a.p) {
              const uint32_t *cwp = a.colsw + (size_t)(k + i) * a.W2rt;
              for (int j = 0; j < 2 * a.W2rt; ++j) {
                const uint32_t cj = (cwp[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
                if (cj == 0 || a.udim[cj] != l) continue;
                double E = 1.0;
                for (int q = 0; q < 2 * a.W2rt; ++q) {
                  const uint32_t cq = (cwp[q >> 1] >> ((q & 1) * 16)) & 0xffffu;
                  if (q != j) E *= tile[cq * TP + r];
                }
                aa = fma(E, tile[(Mu + cj - 1) * TP + r], aa);
              }
            }
            val[i] = cf * aa;
          }
          const double v0 = live0 && rv ? val[0] : 0.0, v1 = live1 && rv ? val[1] : 0.0;
          double *o = a.out + ((uint64_t)li * a.blk_rows + row0 + r) * a.pitch + k;
          if (a.vec && k + 1 < a.pcols) {
            double2 w2;
            w2.x = v0;
            w2.y = v1;
            *(double2 *)o = w2;
          } else {
            if (k < a.pcols) o[0] = v0;
            if (k + 1 < a.pcols) o[1] = v1;
          }
          if (a.g) {
            const double gv = gs[li * kTileRows + r];
            acc0 = fma(v0, gv, acc0);
            acc1 = fma(v1, gv, acc1);
          }
        }
      }
      if (a.g) {
        if ((uint64_t)k < a.pitch) a.ypart[tl * a.pitch + k] = acc0;
        if ((uint64_t)k + 1 < a.pitch) a.ypart[tl * a.pitch + k + 1] = acc1;
      }
    }
    __syncthreads();  // the tile is free for the next tile
  }
}

// part[s][k] = sum over the rows of split s of B[row][k] sqrt(w_j) g[j * ldg + i], row = j * blk_rows + i
// (the further responses of a batch: one pass over the staged chunk per response)
__global__ void __launch_bounds__(256)
k_dx_aty(const double *__restrict__ B, uint64_t pitch, uint64_t blk_rows, uint64_t rows, uint64_t rows_per,
         uint64_t n, const double *__restrict__ sqw, const double *__restrict__ g, uint64_t ldg,
         double *__restrict__ part) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= pitch) return;
  const uint64_t r0 = (uint64_t)blockIdx.y * rows_per, r1 = min(rows, r0 + rows_per);
  double acc = 0.0;
  for (uint64_t row = r0; row < r1; ++row) {
    const uint64_t j = row / blk_rows, i = row - j * blk_rows;
    const double gv = i < n ? sqw[j] * g[j * ldg + i] : 0.0;
    acc = fma(B[row * pitch + k], gv, acc);
  }
  part[(uint64_t)blockIdx.y * pitch + k] = acc;
}

// out[k] (+)= sum_s part[s][k], s ascending
__global__ void __launch_bounds__(256)
k_dx_colsum(const double *__restrict__ part, uint64_t nsplit, uint64_t pitch, int p, int accumulate,
            double *__restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= p) return;
  double acc = 0.0;
  for (uint64_t s = 0; s < nsplit; ++s) acc += part[s * pitch + k];
  out[k] = accumulate ? out[k] + acc : acc;
}

template <int W2, bool HBM>
int run_materialize_dx(const obhip_model &m, obhip_terms &t, const DxStage &s) {
  const uint64_t ncols = 2 * t.Mu - 1 + m.d;
  const size_t lds = ((HBM ? 0 : ncols * kMdPitch) + md_aux_doubles((int)m.d)) * sizeof(double);
  OB_TRY(ensure_dyn_lds((const void *)k_materialize_dx<W2, HBM>, lds));
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t ntiles = (s.n + kTileRows - 1) / kTileRows;
  uint64_t nblk = std::min<uint64_t>(ntiles, (uint64_t)device_cus(dev) * 2);
  DevBuf<double> scratch;
  if (HBM) {
    nblk = hbm_tile_blocks(nblk, ncols);
    OB_TRY(scratch.alloc(nblk * ncols * kTileRows));
  }
  MdArgs a;
  static_cast<PredTabs &>(a) = pred_tabs(m, t);
  a.colsw = (const uint32_t *)t.cols.p;
  a.W2rt = (int)(t.W / 2);
  a.udim = t.dx.udim.p;
  a.p = (int)t.p;
  a.x = s.x, a.ldx = s.ldx, a.n = s.n, a.ntiles = ntiles;
  a.ldims = s.dims, a.sqw = s.sqw, a.L = (int)s.L;
  a.out = s.out, a.pitch = s.pitch, a.blk_rows = s.blk_rows;
  a.pcols = (int)s.pcols;
  a.pad_rows = s.pad_rows ? 1 : 0;
  a.vec = (s.pitch % 2 == 0 && ((uintptr_t)s.out & 15) == 0) ? 1 : 0;
  a.g = s.ypart ? s.g : nullptr;
  a.ldg = s.ldg;
  a.ypart = s.ypart;
  a.scratch = scratch.p;
  hipLaunchKernelGGL((k_materialize_dx<W2, HBM>), dim3((unsigned)nblk), dim3(kMdThreads), lds, cur_stream(), a);
  OB_HIP(hipGetLastError());
  // (scratch goes back to the pool under this stream: handed out again to work queued behind the kernel)
  return 0;
}

}  // namespace

// the fused kernel's domain: at most 8 factors per term and a tile that fits the LDS
bool materialize_dx_supports(const obhip_terms &t) {
  const uint64_t w2 = t.W / 2;
  return w2 >= 1 && w2 <= 4 &&
         ((2 * t.Mu - 1 + t.d) * kMdPitch + md_aux_doubles((int)t.d)) * sizeof(double) <= kLdsBudget;
}

// after ensure_dx_stage(m, t); s.n >= 1
int launch_materialize_dx(const obhip_model &m, obhip_terms &t, const DxStage &s) {
  ProfScope ps("materialize_dx");
  const bool fused = materialize_dx_supports(t) && !getenv("OBHIP_FORCE_GENERIC");
  if (!fused) return run_materialize_dx<0, true>(m, t, s);
  switch (t.W / 2) {
    case 1: return run_materialize_dx<1, false>(m, t, s);
    case 2: return run_materialize_dx<2, false>(m, t, s);
    case 3: return run_materialize_dx<3, false>(m, t, s);
    default: return run_materialize_dx<4, false>(m, t, s);
  }
}

// d_out (p) (+)= (staged chunk)^T (sqrt(w) g) for one further response; d_part: dx_aty_splits x pitch
uint64_t dx_aty_splits(uint64_t rows) { return std::max<uint64_t>(1, std::min<uint64_t>(64, rows / 256)); }

int launch_dx_aty(const double *d_B, uint64_t pitch, uint64_t blk_rows, uint64_t L, uint64_t n, const double *d_sqw,
                  const double *d_g, uint64_t ldg, double *d_part, uint64_t p, bool accumulate, double *d_out) {
  const uint64_t rows = blk_rows * L, ns = dx_aty_splits(rows), per = (rows + ns - 1) / ns;
  hipLaunchKernelGGL(k_dx_aty, dim3((unsigned)((pitch + 255) / 256), (unsigned)ns), dim3(256), 0, cur_stream(), d_B, pitch,
                     blk_rows, rows, per, n, d_sqw, d_g, ldg, d_part);
  OB_HIP(hipGetLastError());
  return launch_dx_colsum(d_part, ns, pitch, p, accumulate, d_out);
}

int launch_dx_colsum(const double *d_part, uint64_t nsplit, uint64_t pitch, uint64_t p, bool accumulate, double *d_out) {
  hipLaunchKernelGGL(k_dx_colsum, dim3((unsigned)((p + 255) / 256)), dim3(256), 0, cur_stream(), d_part, nsplit, pitch,
                     (int)p, accumulate ? 1 : 0, d_out);
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace obhip
