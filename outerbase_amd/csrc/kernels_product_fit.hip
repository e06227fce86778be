// Kernels of the Newton fit on gridded data for gfx950 (include/obhip.h, "Newton fit on the product of two
// input blocks"; product_fit.cpp).  No reference counterpart.  With the notation of
// kernels_product.hip a design-matrix entry of the pair (i, j) is At[i,k] Bt[j,k], At = diag(sA) U (na x p),
// Bt = diag(sB) V (nb x p), so the normal equations of all na nb pairs separate:
//   B^T B = (At^T At) o (Bt^T Bt),   B^T 1 = (At^T 1) o (Bt^T 1),   (B^T y)_k = sum_i At[i,k] (Y Bt)[i,k].
// The matrix work stays in the Gram kernels and launch_atb; what is here streams HBM:
//   k_materialize_side    stages one side, row-major with a pitch -- the layout k_atb_dma2<kAtbGram> reads
//                         (kernels_gram_panel.hip).  Per 64-row tile (8 waves), as k_materialize_dx has it:
//                         1. lane = row: build_tile_side over the side's dimensions into a tile of pitch 65
//                            doubles, the row scale = the product of R_l0 over the side's own dimensions;
//                         2. lane = two adjacent terms, wave = 128 consecutive terms: per row one product of at
//                            most w factors read through the side's right-aligned column list; one wave
//                            instruction stores 1 KB of a staged row.  The column sum rides along: one partial
//                            per (tile, term), summed over the tiles in tile order by k_dx_colsum.
//                         Rows beyond n and terms beyond p are stored as exact zeros.  HBM = true (W2 = 0): the
//                         same code with the tile in a per-block slice of pooled HBM scratch and the column
//                         words read from memory, any number of used columns and of factors.
//   k_product_fit_shift   Y - c into the K x M operand of the right-hand sides' GEMM, padding zeroed.
//   k_product_rhs_dot     part[split][k] = sum_i At[i][k] W2[i][k], rows ascending; k_product_rhs_sum adds the
//                         splits in ascending order.  At is read once per block of responses.
//   k_acc_fold_hadamard   tri[e] += sign GA[e] GB[e] over the packed triangle.
// Every sum has a fixed order and nothing is atomic: two equal calls give the same bits.
#include "obhip_internal.h"
#include "device_dx.h"
#include "vec_ops.h"

namespace obhip {

namespace {

constexpr int kMsThreads = 512, kMsWaves = kMsThreads / 64;
constexpr int kMsPitch = 65;  // doubles between the columns of the LDS tile

struct MsArgs {
  const DimDesc *dims;
  const double *ka, *kb, *kc, *rot, *tab;
  const int *side;        // the side's dimensions; column s of x holds dimension side[s]
  int nside;
  const int *cpos;        // compact column -> the side's used column or -1
  int mu;                 // used columns of the side (column 0 = ones)
  const uint32_t *colsw;  // p x W2rt words of two used-column indices, right-aligned
  int W2rt;
  int p;
  const double *x;
  uint64_t ldx, n, ntiles;
  double *out;
  uint64_t pitch;
  int pcols;        // columns written per row (>= p: the rest zeros)
  int vec;          // 16-byte stores are aligned
  double *colpart;  // [ntiles][pitch] or null
  double *scratch;  // HBM tiles
};

// doubles of LDS behind the tile: [8][64] scale partials, [64] row scales
constexpr size_t kMsAux = (size_t)kMsWaves * kTileRows + kTileRows;

template <int W2, bool HBM>
__global__ void __launch_bounds__(kMsThreads) k_materialize_side(const MsArgs a) {
  extern __shared__ double lds[];
  constexpr int TP = HBM ? kTileRows : kMsPitch;
  constexpr int W = 2 * (W2 > 0 ? W2 : 1);
  double *tile = HBM ? a.scratch + (size_t)blockIdx.x * a.mu * kTileRows : lds;
  double *red = HBM ? lds : lds + (size_t)a.mu * TP;
  double *srow = red + kMsWaves * kTileRows;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ngroups = (a.pcols + 127) / 128;

  for (uint64_t tl = blockIdx.x; tl < a.ntiles; tl += gridDim.x) {
    const uint64_t row0 = tl * kTileRows, row = row0 + lane;
    const bool valid = row < a.n;
    // ---- 1. the side's used columns at the rows of the tile (lane = row) ----
    {
      const StoreTile<TP> store{tile, a.cpos, lane, a.mu};
      build_tile_side<kMsWaves>(a.dims, a.ka, a.kb, a.kc, a.rot, a.tab, a.side, a.nside, a.x, a.ldx, row, valid, wave,
                                wave, store, red);
    }
    __syncthreads();
    if (wave == 0) srow[lane] = valid ? tile_scale<kMsWaves>(red, lane) : 0.0;
    __syncthreads();

    // ---- 2. lane = two adjacent terms ----
    const int nvalid = (int)min((uint64_t)kTileRows, a.n - row0);  // (ntiles = ceil(n / 64): at least 1)
    for (int grp = wave; grp < ngroups; grp += kMsWaves) {
      const int k = grp * 128 + 2 * lane;
      const bool live0 = k < a.p, live1 = k + 1 < a.p;
      double acc0 = 0.0, acc1 = 0.0;
      int ca[2][W];
      if constexpr (W2 > 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int w = 0; w < W2; ++w) {
            const uint32_t cw = (k + i) < a.p ? a.colsw[(size_t)(k + i) * W2 + w] : 0u;
            ca[i][2 * w] = (int)(cw & 0xffffu) * TP;
            ca[i][2 * w + 1] = (int)(cw >> 16) * TP;
          }
      }
      for (int r = 0; r < kTileRows; ++r) {
        const bool rv = r < nvalid;
        double P[2] = {1.0, 1.0};
        if constexpr (W2 > 0) {
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            double pr = tile[ca[i][0] + r];
#pragma unroll
            for (int j = 1; j < W; ++j) pr *= tile[ca[i][j] + r];
            P[i] = pr;
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
        const double sr = srow[r];
        const double v0 = live0 && rv ? sr * P[0] : 0.0, v1 = live1 && rv ? sr * P[1] : 0.0;
        double *o = a.out + (row0 + r) * a.pitch + k;
        if (a.vec && k + 1 < a.pcols) {
          double2 w2;
          w2.x = v0;
          w2.y = v1;
          *(double2 *)o = w2;
        } else {
          if (k < a.pcols) o[0] = v0;
          if (k + 1 < a.pcols) o[1] = v1;
        }
        acc0 += v0;
        acc1 += v1;
      }
      if (a.colpart) {
        if ((uint64_t)k < a.pitch) a.colpart[tl * a.pitch + k] = acc0;
        if ((uint64_t)k + 1 < a.pitch) a.colpart[tl * a.pitch + k + 1] = acc1;
      }
    }
    __syncthreads();  // the tile is free for the next tile
  }
}

template <int W2, bool HBM>
int run_materialize_side(const obhip_model &m, obhip_terms &t, const SideStage &s) {
  const obhip_terms::Product &pr = t.product;
  const ModelDev &md = t.pred_md;
  const uint64_t mu = s.side ? pr.mu_b : pr.mu_a;
  const size_t lds = ((HBM ? 0 : mu * kMsPitch) + kMsAux) * sizeof(double);
  OB_TRY(ensure_dyn_lds((const void *)k_materialize_side<W2, HBM>, lds));
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t ntiles = (s.n + kTileRows - 1) / kTileRows;
  uint64_t nblk = std::min<uint64_t>(ntiles, (uint64_t)device_cus(dev) * 2);
  DevBuf<double> scratch;
  if (HBM) {
    nblk = hbm_tile_blocks(nblk, mu);
    OB_TRY(scratch.alloc(nblk * mu * kTileRows));
  }
  MsArgs a;
  a.dims = md.dims.p, a.ka = md.ka.p, a.kb = md.kb.p, a.kc = md.kc.p, a.rot = md.rot.p, a.tab = md.tab.p;
  a.side = s.side ? pr.side_b.p : pr.side_a.p;
  a.nside = (int)(s.side ? pr.dims_b.size() : m.d - pr.dims_b.size());
  a.cpos = s.side ? pr.cpos_b.p : pr.cpos_a.p;
  a.mu = (int)mu;
  a.colsw = (const uint32_t *)(s.side ? pr.cols_b.p : pr.cols_a.p);
  a.W2rt = (int)((s.side ? pr.wb : pr.wa) / 2);
  a.p = (int)t.p;
  a.x = s.x, a.ldx = s.ldx, a.n = s.n, a.ntiles = ntiles;
  a.out = s.out, a.pitch = s.pitch;
  a.pcols = (int)s.pcols;
  a.vec = (s.pitch % 2 == 0 && ((uintptr_t)s.out & 15) == 0) ? 1 : 0;
  a.colpart = s.colpart;
  a.scratch = scratch.p;
  hipLaunchKernelGGL((k_materialize_side<W2, HBM>), dim3((unsigned)nblk), dim3(kMsThreads), lds, cur_stream(), a);
  OB_HIP(hipGetLastError());
  // (scratch goes back to the pool under this stream: handed out again to work queued behind the kernel)
  return 0;
}

// Ys = Y - c in product_fit_ys_at's layout; one thread per entry of the padded copy
__global__ void __launch_bounds__(256)
k_product_fit_shift(const double *__restrict__ Y, uint64_t lda, uint64_t na, uint64_t nb, uint64_t q, uint64_t rb,
                    uint64_t nbp, uint64_t ldp, const double *__restrict__ mom_batch, double *__restrict__ Ys) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= q * nbp * ldp) return;
  const uint64_t i = e % ldp, j = (e / ldp) % nbp, r = e / (ldp * nbp);
  const double v = (i < na && j < nb) ? Y[(r * nb + j) * lda + i] - mom_batch[4 * r] : 0.0;
  Ys[product_fit_ys_at(r, j, i, q, rb, nbp, ldp)] = v;
}

// part[(rr ns + s) pitch + k] = sum over the rows of split s of A[i][k] W2[rr ldw + i][k]
__global__ void __launch_bounds__(256)
k_product_rhs_dot(const double *__restrict__ A, const double *__restrict__ W2, uint64_t pitch, uint64_t na,
                  uint64_t ldw, int rc, uint64_t rows_per, uint64_t p, double *__restrict__ part) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= p) return;
  const uint64_t s = blockIdx.y, ns = gridDim.y;
  const uint64_t r0 = s * rows_per, r1 = min(na, r0 + rows_per);
  double acc[kFitRespBlock];
#pragma unroll
  for (int rr = 0; rr < (int)kFitRespBlock; ++rr) acc[rr] = 0.0;
  for (uint64_t i = r0; i < r1; ++i) {
    const double av = A[i * pitch + k];
#pragma unroll
    for (int rr = 0; rr < (int)kFitRespBlock; ++rr)
      if (rr < rc) acc[rr] = fma(av, W2[((uint64_t)rr * ldw + i) * pitch + k], acc[rr]);
  }
#pragma unroll
  for (int rr = 0; rr < (int)kFitRespBlock; ++rr)
    if (rr < rc) part[((uint64_t)rr * ns + s) * pitch + k] = acc[rr];
}

// R[rr p + k] (+)= sum_s part[(rr ns + s) pitch + k], s ascending
__global__ void __launch_bounds__(256)
k_product_rhs_sum(const double *__restrict__ part, uint64_t ns, uint64_t pitch, uint64_t p, int accumulate,
                  double *__restrict__ R) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= p) return;
  const uint64_t rr = blockIdx.y;
  double acc = 0.0;
  for (uint64_t s = 0; s < ns; ++s) acc += part[(rr * ns + s) * pitch + k];
  R[rr * p + k] = accumulate ? R[rr * p + k] + acc : acc;
}

// tri[e] += sign GA[e] GB[e]: two entries per lane and load where the three streams are 16-byte aligned,
// grid-stride, then the odd last entry
__global__ void __launch_bounds__(256)
k_acc_fold_hadamard(double *__restrict__ tri, const double *__restrict__ GA, const double *__restrict__ GB,
                    uint64_t count, int vec, double sign) {
  const uint64_t stride = (uint64_t)gridDim.x * 256, first = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (!vec) {
    for (uint64_t e = first; e < count; e += stride) tri[e] += sign * (GA[e] * GB[e]);
    return;
  }
  const uint64_t pairs = count / 2;
  double2 *d2 = reinterpret_cast<double2 *>(tri);
  const double2 *a2 = reinterpret_cast<const double2 *>(GA);
  const double2 *b2 = reinterpret_cast<const double2 *>(GB);
  for (uint64_t e = first; e < pairs; e += stride) {
    double2 d = d2[e];
    const double2 x = a2[e], y = b2[e];
    d.x += sign * (x.x * y.x);
    d.y += sign * (x.y * y.y);
    d2[e] = d;
  }
  if ((count & 1) && first == 0) tri[count - 1] += sign * (GA[count - 1] * GB[count - 1]);
}

}  // namespace

// the fused kernel's domain: at most 8 factors per term on the side and a tile that fits the LDS
bool materialize_side_supports(uint64_t mu, uint64_t w) {
  return w >= 2 && w <= 8 && w % 2 == 0 && (mu * kMsPitch + kMsAux) * sizeof(double) <= kLdsBudget;
}

// after ensure_product_tables(m, t, split); s.n >= 1
int launch_materialize_side(const obhip_model &m, obhip_terms &t, const SideStage &s) {
  ProfScope ps(s.side ? "materialize_side_b" : "materialize_side_a");
  const uint64_t mu = s.side ? t.product.mu_b : t.product.mu_a, w = s.side ? t.product.wb : t.product.wa;
  const bool fused = materialize_side_supports(mu, w) && !getenv("OBHIP_FORCE_GENERIC");
  if (!fused) return run_materialize_side<0, true>(m, t, s);
  switch (w / 2) {
    case 1: return run_materialize_side<1, false>(m, t, s);
    case 2: return run_materialize_side<2, false>(m, t, s);
    case 3: return run_materialize_side<3, false>(m, t, s);
    default: return run_materialize_side<4, false>(m, t, s);
  }
}

int launch_product_fit_moments(const double *d_Y, uint64_t lda, uint64_t na, uint64_t nb, uint64_t q, uint64_t rb,
                               uint64_t nbp, uint64_t ldp, bool empty, const double *d_mom_state, double *d_mom_batch,
                               double *d_Ys, double *d_part) {
  ProfScope ps("product_fit_moments");
  const int isempty = empty ? 1 : 0;
  // the shift of every response: the state's, or the batch's first value for an empty state
  OB_TRY(vmap(q, [=] __device__(uint64_t r) { d_mom_batch[4 * r] = isempty ? d_Y[r * nb * lda] : d_mom_state[4 * r]; }));
  const uint64_t total = q * nbp * ldp;
  if ((total + 255) / 256 > 0x7fffffffull) return fail(OBHIP_ERR_INVALID, "normal_acc_add_product_dev: batch too large");
  hipLaunchKernelGGL(k_product_fit_shift, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, cur_stream(), d_Y, lda, na,
                     nb, q, rb, nbp, ldp, (const double *)d_mom_batch, d_Ys);
  OB_HIP(hipGetLastError());
  // (mu, M2, n) of the shifted batch by launch_acc_batch_moments' two passes over the na nb values, i fast
  const uint64_t n = na * nb;
  const double *ys = d_Ys;
  double *mom = d_mom_batch;
  const double nrows = (double)n;
  OB_TRY(vcolsum(n, q, [=] __device__(int r, uint64_t e, double &acc) {
    acc += ys[product_fit_ys_at((uint64_t)r, e / na, e % na, q, rb, nbp, ldp)];
  }, [=] __device__(int r, double s) {
    mom[4 * r + 1] = s / nrows;
    mom[4 * r + 3] = nrows;
  }, d_part));
  return vcolsum(n, q, [=] __device__(int r, uint64_t e, double &acc) {
    const double c = ys[product_fit_ys_at((uint64_t)r, e / na, e % na, q, rb, nbp, ldp)] - mom[4 * r + 1];
    acc = fma(c, c, acc);
  }, [=] __device__(int r, double s) { mom[4 * r + 2] = s; }, d_part);
}

uint64_t product_rhs_splits(uint64_t na) { return std::max<uint64_t>(1, std::min<uint64_t>(64, na / 64)); }

int launch_product_rhs_dot(const double *d_A, const double *d_W2, uint64_t pitch, uint64_t na, uint64_t ldw,
                           uint64_t rc, uint64_t p, bool accumulate, double *d_part, double *d_R) {
  ProfScope ps("product_rhs_dot");
  const uint64_t ns = product_rhs_splits(na), per = (na + ns - 1) / ns;
  const unsigned kb = (unsigned)((p + 255) / 256);
  hipLaunchKernelGGL(k_product_rhs_dot, dim3(kb, (unsigned)ns), dim3(256), 0, cur_stream(), d_A, d_W2, pitch, na, ldw,
                     (int)rc, per, p, d_part);
  hipLaunchKernelGGL(k_product_rhs_sum, dim3(kb, (unsigned)rc), dim3(256), 0, cur_stream(), (const double *)d_part, ns,
                     pitch, p, accumulate ? 1 : 0, d_R);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_acc_fold_hadamard(uint64_t p, double *d_tri, const double *d_GA, const double *d_GB, double sign) {
  const uint64_t tri = p * (p + 1) / 2;
  const int vec = (((uintptr_t)d_tri | (uintptr_t)d_GA | (uintptr_t)d_GB) & 15) == 0 ? 1 : 0;
  const unsigned blocks = (unsigned)std::min<uint64_t>(8192, (tri / 2 + 255) / 256 + 1);
  hipLaunchKernelGGL(k_acc_fold_hadamard, dim3(blocks), dim3(256), 0, cur_stream(), d_tri, d_GA, d_GB, tri, vec, sign);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_hadamard(uint64_t p, const double *d_a, const double *d_b, double *d_out) {
  return vmap(p, [=] __device__(uint64_t k) { d_out[k] = d_a[k] * d_b[k]; });
}

}  // namespace obhip
