// Kernels of the multi-response Newton fit and predictor (fit_newton.cpp): q responses over one
// design x share the Gram, the Hessian and its Cholesky factor; what depends on Y is batched
// over the responses in column blocks of 16, the n of v_mfma_f64_16x16x4_f64.
//
//   k_aty_multi      C[p x q] = B^T Y from the staged row-major design matrix (ensure_bmat): a
//                    skinny GEMM that reads B once for up to 64 responses; split over row ranges,
//                    the partial tiles summed in a fixed order by k_aty_reduce (no atomics).
//   k_trsm_fwd/_bwd  L Z = R and L^T Theta = Z for up to 64 right-hand sides on the finished factor:
//                    per 64-row block the diagonal solve with the 16 x 16 inverses the panel step of
//                    the factorisation left in the workspace, then the 64 x 64 x 16 updates of the
//                    blocks below (forward) / above (backward) on the matrix cores.  No L^-1.
//   k_predict_multi  per 64-row tile of new inputs the basis goes to LDS as in k_predict; the term
//                    products are formed ONCE per (row, term) as the A operand and multiplied with
//                    the 4 x 16 slice of Theta on the matrix cores.
//
// MFMA operand layout (as in kernels_chol.hip): lane = (m | n) + 16 k for A[m][k] and B[k][n];
// the four accumulator registers of a lane are D[k + 4 r][n], r = 0..3.
#include "obhip_internal.h"
#include "device_dx.h"
#include "vec_ops.h"

namespace obhip {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int NB = 64;        // rows of a block of the factor (kernels_chol.hip)
constexpr int LDP = NB + 1;   // padded LDS pitch of a 64 x 64 block
constexpr int XP = 17;        // pitch of a 64 x 16 block of right-hand sides

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// ---- B^T Y ----------------------------------------------------------------------------------
// Workgroup (cx, split): 256 columns of B (64 per wave, four 16-column MFMA tiles), the rows
// [split * rows_per, ...) in MFMA steps of four.  A[m][k] = B[r + k][c + m] are 128-byte pieces of four
// rows of the row-major matrix; the Y operand is small and re-read from L2 by every column tile.
template <int NQB>
__global__ void __launch_bounds__(256)
k_aty_multi(const double *__restrict__ B, uint64_t ldb, uint64_t n, const double *__restrict__ Y,
            uint64_t ldy, int q, uint64_t rows_per, double *__restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 15, kq = lane >> 4;
  const uint64_t c0 = (uint64_t)blockIdx.x * 256 + wave * 64;
  const uint64_t r0 = (uint64_t)blockIdx.y * rows_per, r1 = min(n, r0 + rows_per);
  d4 acc[4][NQB];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int j = 0; j < NQB; ++j) acc[t][j] = d4{0.0, 0.0, 0.0, 0.0};
  bool cok[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) cok[t] = c0 + 16 * t + m < ldb;
  const double *yp[NQB];
  bool yok[NQB];
#pragma unroll
  for (int j = 0; j < NQB; ++j) {
    yok[j] = 16 * j + m < q;
    yp[j] = Y + (uint64_t)min(16 * j + m, q - 1) * ldy;
  }
  // sixteen rows per trip: the loads of four steps are in flight before the first MFMA needs one
  for (uint64_t r = r0; r < r1; r += 16) {
    double a[4][4], y[4][NQB];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint64_t row = r + 4 * u + kq;
      const bool ok = row < r1;
      const uint64_t rc = ok ? row : r0;
      const double *bp = B + rc * ldb + c0 + m;
#pragma unroll
      for (int t = 0; t < 4; ++t) a[u][t] = (ok && cok[t]) ? bp[16 * t] : 0.0;
#pragma unroll
      for (int j = 0; j < NQB; ++j) y[u][j] = (ok && yok[j]) ? yp[j][rc] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < NQB; ++j) acc[t][j] = mfma(a[u][t], y[u][j], acc[t][j]);
  }
  // part[split][response][column of B]
  double *dst = part + (uint64_t)blockIdx.y * (16 * NQB) * ldb;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int j = 0; j < NQB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint64_t c = c0 + 16 * t + kq + 4 * r;
        if (c < ldb) dst[(uint64_t)(16 * j + m) * ldb + c] = acc[t][j][r];
      }
}

// out[j * ldo + k] = sum over the splits, in ascending order (perm: column k of the staged matrix is term
// perm[k], whose row of out the sum belongs to)
__global__ void __launch_bounds__(256)
k_aty_reduce(const double *__restrict__ part, int nsplit, int qw, uint64_t ldb, int p, int q,
             double *__restrict__ out, uint64_t ldo, const uint32_t *__restrict__ perm) {
  const int k = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  if (k >= p || j >= q) return;
  double s = 0.0;
  for (int sp = 0; sp < nsplit; ++sp) s += part[((uint64_t)sp * qw + j) * ldb + k];
  out[(uint64_t)j * ldo + (perm ? perm[k] : (uint32_t)k)] = s;
}

// ---- triangular solves with up to 64 right-hand sides ------------------------------------------
// Z, X: [p rounded up to 64][64] row-major, rows beyond p and columns beyond the chunk zero.
__global__ void __launch_bounds__(256)
k_trsm_load(const double *__restrict__ R, uint64_t ldr, int p, int pp, int qc, double e2,
            double *__restrict__ Z) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= pp * 64) return;
  const int k = idx >> 6, j = idx & 63;
  Z[idx] = (k < p && j < qc) ? e2 * R[(uint64_t)j * ldr + k] : 0.0;
}

__global__ void __launch_bounds__(256)
k_trsm_store(const double *__restrict__ Z, int p, int qc, double *__restrict__ T, uint64_t ldt) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int j = idx / p, k = idx % p;
  if (j < qc) T[(uint64_t)j * ldt + k] = Z[(size_t)k * 64 + j];
}

// the diagonal block of L (identity padding beyond jb), its four 16 x 16 inverses and the 64 x 16
// block of right-hand sides -> LDS
__device__ __forceinline__ void trsm_stage(const double *__restrict__ L, int p, int j0, int jb,
                                           const double *__restrict__ Iinv, const double *__restrict__ src,
                                           int qoff, double *Ld, double *Iv, double *X) {
  double t[NB * NB / 256], ti[4], tx[4];
#pragma unroll
  for (int i = 0; i < NB * NB / 256; ++i) {
    const int e = threadIdx.x + i * 256;
    t[i] = L[(size_t)(j0 + min(e / NB, jb - 1)) * p + j0 + min(e % NB, jb - 1)];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = threadIdx.x + i * 256;
    ti[i] = Iinv[(size_t)(j0 / NB) * 1024 + e];
    tx[i] = src[(size_t)(j0 + (e >> 4)) * 64 + qoff + (e & 15)];
  }
#pragma unroll
  for (int i = 0; i < NB * NB / 256; ++i) {
    const int e = threadIdx.x + i * 256;
    const int r = e / NB, c = e % NB;
    Ld[r * LDP + c] = (r < jb && c < jb && c <= r) ? t[i] : ((r == c) ? 1.0 : 0.0);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = threadIdx.x + i * 256;
    Iv[e] = ti[i];
    X[(e >> 4) * XP + (e & 15)] = tx[i];
  }
}

// Forward step of block j0: every workgroup solves L_jj X = Z_j itself (cheaper than a launch
// boundary, as k_chol_back does), workgroup x then takes Z_i -= L_ij X for the row block
// i = j + 1 + x.  X goes to a second array: the other workgroups of the launch still read Z_j.
__global__ void __launch_bounds__(256)
k_trsm_fwd(const double *__restrict__ L, int p, int j0, const double *__restrict__ Iinv,
           double *__restrict__ Z, double *__restrict__ Xs) {
  __shared__ double Ld[NB * LDP];
  __shared__ double Iv[4 * 256];
  __shared__ double X[NB * XP];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = lane & 15, kq = lane >> 4;
  const int jb = min(NB, p - j0);
  const int qoff = 16 * (int)blockIdx.y;
  const int i0 = j0 + NB * ((int)blockIdx.x + 1);
  const bool upd = i0 < p;
  const int ib = min(NB, p - i0);
  // the rows of L below do not depend on X: requested now, they arrive under the solve
  double lo[NB * NB / 256];
  if (upd) {
#pragma unroll
    for (int i = 0; i < NB * NB / 256; ++i) {
      const int e = threadIdx.x + i * 256;
      lo[i] = L[(size_t)(i0 + min(e / NB, ib - 1)) * p + j0 + min(e % NB, jb - 1)];
    }
  }
  trsm_stage(L, p, j0, jb, Iinv, Z, qoff, Ld, Iv, X);
  __syncthreads();
  if (wave == 0) {  // wave-local: X_b = inv(L_bb) (Z_b - sum_{c < b} L_bc X_c)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      d4 acc = d4{0.0, 0.0, 0.0, 0.0};
      for (int c = 0; c < b; ++c)
#pragma unroll
        for (int s = 0; s < 4; ++s)
          acc = mfma(Ld[(16 * b + m) * LDP + 16 * c + 4 * s + kq], X[(16 * c + 4 * s + kq) * XP + m], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) X[(16 * b + kq + 4 * r) * XP + m] -= acc[r];
      __builtin_amdgcn_wave_barrier();
      d4 xb = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4; ++s)
        xb = mfma(Iv[b * 256 + m * 16 + 4 * s + kq], X[(16 * b + 4 * s + kq) * XP + m], xb);
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int r = 0; r < 4; ++r) X[(16 * b + kq + 4 * r) * XP + m] = xb[r];
      __builtin_amdgcn_wave_barrier();
    }
  }
  __syncthreads();
  if (blockIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = threadIdx.x + i * 256;
      Xs[(size_t)(j0 + (e >> 4)) * 64 + qoff + (e & 15)] = X[(e >> 4) * XP + (e & 15)];
    }
  }
  if (!upd) return;
  // L_ij takes the place of the diagonal block (zero beyond the matrix)
#pragma unroll
  for (int i = 0; i < NB * NB / 256; ++i) {
    const int e = threadIdx.x + i * 256;
    const int r = e / NB, c = e % NB;
    Ld[r * LDP + c] = (r < ib && c < jb) ? lo[i] : 0.0;
  }
  __syncthreads();
  d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < 16; ++s) acc = mfma(Ld[(16 * wave + m) * LDP + 4 * s + kq], X[(4 * s + kq) * XP + m], acc);
#pragma unroll
  for (int r = 0; r < 4; ++r) Z[(size_t)(i0 + 16 * wave + kq + 4 * r) * 64 + qoff + m] -= acc[r];
}

// Backward step of block j0 (from the last block to the first): L_jj^T X = Xs_j, result into Z;
// workgroup x takes Xs_c -= L[j, c]^T X for the column block c = x (< j).
__global__ void __launch_bounds__(256)
k_trsm_bwd(const double *__restrict__ L, int p, int j0, const double *__restrict__ Iinv,
           double *__restrict__ Xs, double *__restrict__ Z) {
  __shared__ double Ld[NB * LDP];
  __shared__ double Iv[4 * 256];
  __shared__ double X[NB * XP];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = lane & 15, kq = lane >> 4;
  const int jb = min(NB, p - j0);
  const int qoff = 16 * (int)blockIdx.y;
  const int c0 = NB * (int)blockIdx.x;
  const bool upd = c0 < j0;
  double lo[NB * NB / 256];
  if (upd) {
#pragma unroll
    for (int i = 0; i < NB * NB / 256; ++i) {
      const int e = threadIdx.x + i * 256;
      lo[i] = L[(size_t)(j0 + min(e / NB, jb - 1)) * p + c0 + e % NB];
    }
  }
  trsm_stage(L, p, j0, jb, Iinv, Xs, qoff, Ld, Iv, X);
  __syncthreads();
  if (wave == 0) {  // X_b = inv(L_bb)^T (Z_b - sum_{c > b} L_cb^T X_c)
#pragma unroll
    for (int b = 3; b >= 0; --b) {
      d4 acc = d4{0.0, 0.0, 0.0, 0.0};
      for (int c = b + 1; c < 4; ++c)
#pragma unroll
        for (int s = 0; s < 4; ++s)
          acc = mfma(Ld[(16 * c + 4 * s + kq) * LDP + 16 * b + m], X[(16 * c + 4 * s + kq) * XP + m], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) X[(16 * b + kq + 4 * r) * XP + m] -= acc[r];
      __builtin_amdgcn_wave_barrier();
      d4 xb = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4; ++s)
        xb = mfma(Iv[b * 256 + (4 * s + kq) * 16 + m], X[(16 * b + 4 * s + kq) * XP + m], xb);
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int r = 0; r < 4; ++r) X[(16 * b + kq + 4 * r) * XP + m] = xb[r];
      __builtin_amdgcn_wave_barrier();
    }
  }
  __syncthreads();
  if (blockIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = threadIdx.x + i * 256;
      Z[(size_t)(j0 + (e >> 4)) * 64 + qoff + (e & 15)] = X[(e >> 4) * XP + (e & 15)];
    }
  }
  if (!upd) return;
#pragma unroll
  for (int i = 0; i < NB * NB / 256; ++i) {
    const int e = threadIdx.x + i * 256;
    const int r = e / NB, c = e % NB;
    Ld[r * LDP + c] = r < jb ? lo[i] : 0.0;
  }
  __syncthreads();
  d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < 16; ++s) acc = mfma(Ld[(4 * s + kq) * LDP + 16 * wave + m], X[(4 * s + kq) * XP + m], acc);
#pragma unroll
  for (int r = 0; r < 4; ++r) Xs[(size_t)(c0 + 16 * wave + kq + 4 * r) * 64 + qoff + m] -= acc[r];
}

// ---- fused predictor for several responses ------------------------------------------------------
// 8 waves per 64-row tile.  Basis as in k_predict (lane = row).  Contraction: wave = (row group
// of 16, half of the 4-term steps); a lane forms the product of its (row, term) -- the A operand --
// and reads its (term, response) of the term-major copy of Theta -- the B operand.
constexpr int kPmThreads = 512, kPmWaves = kPmThreads / 64;

template <int NQB>
__global__ void __launch_bounds__(kPmThreads)
k_predict_multi(const DimDesc *__restrict__ dims, const double *__restrict__ ka,
                const double *__restrict__ kb, const double *__restrict__ kc,
                const double *__restrict__ rot, const double *__restrict__ tab,
                const int *__restrict__ cpos, int d, int Mu, int tile_doubles,
                const uint32_t *__restrict__ colsw, int W2, int p,
                const double *__restrict__ ThT /* [p][16 NQB] */, int qc, const double *__restrict__ x,
                uint64_t n, double *__restrict__ mean, uint64_t ldm) {
  extern __shared__ double lds[];
  constexpr int QW = 16 * NQB;
  double *reds = lds + tile_doubles;            // [8][64] scale partials
  double *scl = reds + kPmWaves * kTileRows;    // [64] basescale of the rows
  double *red = scl + kTileRows;                // [4][NQB][256] partials of the second half
  double *obuf = lds;                           // [QW][64] results, over the tile once it is spent
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t row0 = (uint64_t)blockIdx.x * kTileRows;
  {
    const uint64_t row = row0 + lane;
    const bool valid = row < n;
    const StoreTile<kTileRows> store{lds, cpos, lane, Mu};
    build_tile<kPmWaves, false>(dims, ka, kb, kc, rot, tab, nullptr, d, x, n, row, valid, wave, store, reds);
  }
  __syncthreads();
  if (wave == 0) scl[lane] = tile_scale<kPmWaves>(reds, lane);
  const int m = lane & 15, kq = lane >> 4;
  const int rg = wave & 3, half = wave >> 2;
  const int trow = 16 * rg + m;
  d4 acc[NQB];
#pragma unroll
  for (int j = 0; j < NQB; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
  const int nsteps = (p + 3) / 4;
  for (int s = half; s < nsteps; s += 2) {
    const int k = 4 * s + kq;
    const bool ok = k < p;
    const int kk = min(k, p - 1);
    double pr = ok ? 1.0 : 0.0;
    const uint32_t *cw = colsw + (size_t)kk * W2;
    for (int w = 0; w < W2; ++w) {
      const uint32_t c = cw[w];
      pr *= lds[(c & 0xffffu) * kTileRows + trow];
      pr *= lds[(c >> 16) * kTileRows + trow];
    }
#pragma unroll
    for (int j = 0; j < NQB; ++j) acc[j] = mfma(pr, ThT[(size_t)kk * QW + 16 * j + m], acc[j]);
  }
  if (half == 1) {
#pragma unroll
    for (int j = 0; j < NQB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(rg * NQB + j) * 256 + 4 * lane + r] = acc[j][r];
  }
  __syncthreads();  // the tile is spent: obuf may take its place
  if (half == 0) {
#pragma unroll
    for (int j = 0; j < NQB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int orow = 16 * rg + kq + 4 * r;
        obuf[(16 * j + m) * kTileRows + orow] = (acc[j][r] + red[(rg * NQB + j) * 256 + 4 * lane + r]) * scl[orow];
      }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < QW * kTileRows; e += kPmThreads) {
    const int j = e >> 6, r = e & 63;
    if (j < qc && row0 + r < n) mean[(uint64_t)j * ldm + row0 + r] = obuf[e];
  }
}

size_t predict_multi_lds(uint64_t Mu, int nqb, int *tile_doubles) {
  const size_t tile = std::max<size_t>(Mu * kTileRows, (size_t)16 * nqb * kTileRows);
  *tile_doubles = (int)tile;
  return (tile + kPmWaves * kTileRows + kTileRows + (size_t)4 * nqb * 256) * sizeof(double);
}

template <int NQB>
int run_predict_multi(const obhip_model &m, obhip_terms &t, const double *d_ThT, int qc, const double *d_x,
                      uint64_t n, double *d_mean, uint64_t ldm) {
  int tile = 0;
  const size_t lds = predict_multi_lds(t.Mu, NQB, &tile);
  OB_TRY(ensure_dyn_lds((const void *)k_predict_multi<NQB>, lds));
  launch_pred<false>(k_predict_multi<NQB>, dim3((unsigned)((n + kTileRows - 1) / kTileRows)), dim3(kPmThreads), lds,
                     pred_tabs(m, t), tile, (const uint32_t *)t.cols.p, (int)(t.W / 2), (int)t.p, d_ThT, qc, d_x, n,
                     d_mean, ldm);
  OB_HIP(hipGetLastError());
  return 0;
}

template <int NQB>
int run_aty(const double *B, uint64_t ldb, uint64_t n, const double *Y, uint64_t ldy, int qc, uint64_t rows_per,
            int nsplit, double *part) {
  hipLaunchKernelGGL(k_aty_multi<NQB>, dim3((unsigned)((ldb + 255) / 256), (unsigned)nsplit), dim3(256), 0,
                     cur_stream(), B, ldb, n, Y, ldy, qc, rows_per, part);
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace

// columns of one pass of the batched kernels
constexpr uint64_t kMultiChunk = 64;

uint64_t multi_solve_scratch_bytes(uint64_t p) {
  return 2 * ((p + NB - 1) / NB * NB) * kMultiChunk * sizeof(double);
}

// d_out (p x q, column-major, leading dimension ldo) = B^T Y from the staged design matrix of
// (b, t), which the caller has made sure is resident -- in the terms' own column order or in their Gram order
// (obhip_basis::bmat_order), whose sums the reduction scatters to their terms: no second staging, and no pass
// over the basis per response
int launch_aty_multi(obhip_basis &b, const obhip_terms &t, const double *d_Y, uint64_t ldy, uint64_t q,
                     double *d_out, uint64_t ldo) {
  const uint32_t *perm = b.bmat_order != 0 && b.bmat_order == t.order.serial ? t.order.perm_dev.p : nullptr;
  if (b.bmat_order != 0 && !perm) return fail(OBHIP_ERR_INVALID, "aty_multi: the staged matrix is in another order");
  ProfScope ps("aty_multi");
  const uint64_t ldb = t.p_pad, n = b.n;
  const int ncu = device_cus(b.device);
  const uint64_t gx = (ldb + 255) / 256;
  for (uint64_t q0 = 0; q0 < q; q0 += kMultiChunk) {
    const int qc = (int)std::min(kMultiChunk, q - q0);
    const int nqb = qc <= 16 ? 1 : (qc <= 32 ? 2 : 4);
    // enough row ranges to fill the GPU four times over, of at least 256 rows each
    uint64_t nsplit = std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (4 * (uint64_t)ncu + gx - 1) / gx));
    const uint64_t rows_per = std::max<uint64_t>(4, ((n + nsplit - 1) / nsplit + 3) / 4 * 4);
    nsplit = std::max<uint64_t>(1, (n + rows_per - 1) / rows_per);
    void *part = nullptr;
    OB_TRY(b.workspace(nsplit * 16 * nqb * ldb * sizeof(double), &part));
    const double *Yc = d_Y + q0 * ldy;
    if (nqb == 1) OB_TRY(run_aty<1>(b.bmat.p, ldb, n, Yc, ldy, qc, rows_per, (int)nsplit, (double *)part));
    if (nqb == 2) OB_TRY(run_aty<2>(b.bmat.p, ldb, n, Yc, ldy, qc, rows_per, (int)nsplit, (double *)part));
    if (nqb == 4) OB_TRY(run_aty<4>(b.bmat.p, ldb, n, Yc, ldy, qc, rows_per, (int)nsplit, (double *)part));
    hipLaunchKernelGGL(k_aty_reduce, dim3((unsigned)((t.p + 255) / 256), (unsigned)qc), dim3(256), 0, cur_stream(),
                       (const double *)part, (int)nsplit, 16 * nqb, ldb, (int)t.p, qc, d_out + q0 * ldo, ldo, perm);
    OB_HIP(hipGetLastError());
  }
  return 0;
}

// d_Theta (p x q, leading dimension p) = inv(L L^T) (e2 d_R), L the factor launch_newton_solve left
// in the lower triangle of d_L (row-major) and d_Iinv the 16 x 16 inverses in its workspace
int launch_trsm_multi(uint64_t p64, const double *d_L, const double *d_Iinv, const double *d_R, uint64_t ldr,
                      uint64_t q, double e2, double *d_Theta, void *d_scratch) {
  if (q == 0) return 0;
  ProfScope ps("trsm_multi");
  const int p = (int)p64, pp = (p + NB - 1) / NB * NB, nblk = pp / NB;
  double *Z = (double *)d_scratch, *Xs = Z + (size_t)pp * kMultiChunk;
  hipStream_t st = cur_stream();
  for (uint64_t q0 = 0; q0 < q; q0 += kMultiChunk) {
    const int qc = (int)std::min(kMultiChunk, q - q0);
    const unsigned nqb = (unsigned)(qc + 15) / 16;
    hipLaunchKernelGGL(k_trsm_load, dim3((unsigned)(pp * 64 + 255) / 256), dim3(256), 0, st, d_R + q0 * ldr, ldr, p,
                       pp, qc, e2, Z);
    for (int jb = 0; jb < nblk; ++jb)
      hipLaunchKernelGGL(k_trsm_fwd, dim3((unsigned)std::max(1, nblk - 1 - jb), nqb), dim3(256), 0, st, d_L, p,
                         jb * NB, d_Iinv, Z, Xs);
    for (int jb = nblk - 1; jb >= 0; --jb)
      hipLaunchKernelGGL(k_trsm_bwd, dim3((unsigned)std::max(1, jb), nqb), dim3(256), 0, st, d_L, p, jb * NB,
                         d_Iinv, Xs, Z);
    hipLaunchKernelGGL(k_trsm_store, dim3((unsigned)(((size_t)p * qc + 255) / 256)), dim3(256), 0, st,
                       (const double *)Z, p, qc, d_Theta + q0 * p64, p64);
    OB_HIP(hipGetLastError());
  }
  return 0;
}

// The fused kernel holds the Mu used basis columns of a 64-row tile in LDS and reads the terms'
// column lists from HBM: any number of factors per term, Mu bounded by the 160 KB of LDS.
bool predict_multi_supports(const obhip_terms &t) {
  int tile = 0;
  return t.W >= 2 && t.W % 2 == 0 && predict_multi_lds(t.Mu, 1, &tile) <= kLdsBudget && !getenv("OBHIP_FORCE_GENERIC");
}

int launch_theta_term_major(const double *d_Theta, uint64_t p, int qc, uint64_t qw, double *d_T) {
  return vmap(p * qw, [=] __device__(uint64_t i) {
    const uint64_t k = i / qw, j = i % qw;
    d_T[i] = j < (uint64_t)qc ? d_Theta[j * p + k] : 0.0;
  });
}

// d_mean (n x q, leading dimension n): column j = B(x) Theta[:, j]; the terms are prepared
int launch_predict_multi(const obhip_model &m, obhip_terms &t, const double *d_Theta, uint64_t q,
                         const double *d_x, uint64_t n, double *d_mean) {
  ProfScope ps("predict_multi");
  const uint64_t p = t.p;
  int tile = 0;
  int nqb_max = 4;
  while (nqb_max > 1 && predict_multi_lds(t.Mu, nqb_max, &tile) > kLdsBudget) nqb_max /= 2;
  DevBuf<double> tht;
  OB_TRY(tht.alloc(p * 16 * nqb_max));
  for (uint64_t q0 = 0; q0 < q; q0 += 16 * (uint64_t)nqb_max) {
    const int qc = (int)std::min<uint64_t>(16 * (uint64_t)nqb_max, q - q0);
    int nqb = 1;
    while (16 * nqb < qc) nqb *= 2;
    OB_TRY(launch_theta_term_major(d_Theta + q0 * p, p, qc, 16 * (uint64_t)nqb, tht.p));
    double *out = d_mean + q0 * n;
    if (nqb == 1) OB_TRY(run_predict_multi<1>(m, t, tht.p, qc, d_x, n, out, n));
    if (nqb == 2) OB_TRY(run_predict_multi<2>(m, t, tht.p, qc, d_x, n, out, n));
    if (nqb == 4) OB_TRY(run_predict_multi<4>(m, t, tht.p, qc, d_x, n, out, n));
  }
  return 0;
}

}  // namespace obhip
