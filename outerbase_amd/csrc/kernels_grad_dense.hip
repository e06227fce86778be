// The dense pass of the transposed hyper-gradient products (tprodmmge_ / dotmultgesub_,
// src/linalg.cpp:362-471): D[h][k] = sum_i a_i ge[h, 0]_i B_ik, every term as if it lacked h's dimension,
// all hyper-parameters at once, in two forms (k_tmm_ge0 / k_tmm_ge0_db and k_bt_times_u below).  Which one
// runs, and what corrects the terms that do have the dimension: grad_plan in kernels_grad.hip.
#include "obhip_internal.h"
#include "device_common.h"

namespace obhip {

namespace {

// ---- transposed products: the dense part of every hyper-parameter in one streaming pass ---------
// out_gradhyp[k, h] = sum_i w_i dB_ik/dhyp_h.  For the terms WITHOUT hyper-parameter h's
// dimension that is sum_i (w_i ge[h, 0]_i) B_ik: a tall-skinny product of the materialised
// row-major design matrix (obhip_basis::bmat, as the Gram kernel uses it) with an n x nhyp
// weight matrix -- one pass over B for all hyper-parameters, HBM-bound.  The terms that do
// have the dimension are recomputed by k_tmm on a view restricted to them (grad_view_restricted).
// Thread = 4 consecutive terms x NH hyper-parameters; the row weights sit in lane registers
// (lane = row of the 64-row tile) and are broadcast with v_readlane.  SQ: squared stores
// (B^2; the level-0 gradient column of the squared store is 2 ge[h, 0]).
constexpr int kNHB = 20;  // hyper-parameters per pass

template <bool SQ>
__global__ void __launch_bounds__(512)
k_bt_times_u(const double *__restrict__ Bmat, uint64_t p_pad, const double *__restrict__ gtile,
             uint64_t Mtot, const int *__restrict__ ge0abs, int nhyp, int h0,
             const double *__restrict__ a, uint64_t n, uint64_t ntiles, uint64_t tiles_per_split,
             double *__restrict__ part) {
  const int tid = threadIdx.x, lane = tid & 63;
  const uint64_t k4 = (uint64_t)blockIdx.y * 2048 + (uint64_t)tid * 4;
  if (k4 >= p_pad) return;
  const uint64_t t0 = (uint64_t)blockIdx.x * tiles_per_split;
  const uint64_t t1 = min(ntiles, t0 + tiles_per_split);
  double acc[4][kNHB];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int h = 0; h < kNHB; ++h) acc[q][h] = 0.0;
  int gcol[kNHB];
#pragma unroll
  for (int h = 0; h < kNHB; ++h) gcol[h] = h0 + h < nhyp ? ge0abs[h0 + h] : -1;
  for (uint64_t tile = t0; tile < t1; ++tile) {
    const uint64_t row = tile * kTileRows + lane;
    const double av = row < n ? a[row] : 0.0;
    double uw[kNHB];
#pragma unroll
    for (int h = 0; h < kNHB; ++h)
      uw[h] = gcol[h] >= 0 ? av * gtile[(tile * Mtot + (uint64_t)gcol[h]) * kTileRows + lane] : 0.0;
    const double *brow = Bmat + tile * kTileRows * p_pad + k4;
#pragma unroll 4
    for (int r = 0; r < kTileRows; ++r) {
      const double4 v4 = *(const double4 *)(brow + (uint64_t)r * p_pad);
      double v[4] = {v4.x, v4.y, v4.z, v4.w};
      if (SQ) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] *= v[q];
      }
#pragma unroll
      for (int h = 0; h < kNHB; ++h) {
        const double wh = readlane_f64(uw[h], r);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q][h] = fma(v[q], wh, acc[q][h]);
      }
    }
  }
#pragma unroll
  for (int h = 0; h < kNHB; ++h)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      part[((uint64_t)blockIdx.x * kNHB + h) * p_pad + k4 + q] = acc[q][h];
}

// ---- the same dense part without the design matrix: products on the fly, MFMA contraction ------
// D[h][k] = sum_i (a_i s_i ge[h, 0]_i) P_k(i) is a (hyper-parameters x rows) x (rows x terms)
// product whose right factor never exists: with lane = (term t16 = l & 15, row r4 = l >> 4) a
// lane's term product at rows 4 s + r4 IS the B operand element B[k = r4][j = t16] of
// v_mfma_f64_16x16x4_f64, and the weight column of hyper-parameter t16 read at the same rows
// is the A operand element A[i = t16][k = r4].  Column addresses are loop-invariant per lane
// as in the term-per-lane kernels (the step is the immediate offset), so a (term, row) costs
// its WE column reads, WE - 1 multiplies and 1/64 of an MFMA per 16 hyper-parameters.  The
// weights (staged behind the tile's columns, premultiplied by a and the basescale) go through
// the same in-order LDS queue one step ahead; every s_waitcnt counts the reads behind its
// target exactly (ge_newer_*).  A wave holds 4 groups of 16 terms, a block 512 terms.
typedef double ge_d4 __attribute__((ext_vector_type(4)));
constexpr int kGeNU = 4, kGeSteps = 16, kGeInflight = 8;

// SQF: the unit's product is squared before it enters the MFMA (the squared stores' products are
// the squares of the plain ones: the double-buffered kernel stages the raw columns by LDS-direct loads)
// N4: further groups of FOUR hyper-parameters on v_mfma_f64_4x4x4_4b_f64 (a quarter of the matrix-pipe
// time of a 16-block: 20 hyper-parameters cost 1.25 blocks instead of 2).  There the product is the A
// operand -- lane (block (l >> 2) & 3, i = l & 3, k = l >> 4) holds A_blk[i][k], which IS term
// t16 = l & 15 at row r4 = l >> 4 -- and the weight of hyper-parameter l & 3 at the same row the B
// operand B_blk[k][j = l & 3], the same in all four blocks; D_blk[i][j] lands in lane (i = l >> 4,
// blk, j = l & 3): term 4 blk + (l >> 4), hyper-parameter l & 3.
template <int WE, int W, int NHB, bool SQF = false, int N4 = 0>
struct GePipe {
  static constexpr int NU = kGeNU, TOT = kGeSteps * kGeNU, NWT = NHB + N4;
  static constexpr int D = (kGeInflight / WE) > 0 ? kGeInflight / WE : 1;
  // units issued once step U has issued (the prologue issues units 0 .. D-2)
  static constexpr int issued(int U) { return U + D < TOT ? U + D : TOT; }
  static constexpr bool wnext(int s) { return s + 1 < kGeSteps; }  // weights of step s+1 exist
  // LDS reads queued behind the weights of step s when step s waits for them
  static constexpr int newer_w(int s) {
    const int units = s == 0 ? issued(0) : issued(s * NU) - issued((s - 1) * NU);
    const int v = units * WE + (wnext(s) ? NWT : 0);
    return v < 15 ? v : 15;
  }
  // LDS reads queued behind the reads of unit U when step U waits for them
  static constexpr int newer_u(int U) {
    const int units = (TOT - 1 - U) < (D - 1) ? (TOT - 1 - U) : (D - 1);
    int wr = 0;
    for (int S = (U - D + 1 > 0 ? U - D + 1 : 0); S <= U; ++S)
      if (S % NU == 0 && wnext(S / NU)) wr += NWT;
    const int v = units * WE + wr;
    return v < 15 ? v : 15;
  }

  template <int U, typename C>
  static __device__ __forceinline__ void issue(C &c, double (&buf)[12]) {
    constexpr int st = U / NU, unit = U % NU, s = (U % D) * WE;
#pragma unroll
    for (int j = 0; j < WE; ++j) buf[s + j] = tl_rd<st * 32>(c.ad[unit][W - WE + j]);
  }
  template <int S, typename C>
  static __device__ __forceinline__ void issue_w(C &c, double (&w)[12]) {
#pragma unroll
    for (int hb = 0; hb < NHB; ++hb) w[(S % 2) * NWT + hb] = tl_rd<S * 32>(c.aw[hb]);
    if constexpr (N4 > 0) {
#pragma unroll
      for (int q = 0; q < N4; ++q) w[(S % 2) * NWT + NHB + q] = tl_rd<S * 32>(c.aw4[q]);
    }
  }
  template <int U, typename C>
  static __device__ __forceinline__ void steps(C &c, double (&buf)[12], double (&w)[12]) {
    if constexpr (U < TOT) {
      constexpr int st = U / NU, unit = U % NU, s = (U % D) * WE;
      if constexpr (U + D - 1 < TOT) issue<U + D - 1>(c, buf);
      if constexpr (unit == 0) {
        if constexpr (wnext(st)) issue_w<st + 1>(c, w);
        tl_waitn<newer_w(st), NWT, (st % 2) * NWT>(w);
      }
      tl_waitn<newer_u(U), WE, s>(buf);
      double v = buf[s];
#pragma unroll
      for (int j = 1; j < WE; ++j) v *= buf[s + j];
      if constexpr (SQF) v = v * v;
#pragma unroll
      for (int hb = 0; hb < NHB; ++hb)
        c.acc[unit][hb] = __builtin_amdgcn_mfma_f64_16x16x4f64(w[(st % 2) * NWT + hb], v,
                                                               c.acc[unit][hb], 0, 0, 0);
      if constexpr (N4 > 0) {
#pragma unroll
        for (int q = 0; q < N4; ++q)
          c.acc4[unit][q] =
              __builtin_amdgcn_mfma_f64_4x4x4f64(v, w[(st % 2) * NWT + NHB + q], c.acc4[unit][q], 0, 0, 0);
      }
      steps<U + 1>(c, buf, w);
    }
  }
  template <int U, typename C>
  static __device__ __forceinline__ void prologue(C &c, double (&buf)[12]) {
    if constexpr (U < D - 1 && U < TOT) {
      issue<U>(c, buf);
      prologue<U + 1>(c, buf);
    }
  }
  template <typename C>
  static __device__ __forceinline__ void run(C &c) {
    double buf[12], w[12];
    issue_w<0>(c, w);
    prologue<0>(c, buf);
    steps<0>(c, buf, w);
  }
};

template <int W, int NHB, int N4 = 0>
struct GeCtx {
  uint32_t ad[kGeNU][W];
  uint32_t aw[NHB > 0 ? NHB : 1];
  ge_d4 acc[kGeNU][NHB > 0 ? NHB : 1];
  uint32_t aw4[N4 > 0 ? N4 : 1];
  double acc4[kGeNU][N4 > 0 ? N4 : 1];
};

template <int W, int NHB, bool SQF = false, int N4 = 0>
__device__ __forceinline__ void ge_tile(GeCtx<W, NHB, N4> &c, int we) {
  if (we == W) {
    GePipe<W, W, NHB, SQF, N4>::run(c);
  } else if (we == W - 1) {
    GePipe<W - 1, W, NHB, SQF, N4>::run(c);
  } else if (W >= 3 && we == W - 2) {
    GePipe<(W >= 3 ? W - 2 : 1), W, NHB, SQF, N4>::run(c);
  } else {
    GePipe<(W >= 4 ? W - 3 : 1), W, NHB, SQF, N4>::run(c);
  }
}

// NW: waves per block (16 where the tile leaves room for only one block per CU)
template <int W2, int NHB, bool SQ, int NW>
__global__ void __launch_bounds__(NW * 64, 4)
k_tmm_ge0(const double *__restrict__ bm, const double *__restrict__ scale,
          const uint32_t *__restrict__ ucol, int Mu, uint64_t Mtot,
          const uint32_t *__restrict__ colsw, const uint32_t *__restrict__ sperm,
          const int *__restrict__ ge0abs, int nhyp, int h0, const double *__restrict__ a, uint64_t n,
          uint64_t ntiles, uint64_t tiles_per_split, uint64_t p_pad, double *__restrict__ part) {
  extern __shared__ double lds[];
  constexpr int W = 2 * W2, HS = 16 * NHB;
  const int lane = threadIdx.x & 63, t16 = lane & 15, r4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t t0 = (uint64_t)blockIdx.x * tiles_per_split;
  const uint64_t t1 = min(ntiles, t0 + tiles_per_split);

  // my terms: slots (blockIdx.y * 8 + wave) * 64 + g * 16 + t16 of the sorted order
  GeCtx<W, NHB> c;
  int nzmax = 1;
#pragma unroll
  for (int g = 0; g < kGeNU; ++g) {
    const uint64_t slot = ((uint64_t)blockIdx.y * NW + wave) * 64 + g * 16 + t16;
    const bool ok = slot < p_pad;
    const uint64_t k = ok ? sperm[slot] : 0;
    uint32_t cw[W2];
#pragma unroll
    for (int w = 0; w < W2; ++w) {
      cw[w] = ok ? colsw[k * W2 + w] : 0u;  // column 0 = ones
      c.ad[g][2 * w] = (cw[w] & 0xffffu) * (kTlPitch * 8) + r4 * 8;
      c.ad[g][2 * w + 1] = (cw[w] >> 16) * (kTlPitch * 8) + r4 * 8;
    }
    nzmax = max(nzmax, tl_nnz<W2>(cw));
#pragma unroll
    for (int hb = 0; hb < NHB; ++hb) c.acc[g][hb] = ge_d4{0.0, 0.0, 0.0, 0.0};
  }
#pragma unroll
  for (int hb = 0; hb < NHB; ++hb) c.aw[hb] = (uint32_t)(Mu + hb * 16 + t16) * (kTlPitch * 8) + r4 * 8;
  const int we = tl_variant<W>(wave_max_i32(nzmax));
  const bool live = ((uint64_t)blockIdx.y * NW + wave) * 64 < p_pad;

  for (uint64_t tile = t0; tile < t1; ++tile) {
    __syncthreads();  // every wave is done with the previous tile
    {
      const double *src = bm + tile * Mtot * kTileRows + lane;
      // SQ: the squared stores formed while staging (basematsq = basemat^2, its level-0 gradient
      // column 2 ge[h, 0], scale^2: k_square_gradbasis) -- no second copy of the gradient basis
      for (int u = wave; u < Mu; u += NW) {
        const double v = src[(size_t)ucol[u] * kTileRows];
        lds[u * kTlPitch + lane] = SQ ? v * v : v;
      }
      const uint64_t row = tile * kTileRows + lane;
      double wr = 0.0;
      if (row < n) {
        const double sc = scale[row];
        wr = a[row] * (SQ ? sc * sc : sc);
      }
      for (int h = wave; h < HS; h += NW) {
        const int col = h0 + h < nhyp ? ge0abs[h0 + h] : -1;
        double gv = col >= 0 ? src[(size_t)col * kTileRows] : 0.0;
        if (SQ) gv = 2.0 * gv;
        lds[(Mu + h) * kTlPitch + lane] = col >= 0 ? wr * gv : 0.0;
      }
    }
    __syncthreads();
    if (live) ge_tile<W, NHB>(c, we);
  }
  // C/D layout of v_mfma_f64_16x16x4_f64: column (term) = lane & 15, row (hyper-parameter) =
  // (lane >> 4) + 4 * reg
#pragma unroll
  for (int g = 0; g < kGeNU; ++g) {
    const uint64_t slot = ((uint64_t)blockIdx.y * NW + wave) * 64 + g * 16 + t16;
    if (slot >= p_pad) continue;
    const uint64_t k = sperm[slot];
#pragma unroll
    for (int hb = 0; hb < NHB; ++hb)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        part[((uint64_t)blockIdx.x * HS + hb * 16 + r4 + 4 * v) * p_pad + k] = c.acc[g][hb][v];
  }
}

// The same with the NEXT tile on its way while this one is worked on: two tile buffers, one block of
// 16 waves per CU, the value columns fetched by LDS-direct loads (global_load_lds_dword as in k_hm2:
// no staging registers -- the kernel sits at 104-128 VGPRs -- and no ds_write), the 16 weight
// columns (one per wave) through two registers.  The columns arrive raw, so the squared stores'
// products are formed as squares of the plain products (GePipe<SQF>).  k_tmm_ge0 above loads its
// tile between two barriers: with two blocks per CU one computes while the other loads, but at a
// few microseconds of compute per tile the matrix pipe still idled half of the time.
// N4: hyper-parameters h0 + 16 .. h0 + 16 + 4 N4 ride along in groups of four (GePipe); NHB = 0:
// groups of four only (the last 1 to 8 hyper-parameters in a pass of their own, whose matrix
// instructions take a quarter or half of a 16-block's time).
template <int W2, bool SQ, int N4, int NHB = 1>
__global__ void __launch_bounds__(1024, 4)
k_tmm_ge0_db(const double *__restrict__ bm, const double *__restrict__ scale,
             const uint32_t *__restrict__ ucol, int Mu, uint64_t Mtot,
             const uint32_t *__restrict__ colsw, const uint32_t *__restrict__ sperm,
             const int *__restrict__ ge0abs, int nhyp, int h0, const double *__restrict__ a, uint64_t n,
             uint64_t ntiles, uint64_t tiles_per_split, uint64_t p_pad, double *__restrict__ part) {
  extern __shared__ double lds[];
  constexpr int W = 2 * W2, H16 = 16 * NHB, HS = H16 + 4 * N4, NW = 16;
  static_assert(NHB <= 1 && HS <= 24 && HS >= 4, "");
  const int lane = threadIdx.x & 63, t16 = lane & 15, r4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t t0 = (uint64_t)blockIdx.x * tiles_per_split;
  const uint64_t t1 = min(ntiles, t0 + tiles_per_split);
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) double *)lds;
  const uint32_t tile_bytes = (uint32_t)(Mu + HS) * (kTlPitch * 8);

  GeCtx<W, NHB, N4> c;
  int nzmax = 1;
#pragma unroll
  for (int g = 0; g < kGeNU; ++g) {
    const uint64_t slot = ((uint64_t)blockIdx.y * NW + wave) * 64 + g * 16 + t16;
    const bool ok = slot < p_pad;
    const uint64_t k = ok ? sperm[slot] : 0;
    uint32_t cw[W2];
#pragma unroll
    for (int w = 0; w < W2; ++w) {
      cw[w] = ok ? colsw[k * W2 + w] : 0u;  // column 0 = ones
      c.ad[g][2 * w] = lds0 + (cw[w] & 0xffffu) * (kTlPitch * 8) + r4 * 8;
      c.ad[g][2 * w + 1] = lds0 + (cw[w] >> 16) * (kTlPitch * 8) + r4 * 8;
    }
    nzmax = max(nzmax, tl_nnz<W2>(cw));
    c.acc[g][0] = ge_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < (N4 > 0 ? N4 : 1); ++q) c.acc4[g][q] = 0.0;
  }
  c.aw[0] = lds0 + (uint32_t)(Mu + t16) * (kTlPitch * 8) + r4 * 8;
#pragma unroll
  for (int q = 0; q < (N4 > 0 ? N4 : 1); ++q)
    c.aw4[q] = lds0 + (uint32_t)(Mu + H16 + 4 * q + (lane & 3)) * (kTlPitch * 8) + r4 * 8;
  const int we = tl_variant<W>(wave_max_i32(nzmax));
  const bool live = ((uint64_t)blockIdx.y * NW + wave) * 64 < p_pad;
  // wave h stages weight column h: a s (SQ: a s^2) times ge[h, 0] (SQ: 2 ge[h, 0]) of the row = lane
  // (the first waves a second one, column 16 + h, where groups of four ride along with a 16-block)
  constexpr bool kSecond = NHB > 0 && N4 > 0;
  const int wcol = (wave < HS && h0 + wave < nhyp) ? ge0abs[h0 + wave] : -1;
  const int wcol2 = (kSecond && wave < 4 * N4 && h0 + 16 + wave < nhyp) ? ge0abs[h0 + 16 + wave] : -1;

  // next tile -> the other buffer.  (The weight column's two loads are requested BEFORE the
  // LDS-direct loads and used at the top of the next tile: the compiler's vmcnt bookkeeping does
  // not see the inline-asm loads, a use right here would wait for all of them.)
  double gvn = 0.0, wrn = 0.0, gvn2 = 0.0;
  auto prefetch = [&](uint64_t tile, int bsel) {
    const char *tb = (const char *)(bm + tile * Mtot * kTileRows);
    const uint64_t row = tile * kTileRows + lane;
    gvn = wrn = gvn2 = 0.0;
    if (row < n && wcol >= 0) {
      const double sc = scale[row];
      wrn = a[row] * (SQ ? sc * sc : sc);
      gvn = ((const double *)tb)[(size_t)wcol * kTileRows + lane];
      if (kSecond && wcol2 >= 0) gvn2 = ((const double *)tb)[(size_t)wcol2 * kTileRows + lane];
    }
    const uint32_t l0 = lds0 + (bsel ? tile_bytes : 0u);
    for (int u = wave; u < Mu; u += NW) {
      const uint32_t col = __builtin_amdgcn_readfirstlane(ucol[u]);
      const uint64_t ga = (uint64_t)(tb + (size_t)col * (kTileRows * 8));
      const uint64_t gu = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(ga >> 32)) << 32) |
                          (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)ga);
      const uint32_t ld = (uint32_t)__builtin_amdgcn_readfirstlane((int)(l0 + (uint32_t)u * (kTlPitch * 8)));
// m0 is written here: on the clobber list so that the compiler never assumes a value of its own
// survives the statement (round-4 advice; m0 is a reserved register, hence the diagnostic)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
      asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1\n\t"
                   "global_load_lds_dword %0, %1 offset:256"
                   :: "v"((uint32_t)lane * 4u), "s"((const char *)gu), "s"(ld) : "memory", "m0");
#pragma clang diagnostic pop
    }
  };
  if (t0 < t1) prefetch(t0, 0);

  for (uint64_t tile = t0; tile < t1; ++tile) {
    const int bsel = (int)((tile - t0) & 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's share of the tile has landed
    if (wave < HS)
      lds[(bsel ? tile_bytes / 8 : 0) + (Mu + wave) * kTlPitch + lane] = wrn * (SQ ? 2.0 * gvn : gvn);
    if (kSecond && wave < 4 * N4)
      lds[(bsel ? tile_bytes / 8 : 0) + (Mu + 16 + wave) * kTlPitch + lane] = wrn * (SQ ? 2.0 * gvn2 : gvn2);
    __syncthreads();  // tile and weights complete; every wave is done with the other buffer
    if (tile + 1 < t1) prefetch(tile + 1, bsel ^ 1);
    if (live) ge_tile<W, NHB, SQ, N4>(c, we);
    // on to the other buffer
    const uint32_t delta = bsel ? 0u - tile_bytes : tile_bytes;
#pragma unroll
    for (int g = 0; g < kGeNU; ++g)
#pragma unroll
      for (int j = 0; j < W; ++j) {
        c.ad[g][j] += delta;
        asm volatile("" : "+v"(c.ad[g][j]));
      }
    c.aw[0] += delta;
    asm volatile("" : "+v"(c.aw[0]));
    if constexpr (N4 > 0) {
#pragma unroll
      for (int q = 0; q < N4; ++q) {
        c.aw4[q] += delta;
        asm volatile("" : "+v"(c.aw4[q]));
      }
    }
  }
#pragma unroll
  for (int g = 0; g < kGeNU; ++g) {
    const uint64_t slot = ((uint64_t)blockIdx.y * NW + wave) * 64 + g * 16 + t16;
    if (NHB > 0 && slot < p_pad) {
      const uint64_t k = sperm[slot];
#pragma unroll
      for (int v = 0; v < 4; ++v) part[((uint64_t)blockIdx.x * HS + r4 + 4 * v) * p_pad + k] = c.acc[g][0][v];
    }
    if constexpr (N4 > 0) {
      // D layout of v_mfma_f64_4x4x4_4b_f64: term 4 blk + (lane >> 4), hyper-parameter lane & 3
      const uint64_t slot4 = ((uint64_t)blockIdx.y * NW + wave) * 64 + g * 16 + ((lane >> 2) & 3) * 4 + r4;
      if (slot4 < p_pad) {
        const uint64_t k4 = sperm[slot4];
#pragma unroll
        for (int q = 0; q < N4; ++q)
          part[((uint64_t)blockIdx.x * HS + H16 + 4 * q + (lane & 3)) * p_pad + k4] = c.acc4[g][q];
      }
    }
  }
}

// D[h0 + h][k] = sum of the row-split partials laid out [split][hs][p_pad]
__global__ void k_ge0_reduce(const double *__restrict__ part, int nsplit, int hs, uint64_t p_pad,
                             int p, int nh, double *__restrict__ out /* [nh][p] */) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int h = blockIdx.y;
  if (k >= (uint64_t)p || h >= nh) return;
  double s = 0.0;
  for (int r = 0; r < nsplit; ++r) s += part[((uint64_t)r * hs + h) * p_pad + k];
  out[(uint64_t)h * p + k] = s;
}

// D[h0 + h][k] = sum of the row-split partials
__global__ void k_btu_reduce(const double *__restrict__ part, int nsplit, uint64_t p_pad, int p,
                             int nh, double *__restrict__ out /* [nh][p] */) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int h = blockIdx.y;
  if (k >= (uint64_t)p || h >= nh) return;
  double s = 0.0;
  for (int r = 0; r < nsplit; ++r) s += part[((uint64_t)r * kNHB + h) * p_pad + k];
  out[(uint64_t)h * p + k] = s;
}

// LDS bytes of a k_tmm_ge0 / k_tmm_ge0_db tile: the used columns and the staged gradient columns of nh
// hyper-parameters
size_t ge0_tile_bytes(const obhip_terms &t, int nh) { return (t.Mu + nh) * kTlPitch * sizeof(double); }

// nw = 8 | 16: k_tmm_ge0 with that many waves and one 16-block of hyper-parameters; nw = 32: k_tmm_ge0_db
// (16 waves, two tile buffers) with n4 > 0: a 16-block and n4 groups of four, n4 < 0: |n4| groups of four
// only, n4 = 0: the 16-block only
int run_tmm_ge0(bool sq, int nw, int n4, const obhip_basis &src, obhip_terms &t, const int *d_c0, int nhyp,
                int h0, const double *d_a, dim3 grid, uint64_t ntiles, uint64_t tps, double *part) {
  const ProdTabs T = prod_tabs(src, t);
  return pick<1, 2, 3, 4>((int)(t.W / 2), [&](auto W2) {
    return pick_bool(sq, [&](auto SQ) {
      if (nw == 32)
        return pick<1, 0>(n4 >= 0 ? 1 : 0, [&](auto NHB) {  // 16-blocks
          return pick<1, 2, 0>(n4 < 0 ? -n4 : n4, [&](auto N4) {
            if constexpr (!NHB() && N4() == 0) return no_kernel();
            else
              return launch_prod(k_tmm_ge0_db<W2(), SQ(), N4(), NHB()>, grid, dim3(1024),
                                 2 * ge0_tile_bytes(t, 16 * NHB() + 4 * N4()), T, t.sperm.p, d_c0, nhyp, h0, d_a,
                                 src.n, ntiles, tps, t.p_pad, part);
          });
        });
      return pick<16, 8>(nw, [&](auto NW) {
        return launch_prod(k_tmm_ge0<W2(), 1, SQ(), NW()>, grid, dim3(NW() * 64), ge0_tile_bytes(t, 16), T,
                           t.sperm.p, d_c0, nhyp, h0, d_a, src.n, ntiles, tps, t.p_pad, part);
      });
    });
  });
}
}  // namespace

bool tmm_ge0_supports(const obhip_terms &t) {
  const uint64_t w2 = t.W / 2;
  return w2 >= 1 && w2 <= 4 && ge0_tile_bytes(t, 32) <= kLdsTile;
}

// a tile of more than half the LDS leaves one block per CU: 16 waves in it instead of 8
// ... and where TWO tiles fit the LDS, 16 waves with the next tile prefetched into the second
// buffer (k_tmm_ge0_db; nw = 32 stands for it below)
// Hyper-parameters beyond a multiple of 16 (d = 20 mat25: 4 of 20) in groups of four on the
// 4 x 4 x 4 matrix instruction instead of a mostly empty 16-block: 1 to 8 left over take a pass of
// their own (NHB = 0), behind a 16-block they ride along with it (the products formed once; 22-39
// registers of the W2 = 2 kernel spilled outside the read pipeline).  d = 20 mat25 at the headline
// terms, 20 hyper-parameters, never / a pass of their own / riding along: dense part
// 5.47 / 4.52 / 3.50 ms, obfit evaluation 30.8 / 29.8 / 28.5 ms (profiles/r05_fours_ab.txt).
Ge0Geom ge0_geometry(const obhip_basis &b, const obhip_terms &t) {
  const int nhyp = (int)b.model->nhyp();
  const uint64_t ntiles = b.n_pad / kTileRows;
  Ge0Geom q;
  const size_t tile_lds = ge0_tile_bytes(t, 16);
  const bool two_tiles = 2 * tile_lds <= kLdsTile;
  bool one_per_cu = tile_lds > 80 * 1024;
  int nw = one_per_cu ? 16 : 8;
  if (two_tiles) nw = 32;
  if (nw == 32) one_per_cu = true;
  q.nw = nw;
  const uint64_t tpb = (uint64_t)(nw == 32 ? 16 : nw) * 64;
  q.pblocks = (t.p_pad + tpb - 1) / tpb;
  const int ncu = device_cus(b.device);
  const RowSplit rs = split_rows(ntiles, (uint64_t)ncu * (one_per_cu ? 1 : 2) / q.pblocks);
  q.nsplit = rs.nsplit, q.tps = rs.tps;
  // 16 hyper-parameters per pass: with two 16-blocks per pass (NHB = 2) the 64 accumulator
  // registers of a wave no longer fit beside the pipeline and the compiler spills them in the
  // inner loop (measured 8.4 ms against 2 x 1.7 ms at C3)
  for (int h0 = 0; h0 < nhyp;) {
    const int rem = nhyp - h0;
    // n4 > 0: 16 + 4 n4 hyper-parameters in this pass; n4 < 0: 4 |n4| only
    int n4 = 0;
    if (nw == 32 && rem > 16 && rem <= 24) n4 = (rem - 16 + 3) / 4;
    if (nw == 32 && rem <= 8) n4 = -((rem + 3) / 4);
    if (n4 > 0 && 2 * ge0_tile_bytes(t, 16 + 4 * n4) > kLdsTile) n4 = 0;
    const int nh = n4 > 0 ? rem : (n4 < 0 ? rem : std::min(16, rem));
    const int hs = n4 > 0 ? 16 + 4 * n4 : (n4 < 0 ? -4 * n4 : 16);
    q.passes.push_back({h0, nh, n4, hs});
    h0 += nh;
  }
  return q;
}

// (squared: the squared stores are formed from the gradient basis while staging -- gbsq is not needed)
int launch_tmm_ge0(obhip_basis &b, obhip_terms &t, bool squared, const double *d_a, double *d_out) {
  obhip_gradbasis &g = *b.grad;
  const obhip_basis &src = *g.gb;
  const int nhyp = (int)b.model->nhyp();
  const DevBuf<int> &dc0 = g.ge0col;  // absolute columns in the combined array (resident: no upload,
                                      // and no synchronisation at the end of this function)
  const uint64_t ntiles = b.n_pad / kTileRows;
  const Ge0Geom geo = ge0_geometry(b, t);
  const uint64_t nsplit = geo.nsplit, tps = geo.tps;
  const dim3 grid((unsigned)nsplit, (unsigned)geo.pblocks);
  ProfScope ps(squared ? "sqtmm_gradhyp_dense" : "tmm_gradhyp_dense");
  for (const Ge0Pass &ps1 : geo.passes) {
    double *part = nullptr;
    OB_TRY(b.workspace(nsplit * ps1.hs * t.p_pad * sizeof(double), (void **)&part));
    OB_TRY(run_tmm_ge0(squared, geo.nw, ps1.n4, src, t, dc0.p, nhyp, ps1.h0, d_a, grid, ntiles, tps, part));
    hipLaunchKernelGGL(k_ge0_reduce, dim3((unsigned)((t.p + 255) / 256), (unsigned)ps1.nh), dim3(256), 0,
                       cur_stream(), part, (int)nsplit, ps1.hs, t.p_pad, (int)t.p, ps1.nh,
                       d_out + (uint64_t)ps1.h0 * t.p);
    OB_HIP(hipGetLastError());
  }
  return 0;
}

BtuGeom btu_geometry(const obhip_basis &b, const obhip_terms &t) {
  const uint64_t ntiles = b.n_pad / kTileRows;
  BtuGeom q;
  q.nhb = kNHB;
  q.gy = (unsigned)((t.p_pad + 2047) / 2048);
  const RowSplit rs = split_rows(ntiles, 1024 / q.gy);
  q.nsplit = rs.nsplit, q.tps = rs.tps;
  return q;
}

int launch_bt_times_ge0(obhip_basis &b, obhip_terms &t, bool squared, const double *d_a, double *d_out) {
  OB_TRY(ensure_bmat(b, t));
  obhip_gradbasis &g = *b.grad;
  const obhip_basis &src = squared ? *g.gbsq : *g.gb;
  const int nhyp = (int)b.model->nhyp();
  const uint64_t ntiles = b.n_pad / kTileRows;
  const BtuGeom geo = btu_geometry(b, t);
  const unsigned gy = geo.gy;
  const uint64_t nsplit = geo.nsplit, tps = geo.tps;
  double *part = nullptr;
  OB_TRY(b.workspace(nsplit * kNHB * t.p_pad * sizeof(double), (void **)&part));
  ProfScope ps(squared ? "sqtmm_gradhyp_dense" : "tmm_gradhyp_dense");
  for (int h0 = 0; h0 < nhyp; h0 += kNHB) {
    const int nh = std::min(kNHB, nhyp - h0);
    pick_bool(squared, [&](auto SQ) {
      hipLaunchKernelGGL(k_bt_times_u<SQ()>, dim3((unsigned)nsplit, gy), dim3(512), 0, cur_stream(), b.bmat.p,
                         t.p_pad, src.bm.p, src.md.Mc, g.ge0col.p, nhyp, h0, d_a, b.n, ntiles, tps, part);
      return 0;
    });
    hipLaunchKernelGGL(k_btu_reduce, dim3((unsigned)((t.p + 255) / 256), (unsigned)nh), dim3(256), 0,
                       cur_stream(), part, (int)nsplit, t.p_pad, (int)t.p, nh,
                       d_out + (uint64_t)h0 * t.p);
  }
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace obhip
