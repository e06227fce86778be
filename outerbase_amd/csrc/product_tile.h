// What the kernels on the product of two input blocks share on the device (kernels_product.hip,
// kernels_product_dx.hip): the arguments of a launch, the staged chunk of terms, the contraction of the two
// side tiles over the terms on the matrix cores, and the pieces of the likelihood epilogue.
//
// MFMA operand layout (as in kernels_chol.hip): lane = (m | n) + 16 k for A[m][k] and B[k][n]; the four
// accumulator registers of a lane are D[k + 4 r][n], r = 0..3.
#pragma once
#include "obhip_internal.h"
#include "device_dx.h"

namespace obhip {

typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int kPpThreads = 256, kPpWaves = kPpThreads / 64;
// LDS beside the two tiles: the waves' scale shares of both sides, the two row scales, the likelihood partials
constexpr int kPpStage = 2 * kPpWaves * kTileRows + 2 * kTileRows + 2 * 4 * kTileRows;
static_assert(kTileRows == (int)kProductTile, "a side of the tile is one basis tile");
// terms per staged chunk of the contraction: their coefficients, coefficient variances and column lists
constexpr int kPpTerms = 256;
struct PpChunk {
  double *th, *cv;          // [kPpTerms]
  uint32_t *cw_a, *cw_b;    // [kPpTerms][wa2], [kPpTerms][wb2]
};

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

struct PpArgs {
  const DimDesc *dims;
  const double *ka, *kb, *kc, *rot, *tab;
  const int *side_a, *side_b;
  int nda, ndb;
  const int *cpos_a, *cpos_b;
  int mu_a, mu_b;
  const uint32_t *cw_a, *cw_b;  // p x wa2, p x wb2 words of two used-column indices
  int wa2, wb2, p;
  const double *theta;          // the first of the qc responses of this launch
  int qc;
  const double *coeffvar;
  double e2sigma;
  const double *xa, *xb;
  uint64_t na, nb, tiles_b, atile0, tiles_a;
  double *mean;                 // of the first response of this launch
  uint64_t lda;
  double *var;
  const double *y, *obsvar;
  double *part;
};

// the operands of the four-term step s of the staged chunk for this lane's term 4 s + kq: U at the A rows ra,
// ra + 16 and V at the B rows rb, rb + 16 of the tiles, theta_k and c_k (both 0 beyond p, the lists all ones)
template <bool DOV>
__device__ __forceinline__ void pp_operands(const PpArgs &a, const double *__restrict__ ta,
                                            const double *__restrict__ tb, const PpChunk &ch, int s, int kq, int ra,
                                            int rb, double (&u)[2], double (&v)[2], double &thk, double &cvk) {
  const int k = 4 * s + kq;
  const uint32_t *ca = ch.cw_a + k * a.wa2;
  const uint32_t *cb = ch.cw_b + k * a.wb2;
  thk = ch.th[k];
  cvk = DOV ? ch.cv[k] : 0.0;
  double u0 = 1.0, u1 = 1.0, v0 = 1.0, v1 = 1.0;
  for (int w = 0; w < a.wa2; ++w) {
    const uint32_t c = ca[w];
    const double *c0 = ta + (c & 0xffffu) * kTileRows + ra, *c1 = ta + (c >> 16) * kTileRows + ra;
    u0 *= c0[0];
    u1 *= c0[16];
    u0 *= c1[0];
    u1 *= c1[16];
  }
  for (int w = 0; w < a.wb2; ++w) {
    const uint32_t c = cb[w];
    const double *c0 = tb + (c & 0xffffu) * kTileRows + rb, *c1 = tb + (c >> 16) * kTileRows + rb;
    v0 *= c0[0];
    v1 *= c0[16];
    v0 *= c1[0];
    v1 *= c1[16];
  }
  u[0] = u0, u[1] = u1, v[0] = v0, v[1] = v1;
}

// acc[b][a] += V_b (theta U_a)^T over all terms and, DOV, accv[b][a] += V_b^2 (c U_a^2)^T.  The terms' column
// lists and coefficients come through LDS in chunks of kPpTerms, loaded by the whole workgroup, so that no step
// waits for HBM; the operands of step s + 1 are formed behind the matrix instructions of step s, which do not
// wait for them.  Called by every thread of the workgroup (barriers).
template <bool DOV>
__device__ __forceinline__ void pp_contract(const PpArgs &a, const double *__restrict__ ta,
                                            const double *__restrict__ tb, const double *__restrict__ th,
                                            const PpChunk &ch, int kq, int ra, int rb, d4 (&acc)[2][2],
                                            d4 (&accv)[2][2]) {
  for (int k0 = 0; k0 < a.p; k0 += kPpTerms) {
    const int kc = min(kPpTerms, a.p - k0);
    __syncthreads();  // the previous chunk is spent
    for (int e = threadIdx.x; e < kPpTerms * a.wa2; e += kPpThreads)
      ch.cw_a[e] = e < kc * a.wa2 ? a.cw_a[(size_t)k0 * a.wa2 + e] : 0u;
    for (int e = threadIdx.x; e < kPpTerms * a.wb2; e += kPpThreads)
      ch.cw_b[e] = e < kc * a.wb2 ? a.cw_b[(size_t)k0 * a.wb2 + e] : 0u;
    for (int e = threadIdx.x; e < kPpTerms; e += kPpThreads) {
      ch.th[e] = e < kc ? th[k0 + e] : 0.0;
      if (DOV) ch.cv[e] = e < kc ? a.coeffvar[k0 + e] : 0.0;
    }
    __syncthreads();
    const int nsteps = (kc + 3) / 4;
    double u[2], v[2], thk, cvk;
    pp_operands<DOV>(a, ta, tb, ch, 0, kq, ra, rb, u, v, thk, cvk);
    for (int s = 0; s < nsteps; ++s) {
      const double tu0 = thk * u[0], tu1 = thk * u[1];
      acc[0][0] = mfma(v[0], tu0, acc[0][0]);
      acc[0][1] = mfma(v[0], tu1, acc[0][1]);
      acc[1][0] = mfma(v[1], tu0, acc[1][0]);
      acc[1][1] = mfma(v[1], tu1, acc[1][1]);
      if constexpr (DOV) {
        const double cu0 = cvk * (u[0] * u[0]), cu1 = cvk * (u[1] * u[1]);
        const double w0 = v[0] * v[0], w1 = v[1] * v[1];
        accv[0][0] = mfma(w0, cu0, accv[0][0]);
        accv[0][1] = mfma(w0, cu1, accv[0][1]);
        accv[1][0] = mfma(w1, cu0, accv[1][0]);
        accv[1][1] = mfma(w1, cu1, accv[1][1]);
      }
      if (s + 1 < nsteps) pp_operands<DOV>(a, ta, tb, ch, s + 1, kq, ra, rb, u, v, thk, cvk);
    }
  }
}

// the sum over the sixteen lanes of a row of the accumulator layout: the same butterfly in every lane
__device__ __forceinline__ double sum16(double v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  return v;
}

// r^2 / v and log v of one pair (0 for a row beyond na)
__device__ __forceinline__ void lik_terms(bool ok, double y, double mean, double var, double obsvar, double &t1,
                                          double &t2) {
  const double r = y - mean, v = var + obsvar;
  t1 = ok ? r * r / v : 0.0;
  t2 = ok ? log(v) : 0.0;
}

}  // namespace obhip
