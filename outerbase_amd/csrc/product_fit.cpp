// Newton fit on gridded data: host side (include/obhip.h, "Newton fit on the product of two input blocks";
// kernels in kernels_product_fit.hip).  No reference counterpart.
//   product_batch_normal_eq   the normal equations of the na nb pairs of one grid batch from the two staged side
//                             matrices At (na x p) and Bt (nb x p): their Grams through gram_of_staged into two
//                             packed triangles (the caller folds their Hadamard product), their column sums, and
//                             R_k = sum_i At[i,k] ((Y - c) Bt)[i,k] with the long index j contracted on the matrix
//                             cores by launch_atb, chunk of j after chunk of j in ascending order
//   obhip_product_side_dev    a staged side matrix itself
//   obhip_product_fit_layout  what the staging kernel does with either side (host only)
// At is staged whole (its rows are the M side of the GEMM and the rows of the final dot); Bt in row chunks sized by
// the free HBM.  Every check that can refuse a call runs before the first device call.
#include <algorithm>
#include <string>

#include "obhip_internal.h"
#include "vec_ops.h"

using namespace obhip;

namespace obhip {

namespace {

uint64_t pad_to(uint64_t n, uint64_t m) { return (n + m - 1) / m * m; }

}  // namespace

int product_batch_normal_eq(obhip_basis &holder, const obhip_model &m, obhip_terms &t, const ProductSplit &s,
                            const double *d_xa, uint64_t na, const double *d_xb, uint64_t nb, const double *d_Y,
                            uint64_t lda, uint64_t q, bool empty, const double *d_mom_state, double *d_GA,
                            double *d_GB, double *d_tail) {
  OB_TRY(ensure_product_tables(m, t, s));
  const uint64_t p = t.p, pp = t.p_pad;
  const uint64_t ta = (na + kTileRows - 1) / kTileRows, tb = (nb + kTileRows - 1) / kTileRows;
  const uint64_t ldp = pad_to(na, 128), nbp = tb * kTileRows;  // launch_atb: M in 128s, K in 64s
  const uint64_t rb = product_fit_resp_block(ldp, pp, q);
  double *d_R = d_tail, *d_b1 = d_tail + p * q, *d_mom = d_tail + p * (q + 1);
  DevBuf<double> Ys, part, At, cpart, a1, bs, W2, dpart, Bt;
  OB_TRY(Ys.alloc(q * nbp * ldp));
  OB_TRY(part.alloc((size_t)kSumBlocks * q));
  OB_TRY(launch_product_fit_moments(d_Y, lda, na, nb, q, rb, nbp, ldp, empty, d_mom_state, d_mom, Ys.p, part.p));

  // side A, whole: the staged matrix, its column sums
  OB_TRY(At.alloc(ta * kTileRows * pp));
  OB_TRY(a1.alloc(p));
  OB_TRY(bs.alloc(p));
  OB_TRY(W2.alloc(rb * ldp * pp));
  OB_TRY(dpart.alloc(rb * product_rhs_splits(na) * pp));
  // Row chunks of the staged sides as grad_batch_normal_eq sizes them: each within a quarter of the free HBM
  // and 16 GB.  Side A stays staged whole and gives the Gram kernels its tiles chunk by chunk.
  size_t free_b = 0, total_b = 0;
  OB_HIP(hipMemGetInfo(&free_b, &total_b));
  const char *forced = getenv("OBHIP_GRAM_CHUNK_ROWS");  // tests
  const uint64_t ctiles = gram_chunk_tiles(free_b, pp * kTileRows * sizeof(double), std::max(ta, tb),
                                           forced ? std::max<uint64_t>(1, (uint64_t)atoll(forced)) : 0);
  if (!ctiles) return fail(OBHIP_ERR_HIP, "not enough free HBM for even one row chunk of a staged side matrix");
  const uint64_t cb = std::min(ctiles, tb);
  OB_TRY(Bt.alloc(cb * kTileRows * pp));
  OB_TRY(cpart.alloc(std::max(ta, cb) * pp));
  {
    SideStage st;
    st.side = 0, st.x = d_xa, st.ldx = na, st.n = na;
    st.out = At.p, st.pitch = pp, st.pcols = pp, st.colpart = cpart.p;
    OB_TRY(launch_materialize_side(m, t, st));
    OB_TRY(launch_dx_colsum(cpart.p, ta, pp, p, false, a1.p));
  }
  GramSink sink;
  sink.packed = true;
  // The Gram de-duplication stays valid on a side matrix: a row of At is still `scale x one function of the
  // level per dimension` -- the constant 1 in the dimensions of the other side -- so an entry of At^T At depends
  // on the unordered level pairs per dimension of that side only, and two entries that gram_dedup.hip found
  // equal by the pairs of ALL dimensions are equal here too.
  {
    ProfScope ps("product_fit_gram_a");
    sink.out = d_GA;
    for (uint64_t t0 = 0; t0 < ta; t0 += ctiles) {
      const uint64_t nt = std::min(ctiles, ta - t0);
      OB_TRY(gram_of_staged(holder, At.p + t0 * kTileRows * pp, nt, t, sink, t0 != 0, t0 + nt >= ta));
    }
  }
  // side B in row chunks: stage, column sums, Gram, and the chunk's share of every right-hand side
  sink.out = d_GB;
  for (uint64_t t0 = 0; t0 < tb; t0 += cb) {
    const uint64_t nt = std::min(cb, tb - t0), j0 = t0 * kTileRows;
    SideStage st;
    st.side = 1, st.x = d_xb + j0, st.ldx = nb, st.n = std::min<uint64_t>(nt * kTileRows, nb - j0);
    st.out = Bt.p, st.pitch = pp, st.pcols = pp, st.colpart = cpart.p;
    OB_TRY(launch_materialize_side(m, t, st));
    OB_TRY(launch_dx_colsum(cpart.p, nt, pp, p, t0 != 0, bs.p));
    {
      ProfScope ps("product_fit_gram_b");
      OB_TRY(gram_of_staged(holder, Bt.p, nt, t, sink, t0 != 0, t0 + nt >= tb));
    }
    for (uint64_t r0 = 0; r0 < q; r0 += rb) {
      const uint64_t rc = std::min(rb, q - r0);
      {
        // W2[rr ldp + i][k] = sum_{j in chunk} (Y - c)[r0 + rr][j][i] Bt[j][k]
        ProfScope ps("product_fit_gemm");
        OB_TRY(launch_atb(kAtbStore, Ys.p + product_fit_ys_at(r0, j0, 0, q, rb, nbp, ldp), rc * ldp, rc * ldp, Bt.p, pp,
                          pp, nt * kTileRows, false, W2.p, pp));
      }
      OB_TRY(launch_product_rhs_dot(At.p, W2.p, pp, na, ldp, rc, p, t0 != 0, dpart.p, d_R + r0 * p));
    }
  }
  return launch_hadamard(p, a1.p, bs.p, d_b1);
}

// the sides' column lists hold 16-bit indices
int check_side_columns(const char *who, const ProductSplit &s) {
  if (s.mu_a > 65535 || s.mu_b > 65535)
    return fail(OBHIP_ERR_INVALID, std::string(who) + ": more than 65535 used basis columns on one side");
  return 0;
}

}  // namespace obhip

extern "C" {

int obhip_product_fit_layout(const obhip_terms *t, const uint32_t *dims_b, uint64_t ndims_b, uint64_t *mu_a,
                             uint64_t *mu_b, int *fused_a, int *fused_b) {
  if (!t) return fail(OBHIP_ERR_INVALID, "product_fit_layout: null terms");
  ProductSplit s;
  OB_TRY(make_split("product_fit_layout", *t, dims_b, ndims_b, s));
  if (mu_a) *mu_a = s.mu_a;
  if (mu_b) *mu_b = s.mu_b;
  if (fused_a) *fused_a = materialize_side_supports(s.mu_a, s.wa) ? 1 : 0;
  if (fused_b) *fused_b = materialize_side_supports(s.mu_b, s.wb) ? 1 : 0;
  return 0;
}

int obhip_product_side_dev(const obhip_model *m, const obhip_terms *t, const uint32_t *dims_b, uint64_t ndims_b,
                           int side, const double *d_x, uint64_t n, double *d_out, uint64_t pitch) {
  if (!m || !t) return fail(OBHIP_ERR_INVALID, "product_side_dev: null model or terms");
  OB_TRY(check_compat(m, t));
  ProductSplit s;
  OB_TRY(make_split("product_side_dev", *t, dims_b, ndims_b, s));
  if (side != 0 && side != 1) return fail(OBHIP_ERR_INVALID, "product_side_dev: side must be 0 (A) or 1 (B)");
  if (pitch < t->p) return fail(OBHIP_ERR_INVALID, "product_side_dev: pitch below the number of terms");
  OB_TRY(check_side_columns("product_side_dev", s));
  if (n > kMaxRowsPerCall) return fail(OBHIP_ERR_INVALID, "product_side_dev: more than 2^40 rows in one call");
  if (n == 0) return 0;
  if (!d_x || !d_out) return fail(OBHIP_ERR_INVALID, "product_side_dev: null x or out");
  OB_TRY(require_device());
  obhip_terms &tt = *const_cast<obhip_terms *>(t);
  OB_TRY(ensure_product_tables(*m, tt, s));
  SideStage st;
  st.side = side, st.x = d_x, st.ldx = n, st.n = n;
  st.out = d_out, st.pitch = pitch, st.pcols = pitch;
  return launch_materialize_side(*m, tt, st);
}

}  // extern "C"
