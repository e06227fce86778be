// Posterior draws: coefficient samples, sample paths and the per-draw extremum over a candidate set, on the
// device (include/obhip.h, "posterior draws").  No reference counterpart: the
// reference package has no sampling.
//
// The handle keeps H = L L^T and X = L^-T.  theta + X z is a draw from N(theta, inv(H)) for z ~ N(0, I_p); the
// caller supplies z (the library has no random number generator).  The draws are formed from the resident X
// (k_draw: an upper-triangular product with one fixed order per entry), not by a back substitution on L: X is
// there already, the product needs no launch per 64-row block of the factor, and its rounding is the one
// posterior_var_dev and the design entry already rest on.
//
//   draw      k_draw, 64 draws per launch, into the caller's p x S.
//   sample    the draws into pooled scratch, then the multi-response predictor's batched pass on them
//             (launch_predict_multi; the column loop over launch_predict where that pass does not take the
//             term set): the bits obhip_predict_multi_dev's batched columns have on the same coefficients.
//   extremum  per pass of 16 NQB <= 128 draws: k_draw writes the term-major block, k_sample_ext forms the paths of a
//             64-row tile on the matrix cores and reduces them where they are formed, k_sample_pick merges
//             the workgroups' partials.  Kernel boundaries only, no host wait.
//             Term sets beyond sample_ext_supports (and OBHIP_FORCE_GENERIC): the paths of <= 64 draws and
//             a row chunk go to pooled scratch (at most 1 GiB) as sample forms them, k_sample_colext
//             reduces the columns from HBM, the row chunks' partials are merged in ascending order.
#include <cmath>

#include "obhip_internal.h"
#include "row_chunks.h"

using namespace obhip;

namespace {

// what all three entries refuse of the draws' own arguments; what needs the handle comes last
int check_draws(const char *who, const obhip_posterior *post, const void *theta, const void *z, uint64_t ldz,
                uint64_t S) {
  const std::string w(who);
  if (S == 0) return fail(OBHIP_ERR_INVALID, w + ": S = 0, no draws asked for");
  if (!theta) return fail(OBHIP_ERR_INVALID, w + ": d_theta is null");
  if (!z) return fail(OBHIP_ERR_INVALID, w + ": d_z is null");
  OB_TRY(check_post_handle(w, post, false));
  if (ldz < post->p) return fail(OBHIP_ERR_INVALID, w + ": ldz < p");
  return 0;
}

// d_Theta (p x S, leading dimension p) = the draws of all S columns of d_z, 64 per launch
int draw_all(const obhip_posterior &post, const double *d_theta, const double *d_z, uint64_t ldz, uint64_t S,
             double *d_Theta) {
  for (uint64_t s0 = 0; s0 < S; s0 += kDrawChunk) {
    const int qc = (int)std::min(kDrawChunk, S - s0);
    OB_TRY(launch_draw(post.f, d_theta, d_z + s0 * ldz, ldz, qc, 0, nullptr, d_Theta + s0 * post.p));
  }
  return 0;
}

// d_path (n x q, leading dimension n) = B(x) Theta; the terms are prepared
int sample_paths(const obhip_model &m, obhip_terms &t, const double *d_Theta, uint64_t q, const double *d_x, uint64_t n,
                 double *d_path) {
  if (predict_multi_supports(t)) return launch_predict_multi(m, t, d_Theta, q, d_x, n, d_path);
  for (uint64_t j = 0; j < q; ++j)
    OB_TRY(launch_predict(m, t, d_Theta + j * t.p, d_x, n, d_path + j * n, nullptr, 0.0, nullptr));
  return 0;
}

}  // namespace

extern "C" int obhip_posterior_draw_dev(const obhip_posterior *post, const double *d_theta, const double *d_z,
                                        uint64_t ldz, uint64_t S, double *d_Theta) {
  if (S != 0 && !d_Theta) return fail(OBHIP_ERR_INVALID, "posterior_draw_dev: the output d_Theta is null");
  OB_TRY(check_draws("posterior_draw_dev", post, d_theta, d_z, ldz, S));
  OB_TRY(require_device());
  return draw_all(*post, d_theta, d_z, ldz, S, d_Theta);
}

extern "C" int obhip_posterior_sample_dev(const obhip_posterior *post, const double *d_theta, const double *d_z,
                                          uint64_t ldz, uint64_t S, const double *d_x, uint64_t n, double *d_path) {
  if (S != 0 && n != 0 && !d_path) return fail(OBHIP_ERR_INVALID, "posterior_sample_dev: the output d_path is null");
  if (S != 0 && n != 0 && !d_x) return fail(OBHIP_ERR_INVALID, "posterior_sample_dev: d_x is null");
  OB_TRY(check_draws("posterior_sample_dev", post, d_theta, d_z, ldz, S));
  OB_TRY(require_device());
  if (n == 0) return 0;
  const obhip_model &om = *post->model;
  obhip_terms &t = *const_cast<obhip_terms *>(post->terms);
  OB_TRY(prepare_predict(om, t, false));
  DevBuf<double> Theta;
  OB_TRY(Theta.alloc(post->p * S));
  OB_TRY(draw_all(*post, d_theta, d_z, ldz, S, Theta.p));
  return sample_paths(om, t, Theta.p, S, d_x, n, d_path);
}

extern "C" int obhip_posterior_extremum_dev(const obhip_posterior *post, const double *d_theta, const double *d_z,
                                            uint64_t ldz, uint64_t S, const double *d_xcand, uint64_t m,
                                            const uint8_t *d_skip, int maximize, int64_t *d_index, double *d_value) {
  const char *who = "posterior_extremum_dev";
  if (S == 0) return check_draws(who, post, d_theta, d_z, ldz, S);
  if (m == 0) return fail(OBHIP_ERR_INVALID, std::string(who) + ": m = 0, no candidates");
  if (!d_xcand) return fail(OBHIP_ERR_INVALID, std::string(who) + ": d_xcand is null");
  if (!d_index || !d_value) return fail(OBHIP_ERR_INVALID, std::string(who) + ": the outputs d_index / d_value are null");
  OB_TRY(check_draws(who, post, d_theta, d_z, ldz, S));
  OB_TRY(require_device());
  const obhip_model &om = *post->model;
  obhip_terms &t = *const_cast<obhip_terms *>(post->terms);
  const uint64_t p = post->p, d = om.d;
  const double sgn = maximize ? -1.0 : 1.0;
  OB_TRY(prepare_predict(om, t, false));
  DevBuf<uint8_t> elig;
  DevBuf<double> pkey;
  DevBuf<int64_t> pidx;
  OB_TRY(elig.alloc(m));
  OB_TRY(launch_sample_elig(d_xcand, m, d, d_skip, elig.p));
  if (sample_ext_supports(t)) {
    const uint64_t qmax = 16 * (uint64_t)sample_ext_nqb_max(t), nblk = (m + kTileRows - 1) / kTileRows;
    DevBuf<double> tht;
    OB_TRY(tht.alloc(p * qmax));
    OB_TRY(pkey.alloc(nblk * qmax));
    OB_TRY(pidx.alloc(nblk * qmax));
    for (uint64_t s0 = 0; s0 < S; s0 += qmax) {
      const int qc = (int)std::min(qmax, S - s0);
      int nqb = 1;
      while (16 * nqb < qc) nqb *= 2;
      const uint64_t qw = 16 * (uint64_t)nqb;
      OB_TRY(launch_draw(post->f, d_theta, d_z + s0 * ldz, ldz, qc, qw, tht.p, nullptr));
      OB_TRY(launch_sample_ext(om, t, tht.p, nqb, d_xcand, m, elig.p, sgn, pkey.p, pidx.p));
      OB_TRY(launch_sample_pick(pkey.p, pidx.p, nblk, qw, qc, sgn, d_index + s0, d_value + s0));
    }
    return 0;
  }
  // the unfused route: row chunks so that the paths of 64 draws stay within 1 GiB of scratch
  const uint64_t cmax = (1ull << 30) / (kDrawChunk * sizeof(double));  // a multiple of kColextRows
  const uint64_t nparts = (m + kColextRows - 1) / kColextRows, rows = std::min(m, cmax);
  const RowChunks chunks{m, cmax};
  DevBuf<double> Theta, path, xc;
  OB_TRY(Theta.alloc(p * kDrawChunk));
  OB_TRY(path.alloc(rows * kDrawChunk));
  OB_TRY(pkey.alloc(nparts * kDrawChunk));
  OB_TRY(pidx.alloc(nparts * kDrawChunk));
  for (uint64_t s0 = 0; s0 < S; s0 += kDrawChunk) {
    const int qc = (int)std::min(kDrawChunk, S - s0);
    OB_TRY(launch_draw(post->f, d_theta, d_z + s0 * ldz, ldz, qc, 0, nullptr, Theta.p));
    for (uint64_t ci = 0; ci < chunks.count(); ++ci) {
      const RowChunk c = chunks.at(ci);
      const double *xsrc = nullptr;
      OB_TRY(gather_rows(xc, d_xcand, m, d, c, &xsrc));
      OB_TRY(sample_paths(om, t, Theta.p, (uint64_t)qc, xsrc, c.nr, path.p));
      OB_TRY(launch_sample_colext(path.p, c.nr, c.nr, c.r0, qc, elig.p, sgn, kDrawChunk, pkey.p, pidx.p));
    }
    OB_TRY(launch_sample_pick(pkey.p, pidx.p, nparts, kDrawChunk, qc, sgn, d_index + s0, d_value + s0));
  }
  return 0;
}
