// Term-count path on a posterior handle (include/obhip.h, "term-count path"; no reference
// counterpart).  The terms stand in list order and the factor of the whole list nests the factor of every prefix, so
// one handle serves the model of the first k terms for every k:
//   path_coef      U = X^T G = L^-1 G, forward substitution nests as well: U_k = U[:k]
//   path_theta     Theta_k = X[:k,:k] U[:k]
//   path_evidence  the log evidence of every checkpoint: host arithmetic over diag L (copied as factor_logdet copies
//                  it), U and prec, one ascending order
//   path_scores    per row chunk (for_row_chunks) the stored product Z = B X by launch_atb in its fixed-order mode --
//                  the pass of post_var_dev, with the product kept for the chunk -- and per block of responses one
//                  pass of k_term_path over it; the chunk's tile sums are folded into the call's groups, the groups
//                  summed at the end (term_path_plan.h has the sizes and the layout)
// Every check that can refuse a call runs before the first launch.
#include <cmath>
#include <string>
#include <vector>

#include "obhip_internal.h"
#include "row_chunks.h"
#include "term_path_plan.h"

using namespace obhip;

namespace {

int refuse(const char *who, const char *why) { return fail(OBHIP_ERR_INVALID, std::string(who) + ": " + why); }

// what the entries on a handle and q responses share
int check_path_handle(const char *who, const obhip_posterior *post, uint64_t q) {
  if (q == 0 || q > kTpMaxQ) return refuse(who, "q must be between 1 and 65534");
  return check_post_handle(who, post, true);
}

}  // namespace

extern "C" int obhip_term_path_layout(uint64_t p, uint64_t q, uint64_t step, uint64_t n, uint64_t chunk_rows,
                                      uint64_t *K, uint64_t *chunk_rows_used, uint64_t *scratch_bytes) {
  if (const char *why = term_path_refusal(p, q, step, n, chunk_rows)) return refuse("term_path_layout", why);
  const TermPathPlan plan = term_path_plan(p, q, step, n, chunk_rows);
  if (K) *K = plan.K();
  if (chunk_rows_used) *chunk_rows_used = plan.cmax;
  if (scratch_bytes) *scratch_bytes = plan.scratch_bytes();
  return 0;
}

extern "C" int obhip_posterior_hessian_diag_dev(const obhip_posterior *post, double *d_diag) {
  if (!post || !d_diag) return refuse("posterior_hessian_diag_dev", "null argument");
  OB_TRY(check_post_handle("posterior_hessian_diag_dev", post, false));
  OB_TRY(require_device());
  const uint64_t p = post->p;
  OB_HIP(hipMemcpy2DAsync(d_diag, sizeof(double), post->H.p, (p + 1) * sizeof(double), sizeof(double), p,
                          hipMemcpyDeviceToDevice, cur_stream()));
  return 0;
}

extern "C" int obhip_posterior_path_coef_dev(const obhip_posterior *post, const double *d_G, uint64_t q, double *d_U) {
  if (!post || !d_G || !d_U) return refuse("posterior_path_coef_dev", "null argument");
  OB_TRY(check_path_handle("posterior_path_coef_dev", post, q));
  OB_TRY(require_device());
  return launch_term_path_coef(post->f.X.p, post->p, post->f.pp, d_G, q, d_U);
}

extern "C" int obhip_posterior_path_theta_dev(const obhip_posterior *post, const double *d_U, uint64_t q, uint64_t k,
                                              double *d_Theta) {
  if (!post || !d_U || !d_Theta) return refuse("posterior_path_theta_dev", "null argument");
  OB_TRY(check_path_handle("posterior_path_theta_dev", post, q));
  if (k == 0 || k > post->p) return refuse("posterior_path_theta_dev", "k must be between 1 and p");
  OB_TRY(require_device());
  return launch_term_path_theta(post->f.X.p, post->p, post->f.pp, d_U, q, k, d_Theta);
}

extern "C" int obhip_posterior_path_evidence(const obhip_posterior *post, const double *d_U, uint64_t q,
                                             const double *prec, const double *yty, uint64_t n_rows, uint64_t step,
                                             double *out) {
  if (!post || !d_U || !prec || !yty || !out) return refuse("posterior_path_evidence", "null argument");
  OB_TRY(check_path_handle("posterior_path_evidence", post, q));
  if (const char *why = term_path_refusal(post->p, q, step, 0, 0)) return refuse("posterior_path_evidence", why);
  OB_TRY(require_device());
  const uint64_t p = post->p;
  const TermPathPlan plan = term_path_plan(p, q, step, 0, 0);
  std::vector<double> diag(p), u(p * q);
  OB_HIP(hipMemcpy2DAsync(diag.data(), sizeof(double), post->f.L.p, (p + 1) * sizeof(double), sizeof(double), p,
                          hipMemcpyDeviceToHost, cur_stream()));
  OB_HIP(hipMemcpyAsync(u.data(), d_U, p * q * sizeof(double), hipMemcpyDeviceToHost, cur_stream()));
  OB_HIP(hipStreamSynchronize(cur_stream()));
  const double sigma = post->sigma, e2 = std::exp(-2.0 * sigma), nn = (double)n_rows;
  const double log2pi = 1.8378770664093454835606594728112;
  // the part every response shares, term after term: -sum log L_jj + 1/2 sum log prec_j
  std::vector<double> shared(plan.K());
  {
    double sl = 0.0, sp = 0.0;
    uint64_t next = plan.next_checkpoint(0), c = 0;
    for (uint64_t j = 0; j < p; ++j) {
      sl += std::log(diag[j]);
      sp += std::log(prec[j]);
      if (j + 1 == next) {
        shared[c++] = 0.5 * sp - sl;
        next = plan.next_checkpoint(next);
      }
    }
  }
  for (uint64_t r = 0; r < q; ++r) {
    const double head = -0.5 * nn * log2pi - nn * sigma - 0.5 * e2 * yty[r];
    double su = 0.0;
    uint64_t next = plan.next_checkpoint(0), c = 0;
    for (uint64_t j = 0; j < p; ++j) {
      su = std::fma(u[r * p + j], u[r * p + j], su);
      if (j + 1 == next) {
        out[c * q + r] = head + 0.5 * su + shared[c];
        ++c;
        next = plan.next_checkpoint(next);
      }
    }
  }
  return 0;
}

extern "C" int obhip_posterior_path_scores_dev(const obhip_posterior *post, const double *d_U, uint64_t q,
                                               const double *d_x, uint64_t n, const double *d_Y, uint64_t ldy,
                                               const double *d_meansd, uint64_t step, int loo, uint64_t chunk_rows,
                                               double *d_scores, double *d_sumv) {
  const char *who = "posterior_path_scores_dev";
  if (!post || !d_U || !d_scores || !d_sumv || (n != 0 && (!d_x || !d_Y))) return refuse(who, "null argument");
  if (loo != 0 && loo != 1) return refuse(who, "loo must be 0 or 1");
  if (ldy < n) return refuse(who, "ldy below the rows");
  OB_TRY(check_path_handle(who, post, q));
  if (const char *why = term_path_refusal(post->p, q, step, n, chunk_rows)) return refuse(who, why);
  OB_TRY(require_device());
  const TermPathPlan plan = term_path_plan(post->p, q, step, n, chunk_rows);
  if (n == 0) {
    OB_HIP(hipMemsetAsync(d_scores, 0, plan.score_entries() * sizeof(double), cur_stream()));
    OB_HIP(hipMemsetAsync(d_sumv, 0, plan.K() * sizeof(double), cur_stream()));
    return 0;
  }
  const uint64_t pp = plan.pp(), E = plan.entries();
  const double nu = std::exp(2.0 * post->sigma);
  DevBuf<double> Z, part, groups;
  OB_TRY(groups.alloc(plan.groups() * E));
  OB_HIP(hipMemsetAsync(groups.p, 0, plan.groups() * E * sizeof(double), cur_stream()));
  OB_TRY(for_row_chunks(*post->model, *const_cast<obhip_terms *>(post->terms), d_x, n, plan.cmax, pp,
                        [&](uint64_t r0, uint64_t nr, uint64_t npad, const double *Bcm) -> int {
    const uint64_t ctiles = npad / kTpTileRows;
    OB_TRY(Z.alloc(npad * pp));
    OB_TRY(part.alloc(ctiles * E));
    {
      ProfScope ps("term_path_gemm");
      OB_TRY(launch_atb(kAtbStoreFixed, Bcm, npad, npad, post->f.X.p, pp, pp, pp, true, Z.p, pp));  // Z = B X
    }
    ProfScope ps("term_path_walk");
    for (uint64_t j0 = 0; j0 < q; j0 += kTpRespBlock)
      OB_TRY(launch_term_path(plan, Z.p, nr, npad, d_U, j0, std::min(kTpRespBlock, q - j0), d_Y + r0, ldy, d_meansd,
                              nu, loo, part.p));
    return launch_term_path_fold(plan, part.p, ctiles, r0 / kTpTileRows, groups.p);
  }));
  OB_TRY(launch_term_path_final(plan, groups.p, d_scores, d_sumv));
  OB_HIP(hipStreamSynchronize(cur_stream()));  // groups is a local
  return 0;
}
