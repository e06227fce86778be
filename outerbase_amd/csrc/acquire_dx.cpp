// Input gradients of the full-covariance posterior variance and of the acquisition criteria: host side
// (include/obhip.h, "acquisition gradients").  No reference counterpart.
//
//   run_acquire_dx      the handle's S = inv(H) (posterior_inverse), then per row chunk (for_row_chunks) the stored
//                       product Y = S B^T by launch_atb in its fixed-order mode (bit-identical rows give bit-identical
//                       columns of Y wherever they stand and however the call is chunked), then k_acquire_dx.
// Every check that can refuse a call runs before the first device call.
#include <cmath>

#include "obhip_internal.h"
#include "row_chunks.h"

using namespace obhip;

namespace {

// rows of a chunk so that B^T and Y (pp x rows doubles each) stay within 1 GiB each
uint64_t default_chunk_rows(uint64_t pp) { return chunk_rows_for(pp, 1ull << 30); }

int check_handle(const std::string &w, const obhip_posterior *post, const void *x, uint64_t n, uint64_t chunk_rows) {
  if (chunk_rows % 128 != 0) return fail(OBHIP_ERR_INVALID, w + ": chunk_rows must be 0 or a positive multiple of 128");
  if (n > kMaxRowsPerCall) return fail(OBHIP_ERR_INVALID, w + ": more than 2^40 rows in one call");
  if (!x && n > 0) return fail(OBHIP_ERR_INVALID, w + ": null x");
  return check_post_handle(w, post, true);
}

int check_criterion(const std::string &w, const void *theta, int criterion, const double *params, const void *score,
                    const void *gradscore) {
  OB_TRY(check_acq_criterion(w, criterion));
  OB_TRY(check_acq_params(w, criterion, params));
  if (!theta) return fail(OBHIP_ERR_INVALID, w + ": theta is null");
  if (!score || !gradscore) return fail(OBHIP_ERR_INVALID, w + ": null outputs score / gradscore");
  return 0;
}

// the checked call: crit kAdxNone or OBHIP_ACQ_*, a's outputs n and n x d with leading dimension n
int run_acquire_dx(const obhip_posterior *post, int crit, const double *d_theta, const double *d_x, uint64_t n,
                   uint64_t chunk_rows, AcqDxArgs a) {
  const obhip_model &om = *post->model;
  obhip_terms &t = *const_cast<obhip_terms *>(post->terms);
  const uint64_t pp = post->f.pp;
  OB_TRY(prepare_predict(om, t, true));
  const double *S = nullptr;
  OB_TRY(posterior_inverse(*post, &S));
  a.ldo = n;
  DevBuf<double> Ycm;
  return for_row_chunks(om, t, d_x, n, chunk_rows ? chunk_rows : default_chunk_rows(pp), pp,
                        [&](uint64_t r0, uint64_t nr, uint64_t npad, const double *Bcm) -> int {
    OB_TRY(Ycm.alloc(pp * npad));
    {
      ProfScope ps("acquire_dx_product");
      OB_TRY(launch_atb(kAtbStoreFixed, S, pp, pp, Bcm, npad, npad, pp, false, Ycm.p, npad));  // Y = S B^T
    }
    a.row0 = r0;
    return launch_acquire_dx(om, t, crit, d_theta, Ycm.p, npad, d_x + r0, n, nr, a);
  });
}

AcqDxArgs criterion_args(const double *params, int maximize) {
  AcqDxArgs a;
  a.sgn = maximize ? -1.0 : 1.0;
  a.best = a.sgn * params[0];
  a.xi = params[1];
  a.kappa = params[2];
  a.level = a.sgn * params[3];
  return a;
}

}  // namespace

extern "C" int obhip_posterior_var_grad_dev(const obhip_posterior *post, const double *d_x, uint64_t n,
                                            uint64_t chunk_rows, int with_noise, double *d_var, double *d_gradvar) {
  const std::string w("posterior_var_grad_dev");
  if (n > 0 && (!d_var || !d_gradvar)) return fail(OBHIP_ERR_INVALID, w + ": null outputs var / gradvar");
  OB_TRY(check_handle(w, post, d_x, n, chunk_rows));
  if (n == 0) return 0;
  OB_TRY(require_device());
  AcqDxArgs a;
  a.noise = with_noise ? std::exp(2.0 * post->sigma) : 0.0;
  a.var = d_var;
  a.gradvar = d_gradvar;
  return run_acquire_dx(post, kAdxNone, nullptr, d_x, n, chunk_rows, a);
}

extern "C" int obhip_acquire_grad_dev(const obhip_posterior *post, const double *d_theta, const double *d_x, uint64_t n,
                                      int criterion, const double params[4], int maximize, uint64_t chunk_rows,
                                      double *d_score, double *d_gradscore, double *d_mean, double *d_gradmean,
                                      double *d_var, double *d_gradvar) {
  const std::string w("acquire_grad_dev");
  OB_TRY(check_criterion(w, d_theta, criterion, params, n ? (const void *)d_score : (const void *)&w,
                         n ? (const void *)d_gradscore : (const void *)&w));
  OB_TRY(check_handle(w, post, d_x, n, chunk_rows));
  if (n == 0) return 0;
  OB_TRY(require_device());
  AcqDxArgs a = criterion_args(params, maximize);
  a.score = d_score;
  a.gradscore = d_gradscore;
  a.mean = d_mean;
  a.gradmean = d_gradmean;
  a.var = d_var;
  a.gradvar = d_gradvar;
  return run_acquire_dx(post, criterion, d_theta, d_x, n, chunk_rows, a);
}

extern "C" int obhip_acquire_grad(const obhip_posterior *post, const double *theta, const double *x, uint64_t n,
                                  int criterion, const double params[4], int maximize, uint64_t chunk_rows,
                                  double *score, double *gradscore, double *mean, double *gradmean, double *var,
                                  double *gradvar) {
  const std::string w("acquire_grad");
  OB_TRY(check_criterion(w, theta, criterion, params, n ? (const void *)score : (const void *)&w,
                         n ? (const void *)gradscore : (const void *)&w));
  OB_TRY(check_handle(w, post, x, n, chunk_rows));
  if (n == 0) return 0;
  OB_TRY(require_device());
  const uint64_t d = post->model->d;
  DevBuf<double> dth, dx, dscore, dgs, dmean, dgm, dvar, dgv;
  OB_TRY(dth.upload(theta, post->p));
  OB_TRY(upload_cols(dx, x, n, d, n));
  OB_TRY(dscore.alloc(n));
  OB_TRY(dgs.alloc(n * d));
  if (mean) OB_TRY(dmean.alloc(n));
  if (gradmean) OB_TRY(dgm.alloc(n * d));
  if (var) OB_TRY(dvar.alloc(n));
  if (gradvar) OB_TRY(dgv.alloc(n * d));
  OB_TRY(obhip_acquire_grad_dev(post, dth.p, dx.p, n, criterion, params, maximize, chunk_rows, dscore.p, dgs.p, dmean.p,
                                dgm.p, dvar.p, dgv.p));
  OB_TRY(d2h(score, dscore.p, n * sizeof(double)));
  OB_TRY(d2h(gradscore, dgs.p, n * d * sizeof(double)));
  if (mean) OB_TRY(d2h(mean, dmean.p, n * sizeof(double)));
  if (gradmean) OB_TRY(d2h(gradmean, dgm.p, n * d * sizeof(double)));
  if (var) OB_TRY(d2h(var, dvar.p, n * sizeof(double)));
  if (gradvar) OB_TRY(d2h(gradvar, dgv.p, n * d * sizeof(double)));
  return 0;
}

extern "C" int obhip_acquire_grad_layout(const obhip_posterior *post, int *fused, uint64_t *lds_bytes,
                                         uint64_t *default_chunk) {
  if (!post) return fail(OBHIP_ERR_INVALID, "acquire_grad_layout: null posterior");
  OB_TRY(check_compat(post->model, post->terms));
  OB_TRY(require_device());
  obhip_terms &t = *const_cast<obhip_terms *>(post->terms);
  OB_TRY(prepare_predict(*post->model, t, false));  // (the used-column count the tile is sized by)
  const bool f = acquire_dx_fused(t);
  if (fused) *fused = f ? 1 : 0;
  if (lds_bytes) *lds_bytes = acquire_dx_lds_bytes(t, post->model->d, f);
  if (default_chunk) *default_chunk = default_chunk_rows(post->f.pp);
  return 0;
}
