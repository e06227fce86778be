// Acquisition picks: expected improvement, probability of improvement, a confidence bound and a contour
// criterion over a candidate set, in batches of k by fantasies, on the device (include/obhip.h, "acquisition
// picks").  No reference counterpart: the reference package has no design criteria.
//
// The state per candidate is the latent mean mu_i = b_i^T theta and the latent variance d_i = b_i^T S b_i,
// S = inv(H).  A fantasised run y* at row j moves them by a_i = b_i^T s, s = S b_j (kernels_acquire.hip); no
// coefficient vector is updated anywhere: mu_j is gathered where the pick is made.
//
//   set-up   d_i and S as the design entry has them (row_forms_dev, GreedyPicks) -- d_i from the stored product in
//            its fixed order of k, so that two bit-identical rows tie wherever they stand -- mu_i by one pass of
//            the one-response predictor on theta, the eligibility map as the draws form it.
//   step t   the predictor's pass on s (a to pooled scratch; zeros before the first pick), k_acq_update
//            (downdate of pick t - 1 and the scores for pick t in one pass), k_acq_pick, ONE host wait for the
//            "nothing left" flag, then b_j by the one-row basis and the design entry's p-space kernels.
//   end      one more predictor pass and update apply the last pick's downdate.
// The predictor chooses its own route (launch_predict: shared sub-products, tile, generic from HBM); there is
// no second route here.
#include <cmath>

#include "obhip_internal.h"

using namespace obhip;

namespace {

int check_acquire(const char *who, const obhip_posterior *post, const void *theta, const void *xcand, uint64_t m,
                  int criterion, const double *params, int lie, double lie_value, uint64_t k, const void *index,
                  const void *score, const uint64_t *n_picked) {
  const std::string w(who);
  // what does not need the handle first: these are refused whatever the handle is
  if (m == 0) return fail(OBHIP_ERR_INVALID, w + ": m = 0, no candidates");
  if (k == 0) return fail(OBHIP_ERR_INVALID, w + ": k = 0, no picks asked for");
  OB_TRY(check_acq_criterion(w, criterion));
  if (lie != OBHIP_LIE_BELIEVER && lie != OBHIP_LIE_CONSTANT)
    return fail(OBHIP_ERR_INVALID, w + ": lie must be OBHIP_LIE_BELIEVER or OBHIP_LIE_CONSTANT");
  OB_TRY(check_acq_params(w, criterion, params));
  if (lie == OBHIP_LIE_CONSTANT && !std::isfinite(lie_value))
    return fail(OBHIP_ERR_INVALID, w + ": lie_value must be finite under OBHIP_LIE_CONSTANT");
  if (!xcand) return fail(OBHIP_ERR_INVALID, w + ": null candidates");
  if (!index || !score || !n_picked) return fail(OBHIP_ERR_INVALID, w + ": null outputs index / score / n_picked");
  if (!theta) return fail(OBHIP_ERR_INVALID, w + ": d_theta is null");
  return check_post_handle(w, post, true);
}

}  // namespace

extern "C" int obhip_acquire_dev(const obhip_posterior *post, const double *d_theta, const double *d_xcand, uint64_t m,
                                 int criterion, const double *params, int maximize, int lie, double lie_value,
                                 const uint8_t *d_skip, uint64_t k, int64_t *d_index, double *d_score,
                                 double *d_score0, double *d_mean, double *d_var, uint64_t *n_picked) {
  OB_TRY(check_acquire("acquire_dev", post, d_theta, d_xcand, m, criterion, params, lie, lie_value, k, d_index, d_score,
                       n_picked));
  OB_TRY(require_device());
  const obhip_model &om = *post->model;
  obhip_terms &t = *const_cast<obhip_terms *>(post->terms);
  const uint64_t p = post->p, pp = post->f.pp, d = om.d;
  const double sgn = maximize ? -1.0 : 1.0;
  OB_TRY(prepare_predict(om, t, false));

  GreedyPicks g;
  DevBuf<double> mu, dvar, a;
  DevBuf<uint8_t> elig;
  OB_TRY(mu.alloc(m));
  OB_TRY(dvar.alloc(m));
  OB_TRY(a.alloc(m));
  OB_TRY(elig.alloc(m));
  OB_TRY(g.init(*post, d_xcand, m, k, kAcqScal, (m + kAcqRows - 1) / kAcqRows));
  hipStream_t st = cur_stream();
  OB_HIP(hipMemsetAsync(a.p, 0, m * sizeof(double), st));  // a = 0 and delta = 0: the first pass downdates nothing
  OB_TRY(launch_sample_elig(d_xcand, m, d, d_skip, elig.p));
  // d_i = || L^-1 b_i ||^2, mu_i = b_i^T theta
  OB_TRY(row_forms_dev(om, t, post->f.X.p, true, p, pp, d_xcand, m, dvar.p, true));
  OB_TRY(launch_predict(om, t, d_theta, d_xcand, m, mu.p, nullptr, 0.0, nullptr));
  g.scal0[kAcqBest] = sgn * params[0];

  AcqStep s;
  s.crit = criterion;
  s.lie = lie;
  s.n = m;
  s.sgn = sgn;
  s.xi = params[1];
  s.kappa = params[2];
  s.level = sgn * params[3];
  s.lie_value = lie_value;
  s.x = d_xcand;
  s.a = a.p;
  s.elig = elig.p;
  s.picked = g.picked.p;
  s.mu = mu.p;
  s.dvar = dvar.p;
  s.scal = g.scal.p;
  s.part_score = g.pscore.p;
  s.part_idx = g.pidx.p;
  // the predictor's pass on s = S b_j of the previous pick, then its downdate and the scores in one pass
  auto pass = [&](uint64_t step) -> int {
    if (step) OB_TRY(launch_predict(om, t, g.vec.p, d_xcand, m, a.p, nullptr, 0.0, nullptr));
    return launch_acq_update(s, step == 0 ? d_score0 : nullptr);
  };
  auto pick = [&](uint64_t step) { return launch_acq_pick(s, d, step, d_index, d_score, g.one.b->x.p); };
  uint64_t npicked = 0;
  OB_TRY(g.run(k, OBHIP_DESIGN_MAXVAR, nullptr, pass, pick, &npicked));
  if (d_mean) OB_HIP(hipMemcpyAsync(d_mean, mu.p, m * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (d_var) OB_HIP(hipMemcpyAsync(d_var, dvar.p, m * sizeof(double), hipMemcpyDeviceToDevice, st));
  OB_HIP(hipStreamSynchronize(st));
  *n_picked = npicked;
  return 0;
}

extern "C" int obhip_acquire(const obhip_posterior *post, const double *theta, const double *xcand, uint64_t m,
                             int criterion, const double *params, int maximize, int lie, double lie_value,
                             const uint8_t *skip, uint64_t k, int64_t *index, double *score, double *score0,
                             double *mean, double *var, uint64_t *n_picked) {
  OB_TRY(check_acquire("acquire", post, theta, xcand, m, criterion, params, lie, lie_value, k, index, score, n_picked));
  OB_TRY(require_device());
  const uint64_t d = post->model->d;
  DevBuf<double> dth, dx, dscore, dscore0, dmean, dvar;
  DevBuf<int64_t> dindex;
  DevBuf<uint8_t> dskip;
  OB_TRY(dth.upload(theta, post->p));
  OB_TRY(upload_cols(dx, xcand, m, d, m));
  if (skip) OB_TRY(dskip.upload(skip, m));
  OB_TRY(dindex.alloc(k));
  OB_TRY(dscore.alloc(k));
  if (score0) OB_TRY(dscore0.alloc(m));
  if (mean) OB_TRY(dmean.alloc(m));
  if (var) OB_TRY(dvar.alloc(m));
  uint64_t np = 0;
  OB_TRY(obhip_acquire_dev(post, dth.p, dx.p, m, criterion, params, maximize, lie, lie_value, dskip.p, k, dindex.p,
                           dscore.p, dscore0.p, dmean.p, dvar.p, &np));
  if (np) OB_TRY(d2h(index, dindex.p, np * sizeof(int64_t)));
  if (np) OB_TRY(d2h(score, dscore.p, np * sizeof(double)));
  if (score0) OB_TRY(d2h(score0, dscore0.p, m * sizeof(double)));
  if (mean) OB_TRY(d2h(mean, dmean.p, m * sizeof(double)));
  if (var) OB_TRY(d2h(var, dvar.p, m * sizeof(double)));
  *n_picked = np;
  return 0;
}
