// Acquisition picks: expected improvement, probability of improvement, a confidence bound and a contour
// criterion over a candidate set, in batches of k by fantasies, on the device (include/obhip.h, "acquisition
// picks").  No reference counterpart: the reference package has no design criteria.
//
// The state per candidate is the latent mean mu_i = b_i^T theta and the latent variance d_i = b_i^T S b_i,
// S = inv(H).  A fantasised run y* at row j moves them by a_i = b_i^T s, s = S b_j (kernels_acquire.hip); no
// coefficient vector is updated anywhere: mu_j is gathered where the pick is made.
//
//   set-up   d_i and S as the design entry forms them (row_forms_dev, X X^T) -- d_i from the stored product in
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
  if (criterion < OBHIP_ACQ_EI || criterion > OBHIP_ACQ_STRADDLE)
    return fail(OBHIP_ERR_INVALID, w + ": criterion must be OBHIP_ACQ_EI, _PI, _LCB or _STRADDLE");
  if (lie != OBHIP_LIE_BELIEVER && lie != OBHIP_LIE_CONSTANT)
    return fail(OBHIP_ERR_INVALID, w + ": lie must be OBHIP_LIE_BELIEVER or OBHIP_LIE_CONSTANT");
  if (!params) return fail(OBHIP_ERR_INVALID, w + ": params (best, xi, kappa, level) is null");
  if ((criterion == OBHIP_ACQ_EI || criterion == OBHIP_ACQ_PI) && !std::isfinite(params[0]))
    return fail(OBHIP_ERR_INVALID, w + ": best must be finite for EI and PI");
  if (!std::isfinite(params[1])) return fail(OBHIP_ERR_INVALID, w + ": xi must be finite");
  if (!std::isfinite(params[2]) || params[2] < 0.0)
    return fail(OBHIP_ERR_INVALID, w + ": kappa must be finite and >= 0");
  if (criterion == OBHIP_ACQ_STRADDLE && !std::isfinite(params[3]))
    return fail(OBHIP_ERR_INVALID, w + ": level must be finite for STRADDLE");
  if (lie == OBHIP_LIE_CONSTANT && !std::isfinite(lie_value))
    return fail(OBHIP_ERR_INVALID, w + ": lie_value must be finite under OBHIP_LIE_CONSTANT");
  if (!xcand) return fail(OBHIP_ERR_INVALID, w + ": null candidates");
  if (!index || !score || !n_picked) return fail(OBHIP_ERR_INVALID, w + ": null outputs index / score / n_picked");
  if (!theta) return fail(OBHIP_ERR_INVALID, w + ": d_theta is null");
  if (!post) return fail(OBHIP_ERR_INVALID, w + ": null posterior");
  OB_TRY(check_compat(post->model, post->terms));
  if (post->terms->p != post->p || post->p > 65535)
    return fail(OBHIP_ERR_INVALID, w + ": the posterior and its terms disagree on p (or p > 65535)");
  return 0;
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
  const double nu = std::exp(2.0 * post->sigma), sgn = maximize ? -1.0 : 1.0;
  const uint64_t nparts = (m + kAcqRows - 1) / kAcqRows;
  OB_TRY(prepare_predict(om, t, false));

  DevBuf<double> mu, dvar, a, S, vec, sh, scal, trace, bj, xj0, pscore;
  DevBuf<int64_t> pidx;
  DevBuf<uint8_t> picked, elig;
  OB_TRY(mu.alloc(m));
  OB_TRY(dvar.alloc(m));
  OB_TRY(a.alloc(m));
  OB_TRY(picked.alloc(m));
  OB_TRY(elig.alloc(m));
  OB_TRY(S.alloc(pp * pp));
  OB_TRY(vec.alloc(2 * p));   // s | h = 0, as launch_design_pspace writes them
  OB_TRY(sh.alloc(p * 16));   // its [p][16] block and its trace: written, not read here
  OB_TRY(trace.alloc(k + 1));
  OB_TRY(scal.alloc(kAcqScal));
  OB_TRY(bj.alloc(p));
  OB_TRY(xj0.alloc(d));
  OB_TRY(pscore.alloc(nparts));
  OB_TRY(pidx.alloc(nparts));
  hipStream_t st = cur_stream();
  OB_HIP(hipMemsetAsync(picked.p, 0, m, st));
  OB_HIP(hipMemsetAsync(a.p, 0, m * sizeof(double), st));
  OB_HIP(hipMemsetAsync(vec.p, 0, 2 * p * sizeof(double), st));
  OB_HIP(hipMemsetAsync(sh.p, 0, p * 16 * sizeof(double), st));
  OB_HIP(hipMemsetAsync(trace.p, 0, (k + 1) * sizeof(double), st));
  OB_TRY(launch_sample_elig(d_xcand, m, d, d_skip, elig.p));
  // d_i = || L^-1 b_i ||^2, S = inv(H) = Linv^T Linv with Linv = X^T, mu_i = b_i^T theta
  OB_TRY(row_forms_dev(om, t, post->f.X.p, true, p, pp, d_xcand, m, dvar.p, true));
  {
    DevBuf<double> Linv;
    OB_TRY(Linv.alloc(pp * pp));
    OB_HIP(hipMemsetAsync(Linv.p, 0, pp * pp * sizeof(double), st));
    OB_TRY(launch_transpose(post->f.X.p, pp, Linv.p, pp, p));
    OB_TRY(launch_atb(kAtbStore, Linv.p, pp, pp, Linv.p, pp, pp, pp, false, S.p, pp));
    OB_HIP(hipStreamSynchronize(st));  // Linv is a local
  }
  OB_TRY(launch_predict(om, t, d_theta, d_xcand, m, mu.p, nullptr, 0.0, nullptr));
  // gamma = 1, delta = 0 and a = 0: the first pass downdates nothing
  double scal0[kAcqScal] = {1.0, 0.0, 0.0, nu, 0.0, 0.0, 0.0, 0.0};
  scal0[kAcqDelta] = 0.0;
  scal0[kAcqBest] = sgn * params[0];
  OB_HIP(hipMemcpyAsync(scal.p, scal0, sizeof(scal0), hipMemcpyHostToDevice, st));
  OB_HIP(hipStreamSynchronize(st));  // scal0 is a local
  // the one-row basis b_j is evaluated with: its x is where k_acq_pick gathers the picked row
  OB_HIP(hipMemcpy2DAsync(xj0.p, sizeof(double), d_xcand, m * sizeof(double), sizeof(double), d,
                          hipMemcpyDeviceToDevice, st));
  BasisGuard one;
  OB_TRY(obhip_basis_create_dev(&one.b, &om, xj0.p, 1, t.maxlev.data()));

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
  s.picked = picked.p;
  s.mu = mu.p;
  s.dvar = dvar.p;
  s.scal = scal.p;
  s.part_score = pscore.p;
  s.part_idx = pidx.p;
  uint64_t npicked = 0;
  bool left = true;
  for (uint64_t step = 0; step < k; ++step) {
    if (step) OB_TRY(launch_predict(om, t, vec.p, d_xcand, m, a.p, nullptr, 0.0, nullptr));
    OB_TRY(launch_acq_update(s, step == 0 ? d_score0 : nullptr));
    OB_TRY(launch_acq_pick(s, d, step, d_index, d_score, one.b->x.p));
    double none = 0.0;
    OB_TRY(d2h(&none, scal.p + 5, sizeof(double)));  // the step's one host wait: is anything left?
    if (none != 0.0) {
      left = false;
      break;
    }
    ++npicked;
    OB_TRY(launch_build_basis(*one.b));
    OB_TRY(launch_getmat(*one.b, t, bj.p, 1));
    OB_TRY(launch_design_pspace(OBHIP_DESIGN_MAXVAR, p, pp, bj.p, S.p, nullptr, vec.p, vec.p + p, sh.p, scal.p,
                                trace.p, step));
  }
  if (left) {  // the last pick's downdate
    OB_TRY(launch_predict(om, t, vec.p, d_xcand, m, a.p, nullptr, 0.0, nullptr));
    OB_TRY(launch_acq_update(s, nullptr));
  }
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
