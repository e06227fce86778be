// Jacobian and vector-Jacobian product of the multi-response predictor: the entry points.  No
// reference counterpart.  The kernel and its dispatch are in kernels_predict_jac.hip.
// Every check that can refuse a call runs before the first device call, in the order of
// obhip_predict_grad_dev (predict_dx.cpp).
#include "obhip_internal.h"

using namespace obhip;

namespace {
}

extern "C" {

int obhip_predict_jac_multi_dev(const obhip_model *m, const obhip_terms *t, const double *d_Theta, uint64_t q,
                                const double *d_x, uint64_t n, double *d_mean, double *d_jac) {
  if (!m || !t || !d_Theta || !d_x || !d_jac || q == 0)
    return fail(OBHIP_ERR_INVALID, "predict_jac_multi_dev: null model, terms, Theta, x or jac, or no response");
  if (n > kMaxRowsPerCall) return fail(OBHIP_ERR_INVALID, "predict_jac_multi_dev: more than 2^40 rows in one call");
  OB_TRY(check_compat(m, t));
  if (n == 0) return 0;
  OB_TRY(require_device());
  return launch_predict_jac(*m, *const_cast<obhip_terms *>(t), d_Theta, q, d_x, n, d_mean, d_jac, nullptr, 0,
                            nullptr);
}

int obhip_predict_vjp_multi_dev(const obhip_model *m, const obhip_terms *t, const double *d_Theta, uint64_t q,
                                const double *d_x, uint64_t n, const double *d_W, uint64_t ldw, double *d_mean,
                                double *d_out) {
  if (!m || !t || !d_Theta || !d_x || !d_W || !d_out || q == 0)
    return fail(OBHIP_ERR_INVALID, "predict_vjp_multi_dev: null model, terms, Theta, x, W or out, or no response");
  if (ldw < n) return fail(OBHIP_ERR_INVALID, "predict_vjp_multi_dev: leading dimension of W below n");
  if (n > kMaxRowsPerCall) return fail(OBHIP_ERR_INVALID, "predict_vjp_multi_dev: more than 2^40 rows in one call");
  OB_TRY(check_compat(m, t));
  if (n == 0) return 0;
  OB_TRY(require_device());
  return launch_predict_jac(*m, *const_cast<obhip_terms *>(t), d_Theta, q, d_x, n, d_mean, nullptr, d_W, ldw, d_out);
}

int obhip_predict_jac_multi(const obhip_model *m, const obhip_terms *t, const double *Theta, uint64_t q,
                            const double *x, uint64_t n, uint64_t ldx, double *mean, double *jac) {
  if (!m || !t || !Theta || !x || !jac || q == 0)
    return fail(OBHIP_ERR_INVALID, "predict_jac_multi: null model, terms, Theta, x or jac, or no response");
  if (n > kMaxRowsPerCall) return fail(OBHIP_ERR_INVALID, "predict_jac_multi: more than 2^40 rows in one call");
  if (ldx < n) return fail(OBHIP_ERR_INVALID, "predict_jac_multi: leading dimension below n");
  OB_TRY(check_compat(m, t));
  if (n == 0) return 0;
  OB_TRY(require_device());
  const uint64_t d = m->d;
  DevBuf<double> dx, dth, dmean, djac;
  OB_TRY(upload_cols(dx, x, n, d, ldx));
  OB_TRY(dth.upload(Theta, t->p * q));
  if (mean) OB_TRY(dmean.alloc(n * q));
  OB_TRY(djac.alloc(n * d * q));
  OB_TRY(obhip_predict_jac_multi_dev(m, t, dth.p, q, dx.p, n, dmean.p, djac.p));
  if (mean) OB_TRY(d2h(mean, dmean.p, n * q * sizeof(double)));
  OB_TRY(d2h(jac, djac.p, n * d * q * sizeof(double)));
  return 0;
}

}  // extern "C"
