// Newton fit of weighted Gaussian, binomial and Poisson responses: iteratively reweighted least
// squares around the pipeline of fit_newton.cpp (include/obhip.h, "weighted, binomial and Poisson
// responses", has the model and the iteration; no reference counterpart).
//
// What an iteration adds to the Gaussian one-step fit: the row pass k_glm_rows (kernels_glm.hip),
// one staging pass of the design matrix (the weights changed, so the staged matrix of the last
// iteration is of no use), one launch_mm for B delta, one or two row passes for the line search and
// the read-back of seven doubles.  The weighted basis is the caller's basis with its `scale` buffer
// exchanged for scale sqrt(w) while the Gram and B_w^T u are taken (ScaleSwap): every consumer of a
// basis reads its row factors from there, padded rows are zero in both, and no copy of the basis is
// made.  The swap is undone and the staged matrix invalidated on every way out, so a later
// unweighted use stages again.
//
// The ascent test compares F(theta + alpha delta) with F(theta) minus the rounding bound of the two
// sums, (n + p + 16) 2^-53 (A + A'), A the sum of the magnitudes F is summed of (the second sum of the
// row pass plus theta^T P theta / 2): a step cannot be refused on rounding noise alone, and tol is
// left as the caller gave it.
//
// One response, all rows on this device.  Row sharding (obhip_comm), several responses and the
// streaming accumulator are out of scope: the weights change with every iteration and differ per
// response, so neither one Gram for all responses nor sufficient statistics that outlive a step exist.
#include <cmath>

#include "obhip_internal.h"
#include "vec_ops.h"

using namespace obhip;

namespace {

constexpr double kU = 1.1102230246251565e-16;  // 2^-53
constexpr int kMaxHalvings = 30;

uint64_t pad64(uint64_t n) { return (n + kTileRows - 1) / kTileRows * kTileRows; }

// the fit's workspace, in doubles, before the Cholesky's own
struct GlmWs {
  double *scale_w, *u, *bd, *eta, *g, *rhs, *delta, *sums, *part;
  void *chol;
  static uint64_t doubles(uint64_t p, uint64_t n) { return 4 * pad64(n) + 3 * p + 8 + (uint64_t)kSumBlocks * 4; }
  GlmWs(void *ws, uint64_t p, uint64_t n) {
    const uint64_t np = pad64(n);
    scale_w = (double *)ws;
    u = scale_w + np;
    bd = u + np;
    eta = bd + np;
    g = eta + np;
    rhs = g + p;
    delta = rhs + p;
    sums = delta + p;  // [0..2] the row pass, [4..7] the p-sized dot products
    part = sums + 8;
    chol = part + (uint64_t)kSumBlocks * 4;
  }
};

// the caller's basis reads scale sqrt(w) for as long as this lives
struct ScaleSwap {
  obhip_basis &b;
  double *saved;
  ScaleSwap(obhip_basis &basis, double *d_scale_w) : b(basis), saved(basis.scale.p) {
    b.scale.p = d_scale_w;
    b.bmat_terms = 0;  // the staged design matrix carries other weights
  }
  ~ScaleSwap() {
    b.scale.p = saved;
    b.bmat_terms = 0;  // ... and the one staged now is not the unweighted one
  }
};

// out[0] = rhs . delta, out[1] = theta^T P theta, out[2] = theta^T P delta, out[3] = delta^T P delta
int step_dots(uint64_t p, const double *prec, const double *theta, const double *delta, const double *rhs,
              double *d_out, double *d_part) {
  return vsum<4>(p, [=] __device__(uint64_t k, double *acc) {
    const double t = theta[k], d = delta[k], pk = prec[k];
    acc[0] = fma(rhs[k], d, acc[0]);
    acc[1] = fma(pk * t, t, acc[1]);
    acc[2] = fma(pk * t, d, acc[2]);
    acc[3] = fma(pk * d, d, acc[3]);
  }, d_out, d_part);
}

// sum a l(y, saturated): what the deviance is measured from
int saturated_loglik(int family, uint64_t n, const double *y, const double *a, double *d_out, double *d_part) {
  return vsum<1>(n, [=] __device__(uint64_t i, double *acc) {
    const double yi = y[i], ai = a ? a[i] : 1.0;
    auto xlogx = [](double v) { return v > 0.0 ? v * log(v) : 0.0; };
    if (family == OBHIP_GLM_BINOMIAL) acc[0] += ai * (xlogx(yi) + xlogx(1.0 - yi));
    if (family == OBHIP_GLM_POISSON) acc[0] += ai * (xlogx(yi) - yi);
  }, d_out, d_part);
}

bool family_ok(int family) {
  return family == OBHIP_GLM_GAUSSIAN || family == OBHIP_GLM_BINOMIAL || family == OBHIP_GLM_POISSON;
}

int fit_glm_body(obhip_basis &b, obhip_terms &t, const obhip_model *m, int family, const double *d_y,
                 const double *d_a, const double *d_o, double sigma, double rho, double tol, uint64_t maxit,
                 double *d_H, double *d_theta, double *d_diagH, double *d_eta, obhip_glm_info *info, void *d_ws) {
  const uint64_t p = t.p, n = b.n;
  GlmWs w(d_ws, p, n);
  const double *d_prec = nullptr;
  OB_TRY(terms_prec_dev(m, t, rho, &d_prec));
  OB_TRY(t.prepare(b.md.cap, b.md.dims_h));
  double *theta = d_theta;
  GlmRows r;
  r.family = family;
  r.n = n;
  r.y = d_y;
  r.a = d_a;
  r.o = d_o;
  r.e2 = family == OBHIP_GLM_GAUSSIAN ? std::exp(-2.0 * sigma) : 1.0;
  r.scale = b.scale.p;
  double h[8];
  // the start: eta = o (+ B theta of the caller), its row pass and F
  if (info->warm_start) {
    OB_TRY(launch_mm(b, t, theta, w.bd, false));
    r.deta = w.bd;
    r.alpha = 1.0;
  } else {
    OB_TRY(launch_fill(theta, p, 0.0));
  }
  r.eta_out = w.eta;
  r.scale_w = w.scale_w;
  r.u = w.u;
  OB_TRY(launch_glm_rows(r, w.sums, w.part));
  OB_TRY(step_dots(p, d_prec, theta, theta, theta, w.sums + 4, w.part));
  OB_TRY(d2h(h, w.sums, sizeof(h)));
  if (h[2] != 0.0 || !std::isfinite(h[0]) || !std::isfinite(h[5]))
    return fail(OBHIP_ERR_NUMERIC, "fit_glm: the penalised log-likelihood is not finite at the start");
  double lik = h[0], mag = h[1] + 0.5 * h[5], F = lik - 0.5 * h[5];
  const double ubound = (double)(n + p + 16) * kU;
  info->converged = 0;
  info->iterations = info->halvings = 0;
  info->dec = 0.0;
  for (uint64_t it = 0; it < maxit; ++it) {
    {
      // H = B_w^T B_w + P (the sink forms it with e2 = 1) and g = B_w^T u, u riding the staging pass
      ScaleSwap swap(b, w.scale_w);
      GramSink sink;
      sink.out = d_H;
      sink.form = true;
      sink.e2 = 1.0;
      sink.prec = d_prec;
      sink.diagH = d_diagH;
      GramFuse fuse;
      fuse.y = w.u;
      fuse.g = w.g;
      OB_TRY(launch_gram_to(b, t, sink, &fuse));
      if (!fuse.done) OB_TRY(launch_tmm(b, t, w.u, w.g, false));
    }
    {
      const double *g = w.g;
      double *rhs = w.rhs;
      OB_TRY(vmap(p, [=] __device__(uint64_t k) { rhs[k] = g[k] - d_prec[k] * theta[k]; }));
    }
    OB_TRY(launch_newton_solve(p, d_H, w.rhs, w.delta, w.chol, newton_workspace_bytes(p)));
    OB_TRY(step_dots(p, d_prec, theta, w.delta, w.rhs, w.sums + 4, w.part));
    OB_TRY(launch_mm(b, t, w.delta, w.bd, false));
    OB_TRY(d2h(h + 4, w.sums + 4, 4 * sizeof(double)));
    const double dec = h[4], qtt = h[5], qtd = h[6], qdd = h[7];
    info->dec = dec;
    if (!std::isfinite(dec) || dec < 0.0)
      return fail(OBHIP_ERR_NUMERIC, "fit_glm: the Newton step is no ascent direction (g^T delta = " +
                                         std::to_string(dec) + ")");
    auto prior_at = [&](double alpha) { return 0.5 * (qtt + alpha * (2.0 * qtd + alpha * qdd)); };
    const bool last = dec <= tol * (1.0 + std::fabs(F));
    double alpha = 1.0;
    r.eta = w.eta;
    r.deta = w.bd;
    if (!last) {
      // trial steps: one row pass each, nothing written but the sums
      GlmRows tr = r;
      tr.eta_out = tr.mu = tr.scale_w = tr.u = nullptr;
      int k = 0;
      for (;; ++k) {
        if (k > kMaxHalvings) return fail(OBHIP_ERR_NUMERIC, "fit_glm: the line search found no step in 30 halvings");
        tr.alpha = alpha;
        OB_TRY(launch_glm_rows(tr, w.sums, w.part));
        OB_TRY(d2h(h, w.sums, 3 * sizeof(double)));
        const double pr = prior_at(alpha), Ft = h[0] - pr;
        if (h[2] == 0.0 && std::isfinite(Ft) && Ft >= F - ubound * (mag + h[1] + pr)) break;
        alpha *= 0.5;
        info->halvings += 1;
      }
    }
    // the step itself: theta, eta, and the weights and working column of the next Hessian
    {
      const double *dl = w.delta;
      const double al = alpha;
      OB_TRY(vmap(p, [=] __device__(uint64_t k) { theta[k] = fma(al, dl[k], theta[k]); }));
    }
    r.alpha = alpha;
    OB_TRY(launch_glm_rows(r, w.sums, w.part));
    OB_TRY(d2h(h, w.sums, 3 * sizeof(double)));
    const double pr = prior_at(alpha);
    info->iterations += 1;
    if (h[2] != 0.0 || !std::isfinite(h[0] - pr))
      return fail(OBHIP_ERR_NUMERIC, "fit_glm: the penalised log-likelihood is not finite after the last step");
    lik = h[0];
    mag = h[1] + pr;
    F = lik - pr;
    if (last) {
      info->converged = 1;
      break;
    }
  }
  OB_TRY(saturated_loglik(family, n, d_y, d_a, w.sums + 3, w.part));
  double lsat = 0.0;
  OB_TRY(d2h(&lsat, w.sums + 3, sizeof(double)));
  info->F = F;
  info->deviance = 2.0 * (lsat - lik);
  if (d_eta) OB_HIP(hipMemcpyAsync(d_eta, w.eta, n * sizeof(double), hipMemcpyDeviceToDevice, cur_stream()));
  return 0;
}

// y in its family's domain, weights finite and > 0, offsets finite (host buffers)
int check_glm_data(const char *who, int family, uint64_t n, const double *y, const double *a, const double *o) {
  for (uint64_t i = 0; i < n; ++i) {
    const double v = y[i];
    const bool ok = std::isfinite(v) && (family == OBHIP_GLM_GAUSSIAN || v >= 0.0) &&
                    (family != OBHIP_GLM_BINOMIAL || v <= 1.0);
    if (!ok) return fail(OBHIP_ERR_INVALID, std::string(who) + ": y is outside the family's domain at row " + std::to_string(i));
    if (a && !(std::isfinite(a[i]) && a[i] > 0.0))
      return fail(OBHIP_ERR_INVALID, std::string(who) + ": weights must be finite and > 0 (row " + std::to_string(i) + ")");
    if (o && !std::isfinite(o[i]))
      return fail(OBHIP_ERR_INVALID, std::string(who) + ": offsets must be finite (row " + std::to_string(i) + ")");
  }
  return 0;
}

}  // namespace

extern "C" {

int obhip_glm_workspace_bytes(uint64_t p, uint64_t n, uint64_t *bytes) {
  if (!bytes || p == 0 || n == 0) return fail(OBHIP_ERR_INVALID, "glm_workspace_bytes: bad argument");
  *bytes = GlmWs::doubles(p, n) * sizeof(double) + newton_workspace_bytes(p);
  return 0;
}

int obhip_glm_rows_dev(int family, uint64_t n, const double *d_eta, const double *d_deta, double alpha,
                       const double *d_y, const double *d_a, const double *d_o, double sigma, const double *d_scale,
                       double *d_eta_out, double *d_mu, double *d_scale_w, double *d_u, double *d_sums) {
  if (!family_ok(family)) return fail(OBHIP_ERR_INVALID, "glm_rows_dev: unknown family");
  if (n == 0 || !d_y || !d_sums) return fail(OBHIP_ERR_INVALID, "glm_rows_dev: null argument");
  const bool trial = !d_eta_out && !d_mu && !d_scale_w && !d_u;
  if (!trial && (!d_eta_out || !d_scale_w || !d_u || !d_scale))
    return fail(OBHIP_ERR_INVALID, "glm_rows_dev: d_eta_out, d_scale_w, d_u and d_scale go together (all NULL: a trial pass)");
  if (!std::isfinite(alpha) || (family == OBHIP_GLM_GAUSSIAN && !std::isfinite(sigma)))
    return fail(OBHIP_ERR_INVALID, "glm_rows_dev: alpha and sigma must be finite");
  OB_TRY(require_device());
  GlmRows r;
  r.family = family;
  r.n = n;
  r.eta = d_eta;
  r.deta = d_deta;
  r.alpha = alpha;
  r.y = d_y;
  r.a = d_a;
  r.o = d_o;
  r.e2 = family == OBHIP_GLM_GAUSSIAN ? std::exp(-2.0 * sigma) : 1.0;
  r.scale = d_scale;
  r.eta_out = d_eta_out;
  r.mu = d_mu;
  r.scale_w = d_scale_w;
  r.u = d_u;
  DevBuf<double> part;
  OB_TRY(part.alloc((size_t)kSumBlocks * kGlmSums));
  return launch_glm_rows(r, d_sums, part.p);
}

int obhip_fit_glm_dev(const obhip_basis *b, const obhip_terms *tc, const obhip_model *m, int family,
                      const double *d_y, const double *d_a, const double *d_o, double sigma, double rho, double tol,
                      uint64_t maxit, double *d_H, double *d_theta, double *d_diagH, double *d_eta,
                      obhip_glm_info *info, void *d_ws, uint64_t ws_bytes) {
  if (!b || !tc || !m || !d_y || !d_H || !d_theta || !info || !d_ws)
    return fail(OBHIP_ERR_INVALID, "fit_glm_dev: null argument");
  if (!family_ok(family)) return fail(OBHIP_ERR_INVALID, "fit_glm_dev: unknown family");
  if (maxit == 0 || !(tol >= 0.0) || !std::isfinite(tol) || !std::isfinite(rho) ||
      (family == OBHIP_GLM_GAUSSIAN && !std::isfinite(sigma)))
    return fail(OBHIP_ERR_INVALID, "fit_glm_dev: maxit >= 1, tol >= 0, finite sigma and rho");
  OB_TRY(check_compat(m, tc));
  if (b->model != m) return fail(OBHIP_ERR_INVALID, "fit_glm_dev: model / terms / basis do not belong together");
  if (b->n == 0) return fail(OBHIP_ERR_INVALID, "fit_glm_dev: the basis has no rows");
  uint64_t need = 0;
  OB_TRY(obhip_glm_workspace_bytes(tc->p, b->n, &need));
  if (ws_bytes < need) return fail(OBHIP_ERR_INVALID, "fit_glm_dev: workspace too small");
  OB_TRY(require_device());
  return fit_glm_body(*const_cast<obhip_basis *>(b), *const_cast<obhip_terms *>(tc), m, family, d_y, d_a, d_o, sigma,
                      rho, tol, maxit, d_H, d_theta, d_diagH, d_eta, info, d_ws);
}

int obhip_predict_glm_dev(const obhip_model *m, const obhip_terms *tc, int family, const double *d_theta,
                          const double *d_x, uint64_t n, const double *d_o, const double *d_coeffvar, double *d_eta,
                          double *d_vareta, double *d_mu, double *d_varmu) {
  if (!m || !tc || !d_theta || (n != 0 && !d_x)) return fail(OBHIP_ERR_INVALID, "predict_glm_dev: null argument");
  if (!family_ok(family)) return fail(OBHIP_ERR_INVALID, "predict_glm_dev: unknown family");
  const bool want_var = d_vareta || d_varmu;
  if (want_var && !d_coeffvar) return fail(OBHIP_ERR_INVALID, "predict_glm_dev: a variance needs d_coeffvar");
  OB_TRY(check_compat(m, tc));
  OB_TRY(require_device());
  if (n == 0) return 0;
  DevBuf<double> eta_tmp, var_tmp;
  if (!d_eta) {
    OB_TRY(eta_tmp.alloc(n));
    d_eta = eta_tmp.p;
  }
  if (want_var && !d_vareta) {
    OB_TRY(var_tmp.alloc(n));
    d_vareta = var_tmp.p;
  }
  // e^{2 sigma} = 0: the variance of the linear predictor, no noise term
  OB_TRY(launch_predict(*m, *const_cast<obhip_terms *>(tc), d_theta, d_x, n, d_eta, want_var ? d_coeffvar : nullptr,
                        0.0, want_var ? d_vareta : nullptr));
  return launch_glm_response(family, n, d_o, d_eta, d_vareta, d_mu, d_varmu);
}

int obhip_fit_glm(const obhip_basis *b, const obhip_terms *t, const obhip_model *m, int family, const double *y,
                  const double *a, const double *o, double sigma, double rho, double tol, uint64_t maxit,
                  double *theta, double *diagH, double *eta, obhip_glm_info *info) {
  if (!b || !t || !m || !y || !theta || !info) return fail(OBHIP_ERR_INVALID, "fit_glm: null argument");
  if (!family_ok(family)) return fail(OBHIP_ERR_INVALID, "fit_glm: unknown family");
  OB_TRY(check_glm_data("fit_glm", family, b->n, y, a, o));
  OB_TRY(check_compat(m, t));
  OB_TRY(require_device());
  const uint64_t p = t->p, n = b->n;
  DevBuf<double> dy, da, dof, dH, dth, ddiag, deta;
  DevBuf<char> ws;
  uint64_t wsb = 0;
  OB_TRY(obhip_glm_workspace_bytes(p, n, &wsb));
  OB_TRY(dy.upload(y, n));
  if (a) OB_TRY(da.upload(a, n));
  if (o) OB_TRY(dof.upload(o, n));
  OB_TRY(dH.alloc(p * p));
  if (info->warm_start) OB_TRY(dth.upload(theta, p));
  else OB_TRY(dth.alloc(p));
  OB_TRY(ddiag.alloc(p));
  OB_TRY(deta.alloc(n));
  OB_TRY(ws.alloc(wsb));
  OB_TRY(obhip_fit_glm_dev(b, t, m, family, dy.p, da.p, dof.p, sigma, rho, tol, maxit, dH.p, dth.p, ddiag.p, deta.p,
                           info, ws.p, wsb));
  OB_TRY(d2h(theta, dth.p, p * sizeof(double)));
  if (diagH) OB_TRY(d2h(diagH, ddiag.p, p * sizeof(double)));
  if (eta) OB_TRY(d2h(eta, deta.p, n * sizeof(double)));
  return 0;
}

int obhip_predict_glm(const obhip_model *m, const obhip_terms *t, int family, const double *theta, const double *x,
                      uint64_t n, uint64_t ldx, const double *o, const double *coeffvar, double *eta, double *vareta,
                      double *mu, double *varmu) {
  if (!m || !t || !theta || !x || n == 0 || ldx < n) return fail(OBHIP_ERR_INVALID, "predict_glm: bad argument");
  if (!family_ok(family)) return fail(OBHIP_ERR_INVALID, "predict_glm: unknown family");
  const bool want_var = vareta || varmu;
  if (want_var && !coeffvar) return fail(OBHIP_ERR_INVALID, "predict_glm: a variance needs coeffvar");
  OB_TRY(check_compat(m, t));
  OB_TRY(require_device());
  DevBuf<double> dx, dth, dof, dcv, deta, dve, dmu, dvm;
  OB_TRY(upload_cols(dx, x, n, m->d, ldx));
  OB_TRY(dth.upload(theta, t->p));
  if (o) OB_TRY(dof.upload(o, n));
  OB_TRY(deta.alloc(n));
  OB_TRY(dmu.alloc(n));
  if (want_var) {
    OB_TRY(dcv.upload(coeffvar, t->p));
    OB_TRY(dve.alloc(n));
    OB_TRY(dvm.alloc(n));
  }
  OB_TRY(obhip_predict_glm_dev(m, t, family, dth.p, dx.p, n, dof.p, dcv.p, deta.p, dve.p, dmu.p, dvm.p));
  if (eta) OB_TRY(d2h(eta, deta.p, n * sizeof(double)));
  if (mu) OB_TRY(d2h(mu, dmu.p, n * sizeof(double)));
  if (vareta) OB_TRY(d2h(vareta, dve.p, n * sizeof(double)));
  if (varmu) OB_TRY(d2h(varmu, dvm.p, n * sizeof(double)));
  return 0;
}

}  // extern "C"
