// The Newton fit of lpdfvec(loglik_std, logpr_gauss) on row-sharded data, start to finish on the
// device (lpdf::optnewton, src/fit.cpp:98-131, with obfit's standardisation of y,
// R/fitting.R:55-57, over the rows of ALL ranks), for one response or q of them over one design
// (the reference fits one y, R/fitting.R:40-120; the matrix forms it has are prodmm_ / tprodmm_,
// src/linalg.cpp:481-637).  ONE pipeline, fit_newton_body, behind obhip_fit_newton_sharded_dev
// (q = 1) and obhip_fit_newton_multi_dev; the streaming fit (normal_acc.cpp) takes its pieces.
//
// What crosses ranks:
//   (sum y, n)            16 bytes per response  -> the mean of y over all rows
//   sum (y - mean)^2       8 bytes per response  -> its standard deviation, two-pass like R's sd()
//   [packed upper triangle of G_r = B_r^T B_r | B_r^T Y_std,r]   p (p + 1) / 2 + p q doubles
// and what touches the p x p matrix on either side of the exchange is one pass each: the
// reduction of the Gram kernel's row-split partials writes the packed triangle straight into
// the exchange buffer, and the unpack forms H = e^{-2 sigma} G + diag(prior) while it restores
// the full symmetric storage the Cholesky wants.  With one rank (comm = NULL) the reduction
// writes H itself and nothing is exchanged.  Y is standardised BEFORE B^T Y is taken, so no
// B^T 1 pass and no cancellation in (B^T y - mean B^T 1).
//
// The model, the terms, sigma and rho are shared by the responses, every response is standardised
// on its own, so G, H and its Cholesky factor are formed ONCE and only what depends on Y is batched:
//   B^T Y      response 0 rides along the staging pass of the design matrix (GramFuse, else
//              launch_tmm); the others come from one pass of k_aty_multi over the staged matrix per
//              64 responses -- or, where the matrix is not resident as a whole (row chunks, Gram
//              backend 3) or fewer than kMultiMinCols columns are left, from a column loop over
//              launch_tmm (bty_columns);
//   the solves launch_newton_solve factorises with response 0's right-hand side; the other columns
//              go through the blocked substitutions of launch_trsm_multi on the finished factor
//              (solve_columns);
//   predict    k_predict_multi where the terms fit it and kMultiMinCols columns are left, a column
//              loop over launch_predict otherwise
//              (and for q = 1, which then is the single predictor bit for bit).
// Everything is column-major: Y n x q (ldy), Theta p x q, mean n_new x q.
#include <cmath>

#include "obhip_internal.h"
#include "vec_ops.h"

using namespace obhip;

namespace obhip {

int terms_prec_dev(const obhip_model *m, obhip_terms &t, double rho, const double **d_prec) {
  // uploaded when the model state or rho changed, otherwise already in HBM
  if (!t.prec_dev.p || t.prec_model != m || t.prec_version != m->version || t.prec_rho != rho) {
    const std::vector<double> prec = prior_prec(*m, t, rho);
    OB_TRY(t.prec_dev.upload(prec.data(), t.p));  // (synchronises: prec is a local)
    t.prec_model = m;
    t.prec_version = m->version;
    t.prec_rho = rho;
  }
  *d_prec = t.prec_dev.p;
  return 0;
}

int bty_columns(obhip_basis &b, obhip_terms &t, const double *d_Y, uint64_t ldy, uint64_t ncols, double *d_out) {
  if (ncols >= kMultiMinCols && b.bmat.p && t.uid != 0 && b.bmat_terms == t.uid)
    return launch_aty_multi(b, t, d_Y, ldy, ncols, d_out, t.p);
  // few columns, or the design matrix is not resident as a whole: one pass over the basis per response
  for (uint64_t j = 0; j < ncols; ++j) OB_TRY(launch_tmm(b, t, d_Y + j * ldy, d_out + j * t.p, false));
  return 0;
}

int solve_columns(uint64_t p, const double *d_H, const void *d_cholws, const double *d_R, uint64_t ncols, double e2,
                  double *d_Theta, void *d_scratch) {
  if (ncols == 0) return 0;
  return launch_trsm_multi(p, d_H, newton_workspace_iinv(p, d_cholws), d_R, p, ncols, e2, d_Theta, d_scratch);
}

}  // namespace obhip

namespace {

// Column j of Y (n x q, ldy) -> (y - cent_j) / sd_j with the mean and the n - 1 standard deviation
// over the rows of ALL ranks, d_meansd: q triples (cent, sd, n).  A rank may hold no rows (n = 0,
// null pointers): it takes part in both sums with zeros.
int standardise_cols(obhip_comm *comm, const double *d_Y_raw, uint64_t n, uint64_t q, uint64_t ldy, double *d_Y,
                     double *d_meansd) {
  DevBuf<double> stb, part;
  OB_TRY(stb.alloc(3 * q));  // [(sum, n) per column][sum of squares per column]
  OB_TRY(part.alloc((size_t)sum_blocks(n) * q));
  double *st = stb.p, *ss = stb.p + 2 * q;
  const double *yi = d_Y_raw;
  const double nrows = (double)n;
  OB_TRY(vcolsum(n, q, [=] __device__(int j, uint64_t i, double &acc) { acc += yi[(uint64_t)j * ldy + i]; },
                 [=] __device__(int j, double s) {
                   st[2 * j] = s;
                   st[2 * j + 1] = nrows;
                 },
                 part.p));
  if (comm) OB_TRY(comm_allreduce(comm, st, 2 * q));
  OB_TRY(vcolsum(n, q, [=] __device__(int j, uint64_t i, double &acc) {
    const double c = yi[(uint64_t)j * ldy + i] - st[2 * j] / st[2 * j + 1];
    acc = fma(c, c, acc);
  }, [=] __device__(int j, double s) { ss[j] = s; }, part.p));
  if (comm) OB_TRY(comm_allreduce(comm, ss, q));
  // (sum, n) and sum (y - cent)^2 over all ranks -> (cent, sd, n) per column
  double *ms = d_meansd;
  OB_TRY(vmap(q, [=] __device__(uint64_t j) {
    const double nt = st[2 * j + 1], cent = st[2 * j] / nt;
    ms[3 * j] = cent;
    ms[3 * j + 1] = sqrt(ss[j] / (nt - 1.0));  // n - 1 denominator (R's sd); n = 1 gives NaN as R's does
    ms[3 * j + 2] = nt;
  }));
  double *yo = d_Y;
  return vmap(n * q, [=] __device__(uint64_t e) {
    const uint64_t j = e / n, i = j * ldy + e % n;
    yo[i] = (yi[i] - ms[3 * j]) / ms[3 * j + 1];
  });
}

int destandardise_cols(double *d_V, uint64_t n, uint64_t q, uint64_t ldv, const double *d_meansd, bool sq) {
  const double *ms = d_meansd;
  return vmap(n * q, [=] __device__(uint64_t e) {
    const uint64_t j = e / n, i = j * ldv + e % n;
    const double sd = ms[3 * j + 1];
    d_V[i] = sq ? sd * sd * d_V[i] : fma(sd, d_V[i], ms[3 * j]);
  });
}

// The fit of q standardised responses (d_Y: n x q, ldy) after the entries' checks: Gram into its
// sink with B^T y_0 alongside, the other columns of B^T Y, exchange and unpack to
// H = e^{-2 sigma} G + prior with a communicator, Cholesky and the substitutions.  d_workspace:
// obhip_newton_workspace_bytes(p); d_multi_scratch: multi_solve_scratch_bytes(p), read only for q > 1.
int fit_newton_body(obhip_comm *comm, obhip_basis &b, obhip_terms &t, const obhip_model *m, const double *d_Y,
                    uint64_t q, uint64_t ldy, double sigma, double rho, double *d_H, double *d_G_rhs,
                    double *d_Theta, double *d_diagH, double *d_exbuf, uint64_t exbuf_count, void *d_workspace,
                    void *d_multi_scratch) {
  const uint64_t p = t.p, tri = p * (p + 1) / 2;
  double *d_rhs = (double *)d_workspace + p;
  void *d_cholws = d_rhs + p;
  const double e2 = std::exp(-2.0 * sigma);
  const double *d_prec = nullptr;
  OB_TRY(terms_prec_dev(m, t, rho, &d_prec));
  GramSink sink;
  if (comm) {
    sink.out = d_exbuf;
    sink.packed = true;
  } else {
    sink.out = d_H;
    sink.form = true;
    sink.e2 = e2;
    sink.prec = d_prec;
    sink.diagH = d_diagH;
  }
  // B^T Y lands behind the packed triangle of a sharded fit.  Response 0 is taken along by the
  // staging pass of the design matrix when there is one (its products are the entries of B), by
  // its own pass over the basis otherwise
  double *g_dst = comm ? d_exbuf + tri : d_G_rhs;
  GramFuse fuse;
  fuse.y = d_Y;
  fuse.g = g_dst;
  OB_TRY(launch_gram_to(b, t, sink, &fuse));
  if (!fuse.done) OB_TRY(launch_tmm(b, t, d_Y, g_dst, false));
  OB_TRY(bty_columns(b, t, d_Y + ldy, ldy, q - 1, g_dst + p));
  if (comm) {
    {
      ProfScope ps("exchange");
      OB_TRY(comm_allreduce(comm, d_exbuf, exbuf_count));
    }
    {
      ProfScope ps("unpack_form");
      OB_TRY(launch_unpack_tri(p, d_exbuf, nullptr, d_H, true, e2, d_prec, d_diagH));
    }
    OB_HIP(hipMemcpyAsync(d_G_rhs, d_exbuf + tri, p * q * sizeof(double), hipMemcpyDeviceToDevice, cur_stream()));
  }
  // grad at coeff = 0: e^{-2 sigma} B^T y   (loglik_std.cpp:113-116)
  const double *g = d_G_rhs;
  OB_TRY(vmap(p, [=] __device__(uint64_t k) { d_rhs[k] = e2 * g[k]; }));
  OB_TRY(launch_newton_solve(p, d_H, d_rhs, d_Theta, d_cholws, newton_workspace_bytes(p)));
  return solve_columns(p, d_H, d_cholws, d_G_rhs + p, q - 1, e2, d_Theta + p, d_multi_scratch);
}

}  // namespace

extern "C" {

int obhip_standardise_dev(obhip_comm *comm, const double *d_y_raw, uint64_t n, double *d_y,
                          double *d_meansd) {
  // A rank of a sharded job may hold no rows (fewer rows than ranks, a ragged last shard): it
  // must still take part in the two sums or its peers wait for ever, so with a communicator
  // n = 0 is legal and contributes (0, 0) and 0.  Fewer than two rows over ALL ranks give
  // sd = NaN, as R's sd() does (the count is known on the device only: rejecting it here would
  // put a host synchronisation into every fit).
  if (!d_meansd || (n != 0 && (!d_y_raw || !d_y))) return fail(OBHIP_ERR_INVALID, "standardise_dev: null argument");
  OB_TRY(require_device());
  if (!comm && n < 2) return fail(OBHIP_ERR_INVALID, "standardise_dev: the standard deviation needs two rows");
  return standardise_cols(comm, d_y_raw, n, 1, n, d_y, d_meansd);
}

int obhip_standardise_multi_dev(obhip_comm *comm, const double *d_Y_raw, uint64_t n, uint64_t q, uint64_t ldy,
                                double *d_Y, double *d_meansd) {
  if (!d_meansd || q == 0 || q > 65535 || (n != 0 && (!d_Y_raw || !d_Y || ldy < n)))
    return fail(OBHIP_ERR_INVALID, "standardise_multi_dev: bad argument");
  OB_TRY(require_device());
  if (!comm && n < 2) return fail(OBHIP_ERR_INVALID, "standardise_multi_dev: the standard deviation needs two rows");
  return standardise_cols(comm, d_Y_raw, n, q, ldy, d_Y, d_meansd);
}

int obhip_destandardise_dev(double *d_v, uint64_t n, const double *d_meansd) {
  if (!d_v || !d_meansd) return fail(OBHIP_ERR_INVALID, "destandardise_dev: null argument");
  return destandardise_cols(d_v, n, 1, n, d_meansd, false);
}

int obhip_destandardise_multi_dev(double *d_V, uint64_t n, uint64_t q, uint64_t ldv, const double *d_meansd,
                                  int squared) {
  if (!d_meansd || (n != 0 && (!d_V || ldv < n))) return fail(OBHIP_ERR_INVALID, "destandardise_multi_dev: bad argument");
  return destandardise_cols(d_V, n, q, ldv, d_meansd, squared != 0);
}

int obhip_fit_newton_count(uint64_t p, int nranks, uint64_t *count) {
  if (!count || nranks < 1 || p == 0) return fail(OBHIP_ERR_INVALID, "fit_newton_count: bad argument");
  return obhip_fit_newton_multi_count(p, 1, nranks, count);
}

int obhip_fit_newton_multi_count(uint64_t p, uint64_t q, int nranks, uint64_t *count) {
  if (!count || nranks < 1 || p == 0 || q == 0) return fail(OBHIP_ERR_INVALID, "fit_newton_multi_count: bad argument");
  const uint64_t raw = p * (p + 1) / 2 + p * q;
  const uint64_t blk = 2 * (uint64_t)nranks;  // equal 16-byte blocks for reduce-scatter
  *count = (raw + blk - 1) / blk * blk;
  return 0;
}

int obhip_newton_multi_workspace_bytes(uint64_t p, uint64_t q, uint64_t *bytes) {
  if (!bytes || p == 0 || q == 0) return fail(OBHIP_ERR_INVALID, "newton_multi_workspace_bytes: bad argument");
  uint64_t single = 0;
  OB_TRY(obhip_newton_workspace_bytes(p, &single));
  // the right-hand sides of one chunk of responses in two copies, whatever q is
  *bytes = single + multi_solve_scratch_bytes(p);
  return 0;
}

int obhip_fit_newton_sharded_dev(obhip_comm *comm, const obhip_basis *b, const obhip_terms *tc,
                                 const obhip_model *m, const double *d_y, double sigma, double rho,
                                 double *d_H, double *d_g, double *d_theta, double *d_diagH,
                                 double *d_exbuf, uint64_t exbuf_count, void *d_workspace,
                                 uint64_t workspace_bytes) {
  if (!b || !tc || !m || !d_y || !d_H || !d_g || !d_theta || !d_workspace)
    return fail(OBHIP_ERR_INVALID, "fit_newton_sharded_dev: null argument");
  OB_TRY(require_device());
  // (knots set, same dimensions, no level beyond the model's knots: term_var indexes the model's
  // tables with the terms' levels)
  OB_TRY(check_compat(m, tc));
  if (b->model != m) return fail(OBHIP_ERR_INVALID, "fit_newton_sharded_dev: model / terms / basis do not belong together");
  uint64_t need = 0;
  obhip_newton_workspace_bytes(tc->p, &need);
  if (workspace_bytes < need) return fail(OBHIP_ERR_INVALID, "fit_newton_sharded_dev: workspace too small");
  if (comm) {
    uint64_t cnt = 0;
    OB_TRY(obhip_fit_newton_count(tc->p, comm_nranks(comm), &cnt));
    if (!d_exbuf || exbuf_count < cnt) return fail(OBHIP_ERR_INVALID, "fit_newton_sharded_dev: exchange buffer too small");
    exbuf_count = cnt;
  }
  return fit_newton_body(comm, *const_cast<obhip_basis *>(b), *const_cast<obhip_terms *>(tc), m, d_y, 1, b->n, sigma,
                         rho, d_H, d_g, d_theta, d_diagH, d_exbuf, exbuf_count, d_workspace, nullptr);
}

int obhip_fit_newton_multi_dev(obhip_comm *comm, const obhip_basis *b, const obhip_terms *tc, const obhip_model *m,
                               const double *d_Y, uint64_t q, uint64_t ldy, double sigma, double rho, double *d_H,
                               double *d_G_rhs, double *d_Theta, double *d_diagH, double *d_exbuf,
                               uint64_t exbuf_count, void *d_workspace, uint64_t workspace_bytes) {
  if (!b || !tc || !m || !d_Y || !d_H || !d_G_rhs || !d_Theta || !d_workspace || q == 0)
    return fail(OBHIP_ERR_INVALID, "fit_newton_multi_dev: bad argument");
  OB_TRY(require_device());
  OB_TRY(check_compat(m, tc));
  if (b->model != m) return fail(OBHIP_ERR_INVALID, "fit_newton_multi_dev: model / terms / basis do not belong together");
  if (ldy < b->n) return fail(OBHIP_ERR_INVALID, "fit_newton_multi_dev: ldy is smaller than the rows of the basis");
  uint64_t need = 0, single = 0;
  OB_TRY(obhip_newton_multi_workspace_bytes(tc->p, q, &need));
  OB_TRY(obhip_newton_workspace_bytes(tc->p, &single));
  if (workspace_bytes < need) return fail(OBHIP_ERR_INVALID, "fit_newton_multi_dev: workspace too small");
  if (comm) {
    uint64_t cnt = 0;
    OB_TRY(obhip_fit_newton_multi_count(tc->p, q, comm_nranks(comm), &cnt));
    if (!d_exbuf || exbuf_count < cnt) return fail(OBHIP_ERR_INVALID, "fit_newton_multi_dev: exchange buffer too small");
    exbuf_count = cnt;
  }
  return fit_newton_body(comm, *const_cast<obhip_basis *>(b), *const_cast<obhip_terms *>(tc), m, d_Y, q, ldy, sigma,
                         rho, d_H, d_G_rhs, d_Theta, d_diagH, d_exbuf, exbuf_count, d_workspace,
                         (char *)d_workspace + single);
}

int obhip_newton_multi_solve_dev(const obhip_model *m, const obhip_terms *t, double *d_G, const double *d_G_rhs,
                                 uint64_t q, double sigma, double rho, double *d_Theta, double *d_diagH,
                                 void *d_workspace, uint64_t workspace_bytes) {
  if (!m || !t || !d_G || !d_G_rhs || !d_Theta || !d_workspace || q == 0)
    return fail(OBHIP_ERR_INVALID, "newton_multi_solve_dev: bad argument");
  OB_TRY(check_compat(m, t));
  const uint64_t p = t->p;
  uint64_t need = 0, single = 0;
  OB_TRY(obhip_newton_multi_workspace_bytes(p, q, &need));
  OB_TRY(obhip_newton_workspace_bytes(p, &single));
  if (workspace_bytes < need) return fail(OBHIP_ERR_INVALID, "newton_multi_solve_dev: workspace too small");
  // H, the factorisation and response 0 by the single-response entry; the factor stays in d_G
  OB_TRY(obhip_newton_solve_dev(m, t, d_G, d_G_rhs, sigma, rho, d_Theta, d_diagH, d_workspace, single));
  return solve_columns(p, d_G, (double *)d_workspace + 2 * p, d_G_rhs + p, q - 1, std::exp(-2.0 * sigma), d_Theta + p,
                       (char *)d_workspace + single);
}

int obhip_predict_multi_dev(const obhip_model *m, const obhip_terms *tc, const double *d_Theta, uint64_t q,
                            const double *d_x, uint64_t n, double *d_mean, const double *d_coeffvar, double sigma,
                            double *d_var) {
  if (!m || !tc || !d_Theta || q == 0 || (n != 0 && (!d_x || !d_mean)))
    return fail(OBHIP_ERR_INVALID, "predict_multi_dev: bad argument");
  OB_TRY(check_compat(m, tc));
  OB_TRY(require_device());
  if (n == 0) return 0;
  obhip_terms &t = *const_cast<obhip_terms *>(tc);
  const double e2s = std::exp(2.0 * sigma);
  const uint64_t p = t.p;
  // response 0 by the single predictor: it prepares the terms' device tables and, when asked,
  // gives the variance, which is the same for every response in standardised units
  OB_TRY(launch_predict(*m, t, d_Theta, d_x, n, d_mean, d_coeffvar, e2s, d_var));
  if (q == 1) return 0;
  if (q - 1 >= kMultiMinCols && predict_multi_supports(t)) return launch_predict_multi(*m, t, d_Theta + p, q - 1, d_x, n, d_mean + n);
  for (uint64_t j = 1; j < q; ++j)
    OB_TRY(launch_predict(*m, t, d_Theta + j * p, d_x, n, d_mean + j * n, nullptr, e2s, nullptr));
  return 0;
}

int obhip_fit_newton_multi(const obhip_basis *b, const obhip_terms *t, const obhip_model *m, const double *Y,
                           uint64_t q, uint64_t ldy, double sigma, double rho, double *Theta, double *diagH) {
  if (!b || !t || !m || !Y || !Theta || q == 0 || ldy < b->n)
    return fail(OBHIP_ERR_INVALID, "fit_newton_multi: bad argument");
  OB_TRY(check_compat(m, t));
  OB_TRY(require_device());
  const uint64_t p = t->p;
  DevBuf<double> dY, dH, dg, dth, ddiag;
  DevBuf<char> ws;
  uint64_t wsb = 0;
  OB_TRY(obhip_newton_multi_workspace_bytes(p, q, &wsb));
  OB_TRY(upload_cols(dY, Y, b->n, q, ldy));
  OB_TRY(dH.alloc(p * p));
  OB_TRY(dg.alloc(p * q));
  OB_TRY(dth.alloc(p * q));
  OB_TRY(ddiag.alloc(p));
  OB_TRY(ws.alloc(wsb));
  OB_TRY(obhip_fit_newton_multi_dev(nullptr, b, t, m, dY.p, q, b->n, sigma, rho, dH.p, dg.p, dth.p, ddiag.p,
                                    nullptr, 0, ws.p, wsb));
  OB_TRY(d2h(Theta, dth.p, p * q * sizeof(double)));
  if (diagH) OB_TRY(d2h(diagH, ddiag.p, p * sizeof(double)));
  return 0;
}

int obhip_predict_multi(const obhip_model *m, const obhip_terms *t, const double *Theta, uint64_t q, const double *x,
                        uint64_t n, uint64_t ldx, double *mean, const double *coeffvar, double sigma, double *var) {
  if (!m || !t || !Theta || !x || !mean || q == 0 || n == 0 || ldx < n)
    return fail(OBHIP_ERR_INVALID, "predict_multi: bad argument");
  OB_TRY(check_compat(m, t));
  OB_TRY(require_device());
  DevBuf<double> dx, dth, dmean, dcv, dvar;
  OB_TRY(upload_cols(dx, x, n, m->d, ldx));
  OB_TRY(dth.upload(Theta, t->p * q));
  OB_TRY(dmean.alloc(n * q));
  const bool do_var = coeffvar && var;
  if (do_var) {
    OB_TRY(dcv.upload(coeffvar, t->p));
    OB_TRY(dvar.alloc(n));
  }
  OB_TRY(obhip_predict_multi_dev(m, t, dth.p, q, dx.p, n, dmean.p, do_var ? dcv.p : nullptr, sigma,
                                 do_var ? dvar.p : nullptr));
  OB_TRY(d2h(mean, dmean.p, n * q * sizeof(double)));
  if (do_var) OB_TRY(d2h(var, dvar.p, n * sizeof(double)));
  return 0;
}

}  // extern "C"
