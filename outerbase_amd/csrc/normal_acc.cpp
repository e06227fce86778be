// Streaming Newton fit (no reference counterpart: obfit, R/fitting.R:40-120, takes all rows at
// once).  An obhip_normal_acc keeps the sufficient statistics of lpdfvec(loglik_std, logpr_gauss)'s
// Newton step for the rows it has been given -- the packed upper triangle of G = B^T B, B^T (Y - c),
// B^T 1 and per response (c, mean - c, M2, n), one device buffer laid out as kernels_acc.hip says --
// so that rows are passed over once, ever:
//   add / remove   the batch's Gram goes through launch_gram_to with a packed sink into scratch,
//                  B^T [Y - c | 1] as fit_newton.cpp forms B^T Y (column 0 with the staging pass, the
//                  others by bty_columns), then one fold with the sign;
//   grid batch     the na nb pairs of two input blocks: the triangle from the Hadamard product of the two sides'
//                  Grams, the rest as product_fit.cpp forms it;
//   combine        the same fold of one accumulator into another;
//   solve          H = e^{-2 sigma} (T - T_minus) + diag(prec) unpacked from the triangle(s), the
//                  moments of the remaining rows and the right-hand sides standardised AFTER the sum,
//                  B^T ((y - cent) / sd) = (B^T y - cent B^T 1) / sd, then launch_newton_solve and the
//                  batched substitutions of the multi-response fit.  Neither state is written.
// G depends on the model's hyper-parameters, so a state is tied to the model version of its first
// batch.  Every check that can refuse a call runs before the first launch: a refused call leaves the
// accumulator as it was.
#include <algorithm>
#include <cmath>
#include <new>
#include <string>

#include "obhip_internal.h"
#include "vec_ops.h"

using namespace obhip;

struct obhip_normal_acc {
  const obhip_model *model = nullptr;
  const obhip_terms *terms = nullptr;
  uint64_t p = 0, q = 0;
  uint64_t rows = 0, batches = 0;
  uint64_t geq = 0, gbatches = 0;  // gradient equations (rows x differentiated dimensions) and their batches
  uint64_t version = 0;  // of the model when the first batch came in (rows > 0 or geq > 0)
  DevBuf<double> st;     // [tri][R p x q][b1 p][moments 4 q]
  // lends the Gram of staged rows (gradient rows, the sides of a grid batch) its device, workspace and task-table
  // cache; it never has rows of its own, and the staged buffer is never its bmat
  std::unique_ptr<obhip_basis> gholder;
};

namespace {

constexpr uint64_t kMaxResponses = 65534;  // grid.y of the column passes holds q + 1

uint64_t state_count(uint64_t p, uint64_t q) { return p * (p + 1) / 2 + p * q + p + 4 * q; }

int zero_state(obhip_normal_acc *a) {
  OB_HIP(hipMemsetAsync(a->st.p, 0, a->st.n * sizeof(double), cur_stream()));
  a->rows = a->batches = 0;
  a->geq = a->gbatches = 0;
  return 0;
}

// the same term set: one handle, or two uploads of the same levels
bool same_terms(const obhip_terms *a, const obhip_terms *b) {
  return a == b || (a->p == b->p && a->d == b->d && a->lev == b->lev);
}

// the model must be what it was when the state's first rows came in
int check_version(const obhip_normal_acc *a, const char *who) {
  if ((a->rows > 0 || a->geq > 0) && a->version != a->model->version)
    return fail(OBHIP_ERR_STATE, std::string(who) +
                                     ": the model's hyper-parameters or knots changed since the accumulator's first "
                                     "batch (G depends on them): reset it and add the rows again");
  return 0;
}

// after rows or gradient equations left.  Nothing of either kind left: the sums are rounding residue of what
// was there, the state starts afresh.  No value rows left beside gradient rows: B^T 1 and the moments are
// such residue (the next value batch brings its own shift)
int after_removal(obhip_normal_acc *a) {
  if (a->rows == 0 && a->geq == 0) return zero_state(a);
  if (a->rows == 0) {
    const uint64_t head = a->p * (a->p + 1) / 2 + a->p * a->q;
    OB_HIP(hipMemsetAsync(a->st.p + head, 0, (a->st.n - head) * sizeof(double), cur_stream()));
    a->batches = 0;
  }
  return 0;
}

// the basis that lends gram_of_staged its device, workspace and task-table cache
int ensure_holder(obhip_normal_acc *a, const char *who) {
  if (a->gholder) return 0;
  a->gholder.reset(new (std::nothrow) obhip_basis());
  if (!a->gholder) return fail(OBHIP_ERR_INVALID, std::string(who) + ": out of host memory");
  a->gholder->model = a->model;
  a->gholder->d = a->model->d;
  (void)hipGetDevice(&a->gholder->device);
  return 0;
}

}  // namespace

extern "C" {

int obhip_normal_acc_bytes(uint64_t p, uint64_t q, uint64_t *bytes) {
  if (!bytes || p == 0 || q == 0 || q > kMaxResponses) return fail(OBHIP_ERR_INVALID, "normal_acc_bytes: bad argument");
  *bytes = state_count(p, q) * sizeof(double);
  return 0;
}

int obhip_normal_acc_create(obhip_normal_acc **out, const obhip_model *m, const obhip_terms *t, uint64_t q) {
  if (!out || !m || !t || q == 0 || q > kMaxResponses) return fail(OBHIP_ERR_INVALID, "normal_acc_create: bad argument");
  OB_TRY(check_compat(m, t));
  OB_TRY(require_device());
  obhip_normal_acc *a = new (std::nothrow) obhip_normal_acc();
  if (!a) return fail(OBHIP_ERR_INVALID, "normal_acc_create: out of host memory");
  a->model = m;
  a->terms = t;
  a->p = t->p;
  a->q = q;
  int rc = a->st.alloc(state_count(a->p, q));
  if (!rc) rc = zero_state(a);
  if (rc) {
    delete a;
    return rc;
  }
  *out = a;
  return 0;
}

int obhip_normal_acc_destroy(obhip_normal_acc *acc) {
  delete acc;
  return 0;
}

int obhip_normal_acc_reset(obhip_normal_acc *acc) {
  if (!acc) return fail(OBHIP_ERR_INVALID, "normal_acc_reset: null argument");
  return zero_state(acc);
}

int obhip_normal_acc_info(const obhip_normal_acc *acc, uint64_t *p, uint64_t *q, uint64_t *rows, uint64_t *batches) {
  if (!acc) return fail(OBHIP_ERR_INVALID, "normal_acc_info: null argument");
  if (p) *p = acc->p;
  if (q) *q = acc->q;
  if (rows) *rows = acc->rows;
  if (batches) *batches = acc->batches;
  return 0;
}

int obhip_normal_acc_export_dev(const obhip_normal_acc *acc, double *d_out, uint64_t count) {
  if (!acc || !d_out) return fail(OBHIP_ERR_INVALID, "normal_acc_export_dev: null argument");
  if (count < acc->st.n) return fail(OBHIP_ERR_INVALID, "normal_acc_export_dev: buffer too small");
  OB_HIP(hipMemcpyAsync(d_out, acc->st.p, acc->st.n * sizeof(double), hipMemcpyDeviceToDevice, cur_stream()));
  return 0;
}

int obhip_normal_acc_add_dev(obhip_normal_acc *acc, const obhip_basis *bc, const double *d_Y_raw, uint64_t ldy,
                             int sign) {
  if (!acc || !bc || (sign != 1 && sign != -1)) return fail(OBHIP_ERR_INVALID, "normal_acc_add_dev: bad argument");
  if (bc->model != acc->model)
    return fail(OBHIP_ERR_INVALID, "normal_acc_add_dev: the basis was built on another model than the accumulator");
  const uint64_t n = bc->n, p = acc->p, q = acc->q;
  if (n == 0) return 0;
  if (!d_Y_raw || ldy < n) return fail(OBHIP_ERR_INVALID, "normal_acc_add_dev: Y is null or ldy below the rows of the basis");
  OB_TRY(check_compat(acc->model, acc->terms));
  OB_TRY(check_version(acc, "normal_acc_add_dev"));
  if (bc->md.model_version != acc->model->version)
    return fail(OBHIP_ERR_STATE, "normal_acc_add_dev: the basis was built before the model last changed");
  if (sign < 0 && n > acc->rows)
    return fail(OBHIP_ERR_STATE, "normal_acc_add_dev: removing " + std::to_string(n) + " rows from an accumulator that holds " +
                                     std::to_string(acc->rows));
  OB_TRY(require_device());
  obhip_terms &t = *const_cast<obhip_terms *>(acc->terms);
  obhip_basis &b = *const_cast<obhip_basis *>(bc);
  const uint64_t tri = p * (p + 1) / 2, nrb = p * (q + 1);
  DevBuf<double> scratch, Ys, part;
  OB_TRY(scratch.alloc(state_count(p, q)));
  OB_TRY(Ys.alloc(n * (q + 1)));
  OB_TRY(part.alloc(kSumBlocks * q));
  const bool empty = acc->rows == 0;
  double *s_rb = scratch.p + tri, *s_mom = scratch.p + tri + nrb;
  OB_TRY(launch_acc_batch_moments(d_Y_raw, ldy, n, q, empty, acc->st.p + tri + nrb, s_mom, Ys.p, part.p));
  GramSink sink;
  sink.out = scratch.p;
  sink.packed = true;
  GramFuse fuse;
  fuse.y = Ys.p;
  fuse.g = s_rb;
  OB_TRY(launch_gram_to(b, t, sink, &fuse));
  // column 0 as the single fit takes it: with the staging pass, or by its own pass over the basis
  if (!fuse.done) OB_TRY(launch_tmm(b, t, Ys.p, s_rb, false));
  // columns 1 .. q - 1 of Y - c, then the ones column: B^T 1
  OB_TRY(bty_columns(b, t, Ys.p + n, n, q, s_rb + p));
  OB_TRY(launch_acc_fold(p, q, acc->st.p, scratch.p, empty, (double)sign));
  if (empty && acc->geq == 0) acc->version = acc->model->version;
  if (sign > 0) {
    acc->rows += n;
    acc->batches += 1;
  } else {
    acc->rows -= n;
    acc->batches -= acc->batches > 0 ? 1 : 0;
    OB_TRY(after_removal(acc));
  }
  return 0;
}

int obhip_normal_acc_add_grad_dev(obhip_normal_acc *acc, const double *d_x, uint64_t n, const uint32_t *dims,
                                  uint64_t ndims, const double *weights, const double *d_dY_raw, uint64_t lddy,
                                  int sign) {
  if (!acc || !dims || (sign != 1 && sign != -1) || (n > 0 && (!d_x || !d_dY_raw)))
    return fail(OBHIP_ERR_INVALID, "normal_acc_add_grad_dev: null accumulator, x, dims or dY, or a sign other than +1 / -1");
  OB_TRY(check_grad_dims("normal_acc_add_grad_dev", acc->model->d, dims, ndims, weights));
  if (lddy < n) return fail(OBHIP_ERR_INVALID, "normal_acc_add_grad_dev: lddy below the rows of the batch");
  if (n > kMaxRowsPerCall) return fail(OBHIP_ERR_INVALID, "normal_acc_add_grad_dev: more than 2^40 rows in one call");
  if (n == 0) return 0;
  OB_TRY(check_compat(acc->model, acc->terms));
  OB_TRY(check_version(acc, "normal_acc_add_grad_dev"));
  const uint64_t eq = n * ndims;
  if (sign < 0 && eq > acc->geq)
    return fail(OBHIP_ERR_STATE, "normal_acc_add_grad_dev: removing " + std::to_string(eq) +
                                     " gradient equations from an accumulator that holds " + std::to_string(acc->geq));
  OB_TRY(require_device());
  OB_TRY(ensure_holder(acc, "normal_acc_add_grad_dev"));
  const uint64_t p = acc->p, q = acc->q, tri = p * (p + 1) / 2;
  DevBuf<double> scratch;
  OB_TRY(scratch.alloc(tri + p * q));
  // sum_l w_l D_l^T D_l to the triangle, sum_l w_l D_l^T g_l (raw g: k_acc_rhs divides by sd) to R; nothing
  // to B^T 1 and the moments -- the gradient has no offset
  OB_TRY(grad_batch_normal_eq(*acc->gholder, *acc->model, *const_cast<obhip_terms *>(acc->terms), d_x, n, dims, weights,
                              ndims, d_dY_raw, lddy, q, scratch.p, scratch.p + tri));
  OB_TRY(launch_acc_fold_grad(p, q, acc->st.p, scratch.p, (double)sign));
  if (acc->rows == 0 && acc->geq == 0) acc->version = acc->model->version;
  if (sign > 0) {
    acc->geq += eq;
    acc->gbatches += 1;
  } else {
    acc->geq -= eq;
    acc->gbatches -= acc->gbatches > 0 ? 1 : 0;
    OB_TRY(after_removal(acc));
  }
  return 0;
}

int obhip_normal_acc_add_product_dev(obhip_normal_acc *acc, const double *d_xa, uint64_t na, const double *d_xb,
                                     uint64_t nb, const uint32_t *dims_b, uint64_t ndims_b, const double *d_Y_raw,
                                     uint64_t lda, int sign) {
  if (!acc || (sign != 1 && sign != -1))
    return fail(OBHIP_ERR_INVALID, "normal_acc_add_product_dev: null accumulator, or a sign other than +1 / -1");
  ProductSplit s;
  OB_TRY(make_split("normal_acc_add_product_dev", *acc->terms, dims_b, ndims_b, s));
  OB_TRY(check_side_columns("normal_acc_add_product_dev", s));
  if (na == 0 || nb == 0) return fail(OBHIP_ERR_INVALID, "normal_acc_add_product_dev: a grid batch needs rows on both sides");
  if (!d_xa || !d_xb || !d_Y_raw) return fail(OBHIP_ERR_INVALID, "normal_acc_add_product_dev: null xa, xb or Y");
  if (lda < na) return fail(OBHIP_ERR_INVALID, "normal_acc_add_product_dev: lda below na");
  if (na > (1ull << 31) || nb > kMaxRowsPerCall || na * nb > (1ull << 48))
    return fail(OBHIP_ERR_INVALID, "normal_acc_add_product_dev: more than 2^31 rows in xa, 2^40 in xb or 2^48 pairs");
  OB_TRY(check_compat(acc->model, acc->terms));
  OB_TRY(check_version(acc, "normal_acc_add_product_dev"));
  const uint64_t n = na * nb;
  if (sign < 0 && n > acc->rows)
    return fail(OBHIP_ERR_STATE, "normal_acc_add_product_dev: removing " + std::to_string(n) +
                                     " rows from an accumulator that holds " + std::to_string(acc->rows));
  OB_TRY(require_device());
  OB_TRY(ensure_holder(acc, "normal_acc_add_product_dev"));
  const uint64_t p = acc->p, q = acc->q, tri = p * (p + 1) / 2, nrb = p * (q + 1);
  const uint64_t tri2 = (tri + 1) & ~1ull;  // the second triangle on a 16-byte boundary as well
  DevBuf<double> scratch;
  OB_TRY(scratch.alloc(2 * tri2 + nrb + 4 * q));
  const bool empty = acc->rows == 0;
  double *s_ga = scratch.p, *s_gb = scratch.p + tri2, *s_tail = scratch.p + 2 * tri2;
  OB_TRY(product_batch_normal_eq(*acc->gholder, *acc->model, *const_cast<obhip_terms *>(acc->terms), s, d_xa, na, d_xb, nb,
                                 d_Y_raw, lda, q, empty, acc->st.p + tri + nrb, s_ga, s_gb, s_tail));
  {
    // B^T B = (At^T At) o (Bt^T Bt), folded from the two factors; [R | b1 | moments] as a row batch's
    ProfScope ps("product_fit_fold");
    OB_TRY(launch_acc_fold_hadamard(p, acc->st.p, s_ga, s_gb, (double)sign));
    OB_TRY(launch_acc_fold_tail(p, q, acc->st.p + tri, s_tail, empty, (double)sign));
  }
  if (empty && acc->geq == 0) acc->version = acc->model->version;
  if (sign > 0) {
    acc->rows += n;
    acc->batches += 1;
  } else {
    acc->rows -= n;
    acc->batches -= acc->batches > 0 ? 1 : 0;
    OB_TRY(after_removal(acc));
  }
  return 0;
}

int obhip_normal_acc_grad_info(const obhip_normal_acc *acc, uint64_t *grad_equations, uint64_t *grad_batches) {
  if (!acc) return fail(OBHIP_ERR_INVALID, "normal_acc_grad_info: null argument");
  if (grad_equations) *grad_equations = acc->geq;
  if (grad_batches) *grad_batches = acc->gbatches;
  return 0;
}

int obhip_normal_acc_combine_dev(obhip_normal_acc *dst, const obhip_normal_acc *src, int sign) {
  if (!dst || !src || (sign != 1 && sign != -1)) return fail(OBHIP_ERR_INVALID, "normal_acc_combine_dev: bad argument");
  if (dst == src) return fail(OBHIP_ERR_INVALID, "normal_acc_combine_dev: an accumulator cannot be combined with itself");
  if (dst->model != src->model || !same_terms(dst->terms, src->terms) || dst->p != src->p || dst->q != src->q)
    return fail(OBHIP_ERR_INVALID, "normal_acc_combine_dev: the accumulators differ in model, terms or responses");
  if (src->rows == 0 && src->geq == 0) return 0;
  OB_TRY(check_version(dst, "normal_acc_combine_dev"));
  OB_TRY(check_version(src, "normal_acc_combine_dev"));
  if (sign < 0 && src->rows > dst->rows)
    return fail(OBHIP_ERR_STATE, "normal_acc_combine_dev: removing " + std::to_string(src->rows) +
                                     " rows from an accumulator that holds " + std::to_string(dst->rows));
  if (sign < 0 && src->geq > dst->geq)
    return fail(OBHIP_ERR_STATE, "normal_acc_combine_dev: removing " + std::to_string(src->geq) +
                                     " gradient equations from an accumulator that holds " + std::to_string(dst->geq));
  OB_TRY(require_device());
  const bool empty = dst->rows == 0;  // of value rows: the shift is theirs alone
  const bool fresh = empty && dst->geq == 0;
  if (src->rows == 0)  // gradient rows only: no B^T 1, no moments, no shift
    OB_TRY(launch_acc_fold_grad(dst->p, dst->q, dst->st.p, src->st.p, (double)sign));
  else
    OB_TRY(launch_acc_fold(dst->p, dst->q, dst->st.p, src->st.p, empty, (double)sign));
  if (fresh) dst->version = src->version;
  if (sign > 0) {
    dst->rows += src->rows;
    dst->batches += src->batches;
    dst->geq += src->geq;
    dst->gbatches += src->gbatches;
  } else {
    dst->rows -= src->rows;
    dst->batches -= std::min(dst->batches, src->batches);
    dst->geq -= src->geq;
    dst->gbatches -= std::min(dst->gbatches, src->gbatches);
    OB_TRY(after_removal(dst));
  }
  return 0;
}

int obhip_normal_acc_solve_dev(const obhip_normal_acc *acc, const obhip_normal_acc *minus, double sigma, double rho,
                               double *d_H, double *d_Theta, double *d_diagH, double *d_meansd, void *d_workspace,
                               uint64_t workspace_bytes) {
  if (!acc || !d_H || !d_Theta || !d_meansd || !d_workspace)
    return fail(OBHIP_ERR_INVALID, "normal_acc_solve_dev: null argument");
  if (minus && (minus->model != acc->model || !same_terms(minus->terms, acc->terms) || minus->p != acc->p || minus->q != acc->q))
    return fail(OBHIP_ERR_INVALID, "normal_acc_solve_dev: the accumulators differ in model, terms or responses");
  const obhip_model *m = acc->model;
  OB_TRY(check_compat(m, acc->terms));
  OB_TRY(check_version(acc, "normal_acc_solve_dev"));
  if (minus) OB_TRY(check_version(minus, "normal_acc_solve_dev"));
  if (minus && (minus->rows > acc->rows || minus->geq > acc->geq))
    return fail(OBHIP_ERR_STATE, "normal_acc_solve_dev: more rows to take out than the accumulator holds");
  const uint64_t left = acc->rows - (minus ? minus->rows : 0);
  if (left < 2)
    return fail(OBHIP_ERR_STATE, "normal_acc_solve_dev: " + std::to_string(left) +
                                     " rows left, the standard deviation of a response needs two");
  const uint64_t p = acc->p, q = acc->q;
  uint64_t need = 0, single = 0;
  OB_TRY(obhip_newton_multi_workspace_bytes(p, q, &need));
  OB_TRY(obhip_newton_workspace_bytes(p, &single));
  if (workspace_bytes < need) return fail(OBHIP_ERR_INVALID, "normal_acc_solve_dev: workspace too small");
  OB_TRY(require_device());
  obhip_terms &t = *const_cast<obhip_terms *>(acc->terms);
  const double *d_prec = nullptr;
  OB_TRY(terms_prec_dev(m, t, rho, &d_prec));
  const double e2 = std::exp(-2.0 * sigma);
  const double *d_minus = minus && (minus->rows > 0 || minus->geq > 0) ? minus->st.p : nullptr;
  DevBuf<double> rhs;
  OB_TRY(rhs.alloc(p * q));
  {
    ProfScope ps("acc_form");
    OB_TRY(launch_unpack_tri(p, acc->st.p, d_minus, d_H, true, e2, d_prec, d_diagH));
  }
  OB_TRY(launch_acc_rhs(p, q, acc->st.p, d_minus, e2, rhs.p, d_meansd));
  void *d_cholws = (double *)d_workspace + 2 * p;
  OB_TRY(launch_newton_solve(p, d_H, rhs.p, d_Theta, d_cholws, newton_workspace_bytes(p)));
  // the right-hand sides carry e^{-2 sigma} already
  return solve_columns(p, d_H, d_cholws, rhs.p + p, q - 1, 1.0, d_Theta + p, (char *)d_workspace + single);
}

// G = e^{-2 sigma} B^T y_std and the moments of the rows in acc (without those of minus): the right-hand sides
// obhip_normal_acc_solve_dev solves for, by the same kernel (the term-count path substitutes them itself)
int obhip_normal_acc_rhs_dev(const obhip_normal_acc *acc, const obhip_normal_acc *minus, double sigma, double *d_G,
                             double *d_meansd) {
  if (!acc || !d_G || !d_meansd || !std::isfinite(sigma)) return fail(OBHIP_ERR_INVALID, "normal_acc_rhs_dev: bad argument");
  if (minus && (minus->model != acc->model || !same_terms(minus->terms, acc->terms) || minus->p != acc->p || minus->q != acc->q))
    return fail(OBHIP_ERR_INVALID, "normal_acc_rhs_dev: the accumulators differ in model, terms or responses");
  OB_TRY(check_compat(acc->model, acc->terms));
  OB_TRY(check_version(acc, "normal_acc_rhs_dev"));
  if (minus) OB_TRY(check_version(minus, "normal_acc_rhs_dev"));
  if (minus && (minus->rows > acc->rows || minus->geq > acc->geq))
    return fail(OBHIP_ERR_STATE, "normal_acc_rhs_dev: more rows to take out than the accumulator holds");
  const uint64_t left = acc->rows - (minus ? minus->rows : 0);
  if (left < 2)
    return fail(OBHIP_ERR_STATE, "normal_acc_rhs_dev: " + std::to_string(left) +
                                     " rows left, the standard deviation of a response needs two");
  OB_TRY(require_device());
  const double *d_minus = minus && (minus->rows > 0 || minus->geq > 0) ? minus->st.p : nullptr;
  return launch_acc_rhs(acc->p, acc->q, acc->st.p, d_minus, std::exp(-2.0 * sigma), d_G, d_meansd);
}

// the posterior of the rows in acc (without those of minus): H as obhip_normal_acc_solve_dev forms it
int obhip_normal_acc_posterior_dev(const obhip_normal_acc *acc, const obhip_normal_acc *minus, double sigma, double rho,
                                   obhip_posterior **out) {
  if (!acc || !out || !std::isfinite(sigma) || !std::isfinite(rho))
    return fail(OBHIP_ERR_INVALID, "normal_acc_posterior_dev: bad argument");
  if (minus && (minus->model != acc->model || !same_terms(minus->terms, acc->terms) || minus->p != acc->p || minus->q != acc->q))
    return fail(OBHIP_ERR_INVALID, "normal_acc_posterior_dev: the accumulators differ in model, terms or responses");
  const obhip_model *m = acc->model;
  OB_TRY(check_compat(m, acc->terms));
  OB_TRY(check_version(acc, "normal_acc_posterior_dev"));
  if (minus) OB_TRY(check_version(minus, "normal_acc_posterior_dev"));
  if (minus && (minus->rows > acc->rows || minus->geq > acc->geq))
    return fail(OBHIP_ERR_STATE, "normal_acc_posterior_dev: more rows to take out than the accumulator holds");
  OB_TRY(require_device());
  obhip_terms &t = *const_cast<obhip_terms *>(acc->terms);
  const uint64_t p = acc->p;
  const double *d_prec = nullptr;
  OB_TRY(terms_prec_dev(m, t, rho, &d_prec));
  const double *d_minus = minus && (minus->rows > 0 || minus->geq > 0) ? minus->st.p : nullptr;
  DevBuf<double> H;
  OB_TRY(H.alloc(p * p));
  OB_TRY(launch_unpack_tri(p, acc->st.p, d_minus, H.p, true, std::exp(-2.0 * sigma), d_prec, nullptr));
  return posterior_from_hessian(out, m, acc->terms, H.p, sigma);
}

int obhip_cv_score_dev(const double *d_mean, const double *d_Y_raw, uint64_t n, uint64_t q, uint64_t ld,
                       const double *d_meansd, double *d_out) {
  if (!d_out || q == 0 || q > kMaxResponses || (n != 0 && (!d_mean || !d_Y_raw || ld < n)))
    return fail(OBHIP_ERR_INVALID, "cv_score_dev: bad argument");
  OB_TRY(require_device());
  DevBuf<double> part;
  OB_TRY(part.alloc(kSumBlocks * q));
  return launch_cv_score(d_mean, d_Y_raw, n, q, ld, d_meansd, d_out, part.p);
}

}  // extern "C"
