// Host side of the predictor on the product of two input blocks (include/obhip.h, "product of two input
// blocks"; kernels in kernels_product.hip): the split of the dimensions, the sides'
// column tables, the choice between the fused kernel and the row route, and the C entry points.  Behind them the
// same for the gradient by xb (kernels_product_dx.hip): the views of the B dimensions, the
// row route through obhip_predict_grad_dev, and its entry points.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "obhip_internal.h"

using namespace obhip;

namespace obhip {

int make_split(const char *who, const obhip_terms &t, const uint32_t *dims_b, uint64_t ndims_b, ProductSplit &s) {
  const uint64_t d = t.d, p = t.p;
  if (!dims_b || ndims_b < 1 || ndims_b + 1 > d)
    return fail(OBHIP_ERR_INVALID, std::string(who) + ": dims_b must name 1 to d - 1 dimensions");
  for (uint64_t k = 0; k < ndims_b; ++k) {
    if (dims_b[k] >= d) return fail(OBHIP_ERR_INVALID, std::string(who) + ": dims_b entry out of range");
    if (k > 0 && dims_b[k] <= dims_b[k - 1])
      return fail(OBHIP_ERR_INVALID, std::string(who) + ": dims_b must be strictly ascending");
  }
  s.dims_b.assign(dims_b, dims_b + ndims_b);
  s.dim_src.assign(d, 0);
  std::vector<char> in_b(d, 0);
  for (uint64_t k = 0; k < ndims_b; ++k) in_b[dims_b[k]] = 1;
  for (uint64_t l = 0; l < d; ++l) {
    if (in_b[l]) {
      s.dim_src[l] = -(int)s.side_b.size() - 1;
      s.side_b.push_back((int)l);
    } else {
      s.dim_src[l] = (int)s.side_a.size();
      s.side_a.push_back((int)l);
    }
  }
  s.seen.resize(d);
  for (uint64_t l = 0; l < d; ++l) {
    s.seen[l].assign(t.maxlev[l] + 1, 0);
    for (uint64_t k = 0; k < p; ++k) s.seen[l][t.lev[k * d + l]] = 1;
    uint64_t used = 0;
    for (int64_t v = 1; v <= t.maxlev[l]; ++v) used += s.seen[l][v];
    (in_b[l] ? s.mu_b : s.mu_a) += used;
  }
  uint64_t nza = 0, nzb = 0;
  for (uint64_t k = 0; k < p; ++k) {
    uint64_t a = 0, b = 0;
    for (uint64_t l = 0; l < d; ++l)
      if (t.lev[k * d + l] > 0) (in_b[l] ? b : a) += 1;
    nza = std::max(nza, a), nzb = std::max(nzb, b);
  }
  s.wa = std::max<uint64_t>(2, (nza + 1) / 2 * 2);
  s.wb = std::max<uint64_t>(2, (nzb + 1) / 2 * 2);
  s.fused = s.mu_a <= 65535 && s.mu_b <= 65535 && predict_product_supports(s.mu_a, s.mu_b, s.wa, s.wb);
  return 0;
}

}  // namespace obhip

namespace obhip {

// one side's tables against the column layout of t.pred_md: its used columns are numbered 1, 2, .. in the
// order of the side's dimensions and, within a dimension, of the levels
void side_tables(const obhip_terms &t, const ProductSplit &s, const std::vector<int> &side, uint64_t w,
                 std::vector<int32_t> &cpos, std::vector<uint16_t> &cols) {
  const std::vector<DimDesc> &dims = t.pred_md.dims_h;
  const uint64_t d = t.d, p = t.p;
  uint64_t Mc = 1;
  for (uint64_t l = 0; l < d; ++l) Mc += (uint64_t)t.pred_md.cap[l];
  cpos.assign(Mc, -1);
  cpos[0] = 0;
  int32_t next = 1;
  std::vector<char> mine(d, 0);
  for (int l : side) {
    mine[l] = 1;
    for (int64_t v = 1; v <= t.maxlev[l]; ++v)
      if (s.seen[l][v]) cpos[dims[l].ccol0 + v - 1] = next++;
  }
  cols.assign(p * w, 0);
  for (uint64_t k = 0; k < p; ++k) {
    uint64_t nnz = 0;
    for (uint64_t l = 0; l < d; ++l) nnz += mine[l] && t.lev[k * d + l] > 0;
    uint64_t at = w - nnz;  // right-aligned: the ones in front, the factors in the order of the dimensions
    for (uint64_t l = 0; l < d; ++l) {
      const uint32_t v = t.lev[k * d + l];
      if (mine[l] && v > 0) cols[k * w + at++] = (uint16_t)cpos[dims[l].ccol0 + v - 1];
    }
  }
}

// the device tables of the split, cached on the terms for the last split and column layout asked for
int ensure_product_tables(const obhip_model &m, obhip_terms &t, const ProductSplit &s) {
  OB_TRY(prepare_predict(m, t, false));
  obhip_terms::Product &pr = t.product;
  if (pr.cols_a.p && pr.dims_b == s.dims_b && pr.cap == t.pred_md.cap) return 0;
  std::vector<int32_t> cpa, cpb;
  std::vector<uint16_t> ca, cb;
  side_tables(t, s, s.side_a, s.wa, cpa, ca);
  side_tables(t, s, s.side_b, s.wb, cpb, cb);
  pr.cols_a.release();  // not valid until every table is in place
  OB_TRY(pr.side_a.upload(s.side_a.data(), s.side_a.size()));
  OB_TRY(pr.side_b.upload(s.side_b.data(), s.side_b.size()));
  OB_TRY(pr.dim_src.upload(s.dim_src.data(), s.dim_src.size()));
  OB_TRY(pr.cpos_a.upload(cpa.data(), cpa.size()));
  OB_TRY(pr.cpos_b.upload(cpb.data(), cpb.size()));
  OB_TRY(pr.cols_b.upload(cb.data(), cb.size()));
  pr.dims_b = s.dims_b, pr.cap = t.pred_md.cap;
  pr.mu_a = s.mu_a, pr.mu_b = s.mu_b, pr.wa = s.wa, pr.wb = s.wb;
  OB_TRY(pr.cols_a.upload(ca.data(), ca.size()));
  return 0;
}

}  // namespace obhip

namespace {

bool take_fused(const ProductSplit &s) { return s.fused && !getenv("OBHIP_FORCE_GENERIC"); }

// The row route: the pairs in chunks (a range of A rows that is all of them or whole tiles, a range of B
// rows) of at most kRowChunk doubles of scratch, written out as full-width rows for the row predictors.
constexpr uint64_t kRowChunk = 1ull << 23;

struct Chunks {
  uint64_t ni = 0, nj = 0;
};
Chunks row_chunks(uint64_t na, uint64_t nb, uint64_t d, uint64_t q) {
  const uint64_t rows = std::max<uint64_t>(kProductTile, kRowChunk / (d + q + 1));
  Chunks c;
  c.ni = na <= rows ? na : rows / kProductTile * kProductTile;
  c.nj = std::min(nb, std::max<uint64_t>(1, rows / c.ni));
  return c;
}

int rows_predict(const obhip_model &m, obhip_terms &t, const ProductCall &c) {
  const bool lik = c.mean == nullptr;
  const bool var = c.coeffvar != nullptr && (lik || c.var != nullptr);
  const Chunks ch = row_chunks(c.na, c.nb, t.d, c.q);
  const uint64_t rows_max = ch.ni * ch.nj;
  DevBuf<double> X, M, V;
  OB_TRY(X.alloc(rows_max * t.d));
  OB_TRY(M.alloc(rows_max * c.q));
  if (var) OB_TRY(V.alloc(rows_max));
  for (uint64_t i0 = 0; i0 < c.na; i0 += ch.ni) {
    const uint64_t ni = std::min(ch.ni, c.na - i0);
    for (uint64_t j0 = 0; j0 < c.nb; j0 += ch.nj) {
      const uint64_t nj = std::min(ch.nj, c.nb - j0), rows = ni * nj;
      OB_TRY(launch_product_expand(t, c.xa, c.na, c.xb, c.nb, i0, ni, j0, nj, X.p));
      OB_TRY(obhip_predict_multi_dev(&m, &t, c.theta, c.q, X.p, rows, M.p, var ? c.coeffvar : nullptr, c.sigma,
                                     var ? V.p : nullptr));
      if (lik) {
        OB_TRY(launch_product_lik_rows(M.p, var ? V.p : nullptr, std::exp(2.0 * c.sigma), c.y, c.obsvar, c.na, c.nb,
                                       i0, ni, j0, nj, c.part));
      } else {
        OB_TRY(launch_product_scatter(M.p, c.q, c.nb, c.lda, i0, ni, j0, nj, c.mean));
        if (var) OB_TRY(launch_product_scatter(V.p, 1, c.nb, c.lda, i0, ni, j0, nj, c.var));
      }
    }
  }
  return 0;
}

int run_product(const obhip_model &m, obhip_terms &t, const ProductSplit &s, const ProductCall &c) {
  OB_TRY(ensure_product_tables(m, t, s));
  return take_fused(s) ? launch_predict_product(m, t, c) : rows_predict(m, t, c);
}

bool bad_obsvar(const double *v, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i)
    if (!(v[i] >= 0.0) || !std::isfinite(v[i])) return true;
  return false;
}

// ---- gradient by xb ----------------------------------------------------------
// sum_l |view_l|: the (term, B dimension) pairs with a factor, from the levels alone
uint64_t view_terms_of(const obhip_terms &t, const ProductSplit &s) {
  uint64_t n = 0;
  for (uint32_t l : s.dims_b)
    for (uint64_t k = 0; k < t.p; ++k) n += t.lev[k * t.d + l] > 0;
  return n;
}

bool grad_fused(const ProductSplit &s) {
  return s.mu_a <= 65535 && s.mu_b <= 65535 && product_grad_supports(s.mu_a, s.mu_b, s.dims_b.size(), s.wa, s.wb);
}
bool take_grad_fused(const ProductSplit &s) { return grad_fused(s) && !getenv("OBHIP_FORCE_GENERIC"); }

// the tables of the split, the derivative interval tables and, for the fused kernel, the views of the B
// dimensions, cached on the terms beside t.product for the last split and column layout asked for
int ensure_product_grad_tables(const obhip_model &m, obhip_terms &t, const ProductSplit &s, bool fused) {
  OB_TRY(ensure_product_tables(m, t, s));
  OB_TRY(ensure_dx_tables(m, t));
  if (!fused) return 0;
  obhip_terms::ProductGrad &pg = t.product_grad;
  if (pg.vw.p && pg.dims_b == s.dims_b && pg.cap == t.pred_md.cap) return 0;
  std::vector<int32_t> cpa, cpb;
  std::vector<uint16_t> ca, cb;
  side_tables(t, s, s.side_a, s.wa, cpa, ca);
  side_tables(t, s, s.side_b, s.wb, cpb, cb);
  const std::vector<DimDesc> &dims = t.pred_md.dims_h;
  const uint64_t wa2 = s.wa / 2, wb2 = s.wb / 2, stride = wa2 + wb2 + 2, nent = view_terms_of(t, s);
  if (nent >= (1ull << 31)) return fail(OBHIP_ERR_INVALID, "product_grad: more than 2^31 term factors on side B");
  std::vector<uint32_t> hw(std::max<uint64_t>(nent, 1) * stride, 0), off(s.dims_b.size() + 1, 0);
  std::vector<uint16_t> other(s.wb);
  auto words = [](const uint16_t *c, uint64_t w2, uint32_t *out) {
    for (uint64_t q = 0; q < w2; ++q) out[q] = (uint32_t)c[2 * q] | ((uint32_t)c[2 * q + 1] << 16);
  };
  uint64_t e = 0;
  for (uint64_t lb = 0; lb < s.dims_b.size(); ++lb) {
    const uint64_t l = s.dims_b[lb];
    for (uint64_t k = 0; k < t.p; ++k) {
      const uint32_t v = t.lev[k * t.d + l];
      if (v == 0) continue;
      const int32_t own = cpb[dims[l].ccol0 + v - 1];
      if (own < 1) return fail(OBHIP_ERR_STATE, "product_grad: a term's column is not in the used list");
      // the term's B columns with its own slot turned into the ones column: a used column belongs to one
      // (dimension, level), so the value finds the slot
      std::copy(cb.begin() + k * s.wb, cb.begin() + (k + 1) * s.wb, other.begin());
      *std::find(other.begin(), other.end(), (uint16_t)own) = 0;
      uint32_t *ent = &hw[e++ * stride];
      words(&ca[k * s.wa], wa2, ent);
      words(other.data(), wb2, ent + wa2);
      ent[wa2 + wb2] = (uint32_t)own;
      ent[wa2 + wb2 + 1] = (uint32_t)k;
    }
    off[lb + 1] = (uint32_t)e;
  }
  pg.vw.release();  // not valid until every table is in place
  OB_TRY(pg.voff.upload(off.data(), off.size()));
  pg.voff_h = off, pg.dims_b = s.dims_b, pg.cap = t.pred_md.cap;
  OB_TRY(pg.vw.upload(hw.data(), hw.size()));
  return 0;
}

// the row route of the gradient: the chunks of rows_predict through obhip_predict_grad_dev on the full-width
// rows, the B dimensions' columns of its gradients scattered or reduced in the fused kernel's order
int rows_grad(const obhip_model &m, obhip_terms &t, const ProductGradCall &c) {
  const bool lik = c.dmean == nullptr;
  const bool var = c.coeffvar != nullptr && (lik || c.dvar != nullptr);
  const std::vector<uint32_t> &dims_b = t.product.dims_b;
  // doubles per row: the row, mean and variance, the two gradients
  const Chunks ch = row_chunks(c.na, c.nb, t.d, 2 * t.d + 1);
  const uint64_t rows_max = ch.ni * ch.nj;
  DevBuf<double> X, M, V, G, GV;
  OB_TRY(X.alloc(rows_max * t.d));
  OB_TRY(M.alloc(rows_max));
  OB_TRY(G.alloc(rows_max * t.d));
  if (var) {
    OB_TRY(V.alloc(rows_max));
    OB_TRY(GV.alloc(rows_max * t.d));
  }
  for (uint64_t i0 = 0; i0 < c.na; i0 += ch.ni) {
    const uint64_t ni = std::min(ch.ni, c.na - i0);
    for (uint64_t j0 = 0; j0 < c.nb; j0 += ch.nj) {
      const uint64_t nj = std::min(ch.nj, c.nb - j0), rows = ni * nj;
      OB_TRY(launch_product_expand(t, c.xa, c.na, c.xb, c.nb, i0, ni, j0, nj, X.p));
      OB_TRY(obhip_predict_grad_dev(&m, &t, c.theta, X.p, rows, M.p, G.p, var ? c.coeffvar : nullptr, c.sigma,
                                    var ? V.p : nullptr, var ? GV.p : nullptr));
      if (lik) {
        OB_TRY(launch_product_lik_grad_rows(t, M.p, var ? V.p : nullptr, std::exp(2.0 * c.sigma), G.p,
                                            var ? GV.p : nullptr, c.y, c.obsvar, c.na, c.nb, i0, ni, j0, nj, c.part));
        // the sums themselves exactly as rows_predict forms them: the same predictor, the same reduction
        OB_TRY(obhip_predict_multi_dev(&m, &t, c.theta, 1, X.p, rows, M.p, var ? c.coeffvar : nullptr, c.sigma,
                                       var ? V.p : nullptr));
        OB_TRY(launch_product_lik_rows(M.p, var ? V.p : nullptr, std::exp(2.0 * c.sigma), c.y, c.obsvar, c.na, c.nb,
                                       i0, ni, j0, nj, c.part));
        continue;
      }
      for (uint64_t lb = 0; lb < dims_b.size(); ++lb) {
        const uint64_t l = dims_b[lb];
        OB_TRY(launch_product_scatter(G.p + l * rows, 1, c.nb, c.lda, i0, ni, j0, nj, c.dmean + lb * c.nb * c.lda));
        if (var)
          OB_TRY(launch_product_scatter(GV.p + l * rows, 1, c.nb, c.lda, i0, ni, j0, nj, c.dvar + lb * c.nb * c.lda));
      }
    }
  }
  return 0;
}

int run_product_grad(const obhip_model &m, obhip_terms &t, const ProductSplit &s, const ProductGradCall &c) {
  const bool fused = take_grad_fused(s);
  OB_TRY(ensure_product_grad_tables(m, t, s, fused));
  return fused ? launch_product_grad(m, t, c) : rows_grad(m, t, c);
}

}  // namespace

extern "C" {

int obhip_product_layout(const obhip_terms *t, const uint32_t *dims_b, uint64_t ndims_b, uint64_t *mu_a,
                         uint64_t *mu_b, int *fused) {
  if (!t) return fail(OBHIP_ERR_INVALID, "product_layout: null terms");
  ProductSplit s;
  OB_TRY(make_split("product_layout", *t, dims_b, ndims_b, s));
  if (mu_a) *mu_a = s.mu_a;
  if (mu_b) *mu_b = s.mu_b;
  if (fused) *fused = s.fused ? 1 : 0;
  return 0;
}

int obhip_predict_product_dev(const obhip_model *m, const obhip_terms *tc, const double *d_Theta, uint64_t q,
                              const uint32_t *dims_b, uint64_t ndims_b, const double *d_xa, uint64_t na,
                              const double *d_xb, uint64_t nb, double *d_mean, uint64_t lda,
                              const double *d_coeffvar, double sigma, double *d_var) {
  if (!m || !tc || !d_Theta || q == 0) return fail(OBHIP_ERR_INVALID, "predict_product_dev: null model, terms or Theta, or q = 0");
  OB_TRY(check_compat(m, tc));
  ProductSplit s;
  OB_TRY(make_split("predict_product_dev", *tc, dims_b, ndims_b, s));
  if (lda < na) return fail(OBHIP_ERR_INVALID, "predict_product_dev: lda below na");
  if (d_var && !d_coeffvar) return fail(OBHIP_ERR_INVALID, "predict_product_dev: d_var needs d_coeffvar");
  if (na == 0 || nb == 0) return 0;
  if (!d_xa || !d_xb || !d_mean) return fail(OBHIP_ERR_INVALID, "predict_product_dev: null xa, xb or mean");
  OB_TRY(require_device());
  ProductCall c;
  c.theta = d_Theta, c.q = q, c.xa = d_xa, c.na = na, c.xb = d_xb, c.nb = nb;
  c.coeffvar = d_var ? d_coeffvar : nullptr, c.sigma = sigma, c.mean = d_mean, c.lda = lda, c.var = d_var;
  return run_product(*m, *const_cast<obhip_terms *>(tc), s, c);
}

int obhip_product_loglik_dev(const obhip_model *m, const obhip_terms *tc, const double *d_theta,
                             const uint32_t *dims_b, uint64_t ndims_b, const double *d_xa, uint64_t na,
                             const double *d_y, const double *d_obsvar, const double *d_xb, uint64_t nb,
                             const double *d_coeffvar, double sigma, double *d_out) {
  if (!m || !tc || !d_theta) return fail(OBHIP_ERR_INVALID, "product_loglik_dev: null model, terms or theta");
  OB_TRY(check_compat(m, tc));
  ProductSplit s;
  OB_TRY(make_split("product_loglik_dev", *tc, dims_b, ndims_b, s));
  if (na == 0 || nb == 0) return 0;
  if (!d_xa || !d_xb || !d_y || !d_out) return fail(OBHIP_ERR_INVALID, "product_loglik_dev: null xa, xb, y or out");
  OB_TRY(require_device());
  if (d_obsvar) {
    int bad = 0;
    OB_TRY(launch_check_nonneg(d_obsvar, na, &bad));
    if (bad) return fail(OBHIP_ERR_NUMERIC, "product_loglik_dev: an observation variance is negative or not finite");
  }
  const uint64_t tiles_a = (na + kProductTile - 1) / kProductTile;
  DevBuf<double> part;
  OB_TRY(part.alloc(2 * tiles_a * nb));
  ProductCall c;
  c.theta = d_theta, c.q = 1, c.xa = d_xa, c.na = na, c.xb = d_xb, c.nb = nb;
  c.coeffvar = d_coeffvar, c.sigma = sigma, c.y = d_y, c.obsvar = d_obsvar, c.part = part.p;
  OB_TRY(run_product(*m, *const_cast<obhip_terms *>(tc), s, c));
  return launch_product_sum_tiles(part.p, tiles_a, nb, d_out);
}

int obhip_predict_product(const obhip_model *m, const obhip_terms *t, const double *Theta, uint64_t q,
                          const uint32_t *dims_b, uint64_t ndims_b, const double *xa, uint64_t na, uint64_t ldxa,
                          const double *xb, uint64_t nb, uint64_t ldxb, double *mean, uint64_t lda,
                          const double *coeffvar, double sigma, double *var) {
  if (!m || !t || !Theta || q == 0) return fail(OBHIP_ERR_INVALID, "predict_product: null model, terms or Theta, or q = 0");
  OB_TRY(check_compat(m, t));
  ProductSplit s;
  OB_TRY(make_split("predict_product", *t, dims_b, ndims_b, s));
  if (lda < na || ldxa < na || ldxb < nb) return fail(OBHIP_ERR_INVALID, "predict_product: leading dimension below the rows");
  if (var && !coeffvar) return fail(OBHIP_ERR_INVALID, "predict_product: var needs coeffvar");
  if (na == 0 || nb == 0) return 0;
  if (!xa || !xb || !mean) return fail(OBHIP_ERR_INVALID, "predict_product: null xa, xb or mean");
  OB_TRY(require_device());
  DevBuf<double> dxa, dxb, dth, dmean, dcv, dvar;
  OB_TRY(upload_cols(dxa, xa, na, s.side_a.size(), ldxa));
  OB_TRY(upload_cols(dxb, xb, nb, s.side_b.size(), ldxb));
  OB_TRY(dth.upload(Theta, t->p * q));
  OB_TRY(dmean.alloc(q * nb * na));
  if (var) {
    OB_TRY(dcv.upload(coeffvar, t->p));
    OB_TRY(dvar.alloc(nb * na));
  }
  OB_TRY(obhip_predict_product_dev(m, t, dth.p, q, dims_b, ndims_b, dxa.p, na, dxb.p, nb, dmean.p, na,
                                   var ? dcv.p : nullptr, sigma, var ? dvar.p : nullptr));
  std::vector<double> h(q * nb * na);
  OB_TRY(d2h(h.data(), dmean.p, h.size() * sizeof(double)));
  for (uint64_t c = 0; c < q * nb; ++c) std::memcpy(mean + c * lda, h.data() + c * na, na * sizeof(double));
  if (var) {
    OB_TRY(d2h(h.data(), dvar.p, nb * na * sizeof(double)));
    for (uint64_t c = 0; c < nb; ++c) std::memcpy(var + c * lda, h.data() + c * na, na * sizeof(double));
  }
  return 0;
}

int obhip_product_loglik(const obhip_model *m, const obhip_terms *t, const double *theta, const uint32_t *dims_b,
                         uint64_t ndims_b, const double *xa, uint64_t na, uint64_t ldxa, const double *y,
                         const double *obsvar, const double *xb, uint64_t nb, uint64_t ldxb, const double *coeffvar,
                         double sigma, double *out) {
  if (!m || !t || !theta) return fail(OBHIP_ERR_INVALID, "product_loglik: null model, terms or theta");
  OB_TRY(check_compat(m, t));
  ProductSplit s;
  OB_TRY(make_split("product_loglik", *t, dims_b, ndims_b, s));
  if (ldxa < na || ldxb < nb) return fail(OBHIP_ERR_INVALID, "product_loglik: leading dimension below the rows");
  if (na == 0 || nb == 0) return 0;
  if (!xa || !xb || !y || !out) return fail(OBHIP_ERR_INVALID, "product_loglik: null xa, xb, y or out");
  if (obsvar && bad_obsvar(obsvar, na))
    return fail(OBHIP_ERR_INVALID, "product_loglik: an observation variance is negative or not finite");
  OB_TRY(require_device());
  DevBuf<double> dxa, dxb, dth, dy, dov, dcv, dout;
  OB_TRY(upload_cols(dxa, xa, na, s.side_a.size(), ldxa));
  OB_TRY(upload_cols(dxb, xb, nb, s.side_b.size(), ldxb));
  OB_TRY(dth.upload(theta, t->p));
  OB_TRY(dy.upload(y, na));
  if (obsvar) OB_TRY(dov.upload(obsvar, na));
  if (coeffvar) OB_TRY(dcv.upload(coeffvar, t->p));
  OB_TRY(dout.alloc(2 * nb));
  OB_TRY(obhip_product_loglik_dev(m, t, dth.p, dims_b, ndims_b, dxa.p, na, dy.p, obsvar ? dov.p : nullptr, dxb.p, nb,
                                  coeffvar ? dcv.p : nullptr, sigma, dout.p));
  return d2h(out, dout.p, 2 * nb * sizeof(double));
}

int obhip_product_grad_layout(const obhip_terms *t, const uint32_t *dims_b, uint64_t ndims_b, uint64_t *mu_a,
                              uint64_t *mu_b, uint64_t *view_terms, int *fused) {
  if (!t) return fail(OBHIP_ERR_INVALID, "product_grad_layout: null terms");
  ProductSplit s;
  OB_TRY(make_split("product_grad_layout", *t, dims_b, ndims_b, s));
  if (mu_a) *mu_a = s.mu_a;
  if (mu_b) *mu_b = s.mu_b;
  if (view_terms) *view_terms = view_terms_of(*t, s);
  if (fused) *fused = grad_fused(s) ? 1 : 0;
  return 0;
}

int obhip_predict_product_grad_dev(const obhip_model *m, const obhip_terms *tc, const double *d_theta,
                                   const uint32_t *dims_b, uint64_t ndims_b, const double *d_xa, uint64_t na,
                                   const double *d_xb, uint64_t nb, double *d_dmean, uint64_t lda,
                                   const double *d_coeffvar, double sigma, double *d_dvar) {
  if (!m || !tc || !d_theta) return fail(OBHIP_ERR_INVALID, "predict_product_grad_dev: null model, terms or theta");
  OB_TRY(check_compat(m, tc));
  ProductSplit s;
  OB_TRY(make_split("predict_product_grad_dev", *tc, dims_b, ndims_b, s));
  if (lda < na) return fail(OBHIP_ERR_INVALID, "predict_product_grad_dev: lda below na");
  if (d_dvar && !d_coeffvar) return fail(OBHIP_ERR_INVALID, "predict_product_grad_dev: d_dvar needs d_coeffvar");
  if (na == 0 || nb == 0) return 0;
  if (!d_xa || !d_xb || !d_dmean) return fail(OBHIP_ERR_INVALID, "predict_product_grad_dev: null xa, xb or dmean");
  OB_TRY(require_device());
  ProductGradCall c;
  c.theta = d_theta, c.xa = d_xa, c.na = na, c.xb = d_xb, c.nb = nb;
  c.coeffvar = d_dvar ? d_coeffvar : nullptr, c.sigma = sigma, c.dmean = d_dmean, c.lda = lda, c.dvar = d_dvar;
  return run_product_grad(*m, *const_cast<obhip_terms *>(tc), s, c);
}

int obhip_product_loglik_grad_dev(const obhip_model *m, const obhip_terms *tc, const double *d_theta,
                                  const uint32_t *dims_b, uint64_t ndims_b, const double *d_xa, uint64_t na,
                                  const double *d_y, const double *d_obsvar, const double *d_xb, uint64_t nb,
                                  const double *d_coeffvar, double sigma, double *d_out) {
  if (!m || !tc || !d_theta) return fail(OBHIP_ERR_INVALID, "product_loglik_grad_dev: null model, terms or theta");
  OB_TRY(check_compat(m, tc));
  ProductSplit s;
  OB_TRY(make_split("product_loglik_grad_dev", *tc, dims_b, ndims_b, s));
  if (na == 0 || nb == 0) return 0;
  if (!d_xa || !d_xb || !d_y || !d_out)
    return fail(OBHIP_ERR_INVALID, "product_loglik_grad_dev: null xa, xb, y or out");
  OB_TRY(require_device());
  if (d_obsvar) {
    int bad = 0;
    OB_TRY(launch_check_nonneg(d_obsvar, na, &bad));
    if (bad)
      return fail(OBHIP_ERR_NUMERIC, "product_loglik_grad_dev: an observation variance is negative or not finite");
  }
  const uint64_t tiles_a = (na + kProductTile - 1) / kProductTile, ncols = 2 + 2 * ndims_b;
  DevBuf<double> part;
  OB_TRY(part.alloc(ncols * tiles_a * nb));
  ProductGradCall c;
  c.theta = d_theta, c.xa = d_xa, c.na = na, c.xb = d_xb, c.nb = nb;
  c.coeffvar = d_coeffvar, c.sigma = sigma, c.y = d_y, c.obsvar = d_obsvar, c.part = part.p;
  OB_TRY(run_product_grad(*m, *const_cast<obhip_terms *>(tc), s, c));
  return launch_product_sum_tile_cols(part.p, tiles_a, nb, ncols, d_out);
}

int obhip_predict_product_grad(const obhip_model *m, const obhip_terms *t, const double *theta,
                               const uint32_t *dims_b, uint64_t ndims_b, const double *xa, uint64_t na,
                               uint64_t ldxa, const double *xb, uint64_t nb, uint64_t ldxb, double *dmean,
                               uint64_t lda, const double *coeffvar, double sigma, double *dvar) {
  if (!m || !t || !theta) return fail(OBHIP_ERR_INVALID, "predict_product_grad: null model, terms or theta");
  OB_TRY(check_compat(m, t));
  ProductSplit s;
  OB_TRY(make_split("predict_product_grad", *t, dims_b, ndims_b, s));
  if (lda < na || ldxa < na || ldxb < nb)
    return fail(OBHIP_ERR_INVALID, "predict_product_grad: leading dimension below the rows");
  if (dvar && !coeffvar) return fail(OBHIP_ERR_INVALID, "predict_product_grad: dvar needs coeffvar");
  if (na == 0 || nb == 0) return 0;
  if (!xa || !xb || !dmean) return fail(OBHIP_ERR_INVALID, "predict_product_grad: null xa, xb or dmean");
  OB_TRY(require_device());
  const uint64_t cols = ndims_b * nb;
  DevBuf<double> dxa, dxb, dth, ddm, dcv, ddv;
  OB_TRY(upload_cols(dxa, xa, na, s.side_a.size(), ldxa));
  OB_TRY(upload_cols(dxb, xb, nb, s.side_b.size(), ldxb));
  OB_TRY(dth.upload(theta, t->p));
  OB_TRY(ddm.alloc(cols * na));
  if (dvar) {
    OB_TRY(dcv.upload(coeffvar, t->p));
    OB_TRY(ddv.alloc(cols * na));
  }
  OB_TRY(obhip_predict_product_grad_dev(m, t, dth.p, dims_b, ndims_b, dxa.p, na, dxb.p, nb, ddm.p, na,
                                        dvar ? dcv.p : nullptr, sigma, dvar ? ddv.p : nullptr));
  std::vector<double> h(cols * na);
  OB_TRY(d2h(h.data(), ddm.p, h.size() * sizeof(double)));
  for (uint64_t c = 0; c < cols; ++c) std::memcpy(dmean + c * lda, h.data() + c * na, na * sizeof(double));
  if (dvar) {
    OB_TRY(d2h(h.data(), ddv.p, h.size() * sizeof(double)));
    for (uint64_t c = 0; c < cols; ++c) std::memcpy(dvar + c * lda, h.data() + c * na, na * sizeof(double));
  }
  return 0;
}

int obhip_product_loglik_grad(const obhip_model *m, const obhip_terms *t, const double *theta,
                              const uint32_t *dims_b, uint64_t ndims_b, const double *xa, uint64_t na,
                              uint64_t ldxa, const double *y, const double *obsvar, const double *xb, uint64_t nb,
                              uint64_t ldxb, const double *coeffvar, double sigma, double *out) {
  if (!m || !t || !theta) return fail(OBHIP_ERR_INVALID, "product_loglik_grad: null model, terms or theta");
  OB_TRY(check_compat(m, t));
  ProductSplit s;
  OB_TRY(make_split("product_loglik_grad", *t, dims_b, ndims_b, s));
  if (ldxa < na || ldxb < nb) return fail(OBHIP_ERR_INVALID, "product_loglik_grad: leading dimension below the rows");
  if (na == 0 || nb == 0) return 0;
  if (!xa || !xb || !y || !out) return fail(OBHIP_ERR_INVALID, "product_loglik_grad: null xa, xb, y or out");
  if (obsvar && bad_obsvar(obsvar, na))
    return fail(OBHIP_ERR_INVALID, "product_loglik_grad: an observation variance is negative or not finite");
  OB_TRY(require_device());
  const uint64_t ncols = 2 + 2 * ndims_b;
  DevBuf<double> dxa, dxb, dth, dy, dov, dcv, dout;
  OB_TRY(upload_cols(dxa, xa, na, s.side_a.size(), ldxa));
  OB_TRY(upload_cols(dxb, xb, nb, s.side_b.size(), ldxb));
  OB_TRY(dth.upload(theta, t->p));
  OB_TRY(dy.upload(y, na));
  if (obsvar) OB_TRY(dov.upload(obsvar, na));
  if (coeffvar) OB_TRY(dcv.upload(coeffvar, t->p));
  OB_TRY(dout.alloc(ncols * nb));
  OB_TRY(obhip_product_loglik_grad_dev(m, t, dth.p, dims_b, ndims_b, dxa.p, na, dy.p, obsvar ? dov.p : nullptr, dxb.p,
                                       nb, coeffvar ? dcv.p : nullptr, sigma, dout.p));
  return d2h(out, dout.p, ncols * nb * sizeof(double));
}

}  // extern "C"
