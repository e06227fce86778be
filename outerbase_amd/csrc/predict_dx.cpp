// Input gradients of the predictive mean and variance: host side.  No reference counterpart.
//   build_dim_views_host  per dimension the terms that have it (from the levels alone)
//   ensure_dx_tables      the views packed against the used-column layout, and the derivative
//                         interval tables of the mat25 / mat25pow dimensions that have tables
//   obhip_predict_grad_dev / obhip_predict_grad / obhip_terms_dimview
// Every check that can refuse a call runs before the first device call.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "obhip_internal.h"

using namespace obhip;

namespace obhip {

// rows one call takes: the view offsets and tile counts of the kernel are 64-bit, the bound keeps
// n * d * 8 bytes far inside the address space

void build_dim_views_host(obhip_terms &t) {
  if (t.dx.voff.size() == t.d + 1) return;
  t.dx.voff.assign(t.d + 1, 0);
  t.dx.vterm.clear();
  for (uint64_t l = 0; l < t.d; ++l) {
    for (uint64_t k = 0; k < t.p; ++k)
      if (t.lev[k * t.d + l] > 0) t.dx.vterm.push_back((uint32_t)k);
    t.dx.voff[l + 1] = t.dx.vterm.size();
  }
}

// Derivative interval tables.  ModelDev::build (core.cpp) writes, per interval J of the sorted
// u_j and level c, six sums over the knots of k(h) = (1 + h + h^2/3) e^{-h} expanded around
// ref = u_(J-1); here the same six of dk/du = -+ (1/3) (h + h^2) e^{-h}:
//   h = t + d_j (j < J):   dk/du = -e^{-t} e^{-d_j} [(d_j + d_j^2) + t (1 + 2 d_j) + t^2] / 3
//   h = d_j - t (j >= J):  dk/du = +e^{+t} e^{-d_j} [(d_j + d_j^2) - t (1 + 2 d_j) + t^2] / 3
// so the device evaluates e^{-t} (A0 + t (A1 + t A2)) + e^{+t} (B0 + t (t B2 - B1)) with these
// entries exactly as it does the value.  Summed in extended precision, every bracket term of one
// sign: what cancels is what cancels in the knot sum of the derivative (the signs of rot).
static void build_dx_tables_host(const obhip_model &m, const ModelDev &md, std::vector<double> &out) {
  out.assign(std::max<size_t>(md.tab.n, 2), 0.0);
  for (uint64_t l = 0; l < m.d; ++l) {
    const DimDesc &D = md.dims_h[l];
    if (D.tab < 0) continue;
    const uint64_t ml = (uint64_t)D.m, o = m.knotptst[l];
    // u_j and their order, as ModelDev::build forms them
    std::vector<double> u(ml);
    for (uint64_t j = 0; j < ml; ++j)
      u[j] = (D.kind == OBHIP_COV_MAT25 ? m.knotpt[o + j] / D.p0 : std::pow(m.knotpt[o + j], D.p0) / D.p1) - D.p2;
    std::vector<int> ord(ml);
    for (uint64_t j = 0; j < ml; ++j) ord[j] = (int)j;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return u[a] < u[b]; });
    std::vector<double> us(ml);
    std::vector<long double> ep(ml), em(ml);
    for (uint64_t j = 0; j < ml; ++j) {
      us[j] = u[ord[j]];
      ep[j] = expl((long double)us[j]);
      em[j] = expl(-(long double)us[j]);
    }
    const uint64_t mu = (ml + 1) / 2 * 2;
    double *cf = out.data() + D.tab + mu;
    for (uint64_t J = 0; J <= ml; ++J) {
      const uint64_t jr = J >= 1 ? J - 1 : 0;
      const double ref = us[jr];
      for (int cc = 0; cc < D.ncol; ++cc) {
        long double A0 = 0, A1 = 0, A2 = 0, B0 = 0, B1 = 0, B2 = 0;
        for (uint64_t j = 0; j < ml; ++j) {
          const long double dj = j < J ? (long double)ref - us[j] : (long double)us[j] - ref;
          const long double w = (j < J ? ep[j] * em[jr] : em[j] * ep[jr]) *
                                (long double)m.rotmat[(o + cc) * m.mmax + ord[j]] / 3;
          const long double q0 = dj + dj * dj, q1 = 1 + 2 * dj;
          if (j < J) {
            A0 -= w * q0;
            A1 -= w * q1;
            A2 -= w;
          } else {
            B0 += w * q0;
            B1 += w * q1;
            B2 += w;
          }
        }
        double *e = cf + (J * D.ncol + cc) * 6;
        e[0] = (double)A0, e[1] = (double)A1, e[2] = (double)A2;
        e[3] = (double)B0, e[4] = (double)B1, e[5] = (double)B2;
      }
    }
  }
}

int ensure_dx_tables(const obhip_model &m, obhip_terms &t) {
  obhip_terms::Dx &dx = t.dx;
  if (!dx.dtab.p || dx.tab_model != &m || dx.tab_version != m.version || dx.tab_cap != t.pred_md.cap) {
    std::vector<double> h;
    build_dx_tables_host(m, t.pred_md, h);
    OB_TRY(dx.dtab.upload(h.data(), h.size()));
    dx.tab_model = &m;
    dx.tab_version = m.version;
    dx.tab_cap = t.pred_md.cap;
  }
  if (dx.vw.p && dx.cap == t.cached_cap) return 0;
  build_dim_views_host(t);
  const uint64_t W2 = t.W / 2, stride = W2 + 2, nent = dx.vterm.size();
  std::vector<uint32_t> hw(std::max<uint64_t>(nent, 1) * stride, 0);
  std::vector<uint16_t> slots(t.W);
  const std::vector<DimDesc> &dims = t.pred_md.dims_h;
  auto used_col = [&](uint64_t l, uint32_t lev) { return t.cpos_h[(size_t)dims[l].ccol0 + lev - 1]; };
  for (uint64_t l = 0; l < t.d; ++l)
    for (uint64_t e = dx.voff[l]; e < dx.voff[l + 1]; ++e) {
      const uint64_t k = dx.vterm[e];
      // the other factors right-aligned in dimension order, like the terms' own lists
      uint64_t nz = 0;
      for (uint64_t j = 0; j < t.d; ++j) nz += j != l && t.lev[k * t.d + j] > 0;
      std::fill(slots.begin(), slots.end(), (uint16_t)0);
      uint64_t w = t.W - nz;
      for (uint64_t j = 0; j < t.d; ++j) {
        const uint32_t lv = t.lev[k * t.d + j];
        if (j == l || lv == 0) continue;
        const int32_t u = used_col(j, lv);
        if (u < 1) return fail(OBHIP_ERR_STATE, "predict_grad: a term's column is not in the used list");
        slots[w++] = (uint16_t)u;
      }
      const int32_t own = used_col(l, t.lev[k * t.d + l]);
      if (own < 1) return fail(OBHIP_ERR_STATE, "predict_grad: a term's column is not in the used list");
      uint32_t *ent = &hw[e * stride];
      for (uint64_t q = 0; q < W2; ++q) ent[q] = (uint32_t)slots[2 * q] | ((uint32_t)slots[2 * q + 1] << 16);
      ent[W2] = (uint32_t)own;
      ent[W2 + 1] = (uint32_t)k;
    }
  if (nent >= (1ull << 31)) return fail(OBHIP_ERR_INVALID, "predict_grad: more than 2^31 term factors");
  std::vector<uint32_t> ho(t.d + 1);
  for (uint64_t l = 0; l <= t.d; ++l) ho[l] = (uint32_t)dx.voff[l];
  OB_TRY(dx.vw.upload(hw.data(), hw.size()));
  OB_TRY(dx.voff_dev.upload(ho.data(), ho.size()));
  dx.cap = t.cached_cap;
  return 0;
}

}  // namespace obhip

extern "C" {

int obhip_predict_grad_dev(const obhip_model *m, const obhip_terms *t, const double *d_theta, const double *d_x,
                           uint64_t n, double *d_mean, double *d_grad, const double *d_coeffvar, double sigma,
                           double *d_var, double *d_gradvar) {
  if (!m || !t || !d_theta || !d_grad || (!d_x && n > 0))
    return fail(OBHIP_ERR_INVALID, "predict_grad_dev: null model, terms, theta, x or grad");
  if (d_gradvar && !d_coeffvar) return fail(OBHIP_ERR_INVALID, "predict_grad_dev: gradvar needs coeffvar");
  if (n > kMaxRowsPerCall) return fail(OBHIP_ERR_INVALID, "predict_grad_dev: more than 2^40 rows in one call");
  OB_TRY(check_compat(m, t));
  if (n == 0) return 0;
  OB_TRY(require_device());
  return launch_predict_dx(*m, *const_cast<obhip_terms *>(t), d_theta, d_x, n, d_mean, d_grad, d_coeffvar,
                           std::exp(2.0 * sigma), d_var, d_gradvar);
}

int obhip_predict_grad(const obhip_model *m, const obhip_terms *t, const double *theta, const double *x, uint64_t n,
                       uint64_t ldx, double *mean, double *grad, uint64_t ldg, const double *coeffvar, double sigma,
                       double *var, double *gradvar) {
  if (!m || !t || !theta || !grad || (!x && n > 0))
    return fail(OBHIP_ERR_INVALID, "predict_grad: null model, terms, theta, x or grad");
  if (gradvar && !coeffvar) return fail(OBHIP_ERR_INVALID, "predict_grad: gradvar needs coeffvar");
  if (n > kMaxRowsPerCall) return fail(OBHIP_ERR_INVALID, "predict_grad: more than 2^40 rows in one call");
  if (ldx < n || ldg < n) return fail(OBHIP_ERR_INVALID, "predict_grad: leading dimension below n");
  OB_TRY(check_compat(m, t));
  if (n == 0) return 0;
  OB_TRY(require_device());
  const uint64_t d = m->d;
  DevBuf<double> dx, dth, dmean, dgrad, dcv, dvar, dgv;
  OB_TRY(upload_cols(dx, x, n, d, ldx));
  OB_TRY(dth.upload(theta, t->p));
  if (mean) OB_TRY(dmean.alloc(n));
  OB_TRY(dgrad.alloc(n * d));
  if (coeffvar) {
    OB_TRY(dcv.upload(coeffvar, t->p));
    if (var) OB_TRY(dvar.alloc(n));
    if (gradvar) OB_TRY(dgv.alloc(n * d));
  }
  OB_TRY(obhip_predict_grad_dev(m, t, dth.p, dx.p, n, dmean.p, dgrad.p, dcv.p, sigma, dvar.p, dgv.p));
  auto rows_back = [&](double *dst, const double *src) -> int {
    if (ldg == n) return d2h(dst, src, n * d * sizeof(double));
    std::vector<double> tmp(n * d);
    OB_TRY(d2h(tmp.data(), src, n * d * sizeof(double)));
    for (uint64_t l = 0; l < d; ++l) std::memcpy(dst + l * ldg, &tmp[l * n], n * sizeof(double));
    return 0;
  };
  if (mean) OB_TRY(d2h(mean, dmean.p, n * sizeof(double)));
  OB_TRY(rows_back(grad, dgrad.p));
  if (coeffvar && var) OB_TRY(d2h(var, dvar.p, n * sizeof(double)));
  if (coeffvar && gradvar) OB_TRY(rows_back(gradvar, dgv.p));
  return 0;
}

int obhip_terms_dimview(const obhip_terms *t, uint64_t dim, uint64_t *count, uint32_t *terms_out) {
  if (!t || !count || dim >= t->d) return fail(OBHIP_ERR_INVALID, "terms_dimview: bad argument");
  obhip_terms &tt = *const_cast<obhip_terms *>(t);
  build_dim_views_host(tt);
  const uint64_t b = tt.dx.voff[dim], e = tt.dx.voff[dim + 1];
  *count = e - b;
  if (terms_out) std::copy(tt.dx.vterm.begin() + b, tt.dx.vterm.begin() + e, terms_out);
  return 0;
}

}  // extern "C"
