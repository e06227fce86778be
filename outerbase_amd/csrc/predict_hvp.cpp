// Hessian-vector and Jacobian-vector product of the multi-response predictor: host side.  No
// reference counterpart.  The kernel and its dispatch are in kernels_predict_hvp.hip.
//   ensure_d2_tables      the second-derivative interval tables of the mat25 / mat25pow dimensions
//   obhip_predict_hvp_multi_dev / obhip_predict_hvp_multi / obhip_predict_hvp_layout
// Every check that can refuse a call runs before the first device call, in the order of
// obhip_predict_grad_dev (predict_dx.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "obhip_internal.h"

using namespace obhip;

namespace obhip {

namespace {
}

// Second-derivative interval tables, beside build_dx_tables_host (predict_dx.cpp): per interval J of
// the sorted u_j and level c the six sums over the knots of d2k/du2 = -(1/3) (1 + h - h^2) e^{-h}
// (even in u - u_j) expanded around ref = u_(J-1):
//   h = t + d_j (j < J):   d2k/du2 = -e^{-t} e^{-d_j} [(1 + d_j - d_j^2) + t (1 - 2 d_j) - t^2] / 3
//   h = d_j - t (j >= J):  d2k/du2 = -e^{+t} e^{-d_j} [(1 + d_j - d_j^2) - t (1 - 2 d_j) - t^2] / 3
// so the device evaluates e^{-t} (A0 + t (A1 + t A2)) + e^{+t} (B0 + t (t B2 - B1)) as it does the
// value.  Summed per knot in extended precision: what cancels is what cancels in the knot sum of the
// second derivative itself, not the difference of two first-derivative sums.
static void build_d2_tables_host(const obhip_model &m, const ModelDev &md, std::vector<double> &out) {
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
          const long double q0 = 1 + dj - dj * dj, q1 = 1 - 2 * dj;
          if (j < J) {
            A0 -= w * q0;
            A1 -= w * q1;
            A2 += w;
          } else {
            B0 -= w * q0;
            B1 -= w * q1;
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

// keyed as ensure_dx_tables keys dtab: the model, its version and the level caps of the device view
int ensure_d2_tables(const obhip_model &m, obhip_terms &t) {
  obhip_terms::Dx &dx = t.dx;
  if (dx.d2tab.p && dx.tab2_model == &m && dx.tab2_version == m.version && dx.tab2_cap == t.pred_md.cap) return 0;
  std::vector<double> h;
  build_d2_tables_host(m, t.pred_md, h);
  OB_TRY(dx.d2tab.upload(h.data(), h.size()));
  dx.tab2_model = &m;
  dx.tab2_version = m.version;
  dx.tab2_cap = t.pred_md.cap;
  return 0;
}

}  // namespace obhip

static int check_hvp(const char *who, const void *m, const void *t, const void *Theta, uint64_t q, const void *x,
                     uint64_t n, const void *W, uint64_t ldw, const void *V, const void *vjp, const void *jvp,
                     const void *hvp) {
  const std::string w(who);
  if (!m || !t || !Theta || (n > 0 && (!x || !V))) return fail(OBHIP_ERR_INVALID, w + ": null model, terms, Theta, x or V");
  if (q == 0) return fail(OBHIP_ERR_INVALID, w + ": no response");
  if (W && ldw < n) return fail(OBHIP_ERR_INVALID, w + ": leading dimension of W below n");
  if (n > kMaxRowsPerCall) return fail(OBHIP_ERR_INVALID, w + ": more than 2^40 rows in one call");
  if (!jvp && !hvp) return fail(OBHIP_ERR_INVALID, w + ": neither jvp nor hvp is asked for");
  if ((vjp || hvp) && !W) return fail(OBHIP_ERR_INVALID, w + ": vjp and hvp need W");
  return 0;
}

extern "C" {

int obhip_predict_hvp_multi_dev(const obhip_model *m, const obhip_terms *t, const double *d_Theta, uint64_t q,
                                const double *d_x, uint64_t n, const double *d_W, uint64_t ldw, const double *d_V,
                                double *d_mean, double *d_vjp, double *d_jvp, double *d_hvp) {
  OB_TRY(check_hvp("predict_hvp_multi_dev", m, t, d_Theta, q, d_x, n, d_W, ldw, d_V, d_vjp, d_jvp, d_hvp));
  OB_TRY(check_compat(m, t));
  if (n == 0) return 0;
  OB_TRY(require_device());
  return launch_predict_hvp(*m, *const_cast<obhip_terms *>(t), d_Theta, q, d_x, n, d_W, ldw, d_V, d_mean, d_vjp,
                            d_jvp, d_hvp);
}

int obhip_predict_hvp_multi(const obhip_model *m, const obhip_terms *t, const double *Theta, uint64_t q,
                            const double *x, uint64_t n, uint64_t ldx, const double *W, uint64_t ldw,
                            const double *V, uint64_t ldg, double *mean, double *vjp, double *jvp, double *hvp) {
  OB_TRY(check_hvp("predict_hvp_multi", m, t, Theta, q, x, n, W, ldw, V, vjp, jvp, hvp));
  if (ldx < n || ldg < n) return fail(OBHIP_ERR_INVALID, "predict_hvp_multi: leading dimension below n");
  OB_TRY(check_compat(m, t));
  if (n == 0) return 0;
  OB_TRY(require_device());
  const uint64_t d = m->d;
  DevBuf<double> dx, dth, dw, dv, dmean, dvjp, djvp, dhvp;
  OB_TRY(upload_cols(dx, x, n, d, ldx));
  OB_TRY(upload_cols(dv, V, n, d, ldg));
  OB_TRY(dth.upload(Theta, t->p * q));
  if (W) OB_TRY(upload_cols(dw, W, n, q, ldw));
  if (mean) OB_TRY(dmean.alloc(n * q));
  if (vjp) OB_TRY(dvjp.alloc(n * d));
  if (jvp) OB_TRY(djvp.alloc(n * q));
  if (hvp) OB_TRY(dhvp.alloc(n * d));
  OB_TRY(obhip_predict_hvp_multi_dev(m, t, dth.p, q, dx.p, n, dw.p, n, dv.p, dmean.p, dvjp.p, djvp.p, dhvp.p));
  auto rows_back = [&](double *dst, const double *src) -> int {
    if (ldg == n) return d2h(dst, src, n * d * sizeof(double));
    std::vector<double> tmp(n * d);
    OB_TRY(d2h(tmp.data(), src, n * d * sizeof(double)));
    for (uint64_t l = 0; l < d; ++l) std::memcpy(dst + l * ldg, &tmp[l * n], n * sizeof(double));
    return 0;
  };
  if (mean) OB_TRY(d2h(mean, dmean.p, n * q * sizeof(double)));
  if (jvp) OB_TRY(d2h(jvp, djvp.p, n * q * sizeof(double)));
  if (vjp) OB_TRY(rows_back(vjp, dvjp.p));
  if (hvp) OB_TRY(rows_back(hvp, dhvp.p));
  return 0;
}

// from the levels alone (what obhip_terms::prepare will find): used columns = the ones column and
// every (dimension, level > 0) some term has
int obhip_predict_hvp_layout(const obhip_terms *t, uint64_t q, uint64_t *mu, uint64_t *tile_rows,
                             uint64_t *lds_bytes, int *fused) {
  if (!t || q == 0) return fail(OBHIP_ERR_INVALID, "predict_hvp_layout: null terms or no response");
  uint64_t Mu = 1;
  for (uint64_t l = 0; l < t->d; ++l) {
    std::vector<char> seen((size_t)t->maxlev[l] + 1, 0);
    for (uint64_t k = 0; k < t->p; ++k) seen[t->lev[k * t->d + l]] = 1;
    for (int64_t v = 1; v <= t->maxlev[l]; ++v) Mu += seen[v];
  }
  const bool fu = predict_hvp_lds(Mu, t->d, 1, false) <= kLdsBudget;
  int nqb = 1;
  if (fu && q > 16 && predict_hvp_lds(Mu, t->d, 2, false) <= kLdsBudget) nqb = 2;
  if (mu) *mu = Mu;
  if (tile_rows) *tile_rows = kHvpRows;
  if (lds_bytes) *lds_bytes = predict_hvp_lds(Mu, t->d, nqb, !fu);
  if (fused) *fused = fu ? 1 : 0;
  return 0;
}

}  // extern "C"
