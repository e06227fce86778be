// Conditional moments of the fitted mean: the entry points (include/obhip.h, "conditional moments"; DESIGN.md
// section 36).  No reference counterpart.  The kernels and their launches are in kernels_conditional.hip, the
// grouping and the chunk arithmetic in conditional_plan.h.
//   cond_setup     the checks (the level, d and p limits of the Sobol passes, the LDS bound on the noise dimensions'
//                  tables, the count of view entries), the split of the dimensions (make_split with dims_b = the
//                  noise dimensions: side A is S) and the groups
//   cond_tables    the group tables on the device: the noise dimensions' tables gathered into compact copies, the
//                  levels of every group's first term and the compact offsets up, then k_cond_tables
//   obhip_conditional_moments_dev   the tables of S (side_tables), the views of its dimensions, then chunk after
//                  chunk of rows through launch_cond_chunk
// Every check of the arguments runs before the first device call; the workspace is one block laid out by CondPlan.
#include <algorithm>
#include <string>
#include <vector>

#include "obhip_internal.h"
#include "conditional_plan.h"
#include "row_chunks.h"

using namespace obhip;

namespace {

int refuse(const char *who, const char *why) { return fail(OBHIP_ERR_INVALID, std::string(who) + ": " + why); }

struct CondSetup {
  ProductSplit split;  // side_a = S, side_b = E
  CondGroups groups;
  uint64_t n_mean = 0, n_cov = 0;      // the packed tables of all d dimensions (what the caller passes)
  uint64_t n_mean_e = 0, n_cov_e = 0;  // those of the noise dimensions alone (what k_cond_tables stages)
  uint64_t view_terms = 0;             // the (term, control dimension) pairs with a factor
  bool fused = false;
};

// what every entry checks from the terms and the noise dimensions alone: the level, d and p limits of the Sobol passes,
// and their LDS bound on the tables of the noise dimensions, the only ones k_cond_tables holds
int cond_setup(const char *who, const obhip_terms *t, const uint32_t *dims_e, uint64_t ndims_e, CondSetup &cs) {
  if (!t) return refuse(who, "null terms");
  if (t->d == 0 || t->d > 255) return refuse(who, "1 to 255 dimensions");
  if (const char *why = cond_dims_refusal(dims_e, ndims_e, t->d)) return refuse(who, why);
  if (t->p == 0 || t->p > kCondMaxP) return refuse(who, "p must be between 1 and 2^24");
  for (uint64_t l = 0; l < t->d; ++l) {
    if (t->maxlev[l] > 255)
      return fail(OBHIP_ERR_INVALID, std::string(who) + ": a level beyond 255 in dimension " + std::to_string(l));
    const uint64_t L = (uint64_t)t->maxlev[l] + 1;
    cs.n_mean += L, cs.n_cov += L * L;
  }
  for (uint64_t e = 0; e < ndims_e; ++e) {
    const uint64_t L = (uint64_t)t->maxlev[dims_e[e]] + 1;
    cs.n_mean_e += L, cs.n_cov_e += L * L;
  }
  if (cond_tables_lds(cs.n_cov_e) > kLdsBudget)
    return fail(OBHIP_ERR_INVALID, std::string(who) + ": the tables of the noise dimensions (" +
                                       std::to_string(cs.n_cov_e) + " covariances) do not fit the LDS of a workgroup");
  OB_TRY(make_split(who, *t, dims_e, ndims_e, cs.split));
  if (cs.split.mu_a > 65535) return refuse(who, "more than 65535 used basis columns on the control dimensions");
  cs.groups = cond_groups(t->lev.data(), t->p, t->d, dims_e, ndims_e);
  if (cs.groups.G > kCondMaxGroups) return refuse(who, "more than 16384 distinct level tuples on the noise dimensions");
  for (int l : cs.split.side_a)
    for (uint64_t k = 0; k < t->p; ++k) cs.view_terms += t->lev[k * t->d + l] > 0;
  if (cs.view_terms >= (1ull << 31)) return refuse(who, "more than 2^31 term factors on the control dimensions");
  cs.fused = cond_rows_supports(cs.split.mu_a, cs.split.side_a.size(), cs.split.wa);
  return 0;
}

// mE (ldk entries, zeros behind G) and K (ldk x ldk, zeros behind G) on the device.  The tables of the noise dimensions
// are gathered into compact copies first, so that the kernel's LDS holds them and nothing else
int cond_tables(const obhip_terms &t, const CondSetup &cs, const double *d_mtab, const double *d_ctab, double *d_mE,
                double *d_K, uint64_t ldk) {
  const uint64_t G = cs.groups.G, ne = cs.split.side_b.size(), d = t.d;
  std::vector<uint8_t> glev(G * ne);
  for (uint64_t g = 0; g < G; ++g)
    for (uint64_t e = 0; e < ne; ++e) glev[g * ne + e] = (uint8_t)t.lev[cs.groups.first[g] * d + cs.split.side_b[e]];
  std::vector<uint64_t> om(d + 1, 0), oc(d + 1, 0);
  for (uint64_t l = 0; l < d; ++l) {
    const uint64_t L = (uint64_t)t.maxlev[l] + 1;
    om[l + 1] = om[l] + L, oc[l + 1] = oc[l] + L * L;
  }
  DevBuf<uint8_t> dl;
  DevBuf<int> dm;
  DevBuf<double> me, ce;
  OB_TRY(me.alloc(cs.n_mean_e));
  OB_TRY(ce.alloc(cs.n_cov_e));
  std::vector<int> meta(3 * ne);
  uint64_t ome = 0, oce = 0;
  for (uint64_t e = 0; e < ne; ++e) {
    const uint64_t l = (uint64_t)cs.split.side_b[e], L = (uint64_t)t.maxlev[l] + 1;
    meta[e] = (int)L, meta[ne + e] = (int)ome, meta[2 * ne + e] = (int)oce;
    OB_HIP(hipMemcpyAsync(me.p + ome, d_mtab + om[l], L * sizeof(double), hipMemcpyDeviceToDevice, cur_stream()));
    OB_HIP(hipMemcpyAsync(ce.p + oce, d_ctab + oc[l], L * L * sizeof(double), hipMemcpyDeviceToDevice, cur_stream()));
    ome += L, oce += L * L;
  }
  OB_TRY(dl.upload(glev.data(), glev.size()));
  OB_TRY(dm.upload(meta.data(), meta.size()));
  if (ldk > G) {
    OB_HIP(hipMemsetAsync(d_mE, 0, ldk * sizeof(double), cur_stream()));
    OB_HIP(hipMemsetAsync(d_K, 0, ldk * ldk * sizeof(double), cur_stream()));
  }
  OB_TRY(launch_cond_tables(dl.p, dm.p, G, ne, cs.n_cov_e, me.p, ce.p, d_mE, d_K, ldk));
  OB_HIP(hipStreamSynchronize(cur_stream()));  // the uploads and the copies go away
  return 0;
}

}  // namespace

extern "C" {

int obhip_conditional_layout(const obhip_terms *t, const uint32_t *dims_e, uint64_t ndims_e, uint64_t *n_groups,
                             uint32_t *group_of, uint64_t *mu_s, int *fused) {
  CondSetup cs;
  OB_TRY(cond_setup("conditional_layout", t, dims_e, ndims_e, cs));
  if (n_groups) *n_groups = cs.groups.G;
  if (group_of) std::copy(cs.groups.group_of.begin(), cs.groups.group_of.end(), group_of);
  if (mu_s) *mu_s = cs.split.mu_a;
  if (fused) *fused = cs.fused ? 1 : 0;
  return 0;
}

int obhip_conditional_tables_dev(const obhip_terms *t, const uint32_t *dims_e, uint64_t ndims_e,
                                 const double *d_mean_tab, const double *d_cov_tab, double *d_mE, double *d_K) {
  if (!t || !d_mean_tab || !d_cov_tab || !d_mE || !d_K)
    return refuse("conditional_tables_dev", "null terms, tables, mE or K");
  CondSetup cs;
  OB_TRY(cond_setup("conditional_tables_dev", t, dims_e, ndims_e, cs));
  OB_TRY(require_device());
  return cond_tables(*t, cs, d_mean_tab, d_cov_tab, d_mE, d_K, cs.groups.G);
}

int obhip_conditional_moments_dev(const obhip_model *m, const obhip_terms *t, const double *d_Theta, uint64_t q,
                                  const uint32_t *dims_e, uint64_t ndims_e, const double *d_mean_tab,
                                  const double *d_cov_tab, const double *d_xs, uint64_t n, uint64_t chunk_rows,
                                  double *d_mean, double *d_var, double *d_gradmean, double *d_gradvar) {
  const char *who = "conditional_moments_dev";
  if (!m || !t || !d_Theta || !d_mean_tab || !d_cov_tab || (!d_xs && n > 0))
    return refuse(who, "null model, terms, Theta, tables or xs");
  if (const char *why = cond_sizes_refusal(t->p, t->d, q, n, chunk_rows)) return refuse(who, why);
  OB_TRY(check_compat(m, t));
  CondSetup cs;
  OB_TRY(cond_setup(who, t, dims_e, ndims_e, cs));
  if (n == 0 || (!d_mean && !d_var && !d_gradmean && !d_gradvar)) return 0;
  OB_TRY(require_device());
  obhip_terms &tt = *const_cast<obhip_terms *>(t);
  const bool grad = d_gradmean || d_gradvar;
  OB_TRY(prepare_predict(*m, tt, grad));
  const ProductSplit &s = cs.split;
  const CondGroups &gr = cs.groups;
  const uint64_t p = t->p, d = t->d, ns = s.side_a.size(), W2 = s.wa / 2;
  const CondPlan plan = cond_plan(gr.G, q, n, chunk_rows);
  const uint64_t Gp = plan.Gp();

  // the tables of S and, for the gradients, the views of its dimensions: W2 words of the term's other columns (own
  // slot = the ones column), its own used column, its index
  std::vector<int32_t> cpos;
  std::vector<uint16_t> cols;
  side_tables(tt, s, s.side_a, s.wa, cpos, cols);
  std::vector<uint32_t> vw(W2 + 2, 0), voff(ns + 1, 0);
  if (grad) {
    const std::vector<DimDesc> &dims = tt.pred_md.dims_h;
    const uint64_t nent = cs.view_terms;
    vw.assign(std::max<uint64_t>(nent, 1) * (W2 + 2), 0);
    std::vector<uint16_t> other(s.wa);
    uint64_t e = 0;
    for (uint64_t a = 0; a < ns; ++a) {
      const uint64_t l = (uint64_t)s.side_a[a];
      for (uint64_t k = 0; k < p; ++k) {
        const uint32_t v = (uint32_t)t->lev[k * d + l];
        if (v == 0) continue;
        const int32_t own = cpos[dims[l].ccol0 + v - 1];
        // (not an argument check: the side's tables disagree with the terms, which no caller's input can bring about)
        if (own < 1) return fail(OBHIP_ERR_STATE, "conditional_moments_dev: a term's column is not in the used list");
        std::copy(cols.begin() + k * s.wa, cols.begin() + (k + 1) * s.wa, other.begin());
        *std::find(other.begin(), other.end(), (uint16_t)own) = 0;
        uint32_t *ent = &vw[e++ * (W2 + 2)];
        for (uint64_t w = 0; w < W2; ++w) ent[w] = (uint32_t)other[2 * w] | ((uint32_t)other[2 * w + 1] << 16);
        ent[W2] = (uint32_t)own;
        ent[W2 + 1] = (uint32_t)k;
      }
      voff[a + 1] = (uint32_t)e;
    }
  }
  DevBuf<int> dside;
  DevBuf<int32_t> dcpos;
  DevBuf<uint16_t> dcols;
  DevBuf<uint32_t> dorder, dgoff, dgof, dvw, dvoff;
  DevBuf<double> ws, xc;
  OB_TRY(dside.upload(s.side_a.data(), ns));
  OB_TRY(dcpos.upload(cpos.data(), cpos.size()));
  OB_TRY(dcols.upload(cols.data(), cols.size()));
  OB_TRY(dorder.upload(gr.order.data(), p));
  OB_TRY(dgoff.upload(gr.off.data(), gr.G + 1));
  OB_TRY(dgof.upload(gr.group_of.data(), p));
  OB_TRY(dvw.upload(vw.data(), vw.size()));
  OB_TRY(dvoff.upload(voff.data(), voff.size()));
  OB_TRY(ws.alloc(plan.workspace_doubles()));
  double *mE = ws.p + plan.off_mE(), *K = ws.p + plan.off_K();
  OB_TRY(cond_tables(*t, cs, d_mean_tab, d_cov_tab, mE, K, Gp));

  CondChunk c;
  const PredTabs T = pred_tabs(*m, tt);
  c.dims = T.dims, c.ka = T.ka, c.kb = T.kb, c.kc = T.kc, c.rot = T.rot, c.tab = T.tab, c.dtab = T.dtab;
  c.side = dside.p, c.cpos = dcpos.p, c.nside = (int)ns, c.mu = (int)s.mu_a, c.W2 = (int)W2, c.p = (int)p;
  c.colsw = (const uint32_t *)dcols.p, c.order = dorder.p, c.goff = dgoff.p, c.gof = dgof.p;
  c.G = (int)gr.G, c.Gp = (int)Gp, c.q = (int)q;
  c.vw = dvw.p, c.voff = dvoff.p;
  c.Theta = d_Theta, c.mE = mE, c.K = K;
  c.n = n, c.C = ws.p + plan.off_C(), c.Y = ws.p + plan.off_Y(), c.Mw = ws.p + plan.off_M(), c.Ww = ws.p + plan.off_W();
  c.mean = d_mean, c.var = d_var, c.gradmean = d_gradmean, c.gradvar = d_gradvar, c.scratch = nullptr;
  c.fused = cs.fused && !getenv("OBHIP_FORCE_GENERIC");
  const RowChunks chunks = plan.chunks();
  for (uint64_t ci = 0; ci < chunks.count(); ++ci) {
    const RowChunk rc = chunks.at(ci);
    OB_TRY(gather_rows(xc, d_xs, n, ns, rc, &c.x));
    c.ldx = rc.whole ? n : rc.nr;
    c.nr = rc.nr, c.npad = rc.npad, c.ntiles = rc.npad / kTileRows, c.row0 = rc.r0;
    OB_TRY(launch_cond_chunk(c));
  }
  OB_HIP(hipStreamSynchronize(cur_stream()));  // the workspace and the tables go away
  return 0;
}

int obhip_conditional_tables(const obhip_terms *t, const uint32_t *dims_e, uint64_t ndims_e, const double *mean_tab,
                             const double *cov_tab, double *mE, double *K) {
  if (!t || !mean_tab || !cov_tab || !mE || !K) return refuse("conditional_tables", "null terms, tables, mE or K");
  CondSetup cs;
  OB_TRY(cond_setup("conditional_tables", t, dims_e, ndims_e, cs));
  OB_TRY(require_device());
  const uint64_t G = cs.groups.G;
  DevBuf<double> dm, dc, dmE, dK;
  OB_TRY(dm.upload(mean_tab, cs.n_mean));
  OB_TRY(dc.upload(cov_tab, cs.n_cov));
  OB_TRY(dmE.alloc(G));
  OB_TRY(dK.alloc(G * G));
  OB_TRY(obhip_conditional_tables_dev(t, dims_e, ndims_e, dm.p, dc.p, dmE.p, dK.p));
  OB_TRY(d2h(mE, dmE.p, G * sizeof(double)));
  return d2h(K, dK.p, G * G * sizeof(double));
}

int obhip_conditional_moments(const obhip_model *m, const obhip_terms *t, const double *Theta, uint64_t q,
                              const uint32_t *dims_e, uint64_t ndims_e, const double *mean_tab, const double *cov_tab,
                              const double *xs, uint64_t n, uint64_t ldx, uint64_t chunk_rows, double *mean,
                              double *var, double *gradmean, double *gradvar) {
  const char *who = "conditional_moments";
  if (!m || !t || !Theta || !mean_tab || !cov_tab || (!xs && n > 0))
    return refuse(who, "null model, terms, Theta, tables or xs");
  if (const char *why = cond_sizes_refusal(t->p, t->d, q, n, chunk_rows)) return refuse(who, why);
  if (ldx < n) return refuse(who, "leading dimension below n");
  OB_TRY(check_compat(m, t));
  CondSetup cs;
  OB_TRY(cond_setup(who, t, dims_e, ndims_e, cs));
  if (n == 0) return 0;
  OB_TRY(require_device());
  const uint64_t ns = cs.split.side_a.size();
  DevBuf<double> dx, dth, dm, dc, o[4];
  double *host[4] = {mean, var, gradmean, gradvar};
  const uint64_t cnt[4] = {n * q, n * q, n * ns * q, n * ns * q};
  OB_TRY(upload_cols(dx, xs, n, ns, ldx));
  OB_TRY(dth.upload(Theta, t->p * q));
  OB_TRY(dm.upload(mean_tab, cs.n_mean));
  OB_TRY(dc.upload(cov_tab, cs.n_cov));
  for (int i = 0; i < 4; ++i)
    if (host[i]) OB_TRY(o[i].alloc(cnt[i]));
  OB_TRY(obhip_conditional_moments_dev(m, t, dth.p, q, dims_e, ndims_e, dm.p, dc.p, dx.p, n, chunk_rows, o[0].p, o[1].p,
                                       o[2].p, o[3].p));
  for (int i = 0; i < 4; ++i)
    if (host[i]) OB_TRY(d2h(host[i], o[i].p, cnt[i] * sizeof(double)));
  return 0;
}

}  // extern "C"
