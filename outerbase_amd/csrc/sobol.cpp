// Variance-based sensitivity of the fitted mean: the entry points (include/obhip.h, "variance-based
// sensitivity" and "active subspaces").  No reference counterpart.  The kernels and their launches are in
// kernels_sobol.hip, kernels_shapley.hip and kernels_active.hip.
// Every check that can refuse a call runs before the first device call.
#include "obhip_internal.h"
#include "sens_plan.h"

#include <cfloat>
#include <cmath>

using namespace obhip;

namespace {

constexpr uint64_t kSobolMaxQ = 65535;  // a grid dimension of the per-response kernels

struct Layout {
  uint64_t d = 0, lmax = 1, n_mean = 0, n_cov = 0;
};

// the packed-table layout of a term set; refuses what the kernels cannot hold
int sobol_layout(const char *who, const obhip_terms &t, Layout &lay) {
  lay.d = t.d;
  if (t.d == 0 || t.d > 255) return fail(OBHIP_ERR_INVALID, std::string(who) + ": 1 to 255 dimensions");
  for (uint64_t l = 0; l < t.d; ++l) {
    if (t.maxlev[l] > 255)
      return fail(OBHIP_ERR_INVALID, std::string(who) + ": a level beyond 255 in dimension " + std::to_string(l));
    const uint64_t L = (uint64_t)t.maxlev[l] + 1;
    lay.lmax = std::max(lay.lmax, L);
    lay.n_mean += L;
    lay.n_cov += L * L;
  }
  if (sobol_pairs_lds(t.d, lay.n_cov) > kLdsBudget)
    return fail(OBHIP_ERR_INVALID, std::string(who) + ": the tables of these terms (" + std::to_string(lay.n_cov) +
                                       " covariances) do not fit the LDS of a workgroup");
  return 0;
}

// sobol_layout with the limits of the gradient tables on top: three tables of n_cov entries in the LDS of
// k_block_pairs<ActiveOp>, two basis tiles in that of the derivative moments
int active_layout(const char *who, const obhip_terms &t, Layout &lay) {
  OB_TRY(sobol_layout(who, t, lay));
  if (active_pairs_lds(lay.n_cov) > kLdsBudget || active_moments_lds(lay.lmax) > kLdsBudget)
    return fail(OBHIP_ERR_INVALID, std::string(who) + ": the tables of these terms (" + std::to_string(lay.n_cov) +
                                       " entries each) do not fit the LDS of a workgroup");
  return 0;
}

uint64_t align256(uint64_t b) { return (b + 255) / 256 * 256; }

int check_q(const char *who, uint64_t q) {
  if (q == 0 || q > kSobolMaxQ) return fail(OBHIP_ERR_INVALID, std::string(who) + ": 1 to 65535 responses");
  return 0;
}

// the nodes of a measure and, where there are weights, their leading dimension
int check_nodes(const char *who, uint64_t n, uint64_t ldx, bool weights, uint64_t ldw) {
  const std::string w(who);
  if (n == 0) return fail(OBHIP_ERR_INVALID, w + ": no nodes, so no measure");
  if (n > kMaxRowsPerCall) return fail(OBHIP_ERR_INVALID, w + ": more than 2^40 nodes in one call");
  if (ldx < n) return fail(OBHIP_ERR_INVALID, w + ": leading dimension of the nodes below n");
  if (weights && ldw < n) return fail(OBHIP_ERR_INVALID, w + ": leading dimension of the weights below n");
  return 0;
}

// the arguments of a *_workspace_bytes call
int check_ws_args(const char *who, uint64_t p, uint64_t d, uint64_t q, const uint64_t *bytes) {
  if (!bytes || p == 0 || d == 0 || d > 255 || q == 0 || q > kSobolMaxQ || p > (1ull << 24))
    return fail(OBHIP_ERR_INVALID, std::string(who) + ": null bytes, or p, d, q out of range");
  return 0;
}

// the workspace of a pair sum that also needs the exclusion products: excl (p x d), u (p), the partials
struct PairWs {
  double *excl, *u, *part;
  PairWs(void *ws, uint64_t p, uint64_t d)
      : excl((double *)ws), u((double *)((char *)ws + align256(p * d * sizeof(double)))),
        part((double *)((char *)ws + align256(p * d * sizeof(double)) + align256(p * sizeof(double)))) {}
  static uint64_t bytes(uint64_t p, uint64_t d, uint64_t part_doubles) {
    return align256(p * d * sizeof(double)) + align256(p * sizeof(double)) + align256(part_doubles * sizeof(double));
  }
};

// the device side of a host entry: Theta and the mean and covariance tables up, the output and the workspace
struct HostSums {
  DevBuf<double> th, mean, cov, out;
  DevBuf<char> ws;
  uint64_t n_out = 0;
  int up(const obhip_terms *t, const Layout &lay, const double *Theta, uint64_t q, const double *mean_tab,
         const double *cov_tab, uint64_t out_doubles, uint64_t ws_bytes) {
    n_out = out_doubles;
    OB_TRY(th.upload(Theta, t->p * q));
    OB_TRY(mean.upload(mean_tab, lay.n_mean));
    OB_TRY(cov.upload(cov_tab, lay.n_cov));
    OB_TRY(out.alloc(n_out));
    return ws.alloc(ws_bytes);
  }
  int down(double *host_out) { return d2h(host_out, out.p, n_out * sizeof(double)); }
};

// levels as bytes and the table offsets on the device, once per term set
int ensure_sobol_tables(obhip_terms &t) {
  if (t.sobol_lev.p && t.sobol_meta.p) return 0;
  std::vector<uint8_t> lev(t.p * t.d);
  for (uint64_t i = 0; i < t.p * t.d; ++i) lev[i] = (uint8_t)t.lev[i];
  std::vector<int> meta(3 * t.d);
  int om = 0, oc = 0;
  for (uint64_t l = 0; l < t.d; ++l) {
    const int L = (int)t.maxlev[l] + 1;
    meta[l] = L;
    meta[t.d + l] = om;
    meta[2 * t.d + l] = oc;
    om += L;
    oc += L * L;
  }
  OB_TRY(t.sobol_lev.upload(lev.data(), lev.size()));
  OB_TRY(t.sobol_meta.upload(meta.data(), meta.size()));
  return 0;
}

// the pairs i < j of dimensions in the order (0,1), (0,2), .. (0,d-1), (1,2), ..
struct PairLayout {
  uint64_t n_pairs = 0, n_G = 0, gmax = 1;
};

PairLayout pair_layout(const obhip_terms &t) {
  PairLayout pl;
  for (uint64_t i = 0; i < t.d; ++i)
    for (uint64_t j = i + 1; j < t.d; ++j) {
      const uint64_t g = ((uint64_t)t.maxlev[i] + 1) * ((uint64_t)t.maxlev[j] + 1);
      ++pl.n_pairs;
      pl.n_G += g;
      pl.gmax = std::max(pl.gmax, g);
    }
  return pl;
}

// i, j and the offset of G_ij on the device, once per term set
int ensure_sobol_pairs(obhip_terms &t) {
  if (t.sobol_pairs.p || t.d < 2) return 0;
  std::vector<int> pr;
  int go = 0;
  for (uint64_t i = 0; i < t.d; ++i)
    for (uint64_t j = i + 1; j < t.d; ++j) {
      pr.push_back((int)i), pr.push_back((int)j), pr.push_back(go);
      go += ((int)t.maxlev[i] + 1) * ((int)t.maxlev[j] + 1);
    }
  return t.sobol_pairs.upload(pr.data(), pr.size());
}

// The players of a call and the sweep the pair kernel makes over them (ShapPlan, obhip_internal.h); refuses ids
// that are not exactly 0 .. P-1 and more players than the kernel has slots.  groups == NULL: player l = dimension l.
int shapley_plan(const char *who, const obhip_terms &t, const int32_t *groups, ShapPlan &plan) {
  const uint64_t d = t.d;
  std::vector<int> gid(d);
  uint64_t P = 0;
  for (uint64_t l = 0; l < d; ++l) {
    gid[l] = groups ? groups[l] : (int)l;
    if (gid[l] < 0 || (uint64_t)gid[l] >= d)
      return fail(OBHIP_ERR_INVALID, std::string(who) + ": player id of dimension " + std::to_string(l) +
                                         " outside 0 .. d-1");
    P = std::max<uint64_t>(P, (uint64_t)gid[l] + 1);
  }
  std::vector<int> count(P, 0);
  for (uint64_t l = 0; l < d; ++l) ++count[gid[l]];
  for (uint64_t g = 0; g < P; ++g)
    if (!count[g])
      return fail(OBHIP_ERR_INVALID, std::string(who) + ": player ids must be 0 .. P-1 without a gap; " +
                                         std::to_string(g) + " is not used");
  if (P > (uint64_t)kShapMaxPlayers)
    return fail(OBHIP_ERR_INVALID, std::string(who) + ": " + std::to_string(P) + " players, at most " +
                                       std::to_string(kShapMaxPlayers) + " (group the dimensions)");
  plan = ShapPlan{};
  plan.nplayers = (int)P;
  plan.nnode = (int)((P + 1) / 2);
  OB_TRY(obhip_gauss_legendre01((uint64_t)plan.nnode, plan.node, plan.wt));
  // the sweep order: by player, a player's dimensions ascending
  uint64_t pos = 0;
  std::vector<uint8_t> is_last(d, 0);
  for (uint64_t g = 0; g < P; ++g) {
    for (uint64_t l = 0; l < d; ++l)
      if ((uint64_t)gid[l] == g) plan.perm[pos++] = (uint8_t)l;
    is_last[pos - 1] = 1;
  }
  // d <= NS: every dimension has a slot.  Beyond, the first d - NS dimensions that do not end a player are read
  // per pair, in front of the next slot (there are d - P >= d - NS of them)
  const uint64_t ns = std::min<uint64_t>(d, (uint64_t)shapley_slots(d));
  uint64_t nomem = d - ns, s = 0, run = 0;
  for (pos = 0; pos < d; ++pos) {
    if (nomem && !is_last[pos]) {
      --nomem, ++run;
      continue;
    }
    plan.regdim[s] = plan.perm[pos];
    plan.nmem[s / 4] |= (uint32_t)run << (8 * (s % 4));
    run = 0;
    if (is_last[pos]) {
      plan.lastmask |= 1ull << s;
      plan.slot[gid[plan.perm[pos]]] = (uint8_t)s;
    }
    ++s;
  }
  plan.ns = (int)ns;
  return 0;
}

}  // namespace

extern "C" {

int obhip_sobol_layout(const obhip_terms *t, uint64_t *n_mean, uint64_t *n_cov) {
  if (!t) return fail(OBHIP_ERR_INVALID, "sobol_layout: null terms");
  Layout lay;
  OB_TRY(sobol_layout("sobol_layout", *t, lay));
  if (n_mean) *n_mean = lay.n_mean;
  if (n_cov) *n_cov = lay.n_cov;
  return 0;
}

int obhip_dim_moments_dev(const obhip_model *m, const obhip_terms *t, const double *d_nodes, uint64_t n, uint64_t ldx,
                          const double *d_weights, uint64_t ldw, double *d_mean, double *d_cov) {
  if (!m || !t || !d_nodes || !d_mean || !d_cov)
    return fail(OBHIP_ERR_INVALID, "dim_moments_dev: null model, terms, nodes, mean or cov");
  OB_TRY(check_nodes("dim_moments_dev", n, ldx, d_weights != nullptr, ldw));
  OB_TRY(check_compat(m, t));
  Layout lay;
  OB_TRY(sobol_layout("dim_moments_dev", *t, lay));
  OB_TRY(require_device());
  int flag = 0;
  OB_TRY(launch_dim_moments(*m, *const_cast<obhip_terms *>(t), d_nodes, n, ldx, d_weights, ldw, d_mean, d_cov, &flag));
  if (flag)
    return fail(OBHIP_ERR_NUMERIC,
                "dim_moments_dev: a weight is negative or not finite, or the weights of a dimension do not sum to > 0");
  return 0;
}

int obhip_sobol_workspace_bytes(uint64_t p, uint64_t d, uint64_t q, uint64_t *bytes) {
  OB_TRY(check_ws_args("sobol_workspace_bytes", p, d, q, bytes));
  *bytes = PairWs::bytes(p, d, sobol_part_doubles(p, d, q));
  return 0;
}

int obhip_sobol_dev(const obhip_terms *t, const double *d_Theta, uint64_t q, const double *d_mean_tab,
                    const double *d_cov_tab, double *d_out, double *d_g, void *d_ws, uint64_t ws_bytes) {
  if (!t || !d_Theta || !d_mean_tab || !d_cov_tab || !d_out || !d_ws)
    return fail(OBHIP_ERR_INVALID, "sobol_dev: null terms, Theta, tables, out or workspace");
  OB_TRY(check_q("sobol_dev", q));
  Layout lay;
  OB_TRY(sobol_layout("sobol_dev", *t, lay));
  uint64_t need = 0;
  OB_TRY(obhip_sobol_workspace_bytes(t->p, t->d, q, &need));
  if (ws_bytes < need) return fail(OBHIP_ERR_INVALID, "sobol_dev: workspace smaller than obhip_sobol_workspace_bytes");
  OB_TRY(require_device());
  obhip_terms &tt = *const_cast<obhip_terms *>(t);
  OB_TRY(ensure_sobol_tables(tt));
  const uint64_t p = t->p, d = t->d;
  const PairWs ws(d_ws, p, d);
  OB_TRY(launch_sobol_first(tt.sobol_lev.p, tt.sobol_meta.p, p, d, q, lay.lmax, lay.n_mean, d_Theta, d_mean_tab,
                            d_cov_tab, ws.excl, ws.u, d_out, d_g));
  return launch_sobol_pairs(tt.sobol_lev.p, tt.sobol_meta.p, p, d, q, lay.n_cov, d_Theta, d_mean_tab, d_cov_tab,
                            ws.part, d_out);
}

int obhip_sobol2_layout(const obhip_terms *t, uint64_t *n_pairs, uint64_t *n_G) {
  if (!t) return fail(OBHIP_ERR_INVALID, "sobol2_layout: null terms");
  Layout lay;
  OB_TRY(sobol_layout("sobol2_layout", *t, lay));
  const PairLayout pl = pair_layout(*t);
  if (n_pairs) *n_pairs = pl.n_pairs;
  if (n_G) *n_G = pl.n_G;
  return 0;
}

int obhip_sobol2_workspace_bytes(uint64_t p, uint64_t d, uint64_t q, uint64_t *bytes) {
  OB_TRY(check_ws_args("sobol2_workspace_bytes", p, d, q, bytes));
  const uint64_t part = pair_part_doubles(p, d, q, kSobol2T, kSobolRC, kSobolTW);
  *bytes = std::max<uint64_t>(256, align256(part * sizeof(double)));
  return 0;
}

int obhip_sobol2_dev(const obhip_terms *t, const double *d_Theta, uint64_t q, const double *d_mean_tab,
                     const double *d_cov_tab, double *d_out, double *d_G, void *d_ws, uint64_t ws_bytes) {
  if (!t || !d_Theta || !d_mean_tab || !d_cov_tab)
    return fail(OBHIP_ERR_INVALID, "sobol2_dev: null terms, Theta or tables");
  OB_TRY(check_q("sobol2_dev", q));
  Layout lay;
  OB_TRY(sobol_layout("sobol2_dev", *t, lay));
  if (t->d == 1) return 0;  // no pairs: nothing to write
  if (!d_out || !d_ws) return fail(OBHIP_ERR_INVALID, "sobol2_dev: null out or workspace");
  uint64_t need = 0;
  OB_TRY(obhip_sobol2_workspace_bytes(t->p, t->d, q, &need));
  if (ws_bytes < need)
    return fail(OBHIP_ERR_INVALID, "sobol2_dev: workspace smaller than obhip_sobol2_workspace_bytes");
  const PairLayout pl = pair_layout(*t);
  OB_TRY(require_device());
  obhip_terms &tt = *const_cast<obhip_terms *>(t);
  OB_TRY(ensure_sobol_tables(tt));
  OB_TRY(ensure_sobol_pairs(tt));
  OB_TRY(launch_sobol2_second(tt.sobol_lev.p, tt.sobol_meta.p, tt.sobol_pairs.p, t->p, t->d, q, pl.n_pairs, pl.n_G,
                              pl.gmax, d_Theta, d_mean_tab, d_cov_tab, d_out, d_G));
  return launch_sobol2_pairs(tt.sobol_lev.p, tt.sobol_meta.p, t->p, t->d, q, lay.n_cov, d_Theta, d_mean_tab, d_cov_tab,
                             (double *)d_ws, d_out);
}

int obhip_gauss_legendre01(uint64_t G, double *nodes, double *weights) {
  if (G == 0 || G > 128 || !nodes || !weights)
    return fail(OBHIP_ERR_INVALID, "gauss_legendre01: 1 to 128 nodes, and somewhere to put them");
  // Newton on Q_G(s) = (-1)^G P_G(2 s - 1) for the nodes below 1/2, the others by symmetry.  The recurrence runs
  // on the differences D_k = Q_k - Q_{k-1}, (k + 1) D_{k+1} = k D_k - 2 (2 k + 1) s Q_k, which takes s itself and
  // never forms 2 s - 1: a node near 0 keeps its relative accuracy.  w = 1 / (s (1 - s) Q_G'(s)^2).
  const long double pi = 3.141592653589793238462643383279502884L;
  for (uint64_t i = 0; i < (G + 1) / 2; ++i) {
    const long double th = pi * ((long double)i + 0.75L) / ((long double)G + 0.5L), sh = sinl(0.5L * th);
    long double s = sh * sh, dq = 0.0L;
    if (2 * i + 1 == G) s = 0.5L;
    for (int it = 0; it < 100; ++it) {
      long double q = 1.0L, dk = 0.0L, ddk = 0.0L;
      dq = 0.0L;
      for (uint64_t k = 0; k < G; ++k) {
        const long double kk = (long double)k;
        const long double dn = (kk * dk - 2.0L * (2.0L * kk + 1.0L) * s * q) / (kk + 1.0L);
        const long double ddn = (kk * ddk - 2.0L * (2.0L * kk + 1.0L) * (q + s * dq)) / (kk + 1.0L);
        q += dn, dq += ddn, dk = dn, ddk = ddn;
      }
      if (2 * i + 1 == G) break;                         // (the middle node of an odd rule is 1/2 itself)
      const long double step = q / dq;
      s -= step;
      if (fabsl(step) <= 4.0L * LDBL_EPSILON * s) break;
    }
    const long double w = 1.0L / (s * (1.0L - s) * dq * dq);
    nodes[i] = (double)s, weights[i] = (double)w;
    nodes[G - 1 - i] = (double)(1.0L - s), weights[G - 1 - i] = (double)w;
  }
  return 0;
}

int obhip_shapley_layout(const obhip_terms *t, const int32_t *groups, uint64_t *n_players, uint64_t *n_nodes) {
  if (!t) return fail(OBHIP_ERR_INVALID, "shapley_layout: null terms");
  Layout lay;
  OB_TRY(sobol_layout("shapley_layout", *t, lay));
  ShapPlan plan;
  OB_TRY(shapley_plan("shapley_layout", *t, groups, plan));
  if (n_players) *n_players = (uint64_t)plan.nplayers;
  if (n_nodes) *n_nodes = (uint64_t)plan.nnode;
  return 0;
}

int obhip_shapley_workspace_bytes(uint64_t p, uint64_t d, uint64_t q, uint64_t *bytes) {
  OB_TRY(check_ws_args("shapley_workspace_bytes", p, d, q, bytes));
  *bytes = align256(shapley_part_doubles(p, d, q) * sizeof(double));
  return 0;
}

int obhip_shapley_dev(const obhip_terms *t, const int32_t *groups, const double *d_Theta, uint64_t q,
                      const double *d_mean_tab, const double *d_cov_tab, double *d_out, void *d_ws, uint64_t ws_bytes) {
  if (!t || !d_Theta || !d_mean_tab || !d_cov_tab || !d_out || !d_ws)
    return fail(OBHIP_ERR_INVALID, "shapley_dev: null terms, Theta, tables, out or workspace");
  OB_TRY(check_q("shapley_dev", q));
  Layout lay;
  OB_TRY(sobol_layout("shapley_dev", *t, lay));  // (tables that fit k_sobol_pairs fit k_shapley_pairs: two of three)
  if (shapley_pairs_lds(t->d, lay.n_cov) > kLdsBudget)
    return fail(OBHIP_ERR_INVALID, "shapley_dev: the tables of these terms do not fit the LDS of a workgroup");
  ShapPlan plan;
  OB_TRY(shapley_plan("shapley_dev", *t, groups, plan));
  uint64_t need = 0;
  OB_TRY(obhip_shapley_workspace_bytes(t->p, t->d, q, &need));
  if (ws_bytes < need)
    return fail(OBHIP_ERR_INVALID, "shapley_dev: workspace smaller than obhip_shapley_workspace_bytes");
  OB_TRY(require_device());
  obhip_terms &tt = *const_cast<obhip_terms *>(t);
  OB_TRY(ensure_sobol_tables(tt));
  return launch_shapley_pairs(plan, tt.sobol_lev.p, tt.sobol_meta.p, t->p, t->d, q, lay.n_cov, d_Theta, d_mean_tab,
                              d_cov_tab, (double *)d_ws, d_out);
}

int obhip_interaction_effect_dev(const obhip_model *m, const obhip_terms *t, uint64_t dim_i, uint64_t dim_j,
                                 const double *d_G, uint64_t q, const double *d_grid_i, uint64_t Gi,
                                 const double *d_grid_j, uint64_t Gj, double *d_out) {
  if (!m || !t || !d_G || !d_grid_i || !d_grid_j || !d_out)
    return fail(OBHIP_ERR_INVALID, "interaction_effect_dev: null model, terms, G, grids or out");
  OB_TRY(check_q("interaction_effect_dev", q));
  if (Gi > (1ull << 32) || Gj > (1ull << 32) || Gi * Gj > (1ull << 32))
    return fail(OBHIP_ERR_INVALID, "interaction_effect_dev: more than 2^32 grid points in one call");
  OB_TRY(check_compat(m, t));
  if (dim_i >= m->d || dim_j >= m->d) return fail(OBHIP_ERR_INVALID, "interaction_effect_dev: dimension out of range");
  if (dim_i == dim_j) return fail(OBHIP_ERR_INVALID, "interaction_effect_dev: the two dimensions are the same");
  Layout lay;
  OB_TRY(sobol_layout("interaction_effect_dev", *t, lay));
  if (Gi * Gj == 0) return 0;
  OB_TRY(require_device());
  // G is stored for the lower dimension first: the other order reads it transposed
  const uint64_t lo = std::min(dim_i, dim_j), hi = std::max(dim_i, dim_j);
  uint64_t goff = 0;
  for (uint64_t i = 0; i <= lo; ++i)
    for (uint64_t j = i + 1; j < (i == lo ? hi : t->d); ++j)
      goff += ((uint64_t)t->maxlev[i] + 1) * ((uint64_t)t->maxlev[j] + 1);
  return launch_interaction_effect(*m, *const_cast<obhip_terms *>(t), dim_i, dim_j, d_G + goff, pair_layout(*t).n_G, q,
                                   d_grid_i, Gi, d_grid_j, Gj, d_out);
}

int obhip_main_effect_dev(const obhip_model *m, const obhip_terms *t, uint64_t dim, const double *d_g, uint64_t q,
                          const double *d_grid, uint64_t G, double *d_out) {
  if (!m || !t || !d_g || !d_grid || !d_out)
    return fail(OBHIP_ERR_INVALID, "main_effect_dev: null model, terms, g, grid or out");
  OB_TRY(check_q("main_effect_dev", q));
  if (G > kMaxRowsPerCall) return fail(OBHIP_ERR_INVALID, "main_effect_dev: more than 2^40 grid points in one call");
  OB_TRY(check_compat(m, t));
  if (dim >= m->d) return fail(OBHIP_ERR_INVALID, "main_effect_dev: dimension out of range");
  Layout lay;
  OB_TRY(sobol_layout("main_effect_dev", *t, lay));
  if (G == 0) return 0;
  OB_TRY(require_device());
  return launch_main_effect(*m, *const_cast<obhip_terms *>(t), dim, d_g, q, d_grid, G, d_out);
}

int obhip_dim_moments(const obhip_model *m, const obhip_terms *t, const double *nodes, uint64_t n, uint64_t ldx,
                      const double *weights, uint64_t ldw, double *mean, double *cov) {
  if (!m || !t || !nodes || !mean || !cov)
    return fail(OBHIP_ERR_INVALID, "dim_moments: null model, terms, nodes, mean or cov");
  OB_TRY(check_nodes("dim_moments", n, ldx, weights != nullptr, ldw));
  OB_TRY(check_compat(m, t));
  Layout lay;
  OB_TRY(sobol_layout("dim_moments", *t, lay));
  OB_TRY(require_device());
  DevBuf<double> dx, dw, dm, dc;
  OB_TRY(upload_cols(dx, nodes, n, m->d, ldx));
  if (weights) OB_TRY(upload_cols(dw, weights, n, m->d, ldw));
  OB_TRY(dm.alloc(lay.n_mean));
  OB_TRY(dc.alloc(lay.n_cov));
  OB_TRY(obhip_dim_moments_dev(m, t, dx.p, n, n, dw.p, n, dm.p, dc.p));
  OB_TRY(d2h(mean, dm.p, lay.n_mean * sizeof(double)));
  return d2h(cov, dc.p, lay.n_cov * sizeof(double));
}

int obhip_sobol(const obhip_terms *t, const double *Theta, uint64_t q, const double *mean_tab, const double *cov_tab,
                double *out, double *g) {
  if (!t || !Theta || !mean_tab || !cov_tab || !out)
    return fail(OBHIP_ERR_INVALID, "sobol: null terms, Theta, tables or out");
  OB_TRY(check_q("sobol", q));
  Layout lay;
  OB_TRY(sobol_layout("sobol", *t, lay));
  uint64_t wsb = 0;
  OB_TRY(obhip_sobol_workspace_bytes(t->p, t->d, q, &wsb));
  OB_TRY(require_device());
  HostSums h;
  DevBuf<double> dg;
  OB_TRY(h.up(t, lay, Theta, q, mean_tab, cov_tab, q * (2 + 2 * t->d), wsb));
  if (g) OB_TRY(dg.alloc(q * lay.n_mean));
  OB_TRY(obhip_sobol_dev(t, h.th.p, q, h.mean.p, h.cov.p, h.out.p, dg.p, h.ws.p, wsb));
  OB_TRY(h.down(out));
  if (g) OB_TRY(d2h(g, dg.p, q * lay.n_mean * sizeof(double)));
  return 0;
}

int obhip_sobol2(const obhip_terms *t, const double *Theta, uint64_t q, const double *mean_tab, const double *cov_tab,
                 double *out, double *G) {
  if (!t || !Theta || !mean_tab || !cov_tab) return fail(OBHIP_ERR_INVALID, "sobol2: null terms, Theta or tables");
  OB_TRY(check_q("sobol2", q));
  Layout lay;
  OB_TRY(sobol_layout("sobol2", *t, lay));
  if (t->d == 1) return 0;
  if (!out) return fail(OBHIP_ERR_INVALID, "sobol2: null out");
  uint64_t wsb = 0;
  OB_TRY(obhip_sobol2_workspace_bytes(t->p, t->d, q, &wsb));
  const PairLayout pl = pair_layout(*t);
  OB_TRY(require_device());
  HostSums h;
  DevBuf<double> dg;
  OB_TRY(h.up(t, lay, Theta, q, mean_tab, cov_tab, q * 2 * pl.n_pairs, wsb));
  if (G) OB_TRY(dg.alloc(q * pl.n_G));
  OB_TRY(obhip_sobol2_dev(t, h.th.p, q, h.mean.p, h.cov.p, h.out.p, dg.p, h.ws.p, wsb));
  OB_TRY(h.down(out));
  if (G) OB_TRY(d2h(G, dg.p, q * pl.n_G * sizeof(double)));
  return 0;
}

int obhip_shapley(const obhip_terms *t, const int32_t *groups, const double *Theta, uint64_t q, const double *mean_tab,
                  const double *cov_tab, double *out) {
  if (!t || !Theta || !mean_tab || !cov_tab || !out)
    return fail(OBHIP_ERR_INVALID, "shapley: null terms, Theta, tables or out");
  OB_TRY(check_q("shapley", q));
  Layout lay;
  OB_TRY(sobol_layout("shapley", *t, lay));
  ShapPlan plan;
  OB_TRY(shapley_plan("shapley", *t, groups, plan));
  uint64_t wsb = 0;
  OB_TRY(obhip_shapley_workspace_bytes(t->p, t->d, q, &wsb));
  OB_TRY(require_device());
  HostSums h;
  OB_TRY(h.up(t, lay, Theta, q, mean_tab, cov_tab, q * (uint64_t)plan.nplayers, wsb));
  OB_TRY(obhip_shapley_dev(t, groups, h.th.p, q, h.mean.p, h.cov.p, h.out.p, h.ws.p, wsb));
  return h.down(out);
}

// ---- active subspaces and derivative-based sensitivity ---------------------------------
int obhip_active_layout(const obhip_terms *t, uint64_t *n_mean, uint64_t *n_cov, uint64_t *n_out) {
  if (!t) return fail(OBHIP_ERR_INVALID, "active_layout: null terms");
  Layout lay;
  OB_TRY(active_layout("active_layout", *t, lay));
  if (n_mean) *n_mean = lay.n_mean;
  if (n_cov) *n_cov = lay.n_cov;
  if (n_out) *n_out = t->d + t->d * (t->d + 1) / 2;
  return 0;
}

int obhip_dim_grad_moments_dev(const obhip_model *m, const obhip_terms *t, const double *d_nodes, uint64_t n,
                               uint64_t ldx, const double *d_weights, uint64_t ldw, double *d_dmean, double *d_cross,
                               double *d_dd) {
  if (!m || !t || !d_nodes || !d_dmean || !d_cross || !d_dd)
    return fail(OBHIP_ERR_INVALID, "dim_grad_moments_dev: null model, terms, nodes, dmean, cross or dd");
  OB_TRY(check_nodes("dim_grad_moments_dev", n, ldx, d_weights != nullptr, ldw));
  OB_TRY(check_compat(m, t));
  Layout lay;
  OB_TRY(active_layout("dim_grad_moments_dev", *t, lay));
  OB_TRY(require_device());
  int flag = 0;
  OB_TRY(launch_dim_grad_moments(*m, *const_cast<obhip_terms *>(t), d_nodes, n, ldx, d_weights, ldw, d_dmean, d_cross,
                                 d_dd, &flag));
  if (flag)
    return fail(OBHIP_ERR_NUMERIC, "dim_grad_moments_dev: a weight is negative or not finite, or the weights of a "
                                   "dimension do not sum to > 0");
  return 0;
}

int obhip_active_workspace_bytes(uint64_t p, uint64_t d, uint64_t q, uint64_t *bytes) {
  OB_TRY(check_ws_args("active_workspace_bytes", p, d, q, bytes));
  *bytes = PairWs::bytes(p, d, pair_part_doubles(p, d, q, kActiveT, kActiveRC, kSobolTW));
  return 0;
}

int obhip_active_dev(const obhip_terms *t, const double *d_Theta, uint64_t q, const double *d_mean_tab,
                     const double *d_cov_tab, const double *d_dmean, const double *d_cross, const double *d_dd,
                     double *d_out, void *d_ws, uint64_t ws_bytes) {
  if (!t || !d_Theta || !d_mean_tab || !d_cov_tab || !d_dmean || !d_cross || !d_dd || !d_out || !d_ws)
    return fail(OBHIP_ERR_INVALID, "active_dev: null terms, Theta, tables, out or workspace");
  OB_TRY(check_q("active_dev", q));
  Layout lay;
  OB_TRY(active_layout("active_dev", *t, lay));
  uint64_t need = 0;
  OB_TRY(obhip_active_workspace_bytes(t->p, t->d, q, &need));
  if (ws_bytes < need)
    return fail(OBHIP_ERR_INVALID, "active_dev: workspace smaller than obhip_active_workspace_bytes");
  OB_TRY(require_device());
  obhip_terms &tt = *const_cast<obhip_terms *>(t);
  OB_TRY(ensure_sobol_tables(tt));
  const uint64_t p = t->p, d = t->d;
  const PairWs ws(d_ws, p, d);
  return launch_active(tt.sobol_lev.p, tt.sobol_meta.p, p, d, q, lay.n_cov, d_Theta, d_mean_tab, d_cov_tab, d_dmean,
                       d_cross, d_dd, ws.excl, ws.u, ws.part, d_out);
}

int obhip_dim_grad_moments(const obhip_model *m, const obhip_terms *t, const double *nodes, uint64_t n, uint64_t ldx,
                           const double *weights, uint64_t ldw, double *dmean, double *cross, double *dd) {
  if (!m || !t || !nodes || !dmean || !cross || !dd)
    return fail(OBHIP_ERR_INVALID, "dim_grad_moments: null model, terms, nodes, dmean, cross or dd");
  OB_TRY(check_nodes("dim_grad_moments", n, ldx, weights != nullptr, ldw));
  OB_TRY(check_compat(m, t));
  Layout lay;
  OB_TRY(active_layout("dim_grad_moments", *t, lay));
  OB_TRY(require_device());
  DevBuf<double> dx, dw, dm, dc, dv;
  OB_TRY(upload_cols(dx, nodes, n, m->d, ldx));
  if (weights) OB_TRY(upload_cols(dw, weights, n, m->d, ldw));
  OB_TRY(dm.alloc(lay.n_mean));
  OB_TRY(dc.alloc(lay.n_cov));
  OB_TRY(dv.alloc(lay.n_cov));
  OB_TRY(obhip_dim_grad_moments_dev(m, t, dx.p, n, n, dw.p, n, dm.p, dc.p, dv.p));
  OB_TRY(d2h(dmean, dm.p, lay.n_mean * sizeof(double)));
  OB_TRY(d2h(cross, dc.p, lay.n_cov * sizeof(double)));
  return d2h(dd, dv.p, lay.n_cov * sizeof(double));
}

int obhip_active(const obhip_terms *t, const double *Theta, uint64_t q, const double *mean_tab, const double *cov_tab,
                 const double *dmean, const double *cross, const double *dd, double *out) {
  if (!t || !Theta || !mean_tab || !cov_tab || !dmean || !cross || !dd || !out)
    return fail(OBHIP_ERR_INVALID, "active: null terms, Theta, tables or out");
  OB_TRY(check_q("active", q));
  Layout lay;
  OB_TRY(active_layout("active", *t, lay));
  uint64_t wsb = 0;
  OB_TRY(obhip_active_workspace_bytes(t->p, t->d, q, &wsb));
  OB_TRY(require_device());
  const uint64_t nout = t->d + t->d * (t->d + 1) / 2;
  HostSums h;
  DevBuf<double> ddm, dx, dv;
  OB_TRY(h.up(t, lay, Theta, q, mean_tab, cov_tab, q * nout, wsb));
  OB_TRY(ddm.upload(dmean, lay.n_mean));
  OB_TRY(dx.upload(cross, lay.n_cov));
  OB_TRY(dv.upload(dd, lay.n_cov));
  OB_TRY(obhip_active_dev(t, h.th.p, q, h.mean.p, h.cov.p, ddm.p, dx.p, dv.p, h.out.p, h.ws.p, wsb));
  return h.down(out);
}

int obhip_sym_eigh(uint64_t n, const double *A, double *w, double *V) {
  if (n == 0 || !A || !w || !V) return fail(OBHIP_ERR_INVALID, "sym_eigh: n = 0, or null A, w or V");
  if (n > 4096) return fail(OBHIP_ERR_INVALID, "sym_eigh: more than 4096 rows");
  for (uint64_t i = 0; i < n * n; ++i)
    if (!std::isfinite(A[i])) return fail(OBHIP_ERR_NUMERIC, "sym_eigh: an entry of A is not finite");
  const int N = (int)n;
  std::vector<double> a(n * n), ev, vec;
  for (uint64_t i = 0; i < n; ++i)                       // the upper triangle, mirrored
    for (uint64_t j = i; j < n; ++j) a[i * n + j] = a[j * n + i] = A[j * n + i];
  jacobi_eigh(N, a, ev, vec);                            // ascending; vector j at vec[j n ..]
  for (uint64_t j = 0; j < n; ++j) {
    const double *v = &vec[(n - 1 - j) * n];
    uint64_t big = 0;
    for (uint64_t i = 1; i < n; ++i)
      if (std::fabs(v[i]) > std::fabs(v[big])) big = i;  // (the lowest index wins a tie)
    const double sg = v[big] < 0.0 ? -1.0 : 1.0;
    w[j] = ev[n - 1 - j];
    for (uint64_t i = 0; i < n; ++i) V[j * n + i] = sg * v[i];
  }
  return 0;
}

}  // extern "C"
