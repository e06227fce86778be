// Acquisition picks over several responses: constrained expected improvement and probability of improvement, the
// probability of feasibility and the two-objective expected hypervolume improvement over a candidate set, in batches
// of k by fantasies, on the device (include/obhip.h, "acquisition over several responses").
// No reference counterpart.
//
// acquire.cpp's frame with q means per candidate: the responses share H, so d_i, s = S b_j, gamma and a_i = b_i^T s
// are formed once per pick whatever q is.
//   set-up   d_i as acquire.cpp forms it (row_forms_dev in its fixed order), the q means by the multi-response
//            predictor (q = 1: the one-response predictor, acquire.cpp's bits), the eligibility map, the caller's
//            front normalised on the host (acquire_front.h) into the state block.
//   step t   the predictor's pass on s, k_macq_update (the q + 1 downdates of pick t - 1 and the scores for pick t),
//            k_macq_pick, ONE host wait, then b_j and the design entry's p-space kernels (GreedyPicks::run).
//   end      one more predictor pass and update apply the last pick's downdate.
#include <cmath>
#include <vector>

#include "obhip_internal.h"
#include "acquire_front.h"

using namespace obhip;

namespace {

static_assert(kMacqC - kMacqU == (int)kMacqFrontCap + 1 && kMacqRole - kMacqLie == kMacqMaxQ, "the state block's layout");

struct MacqCall {
  int obj1 = -1, obj2 = -1;
  std::vector<double> state;  // kMacqState doubles, the front normalised
  uint64_t F = 0;
};

int check_macq(const char *who, const obhip_posterior *post, const void *Theta, uint64_t q, const void *xcand, uint64_t m,
               int criterion, const int32_t *roles, const double *signs, const double *limits, double xi,
               const double *front0, uint64_t F0, int lie, const double *lie_value, uint64_t k, const void *index,
               const void *score, const uint64_t *n_picked, MacqCall &c) {
  const std::string w(who);
  if (m == 0) return fail(OBHIP_ERR_INVALID, w + ": m = 0, no candidates");
  if (k == 0) return fail(OBHIP_ERR_INVALID, w + ": k = 0, no picks asked for");
  if (q < 1 || q > (uint64_t)kMacqMaxQ) return fail(OBHIP_ERR_INVALID, w + ": q must be 1 .. 16 responses");
  if (criterion < OBHIP_MACQ_CEI || criterion > OBHIP_MACQ_EHVI)
    return fail(OBHIP_ERR_INVALID, w + ": criterion must be one of OBHIP_MACQ_*");
  if (lie != OBHIP_LIE_BELIEVER && lie != OBHIP_LIE_CONSTANT)
    return fail(OBHIP_ERR_INVALID, w + ": lie must be OBHIP_LIE_BELIEVER or OBHIP_LIE_CONSTANT");
  if (!roles || !signs || !limits) return fail(OBHIP_ERR_INVALID, w + ": null roles / signs / limits");
  if (!std::isfinite(xi)) return fail(OBHIP_ERR_INVALID, w + ": xi must be finite");
  const bool ehvi = criterion == OBHIP_MACQ_EHVI;
  int nobj = 0, ncon = 0;
  for (uint64_t r = 0; r < q; ++r) {
    if (roles[r] < OBHIP_ROLE_OBJECTIVE || roles[r] > OBHIP_ROLE_NONE)
      return fail(OBHIP_ERR_INVALID, w + ": roles must be OBHIP_ROLE_OBJECTIVE, _CONSTRAINT or _NONE");
    if (roles[r] == OBHIP_ROLE_NONE) continue;
    if (signs[r] != 1.0 && signs[r] != -1.0) return fail(OBHIP_ERR_INVALID, w + ": signs must be +1 or -1");
    if (roles[r] == OBHIP_ROLE_CONSTRAINT) {
      ++ncon;
      if (!std::isfinite(limits[r])) return fail(OBHIP_ERR_INVALID, w + ": a constraint's limit must be finite");
      continue;
    }
    (nobj == 0 ? c.obj1 : c.obj2) = (int)r;
    ++nobj;
  }
  const int want = ehvi ? 2 : (criterion == OBHIP_MACQ_POF ? 0 : 1);
  if (nobj != want)
    return fail(OBHIP_ERR_INVALID, w + ": the criterion takes " + std::to_string(want) + " objectives, the roles name " +
                                       std::to_string(nobj));
  if (criterion == OBHIP_MACQ_POF && ncon == 0)
    return fail(OBHIP_ERR_INVALID, w + ": OBHIP_MACQ_POF needs at least one constraint");
  if (ehvi && !(std::isfinite(limits[c.obj1]) && std::isfinite(limits[c.obj2])))
    return fail(OBHIP_ERR_INVALID, w + ": the reference point must be finite");
  if (want == 1) {
    const double b = signs[c.obj1] * limits[c.obj1];
    if (!(std::isfinite(b) || b == INFINITY))
      return fail(OBHIP_ERR_INVALID, w + ": the incumbent must be finite or +inf in the signed sense (no feasible run yet)");
  }
  if (ehvi) {
    if (F0 && !front0) return fail(OBHIP_ERR_INVALID, w + ": null front0 with F0 > 0");
    if (F0 > kMacqFrontCap || k > kMacqFrontCap || F0 + k > kMacqFrontCap)
      return fail(OBHIP_ERR_INVALID, w + ": F0 + k must not exceed 2048 front points");
    for (uint64_t s = 0; s < 2 * F0; ++s)
      if (!std::isfinite(front0[s])) return fail(OBHIP_ERR_INVALID, w + ": the front's points must be finite");
  }
  if (lie == OBHIP_LIE_CONSTANT) {
    if (!lie_value) return fail(OBHIP_ERR_INVALID, w + ": null lie_value under OBHIP_LIE_CONSTANT");
    for (uint64_t r = 0; r < q; ++r)
      if (!std::isfinite(lie_value[r]))
        return fail(OBHIP_ERR_INVALID, w + ": lie_value must be finite under OBHIP_LIE_CONSTANT");
  }
  if (!xcand) return fail(OBHIP_ERR_INVALID, w + ": null candidates");
  if (!index || !score || !n_picked) return fail(OBHIP_ERR_INVALID, w + ": null outputs index / score / n_picked");
  if (!Theta) return fail(OBHIP_ERR_INVALID, w + ": d_Theta is null");
  OB_TRY(check_post_handle(w, post, true));

  c.state.assign(kMacqState, 0.0);
  for (uint64_t r = 0; r < q; ++r) {
    const bool used = roles[r] != OBHIP_ROLE_NONE;
    c.state[kMacqSign + r] = used ? signs[r] : 1.0;
    c.state[kMacqLimit + r] = used ? signs[r] * limits[r] : 0.0;
    c.state[kMacqLie + r] = lie == OBHIP_LIE_CONSTANT ? lie_value[r] : 0.0;
    c.state[kMacqRole + r] = (double)roles[r];
  }
  c.state[kMacqBest] = want == 1 ? c.state[kMacqLimit + c.obj1] : INFINITY;
  if (ehvi) {
    const double g1 = signs[c.obj1], g2 = signs[c.obj2];
    for (uint64_t s = 0; s < F0; ++s)
      c.F = front_insert(&c.state[kMacqU], &c.state[kMacqC], c.F, g1 * front0[2 * s], g2 * front0[2 * s + 1],
                         c.state[kMacqLimit + c.obj1], c.state[kMacqLimit + c.obj2]);
    c.state[kMacqF] = (double)c.F;
  }
  return 0;
}

}  // namespace

extern "C" int obhip_acquire_multi_layout(uint64_t q, int criterion, uint64_t front_cap, uint64_t *lds_bytes,
                                          uint64_t *max_q, uint64_t *max_front) {
  if (q < 1 || q > (uint64_t)kMacqMaxQ) return fail(OBHIP_ERR_INVALID, "acquire_multi_layout: q must be 1 .. 16 responses");
  if (criterion < OBHIP_MACQ_CEI || criterion > OBHIP_MACQ_EHVI)
    return fail(OBHIP_ERR_INVALID, "acquire_multi_layout: criterion must be one of OBHIP_MACQ_*");
  if (front_cap > kMacqFrontCap)
    return fail(OBHIP_ERR_INVALID, "acquire_multi_layout: F0 + k must not exceed 2048 front points");
  if (lds_bytes) *lds_bytes = macq_update_lds_bytes(criterion, front_cap);
  if (max_q) *max_q = kMacqMaxQ;
  if (max_front) *max_front = kMacqFrontCap;
  return 0;
}

extern "C" int obhip_acquire_multi_dev(const obhip_posterior *post, const double *d_Theta, uint64_t q,
                                       const double *d_xcand, uint64_t m, int criterion, const int32_t *roles,
                                       const double *signs, const double *limits, double xi, const double *front0,
                                       uint64_t F0, int lie, const double *lie_value, const uint8_t *d_skip, uint64_t k,
                                       int64_t *d_index, double *d_score, double *d_score0, double *d_pof0,
                                       double *d_mean, double *d_var, double *front_out, uint64_t *n_front,
                                       double *best_out, uint64_t *n_picked) {
  MacqCall c;
  OB_TRY(check_macq("acquire_multi_dev", post, d_Theta, q, d_xcand, m, criterion, roles, signs, limits, xi, front0, F0,
                    lie, lie_value, k, d_index, d_score, n_picked, c));
  OB_TRY(require_device());
  const obhip_model &om = *post->model;
  obhip_terms &t = *const_cast<obhip_terms *>(post->terms);
  const uint64_t p = post->p, pp = post->f.pp, d = om.d;
  OB_TRY(prepare_predict(om, t, false));

  GreedyPicks g;
  DevBuf<double> mu, dvar, a, mst;
  DevBuf<uint8_t> elig;
  OB_TRY(mu.alloc(m * q));
  OB_TRY(dvar.alloc(m));
  OB_TRY(a.alloc(m));
  OB_TRY(elig.alloc(m));
  OB_TRY(mst.upload(c.state.data(), c.state.size()));
  OB_TRY(g.init(*post, d_xcand, m, k, kDesignScal, (m + kAcqRows - 1) / kAcqRows));
  hipStream_t st = cur_stream();
  OB_HIP(hipMemsetAsync(a.p, 0, m * sizeof(double), st));  // a = 0 and delta = 0: the first pass downdates nothing
  OB_TRY(launch_sample_elig(d_xcand, m, d, d_skip, elig.p));
  // d_i = || L^-1 b_i ||^2, mu_ir = b_i^T theta_r
  OB_TRY(row_forms_dev(om, t, post->f.X.p, true, p, pp, d_xcand, m, dvar.p, true));
  if (q > 1 && predict_multi_supports(t)) {
    OB_TRY(launch_predict_multi(om, t, d_Theta, q, d_xcand, m, mu.p));
  } else {
    for (uint64_t r = 0; r < q; ++r)
      OB_TRY(launch_predict(om, t, d_Theta + r * p, d_xcand, m, mu.p + r * m, nullptr, 0.0, nullptr));
  }

  MacqStep s;
  s.crit = criterion;
  s.lie = lie;
  s.q = (int)q;
  s.obj1 = c.obj1;
  s.obj2 = c.obj2;
  s.n = m;
  s.front_cap = criterion == OBHIP_MACQ_EHVI ? c.F + k : 0;
  s.xi = xi;
  s.x = d_xcand;
  s.a = a.p;
  s.elig = elig.p;
  s.picked = g.picked.p;
  s.mean = mu.p;
  s.dvar = dvar.p;
  s.scal = g.scal.p;
  s.mst = mst.p;
  s.part_score = g.pscore.p;
  s.part_idx = g.pidx.p;
  auto pass = [&](uint64_t step) -> int {
    if (step) OB_TRY(launch_predict(om, t, g.vec.p, d_xcand, m, a.p, nullptr, 0.0, nullptr));
    return launch_macq_update(s, step == 0 ? d_score0 : nullptr, step == 0 ? d_pof0 : nullptr);
  };
  auto pick = [&](uint64_t step) { return launch_macq_pick(s, d, step, d_index, d_score, g.one.b->x.p); };
  uint64_t npicked = 0;
  OB_TRY(g.run(k, OBHIP_DESIGN_MAXVAR, nullptr, pass, pick, &npicked));
  if (d_mean) OB_HIP(hipMemcpyAsync(d_mean, mu.p, m * q * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (d_var) OB_HIP(hipMemcpyAsync(d_var, dvar.p, m * sizeof(double), hipMemcpyDeviceToDevice, st));
  OB_TRY(d2h(c.state.data(), mst.p, c.state.size() * sizeof(double)));  // (waits for the stream)
  OB_HIP(hipStreamSynchronize(st));
  if (criterion == OBHIP_MACQ_EHVI) {
    const uint64_t F = (uint64_t)c.state[kMacqF];
    if (front_out)
      for (uint64_t i = 0; i < F; ++i) {
        front_out[2 * i] = signs[c.obj1] * c.state[kMacqU + i];
        front_out[2 * i + 1] = signs[c.obj2] * c.state[kMacqC + i];
      }
    if (n_front) *n_front = F;
  } else if (n_front) {
    *n_front = 0;
  }
  if (best_out && c.obj1 >= 0 && criterion != OBHIP_MACQ_EHVI) *best_out = signs[c.obj1] * c.state[kMacqBest];
  *n_picked = npicked;
  return 0;
}

extern "C" int obhip_acquire_multi(const obhip_posterior *post, const double *Theta, uint64_t q, const double *xcand,
                                   uint64_t m, int criterion, const int32_t *roles, const double *signs,
                                   const double *limits, double xi, const double *front0, uint64_t F0, int lie,
                                   const double *lie_value, const uint8_t *skip, uint64_t k, int64_t *index,
                                   double *score, double *score0, double *pof0, double *mean, double *var,
                                   double *front_out, uint64_t *n_front, double *best_out, uint64_t *n_picked) {
  MacqCall c;
  OB_TRY(check_macq("acquire_multi", post, Theta, q, xcand, m, criterion, roles, signs, limits, xi, front0, F0, lie,
                    lie_value, k, index, score, n_picked, c));
  OB_TRY(require_device());
  const uint64_t d = post->model->d;
  DevBuf<double> dth, dx, dscore, dscore0, dpof0, dmean, dvar;
  DevBuf<int64_t> dindex;
  DevBuf<uint8_t> dskip;
  OB_TRY(dth.upload(Theta, post->p * q));
  OB_TRY(upload_cols(dx, xcand, m, d, m));
  if (skip) OB_TRY(dskip.upload(skip, m));
  OB_TRY(dindex.alloc(k));
  OB_TRY(dscore.alloc(k));
  if (score0) OB_TRY(dscore0.alloc(m));
  if (pof0) OB_TRY(dpof0.alloc(m));
  if (mean) OB_TRY(dmean.alloc(m * q));
  if (var) OB_TRY(dvar.alloc(m));
  uint64_t np = 0;
  OB_TRY(obhip_acquire_multi_dev(post, dth.p, q, dx.p, m, criterion, roles, signs, limits, xi, front0, F0, lie, lie_value,
                                 dskip.p, k, dindex.p, dscore.p, dscore0.p, dpof0.p, dmean.p, dvar.p, front_out, n_front,
                                 best_out, &np));
  if (np) OB_TRY(d2h(index, dindex.p, np * sizeof(int64_t)));
  if (np) OB_TRY(d2h(score, dscore.p, np * sizeof(double)));
  if (score0) OB_TRY(d2h(score0, dscore0.p, m * sizeof(double)));
  if (pof0) OB_TRY(d2h(pof0, dpof0.p, m * sizeof(double)));
  if (mean) OB_TRY(d2h(mean, dmean.p, m * q * sizeof(double)));
  if (var) OB_TRY(d2h(var, dvar.p, m * sizeof(double)));
  *n_picked = np;
  return 0;
}
