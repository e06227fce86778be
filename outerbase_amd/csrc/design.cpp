// Sequential design: greedy max-variance and integrated-variance picks over a candidate set, on the
// device (include/obhip.h, "sequential design").  No reference counterpart: the
// reference package has no design criteria.
//
// The model is linear in its coefficients, so a run at row j takes H to H + b_j b_j^T / nu whatever the
// run returns, and S = inv(H) to S - s s^T / gamma.  The m-sized work of a step is ONE pass over the
// candidates (kernels_design.hip): a = B_c s and c = B_c h are formed tile by tile and used where they are
// formed.  Everything else is p-sized and stays in p-space, on explicit S and T = S M S.
//
//   set-up   d_i = || L^-1 b_i ||^2 as post_var_dev forms it, but from the stored product B X and a sum per
//            row (row_forms_dev says why); S = a copy of the handle's X X^T (posterior_inverse); for IMSE M from the
//            Gram kernels on the reference rows scaled by sqrt(u / sum u) (the row scale is where the GLM fit
//            puts sqrt(w)), T = S M S by launch_atb, num_i = b_i^T T b_i by launch_atb in store mode on the
//            term-major candidate chunk and a dot per row, tr(M S) by a fixed-order sum.
//   step t   pass (downdate of pick t - 1, scores, per-workgroup argmax), pick, ONE host wait for the
//            "nothing left" flag, then b_j by the one-row basis and launch_getmat and the p-space kernels.
//   end      one more pass applies the last pick's downdate.
// The working set of the steps and their loop are GreedyPicks, which the acquisition entry runs as well.
// Fused pass: k_design_step.  Term sets beyond design_step_supports (and OBHIP_FORCE_GENERIC): the
// predictor writes a and c to pooled scratch and k_design_update does the same epilogue from HBM.
#include <cmath>
#include <cstring>

#include "obhip_internal.h"
#include "row_chunks.h"
#include "vec_ops.h"

using namespace obhip;

namespace {

// d_M (p x p) = sum_r u_r b_r b_r^T / sum u over the rows of d_xref
int reference_moment(const obhip_model &m, obhip_terms &t, const double *d_xref, uint64_t r, const double *d_u,
                     double *d_M) {
  double total = (double)r;
  if (d_u) {
    DevBuf<double> sums, part;
    OB_TRY(sums.alloc(2));
    OB_TRY(part.alloc(2 * kSumBlocks));
    OB_TRY(vsum<2>(
        r,
        [=] __device__(uint64_t i, double *acc) {
          const double u = d_u[i];
          acc[0] += u;
          acc[1] += (u >= 0.0 && isfinite(u)) ? 0.0 : 1.0;
        },
        sums.p, part.p));
    double h[2];
    OB_TRY(d2h(h, sums.p, sizeof(h)));
    if (h[1] != 0.0 || !(h[0] > 0.0) || !std::isfinite(h[0]))
      return fail(OBHIP_ERR_NUMERIC, "design_select: the reference weights must be finite, >= 0 and have mass");
    total = h[0];
  }
  BasisGuard g;
  OB_TRY(obhip_basis_create_dev(&g.b, &m, d_xref, r, t.maxlev.data()));
  double *scale = g.b->scale.p;
  OB_TRY(vmap(r, [=] __device__(uint64_t i) { scale[i] *= sqrt((d_u ? d_u[i] : 1.0) / total); }));
  return launch_gram(*g.b, t, d_M);
}

}  // namespace

namespace obhip {
// d_out[i] = b_i^T Q b_i at the n rows of d_x, Q symmetric (norms false: Y = Q B^T, then b_i . y_i), or
// || X^T b_i ||^2 for the upper triangular X = L^-T (norms true: Z = B X, then the squares of row i).  Either
// way a stored product of launch_atb and one thread per row that sums its p entries in ascending order: two
// bit-identical rows get bit-identical results wherever they stand, which the tie rule of the selection rests
// on.  (post_var_dev's fused row norms are the same mathematics but sum a row's columns in an order that
// depends on the row's place in its tile; they stay what obhip_posterior_var_dev returns.)  That holds for rows
// whose 128-row tiles have the same index mod 8 only: launch_atb's stored product starts a tile's chunks of k
// at (I + J) mod 8.  fixed_order (the acquisition entry) takes the product that does not; the selection keeps
// the bits it has always returned.
int row_forms_dev(const obhip_model &m, obhip_terms &t, const double *d_Q, bool norms, uint64_t p, uint64_t pp,
                  const double *d_x, uint64_t n, double *d_out, bool fixed_order) {
  // row chunks so that the two blocks (pp x rows doubles each) stay below 1 GB each
  const int mode = fixed_order ? kAtbStoreFixed : kAtbStore;
  DevBuf<double> Ycm;
  return for_row_chunks(m, t, d_x, n, chunk_rows_for(pp, 1ull << 30), pp,
                        [&](uint64_t r0, uint64_t nr, uint64_t npad, const double *B) -> int {
    OB_TRY(Ycm.alloc(pp * npad));
    const double *Y = Ycm.p;
    double *out = d_out + r0;
    if (norms) {
      OB_TRY(launch_atb(mode, B, npad, npad, d_Q, pp, pp, pp, true, Ycm.p, pp));  // Z = B X, npad x pp
      return vmap(nr, [=] __device__(uint64_t i) {
        double s = 0.0;
        for (uint64_t k = 0; k < p; ++k) s = fma(Y[i * pp + k], Y[i * pp + k], s);
        out[i] = s;
      });
    }
    OB_TRY(launch_atb(mode, d_Q, pp, pp, B, npad, npad, pp, false, Ycm.p, npad));  // Y = Q B^T, pp x npad
    return vmap(nr, [=] __device__(uint64_t i) {
      double s = 0.0;
      for (uint64_t k = 0; k < p; ++k) s = fma(B[k * npad + i], Y[k * npad + i], s);
      out[i] = s;
    });
  });
}

int GreedyPicks::init(const obhip_posterior &post, const double *d_xcand, uint64_t m, uint64_t k, uint64_t nscal,
                      uint64_t nparts) {
  const obhip_model &om = *post.model;
  terms = const_cast<obhip_terms *>(post.terms);
  p = post.p, pp = post.f.pp, d = om.d;
  OB_TRY(picked.alloc(m));
  OB_TRY(S.alloc(pp * pp));
  OB_TRY(vec.alloc(2 * p));
  OB_TRY(sh.alloc(p * 16));
  OB_TRY(scal.alloc(nscal));
  OB_TRY(trace.alloc(k + 1));
  OB_TRY(bj.alloc(p));
  OB_TRY(xj0.alloc(d));
  OB_TRY(pscore.alloc(nparts));
  OB_TRY(pidx.alloc(nparts));
  hipStream_t st = cur_stream();
  OB_HIP(hipMemsetAsync(picked.p, 0, m, st));
  OB_HIP(hipMemsetAsync(vec.p, 0, 2 * p * sizeof(double), st));
  OB_HIP(hipMemsetAsync(sh.p, 0, p * 16 * sizeof(double), st));
  OB_HIP(hipMemsetAsync(trace.p, 0, (k + 1) * sizeof(double), st));
  const double *Sinv = nullptr;  // read-only: the picks downdate the copy
  OB_TRY(posterior_inverse(post, &Sinv));
  OB_HIP(hipMemcpyAsync(S.p, Sinv, pp * pp * sizeof(double), hipMemcpyDeviceToDevice, st));
  scal0.assign(nscal, 0.0);
  scal0[0] = 1.0;
  scal0[3] = std::exp(2.0 * post.sigma);
  // the one-row basis b_j is evaluated with: its x is where the pick kernel gathers the picked row
  OB_HIP(hipMemcpy2DAsync(xj0.p, sizeof(double), d_xcand, m * sizeof(double), sizeof(double), d,
                          hipMemcpyDeviceToDevice, st));
  return obhip_basis_create_dev(&one.b, &om, xj0.p, 1, terms->maxlev.data());
}

int GreedyPicks::run(uint64_t k, int crit, double *d_T, const std::function<int(uint64_t)> &pass,
                     const std::function<int(uint64_t)> &pick, uint64_t *npicked) {
  OB_HIP(hipMemcpyAsync(scal.p, scal0.data(), scal0.size() * sizeof(double), hipMemcpyHostToDevice, cur_stream()));
  OB_HIP(hipStreamSynchronize(cur_stream()));  // (scal0 may go away with the caller)
  uint64_t np = 0;
  bool left = true;
  for (uint64_t step = 0; step < k; ++step) {
    OB_TRY(pass(step));
    OB_TRY(pick(step));
    double none = 0.0;
    OB_TRY(d2h(&none, scal.p + 5, sizeof(double)));  // the step's one host wait: is anything left?
    if (none != 0.0) {
      left = false;
      break;
    }
    ++np;
    OB_TRY(launch_build_basis(*one.b));
    OB_TRY(launch_getmat(*one.b, *terms, bj.p, 1));
    OB_TRY(launch_design_pspace(crit, p, pp, bj.p, S.p, d_T, vec.p, vec.p + p, sh.p, scal.p, trace.p, step));
  }
  if (left) OB_TRY(pass(np));  // the last pick's downdate
  *npicked = np;
  return 0;
}
}  // namespace obhip

namespace {

int check_select(const char *who, const obhip_posterior *post, const void *xcand, uint64_t m, int criterion,
                 const void *xref, uint64_t r, uint64_t k, const void *index, const void *score,
                 const uint64_t *n_picked) {
  const std::string w(who);
  // what does not need the handle first: these are refused whatever the handle is
  if (m == 0 || k == 0) return fail(OBHIP_ERR_INVALID, w + ": no candidates or k = 0");
  if (criterion != OBHIP_DESIGN_MAXVAR && criterion != OBHIP_DESIGN_IMSE)
    return fail(OBHIP_ERR_INVALID, w + ": criterion must be OBHIP_DESIGN_MAXVAR or OBHIP_DESIGN_IMSE");
  if (criterion == OBHIP_DESIGN_IMSE && (!xref || r == 0))
    return fail(OBHIP_ERR_INVALID, w + ": the integrated variance needs reference rows");
  if (!xcand || !index || !score || !n_picked) return fail(OBHIP_ERR_INVALID, w + ": null candidates or outputs");
  return check_post_handle(w, post, true);
}

}  // namespace

extern "C" int obhip_design_select_dev(const obhip_posterior *post, const double *d_xcand, uint64_t m, int criterion,
                                       const double *d_xref, uint64_t r, const double *d_uref,
                                       const double *d_weights, uint64_t k, int replace, int64_t *d_index,
                                       double *d_score, double *d_var, double *d_trace, uint64_t *n_picked) {
  OB_TRY(check_select("design_select_dev", post, d_xcand, m, criterion, d_xref, r, k, d_index, d_score, n_picked));
  OB_TRY(require_device());
  const obhip_model &om = *post->model;
  obhip_terms &t = *const_cast<obhip_terms *>(post->terms);
  const uint64_t p = post->p, pp = post->f.pp, d = om.d;
  const bool imse = criterion == OBHIP_DESIGN_IMSE;
  OB_TRY(prepare_predict(om, t, false));
  const bool fused = design_step_supports(t);
  const uint64_t nparts = design_step_parts(m, fused);

  GreedyPicks g;
  DevBuf<double> dvar, num, T, ac;
  OB_TRY(dvar.alloc(m));
  OB_TRY(g.init(*post, d_xcand, m, k, kDesignScal, nparts));
  hipStream_t st = cur_stream();
  if (!fused) {
    OB_TRY(ac.alloc(2 * m));
    OB_HIP(hipMemsetAsync(ac.p, 0, 2 * m * sizeof(double), st));
  }
  // d_i = || L^-1 b_i ||^2
  OB_TRY(row_forms_dev(om, t, post->f.X.p, true, p, pp, d_xcand, m, dvar.p));
  if (imse) {
    DevBuf<double> M, Mp, W, part;
    OB_TRY(M.alloc(p * p));
    OB_TRY(Mp.alloc(pp * pp));
    OB_TRY(W.alloc(pp * pp));
    OB_TRY(T.alloc(pp * pp));
    OB_TRY(num.alloc(m));
    OB_TRY(part.alloc(kSumBlocks));
    OB_TRY(reference_moment(om, t, d_xref, r, d_uref, M.p));
    const double *Mc = M.p, *Sc = g.S.p;
    double *Mpp = Mp.p;
    OB_TRY(vmap(pp * pp, [=] __device__(uint64_t i) {
      const uint64_t a = i / pp, b = i % pp;
      Mpp[i] = (a < p && b < p) ? Mc[a * p + b] : 0.0;
    }));
    OB_TRY(launch_atb(kAtbStore, Mp.p, pp, pp, g.S.p, pp, pp, pp, false, W.p, pp));  // M S
    OB_TRY(launch_atb(kAtbStore, W.p, pp, pp, g.S.p, pp, pp, pp, false, T.p, pp));   // (M S)^T S = S M S
    OB_TRY(row_forms_dev(om, t, T.p, false, p, pp, d_xcand, m, num.p));
    // tr(M S_0) = sum_kl M_kl S_kl
    OB_TRY(vsum<1>(pp * pp, [=] __device__(uint64_t i, double *acc) { acc[0] += Mpp[i] * Sc[i]; }, g.trace.p, part.p));
    OB_HIP(hipStreamSynchronize(st));  // M, Mp, W and part are locals
  }

  DesignStep s;
  s.crit = criterion;
  s.replace = replace != 0;
  s.n = m;
  s.x = d_xcand;
  s.w = d_weights;
  s.sh = g.sh.p;
  s.scal = g.scal.p;
  s.dvar = dvar.p;
  s.num = num.p;
  s.picked = g.picked.p;
  s.part_score = g.pscore.p;
  s.part_idx = g.pidx.p;
  auto pass = [&](uint64_t) -> int {
    if (fused) return launch_design_step(om, t, s);
    if (imse && predict_multi_supports(t)) {
      OB_TRY(launch_predict_multi(om, t, g.vec.p, 2, d_xcand, m, ac.p));
    } else {
      for (uint64_t j = 0; j < (imse ? 2u : 1u); ++j)
        OB_TRY(launch_predict(om, t, g.vec.p + j * p, d_xcand, m, ac.p + j * m, nullptr, 0.0, nullptr));
    }
    return launch_design_update(s, ac.p);
  };
  auto pick = [&](uint64_t step) {
    return launch_design_pick(s, nparts, d, step, d_index, d_score, g.one.b->x.p, g.picked.p, g.scal.p);
  };
  uint64_t npicked = 0;
  OB_TRY(g.run(k, criterion, imse ? T.p : nullptr, pass, pick, &npicked));
  if (d_var) OB_HIP(hipMemcpyAsync(d_var, dvar.p, m * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (d_trace)
    OB_HIP(hipMemcpyAsync(d_trace, g.trace.p, (npicked + 1) * sizeof(double), hipMemcpyDeviceToDevice, st));
  OB_HIP(hipStreamSynchronize(st));
  *n_picked = npicked;
  return 0;
}

extern "C" int obhip_design_select(const obhip_posterior *post, const double *xcand, uint64_t m, int criterion,
                                   const double *xref, uint64_t r, const double *uref, const double *weights,
                                   uint64_t k, int replace, int64_t *index, double *score, double *var, double *trace,
                                   uint64_t *n_picked) {
  OB_TRY(check_select("design_select", post, xcand, m, criterion, xref, r, k, index, score, n_picked));
  OB_TRY(require_device());
  const uint64_t d = post->model->d;
  const bool imse = criterion == OBHIP_DESIGN_IMSE;
  DevBuf<double> dx, dr, du, dw, dscore, dvar, dtrace;
  DevBuf<int64_t> dindex;
  OB_TRY(upload_cols(dx, xcand, m, d, m));
  if (imse) OB_TRY(upload_cols(dr, xref, r, d, r));
  if (imse && uref) OB_TRY(du.upload(uref, r));
  if (weights) OB_TRY(dw.upload(weights, m));
  OB_TRY(dindex.alloc(k));
  OB_TRY(dscore.alloc(k));
  OB_TRY(dvar.alloc(m));
  OB_TRY(dtrace.alloc(k + 1));
  uint64_t np = 0;
  OB_TRY(obhip_design_select_dev(post, dx.p, m, criterion, imse ? dr.p : nullptr, r, du.p, dw.p, k, replace, dindex.p,
                                 dscore.p, dvar.p, dtrace.p, &np));
  if (np) OB_TRY(d2h(index, dindex.p, np * sizeof(int64_t)));
  if (np) OB_TRY(d2h(score, dscore.p, np * sizeof(double)));
  if (var) OB_TRY(d2h(var, dvar.p, m * sizeof(double)));
  if (trace) OB_TRY(d2h(trace, dtrace.p, (np + 1) * sizeof(double)));
  *n_picked = np;
  return 0;
}
