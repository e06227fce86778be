// Hyper-parameter gradient products of the outer-product basis for gfx950:
//   getmat_gradhyp         getmge_                            src/linalg.cpp:778-822
//   matmul_gradhyp         prodmmge_ / domultgesub_           src/linalg.cpp:139-276
//   tmatmul_gradhyp        tprodmmge_ / dotmultgesub_         src/linalg.cpp:362-471
// The C entry points and the device-level forms of the likelihood classes (lpdf.cpp).  Below them:
// the gradient basis (kernels_grad_basis.hip), the term views and pass groups (grad_views.cpp), the
// dense pass (kernels_grad_dense.hip) and the fused pass k_tmm_d3 (kernels_grad_d3.hip).
//
// Who computes what:
//   getmat_gradhyp            getmat on the full view, one pass per hyper-parameter
//   matmul / sqmm _gradhyp    with M = sum_k a_k P_k (one k_mm pass over all terms) and
//                             delta[h, t] = ge[h, t] - basemat[col(dim h, t)] ge[h, 0]:
//                             out[:, h] = s (ge[h, 0] M + sum_{k: t_kl > 0} a_k E_k delta[h, t_kl]),
//                             so per hyper-parameter only the terms that HAVE its dimension are
//                             multiplied out (k_mm on the delta view): nnz(terms) products instead
//                             of p x nhyp
//   matmul_gradhyp_dot        w^T of that without the n x nhyp matrix (mm_gradhyp_dot_dev)
//   tmatmul / sqtmm _gradhyp  one of the four plans of GradPlan below: a dense pass that treats
//                             every term as if it lacked the hyper-parameter's dimension, and a
//                             pass over the terms that have it which adds to (k_tmm_d3) or
//                             overwrites (restricted views) their entries
//   both of a likelihood      grad_dual_dev: the fused plan only, one sweep and one copy
#include "obhip_internal.h"
#include "device_common.h"

using namespace obhip;

namespace {

// out_gradhyp[h][i] += ge[h, 0]_i * M_i  (M = B a or B^2 a, already scaled by basescale)
__global__ void k_ge0_combine(const double *__restrict__ bm, uint64_t Mtot,
                              const int *__restrict__ ge0col, const double *__restrict__ M,
                              uint64_t n, double *__restrict__ outge) {
  const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const int h = blockIdx.y;
  const double g0 = bm[((row >> 6) * Mtot + (uint64_t)ge0col[h]) * kTileRows + (row & 63)];
  outge[(uint64_t)h * n + row] = fma(g0, M[row], outge[(uint64_t)h * n + row]);
}

// part[h][blk] = partial sums of w_i G[h][i] over the rows blk, blk + gridDim.x, ...
__global__ void __launch_bounds__(256)
k_wdot1(const double *__restrict__ G, const double *__restrict__ w, uint64_t n,
        double *__restrict__ part) {
  __shared__ double red[256];
  const double *g = G + (uint64_t)blockIdx.y * n;
  double s = 0.0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
    s = fma(w[i], g[i], s);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}
__global__ void k_wdot2(const double *__restrict__ part, int nblk, double *__restrict__ out) {
  const int h = blockIdx.x;
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < nblk; ++i) s += part[(uint64_t)h * nblk + i];
  out[h] = s;
}

// part[h][blk] = partial sums of w_i M_i ge[h, 0]_i (the level-0 gradient column of hyper-parameter
// h in the tiled gradient basis)
__global__ void __launch_bounds__(256)
k_wdot_ge0(const double *__restrict__ bm, uint64_t Mtot, const int *__restrict__ ge0col,
           const double *__restrict__ M, const double *__restrict__ w, uint64_t n,
           double *__restrict__ part) {
  __shared__ double red[256];
  const uint64_t c = (uint64_t)ge0col[blockIdx.y];
  double s = 0.0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
    s = fma(w[i] * M[i], bm[((i >> 6) * Mtot + c) * kTileRows + (i & 63)], s);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

constexpr int kWdotBlocks = 256;  // partial sums per column of the k_wdot* kernels

// d_out[h] = sum_i w_i M_i ge[h, 0]_i, enqueued; dpart (partial sums): the caller keeps it until the stream has run
int launch_wdot_ge0(const obhip_basis &b, const double *d_M, const double *d_w, DevBuf<double> &dpart,
                    double *d_out) {
  const obhip_gradbasis &g = *b.grad;
  const obhip_basis &src = *g.gb;
  const uint64_t nh = b.model->nhyp();
  OB_TRY(dpart.alloc(nh * kWdotBlocks));
  hipLaunchKernelGGL(k_wdot_ge0, dim3(kWdotBlocks, (unsigned)nh), dim3(256), 0, cur_stream(), src.bm.p,
                     src.md.Mc, g.ge0col.p, d_M, d_w, b.n, dpart.p);
  hipLaunchKernelGGL(k_wdot2, dim3((unsigned)nh), dim3(64), 0, cur_stream(), dpart.p, kWdotBlocks, d_out);
  OB_HIP(hipGetLastError());
  return 0;
}

int check_grad_args(const obhip_basis *b, const obhip_terms *t) {
  if (!b || !t) return fail(OBHIP_ERR_INVALID, "gradhyp: null argument");
  if (t->d != b->model->d) return fail(OBHIP_ERR_INVALID, "terms and model disagree on d");
  for (uint64_t l = 0; l < t->d; ++l)
    if (t->maxlev[l] > b->md.cap[l])
      return fail(OBHIP_ERR_INVALID, "terms use a level above the basis' level cap");
  return 0;
}

// How the transposed products sum_i a_i dB_ik/dhyp_h of (b, t) are formed
enum class GradPlan {
  // k_tmm_ge0 + k_tmm_d3, which ADDS the delta part of the terms that have the dimension; both form
  // the squares themselves, so only this plan never reads the squared store.  The terms fit
  // k_tmm_ge0 (tmm_ge0_supports) and every view fits k_tmm_d3 (build_d3_groups).
  Fused,
  // k_tmm_ge0 + one k_tmm pass per group of restricted views, which OVERWRITES those terms' entries:
  // some view does not fit k_tmm_d3 (or OBHIP_GRAD_D3=0)
  Ge0Views,
  // k_bt_times_u on the materialised design matrix + the restricted views: the terms do not fit
  // k_tmm_ge0 (more than 8 factors) and there is room for the matrix (gram_panel_supports)
  BmatViews,
  // one k_tmm pass per hyper-parameter on the full views: neither dense pass takes the terms
  FullViews,
};
GradPlan grad_plan(obhip_basis &b, obhip_terms &t) {  // t prepared for b, b.grad built
  if (tmm_ge0_supports(t)) return build_d3_groups(t, b) ? GradPlan::Fused : GradPlan::Ge0Views;
  return gram_panel_supports(b, t) ? GradPlan::BmatViews : GradPlan::FullViews;
}

// ---- the k_tmm_d3 groups of a term set, their results group after group, each [2 nh][view-terms] ----
uint64_t d3_doubles(const obhip_terms &t) {
  uint64_t total = 0;
  for (const obhip_terms::GeD3 &grp : t.ge.d3) total += 2 * (uint64_t)grp.nh * grp.v->p;
  return total;
}
// every group enqueued, into d_out (d3_doubles); mode, d_w1, d_w2 as launch_tmm_d3
int enqueue_d3_groups(obhip_basis &b, obhip_terms &t, int mode, const double *d_w1, const double *d_w2,
                      double *d_out) {
  for (const obhip_terms::GeD3 &grp : t.ge.d3) {
    OB_TRY(launch_tmm_d3(b, grp, mode, d_w1, d_w2, d_out));
    d_out += 2 * (uint64_t)grp.nh * grp.v->p;
  }
  return 0;
}

// each(h, term indices, u1, u2) for every hyper-parameter h of every member, from the host copy of
// that layout (of u1 and u2 only what the mode computed holds anything)
template <typename F>
void each_d3_member(const obhip_terms &t, const double *res, F &&each) {
  for (const obhip_terms::GeD3 &grp : t.ge.d3) {
    const uint64_t vp = grp.v->p;
    for (size_t j = 0; j < grp.hyp0.size(); ++j)
      for (int hh = 0; hh < grp.nh; ++hh) {
        const uint64_t h = grp.hyp0[j] + hh;
        each(h, t.ge.sidx[h], res + hh * vp + grp.off[j], res + (grp.nh + hh) * vp + grp.off[j]);
      }
    res += 2 * (uint64_t)grp.nh * vp;
  }
}

// the three together: all groups enqueued, one blocking copy, then the members
template <typename F>
int run_d3_groups(obhip_basis &b, obhip_terms &t, int mode, const double *d_w1, const double *d_w2, F &&each) {
  std::vector<double> res(d3_doubles(t));
  if (res.empty()) return 0;
  DevBuf<double> dres;
  OB_TRY(dres.alloc(res.size()));
  OB_TRY(enqueue_d3_groups(b, t, mode, d_w1, d_w2, dres.p));
  OB_TRY(d2h(res.data(), dres.p, res.size() * sizeof(double)));
  each_d3_member(t, res.data(), each);
  return 0;
}

// ---- the groups of restricted views of a term set (delta: the delta views) -----------------------
// One k_tmm pass over src (b's gradient basis or its squared store) and one blocking copy per group -- per
// hyper-parameter where a group's columns exceed one LDS tile -- then each(h, term indices, values).
// (one pass for the group: its concatenated view prepares and its columns fit one LDS tile)
bool view_group_one_pass(obhip_terms &all, const obhip_basis &src) {
  return all.prepare(src.md.cap, src.md.dims_h) == 0 && all.Mu <= 296;
}
template <typename F>
int run_view_groups(const obhip_basis &src, obhip_terms &t, const obhip_basis &b, bool delta, const double *d_w,
                    F &&each) {
  DevBuf<double> dall;
  std::vector<double> tmp;
  auto pass = [&](obhip_terms &v) -> int {
    OB_TRY(dall.alloc(std::max<uint64_t>(v.p, dall.n)));
    OB_TRY(launch_tmm(src, v, d_w, dall.p, false));
    tmp.resize(v.p);
    return d2h(tmp.data(), dall.p, tmp.size() * sizeof(double));
  };
  for (obhip_terms::GeGroup &grp : grad_view_groups(t, b, delta)) {
    obhip_terms *all = grp.v.get();
    if (view_group_one_pass(*all, src)) {
      OB_TRY(pass(*all));
      for (size_t j = 0; j < grp.hyps.size(); ++j) each(grp.hyps[j], t.ge.sidx[grp.hyps[j]], tmp.data() + grp.off[j]);
      continue;
    }
    for (uint64_t h : grp.hyps) {
      const std::vector<uint32_t> *idx = nullptr;
      obhip_terms *v = grad_view_restricted(t, b, h, delta, &idx);
      if (!v) continue;
      OB_TRY(pass(*v));
      each(h, *idx, tmp.data());
    }
  }
  return 0;
}

// out_gradhyp (host, n x nhyp) = d(B a)/dhyp_h (squared: d(B^2 a)/dhyp_h); d_M receives
// B a (B^2 a).  One k_mm pass over all terms for M, per hyper-parameter one k_mm pass over
// the terms that have its dimension (delta view), then out[:, h] = ge[h, 0] M + that.
int mm_gradhyp_dev(obhip_basis &b, obhip_terms &t, bool squared, const double *a, const double *d_a,
                   double *d_M, DevBuf<double> &dge) {
  HostTimer ht("mm_gradhyp_dev");
  obhip_gradbasis &g = *b.grad;
  const obhip_basis &src = squared ? *g.gbsq : *g.gb;
  const uint64_t nh = b.model->nhyp(), n = b.n;
  DevBuf<double> dacat;
  OB_TRY(dge.alloc(n * nh));
  OB_HIP(hipMemsetAsync(dge.p, 0, n * nh * sizeof(double), cur_stream()));
  // coefficients of the restricted views, concatenated
  std::vector<double> acat;
  std::vector<uint64_t> off(nh + 1, 0);
  for (uint64_t h = 0; h < nh; ++h) {
    const std::vector<uint32_t> *idx = nullptr;
    grad_view_restricted(t, b, h, true, &idx);
    for (uint32_t k : *idx) acat.push_back(a[k]);
    off[h + 1] = acat.size();
  }
  if (!acat.empty()) OB_TRY(dacat.upload(acat.data(), acat.size()));
  OB_TRY(launch_mm(b, t, d_a, d_M, squared));
  {
    ProfScope ps(squared ? "sqmm_gradhyp" : "mm_gradhyp");
    for (uint64_t h = 0; h < nh; ++h) {
      const std::vector<uint32_t> *idx = nullptr;
      obhip_terms *v = grad_view_restricted(t, b, h, true, &idx);
      if (!v) continue;
      OB_TRY(launch_mm(src, *v, dacat.p + off[h], dge.p + h * n, false));
    }
    hipLaunchKernelGGL(k_ge0_combine, dim3((unsigned)((n + 255) / 256), (unsigned)nh), dim3(256), 0,
                       cur_stream(), src.bm.p, src.md.Mc, g.ge0col.p, d_M, n, dge.p);
    OB_HIP(hipGetLastError());
  }
  OB_HIP(hipStreamSynchronize(cur_stream()));  // dacat is a local
  return 0;
}

int mm_gradhyp_all(obhip_basis &b, obhip_terms &t, bool squared, const double *a, const double *d_a,
                   double *d_M, double *out_gradhyp) {
  DevBuf<double> dge;
  OB_TRY(mm_gradhyp_dev(b, t, squared, a, d_a, d_M, dge));
  return d2h(out_gradhyp, dge.p, b.n * b.model->nhyp() * sizeof(double));
}

// out_host[h] = w^T d(B a)/dhyp_h without the n x nhyp matrix.  d(B a)/dhyp_h = ge[h, 0] % (B a) +
// B_delta,h a_h (mm_gradhyp_dev), and the likelihoods only ever contract it with one row vector
// (loglik_gauss.cpp:127, loglik_std.cpp:143, loglik_gda.cpp:141: gradhyp = yhat_gradhyp^T r), so
//   out[h] = sum_i w_i ge[h, 0]_i M_i  +  a_h^T (B_delta,h^T w):
// one streaming pass for the level-0 columns and B^T passes whose accumulators stay in the lanes (no
// cross-lane sum per row, which is what the nhyp restricted k_mm passes of mm_gradhyp_dev pay).  d_M = B a.
int mm_gradhyp_dot_dev(obhip_basis &b, obhip_terms &t, const double *a, const double *d_M,
                       const double *d_w, double *out_host) {
  HostTimer ht("mm_gradhyp_dot_dev");
  const uint64_t nh = b.model->nhyp();
  if (nh == 0) return 0;
  DevBuf<double> dpart, dres;
  OB_TRY(dres.alloc(nh));
  ProfScope ps("mm_gradhyp_dot");
  OB_TRY(launch_wdot_ge0(b, d_M, d_w, dpart, dres.p));
  OB_TRY(d2h(out_host, dres.p, nh * sizeof(double)));
  auto contract = [&](uint64_t h, const std::vector<uint32_t> &ix, const double *v) {  // out[h] += a_h^T v
    long double s = 0;
    for (size_t q = 0; q < ix.size(); ++q) s += (long double)a[ix[q]] * v[q];
    out_host[h] += (double)s;
  };
  // There is no dense pass here, so less is asked than GradPlan::Fused asks: k_tmm_d3 wherever
  // build_d3_groups takes the terms, whether or not they fit k_tmm_ge0; else the groups of delta
  // views, as the restricted views of GradPlan::Ge0Views / BmatViews
  if (build_d3_groups(t, b))
    return run_d3_groups(b, t, 1, d_w, nullptr,
                         [&](uint64_t h, const std::vector<uint32_t> &ix, const double *u1, const double *) {
                           contract(h, ix, u1);
                         });
  return run_view_groups(*b.grad->gb, t, b, true, d_w, contract);
}

// out_gradhyp (host, p x nhyp) = sum_i a_i dB_ik/dhyp_h (squared: of B^2), by the plan of (b, t)
int tmm_gradhyp_all(obhip_basis &b, obhip_terms &t, bool squared, const double *d_a, double *out_gradhyp) {
  HostTimer ht("tmm_gradhyp_all");
  const uint64_t nh = b.model->nhyp(), p = t.p;
  DevBuf<double> dout;
  OB_TRY(dout.alloc(p * nh));
  OB_TRY(t.prepare(b.md.cap, b.md.dims_h));
  const GradPlan plan = grad_plan(b, t);
  // the squared store of the gradient basis (a second array of its size) only where it is read
  const bool sq_store = squared && plan != GradPlan::Fused;
  if (sq_store) OB_TRY(ensure_gradbasis_sq(b));
  const obhip_basis &src = sq_store ? *b.grad->gbsq : *b.grad->gb;
  if (plan == GradPlan::FullViews) {
    for (uint64_t h = 0; h < nh; ++h) {
      OB_TRY(launch_tmm(src, *grad_view(t, b, h), d_a, dout.p, false));
      OB_TRY(d2h(out_gradhyp + h * p, dout.p, p * sizeof(double)));
    }
    return 0;
  }
  if (plan == GradPlan::BmatViews)
    OB_TRY(launch_bt_times_ge0(b, t, squared, d_a, dout.p));
  else
    OB_TRY(launch_tmm_ge0(b, t, squared, d_a, dout.p));
  OB_TRY(d2h(out_gradhyp, dout.p, p * nh * sizeof(double)));
  if (plan == GradPlan::Fused)
    // the dense pass gave ge[h, 0] B (squared: 2 ge[h, 0] B^2) for EVERY term; the terms that have the
    // dimension add their delta part, squared: 2 u2
    return run_d3_groups(b, t, squared ? 2 : 1, d_a, d_a,
                         [&](uint64_t h, const std::vector<uint32_t> &ix, const double *u1, const double *u2) {
                           for (size_t q = 0; q < ix.size(); ++q)
                             out_gradhyp[h * p + ix[q]] += squared ? 2.0 * u2[q] : u1[q];
                         });
  return run_view_groups(src, t, b, false, d_a, [&](uint64_t h, const std::vector<uint32_t> &ix, const double *v) {
    for (size_t q = 0; q < ix.size(); ++q) out_gradhyp[h * p + ix[q]] = v[q];
  });
}

// products on the squared stores: ob$sqmm_gradhyp / ob$sqtmm_gradhyp
// (modandbase.cpp:798-809, 845-856)
// a == nullptr with transposed: the all-ones vector, filled on the device (sqcolsums_gradhyp)
int sq_gradhyp(const obhip_basis *bc, const obhip_terms *tc, const double *a, double *out_gradhyp,
               bool transposed) {
  OB_TRY(check_grad_args(bc, tc));
  if ((!a && !transposed) || !out_gradhyp)
    return fail(OBHIP_ERR_INVALID, "sq*_gradhyp: null argument");
  obhip_basis &b = *const_cast<obhip_basis *>(bc);
  obhip_terms &t = *const_cast<obhip_terms *>(tc);
  // (the transposed product asks for the squared store itself, where it needs it)
  OB_TRY(transposed ? ensure_gradbasis(b) : ensure_gradbasis_sq(b));
  const uint64_t nin = transposed ? b.n : t.p, nout = transposed ? t.p : b.n;
  DevBuf<double> da, dout;
  if (a) {
    OB_TRY(da.upload(a, nin));
  } else {
    OB_TRY(da.alloc(nin));
    OB_TRY(launch_fill(da.p, nin, 1.0));
  }
  OB_TRY(dout.alloc(nout));
  if (transposed) return tmm_gradhyp_all(b, t, true, da.p, out_gradhyp);
  return mm_gradhyp_all(b, t, true, a, da.p, dout.p, out_gradhyp);
}

}  // namespace

extern "C" {

int obhip_basis_getmat_gradhyp(const obhip_basis *bc, const obhip_terms *tc, double *out) {
  OB_TRY(check_grad_args(bc, tc));
  if (!out) return fail(OBHIP_ERR_INVALID, "getmat_gradhyp: null argument");
  obhip_basis &b = *const_cast<obhip_basis *>(bc);
  obhip_terms &t = *const_cast<obhip_terms *>(tc);
  OB_TRY(ensure_gradbasis(b));
  DevBuf<double> tmp;
  OB_TRY(tmp.alloc(b.n * t.p));
  for (uint64_t h = 0; h < b.model->nhyp(); ++h) {
    OB_TRY(launch_getmat(*b.grad->gb, *grad_view(t, b, h), tmp.p));
    OB_TRY(d2h(out + h * b.n * t.p, tmp.p, b.n * t.p * sizeof(double)));
  }
  return 0;
}

int obhip_basis_mm_gradhyp(const obhip_basis *bc, const obhip_terms *tc, const double *a,
                           double *out, double *out_gradhyp) {
  OB_TRY(check_grad_args(bc, tc));
  if (!a || !out_gradhyp) return fail(OBHIP_ERR_INVALID, "mm_gradhyp: null argument");
  obhip_basis &b = *const_cast<obhip_basis *>(bc);
  obhip_terms &t = *const_cast<obhip_terms *>(tc);
  OB_TRY(ensure_gradbasis(b));
  DevBuf<double> da, dout;
  OB_TRY(da.upload(a, t.p));
  OB_TRY(dout.alloc(b.n));
  OB_TRY(mm_gradhyp_all(b, t, false, a, da.p, dout.p, out_gradhyp));
  if (out) OB_TRY(d2h(out, dout.p, b.n * sizeof(double)));
  return 0;
}

// w^T d(B a)/dhyp without moving the n x nhyp matrix to the host: what the likelihoods need
// of matmul_gradhyp (loglik_gauss.cpp:127, loglik_std.cpp:143: gradhyp = r^T yhat_gradhyp)
int obhip_basis_mm_gradhyp_dot(const obhip_basis *bc, const obhip_terms *tc, const double *a,
                               const double *w, double *out, double *out_dot) {
  OB_TRY(check_grad_args(bc, tc));
  if (!a || !w || !out_dot) return fail(OBHIP_ERR_INVALID, "mm_gradhyp_dot: null argument");
  obhip_basis &b = *const_cast<obhip_basis *>(bc);
  obhip_terms &t = *const_cast<obhip_terms *>(tc);
  OB_TRY(ensure_gradbasis(b));
  DevBuf<double> da, dw, dout;
  OB_TRY(da.upload(a, t.p));
  OB_TRY(dw.upload(w, b.n));
  OB_TRY(dout.alloc(b.n));
  OB_TRY(launch_mm(b, t, da.p, dout.p, false));
  OB_TRY(mm_gradhyp_dot_dev(b, t, a, dout.p, dw.p, out_dot));
  if (out) OB_TRY(d2h(out, dout.p, b.n * sizeof(double)));
  return 0;
}

int obhip_basis_sqmm_gradhyp(const obhip_basis *b, const obhip_terms *t, const double *a, double *out_gradhyp) {
  return sq_gradhyp(b, t, a, out_gradhyp, false);
}

int obhip_basis_sqtmm_gradhyp(const obhip_basis *b, const obhip_terms *t, const double *a, double *out_gradhyp) {
  return sq_gradhyp(b, t, a, out_gradhyp, true);
}

int obhip_basis_sqcolsums_gradhyp(const obhip_basis *b, const obhip_terms *t, double *out_gradhyp) {
  if (!b) return fail(OBHIP_ERR_INVALID, "sqcolsums_gradhyp: null argument");
  return sq_gradhyp(b, t, nullptr, out_gradhyp, true);  // ones: modandbase.cpp:875-879
}

int obhip_basis_residvar_gradhyp(const obhip_basis *b, const obhip_terms *t, const obhip_model *m,
                                 double *out_gradhyp) {
  if (!b || !t || !m || !out_gradhyp) return fail(OBHIP_ERR_INVALID, "residvar_gradhyp: null argument");
  if (m != b->model) return fail(OBHIP_ERR_INVALID, "residvar_gradhyp: basis belongs to another model");
  const uint64_t p = t->p, n = b->n, nh = m->nhyp(), d = m->d;
  // varc = getvar(terms), lvarge = getlvar_gradhyp(terms) (modandbase.cpp:350-356, 364-379)
  std::vector<double> varc(p), col(p), tmp(n);
  for (uint64_t k = 0; k < p; ++k) {
    double sv = 0;
    for (uint64_t l = 0; l < d; ++l) sv += m->basisvar[m->knotptst[l] + t->lev[k * d + l]];
    varc[k] = std::exp(sv);
  }
  OB_TRY(sq_gradhyp(b, t, varc.data(), out_gradhyp, false));  // :909
  for (uint64_t i = 0; i < n * nh; ++i) out_gradhyp[i] = -out_gradhyp[i];
  for (uint64_t h = 0; h < nh; ++h) {  // :912-919: minus B^2 (lvarge % varc), column by column
    const uint64_t l = m->hypmatch[h];
    for (uint64_t k = 0; k < p; ++k)
      col[k] = varc[k] * m->logbasisvar_gradhyp[m->gest[h] + t->lev[k * d + l]];
    OB_TRY(obhip_basis_sqmm(b, t, col.data(), 1, tmp.data()));
    for (uint64_t i = 0; i < n; ++i) out_gradhyp[h * n + i] -= tmp[i];
  }
  return 0;
}

int obhip_basis_tmm_gradhyp(const obhip_basis *bc, const obhip_terms *tc, const double *a,
                            double *out, double *out_gradhyp) {
  OB_TRY(check_grad_args(bc, tc));
  if (!a || !out_gradhyp) return fail(OBHIP_ERR_INVALID, "tmm_gradhyp: null argument");
  obhip_basis &b = *const_cast<obhip_basis *>(bc);
  obhip_terms &t = *const_cast<obhip_terms *>(tc);
  OB_TRY(ensure_gradbasis(b));
  DevBuf<double> da, dout;
  OB_TRY(da.upload(a, b.n));
  if (out) {
    OB_TRY(dout.alloc(t.p));
    OB_TRY(launch_tmm(b, t, da.p, dout.p, false));
    OB_TRY(d2h(out, dout.p, t.p * sizeof(double)));
  }
  return tmm_gradhyp_all(b, t, false, da.p, out_gradhyp);
}

// What the gradient products of (b, t) will launch, from the very functions the launchers take their
// geometry from (grad_plan, build_d3_groups, d3_geometry, ge0_geometry, btu_geometry, grad_view_groups).
// Nothing is launched but what prepares the tables: the gradient basis and the terms' device tables.
int obhip_grad_plan_info(const obhip_basis *bc, const obhip_terms *tc, uint64_t *info, uint64_t *groups,
                         uint64_t *members, int64_t *passes) {
  OB_TRY(check_grad_args(bc, tc));
  if (!info) return fail(OBHIP_ERR_INVALID, "grad_plan_info: null argument");
  obhip_basis &b = *const_cast<obhip_basis *>(bc);
  obhip_terms &t = *const_cast<obhip_terms *>(tc);
  OB_TRY(ensure_gradbasis(b));
  OB_TRY(t.prepare(b.md.cap, b.md.dims_h));
  const GradPlan plan = grad_plan(b, t);
  const bool d3 = build_d3_groups(t, b);  // (matmul_gradhyp_dot takes the groups under every plan that has them)
  std::fill(info, info + 16, (uint64_t)0);
  info[0] = (uint64_t)plan;
  info[13] = b.model->nhyp();
  info[14] = b.n_pad / kTileRows;
  info[15] = (uint64_t)device_cus(b.device);
  if (d3) {
    info[1] = t.ge.d3.size();
    for (const obhip_terms::GeD3 &grp : t.ge.d3) {
      const D3Geom q = d3_geometry(b, grp);
      const obhip_terms &v = *grp.v;
      if (groups) {
        const uint64_t row[10] = {(uint64_t)grp.nh, v.W, v.Mu, v.p, v.p_pad, (uint64_t)q.nu, q.pblocks, q.nsplit,
                                  q.tps, (uint64_t)grp.hyp0.size()};
        groups = std::copy(row, row + 10, groups);
      }
      if (members) members = std::copy(grp.hyp0.begin(), grp.hyp0.end(), members);
      info[10] += grp.hyp0.size();
    }
  }
  if (plan == GradPlan::Fused || plan == GradPlan::Ge0Views) {
    const Ge0Geom q = ge0_geometry(b, t);
    info[2] = q.nw == 32 ? 1 : (q.nw == 16 ? 2 : 3);
    info[6] = q.pblocks, info[7] = q.nsplit, info[8] = q.tps, info[9] = q.passes.size();
    if (passes)
      for (const Ge0Pass &ps : q.passes) {
        const int64_t row[4] = {ps.h0, ps.nh, ps.n4 >= 0 ? 1 : 0, ps.n4 < 0 ? -ps.n4 : ps.n4};
        passes = std::copy(row, row + 4, passes);
      }
  } else if (plan == GradPlan::BmatViews) {
    const BtuGeom q = btu_geometry(b, t);
    const int nhyp = (int)b.model->nhyp();
    info[2] = 4;
    info[6] = q.gy, info[7] = q.nsplit, info[8] = q.tps, info[9] = (uint64_t)((nhyp + q.nhb - 1) / q.nhb);
    if (passes)
      for (int h0 = 0; h0 < nhyp; h0 += q.nhb) {
        const int64_t row[4] = {h0, std::min(q.nhb, nhyp - h0), 0, 0};
        passes = std::copy(row, row + 4, passes);
      }
  }
  info[3] = t.W / 2, info[4] = t.Mu, info[5] = t.p_pad;
  if (plan == GradPlan::Ge0Views || plan == GradPlan::BmatViews) {
    const obhip_basis &src = *b.grad->gb;
    for (obhip_terms::GeGroup &grp : grad_view_groups(t, b, false)) {
      ++info[11];
      if (!view_group_one_pass(*grp.v, src)) ++info[12];
    }
  }
  return 0;
}

}  // extern "C"

// ---- device-level forms for the likelihood classes (lpdf.cpp): inputs and the n-sized
// results stay in HBM, only p- and nhyp-sized results go to the host -----------------------
namespace obhip {

// dge (n x nhyp, device) = d(B a)/dhyp (squared: d(B^2 a)/dhyp), d_M = B a (B^2 a);
// a_host / d_a: the same p coefficients on the host and on the device
int grad_mm_dev(obhip_basis &b, obhip_terms &t, bool squared, const double *a_host, const double *d_a,
                double *d_M, DevBuf<double> &dge) {
  OB_TRY(check_grad_args(&b, &t));
  OB_TRY(squared ? ensure_gradbasis_sq(b) : ensure_gradbasis(b));
  return mm_gradhyp_dev(b, t, squared, a_host, d_a, d_M, dge);
}

// out_host[h] = w^T d(B a)/dhyp_h from d_M = B a (mm_gradhyp_dot_dev)
int grad_mm_dot_dev(obhip_basis &b, obhip_terms &t, const double *a_host, const double *d_M,
                    const double *d_w, double *out_host) {
  OB_TRY(check_grad_args(&b, &t));
  OB_TRY(ensure_gradbasis(b));
  return mm_gradhyp_dot_dev(b, t, a_host, d_M, d_w, out_host);
}

// Both hyper-gradient contractions of a likelihood in one sweep (k_tmm_d3 MODE 3):
//   out_dot (nhyp)       = w1^T d(B a)/dhyp            (grad_mm_dot_dev; d_M = B a)
//   out_sq  (p x nhyp)   = sum_i w2_i d(B^2)_ik/dhyp   (grad_tmm_host squared; d_w2 null: ones)
// kNotFused unless the plan is GradPlan::Fused: the caller then asks for the two singly.
int grad_dual_dev(obhip_basis &b, obhip_terms &t, const double *a_host, const double *d_M, const double *d_w1,
                  const double *d_w2, double *out_dot, double *out_sq) {
  HostTimer ht("grad_dual_dev");
  OB_TRY(check_grad_args(&b, &t));
  OB_TRY(ensure_gradbasis(b));
  OB_TRY(t.prepare(b.md.cap, b.md.dims_h));
  if (grad_plan(b, t) != GradPlan::Fused) return kNotFused;
  const uint64_t nh = b.model->nhyp(), n = b.n, p = t.p;
  if (nh == 0) return 0;
  DevBuf<double> ones, dpart, dres;
  if (!d_w2) {
    OB_TRY(ones.alloc(n));
    OB_TRY(launch_fill(ones.p, n, 1.0));
    d_w2 = ones.p;
  }
  // The whole sweep is enqueued before the host reads anything: [nh level-0 dot products |
  // p x nh dense part | the groups' blocks], ONE copy at the end (every blocking copy in between
  // would drain the queue: ten of them per evaluation in the first version).
  const uint64_t head = nh + p * nh;
  std::vector<double> host(head + d3_doubles(t));
  OB_TRY(dres.alloc(host.size()));
  OB_TRY(launch_wdot_ge0(b, d_M, d_w1, dpart, dres.p));
  OB_TRY(launch_tmm_ge0(b, t, true, d_w2, dres.p + nh));
  OB_TRY(enqueue_d3_groups(b, t, 3, d_w1, d_w2, dres.p + head));
  OB_TRY(d2h(host.data(), dres.p, host.size() * sizeof(double)));
  std::copy(host.begin(), host.begin() + nh, out_dot);
  std::copy(host.begin() + nh, host.begin() + head, out_sq);
  each_d3_member(t, host.data() + head,
                 [&](uint64_t h, const std::vector<uint32_t> &ix, const double *u1, const double *u2) {
                   long double s2 = 0;
                   for (size_t q = 0; q < ix.size(); ++q) {
                     s2 += (long double)a_host[ix[q]] * u1[q];
                     out_sq[h * p + ix[q]] += 2.0 * u2[q];
                   }
                   out_dot[h] += (double)s2;
                 });
  return 0;
}

// out_host[c] = sum_i w_i G[i + c n], c < ncol (G: n x ncol column-major, device)
int grad_wdot_dev(const double *d_G, const double *d_w, uint64_t n, uint64_t ncol, double *out_host) {
  if (ncol == 0) return 0;
  DevBuf<double> dpart, dres;
  OB_TRY(dpart.alloc(ncol * kWdotBlocks));
  OB_TRY(dres.alloc(ncol));
  hipLaunchKernelGGL(k_wdot1, dim3(kWdotBlocks, (unsigned)ncol), dim3(256), 0, cur_stream(), d_G, d_w, n,
                     dpart.p);
  hipLaunchKernelGGL(k_wdot2, dim3((unsigned)ncol), dim3(64), 0, cur_stream(), dpart.p, kWdotBlocks, dres.p);
  OB_HIP(hipGetLastError());
  return d2h(out_host, dres.p, ncol * sizeof(double));
}

// out_host (p x nhyp column-major) = sum_i a_i dB_ik/dhyp_h (squared: of B^2)
int grad_tmm_host(obhip_basis &b, obhip_terms &t, bool squared, const double *d_a, double *out_host) {
  OB_TRY(check_grad_args(&b, &t));
  OB_TRY(ensure_gradbasis(b));  // (tmm_gradhyp_all asks for the squared store where it needs it)
  return tmm_gradhyp_all(b, t, squared, d_a, out_host);
}

}  // namespace obhip
