// Newton fit and predictor for q responses over one design x (no reference counterpart: the
// reference fits one y, R/fitting.R:40-120; the matrix forms it has are prodmm_ / tprodmm_,
// src/linalg.cpp:481-637).  The model, the terms, sigma and rho are shared, every response is
// standardised on its own (R/fitting.R:55-57), so G = B^T B, H = e^{-2 sigma} G + prior and its
// Cholesky factor are formed ONCE and only what depends on Y is batched over the responses:
//   B^T Y      response 0 rides along the staging pass of the design matrix exactly as the single
//              fit's y does (GramFuse, else launch_tmm); the others come from one pass of k_aty_multi over the
//              staged matrix per 64 responses -- or, where the matrix is not resident as a whole
//              (row chunks, Gram backend 3) or fewer than kMultiMinCols columns are left, from a
//              column loop over launch_tmm;
//   the solves launch_newton_solve factorises with response 0's right-hand side (today's code path,
//              untouched, and its theta is response 0's); the other columns go through the blocked
//              substitutions of launch_trsm_multi on the finished factor;
//   predict    k_predict_multi where the terms fit it and kMultiMinCols columns are left, a column
//              loop over launch_predict otherwise
//              (and for q = 1, which then is the single predictor bit for bit).
// Everything is column-major: Y n x q (ldy), Theta p x q, mean n_new x q.
#include <cmath>
#include <cstring>

#include "obhip_internal.h"
#include "vec_ops.h"

using namespace obhip;

namespace obhip {
int launch_unpack_form(uint64_t p, const double *d_tri, double *d_H, double e2, const double *d_prec,
                       double *d_diagH);
std::vector<double> prior_prec_of(const obhip_model &m, const obhip_terms &t, double rho);
int check_compat_of(const obhip_model *m, const obhip_terms *t);
}  // namespace obhip

namespace {

// Column sums in the summation order of vsum (vec_ops.h), so that a column gets the bits
// obhip_standardise_dev gives it: grid (blocks, q), MODE 0: sum y, 1: sum (y - cent)^2 with
// cent = st[2 j] / st[2 j + 1].
template <int MODE>
__global__ void __launch_bounds__(256)
k_colsum1(const double *__restrict__ Y, uint64_t ldy, uint64_t n, const double *__restrict__ st,
          double *__restrict__ part) {
  __shared__ double red[256];
  const int j = blockIdx.y;
  const double *y = Y + (uint64_t)j * ldy;
  double acc = 0.0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    if (MODE == 0) {
      acc += y[i];
    } else {
      const double c = y[i] - st[2 * j] / st[2 * j + 1];
      acc = fma(c, c, acc);
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(uint64_t)j * gridDim.x + blockIdx.x] = red[0];
}

// one wave per column; MODE 0: st[2 j] = sum, st[2 j + 1] = n; MODE 1: ss[j] = sum
template <int MODE>
__global__ void __launch_bounds__(64)
k_colsum2(const double *__restrict__ part, int nblk, double nrows, double *__restrict__ out) {
  const int j = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 64) s += part[(uint64_t)j * nblk + b];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  if (threadIdx.x == 0) {
    if (MODE == 0) {
      out[2 * j] = s;
      out[2 * j + 1] = nrows;
    } else {
      out[j] = s;
    }
  }
}

// (sum, n) and sum (y - cent)^2 over all ranks -> (cent, sd, n) per column
__global__ void __launch_bounds__(256)
k_meansd_multi(const double *__restrict__ st, const double *__restrict__ ss, int q,
               double *__restrict__ meansd) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= q) return;
  const double n = st[2 * j + 1], cent = st[2 * j] / n;
  meansd[3 * j] = cent;
  meansd[3 * j + 1] = sqrt(ss[j] / (n - 1.0));  // n - 1 denominator (R's sd)
  meansd[3 * j + 2] = n;
}

int copy_in(DevBuf<double> &d, const double *src, uint64_t rows, uint64_t cols, uint64_t ld) {
  if (ld == rows) return d.upload(src, rows * cols);
  std::vector<double> c(rows * cols);
  for (uint64_t j = 0; j < cols; ++j) std::memcpy(&c[j * rows], src + j * ld, rows * sizeof(double));
  return d.upload(c.data(), c.size());
}

int d2h(void *dst, const void *src, size_t bytes) {
  OB_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, cur_stream()));
  OB_HIP(hipStreamSynchronize(cur_stream()));
  return 0;
}

// columns [1, q) of Theta on the factor launch_newton_solve has just left in d_H
int solve_rest(uint64_t p, const double *d_H, const void *d_cholws, const double *d_G_rhs, uint64_t q, double e2,
               double *d_Theta, void *d_scratch) {
  if (q <= 1) return 0;
  return launch_trsm_multi(p, d_H, newton_workspace_iinv(p, d_cholws), d_G_rhs + p, p, q - 1, e2, d_Theta + p,
                           d_scratch);
}

}  // namespace

extern "C" {

int obhip_standardise_multi_dev(obhip_comm *comm, const double *d_Y_raw, uint64_t n, uint64_t q, uint64_t ldy,
                                double *d_Y, double *d_meansd) {
  if (!d_meansd || q == 0 || q > 65535 || (n != 0 && (!d_Y_raw || !d_Y || ldy < n)))
    return fail(OBHIP_ERR_INVALID, "standardise_multi_dev: bad argument");
  OB_TRY(require_device());
  if (!comm && n < 2) return fail(OBHIP_ERR_INVALID, "standardise_multi_dev: the standard deviation needs two rows");
  const int nblk = (int)std::min<uint64_t>(kSumBlocks, std::max<uint64_t>(1, (n + 255) / 256));
  DevBuf<double> st, part;
  OB_TRY(st.alloc(3 * q));  // [(sum, n) per column][sum of squares per column]
  OB_TRY(part.alloc((size_t)nblk * q));
  hipStream_t s = cur_stream();
  double *ss = st.p + 2 * q;
  hipLaunchKernelGGL(k_colsum1<0>, dim3(nblk, (unsigned)q), dim3(256), 0, s, d_Y_raw, ldy, n, (const double *)st.p,
                     part.p);
  hipLaunchKernelGGL(k_colsum2<0>, dim3((unsigned)q), dim3(64), 0, s, (const double *)part.p, nblk, (double)n, st.p);
  if (comm) OB_TRY(comm_allreduce(comm, st.p, 2 * q));
  hipLaunchKernelGGL(k_colsum1<1>, dim3(nblk, (unsigned)q), dim3(256), 0, s, d_Y_raw, ldy, n, (const double *)st.p,
                     part.p);
  hipLaunchKernelGGL(k_colsum2<1>, dim3((unsigned)q), dim3(64), 0, s, (const double *)part.p, nblk, (double)n, ss);
  if (comm) OB_TRY(comm_allreduce(comm, ss, q));
  hipLaunchKernelGGL(k_meansd_multi, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, s, (const double *)st.p,
                     (const double *)ss, (int)q, d_meansd);
  OB_HIP(hipGetLastError());
  const double *ms = d_meansd, *yi = d_Y_raw;
  double *yo = d_Y;
  return vmap(n * q, [=] __device__(uint64_t e) {
    const uint64_t j = e / n, i = j * ldy + e % n;
    yo[i] = (yi[i] - ms[3 * j]) / ms[3 * j + 1];
  });
}

int obhip_destandardise_multi_dev(double *d_V, uint64_t n, uint64_t q, uint64_t ldv, const double *d_meansd,
                                  int squared) {
  if (!d_meansd || (n != 0 && (!d_V || ldv < n))) return fail(OBHIP_ERR_INVALID, "destandardise_multi_dev: bad argument");
  const double *ms = d_meansd;
  const bool sq = squared != 0;
  return vmap(n * q, [=] __device__(uint64_t e) {
    const uint64_t j = e / n, i = j * ldv + e % n;
    const double sd = ms[3 * j + 1];
    d_V[i] = sq ? sd * sd * d_V[i] : fma(sd, d_V[i], ms[3 * j]);
  });
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

int obhip_newton_multi_solve_dev(const obhip_model *m, const obhip_terms *t, double *d_G, const double *d_G_rhs,
                                 uint64_t q, double sigma, double rho, double *d_Theta, double *d_diagH,
                                 void *d_workspace, uint64_t workspace_bytes) {
  if (!m || !t || !d_G || !d_G_rhs || !d_Theta || !d_workspace || q == 0)
    return fail(OBHIP_ERR_INVALID, "newton_multi_solve_dev: bad argument");
  OB_TRY(check_compat_of(m, t));
  const uint64_t p = t->p;
  uint64_t need = 0, single = 0;
  OB_TRY(obhip_newton_multi_workspace_bytes(p, q, &need));
  OB_TRY(obhip_newton_workspace_bytes(p, &single));
  if (workspace_bytes < need) return fail(OBHIP_ERR_INVALID, "newton_multi_solve_dev: workspace too small");
  // H, the factorisation and response 0 by the single-response entry; the factor stays in d_G
  OB_TRY(obhip_newton_solve_dev(m, t, d_G, d_G_rhs, sigma, rho, d_Theta, d_diagH, d_workspace, single));
  return solve_rest(p, d_G, (double *)d_workspace + 2 * p, d_G_rhs, q, std::exp(-2.0 * sigma), d_Theta,
                    (char *)d_workspace + single);
}

int obhip_fit_newton_multi_dev(obhip_comm *comm, const obhip_basis *bc, const obhip_terms *tc, const obhip_model *m,
                               const double *d_Y, uint64_t q, uint64_t ldy, double sigma, double rho, double *d_H,
                               double *d_G_rhs, double *d_Theta, double *d_diagH, double *d_exbuf,
                               uint64_t exbuf_count, void *d_workspace, uint64_t workspace_bytes) {
  if (!bc || !tc || !m || !d_Y || !d_H || !d_G_rhs || !d_Theta || !d_workspace || q == 0)
    return fail(OBHIP_ERR_INVALID, "fit_newton_multi_dev: bad argument");
  OB_TRY(require_device());
  OB_TRY(check_compat_of(m, tc));
  obhip_terms &t = *const_cast<obhip_terms *>(tc);
  obhip_basis &b = *const_cast<obhip_basis *>(bc);
  if (b.model != m) return fail(OBHIP_ERR_INVALID, "fit_newton_multi_dev: model / terms / basis do not belong together");
  if (ldy < b.n) return fail(OBHIP_ERR_INVALID, "fit_newton_multi_dev: ldy is smaller than the rows of the basis");
  const uint64_t p = t.p;
  uint64_t need = 0, single = 0;
  OB_TRY(obhip_newton_multi_workspace_bytes(p, q, &need));
  OB_TRY(obhip_newton_workspace_bytes(p, &single));
  if (workspace_bytes < need) return fail(OBHIP_ERR_INVALID, "fit_newton_multi_dev: workspace too small");
  const uint64_t tri = p * (p + 1) / 2;
  if (comm) {
    uint64_t cnt = 0;
    OB_TRY(obhip_fit_newton_multi_count(p, q, comm_nranks(comm), &cnt));
    if (!d_exbuf || exbuf_count < cnt) return fail(OBHIP_ERR_INVALID, "fit_newton_multi_dev: exchange buffer too small");
    exbuf_count = cnt;
  }
  double *d_rhs = (double *)d_workspace + p;
  void *d_cholws = d_rhs + p;
  const double e2 = std::exp(-2.0 * sigma);
  hipStream_t st = cur_stream();
  if (!t.prec_dev.p || t.prec_model != m || t.prec_version != m->version || t.prec_rho != rho) {
    const std::vector<double> prec = prior_prec_of(*m, t, rho);
    OB_TRY(t.prec_dev.upload(prec.data(), p));  // (synchronises: prec is a local)
    t.prec_model = m;
    t.prec_version = m->version;
    t.prec_rho = rho;
  }
  const double *d_prec = t.prec_dev.p;
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
  // B^T Y lands behind the packed triangle of a sharded fit
  double *g_dst = comm ? d_exbuf + tri : d_G_rhs;
  GramFuse fuse;
  fuse.y = d_Y;
  fuse.g = g_dst;
  OB_TRY(launch_gram_to(b, t, sink, &fuse));
  // response 0 as the single fit takes it: with the staging pass, or by its own pass over the basis
  if (!fuse.done) OB_TRY(launch_tmm(b, t, d_Y, g_dst, false));
  if (q > 1) {
    if (q - 1 >= kMultiMinCols && b.bmat.p && t.uid != 0 && b.bmat_terms == t.uid) {
      OB_TRY(launch_aty_multi(b, t, d_Y + ldy, ldy, q - 1, g_dst + p, p));
    } else {
      // few columns, or the design matrix is not resident as a whole: one pass over the basis per response
      for (uint64_t j = 1; j < q; ++j) OB_TRY(launch_tmm(b, t, d_Y + j * ldy, g_dst + j * p, false));
    }
  }
  if (comm) {
    {
      ProfScope ps("exchange");
      OB_TRY(comm_allreduce(comm, d_exbuf, exbuf_count));
    }
    OB_TRY(launch_unpack_form(p, d_exbuf, d_H, e2, d_prec, d_diagH));
    OB_HIP(hipMemcpyAsync(d_G_rhs, d_exbuf + tri, p * q * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  // grad at coeff = 0: e^{-2 sigma} B^T y   (loglik_std.cpp:113-116)
  const double *g = d_G_rhs;
  OB_TRY(vmap(p, [=] __device__(uint64_t k) { d_rhs[k] = e2 * g[k]; }));
  OB_TRY(launch_newton_solve(p, d_H, d_rhs, d_Theta, d_cholws, newton_workspace_bytes(p)));
  return solve_rest(p, d_H, d_cholws, d_G_rhs, q, e2, d_Theta, (char *)d_workspace + single);
}

int obhip_predict_multi_dev(const obhip_model *m, const obhip_terms *tc, const double *d_Theta, uint64_t q,
                            const double *d_x, uint64_t n, double *d_mean, const double *d_coeffvar, double sigma,
                            double *d_var) {
  if (!m || !tc || !d_Theta || q == 0 || (n != 0 && (!d_x || !d_mean)))
    return fail(OBHIP_ERR_INVALID, "predict_multi_dev: bad argument");
  OB_TRY(check_compat_of(m, tc));
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
  OB_TRY(check_compat_of(m, t));
  OB_TRY(require_device());
  const uint64_t p = t->p;
  DevBuf<double> dY, dH, dg, dth, ddiag;
  DevBuf<char> ws;
  uint64_t wsb = 0;
  OB_TRY(obhip_newton_multi_workspace_bytes(p, q, &wsb));
  OB_TRY(copy_in(dY, Y, b->n, q, ldy));
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
  OB_TRY(check_compat_of(m, t));
  OB_TRY(require_device());
  DevBuf<double> dx, dth, dmean, dcv, dvar;
  OB_TRY(copy_in(dx, x, n, m->d, ldx));
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
