// Kernels of the streaming Newton fit (normal_acc.cpp; no reference counterpart).  An accumulator
// keeps the normal equations of the rows it has seen in ONE device buffer
//   [ upper triangle of G = B^T B, row-major packed: p (p + 1) / 2 ][ R = B^T (Y - c) : p x q ]
//   [ b1 = B^T 1 : p ][ per response (c, mu, M2, n) : 4 q ]
// with c_j a fixed shift of response j (its first row ever added), mu_j = mean(y_j) - c_j and
// M2_j = sum (y_j - mean)^2 of the rows in the state.  A batch is brought into the same layout in
// scratch (Gram kernels, B^T [Y - c | 1]) and folded in with a sign; two states merge the same way.
// The moments merge by the pairwise update of Chan, Golub and LeVeque (1983) and leave by its
// inverse; every quantity that is merged is a difference from c, so a response whose mean is 1e6
// standard deviations from zero loses no digits to the offset.
// All kernels stream HBM once, index with 64 bits (p = 16384: 1.34e8 triangle entries) and sum in
// a fixed order: no atomics.
#include "obhip_internal.h"
#include "vec_ops.h"

namespace obhip {

namespace {

// (c, mu, M2, n) of a state whose shift is moved to c_to
struct Mom {
  double mu, M2, n;
};

// a + b
__device__ __forceinline__ Mom mom_merge(Mom a, Mom b) {
  if (a.n == 0.0) return b;
  if (b.n == 0.0) return a;
  const double n = a.n + b.n, delta = b.mu - a.mu;
  Mom r;
  r.n = n;
  r.mu = a.mu + delta * (b.n / n);
  r.M2 = a.M2 + b.M2 + delta * delta * (a.n * b.n / n);
  return r;
}

// t - b for b a part of t
__device__ __forceinline__ Mom mom_remove(Mom t, Mom b) {
  Mom r;
  r.n = t.n - b.n;
  if (b.n == 0.0) return t;
  if (r.n <= 0.0) {
    r.n = r.mu = r.M2 = 0.0;
    return r;
  }
  r.mu = t.mu - (b.mu - t.mu) * (b.n / r.n);
  const double delta = b.mu - r.mu;
  r.M2 = fmax(t.M2 - b.M2 - delta * delta * (r.n * b.n / t.n), 0.0);
  return r;
}

// ---- a batch into the state's layout --------------------------------------------------------
// shift of every response for this batch: the state's, or the batch's first row for an empty state
__global__ void __launch_bounds__(256)
k_acc_pick_shift(const double *__restrict__ Y, uint64_t ldy, int q, int empty,
                 const double *__restrict__ mom_state, double *__restrict__ mom_batch) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < q) mom_batch[4 * j] = empty ? Y[(uint64_t)j * ldy] : mom_state[4 * j];
}

// Ys (n x (q + 1), ld = n) = [Y - c | 1]
__global__ void __launch_bounds__(256)
k_acc_shift_y(const double *__restrict__ Y, uint64_t ldy, uint64_t n, int q,
              const double *__restrict__ mom_batch, double *__restrict__ Ys) {
  const int j = blockIdx.y;
  const double c = j < q ? mom_batch[4 * j] : 0.0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
    Ys[(uint64_t)j * n + i] = j < q ? Y[(uint64_t)j * ldy + i] - c : 1.0;
}

// ---- folding one state into another ---------------------------------------------------------
// dst[e] += sign src[e] over the packed triangle: two doubles per lane and load (the triangle
// starts on a 16-byte boundary), grid-stride, then the odd last entry
__global__ void __launch_bounds__(256)
k_acc_fold(double *__restrict__ dst, const double *__restrict__ src, uint64_t count, double sign) {
  const uint64_t pairs = count / 2;
  double2 *d2 = reinterpret_cast<double2 *>(dst);
  const double2 *s2 = reinterpret_cast<const double2 *>(src);
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < pairs; e += stride) {
    double2 a = d2[e];
    const double2 b = s2[e];
    a.x += sign * b.x;
    a.y += sign * b.y;
    d2[e] = a;
  }
  if ((count & 1) && blockIdx.x == 0 && threadIdx.x == 0) dst[count - 1] += sign * src[count - 1];
}

// [R | b1] (p x (q + 1)): the source's right-hand sides are first moved to the destination's shift,
// B^T (y - c_dst) = B^T (y - c_src) + (c_src - c_dst) B^T 1; an empty destination takes the source's
__global__ void __launch_bounds__(256)
k_acc_fold_rhs(double *__restrict__ dst, const double *__restrict__ src, uint64_t p, int q,
               const double *__restrict__ mom_dst, const double *__restrict__ mom_src, int dst_empty,
               double sign) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= p * (uint64_t)(q + 1)) return;
  const uint64_t j = e / p, k = e % p;
  double v = src[e];
  if (j < (uint64_t)q && !dst_empty) v = fma(mom_src[4 * j] - mom_dst[4 * j], src[(uint64_t)q * p + k], v);
  dst[e] += sign * v;
}

// the moments (after k_acc_fold_rhs, which reads the shifts as they were)
__global__ void __launch_bounds__(256)
k_acc_fold_mom(double *__restrict__ mom_dst, const double *__restrict__ mom_src, int q, int dst_empty,
               double sign) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= q) return;
  const double cs = mom_src[4 * j];
  const double cd = dst_empty ? cs : mom_dst[4 * j];
  Mom a = {mom_dst[4 * j + 1], mom_dst[4 * j + 2], dst_empty ? 0.0 : mom_dst[4 * j + 3]};
  Mom b = {mom_src[4 * j + 1] + (cs - cd), mom_src[4 * j + 2], mom_src[4 * j + 3]};
  const Mom r = sign > 0.0 ? mom_merge(a, b) : mom_remove(a, b);
  mom_dst[4 * j] = cd;
  mom_dst[4 * j + 1] = r.mu;
  mom_dst[4 * j + 2] = r.M2;
  mom_dst[4 * j + 3] = r.n;
}

// ---- the Newton step on a state (minus another) ------------------------------------------------
// moments of the rows that remain and the right-hand sides of their standardised problem,
// e2 B^T ((y_j - cent_j) / sd_j) = e2 ((R - mu b1) - (R' - (mu + c - c') b1')) / sd_j with the
// primed quantities of the state taken out; meansd: q triples (cent, sd with n - 1 denominator, n).
// Every thread of column j derives the same moments from the same 8 numbers.
__global__ void __launch_bounds__(256)
k_acc_rhs(const double *__restrict__ rb, const double *__restrict__ mom, const double *__restrict__ rb_minus,
          const double *__restrict__ mom_minus, uint64_t p, int q, double e2, double *__restrict__ rhs,
          double *__restrict__ meansd) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= p * (uint64_t)q) return;
  const uint64_t j = e / p, k = e % p;
  const double c = mom[4 * j];
  Mom m = {mom[4 * j + 1], mom[4 * j + 2], mom[4 * j + 3]};
  double dc = 0.0;
  if (rb_minus) {
    dc = c - mom_minus[4 * j];
    const Mom b = {mom_minus[4 * j + 1] - dc, mom_minus[4 * j + 2], mom_minus[4 * j + 3]};
    m = mom_remove(m, b);
  }
  const double sd = sqrt(m.M2 / (m.n - 1.0));
  double v = fma(-m.mu, rb[(uint64_t)q * p + k], rb[e]);
  if (rb_minus) v -= fma(-(m.mu + dc), rb_minus[(uint64_t)q * p + k], rb_minus[e]);
  rhs[e] = e2 * (v / sd);
  if (k == 0) {
    meansd[3 * j] = c + m.mu;
    meansd[3 * j + 1] = sd;
    meansd[3 * j + 2] = m.n;
  }
}

}  // namespace

// d_mom_batch[4 j] = shift, d_Ys (n x (q + 1)) = [Y - shift | 1], then (mu, M2, n) of the shifted
// batch by two passes of vcolsum; d_part: kSumBlocks q doubles
int launch_acc_batch_moments(const double *d_Y, uint64_t ldy, uint64_t n, uint64_t q, bool empty,
                             const double *d_mom_state, double *d_mom_batch, double *d_Ys, double *d_part) {
  hipStream_t st = cur_stream();
  const unsigned qb = (unsigned)((q + 255) / 256);
  hipLaunchKernelGGL(k_acc_pick_shift, dim3(qb), dim3(256), 0, st, d_Y, ldy, (int)q, empty ? 1 : 0, d_mom_state,
                     d_mom_batch);
  hipLaunchKernelGGL(k_acc_shift_y, dim3(sum_blocks(n), (unsigned)q + 1), dim3(256), 0, st, d_Y, ldy, n, (int)q,
                     (const double *)d_mom_batch, d_Ys);
  OB_HIP(hipGetLastError());
  const double *ys = d_Ys;
  double *mom = d_mom_batch;
  const double nrows = (double)n;
  OB_TRY(vcolsum(n, q, [=] __device__(int j, uint64_t i, double &acc) { acc += ys[(uint64_t)j * n + i]; },
                 [=] __device__(int j, double s) {
                   mom[4 * j + 1] = s / nrows;
                   mom[4 * j + 3] = nrows;
                 },
                 d_part));
  return vcolsum(n, q, [=] __device__(int j, uint64_t i, double &acc) {
    const double c = ys[(uint64_t)j * n + i] - mom[4 * j + 1];
    acc = fma(c, c, acc);
  }, [=] __device__(int j, double s) { mom[4 * j + 2] = s; }, d_part);
}

// dst +/- src, both in the accumulator's layout
int launch_acc_fold(uint64_t p, uint64_t q, double *d_dst, const double *d_src, bool dst_empty, double sign) {
  ProfScope ps("acc_fold");
  hipStream_t st = cur_stream();
  const uint64_t tri = p * (p + 1) / 2;
  const unsigned blocks = (unsigned)std::min<uint64_t>(8192, (tri / 2 + 255) / 256 + 1);
  hipLaunchKernelGGL(k_acc_fold, dim3(blocks), dim3(256), 0, st, d_dst, d_src, tri, sign);
  return launch_acc_fold_tail(p, q, d_dst + tri, d_src + tri, dst_empty, sign);
}

// [R | b1] and the moments alone (a grid batch folds its triangle from two factors: kernels_product_fit.hip)
int launch_acc_fold_tail(uint64_t p, uint64_t q, double *d_dst_tail, const double *d_src_tail, bool dst_empty,
                         double sign) {
  hipStream_t st = cur_stream();
  const uint64_t nrb = p * (q + 1);
  hipLaunchKernelGGL(k_acc_fold_rhs, dim3((unsigned)((nrb + 255) / 256)), dim3(256), 0, st, d_dst_tail, d_src_tail, p,
                     (int)q, (const double *)(d_dst_tail + nrb), d_src_tail + nrb, dst_empty ? 1 : 0, sign);
  hipLaunchKernelGGL(k_acc_fold_mom, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, st, d_dst_tail + nrb,
                     d_src_tail + nrb, (int)q, dst_empty ? 1 : 0, sign);
  OB_HIP(hipGetLastError());
  return 0;
}

// dst +/- src over [tri][R] alone: gradient rows add nothing to B^T 1 and the moments, and R needs no
// move of the shift (their part of it does not depend on c)
int launch_acc_fold_grad(uint64_t p, uint64_t q, double *d_dst, const double *d_src, double sign) {
  ProfScope ps("acc_fold");
  const uint64_t count = p * (p + 1) / 2 + p * q;
  const unsigned blocks = (unsigned)std::min<uint64_t>(8192, (count / 2 + 255) / 256 + 1);
  hipLaunchKernelGGL(k_acc_fold, dim3(blocks), dim3(256), 0, cur_stream(), d_dst, d_src, count, sign);
  OB_HIP(hipGetLastError());
  return 0;
}

// d_state / d_minus (may be null): whole accumulator buffers
int launch_acc_rhs(uint64_t p, uint64_t q, const double *d_state, const double *d_minus, double e2, double *d_rhs,
                   double *d_meansd) {
  const uint64_t tri = p * (p + 1) / 2, nrb = p * (q + 1);
  hipLaunchKernelGGL(k_acc_rhs, dim3((unsigned)((p * q + 255) / 256)), dim3(256), 0, cur_stream(), d_state + tri,
                     d_state + tri + nrb, d_minus ? d_minus + tri : nullptr, d_minus ? d_minus + tri + nrb : nullptr, p,
                     (int)q, e2, d_rhs, d_meansd);
  OB_HIP(hipGetLastError());
  return 0;
}

// per response the sum over the rows of (cent + sd mean - y)^2 (meansd null: mean is in raw units
// already) and the row count, in the summation order of vsum; d_part: kSumBlocks q doubles
int launch_cv_score(const double *d_mean, const double *d_Y, uint64_t n, uint64_t q, uint64_t ld,
                    const double *d_meansd, double *d_out, double *d_part) {
  const double nrows = (double)n;
  return vcolsum(n, q, [=] __device__(int j, uint64_t i, double &acc) {
    const double cent = d_meansd ? d_meansd[3 * j] : 0.0, sd = d_meansd ? d_meansd[3 * j + 1] : 1.0;
    const double r = fma(sd, d_mean[(uint64_t)j * ld + i], cent) - d_Y[(uint64_t)j * ld + i];
    acc = fma(r, r, acc);
  }, [=] __device__(int j, double s) {
    d_out[2 * j] = s;
    d_out[2 * j + 1] = nrows;
  }, d_part);
}

}  // namespace obhip
