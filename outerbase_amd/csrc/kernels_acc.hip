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

namespace obhip {

namespace {

__device__ __forceinline__ uint64_t tri_off(uint64_t i, uint64_t p) {
  return i * p - i * (i - 1) / 2;  // start of row i (entries j >= i) in the packed triangle
}

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

// column sums of the shifted batch in the summation order of vsum (vec_ops.h): grid (blocks, q);
// MODE 0: sum v, MODE 1: sum (v - mu)^2 with mu = mom_batch[4 j + 1]
template <int MODE>
__global__ void __launch_bounds__(256)
k_acc_colsum1(const double *__restrict__ Ys, uint64_t n, const double *__restrict__ mom_batch,
              double *__restrict__ part) {
  __shared__ double red[256];
  const int j = blockIdx.y;
  const double *y = Ys + (uint64_t)j * n;
  const double mu = MODE == 1 ? mom_batch[4 * j + 1] : 0.0;
  double acc = 0.0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    if (MODE == 0) {
      acc += y[i];
    } else {
      const double c = y[i] - mu;
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

// one wave per column; MODE 0: mu = sum / n and n; MODE 1: M2 = sum
template <int MODE>
__global__ void __launch_bounds__(64)
k_acc_colsum2(const double *__restrict__ part, int nblk, double nrows, double *__restrict__ mom_batch) {
  const int j = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 64) s += part[(uint64_t)j * nblk + b];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  if (threadIdx.x == 0) {
    if (MODE == 0) {
      mom_batch[4 * j + 1] = s / nrows;
      mom_batch[4 * j + 3] = nrows;
    } else {
      mom_batch[4 * j + 2] = s;
    }
  }
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
// 64 x 64 tile (bi <= bj) of the packed triangle(s) -> H = e2 (T - T_minus) + diag(prec) in full
// symmetric storage (lpdfvec::hess_, fit.cpp:503-512) and its diagonal: H[i][j] in 512-byte row
// segments and, transposed through LDS, H[j][i] likewise
__global__ void __launch_bounds__(256)
k_acc_form(const double *__restrict__ tri, const double *__restrict__ tri_minus, uint64_t p, int nb,
           double *__restrict__ H, double e2, const double *__restrict__ prec, double *__restrict__ diagH) {
  __shared__ double S[64 * 65];
  int bi = 0, rem = blockIdx.x;
  while (rem >= nb - bi) {
    rem -= nb - bi;
    ++bi;
  }
  const int bj = bi + rem;
  const int c = threadIdx.x & 63, r4 = threadIdx.x >> 6;
  const uint64_t j = (uint64_t)bj * 64 + c;
  for (int r = r4; r < 64; r += 4) {
    const uint64_t i = (uint64_t)bi * 64 + r;
    double v = 0.0;
    if (i < p && j < p && j >= i) {
      const uint64_t o = tri_off(i, p) + (j - i);
      v = tri[o];
      if (tri_minus) v -= tri_minus[o];
      v *= e2;
      if (i == j) {
        v += prec[i];
        if (diagH) diagH[i] = v;
      }
      H[i * p + j] = v;
    }
    S[r * 65 + c] = v;
  }
  __syncthreads();
  // mirror: row jj = 64 bj + r, column ii = 64 bi + c holds S[c][r]; strictly below the diagonal only
  const uint64_t ii = (uint64_t)bi * 64 + c;
  for (int r = r4; r < 64; r += 4) {
    const uint64_t jj = (uint64_t)bj * 64 + r;
    if (jj < p && ii < p && ii < jj) H[jj * p + ii] = S[c * 65 + r];
  }
}

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

// ---- held-out score ------------------------------------------------------------------------------
// per response the sum over the rows of (cent + sd mean - y)^2 (meansd null: mean is in raw units
// already), in the summation order of vsum
__global__ void __launch_bounds__(256)
k_cv_score1(const double *__restrict__ mean, const double *__restrict__ Y, uint64_t n, uint64_t ld,
            const double *__restrict__ meansd, double *__restrict__ part) {
  __shared__ double red[256];
  const int j = blockIdx.y;
  const double cent = meansd ? meansd[3 * j] : 0.0, sd = meansd ? meansd[3 * j + 1] : 1.0;
  const double *m = mean + (uint64_t)j * ld, *y = Y + (uint64_t)j * ld;
  double acc = 0.0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const double r = fma(sd, m[i], cent) - y[i];
    acc = fma(r, r, acc);
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(uint64_t)j * gridDim.x + blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(64)
k_cv_score2(const double *__restrict__ part, int nblk, double nrows, double *__restrict__ out) {
  const int j = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 64) s += part[(uint64_t)j * nblk + b];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  if (threadIdx.x == 0) {
    out[2 * j] = s;
    out[2 * j + 1] = nrows;
  }
}

int sum_blocks(uint64_t n) { return (int)std::min<uint64_t>(512, std::max<uint64_t>(1, (n + 255) / 256)); }

}  // namespace

// d_mom_batch[4 j] = shift, d_Ys (n x (q + 1)) = [Y - shift | 1], then (mu, M2, n) of the shifted
// batch by two passes; d_part: 512 q doubles
int launch_acc_batch_moments(const double *d_Y, uint64_t ldy, uint64_t n, uint64_t q, bool empty,
                             const double *d_mom_state, double *d_mom_batch, double *d_Ys, double *d_part) {
  hipStream_t st = cur_stream();
  const int nblk = sum_blocks(n);
  const unsigned qb = (unsigned)((q + 255) / 256);
  hipLaunchKernelGGL(k_acc_pick_shift, dim3(qb), dim3(256), 0, st, d_Y, ldy, (int)q, empty ? 1 : 0, d_mom_state,
                     d_mom_batch);
  hipLaunchKernelGGL(k_acc_shift_y, dim3(nblk, (unsigned)q + 1), dim3(256), 0, st, d_Y, ldy, n, (int)q,
                     (const double *)d_mom_batch, d_Ys);
  hipLaunchKernelGGL(k_acc_colsum1<0>, dim3(nblk, (unsigned)q), dim3(256), 0, st, (const double *)d_Ys, n,
                     (const double *)d_mom_batch, d_part);
  hipLaunchKernelGGL(k_acc_colsum2<0>, dim3((unsigned)q), dim3(64), 0, st, (const double *)d_part, nblk, (double)n,
                     d_mom_batch);
  hipLaunchKernelGGL(k_acc_colsum1<1>, dim3(nblk, (unsigned)q), dim3(256), 0, st, (const double *)d_Ys, n,
                     (const double *)d_mom_batch, d_part);
  hipLaunchKernelGGL(k_acc_colsum2<1>, dim3((unsigned)q), dim3(64), 0, st, (const double *)d_part, nblk, (double)n,
                     d_mom_batch);
  OB_HIP(hipGetLastError());
  return 0;
}

// dst +/- src, both in the accumulator's layout
int launch_acc_fold(uint64_t p, uint64_t q, double *d_dst, const double *d_src, bool dst_empty, double sign) {
  ProfScope ps("acc_fold");
  hipStream_t st = cur_stream();
  const uint64_t tri = p * (p + 1) / 2, nrb = p * (q + 1);
  const unsigned blocks = (unsigned)std::min<uint64_t>(8192, (tri / 2 + 255) / 256 + 1);
  hipLaunchKernelGGL(k_acc_fold, dim3(blocks), dim3(256), 0, st, d_dst, d_src, tri, sign);
  hipLaunchKernelGGL(k_acc_fold_rhs, dim3((unsigned)((nrb + 255) / 256)), dim3(256), 0, st, d_dst + tri, d_src + tri, p,
                     (int)q, (const double *)(d_dst + tri + nrb), d_src + tri + nrb, dst_empty ? 1 : 0, sign);
  hipLaunchKernelGGL(k_acc_fold_mom, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, st, d_dst + tri + nrb,
                     d_src + tri + nrb, (int)q, dst_empty ? 1 : 0, sign);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_acc_form(uint64_t p, const double *d_tri, const double *d_tri_minus, double *d_H, double e2,
                    const double *d_prec, double *d_diagH) {
  ProfScope ps("acc_form");
  const int nb = (int)((p + 63) / 64);
  hipLaunchKernelGGL(k_acc_form, dim3((unsigned)(nb * (nb + 1) / 2)), dim3(256), 0, cur_stream(), d_tri, d_tri_minus, p,
                     nb, d_H, e2, d_prec, d_diagH);
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

// d_part: 512 q doubles
int launch_cv_score(const double *d_mean, const double *d_Y, uint64_t n, uint64_t q, uint64_t ld,
                    const double *d_meansd, double *d_out, double *d_part) {
  const int nblk = sum_blocks(n);
  hipStream_t st = cur_stream();
  hipLaunchKernelGGL(k_cv_score1, dim3(nblk, (unsigned)q), dim3(256), 0, st, d_mean, d_Y, n, ld, d_meansd, d_part);
  hipLaunchKernelGGL(k_cv_score2, dim3((unsigned)q), dim3(64), 0, st, (const double *)d_part, nblk, (double)n, d_out);
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace obhip
