// The frame of the sums over pairs of terms: the pieces that k_sobol_pairs (kernels_sobol.hip)
// uses, and on top of them k_block_pairs<Op, ND, DIAG>, k_block_reduce and launch_block_pairs<Op> for the sums
// whose outputs form a d x d triangle (Sobol2Op in kernels_sobol.hip, ActiveOp in kernels_active.hip).
//
// Shape: lane = term k of term tile I, its row offsets into the tables in registers; the partner k' of tile J >= I
// is wave-uniform (levels and coefficients by scalar loads); the per-dimension L x L tables of every dimension in
// LDS, entry n_cov of each the neutral factor of a dimension beyond d or one that a pass leaves out.  The triangle of
// outputs is cut into blocks of T dimensions (passes over grid z, sens_plan.h); a pass holds T x T outputs for RC
// responses.  Per term pair: the product of table 0 ("A") over the dimensions outside the pass's blocks (row
// offsets of the first ND dimensions packed in registers, two to a word), then Op::Lane::factors fills f[a * T + b].
// Sums: per lane over k', butterfly per wave, wave 0 + wave 1, k_block_reduce over the tile pairs: a fixed order.
#pragma once
#include "sobol_device.h"

namespace obhip {

// entry(i, ia, ib) for every entry i of the packed L x L tables, ia / ib its row and column in the packed mean table;
// then neutral() by one thread, and the barrier
template <typename Entry, typename Neutral>
__device__ __forceinline__ void stage_pair_tables(const int *__restrict__ meta, int d, Entry entry, Neutral neutral) {
  for (int l = 0; l < d; ++l) {
    const int L = meta[l], om = meta[d + l], oc = meta[2 * d + l];
    for (int e = threadIdx.x; e < L * L; e += kSobolTW) entry(oc + e, om + e / L, om + e % L);
  }
  if (threadIdx.x == 0) neutral();
  __syncthreads();
}

// the lane's term of tile I
struct LaneTerm {
  int k;
  bool valid;
  const uint8_t *lv;  // its levels (a lane beyond p: any term, its coefficient is 0)
};
__device__ __forceinline__ LaneTerm lane_term(const uint8_t *__restrict__ lev, int p, int d, int I) {
  const int k = I * kSobolTW + threadIdx.x;
  const bool valid = k < p;
  return LaneTerm{k, valid, lev + (uint64_t)(valid ? k : p - 1) * d};
}

template <int RC>
__device__ __forceinline__ void load_theta(double (&th)[RC], const double *__restrict__ Theta, const LaneTerm &me,
                                           int j0, int q, int p) {
#pragma unroll
  for (int r = 0; r < RC; ++r) th[r] = me.valid && j0 + r < q ? Theta[(uint64_t)(j0 + r) * p + me.k] : 0.0;
}
// theta_k theta_k' of response j (clamped: th is 0 beyond q)
__device__ __forceinline__ double pair_weight(double th, const double *__restrict__ Theta, int j, int q, int p, int k2) {
  return th * Theta[(uint64_t)min(j, q - 1) * p + k2];
}

// row offsets of the first ND dimensions, two to a word; bit l of umask: the outside product takes dimension l
template <int ND>
struct OutsideOffsets {
  unsigned offp[ND / 2], umask;
};
template <int ND, typename Pred>
__device__ __forceinline__ void pack_outside(OutsideOffsets<ND> &o, const int *__restrict__ meta, int d, int n_cov,
                                             const uint8_t *lv, Pred outside) {
  o.umask = 0;
#pragma unroll
  for (int h = 0; h < ND / 2; ++h) {
    unsigned w = 0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int l = 2 * h + e;
      const bool use = outside(l);
      const int lc = min(l, d - 1);
      w |= (unsigned)(use ? meta[2 * d + lc] + (int)lv[lc] * meta[lc] : n_cov) << (16 * e);
      o.umask |= (use ? 1u : 0u) << l;
    }
    o.offp[h] = w;
  }
}
// the outside product, even and odd dimensions apart (two shorter chains), then the dimensions beyond ND
template <int ND, typename Pred>
__device__ __forceinline__ double outside_product(const OutsideOffsets<ND> &o, const double *tA,
                                                  const int *__restrict__ meta, int d, const uint8_t *lv,
                                                  const uint8_t *lp, Pred outside) {
  double pe = 1.0, po = 1.0;
#pragma unroll
  for (int l = 0; l < ND; ++l) {
    const int off = (int)((o.offp[l / 2] >> (16 * (l & 1))) & 0xffffu);
    const int add = (o.umask >> l) & 1u ? (int)lp[min(l, d - 1)] : 0;
    if (l & 1) po *= tA[off + add];
    else pe *= tA[off + add];
  }
  for (int l = ND; l < d; ++l)                           // (d > ND only)
    if (outside(l)) pe *= tA[meta[2 * d + l] + (int)lv[l] * meta[l] + lp[l]];
  return pe * po;
}

// part[e] = scale * (sum over the block of acc[e]), e < N, where keep(e); 0 elsewhere.  Butterfly per wave, wave 0 +
// wave 1 (blocks of kSobolTW = 128 threads); red: 2 * N doubles of LDS
template <int N, typename Keep>
__device__ __forceinline__ void write_pair_partials(const double (&acc)[N], Keep keep, double *red,
                                                    double *__restrict__ part, double scale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const double v = keep(e) ? wave_sum(acc[e]) : 0.0;
    if (lane == 0) red[wave * N + e] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < N) part[threadIdx.x] = scale * (red[threadIdx.x] + red[N + threadIdx.x]);
}

// Op: T, RC, kTables (LDS tables of n_cov + 1 entries, table 0 = A), kDiagOutputs (a DIAG pass holds b >= a, not
// only b > a), Tables (the device tables, by value), stage(lds, n_cov, meta, d, tabs), scale(I == J) and
// Lane<DIAG> with init(..) per lane and factors(..) per term pair.
// dynamic LDS: [kTables tables: n_cov + 1 each][reduction 2 * RC * T * T].  grid (tile pairs, response chunks, passes
// of this launch); DIAG: pass z holds the outputs of the dimensions [z T, z T + T); otherwise pass z is the z-th
// pair bi < bj of dimension blocks, rows [bi T, bi T + T) and columns [bj T, bj T + T); zbase: passes before it
template <typename Op, int ND, bool DIAG>
__global__ void __launch_bounds__(kSobolTW)
k_block_pairs(const uint8_t *__restrict__ lev, const int *__restrict__ meta, int p, int d, int q, int n_cov,
              const double *__restrict__ Theta, const typename Op::Tables tabs, int zbase, double *__restrict__ part) {
  constexpr int RC = Op::RC, T = Op::T, NO = T * T;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const double *tA = smem;
  double *red = smem + Op::kTables * (n_cov + 1);
  int I, J, bi, bj;
  tile_pair(blockIdx.x, (p + kSobolTW - 1) / kSobolTW, I, J);
  pass_blocks(blockIdx.z, dim_blocks(d, T), DIAG, bi, bj);
  const int i0 = bi * T, j0 = bj * T, j0r = blockIdx.y * RC;
  Op::stage(smem, n_cov, meta, d, tabs);
  const LaneTerm me = lane_term(lev, p, d, I);
  const uint8_t *lv = me.lv;
  // whether the product over the outside dimensions takes dimension l
  auto outside = [&](int l) { return l < d && (unsigned)(l - i0) >= (unsigned)T && (DIAG || (unsigned)(l - j0) >= (unsigned)T); };
  typename Op::template Lane<DIAG> ln;
  ln.init(meta, d, n_cov, lv, i0, j0);
  OutsideOffsets<ND> oo;
  pack_outside(oo, meta, d, n_cov, lv, outside);
  double th[RC], acc[RC * NO];
  load_theta(th, Theta, me, j0r, q, p);
#pragma unroll
  for (int e = 0; e < RC * NO; ++e) acc[e] = 0.0;
  const int nj = min(kSobolTW, p - J * kSobolTW);
  for (int kk = 0; kk < nj; ++kk) {
    const int k2 = J * kSobolTW + kk;                   // (wave-uniform)
    const uint8_t *lp = lev + (uint64_t)k2 * d;
    const double outp = outside_product(oo, tA, meta, d, lv, lp, outside);
    double f[NO];
    ln.factors(smem, n_cov, lp, d, i0, j0, outp, f);
#pragma unroll
    for (int r = 0; r < RC; ++r) {
      const double wv = pair_weight(th[r], Theta, j0r + r, q, p, k2);
#pragma unroll
      for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = DIAG ? a + (Op::kDiagOutputs ? 0 : 1) : 0; b < T; ++b)
          acc[r * NO + a * T + b] = fma(wv, f[a * T + b], acc[r * NO + a * T + b]);
    }
  }
  auto keep = [](int e) { return !DIAG || e % NO % T + (Op::kDiagOutputs ? 1 : 0) > e % NO / T; };
  write_pair_partials<RC * NO>(
      acc, keep, red,
      part + pair_part_index((uint64_t)zbase + blockIdx.z, gridDim.y, blockIdx.y, gridDim.x, blockIdx.x, RC * NO),
      Op::scale(I == J));
}

// block (entry o of the packed upper triangle of dimensions, with or without its diagonal; response j), one wave
// over the tile pairs: out[j * out_ld + out_off + o]
template <int T, int RC, bool WITH_DIAG>
__global__ void __launch_bounds__(64)
k_block_reduce(const double *__restrict__ part, int npairs, int nrc, int d, int out_ld, int out_off,
               double *__restrict__ out) {
  constexpr int NO = T * T;
  const int j = blockIdx.y;
  int di, dj;
  packed_pair(blockIdx.x, d, WITH_DIAG, di, dj);
  const double *base =
      part + pair_part_index(pass_of(di, dj, d, T), nrc, j / RC, npairs, 0, RC * NO) + j % RC * NO + (di % T) * T + dj % T;
  double s = 0.0;
  for (int b = threadIdx.x; b < npairs; b += 64) s += base[(uint64_t)b * RC * NO];
  s = wave_sum(s);
  if (threadIdx.x == 0) out[(uint64_t)j * out_ld + out_off + blockIdx.x] = s;
}

inline size_t block_pairs_lds(int ntab, uint64_t n_cov, int T, int RC) {
  return (ntab * (n_cov + 1) + 2 * RC * T * T) * sizeof(double);
}

// the diagonal passes, the off-diagonal passes, the reduction into d_out[j * out_ld + out_off + o]
template <typename Op>
int launch_block_pairs(const uint8_t *d_lev, const int *d_meta, uint64_t p, uint64_t d, uint64_t q, uint64_t n_cov,
                       const double *d_Theta, const typename Op::Tables &tabs, double *d_part, int out_ld, int out_off,
                       double *d_out) {
  const int nb = dim_blocks((int)d, Op::T), nrc = (int)((q + Op::RC - 1) / Op::RC);
  const int nt = (int)((p + kSobolTW - 1) / kSobolTW), npairs = nt * (nt + 1) / 2;
  const size_t lds = block_pairs_lds(Op::kTables, n_cov, Op::T, Op::RC);
  const int rc = pick_or<8, 24>(sobol2_reg_dims(d), -1, [&](auto NDc) {
    OB_TRY(ensure_dyn_lds((const void *)k_block_pairs<Op, NDc(), true>, lds));
    OB_TRY(ensure_dyn_lds((const void *)k_block_pairs<Op, NDc(), false>, lds));
    hipLaunchKernelGGL((k_block_pairs<Op, NDc(), true>), dim3(npairs, nrc, nb), dim3(kSobolTW), lds, cur_stream(), d_lev,
                       d_meta, (int)p, (int)d, (int)q, (int)n_cov, d_Theta, tabs, 0, d_part);
    if (nb > 1)
      hipLaunchKernelGGL((k_block_pairs<Op, NDc(), false>), dim3(npairs, nrc, nb * (nb - 1) / 2), dim3(kSobolTW), lds,
                         cur_stream(), d_lev, d_meta, (int)p, (int)d, (int)q, (int)n_cov, d_Theta, tabs, nb, d_part);
    return 0;
  });
  if (rc < 0) return no_kernel();
  OB_TRY(rc);
  const unsigned n_out = (unsigned)(Op::kDiagOutputs ? d * (d + 1) / 2 : d * (d - 1) / 2);
  hipLaunchKernelGGL((k_block_reduce<Op::T, Op::RC, Op::kDiagOutputs>), dim3(n_out, (unsigned)q), dim3(64), 0,
                     cur_stream(), (const double *)d_part, npairs, nrc, (int)d, out_ld, out_off, d_out);
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace obhip
