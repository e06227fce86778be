// Derivative-based sensitivity of the fitted mean: C = E[grad f grad f^T] and E[grad f] in closed form
// (sobol.cpp; include/obhip.h, "active subspaces").  No reference counterpart.
//
// k_dim_grad_moments<MODE>: k_dim_moments' block shape -- lane = node row, block = (row slice, dimension, tile of
//   8 levels or pair of such tiles).  A row's raw R_t and R'_t come from the raw twins of the derivative builders
//   (device_dx_raw.h) into two [level][thread] LDS tiles -- never into HBM.  All three tables are raw moments:
//   one pass, nothing centred.  MODE 0 sums w R'_t, w and the bad weights; MODE 1 sums w (R'_a R_b) over ALL
//   ordered pairs of level tiles (X is not symmetric); MODE 2 sums w (R'_a R'_b) over the lower triangle of tile
//   pairs, the product of the two factors first, so that (a, b) and (b, a) get the same bits, and the finish
//   mirrors it.  Sums: per thread over its rows, butterfly per wave, the waves in order, then
//   k_grad_moments_fin<MODE> over the row slices (lane-strided, butterfly): a fixed order.
// k_active_gbar: block (dimension l, response): sum_k theta_k dm_l[t_kl] prod_{i != l} m_i[t_ki], the products
//   those of k_sobol_excl (no division), a tree over the threads.
// k_active_pairs<ND, DIAG>: the p^2 part in k_sobol_pairs2's shape -- lane = term k, the partner k' wave-uniform,
//   A_l, X_l and D_l of every dimension in LDS with a neutral entry (A = 1, X = D = 0), the d x d triangle of
//   outputs cut into blocks of kActiveT dimensions over grid z, kActiveRC responses per chunk, the product of A
//   over the outside dimensions from packed row offsets, prefix and suffix products inside the blocks.  X is
//   read in both orientations per term pair: forward X_a[t,t'] at off_a + t L_a + t' and backward X_a[t',t] at
//   off_a + t' L_a + t (a lane part and a wave-uniform part either way).  Exchanging k and k' maps the summand
//   of C_lm onto that of C_ml, so over the upper triangle of term-tile pairs a pair (k, k') adds BOTH
//   orientations, f_ab = Rf_a Sb_b + Rb_a Sf_b, with weight 1; a diagonal tile pair runs over all its ordered
//   pairs and takes 1/2, which is exact.  On the diagonal of the output triangle 2 D_a prod_{l != a} A_l rides in
//   the DIAG pass.  k_active_reduce sums the per-block partials in a fixed order.  No atomics.
#include "obhip_internal.h"
#include "device_common.h"
#include "device_dx_raw.h"
#include "sobol_device.h"

namespace obhip {

namespace {

// dynamic LDS: [interval tables kIntervalTabMax][reduction 4 * 64][values lmax * threads][derivatives lmax * threads]
template <int MODE>
__global__ void __launch_bounds__(256)
k_dim_grad_moments(const DimDesc *__restrict__ dims, const double *__restrict__ ka, const double *__restrict__ kb,
                   const double *__restrict__ kc, const double *__restrict__ rot, const double *__restrict__ tab,
                   const double *__restrict__ dtab, const double *__restrict__ x, uint64_t n, uint64_t ldx,
                   const double *__restrict__ w, uint64_t ldw, int nlt, int lmax, double *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int l = blockIdx.y, nt = blockDim.x;
  double *ltab = smem, *red = smem + kIntervalTabMax, *val = red + 4 * kMomP2 + threadIdx.x;
  double *der = val + (size_t)lmax * nt;
  DimDesc D = dims[l];
  const int L = D.ncol, dtab_off = D.tab;
  int ta = blockIdx.z, tb = 0;
  if (MODE == 1) {
    ta = blockIdx.z / nlt;
    tb = blockIdx.z % nlt;
  } else if (MODE == 2) {
    tile_pair_lower(blockIdx.z, ta, tb);
  }
  if (ta * kMomLT >= L || tb * kMomLT >= L) return;  // (block-uniform, before the first barrier)
  const double *tb_ = stage_tab(D, tab, ltab);
  constexpr int K = MODE == 0 ? kMomP1 : kMomP2;
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  for (uint64_t i = (uint64_t)blockIdx.x * nt + threadIdx.x; i < n; i += (uint64_t)gridDim.x * nt) {
    const double xv = x[(uint64_t)l * ldx + i];
    double wv = w ? w[(uint64_t)l * ldw + i] : 1.0;
    const bool bad = !(wv >= 0.0) || wv > 1.7976931348623157e308;
    if (bad) wv = 0.0;
    build_dim_raw_dx_any(D, ka, kb, kc, rot, tb_, dtab, dtab_off, xv, val, der, nt);
    if (MODE == 0) {
      if (bad) acc[kMomLT + 1] += 1.0;
      acc[kMomLT] += wv;
#pragma unroll
      for (int a = 0; a < kMomLT; ++a) {
        const int t = ta * kMomLT + a;
        if (t < L) acc[a] = fma(wv, der[(size_t)t * nt], acc[a]);
      }
    } else {
      double da[kMomLT], fb[kMomLT];
#pragma unroll
      for (int a = 0; a < kMomLT; ++a) {
        const int t = ta * kMomLT + a, u = tb * kMomLT + a;
        da[a] = t < L ? der[(size_t)t * nt] : 0.0;
        fb[a] = u < L ? (MODE == 1 ? val[(size_t)u * nt] : der[(size_t)u * nt]) : 0.0;
      }
      // w (F_a F_b): the product of the two factors first, so that D's (a, b) and (b, a) get the same bits
#pragma unroll
      for (int a = 0; a < kMomLT; ++a)
#pragma unroll
        for (int b = 0; b < kMomLT; ++b) acc[a * kMomLT + b] = fma(wv, da[a] * fb[b], acc[a * kMomLT + b]);
    }
  }
  __syncthreads();
  block_sums<K>(acc, red, part + (((uint64_t)l * gridDim.z + blockIdx.z) * gridDim.x + blockIdx.x) * K);
}

// block (dimension, level tile or pair of level tiles as k_dim_grad_moments<MODE> numbers them), one wave:
// MODE 0 the derivative means, the weight sum of the dimension and the flag; MODE 1 the cross table;
// MODE 2 the derivative products, mirrored
template <int MODE>
__global__ void __launch_bounds__(64)
k_grad_moments_fin(const DimDesc *__restrict__ dims, const double *__restrict__ part, int nblk, int nlt,
                   double *__restrict__ wsum, int *__restrict__ flag, double *__restrict__ out) {
  constexpr int K = MODE == 0 ? kMomP1 : kMomP2;
  const int l = blockIdx.x, L = dims[l].ncol;
  int ta = blockIdx.y, tb = 0;
  if (MODE == 1) {
    ta = blockIdx.y / nlt;
    tb = blockIdx.y % nlt;
  } else if (MODE == 2) {
    tile_pair_lower(blockIdx.y, ta, tb);
  }
  if (ta * kMomLT >= L || tb * kMomLT >= L) return;
  const double *base = part + ((uint64_t)l * gridDim.y + blockIdx.y) * nblk * K;
  if (MODE == 0) {
    const double W = slices_sum<K>(base, nblk, kMomLT), bad = slices_sum<K>(base, nblk, kMomLT + 1);
    if (ta == 0 && threadIdx.x == 0) {
      wsum[l] = W;
      if (bad > 0.0 || !(W > 0.0) || W > 1.7976931348623157e308) flag[0] = 1;
    }
    const int om = mean_offset(dims, l);
    for (int a = 0; a < kMomLT; ++a) {
      const double s = slices_sum<K>(base, nblk, a);
      const int t = ta * kMomLT + a;
      if (t < L && threadIdx.x == 0) out[om + t] = s / W;
    }
  } else {
    const double W = wsum[l];
    const int oc = cov_offset(dims, l);
    for (int k = 0; k < K; ++k) {
      const int ia = ta * kMomLT + k / kMomLT, ib = tb * kMomLT + k % kMomLT;
      if (ia >= L || ib >= L || (MODE == 2 && ib > ia)) continue;  // (wave-uniform)
      const double s = slices_sum<K>(base, nblk, k);
      if (threadIdx.x == 0) {
        const double c = s / W;
        out[oc + ia * L + ib] = c;
        if (MODE == 2) out[oc + ib * L + ia] = c;
      }
    }
  }
}

// block (dimension l, response j).  dynamic LDS: none; static tree of 256
__global__ void __launch_bounds__(256)
k_active_gbar(const uint8_t *__restrict__ lev, const int *__restrict__ meta, int p, int d, int nout,
              const double *__restrict__ Theta, const double *__restrict__ dmtab, const double *__restrict__ excl,
              double *__restrict__ out) {
  __shared__ double red[256];
  const int l = blockIdx.x, j = blockIdx.y, om = meta[d + l];
  const double *th = Theta + (uint64_t)j * p;
  double s = 0.0;
  for (int k = threadIdx.x; k < p; k += 256)
    s = fma(th[k] * dmtab[om + lev[(uint64_t)k * d + l]], excl[(uint64_t)k * d + l], s);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[(uint64_t)j * nout + l] = red[0];
}

// dynamic LDS: [A: n_cov + 1][X: n_cov + 1][D: n_cov + 1][reduction 2 * RC * T * T]; entry n_cov of the tables is
// the factor of a dimension beyond d or one that a pass leaves out (A = 1, X = D = 0).  grid (tile pairs, response
// chunks, passes); DIAG: pass z holds the outputs (a, b), a <= b, of the dimensions [z T, z T + T); otherwise pass
// z is the z-th pair bi < bj of dimension blocks, rows [bi T, bi T + T) and columns [bj T, bj T + T).
// part[(((zbase + z) * nrc + rc) * npairs + pair) * RC * T * T + r * T * T + a * T + b]
template <int ND, bool DIAG>
__global__ void __launch_bounds__(kSobolTW)
k_active_pairs(const uint8_t *__restrict__ lev, const int *__restrict__ meta, int p, int d, int q, int n_cov,
               const double *__restrict__ Theta, const double *__restrict__ mtab, const double *__restrict__ ctab,
               const double *__restrict__ xtab, const double *__restrict__ dtab, int zbase,
               double *__restrict__ part) {
  constexpr int RC = kActiveRC, T = kActiveT, NO = T * T;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *tA = smem, *tX = tA + n_cov + 1, *tD = tX + n_cov + 1, *red = tD + n_cov + 1;
  int I, J;
  const int ntile = (p + kSobolTW - 1) / kSobolTW;
  tile_pair(blockIdx.x, ntile, I, J);
  // the blocks of dimensions of this pass
  int bi = blockIdx.z, bj = blockIdx.z;
  if (!DIAG) {
    const int nb = (d + T - 1) / T;
    int zz = blockIdx.z;
    bi = 0;
    while (zz >= nb - 1 - bi) {
      zz -= nb - 1 - bi;
      ++bi;
    }
    bj = bi + 1 + zz;
  }
  const int i0 = bi * T, j0 = bj * T, j0r = blockIdx.y * RC;
  for (int l = 0; l < d; ++l) {
    const int L = meta[l], om = meta[d + l], oc = meta[2 * d + l];
    for (int e = threadIdx.x; e < L * L; e += kSobolTW) {
      tA[oc + e] = ctab[oc + e] + mtab[om + e / L] * mtab[om + e % L];
      tX[oc + e] = xtab[oc + e];
      tD[oc + e] = dtab[oc + e];
    }
  }
  if (threadIdx.x == 0) {
    tA[n_cov] = 1.0;
    tX[n_cov] = 0.0;
    tD[n_cov] = 0.0;
  }
  __syncthreads();
  const int k = I * kSobolTW + threadIdx.x;
  const bool valid = k < p;
  const uint8_t *lv = lev + (uint64_t)(valid ? k : p - 1) * d;  // (a lane beyond p: any term, its coefficient is 0)
  // whether the product over the outside dimensions takes dimension l
  auto outside = [&](int l) { return l < d && (unsigned)(l - i0) >= (unsigned)T && (DIAG || (unsigned)(l - j0) >= (unsigned)T); };
  // per dimension of the two blocks: the forward offset off + t L (to which t' is added), the backward one
  // off + t (to which t' L is added) and L itself (wave-uniform; 0 for a dimension beyond d)
  int rf[T], rb[T], rL[T], cf[T], cb[T], cL[T];
#pragma unroll
  for (int a = 0; a < T; ++a) {
    const int li = i0 + a, lj = j0 + a;
    const bool ri = li < d, ci = !DIAG && lj < d;
    const int lic = min(li, d - 1), ljc = min(lj, d - 1);
    rL[a] = ri ? meta[lic] : 0;
    rf[a] = ri ? meta[2 * d + lic] + (int)lv[lic] * meta[lic] : n_cov;
    rb[a] = ri ? meta[2 * d + lic] + (int)lv[lic] : n_cov;
    cL[a] = ci ? meta[ljc] : 0;
    cf[a] = ci ? meta[2 * d + ljc] + (int)lv[ljc] * meta[ljc] : n_cov;
    cb[a] = ci ? meta[2 * d + ljc] + (int)lv[ljc] : n_cov;
  }
  unsigned offp[ND / 2], umask = 0;                      // row offsets of the first ND dimensions, two to a word
#pragma unroll
  for (int h = 0; h < ND / 2; ++h) {
    unsigned wd = 0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int l = 2 * h + e;
      const bool use = outside(l);
      const int lc = min(l, d - 1);
      wd |= (unsigned)(use ? meta[2 * d + lc] + (int)lv[lc] * meta[lc] : n_cov) << (16 * e);
      umask |= (use ? 1u : 0u) << l;
    }
    offp[h] = wd;
  }
  double th[RC], acc[RC][NO];
#pragma unroll
  for (int r = 0; r < RC; ++r) {
    th[r] = valid && j0r + r < q ? Theta[(uint64_t)(j0r + r) * p + k] : 0.0;
#pragma unroll
    for (int e = 0; e < NO; ++e) acc[r][e] = 0.0;
  }
  const int nj = min(kSobolTW, p - J * kSobolTW);
  for (int kk = 0; kk < nj; ++kk) {
    const int k2 = J * kSobolTW + kk;                   // (wave-uniform)
    const uint8_t *lp = lev + (uint64_t)k2 * d;
    // the outside product, even and odd dimensions apart (two shorter chains), then the dimensions beyond ND
    double pe = 1.0, po = 1.0;
#pragma unroll
    for (int l = 0; l < ND; ++l) {
      const int off = (int)((offp[l / 2] >> (16 * (l & 1))) & 0xffffu);
      const int add = (umask >> l) & 1u ? (int)lp[min(l, d - 1)] : 0;
      if (l & 1) po *= tA[off + add];
      else pe *= tA[off + add];
    }
    for (int l = ND; l < d; ++l)                         // (d > ND only)
      if (outside(l)) pe *= tA[meta[2 * d + l] + (int)lv[l] * meta[l] + lp[l]];
    const double outp = pe * po;
    double ar[T], xf[T], xb[T], dr[T], f[NO];
#pragma unroll
    for (int a = 0; a < T; ++a) {
      const int tp = i0 + a < d ? (int)lp[min(i0 + a, d - 1)] : 0;
      ar[a] = tA[rf[a] + tp];
      xf[a] = tX[rf[a] + tp];                            // X_a[t, t']
      xb[a] = tX[rb[a] + tp * rL[a]];                    // X_a[t', t]
      if (DIAG) dr[a] = tD[rf[a] + tp];
    }
    if (DIAG) {
      double Sf[T], Sb[T], sufA[T], suf = 1.0;
#pragma unroll
      for (int b = T - 1; b >= 0; --b) {
        sufA[b] = suf;                                   // prod_{l > b} A_l of the block
        Sf[b] = xf[b] * suf;
        Sb[b] = xb[b] * suf;
        suf *= ar[b];
      }
      double pre = outp;                                 // outside . prod_{l < a} A_l
#pragma unroll
      for (int a = 0; a < T; ++a) {
        const double dg = (pre * dr[a]) * sufA[a];
        f[a * T + a] = dg + dg;                          // both orientations of the symmetric D_a
        double mf = pre * xf[a], mb = pre * xb[a];       // . prod_{a < l < b} A_l
#pragma unroll
        for (int b = a + 1; b < T; ++b) {
          f[a * T + b] = mf * Sb[b] + mb * Sf[b];
          mf *= ar[b];
          mb *= ar[b];
        }
        pre *= ar[a];
      }
    } else {
      double Rf[T], Rb[T], Sf[T], Sb[T], ac[T], suf = 1.0, pre = outp;
#pragma unroll
      for (int a = 0; a < T; ++a) {
        Rf[a] = pre;                                     // outside . prod_{l < a} A_l of the row block
        pre *= ar[a];
      }
#pragma unroll
      for (int a = T - 1; a >= 0; --a) {
        const double P = Rf[a] * suf;                    // . prod_{l > a} A_l
        Rf[a] = P * xf[a];
        Rb[a] = P * xb[a];
        suf *= ar[a];
      }
      pre = 1.0;
#pragma unroll
      for (int b = 0; b < T; ++b) {
        const int tp = j0 + b < d ? (int)lp[min(j0 + b, d - 1)] : 0;
        ac[b] = tA[cf[b] + tp];
        Sf[b] = tX[cf[b] + tp];
        Sb[b] = tX[cb[b] + tp * cL[b]];
      }
      double Q[T];
#pragma unroll
      for (int b = 0; b < T; ++b) {
        Q[b] = pre;
        pre *= ac[b];
      }
      suf = 1.0;
#pragma unroll
      for (int b = T - 1; b >= 0; --b) {
        const double P = Q[b] * suf;                     // prod_{l != b} A_l of the column block
        Sf[b] *= P;
        Sb[b] *= P;
        suf *= ac[b];
      }
#pragma unroll
      for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = 0; b < T; ++b) f[a * T + b] = Rf[a] * Sb[b] + Rb[a] * Sf[b];
    }
#pragma unroll
    for (int r = 0; r < RC; ++r) {
      const double wv = th[r] * Theta[(uint64_t)min(j0r + r, q - 1) * p + k2];
#pragma unroll
      for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = DIAG ? a : 0; b < T; ++b) acc[r][a * T + b] = fma(wv, f[a * T + b], acc[r][a * T + b]);
    }
  }
  // the block's partials: butterfly per wave, wave 0 + wave 1.  Every pair added both orientations: an off-diagonal
  // tile pair stands as it is, a diagonal one has met every unordered pair twice
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < RC; ++r)
#pragma unroll
    for (int e = 0; e < NO; ++e) {
      const double v = !DIAG || e % T >= e / T ? wave_sum(acc[r][e]) : 0.0;
      if (lane == 0) red[wave * RC * NO + r * NO + e] = v;
    }
  __syncthreads();
  if ((int)threadIdx.x < RC * NO) {
    const double s = red[threadIdx.x] + red[RC * NO + threadIdx.x];
    part[((((uint64_t)zbase + blockIdx.z) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * RC * NO + threadIdx.x] =
        (I == J ? 0.5 : 1.0) * s;
  }
}

// block (entry o of the packed upper triangle, response j), one wave over the tile pairs
__global__ void __launch_bounds__(64)
k_active_reduce(const double *__restrict__ part, int npairs, int nrc, int d, int nout, double *__restrict__ out) {
  constexpr int T = kActiveT, NO = T * T;
  const int j = blockIdx.y;
  int di = 0, dj = blockIdx.x;                           // row-major with the diagonal: (0,0), (0,1), .. (1,1), ..
  while (dj >= d - di) {
    dj -= d - di;
    ++di;
  }
  dj += di;
  const int nb = (d + T - 1) / T, bi = di / T, bj = dj / T;
  const int zc = bi == bj ? bi : nb + bi * (nb - 1) - bi * (bi - 1) / 2 + (bj - bi - 1);
  const int rc = j / kActiveRC, r = j % kActiveRC;
  const double *base = part + ((uint64_t)zc * nrc + rc) * npairs * kActiveRC * NO + r * NO + (di % T) * T + dj % T;
  double s = 0.0;
  for (int b = threadIdx.x; b < npairs; b += 64) s += base[(uint64_t)b * kActiveRC * NO];
  s = wave_sum(s);
  if (threadIdx.x == 0) out[(uint64_t)j * nout + d + blockIdx.x] = s;
}

}  // namespace

int active_moment_threads(uint64_t lmax) { return lmax <= 16 ? 256 : 64; }
size_t active_moments_lds(uint64_t lmax) {
  return (kIntervalTabMax + 4 * kMomP2 + 2 * lmax * active_moment_threads(lmax)) * sizeof(double);
}

size_t active_pairs_lds(uint64_t n_cov) {
  return (3 * (n_cov + 1) + 2 * kActiveRC * kActiveT * kActiveT) * sizeof(double);
}

uint64_t active_part_doubles(uint64_t p, uint64_t d, uint64_t q) {
  const uint64_t nb = (d + kActiveT - 1) / kActiveT, nz = nb + nb * (nb - 1) / 2;
  const uint64_t nrc = (q + kActiveRC - 1) / kActiveRC, nt = (p + kSobolTW - 1) / kSobolTW;
  return nz * nrc * (nt * (nt + 1) / 2) * kActiveRC * kActiveT * kActiveT;
}

int launch_dim_grad_moments(const obhip_model &m, obhip_terms &t, const double *d_nodes, uint64_t n, uint64_t ldx,
                            const double *d_w, uint64_t ldw, double *d_dmean, double *d_cross, double *d_dd,
                            int *flag_out) {
  OB_TRY(prepare_predict(m, t, true));
  const ModelDev &md = t.pred_md;
  const uint64_t d = m.d;
  uint64_t lmax = 1;
  for (uint64_t l = 0; l < d; ++l) lmax = std::max<uint64_t>(lmax, t.maxlev[l] + 1);
  const int nth = active_moment_threads(lmax);
  const size_t lds = active_moments_lds(lmax);
  const int nblk = (int)std::min<uint64_t>(kMomBlocks, (n + nth - 1) / nth);
  const int nlt = (int)((lmax + kMomLT - 1) / kMomLT), nt2 = nlt * (nlt + 1) / 2, ntx = nlt * nlt;
  DevBuf<double> part, wsum;
  DevBuf<int> flag;
  OB_TRY(part.alloc(d * nblk * std::max<uint64_t>((uint64_t)nlt * kMomP1, (uint64_t)ntx * kMomP2)));
  OB_TRY(wsum.alloc(d));
  OB_TRY(flag.alloc(1));
  OB_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), cur_stream()));
  OB_TRY(ensure_dyn_lds((const void *)k_dim_grad_moments<0>, lds));
  OB_TRY(ensure_dyn_lds((const void *)k_dim_grad_moments<1>, lds));
  OB_TRY(ensure_dyn_lds((const void *)k_dim_grad_moments<2>, lds));
  {
    ProfScope ps("dim_grad_moments");
    const double *dtab = t.dx.dtab.p;
    hipLaunchKernelGGL(k_dim_grad_moments<0>, dim3(nblk, (unsigned)d, nlt), dim3(nth), lds, cur_stream(), md.dims.p,
                       md.ka.p, md.kb.p, md.kc.p, md.rot.p, md.tab.p, dtab, d_nodes, n, ldx, d_w, ldw, nlt, (int)lmax,
                       part.p);
    hipLaunchKernelGGL(k_grad_moments_fin<0>, dim3((unsigned)d, nlt), dim3(64), 0, cur_stream(), md.dims.p,
                       (const double *)part.p, nblk, nlt, wsum.p, flag.p, d_dmean);
    hipLaunchKernelGGL(k_dim_grad_moments<1>, dim3(nblk, (unsigned)d, ntx), dim3(nth), lds, cur_stream(), md.dims.p,
                       md.ka.p, md.kb.p, md.kc.p, md.rot.p, md.tab.p, dtab, d_nodes, n, ldx, d_w, ldw, nlt, (int)lmax,
                       part.p);
    hipLaunchKernelGGL(k_grad_moments_fin<1>, dim3((unsigned)d, ntx), dim3(64), 0, cur_stream(), md.dims.p,
                       (const double *)part.p, nblk, nlt, wsum.p, flag.p, d_cross);
    hipLaunchKernelGGL(k_dim_grad_moments<2>, dim3(nblk, (unsigned)d, nt2), dim3(nth), lds, cur_stream(), md.dims.p,
                       md.ka.p, md.kb.p, md.kc.p, md.rot.p, md.tab.p, dtab, d_nodes, n, ldx, d_w, ldw, nlt, (int)lmax,
                       part.p);
    hipLaunchKernelGGL(k_grad_moments_fin<2>, dim3((unsigned)d, nt2), dim3(64), 0, cur_stream(), md.dims.p,
                       (const double *)part.p, nblk, nlt, wsum.p, flag.p, d_dd);
    OB_HIP(hipGetLastError());
  }
  return d2h(flag_out, flag.p, sizeof(int));  // (waits: the scratch above is released behind it)
}

int launch_active(const uint8_t *d_lev, const int *d_meta, uint64_t p, uint64_t d, uint64_t q, uint64_t n_cov,
                  const double *d_Theta, const double *d_mtab, const double *d_ctab, const double *d_dmtab,
                  const double *d_xtab, const double *d_ddtab, double *d_excl, double *d_u, double *d_part,
                  double *d_out) {
  const int nout = (int)(d + d * (d + 1) / 2);
  OB_TRY(launch_sobol_excl(d_lev, d_meta, p, d, d_mtab, d_excl, d_u));
  const int nb = (int)((d + kActiveT - 1) / kActiveT), nrc = (int)((q + kActiveRC - 1) / kActiveRC);
  const int nt = (int)((p + kSobolTW - 1) / kSobolTW), npairs = nt * (nt + 1) / 2;
  const size_t lds = active_pairs_lds(n_cov);
  ProfScope ps("active_pairs");
  hipLaunchKernelGGL(k_active_gbar, dim3((unsigned)d, (unsigned)q), dim3(256), 0, cur_stream(), d_lev, d_meta, (int)p,
                     (int)d, nout, d_Theta, d_dmtab, (const double *)d_excl, d_out);
  const int rc = pick_or<8, 24>(sobol2_reg_dims(d), -1, [&](auto NDc) {
    OB_TRY(ensure_dyn_lds((const void *)k_active_pairs<NDc(), true>, lds));
    OB_TRY(ensure_dyn_lds((const void *)k_active_pairs<NDc(), false>, lds));
    hipLaunchKernelGGL((k_active_pairs<NDc(), true>), dim3(npairs, nrc, nb), dim3(kSobolTW), lds, cur_stream(), d_lev,
                       d_meta, (int)p, (int)d, (int)q, (int)n_cov, d_Theta, d_mtab, d_ctab, d_xtab, d_ddtab, 0, d_part);
    if (nb > 1)
      hipLaunchKernelGGL((k_active_pairs<NDc(), false>), dim3(npairs, nrc, nb * (nb - 1) / 2), dim3(kSobolTW), lds,
                         cur_stream(), d_lev, d_meta, (int)p, (int)d, (int)q, (int)n_cov, d_Theta, d_mtab, d_ctab,
                         d_xtab, d_ddtab, nb, d_part);
    return 0;
  });
  if (rc < 0) return no_kernel();
  OB_TRY(rc);
  hipLaunchKernelGGL(k_active_reduce, dim3((unsigned)(d * (d + 1) / 2), (unsigned)q), dim3(64), 0, cur_stream(),
                     (const double *)d_part, npairs, nrc, (int)d, nout, d_out);
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace obhip
