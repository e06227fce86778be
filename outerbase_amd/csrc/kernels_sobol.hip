// Variance-based sensitivity of the fitted mean (sobol.cpp; include/obhip.h, "variance-based
// sensitivity").  No reference counterpart.
//
// k_dim_moments<PASS>: lane = node row, block = (row slice, dimension, tile of 8 levels or pair of
//   such tiles).  A row's raw psi_{l,t} come from the library's own builder (build_dim_any: interval
//   tables staged in LDS where the model has them, the knot loop otherwise), level 0 returned and
//   the normalised levels multiplied by it again, into a [level][thread] LDS tile -- never into HBM.
//   PASS 1 sums w psi_t, w and the bad weights; PASS 2 sums w (psi_t - m_t)(psi_t' - m_t') with the
//   means of pass 1.  Rows >= n are never read.  Sums: per thread over its rows, butterfly per wave,
//   the waves in order, then k_moments_fin* over the blocks (lane-strided, butterfly): a fixed order.
// k_sobol_excl / k_sobol_first: prod_{i != l} m_i[t_ki] by suffix and prefix products (no
//   division), then one block per (dimension, response): g_l by one wave per level, V1_l = g^T C g.
// k_sobol_pairs<DC>: the p^2 part over the upper triangle of pairs of 128-term tiles.  Lane = term
//   k, its row offsets into the tables in registers; the partner k' is wave-uniform (levels and
//   coefficients by scalar loads); A_l = C_l + m_l m_l^T, C_l and m_l m_l^T of every dimension in LDS.
//   Per pair: suffix products of A, then one forward sweep gives the DC factors
//   C_l prod_{i != l} A_i and, by D_l = C_l prod_{i<l} A_i + (m m)_l D_{l-1}, the telescoped
//   prod A - prod m m; they are formed once per pair and used for the kSobolRC responses of the chunk.
//   k_sobol_reduce sums the per-block partials in a fixed order.
// Pairs of dimensions:
// k_sobol2_second: block (pair i < j, response).  theta_k prod_{l != i,j} m_l[t_kl] is multiplied out per term
//   (no division) and staged in LDS with the term's cell t_ki L_j + t_kj; the thread that owns a cell of
//   G_ij adds the staged terms of that cell in term order.  Then V2_ij = sum_{t,s} (C_i G)[t,s] (G C_j)[t,s],
//   the two products summed over ascending t' / s', the cells per thread in order, a tree over the threads.
// k_sobol_pairs2<ND, DIAG>: the p^2 part, VT2_ij, in k_sobol_pairs' shape.  The d x d triangle of outputs is
//   cut into blocks of kSobol2T dimensions (grid z); a pass holds T x T outputs for kSobolRC responses.
//   Per term pair: the product of A over the dimensions outside the pass's two blocks (row offsets of the
//   first ND dimensions packed in registers, two to a word), then inside the blocks
//   C_a prod_{l != a} A_l by prefix and suffix products; off the diagonal an output is one product of a row
//   and a column factor, on it (i and j in one block) a running middle product prod_{i<l<j} A_l.
//   k_sobol2_reduce sums the per-block partials in a fixed order.
// k_interaction_effect: thread = grid point (a, b): psi_i(z_a) and psi_j(z'_b) into two LDS tiles, then the
//   L_i x L_j contraction with G_ij of every response.
#include "obhip_internal.h"
#include "device_common.h"
#include "sobol_device.h"

namespace obhip {

namespace {

struct StoreCol {
  double *col;  // tile + thread
  int ccol0, nt;
  __device__ __forceinline__ void operator()(int ccol, double v) const { col[(size_t)(ccol - ccol0 + 1) * nt] = v; }
};

// raw psi_{l,t}(xv), t < D.ncol, into col[t * nt]
__device__ __forceinline__ void eval_raw(const DimDesc &D, const double *ka, const double *kb, const double *kc,
                                         const double *rot, const double *tab, double xv, double *col, int nt) {
  const StoreCol st{col, D.ccol0, nt};
  const double c0 = build_dim_any(D, ka, kb, kc, rot, tab, xv, st);
  col[0] = c0;
  for (int t = 1; t < D.ncol; ++t) col[(size_t)t * nt] *= c0;
}

// dynamic LDS: [interval tables kIntervalTabMax][reduction 4 * 64][tile lmax * threads]
template <int PASS>
__global__ void __launch_bounds__(256)
k_dim_moments(const DimDesc *__restrict__ dims, const double *__restrict__ ka, const double *__restrict__ kb,
              const double *__restrict__ kc, const double *__restrict__ rot, const double *__restrict__ tab,
              const double *__restrict__ x, uint64_t n, uint64_t ldx, const double *__restrict__ w, uint64_t ldw,
              int nlt, const double *__restrict__ mean, double *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *ltab = smem, *red = smem + kIntervalTabMax, *tile = red + 4 * kMomP2;
  const int l = blockIdx.y, nt = blockDim.x;
  DimDesc D = dims[l];
  const int L = D.ncol;
  int ta = blockIdx.z, tb = 0;
  if (PASS == 2) {
    int z = blockIdx.z;
    ta = 0;
    while (z >= ta + 1) {
      z -= ta + 1;
      ++ta;
    }
    tb = z;
  }
  if (ta * kMomLT >= L) return;  // (block-uniform, before the first barrier)
  const double *tb_ = stage_tab(D, tab, ltab);
  double *col = tile + threadIdx.x;
  constexpr int K = PASS == 1 ? kMomP1 : kMomP2;
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  double ma[kMomLT], mb[kMomLT];
  if (PASS == 2) {
    const int om = mean_offset(dims, l);
#pragma unroll
    for (int a = 0; a < kMomLT; ++a) {
      ma[a] = ta * kMomLT + a < L ? mean[om + ta * kMomLT + a] : 0.0;
      mb[a] = tb * kMomLT + a < L ? mean[om + tb * kMomLT + a] : 0.0;
    }
  }
  for (uint64_t i = (uint64_t)blockIdx.x * nt + threadIdx.x; i < n; i += (uint64_t)gridDim.x * nt) {
    const double xv = x[(uint64_t)l * ldx + i];
    double wv = w ? w[(uint64_t)l * ldw + i] : 1.0;
    eval_raw(D, ka, kb, kc, rot, tb_, xv, col, nt);
    if (PASS == 1) {
      if (!(wv >= 0.0) || wv > 1.7976931348623157e308) {
        acc[kMomLT + 1] += 1.0;
        wv = 0.0;
      }
      acc[kMomLT] += wv;
#pragma unroll
      for (int a = 0; a < kMomLT; ++a) {
        const int t = ta * kMomLT + a;
        if (t < L) acc[a] = fma(wv, col[(size_t)t * nt], acc[a]);
      }
    } else {
      double da[kMomLT], db[kMomLT];
#pragma unroll
      for (int a = 0; a < kMomLT; ++a) {
        const int t = ta * kMomLT + a, u = tb * kMomLT + a;
        da[a] = t < L ? col[(size_t)t * nt] - ma[a] : 0.0;
        db[a] = u < L ? col[(size_t)u * nt] - mb[a] : 0.0;
      }
      // w (D_t D_t'): the product of the two deviations first, so that (t, t') and (t', t) get the same bits
#pragma unroll
      for (int a = 0; a < kMomLT; ++a)
#pragma unroll
        for (int b = 0; b < kMomLT; ++b) acc[a * kMomLT + b] = fma(wv, da[a] * db[b], acc[a * kMomLT + b]);
    }
  }
  __syncthreads();
  block_sums<K>(acc, red, part + (((uint64_t)l * gridDim.z + blockIdx.z) * gridDim.x + blockIdx.x) * K);
}

// block (dimension, level tile), one wave: the means, the weight sum of the dimension, the flag
__global__ void __launch_bounds__(64)
k_moments_fin1(const DimDesc *__restrict__ dims, const double *__restrict__ part, int nblk, int nlt,
               double *__restrict__ mean, double *__restrict__ wsum, int *__restrict__ flag) {
  const int l = blockIdx.x, tile = blockIdx.y, L = dims[l].ncol;
  if (tile * kMomLT >= L) return;
  const double *base = part + ((uint64_t)l * nlt + tile) * nblk * kMomP1;
  const double W = slices_sum<kMomP1>(base, nblk, kMomLT), bad = slices_sum<kMomP1>(base, nblk, kMomLT + 1);
  const int om = mean_offset(dims, l);
  if (tile == 0 && threadIdx.x == 0) {
    wsum[l] = W;
    if (bad > 0.0 || !(W > 0.0) || W > 1.7976931348623157e308) flag[0] = 1;
  }
  for (int a = 0; a < kMomLT; ++a) {
    const double s = slices_sum<kMomP1>(base, nblk, a);
    const int t = tile * kMomLT + a;
    if (t < L && threadIdx.x == 0) mean[om + t] = s / W;
  }
}

// block (dimension, pair of level tiles), one wave: the covariances, mirrored
__global__ void __launch_bounds__(64)
k_moments_fin2(const DimDesc *__restrict__ dims, const double *__restrict__ part, int nblk, int nt2,
               const double *__restrict__ wsum, double *__restrict__ cov) {
  const int l = blockIdx.x, L = dims[l].ncol;
  int z = blockIdx.y, ta = 0;
  while (z >= ta + 1) {
    z -= ta + 1;
    ++ta;
  }
  const int tb = z;
  if (ta * kMomLT >= L) return;
  const double *base = part + ((uint64_t)l * nt2 + blockIdx.y) * nblk * kMomP2;
  const double W = wsum[l];
  const int oc = cov_offset(dims, l);
  for (int k = 0; k < kMomP2; ++k) {
    const int ia = ta * kMomLT + k / kMomLT, ib = tb * kMomLT + k % kMomLT;
    if (ia >= L || ib > ia) continue;  // (wave-uniform)
    const double s = slices_sum<kMomP2>(base, nblk, k);
    if (threadIdx.x == 0) {
      const double c = s / W;
      cov[oc + ia * L + ib] = c;
      cov[oc + ib * L + ia] = c;
    }
  }
}

// dynamic LDS as k_dim_moments; thread = grid point
__global__ void __launch_bounds__(256)
k_main_effect(const DimDesc *__restrict__ dims, const double *__restrict__ ka, const double *__restrict__ kb,
              const double *__restrict__ kc, const double *__restrict__ rot, const double *__restrict__ tab, int l,
              const double *__restrict__ g, int sum_l, int q, const double *__restrict__ grid, uint64_t G,
              double *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *ltab = smem, *tile = smem + kIntervalTabMax + 4 * kMomP2;
  DimDesc D = dims[l];
  const int L = D.ncol, nt = blockDim.x, om = mean_offset(dims, l);
  const double *tb_ = stage_tab(D, tab, ltab);
  const uint64_t i = (uint64_t)blockIdx.x * nt + threadIdx.x;
  if (i >= G) return;
  double *col = tile + threadIdx.x;
  eval_raw(D, ka, kb, kc, rot, tb_, grid[i], col, nt);
  for (int j = 0; j < q; ++j) {
    const double *gj = g + (uint64_t)j * sum_l + om;
    double s = 0.0;
    for (int t = 0; t < L; ++t) s = fma(gj[t], col[(size_t)t * nt], s);
    out[(uint64_t)j * G + i] = s;
  }
}

// thread = term: excl[k][l] = prod_{i != l} m_i[t_ki] (suffix products written first, then multiplied
// by the running prefix), u[k] = the whole product
__global__ void __launch_bounds__(256)
k_sobol_excl(const uint8_t *__restrict__ lev, const int *__restrict__ meta, int p, int d,
             const double *__restrict__ mtab, double *__restrict__ excl, double *__restrict__ u) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= p) return;
  const uint8_t *lv = lev + (uint64_t)k * d;
  double *e = excl + (uint64_t)k * d;
  double s = 1.0;
  for (int l = d - 1; l >= 0; --l) {
    e[l] = s;
    s *= mtab[meta[d + l] + lv[l]];
  }
  double pre = 1.0;
  for (int l = 0; l < d; ++l) {
    e[l] *= pre;
    pre *= mtab[meta[d + l] + lv[l]];
  }
  u[k] = pre;
}

// block (dimension l or, at l = d, the mean; response j).  dynamic LDS: [g: lmax][tree: 256]
__global__ void __launch_bounds__(256)
k_sobol_first(const uint8_t *__restrict__ lev, const int *__restrict__ meta, int p, int d, int sum_l,
              const double *__restrict__ Theta, const double *__restrict__ ctab, const double *__restrict__ excl,
              const double *__restrict__ u, int lmax, double *__restrict__ out, double *__restrict__ g_out) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *gs = smem, *red = smem + lmax;
  const int l = blockIdx.x, j = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double *th = Theta + (uint64_t)j * p;
  double *o = out + (uint64_t)j * (2 + 2 * d);
  if (l == d) {
    double s = 0.0;
    for (int k = threadIdx.x; k < p; k += 256) s = fma(th[k], u[k], s);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
      if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0) o[0] = red[0];
    return;
  }
  const int L = meta[l], om = meta[d + l], oc = meta[2 * d + l];
  for (int t = wave; t < L; t += 4) {
    double s = 0.0;
    for (int k = lane; k < p; k += 64)
      if (lev[(uint64_t)k * d + l] == t) s = fma(th[k], excl[(uint64_t)k * d + l], s);
    s = wave_sum(s);
    if (lane == 0) {
      gs[t] = s;
      if (g_out) g_out[(uint64_t)j * sum_l + om + t] = s;
    }
  }
  __syncthreads();
  if (wave == 0) {
    double s = 0.0;
    for (int e = lane; e < L * L; e += 64) s = fma(gs[e / L] * ctab[oc + e], gs[e % L], s);
    s = wave_sum(s);
    if (lane == 0) o[2 + l] = s;
  }
}

// dynamic LDS: [A: n_cov + 1][C: n_cov + 1][m m^T: n_cov + 1][reduction 2 * RC * (DC + 1)]; entry n_cov of the
// tables is the factor of a dimension beyond d (A = 1, C = 0, m m = 1).  grid (tile pairs, response chunks,
// dimension chunks); part[((zc * nrc + rc) * npairs + pair) * RC * (DC + 1) + r * (DC + 1) + jj], jj = DC: V
template <int DC>
__global__ void __launch_bounds__(kSobolTW)
k_sobol_pairs(const uint8_t *__restrict__ lev, const int *__restrict__ meta, int p, int d, int q, int n_cov,
              const double *__restrict__ Theta, const double *__restrict__ mtab, const double *__restrict__ ctab,
              double *__restrict__ part) {
  constexpr int RC = kSobolRC, NF = DC + 1;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *tA = smem, *tC = tA + n_cov + 1, *tM = tC + n_cov + 1, *red = tM + n_cov + 1;
  // the tile pair (I <= J) of this block
  int I = 0, z = blockIdx.x;
  const int ntile = (p + kSobolTW - 1) / kSobolTW;
  while (z >= ntile - I) {
    z -= ntile - I;
    ++I;
  }
  const int J = I + z;
  const int j0 = blockIdx.y * RC, c0 = blockIdx.z * DC;
  for (int l = 0; l < d; ++l) {
    const int L = meta[l], om = meta[d + l], oc = meta[2 * d + l];
    for (int e = threadIdx.x; e < L * L; e += kSobolTW) {
      const double c = ctab[oc + e], mm = mtab[om + e / L] * mtab[om + e % L];
      tC[oc + e] = c;
      tM[oc + e] = mm;
      tA[oc + e] = c + mm;
    }
  }
  if (threadIdx.x == 0) {
    tA[n_cov] = 1.0;
    tC[n_cov] = 0.0;
    tM[n_cov] = 1.0;
  }
  __syncthreads();
  const int k = I * kSobolTW + threadIdx.x;
  const bool valid = k < p;
  const uint8_t *lv = lev + (uint64_t)(valid ? k : p - 1) * d;  // (a lane beyond p: any term, its coefficient is 0)
  int rowb[DC];
#pragma unroll
  for (int jj = 0; jj < DC; ++jj) {
    const int l = c0 + jj;
    rowb[jj] = l < d ? meta[2 * d + l] + (int)lv[l] * meta[l] : n_cov;
  }
  double th[RC], acc[RC][NF];
#pragma unroll
  for (int r = 0; r < RC; ++r) {
    th[r] = valid && j0 + r < q ? Theta[(uint64_t)(j0 + r) * p + k] : 0.0;
#pragma unroll
    for (int jj = 0; jj < NF; ++jj) acc[r][jj] = 0.0;
  }
  const int nj = min(kSobolTW, p - J * kSobolTW);
  for (int kk = 0; kk < nj; ++kk) {
    const int k2 = J * kSobolTW + kk;                   // (wave-uniform)
    const uint8_t *lp = lev + (uint64_t)k2 * d;
    double pa = 1.0, dd = 0.0, sufa = 1.0;
    for (int i = 0; i < c0; ++i) {                       // dimensions before the chunk (d > DC only)
      const int idx = meta[2 * d + i] + (int)lv[i] * meta[i] + lp[i];
      dd = fma(tM[idx], dd, pa * tC[idx]);
      pa *= tA[idx];
    }
    for (int i = c0 + DC; i < d; ++i)                    // and behind it
      sufa *= tA[meta[2 * d + i] + (int)lv[i] * meta[i] + lp[i]];
    int idx[DC];
    double f[DC];
#pragma unroll
    for (int jj = 0; jj < DC; ++jj) idx[jj] = rowb[jj] + (c0 + jj < d ? (int)lp[c0 + jj] : 0);
    f[DC - 1] = sufa;
#pragma unroll
    for (int jj = DC - 1; jj >= 1; --jj) f[jj - 1] = f[jj] * tA[idx[jj]];
#pragma unroll
    for (int jj = 0; jj < DC; ++jj) {
      const double pc = pa * tC[idx[jj]];
      f[jj] *= pc;                                       // C_l prod_{i != l} A_i
      dd = fma(tM[idx[jj]], dd, pc);                     // prod A - prod m m up to l
      pa *= tA[idx[jj]];
    }
#pragma unroll
    for (int r = 0; r < RC; ++r) {
      const double wv = th[r] * Theta[(uint64_t)min(j0 + r, q - 1) * p + k2];
#pragma unroll
      for (int jj = 0; jj < DC; ++jj) acc[r][jj] = fma(wv, f[jj], acc[r][jj]);
      acc[r][DC] = fma(wv, dd, acc[r][DC]);
    }
  }
  // the block's partials: butterfly per wave, wave 0 + wave 1; an off-diagonal tile pair stands for its mirror too
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < RC; ++r)
#pragma unroll
    for (int jj = 0; jj < NF; ++jj) {
      const double v = wave_sum(acc[r][jj]);
      if (lane == 0) red[wave * RC * NF + r * NF + jj] = v;
    }
  __syncthreads();
  if ((int)threadIdx.x < RC * NF) {
    const double s = red[threadIdx.x] + red[RC * NF + threadIdx.x];
    part[(((uint64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * RC * NF + threadIdx.x] =
        (I == J ? 1.0 : 2.0) * s;
  }
}

// block (output o: VT_o for o < d, V at o = d; response j), one wave over the tile pairs
__global__ void __launch_bounds__(64)
k_sobol_reduce(const double *__restrict__ part, int npairs, int nrc, int ndc, int dc, int d, double *__restrict__ out) {
  const int o = blockIdx.x, j = blockIdx.y, nf = dc + 1;
  const int zc = o < d ? o / dc : ndc - 1, jj = o < d ? o % dc : dc;
  const int rc = j / kSobolRC, r = j % kSobolRC;
  const double *base = part + ((uint64_t)zc * nrc + rc) * npairs * kSobolRC * nf + r * nf + jj;
  double s = 0.0;
  for (int b = threadIdx.x; b < npairs; b += 64) s += base[(uint64_t)b * kSobolRC * nf];
  s = wave_sum(s);
  if (threadIdx.x == 0) out[(uint64_t)j * (2 + 2 * d) + (o < d ? 2 + d + o : 1)] = s;
}

// ---- pairs of dimensions ---------------------------------------------------------------------------------
constexpr int kS2Stage = 1024;  // terms staged per round of k_sobol2_second

// block (pair o of dimensions, response).  dynamic LDS: [G: gmax][values: kS2Stage][tree: 256][cells: kS2Stage ints]
__global__ void __launch_bounds__(256)
k_sobol2_second(const uint8_t *__restrict__ lev, const int *__restrict__ meta, const int *__restrict__ pairs, int p,
                int d, int n_pairs, uint64_t n_G, int gmax, const double *__restrict__ Theta,
                const double *__restrict__ mtab, const double *__restrict__ ctab, double *__restrict__ out,
                double *__restrict__ G_out) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *gs = smem, *sv = gs + gmax, *red = sv + kS2Stage;
  int *sc = (int *)(red + 256);
  const int o = blockIdx.x, jr = blockIdx.y;
  const int di = pairs[3 * o], dj = pairs[3 * o + 1], goff = pairs[3 * o + 2];
  const int Li = meta[di], Lj = meta[dj], nc = Li * Lj;
  const double *th = Theta + (uint64_t)jr * p;
  for (int c = threadIdx.x; c < nc; c += 256) gs[c] = 0.0;
  for (int k0 = 0; k0 < p; k0 += kS2Stage) {
    __syncthreads();
    const int ne = min(kS2Stage, p - k0);
    for (int e = threadIdx.x; e < ne; e += 256) {
      const uint8_t *lv = lev + (uint64_t)(k0 + e) * d;
      double h = th[k0 + e];
      for (int l = 0; l < d; ++l)
        if (l != di && l != dj) h *= mtab[meta[d + l] + lv[l]];
      sv[e] = h;
      sc[e] = (int)lv[di] * Lj + lv[dj];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < nc; c += 256) {
      double s = gs[c];
      for (int e = 0; e < ne; ++e)
        if (sc[e] == c) s += sv[e];
      gs[c] = s;
    }
  }
  __syncthreads();
  if (G_out)
    for (int c = threadIdx.x; c < nc; c += 256) G_out[(uint64_t)jr * n_G + goff + c] = gs[c];
  const double *Ci = ctab + meta[2 * d + di], *Cj = ctab + meta[2 * d + dj];
  double s = 0.0;
  for (int c = threadIdx.x; c < nc; c += 256) {
    const int t = c / Lj, u = c % Lj;
    double h = 0.0, g = 0.0;
    for (int t2 = 0; t2 < Li; ++t2) h = fma(Ci[t * Li + t2], gs[t2 * Lj + u], h);   // (C_i G)[t,u]
    for (int u2 = 0; u2 < Lj; ++u2) g = fma(gs[t * Lj + u2], Cj[u2 * Lj + u], g);   // (G C_j)[t,u]
    s = fma(h, g, s);
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[(uint64_t)jr * 2 * n_pairs + o] = red[0];
}

// dynamic LDS: [A: n_cov + 1][C: n_cov + 1][reduction 2 * RC * T * T]; entry n_cov of the tables is the factor of a
// dimension beyond d or one that a pass leaves out (A = 1, C = 0).  grid (tile pairs, response chunks, passes);
// DIAG: pass z holds the outputs (i, j), i < j, of the dimensions [z T, z T + T); otherwise pass z is the z-th
// pair bi < bj of dimension blocks, rows [bi T, bi T + T) and columns [bj T, bj T + T).
// part[(((zbase + z) * nrc + rc) * npairs + pair) * RC * T * T + r * T * T + a * T + b]
template <int ND, bool DIAG>
__global__ void __launch_bounds__(kSobolTW)
k_sobol_pairs2(const uint8_t *__restrict__ lev, const int *__restrict__ meta, int p, int d, int q, int n_cov,
               const double *__restrict__ Theta, const double *__restrict__ mtab, const double *__restrict__ ctab,
               int zbase, double *__restrict__ part) {
  constexpr int RC = kSobolRC, T = kSobol2T, NO = T * T;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *tA = smem, *tC = tA + n_cov + 1, *red = tC + n_cov + 1;
  // the tile pair (I <= J) of this block
  int I = 0, z = blockIdx.x;
  const int ntile = (p + kSobolTW - 1) / kSobolTW;
  while (z >= ntile - I) {
    z -= ntile - I;
    ++I;
  }
  const int J = I + z;
  // and its blocks of dimensions
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
      const double c = ctab[oc + e], mm = mtab[om + e / L] * mtab[om + e % L];
      tC[oc + e] = c;
      tA[oc + e] = c + mm;
    }
  }
  if (threadIdx.x == 0) {
    tA[n_cov] = 1.0;
    tC[n_cov] = 0.0;
  }
  __syncthreads();
  const int k = I * kSobolTW + threadIdx.x;
  const bool valid = k < p;
  const uint8_t *lv = lev + (uint64_t)(valid ? k : p - 1) * d;  // (a lane beyond p: any term, its coefficient is 0)
  // whether the product over the outside dimensions takes dimension l
  auto outside = [&](int l) { return l < d && (unsigned)(l - i0) >= (unsigned)T && (DIAG || (unsigned)(l - j0) >= (unsigned)T); };
  int ro[T], co[T];
#pragma unroll
  for (int a = 0; a < T; ++a) {
    const int li = i0 + a, lj = j0 + a;
    ro[a] = li < d ? meta[2 * d + li] + (int)lv[li] * meta[li] : n_cov;
    co[a] = !DIAG && lj < d ? meta[2 * d + lj] + (int)lv[lj] * meta[lj] : n_cov;
  }
  unsigned offp[ND / 2], umask = 0;                      // row offsets of the first ND dimensions, two to a word
#pragma unroll
  for (int h = 0; h < ND / 2; ++h) {
    unsigned w = 0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int l = 2 * h + e;
      const bool use = outside(l);
      const int lc = min(l, d - 1);
      w |= (unsigned)(use ? meta[2 * d + lc] + (int)lv[lc] * meta[lc] : n_cov) << (16 * e);
      umask |= (use ? 1u : 0u) << l;
    }
    offp[h] = w;
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
    double ar[T], cr[T], R[T], f[NO];
#pragma unroll
    for (int a = 0; a < T; ++a) {
      const int idx = ro[a] + (i0 + a < d ? (int)lp[min(i0 + a, d - 1)] : 0);
      ar[a] = tA[idx];
      cr[a] = tC[idx];
    }
    double pre = outp;
#pragma unroll
    for (int a = 0; a < T; ++a) {
      R[a] = pre * cr[a];                                // outside . prod_{l < a} A_l . C_a
      pre *= ar[a];
    }
    if (DIAG) {
      double S[T], suf = 1.0;
#pragma unroll
      for (int b = T - 1; b >= 0; --b) {
        S[b] = cr[b] * suf;                              // C_b prod_{l > b} A_l
        suf *= ar[b];
      }
#pragma unroll
      for (int a = 0; a < T; ++a) {
        double m = R[a];                                 // . prod_{a < l < b} A_l
#pragma unroll
        for (int b = a + 1; b < T; ++b) {
          f[a * T + b] = m * S[b];
          m *= ar[b];
        }
      }
    } else {
      double ac[T], cc[T], S[T], suf = 1.0;
#pragma unroll
      for (int b = 0; b < T; ++b) {
        const int idx = co[b] + (j0 + b < d ? (int)lp[min(j0 + b, d - 1)] : 0);
        ac[b] = tA[idx];
        cc[b] = tC[idx];
      }
#pragma unroll
      for (int a = T - 1; a >= 0; --a) {
        R[a] *= suf;                                     // . prod_{l > a} A_l of the row block
        suf *= ar[a];
      }
      pre = 1.0;
#pragma unroll
      for (int b = 0; b < T; ++b) {
        S[b] = pre * cc[b];
        pre *= ac[b];
      }
      suf = 1.0;
#pragma unroll
      for (int b = T - 1; b >= 0; --b) {
        S[b] *= suf;                                     // C_b prod_{l != b} A_l of the column block
        suf *= ac[b];
      }
#pragma unroll
      for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = 0; b < T; ++b) f[a * T + b] = R[a] * S[b];
    }
#pragma unroll
    for (int r = 0; r < RC; ++r) {
      const double wv = th[r] * Theta[(uint64_t)min(j0r + r, q - 1) * p + k2];
#pragma unroll
      for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = DIAG ? a + 1 : 0; b < T; ++b) acc[r][a * T + b] = fma(wv, f[a * T + b], acc[r][a * T + b]);
    }
  }
  // the block's partials: butterfly per wave, wave 0 + wave 1; an off-diagonal tile pair stands for its mirror too
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < RC; ++r)
#pragma unroll
    for (int e = 0; e < NO; ++e) {
      const double v = !DIAG || e % T > e / T ? wave_sum(acc[r][e]) : 0.0;
      if (lane == 0) red[wave * RC * NO + r * NO + e] = v;
    }
  __syncthreads();
  if ((int)threadIdx.x < RC * NO) {
    const double s = red[threadIdx.x] + red[RC * NO + threadIdx.x];
    part[((((uint64_t)zbase + blockIdx.z) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * RC * NO + threadIdx.x] =
        (I == J ? 1.0 : 2.0) * s;
  }
}

// block (pair o of dimensions, response j), one wave over the tile pairs
__global__ void __launch_bounds__(64)
k_sobol2_reduce(const double *__restrict__ part, const int *__restrict__ pairs, int npairs, int nrc, int d, int n_pairs,
                double *__restrict__ out) {
  constexpr int T = kSobol2T, NO = T * T;
  const int o = blockIdx.x, j = blockIdx.y;
  const int di = pairs[3 * o], dj = pairs[3 * o + 1];
  const int nb = (d + T - 1) / T, bi = di / T, bj = dj / T;
  const int zc = bi == bj ? bi : nb + bi * (nb - 1) - bi * (bi - 1) / 2 + (bj - bi - 1);
  const int rc = j / kSobolRC, r = j % kSobolRC;
  const double *base = part + ((uint64_t)zc * nrc + rc) * npairs * kSobolRC * NO + r * NO + (di % T) * T + dj % T;
  double s = 0.0;
  for (int b = threadIdx.x; b < npairs; b += 64) s += base[(uint64_t)b * kSobolRC * NO];
  s = wave_sum(s);
  if (threadIdx.x == 0) out[(uint64_t)j * 2 * n_pairs + n_pairs + o] = s;
}

// dynamic LDS: [interval tables kIntervalTabMax][tile of dimension di: L_i * threads][of dj: L_j * threads];
// thread = grid point e = a Gj + b, a along grid_i; di < dj are the pair's dimensions in G's order and swap says that
// grid_i belongs to dj; out[r * Gi * Gj + e]
__global__ void __launch_bounds__(256)
k_interaction_effect(const DimDesc *__restrict__ dims, const double *__restrict__ ka, const double *__restrict__ kb,
                     const double *__restrict__ kc, const double *__restrict__ rot, const double *__restrict__ tab,
                     int di, int dj, const double *__restrict__ Gij, uint64_t n_G, int q,
                     const double *__restrict__ grid_i, const double *__restrict__ grid_j, uint64_t Gj, uint64_t total,
                     int swap, double *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int nt = blockDim.x;
  DimDesc Di = dims[di], Dj = dims[dj];
  const int Li = Di.ncol, Lj = Dj.ncol;
  double *ltab = smem, *coli = smem + kIntervalTabMax + threadIdx.x, *colj = coli + (size_t)Li * nt;
  const uint64_t e = (uint64_t)blockIdx.x * nt + threadIdx.x, ec = e < total ? e : total - 1;  // (every thread evaluates:
  const double *tbi = stage_tab(Di, tab, ltab);                                               //  the barriers below)
  const double za = grid_i[ec / Gj], zb = grid_j[ec % Gj];
  eval_raw(Di, ka, kb, kc, rot, tbi, swap ? zb : za, coli, nt);
  __syncthreads();
  const double *tbj = stage_tab(Dj, tab, ltab);
  eval_raw(Dj, ka, kb, kc, rot, tbj, swap ? za : zb, colj, nt);
  if (e >= total) return;
  for (int r = 0; r < q; ++r) {
    const double *g = Gij + (uint64_t)r * n_G;
    double s = 0.0;
    for (int t = 0; t < Li; ++t) {
      double u = 0.0;
      for (int v = 0; v < Lj; ++v) u = fma(g[t * Lj + v], colj[(size_t)v * nt], u);
      s = fma(u, coli[(size_t)t * nt], s);
    }
    out[(uint64_t)r * total + e] = s;
  }
}

// threads per block and dynamic LDS of the kernels that evaluate a basis tile
inline int eval_threads(uint64_t lmax) { return lmax <= 32 ? 256 : 64; }
inline size_t eval_lds(uint64_t lmax) {
  return (kIntervalTabMax + 4 * kMomP2 + lmax * eval_threads(lmax)) * sizeof(double);
}

}  // namespace

size_t sobol_pairs_lds(uint64_t d, uint64_t n_cov) {
  return (3 * (n_cov + 1) + 2 * kSobolRC * (sobol_dim_chunk(d) + 1)) * sizeof(double);
}

uint64_t sobol_part_doubles(uint64_t p, uint64_t d, uint64_t q) {
  const uint64_t dc = sobol_dim_chunk(d), ndc = (d + dc - 1) / dc, nrc = (q + kSobolRC - 1) / kSobolRC;
  const uint64_t nt = (p + kSobolTW - 1) / kSobolTW;
  return ndc * nrc * (nt * (nt + 1) / 2) * kSobolRC * (dc + 1);
}

int launch_dim_moments(const obhip_model &m, obhip_terms &t, const double *d_nodes, uint64_t n, uint64_t ldx,
                       const double *d_w, uint64_t ldw, double *d_mean, double *d_cov, int *flag_out) {
  OB_TRY(prepare_predict(m, t, false));
  const ModelDev &md = t.pred_md;
  const uint64_t d = m.d;
  uint64_t lmax = 1;
  for (uint64_t l = 0; l < d; ++l) lmax = std::max<uint64_t>(lmax, t.maxlev[l] + 1);
  const int nth = eval_threads(lmax);
  const size_t lds = eval_lds(lmax);
  const int nblk = (int)std::min<uint64_t>(kMomBlocks, (n + nth - 1) / nth);
  const int nlt = (int)((lmax + kMomLT - 1) / kMomLT), nt2 = nlt * (nlt + 1) / 2;
  DevBuf<double> part, wsum;
  DevBuf<int> flag;
  OB_TRY(part.alloc(d * nblk * std::max<uint64_t>((uint64_t)nlt * kMomP1, (uint64_t)nt2 * kMomP2)));
  OB_TRY(wsum.alloc(d));
  OB_TRY(flag.alloc(1));
  OB_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), cur_stream()));
  OB_TRY(ensure_dyn_lds((const void *)k_dim_moments<1>, lds));
  OB_TRY(ensure_dyn_lds((const void *)k_dim_moments<2>, lds));
  {
    ProfScope ps("dim_moments");
    hipLaunchKernelGGL(k_dim_moments<1>, dim3(nblk, (unsigned)d, nlt), dim3(nth), lds, cur_stream(), md.dims.p, md.ka.p,
                       md.kb.p, md.kc.p, md.rot.p, md.tab.p, d_nodes, n, ldx, d_w, ldw, nlt, (const double *)nullptr,
                       part.p);
    hipLaunchKernelGGL(k_moments_fin1, dim3((unsigned)d, nlt), dim3(64), 0, cur_stream(), md.dims.p,
                       (const double *)part.p, nblk, nlt, d_mean, wsum.p, flag.p);
    hipLaunchKernelGGL(k_dim_moments<2>, dim3(nblk, (unsigned)d, nt2), dim3(nth), lds, cur_stream(), md.dims.p, md.ka.p,
                       md.kb.p, md.kc.p, md.rot.p, md.tab.p, d_nodes, n, ldx, d_w, ldw, nlt, (const double *)d_mean,
                       part.p);
    hipLaunchKernelGGL(k_moments_fin2, dim3((unsigned)d, nt2), dim3(64), 0, cur_stream(), md.dims.p,
                       (const double *)part.p, nblk, nt2, (const double *)wsum.p, d_cov);
    OB_HIP(hipGetLastError());
  }
  return d2h(flag_out, flag.p, sizeof(int));  // (waits: the scratch above is released behind it)
}

int launch_sobol_first(const uint8_t *d_lev, const int *d_meta, uint64_t p, uint64_t d, uint64_t q, uint64_t lmax,
                       uint64_t sum_l, const double *d_Theta, const double *d_mtab, const double *d_ctab, double *d_excl,
                       double *d_u, double *d_out, double *d_g) {
  ProfScope ps("sobol_first");
  hipLaunchKernelGGL(k_sobol_excl, dim3((unsigned)((p + 255) / 256)), dim3(256), 0, cur_stream(), d_lev, d_meta, (int)p,
                     (int)d, d_mtab, d_excl, d_u);
  hipLaunchKernelGGL(k_sobol_first, dim3((unsigned)d + 1, (unsigned)q), dim3(256), (lmax + 256) * sizeof(double),
                     cur_stream(), d_lev, d_meta, (int)p, (int)d, (int)sum_l, d_Theta, d_ctab, (const double *)d_excl,
                     (const double *)d_u, (int)lmax, d_out, d_g);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_sobol_excl(const uint8_t *d_lev, const int *d_meta, uint64_t p, uint64_t d, const double *d_mtab,
                      double *d_excl, double *d_u) {
  hipLaunchKernelGGL(k_sobol_excl, dim3((unsigned)((p + 255) / 256)), dim3(256), 0, cur_stream(), d_lev, d_meta, (int)p,
                     (int)d, d_mtab, d_excl, d_u);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_sobol_pairs(const uint8_t *d_lev, const int *d_meta, uint64_t p, uint64_t d, uint64_t q, uint64_t n_cov,
                       const double *d_Theta, const double *d_mtab, const double *d_ctab, double *d_part, double *d_out) {
  const int dc = sobol_dim_chunk(d), ndc = (int)((d + dc - 1) / dc), nrc = (int)((q + kSobolRC - 1) / kSobolRC);
  const int nt = (int)((p + kSobolTW - 1) / kSobolTW), npairs = nt * (nt + 1) / 2;
  const size_t lds = sobol_pairs_lds(d, n_cov);
  ProfScope ps("sobol_pairs");
  const int rc = pick_or<8, 24>(dc, -1, [&](auto DCc) {
    OB_TRY(ensure_dyn_lds((const void *)k_sobol_pairs<DCc()>, lds));
    hipLaunchKernelGGL(k_sobol_pairs<DCc()>, dim3(npairs, nrc, ndc), dim3(kSobolTW), lds, cur_stream(), d_lev, d_meta,
                       (int)p, (int)d, (int)q, (int)n_cov, d_Theta, d_mtab, d_ctab, d_part);
    return 0;
  });
  if (rc < 0) return no_kernel();
  OB_TRY(rc);
  hipLaunchKernelGGL(k_sobol_reduce, dim3((unsigned)d + 1, (unsigned)q), dim3(64), 0, cur_stream(),
                     (const double *)d_part, npairs, nrc, ndc, dc, (int)d, d_out);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_main_effect(const obhip_model &m, obhip_terms &t, uint64_t dim, const double *d_g, uint64_t q,
                       const double *d_grid, uint64_t G, double *d_out) {
  OB_TRY(prepare_predict(m, t, false));
  const ModelDev &md = t.pred_md;
  uint64_t lmax = 1, sum_l = 0;
  for (uint64_t l = 0; l < m.d; ++l) {
    lmax = std::max<uint64_t>(lmax, t.maxlev[l] + 1);
    sum_l += t.maxlev[l] + 1;
  }
  const int nth = eval_threads(lmax);
  const size_t lds = eval_lds(lmax);
  OB_TRY(ensure_dyn_lds((const void *)k_main_effect, lds));
  ProfScope ps("main_effect");
  hipLaunchKernelGGL(k_main_effect, dim3((unsigned)((G + nth - 1) / nth)), dim3(nth), lds, cur_stream(), md.dims.p,
                     md.ka.p, md.kb.p, md.kc.p, md.rot.p, md.tab.p, (int)dim, d_g, (int)sum_l, (int)q, d_grid, G, d_out);
  OB_HIP(hipGetLastError());
  return 0;
}

size_t sobol2_pairs_lds(uint64_t n_cov) {
  return (2 * (n_cov + 1) + 2 * kSobolRC * kSobol2T * kSobol2T) * sizeof(double);
}

uint64_t sobol2_part_doubles(uint64_t p, uint64_t d, uint64_t q) {
  const uint64_t nb = (d + kSobol2T - 1) / kSobol2T, nz = nb + nb * (nb - 1) / 2;
  const uint64_t nrc = (q + kSobolRC - 1) / kSobolRC, nt = (p + kSobolTW - 1) / kSobolTW;
  return nz * nrc * (nt * (nt + 1) / 2) * kSobolRC * kSobol2T * kSobol2T;
}

int launch_sobol2_second(const uint8_t *d_lev, const int *d_meta, const int *d_pairs, uint64_t p, uint64_t d, uint64_t q,
                         uint64_t n_pairs, uint64_t n_G, uint64_t gmax, const double *d_Theta, const double *d_mtab,
                         const double *d_ctab, double *d_out, double *d_G) {
  ProfScope ps("sobol2_second");
  const size_t lds = (gmax + kS2Stage + 256) * sizeof(double) + kS2Stage * sizeof(int);
  OB_TRY(ensure_dyn_lds((const void *)k_sobol2_second, lds));
  hipLaunchKernelGGL(k_sobol2_second, dim3((unsigned)n_pairs, (unsigned)q), dim3(256), lds, cur_stream(), d_lev, d_meta,
                     d_pairs, (int)p, (int)d, (int)n_pairs, n_G, (int)gmax, d_Theta, d_mtab, d_ctab, d_out, d_G);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_sobol2_pairs(const uint8_t *d_lev, const int *d_meta, const int *d_pairs, uint64_t p, uint64_t d, uint64_t q,
                        uint64_t n_cov, const double *d_Theta, const double *d_mtab, const double *d_ctab,
                        double *d_part, double *d_out) {
  const int nb = (int)((d + kSobol2T - 1) / kSobol2T), nrc = (int)((q + kSobolRC - 1) / kSobolRC);
  const int nt = (int)((p + kSobolTW - 1) / kSobolTW), npairs = nt * (nt + 1) / 2;
  const size_t lds = sobol2_pairs_lds(n_cov);
  ProfScope ps("sobol2_pairs");
  const int rc = pick_or<8, 24>(sobol2_reg_dims(d), -1, [&](auto NDc) {
    OB_TRY(ensure_dyn_lds((const void *)k_sobol_pairs2<NDc(), true>, lds));
    OB_TRY(ensure_dyn_lds((const void *)k_sobol_pairs2<NDc(), false>, lds));
    hipLaunchKernelGGL((k_sobol_pairs2<NDc(), true>), dim3(npairs, nrc, nb), dim3(kSobolTW), lds, cur_stream(), d_lev,
                       d_meta, (int)p, (int)d, (int)q, (int)n_cov, d_Theta, d_mtab, d_ctab, 0, d_part);
    if (nb > 1)
      hipLaunchKernelGGL((k_sobol_pairs2<NDc(), false>), dim3(npairs, nrc, nb * (nb - 1) / 2), dim3(kSobolTW), lds,
                         cur_stream(), d_lev, d_meta, (int)p, (int)d, (int)q, (int)n_cov, d_Theta, d_mtab, d_ctab, nb,
                         d_part);
    return 0;
  });
  if (rc < 0) return no_kernel();
  OB_TRY(rc);
  const uint64_t n_pairs = d * (d - 1) / 2;
  hipLaunchKernelGGL(k_sobol2_reduce, dim3((unsigned)n_pairs, (unsigned)q), dim3(64), 0, cur_stream(),
                     (const double *)d_part, d_pairs, npairs, nrc, (int)d, (int)n_pairs, d_out);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_interaction_effect(const obhip_model &m, obhip_terms &t, uint64_t di, uint64_t dj, const double *d_Gij,
                              uint64_t n_G, uint64_t q, const double *d_grid_i, uint64_t Gi, const double *d_grid_j,
                              uint64_t Gj, double *d_out) {
  OB_TRY(prepare_predict(m, t, false));
  const ModelDev &md = t.pred_md;
  const uint64_t Ls = (uint64_t)t.maxlev[di] + t.maxlev[dj] + 2, total = Gi * Gj;
  int nth = 256;  // two basis tiles: the most threads whose tiles fit
  while (nth > 32 && (kIntervalTabMax + Ls * nth) * sizeof(double) > kLdsBudget - 4096) nth /= 2;
  const size_t lds = (kIntervalTabMax + Ls * nth) * sizeof(double);
  OB_TRY(ensure_dyn_lds((const void *)k_interaction_effect, lds));
  ProfScope ps("interaction_effect");
  hipLaunchKernelGGL(k_interaction_effect, dim3((unsigned)((total + nth - 1) / nth)), dim3(nth), lds, cur_stream(),
                     md.dims.p, md.ka.p, md.kb.p, md.kc.p, md.rot.p, md.tab.p, (int)std::min(di, dj), (int)std::max(di, dj),
                     d_Gij, n_G, (int)q, d_grid_i, d_grid_j, Gj, total, di > dj ? 1 : 0, d_out);
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace obhip
