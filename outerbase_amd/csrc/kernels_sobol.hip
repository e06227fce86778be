// Variance-based sensitivity of the fitted mean (sobol.cpp; include/obhip.h, "variance-based
// sensitivity"; DESIGN.md sections 19, 23 and 33).  No reference counterpart.  The moment tables are in
// kernels_moments.hip, the frame of the term-pair sums in pair_sum.h.
//
// k_sobol_excl / k_sobol_first: prod_{i != l} m_i[t_ki] by suffix and prefix products (no
//   division), then one block per (dimension, response): g_l by one wave per level, V1_l = g^T C g.
// k_sobol_pairs<DC>: the p^2 part over the upper triangle of pairs of 128-term tiles, A_l = C_l + m_l m_l^T, C_l
//   and m_l m_l^T of every dimension in LDS.  Per pair: suffix products of A, then one forward sweep gives the DC
//   factors C_l prod_{i != l} A_i and, by D_l = C_l prod_{i<l} A_i + (m m)_l D_{l-1}, the telescoped
//   prod A - prod m m; they are formed once per pair and used for the kSobolRC responses of the chunk.
//   k_sobol_reduce sums the per-block partials in a fixed order.
// Pairs of dimensions:
// k_sobol2_second: block (pair i < j, response).  theta_k prod_{l != i,j} m_l[t_kl] is multiplied out per term
//   (no division) and staged in LDS with the term's cell t_ki L_j + t_kj; the thread that owns a cell of
//   G_ij adds the staged terms of that cell in term order.  Then V2_ij = sum_{t,s} (C_i G)[t,s] (G C_j)[t,s],
//   the two products summed over ascending t' / s', the cells per thread in order, a tree over the threads.
// Sobol2Op: VT2_ij by k_block_pairs.  Inside the pass's blocks C_a prod_{l != a} A_l by prefix and suffix
//   products; off the diagonal an output is one product of a row and a column factor, on it (i and j in one
//   block) a running middle product prod_{i<l<j} A_l.
// k_interaction_effect: thread = grid point (a, b): psi_i(z_a) and psi_j(z'_b) into two LDS tiles, then the
//   L_i x L_j contraction with G_ij of every response.
#include "obhip_internal.h"
#include "device_common.h"
#include "pair_sum.h"

namespace obhip {

namespace {

// dynamic LDS: eval_lds; thread = grid point
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
    s = block_tree_256(s, red);
    if (threadIdx.x == 0) o[0] = s;
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
  int I, J;
  tile_pair(blockIdx.x, (p + kSobolTW - 1) / kSobolTW, I, J);
  const int j0 = blockIdx.y * RC, c0 = blockIdx.z * DC;
  stage_pair_tables(
      meta, d,
      [&](int i, int ia, int ib) {
        const double c = ctab[i], mm = mtab[ia] * mtab[ib];
        tC[i] = c;
        tM[i] = mm;
        tA[i] = c + mm;
      },
      [&] {
        tA[n_cov] = 1.0;
        tC[n_cov] = 0.0;
        tM[n_cov] = 1.0;
      });
  const LaneTerm me = lane_term(lev, p, d, I);
  const uint8_t *lv = me.lv;
  int rowb[DC];
#pragma unroll
  for (int jj = 0; jj < DC; ++jj) {
    const int l = c0 + jj;
    rowb[jj] = l < d ? meta[2 * d + l] + (int)lv[l] * meta[l] : n_cov;
  }
  double th[RC], acc[RC * NF];
  load_theta(th, Theta, me, j0, q, p);
#pragma unroll
  for (int e = 0; e < RC * NF; ++e) acc[e] = 0.0;
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
      const double wv = pair_weight(th[r], Theta, j0 + r, q, p, k2);
#pragma unroll
      for (int jj = 0; jj < DC; ++jj) acc[r * NF + jj] = fma(wv, f[jj], acc[r * NF + jj]);
      acc[r * NF + DC] = fma(wv, dd, acc[r * NF + DC]);
    }
  }
  // an off-diagonal tile pair stands for its mirror too
  write_pair_partials<RC * NF>(
      acc, [](int) { return true; }, red,
      part + (((uint64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * RC * NF, I == J ? 1.0 : 2.0);
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
  s = block_tree_256(s, red);
  if (threadIdx.x == 0) out[(uint64_t)jr * 2 * n_pairs + o] = s;
}

// VT2_ij by k_block_pairs (pair_sum.h).  LDS tables: A, C; the neutral entry A = 1, C = 0.  A DIAG pass holds the
// outputs (i, j), i < j, of its block
struct Sobol2Op {
  static constexpr int T = kSobol2T, RC = kSobolRC, NO = T * T, kTables = 2;
  static constexpr bool kDiagOutputs = false;
  struct Tables {
    const double *mtab, *ctab;
  };
  // an off-diagonal tile pair stands for its mirror too
  static __device__ __forceinline__ double scale(bool diag_tiles) { return diag_tiles ? 1.0 : 2.0; }
  static __device__ __forceinline__ void stage(double *lds, int n_cov, const int *__restrict__ meta, int d,
                                               const Tables &tb) {
    double *tA = lds, *tC = tA + n_cov + 1;
    stage_pair_tables(
        meta, d,
        [&](int i, int ia, int ib) {
          const double c = tb.ctab[i], mm = tb.mtab[ia] * tb.mtab[ib];
          tC[i] = c;
          tA[i] = c + mm;
        },
        [&] {
          tA[n_cov] = 1.0;
          tC[n_cov] = 0.0;
        });
  }
  template <bool DIAG>
  struct Lane {
    int ro[T], co[T];  // row offsets of the lane's term in the dimensions of the row and of the column block
    __device__ __forceinline__ void init(const int *__restrict__ meta, int d, int n_cov, const uint8_t *lv, int i0,
                                         int j0) {
#pragma unroll
      for (int a = 0; a < T; ++a) {
        const int li = i0 + a, lj = j0 + a;
        ro[a] = li < d ? meta[2 * d + li] + (int)lv[li] * meta[li] : n_cov;
        co[a] = !DIAG && lj < d ? meta[2 * d + lj] + (int)lv[lj] * meta[lj] : n_cov;
      }
    }
    __device__ __forceinline__ void factors(const double *lds, int n_cov, const uint8_t *lp, int d, int i0, int j0,
                                            double outp, double (&f)[NO]) const {
      const double *tA = lds, *tC = tA + n_cov + 1;
      double ar[T], cr[T], R[T];
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
    }
  };
};

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

}  // namespace

size_t sobol_pairs_lds(uint64_t d, uint64_t n_cov) {
  return (3 * (n_cov + 1) + 2 * kSobolRC * (sobol_dim_chunk(d) + 1)) * sizeof(double);
}

uint64_t sobol_part_doubles(uint64_t p, uint64_t d, uint64_t q) {
  const uint64_t dc = sobol_dim_chunk(d), ndc = (d + dc - 1) / dc, nrc = (q + kSobolRC - 1) / kSobolRC;
  const uint64_t nt = (p + kSobolTW - 1) / kSobolTW;
  return ndc * nrc * (nt * (nt + 1) / 2) * kSobolRC * (dc + 1);
}

int launch_sobol_first(const uint8_t *d_lev, const int *d_meta, uint64_t p, uint64_t d, uint64_t q, uint64_t lmax,
                       uint64_t sum_l, const double *d_Theta, const double *d_mtab, const double *d_ctab, double *d_excl,
                       double *d_u, double *d_out, double *d_g) {
  ProfScope ps("sobol_first");
  OB_TRY(launch_sobol_excl(d_lev, d_meta, p, d, d_mtab, d_excl, d_u));
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
  return block_pairs_lds(Sobol2Op::kTables, n_cov, Sobol2Op::T, Sobol2Op::RC);
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

int launch_sobol2_pairs(const uint8_t *d_lev, const int *d_meta, uint64_t p, uint64_t d, uint64_t q, uint64_t n_cov,
                        const double *d_Theta, const double *d_mtab, const double *d_ctab, double *d_part,
                        double *d_out) {
  ProfScope ps("sobol2_pairs");
  const int n_pairs = (int)(d * (d - 1) / 2);
  return launch_block_pairs<Sobol2Op>(d_lev, d_meta, p, d, q, n_cov, d_Theta, Sobol2Op::Tables{d_mtab, d_ctab}, d_part,
                                      2 * n_pairs, n_pairs, d_out);
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
