// Derivative-based sensitivity of the fitted mean: C = E[grad f grad f^T] and E[grad f] in closed form
// (sobol.cpp; include/obhip.h, "active subspaces"; DESIGN.md sections 31 and 33).  No reference counterpart.  The
// gradient tables are in kernels_moments.hip, the frame of the term-pair sum in pair_sum.h.
//
// k_active_gbar: block (dimension l, response): sum_k theta_k dm_l[t_kl] prod_{i != l} m_i[t_ki], the products
//   those of k_sobol_excl (no division), a tree over the threads.
// ActiveOp: the p^2 part by k_block_pairs, A_l, X_l and D_l of every dimension in LDS.  X is read in both
//   orientations per term pair: forward X_a[t,t'] at off_a + t L_a + t' and backward X_a[t',t] at
//   off_a + t' L_a + t (a lane part and a wave-uniform part either way).  Exchanging k and k' maps the summand
//   of C_lm onto that of C_ml, so over the upper triangle of term-tile pairs a pair (k, k') adds BOTH
//   orientations, f_ab = Rf_a Sb_b + Rb_a Sf_b, with weight 1; a diagonal tile pair runs over all its ordered
//   pairs and takes 1/2, which is exact.  On the diagonal of the output triangle 2 D_a prod_{l != a} A_l rides in
//   the DIAG pass.  The sum of the two orientations is written as fma(first product's factors, second product):
//   left to the compiler's contraction, which of the two products is rounded depends on the order in which it
//   happens to see them.  No atomics.
#include "obhip_internal.h"
#include "pair_sum.h"

namespace obhip {

namespace {

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
  s = block_tree_256(s, red);
  if (threadIdx.x == 0) out[(uint64_t)j * nout + l] = s;
}

// LDS tables: A, X, D; the neutral entry A = 1, X = D = 0.  A DIAG pass holds the outputs (a, b), a <= b, of its block
struct ActiveOp {
  static constexpr int T = kActiveT, RC = kActiveRC, NO = T * T, kTables = 3;
  static constexpr bool kDiagOutputs = true;
  struct Tables {
    const double *mtab, *ctab, *xtab, *dtab;
  };
  // every pair added both orientations: an off-diagonal tile pair stands as it is, a diagonal one has met every
  // unordered pair twice
  static __device__ __forceinline__ double scale(bool diag_tiles) { return diag_tiles ? 0.5 : 1.0; }
  static __device__ __forceinline__ void stage(double *lds, int n_cov, const int *__restrict__ meta, int d,
                                               const Tables &tb) {
    double *tA = lds, *tX = tA + n_cov + 1, *tD = tX + n_cov + 1;
    stage_pair_tables(
        meta, d,
        [&](int i, int ia, int ib) {
          tA[i] = tb.ctab[i] + tb.mtab[ia] * tb.mtab[ib];
          tX[i] = tb.xtab[i];
          tD[i] = tb.dtab[i];
        },
        [&] {
          tA[n_cov] = 1.0;
          tX[n_cov] = 0.0;
          tD[n_cov] = 0.0;
        });
  }
  template <bool DIAG>
  struct Lane {
    // per dimension of the two blocks: the forward offset off + t L (to which t' is added), the backward one
    // off + t (to which t' L is added) and L itself (wave-uniform; 0 for a dimension beyond d)
    int rf[T], rb[T], rL[T], cf[T], cb[T], cL[T];
    __device__ __forceinline__ void init(const int *__restrict__ meta, int d, int n_cov, const uint8_t *lv, int i0,
                                         int j0) {
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
    }
    __device__ __forceinline__ void factors(const double *lds, int n_cov, const uint8_t *lp, int d, int i0, int j0,
                                            double outp, double (&f)[NO]) const {
      const double *tA = lds, *tX = tA + n_cov + 1, *tD = tX + n_cov + 1;
      double ar[T], xf[T], xb[T], dr[T];
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
            f[a * T + b] = fma(mf, Sb[b], mb * Sf[b]);
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
          for (int b = 0; b < T; ++b) f[a * T + b] = fma(Rf[a], Sb[b], Rb[a] * Sf[b]);
      }
    }
  };
};

}  // namespace

size_t active_pairs_lds(uint64_t n_cov) {
  return block_pairs_lds(ActiveOp::kTables, n_cov, ActiveOp::T, ActiveOp::RC);
}

int launch_active(const uint8_t *d_lev, const int *d_meta, uint64_t p, uint64_t d, uint64_t q, uint64_t n_cov,
                  const double *d_Theta, const double *d_mtab, const double *d_ctab, const double *d_dmtab,
                  const double *d_xtab, const double *d_ddtab, double *d_excl, double *d_u, double *d_part,
                  double *d_out) {
  const int nout = (int)(d + d * (d + 1) / 2);
  OB_TRY(launch_sobol_excl(d_lev, d_meta, p, d, d_mtab, d_excl, d_u));
  ProfScope ps("active_pairs");
  hipLaunchKernelGGL(k_active_gbar, dim3((unsigned)d, (unsigned)q), dim3(256), 0, cur_stream(), d_lev, d_meta, (int)p,
                     (int)d, nout, d_Theta, d_dmtab, (const double *)d_excl, d_out);
  return launch_block_pairs<ActiveOp>(d_lev, d_meta, p, d, q, n_cov, d_Theta,
                                      ActiveOp::Tables{d_mtab, d_ctab, d_xtab, d_ddtab}, d_part, nout, (int)d, d_out);
}

}  // namespace obhip
