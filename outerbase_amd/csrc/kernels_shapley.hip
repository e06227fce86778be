// Shapley effects of the fitted mean (sobol.cpp; include/obhip.h, "variance-based sensitivity"; DESIGN.md
// section 29).  No reference counterpart.
//
// Players are groups of dimensions.  Per term pair (k, k') a player g has mm_g = prod_{i in g} (m m)_i and
// c_g = prod_{i in g} A_i - prod_{i in g} (m m)_i, A = C + m m, and
//   Sh_g = sum_{k,k'} theta_k theta_k' c_g int_0^1 prod_{h != g} (mm_h + s c_h) ds,
// the integrand a polynomial of degree P - 1 in s: ceil(P / 2) Gauss-Legendre nodes on [0,1] are exact.
// k_shapley_pairs<NS, RC>: k_sobol_pairs' shape -- the upper triangle of pairs of 128-term tiles, lane = term k,
//   the partner k' wave-uniform, C_l and m_l m_l^T of every dimension in LDS (A is their sum in registers).  Per
//   pair the dimensions are swept in the plan's order (ShapPlan, obhip_internal.h), every player contiguous:
//   D <- c PA + mm D, PA <- PA A, MM <- MM mm run over a player's dimensions and leave (c_g, mm_g) = (D, MM) in the
//   slot of its last dimension; every other slot holds the neutral player (0, 1), whose factor is 1 at every node
//   and whose effect is 0.  Then per node s_n a backward sweep stores the suffix products of mm + s_n c and a
//   forward sweep with the running prefix adds theta_k theta_k' w_n c prefix suffix to the slot's sum, for the RC
//   responses of the chunk.  Nodes, weights and the plan are kernel arguments: scalar loads.  The partner's levels
//   in the dimensions that have a slot are staged in LDS once per block, a byte per slot, and read four to a word.
// k_shapley_reduce sums the per-block partials in a fixed order.  No atomics: the same bits on every call.
#include "obhip_internal.h"
#include "sobol_device.h"

namespace obhip {

namespace {

// A wave-uniform value the compiler must take as new at this point.  Without it every predicate on the plan (a
// slot's last-dimension bit, s < ns) is hoisted out of the pair loop as a lane mask of its own, two SGPRs each,
// and the SGPR file spills; with it they are one scalar compare where they are used.
__device__ __forceinline__ unsigned fresh(unsigned v) {
  asm volatile("" : "+s"(v));
  return v;
}

// dynamic LDS: [C: n_cov][m m^T: n_cov][reduction 2 * RC * NS][levels of the partners: 128 * NS bytes].
// grid (tile pairs, response chunks); part[(rc * npairs + pair) * RC * NS + r * NS + s]
template <int NS, int RC, bool MEM>
__global__ void __launch_bounds__(kSobolTW)
k_shapley_pairs(const ShapPlan plan, const uint8_t *__restrict__ lev, const int *__restrict__ meta, int p, int d, int q,
                int n_cov, const double *__restrict__ Theta, const double *__restrict__ mtab,
                const double *__restrict__ ctab, double *__restrict__ part) {
  constexpr int SB = 4;  // slots per guarded block of the sweeps: slots [ns, a multiple of SB) run as neutral players
  static_assert(NS % SB == 0 && NS <= kShapMaxPlayers && RC * NS <= kSobolTW, "slot layout");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *tC = smem, *tM = tC + n_cov, *red = tM + n_cov;
  uint8_t *plv = (uint8_t *)(red + 2 * RC * NS);
  int I, J;
  tile_pair(blockIdx.x, (p + kSobolTW - 1) / kSobolTW, I, J);
  const int j0 = blockIdx.y * RC, ns = plan.ns;
  for (int l = 0; l < d; ++l) {
    const int L = meta[l], om = meta[d + l], oc = meta[2 * d + l];
    for (int e = threadIdx.x; e < L * L; e += kSobolTW) {
      tC[oc + e] = ctab[oc + e];
      tM[oc + e] = mtab[om + e / L] * mtab[om + e % L];
    }
  }
  const int nj = min(kSobolTW, p - J * kSobolTW);
  for (int e = threadIdx.x; e < nj * NS; e += kSobolTW) {
    const int s = e % NS;
    plv[e] = s < ns ? lev[(uint64_t)(J * kSobolTW + e / NS) * d + plan.regdim[s]] : 0;
  }
  __syncthreads();
  const int k = I * kSobolTW + threadIdx.x;
  const bool valid = k < p;
  const uint8_t *lv = lev + (uint64_t)(valid ? k : p - 1) * d;  // (a lane beyond p: any term, its coefficient is 0)
  int rowb[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    int l = plan.regdim[s < ns ? s : 0];
    asm volatile("" : "+v"(l));                          // (vector loads of meta: NS scalar addresses at once spill)
    rowb[s] = meta[2 * d + l] + (int)lv[l] * meta[l];
  }
  double th[RC], acc[RC][NS];
#pragma unroll
  for (int r = 0; r < RC; ++r) {
    th[r] = valid && j0 + r < q ? Theta[(uint64_t)(j0 + r) * p + k] : 0.0;
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[r][s] = 0.0;
  }
  for (int kk = 0; kk < nj; ++kk) {
    const int k2 = J * kSobolTW + kk;                   // (wave-uniform)
    const uint8_t *lp = lev + (uint64_t)k2 * d;
    // the players of this pair, into the slots
    double cs[NS], ms[NS], pa = 1.0, dd = 0.0, mmm = 1.0;
    int pos = 0;
    unsigned lw = 0;
    const unsigned nsl = fresh(ns), last_lo = fresh((unsigned)plan.lastmask);
    const unsigned last_hi = fresh((unsigned)(plan.lastmask >> 32));
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      cs[s] = 0.0;
      ms[s] = 1.0;
      if (s % 4 == 0) lw = ((const unsigned *)plv)[kk * (NS / 4) + s / 4];   // (one address per wave: a broadcast)
      if (s < (int)nsl) {                                // (wave-uniform, like every branch on the plan)
        if (MEM) {                                       // dimensions without a register (d > NS)
          const int nm = (fresh(plan.nmem[s / 4]) >> (8 * (s % 4))) & 0xffu;
          for (int i = 0; i < nm; ++i, ++pos) {
            const int l = plan.perm[pos], idx = meta[2 * d + l] + (int)lv[l] * meta[l] + lp[l];
            const double c = tC[idx], mm = tM[idx];
            dd = fma(mm, dd, pa * c);
            pa *= c + mm;
            mmm *= mm;
          }
          ++pos;
        }
        const int idx = rowb[s] + (int)((lw >> (8 * (s % 4))) & 0xffu);
        const double c = tC[idx], mm = tM[idx];
        dd = fma(mm, dd, pa * c);                        // prod A - prod m m over the player so far
        pa *= c + mm;
        mmm *= mm;
        if (((s < 32 ? last_lo : last_hi) >> (s % 32)) & 1u) {
          cs[s] = dd;
          ms[s] = mmm;
          pa = 1.0, dd = 0.0, mmm = 1.0;
        }
      }
    }
    double wv[RC];
#pragma unroll
    for (int r = 0; r < RC; ++r) wv[r] = th[r] * Theta[(uint64_t)min(j0 + r, q - 1) * p + k2];
    for (int n = 0; n < plan.nnode; ++n) {
      const double sn = plan.node[n];
      double sf[NS], suf = 1.0, pre = plan.wt[n];
      const int nsn = (int)fresh(ns);
#pragma unroll
      for (int b = NS / SB - 1; b >= 0; --b)
        if (b * SB < nsn) {
#pragma unroll
          for (int s = b * SB + SB - 1; s >= b * SB; --s) {
            sf[s] = suf;                                 // prod_{h > s} (mm_h + s_n c_h)
            suf *= fma(sn, cs[s], ms[s]);
          }
        }
#pragma unroll
      for (int b = 0; b < NS / SB; ++b)
        if (b * SB < nsn) {
#pragma unroll
          for (int s = b * SB; s < b * SB + SB; ++s) {
            const double f = cs[s] * (pre * sf[s]);      // w_n c_s prod_{h != s} (mm_h + s_n c_h)
#pragma unroll
            for (int r = 0; r < RC; ++r) acc[r][s] = fma(wv[r], f, acc[r][s]);
            pre *= fma(sn, cs[s], ms[s]);
          }
        }
    }
  }
  // the block's partials: butterfly per wave, wave 0 + wave 1; an off-diagonal tile pair stands for its mirror too
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < RC; ++r)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const double v = wave_sum(acc[r][s]);
      if (lane == 0) red[wave * RC * NS + r * NS + s] = v;
    }
  __syncthreads();
  if ((int)threadIdx.x < RC * NS) {
    const double s = red[threadIdx.x] + red[RC * NS + threadIdx.x];
    part[((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * RC * NS + threadIdx.x] = (I == J ? 1.0 : 2.0) * s;
  }
}

// block (player g, response j), one wave over the tile pairs
__global__ void __launch_bounds__(64)
k_shapley_reduce(const ShapPlan plan, const double *__restrict__ part, int npairs, int nslot, int rcw,
                 double *__restrict__ out) {
  const int g = blockIdx.x, j = blockIdx.y;
  const int rc = j / rcw, r = j % rcw;
  const double *base = part + (uint64_t)rc * npairs * rcw * nslot + r * nslot + plan.slot[g];
  double s = 0.0;
  for (int b = threadIdx.x; b < npairs; b += 64) s += base[(uint64_t)b * rcw * nslot];
  s = wave_sum(s);
  if (threadIdx.x == 0) out[(uint64_t)j * plan.nplayers + g] = s;
}

}  // namespace

size_t shapley_pairs_lds(uint64_t d, uint64_t n_cov) {
  return (2 * n_cov + 2 * shapley_rc(d) * shapley_slots(d)) * sizeof(double) + (size_t)kSobolTW * shapley_slots(d);
}

uint64_t shapley_part_doubles(uint64_t p, uint64_t d, uint64_t q) {
  const uint64_t rc = shapley_rc(d), nrc = (q + rc - 1) / rc, nt = (p + kSobolTW - 1) / kSobolTW;
  return nrc * (nt * (nt + 1) / 2) * rc * shapley_slots(d);
}

int launch_shapley_pairs(const ShapPlan &plan, const uint8_t *d_lev, const int *d_meta, uint64_t p, uint64_t d,
                         uint64_t q, uint64_t n_cov, const double *d_Theta, const double *d_mtab, const double *d_ctab,
                         double *d_part, double *d_out) {
  const int nslot = shapley_slots(d), rcw = shapley_rc(d), nrc = (int)((q + rcw - 1) / rcw);
  const int nt = (int)((p + kSobolTW - 1) / kSobolTW), npairs = nt * (nt + 1) / 2;
  const size_t lds = shapley_pairs_lds(d, n_cov);
  ProfScope ps("shapley_pairs");
  const int rc = pick_or<8, 24, 40>(nslot, -1, [&](auto NSc) {
    constexpr int RC = NSc() <= 24 ? 2 : 1;
    if (RC != rcw) return no_kernel();
    return pick_bool(d > (uint64_t)nslot, [&](auto MEMc) {
      if constexpr (MEMc() && NSc() != kShapMaxPlayers) {
        return no_kernel();
      } else {
        OB_TRY(ensure_dyn_lds((const void *)k_shapley_pairs<NSc(), RC, MEMc()>, lds));
        hipLaunchKernelGGL((k_shapley_pairs<NSc(), RC, MEMc()>), dim3(npairs, nrc), dim3(kSobolTW), lds, cur_stream(),
                           plan, d_lev, d_meta, (int)p, (int)d, (int)q, (int)n_cov, d_Theta, d_mtab, d_ctab, d_part);
        return 0;
      }
    });
  });
  if (rc < 0) return no_kernel();
  OB_TRY(rc);
  hipLaunchKernelGGL(k_shapley_reduce, dim3((unsigned)plan.nplayers, (unsigned)q), dim3(64), 0, cur_stream(), plan,
                     (const double *)d_part, npairs, nslot, rcw, d_out);
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace obhip
