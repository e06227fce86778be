// Kernels of the acquisition picks over several responses (acquire_multi.cpp; include/obhip.h, "acquisition over
// several responses").  No reference counterpart.
//
// All q responses of a fit share H, so one pick's s = S b_j, gamma and a_i = b_i^T s serve them all: per step
//     mu_ir <- mu_ir + a_i delta_r / gamma  (r < q)        d_i <- d_i - a_i^2 / gamma  (once)
// and, on the signed means ms_r = g_r mu_r with sd = sqrt(max(d, 0)) (acquire_device.h: Psi = acq_score<EI>,
// P = acq_score<PI>, both with their sd = 0 branches),
//     pof   = prod_{r constraint, ascending} P(cs_r; ms_r, d)
//     CEI   Psi(best - xi; ms, d) pof   (best = +inf: pof)       CPI   P(best - xi; ms, d) pof   (likewise)
//     POF   pof
//     EHVI  pof sum_{s = 0 .. F} [Psi(U_s; ms_1, d) - Psi(U_{s-1}; ms_1, d)] Psi(C_s; ms_2, d),   Psi(U_{-1}) = 0,
//           U = (u_0 .. u_{F-1}, r1), C = (r2, c_0 .. c_{F-1}): the strips of the front in ascending order.
//
//   k_macq_update  256 rows per workgroup, lane = row.  The q deltas, signs, limits and roles and the front (U and C,
//                  F + 1 doubles each) are staged in LDS once per workgroup; in the strip loop every lane reads the
//                  same word in the same cycle (a broadcast).  Psi(U_{s-1}) is carried in a register.  Then the wave
//                  butterfly and the (best score, lowest index among equals) pair of k_acq_update.
//   k_macq_pick    one workgroup: the argmax tree of k_acq_pick, then thread 0 alone forms the q values y*_r and
//                  deltas, the believed-feasibility flag and the new incumbent or front (front_insert, serial).
// Every product, sum and argmax runs in a fixed order; the hand-overs are kernel boundaries.
#include <cmath>

#include "obhip_internal.h"
#include "acquire_device.h"
#include "acquire_front.h"

namespace obhip {

namespace {

template <int CRIT>
__global__ void __launch_bounds__(256)
k_macq_update(uint64_t n, int q, int obj1, int obj2, double xi, const double *__restrict__ a,
              const double *__restrict__ scal, const double *__restrict__ mst, const uint8_t *__restrict__ elig,
              const uint8_t *__restrict__ picked, double *__restrict__ mean, double *__restrict__ dvar,
              double *__restrict__ score0, double *__restrict__ pof0, double *__restrict__ part_score,
              int64_t *__restrict__ part_idx) {
  extern __shared__ double fr[];  // EHVI: U (F + 1), C (F + 1)
  __shared__ double sdel[kMacqMaxQ], sg[kMacqMaxQ], scs[kMacqMaxQ];
  __shared__ int srole[kMacqMaxQ];
  __shared__ double ws[4];
  __shared__ int64_t wi[4];
  const int tid = threadIdx.x;
  if (tid < q) {
    sdel[tid] = mst[kMacqDelta + tid];
    sg[tid] = mst[kMacqSign + tid];
    scs[tid] = mst[kMacqLimit + tid];
    srole[tid] = (int)mst[kMacqRole + tid];
  }
  uint64_t F = 0;
  double *U = fr, *Cc = fr;
  if (CRIT == OBHIP_MACQ_EHVI) {
    F = (uint64_t)mst[kMacqF];
    Cc = fr + (F + 1);
    for (uint64_t s = tid; s < F; s += 256) {
      U[s] = mst[kMacqU + s];
      Cc[s + 1] = mst[kMacqC + s];
    }
    if (tid == 0) {
      U[F] = mst[kMacqLimit + obj1];
      Cc[0] = mst[kMacqLimit + obj2];
    }
  }
  __syncthreads();
  const uint64_t row = (uint64_t)blockIdx.x * kAcqRows + tid;
  double score = -INFINITY;
  int64_t idx = kNoIndex;
  if (row < n) {
    const double gamma = scal[0];
    const double ai = a[row], ag = ai / gamma;
    const double d = dvar[row] - ai * ag;
    dvar[row] = d;
    double pof = 1.0, m1 = 0.0, m2 = 0.0;
    for (int r = 0; r < q; ++r) {
      const double m = mean[(uint64_t)r * n + row] + ag * sdel[r];
      mean[(uint64_t)r * n + row] = m;
      if (srole[r] == OBHIP_ROLE_CONSTRAINT) pof *= acq_score<OBHIP_ACQ_PI>(sg[r] * m, d, scs[r], 0.0, 0.0, 0.0);
      if (r == obj1) m1 = m;
      if (r == obj2) m2 = m;
    }
    double base = 1.0;
    if (CRIT == OBHIP_MACQ_CEI || CRIT == OBHIP_MACQ_CPI) {
      const double best = mst[kMacqBest];
      if (best < INFINITY)
        base = acq_score<CRIT == OBHIP_MACQ_CEI ? OBHIP_ACQ_EI : OBHIP_ACQ_PI>(sg[obj1] * m1, d, best, xi, 0.0, 0.0);
    }
    if (CRIT == OBHIP_MACQ_EHVI) {
      const double ms1 = sg[obj1] * m1, ms2 = sg[obj2] * m2;
      double prev = 0.0, sum = 0.0;
      for (uint64_t s = 0; s <= F; ++s) {
        const double pu = acq_score<OBHIP_ACQ_EI>(ms1, d, U[s], 0.0, 0.0, 0.0);
        const double pc = acq_score<OBHIP_ACQ_EI>(ms2, d, Cc[s], 0.0, 0.0, 0.0);
        sum += (pu - prev) * pc;
        prev = pu;
      }
      base = sum;
    }
    const double sc = base * pof;
    if (score0) score0[row] = sc;
    if (pof0) pof0[row] = pof;
    if (elig[row] && !picked[row] && isfinite(sc)) {
      score = sc;
      idx = (int64_t)row;
    }
  }
  wave_best(score, idx);
  if ((tid & 63) == 0) {
    ws[tid >> 6] = score;
    wi[tid >> 6] = idx;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w)
      if (beats(ws[w], wi[w], score, idx)) {
        score = ws[w];
        idx = wi[w];
      }
    part_score[blockIdx.x] = score;
    part_idx[blockIdx.x] = idx;
  }
}

// scal: the design step's block ([0] gamma, [5] 1 = no eligible candidate was left); mst: the state block of
// obhip_internal.h (deltas, signs, limits, lie values, roles, the incumbent, F and the front)
__global__ void __launch_bounds__(256)
k_macq_pick(const double *__restrict__ part_score, const int64_t *__restrict__ part_idx, uint64_t nparts,
            const double *__restrict__ x, uint64_t n, int d, uint64_t step, const double *__restrict__ mean, int q,
            int crit, int lie, int obj1, int obj2, int64_t *__restrict__ index, double *__restrict__ score_out,
            double *__restrict__ xj, uint8_t *__restrict__ picked, double *__restrict__ scal, double *__restrict__ mst) {
  __shared__ double ws[256];
  __shared__ int64_t wi[256];
  double score = -INFINITY;
  int64_t idx = kNoIndex;
  for (uint64_t b = threadIdx.x; b < nparts; b += 256) {
    const double os = part_score[b];
    const int64_t oi = part_idx[b];
    if (beats(os, oi, score, idx)) {
      score = os;
      idx = oi;
    }
  }
  ws[threadIdx.x] = score;
  wi[threadIdx.x] = idx;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off && beats(ws[threadIdx.x + off], wi[threadIdx.x + off], ws[threadIdx.x], wi[threadIdx.x])) {
      ws[threadIdx.x] = ws[threadIdx.x + off];
      wi[threadIdx.x] = wi[threadIdx.x + off];
    }
    __syncthreads();
  }
  score = ws[0];
  idx = wi[0];
  const bool none = !(score > -INFINITY) || idx < 0 || (uint64_t)idx >= n;
  if (none) {
    if (threadIdx.x == 0) scal[5] = 1.0;
    return;
  }
  if (threadIdx.x == 0) {
    index[step] = idx;
    score_out[step] = score;
    picked[idx] = 1;
    bool feasible = true;
    double y1 = 0.0, y2 = 0.0;
    for (int r = 0; r < q; ++r) {
      const double muj = mean[(uint64_t)r * n + (uint64_t)idx];
      const double ystar = lie == OBHIP_LIE_CONSTANT ? mst[kMacqLie + r] : muj;
      mst[kMacqDelta + r] = ystar - muj;
      const double ys = mst[kMacqSign + r] * ystar;
      if ((int)mst[kMacqRole + r] == OBHIP_ROLE_CONSTRAINT && !(ys <= mst[kMacqLimit + r])) feasible = false;
      if (r == obj1) y1 = ys;
      if (r == obj2) y2 = ys;
    }
    if (feasible) {  // only a believed-feasible pick moves the incumbent or the front
      if (crit == OBHIP_MACQ_CEI || crit == OBHIP_MACQ_CPI) mst[kMacqBest] = fmin(mst[kMacqBest], y1);
      if (crit == OBHIP_MACQ_EHVI)
        mst[kMacqF] = (double)front_insert(mst + kMacqU, mst + kMacqC, (uint64_t)mst[kMacqF], y1, y2,
                                           mst[kMacqLimit + obj1], mst[kMacqLimit + obj2]);
    }
  }
  for (int l = threadIdx.x; l < d; l += 256) xj[l] = x[(uint64_t)l * n + (uint64_t)idx];
}

template <int CRIT>
void run_macq_update(const MacqStep &s, double *d_score0, double *d_pof0) {
  const size_t dyn = CRIT == OBHIP_MACQ_EHVI ? 2 * (s.front_cap + 1) * sizeof(double) : 0;
  hipLaunchKernelGGL(k_macq_update<CRIT>, dim3((unsigned)((s.n + kAcqRows - 1) / kAcqRows)), dim3(256), dyn,
                     cur_stream(), s.n, s.q, s.obj1, s.obj2, s.xi, s.a, (const double *)s.scal, (const double *)s.mst,
                     s.elig, (const uint8_t *)s.picked, s.mean, s.dvar, d_score0, d_pof0, s.part_score, s.part_idx);
}

}  // namespace

uint64_t macq_update_lds_bytes(int crit, uint64_t front_cap) {
  // sdel, sg, scs, srole, ws, wi, then U and C
  const uint64_t fixed = 3 * kMacqMaxQ * sizeof(double) + kMacqMaxQ * sizeof(int) + 4 * sizeof(double) + 4 * sizeof(int64_t);
  return fixed + (crit == OBHIP_MACQ_EHVI ? 2 * (front_cap + 1) * sizeof(double) : 0);
}

int launch_macq_update(const MacqStep &s, double *d_score0, double *d_pof0) {
  ProfScope ps("macq_update");
  switch (s.crit) {
    case OBHIP_MACQ_CEI: run_macq_update<OBHIP_MACQ_CEI>(s, d_score0, d_pof0); break;
    case OBHIP_MACQ_CPI: run_macq_update<OBHIP_MACQ_CPI>(s, d_score0, d_pof0); break;
    case OBHIP_MACQ_POF: run_macq_update<OBHIP_MACQ_POF>(s, d_score0, d_pof0); break;
    case OBHIP_MACQ_EHVI: run_macq_update<OBHIP_MACQ_EHVI>(s, d_score0, d_pof0); break;
    default: return fail(OBHIP_ERR_INVALID, "acquire_multi: no kernel for this criterion");
  }
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_macq_pick(const MacqStep &s, uint64_t d, uint64_t step, int64_t *d_index, double *d_score, double *d_xj) {
  ProfScope ps("macq_pick");
  hipLaunchKernelGGL(k_macq_pick, dim3(1), dim3(256), 0, cur_stream(), (const double *)s.part_score,
                     (const int64_t *)s.part_idx, (s.n + kAcqRows - 1) / kAcqRows, s.x, s.n, (int)d, step,
                     (const double *)s.mean, s.q, s.crit, s.lie, s.obj1, s.obj2, d_index, d_score, d_xj, s.picked, s.scal,
                     s.mst);
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace obhip
