// The row passes of the GLM fit (glm.cpp; include/obhip.h, "weighted, binomial and Poisson responses").
//
// k_glm_rows<FAMILY, TRIAL>: lane = row.  Between two Newton steps it turns the linear predictor
// eta into the mean mu, the IRLS weight w, the weighted row factor scale sqrt(w) that every consumer
// of the basis reads in place of `scale` for the next Gram, and the working column u; it also sums
// the log-likelihood.  With TRIAL (a step length of the line search being tried) it writes nothing
// but the sums.  HBM-streaming: 5 reads and 4 writes of 8 bytes per row at most.
//
// The sums are those of vsum<3> (vec_ops.h): grid-stride accumulation per thread, the 128 -> 1 tree
// in LDS, then k_vsum2 -- a fixed order, no atomics, the same bits on every call.
//
// k_glm_response<FAMILY>: the predictor's way from the link scale to the response scale.
#include "glm_row.h"
#include "obhip_internal.h"
#include "vec_ops.h"

namespace obhip {

namespace {

template <int FAMILY, bool TRIAL>
__global__ void __launch_bounds__(256) k_glm_rows(GlmRows r, uint64_t n_pad, double *__restrict__ part) {
  __shared__ double red[kGlmSums][256];
  double acc[kGlmSums];
#pragma unroll
  for (int k = 0; k < kGlmSums; ++k) acc[k] = 0.0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_pad; i += (uint64_t)gridDim.x * 256) {
    if (i >= r.n) {
      // the padding of the last row tile: zeros whatever the inputs hold there (a NaN times a zero
      // row factor would poison every entry of the Gram)
      if constexpr (!TRIAL) {
        r.scale_w[i] = 0.0;
        r.u[i] = 0.0;
      }
      continue;
    }
    double eta = r.eta ? r.eta[i] : (r.o ? r.o[i] : 0.0);
    if (r.deta) eta = fma(r.alpha, r.deta[i], eta);
    const double y = r.y[i], a = r.a ? r.a[i] : 1.0;
    const GlmRow v = glm_row<FAMILY>(eta, y, a, r.e2);
    if (v.finite) {
      acc[0] += v.al;
      acc[1] += v.mag;
    } else {
      acc[2] += 1.0;
    }
    if constexpr (!TRIAL) {
      r.eta_out[i] = eta;
      if (r.mu) r.mu[i] = v.mu;
      r.scale_w[i] = r.scale[i] * v.sw;
      r.u[i] = v.u;
    }
  }
#pragma unroll
  for (int k = 0; k < kGlmSums; ++k) red[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) {
#pragma unroll
      for (int k = 0; k < kGlmSums; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x < kGlmSums) part[(uint64_t)blockIdx.x * kGlmSums + threadIdx.x] = red[threadIdx.x][0];
}

template <int FAMILY>
__global__ void __launch_bounds__(256) k_glm_response(uint64_t n, const double *__restrict__ o, double *eta_io,
                                                      const double *__restrict__ vareta, double *__restrict__ mu_out,
                                                      double *__restrict__ varmu) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double eta = eta_io[i] + (o ? o[i] : 0.0);
  double mu, dmu, b;
  glm_link<FAMILY>(eta, mu, dmu, b);
  if (o) eta_io[i] = eta;
  if (mu_out) mu_out[i] = mu;
  if (varmu) varmu[i] = dmu * dmu * vareta[i];
}

}  // namespace

int launch_glm_rows(const GlmRows &r, double *d_sums, double *d_part) {
  const bool trial = r.scale_w == nullptr;
  const uint64_t n_pad = (r.n + kTileRows - 1) / kTileRows * kTileRows;
  const int nblk = sum_blocks(n_pad);
  ProfScope ps(trial ? "glm_rows_trial" : "glm_rows");
  const int rc = pick_or<OBHIP_GLM_GAUSSIAN, OBHIP_GLM_BINOMIAL, OBHIP_GLM_POISSON>(r.family, -1, [&](auto FAM) {
    return pick_bool(trial, [&](auto TR) {
      hipLaunchKernelGGL((k_glm_rows<FAM(), TR()>), dim3(nblk), dim3(256), 0, cur_stream(), r, n_pad, d_part);
      return 0;
    });
  });
  if (rc) return no_kernel();
  hipLaunchKernelGGL(k_vsum2<kGlmSums>, dim3(kGlmSums), dim3(64), 0, cur_stream(), (const double *)d_part, nblk,
                     d_sums);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_glm_response(int family, uint64_t n, const double *d_o, double *d_eta, const double *d_vareta,
                        double *d_mu, double *d_varmu) {
  if (n == 0) return 0;
  ProfScope ps("glm_response");
  const int rc = pick_or<OBHIP_GLM_GAUSSIAN, OBHIP_GLM_BINOMIAL, OBHIP_GLM_POISSON>(family, -1, [&](auto FAM) {
    hipLaunchKernelGGL(k_glm_response<FAM()>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cur_stream(), n, d_o,
                       d_eta, d_vareta, d_mu, d_varmu);
    return 0;
  });
  if (rc) return no_kernel();
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace obhip
