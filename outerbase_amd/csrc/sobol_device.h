// Device helpers shared by kernels_sobol.hip and kernels_shapley.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace obhip {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the z-th pair (I <= J) of ntile term tiles in the order (0,0), (0,1), .. (0,ntile-1), (1,1), ..
__device__ __forceinline__ void tile_pair(int z, int ntile, int &I, int &J) {
  I = 0;
  while (z >= ntile - I) {
    z -= ntile - I;
    ++I;
  }
  J = I + z;
}

}  // namespace obhip
