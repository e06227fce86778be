// The two-objective front of the acquisition picks over several responses, once: acquire_multi.cpp normalises the
// caller's points with it on the host, k_macq_pick (kernels_acquire_multi.hip) enters a believed-feasible pick with
// it on the device.  Plain C++ (tests/acquire_front_check.cpp walks it as a program of its own).
//
// The front is F points (u[s], c[s]) in signed units, u strictly ascending and c strictly descending, all strictly
// inside the reference box (u < r1, c < r2).  A point y = (y1, y2):
//   unchanged  when y is not strictly inside the box (a coordinate that is not a number included),
//   unchanged  when some front point is <= y in both coordinates,
//   otherwise  every front point >= y in both coordinates leaves and y is inserted in order.
// Serial and in place; the arrays hold at least F + 1 entries.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define OBHIP_FRONT_HD __host__ __device__
#else
#define OBHIP_FRONT_HD
#endif

namespace obhip {

constexpr uint64_t kMacqFrontCap = 2048;  // F0 + k at most: the front never holds more
constexpr int kMacqMaxQ = 16;

// -> the new F
OBHIP_FRONT_HD inline uint64_t front_insert(double *u, double *c, uint64_t F, double y1, double y2, double r1,
                                            double r2) {
  if (!(y1 < r1 && y2 < r2)) return F;
  for (uint64_t s = 0; s < F; ++s)
    if (u[s] <= y1 && c[s] <= y2) return F;
  uint64_t w = 0;  // the survivors, in their order
  for (uint64_t s = 0; s < F; ++s)
    if (!(u[s] >= y1 && c[s] >= y2)) {
      u[w] = u[s];
      c[w] = c[s];
      ++w;
    }
  // a survivor with u == y1 would dominate y or be dominated by it: u is strictly ascending after the insertion
  uint64_t pos = 0;
  while (pos < w && u[pos] < y1) ++pos;
  for (uint64_t s = w; s > pos; --s) {
    u[s] = u[s - 1];
    c[s] = c[s - 1];
  }
  u[pos] = y1;
  c[pos] = y2;
  return w + 1;
}

}  // namespace obhip
