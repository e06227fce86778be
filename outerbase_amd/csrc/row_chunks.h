// Row chunks of the posterior family (posterior.cpp, design.cpp, acquire_dx.cpp, sample.cpp):
// a call's n rows are worked on cmax at a time so that the term-major blocks of a chunk (pp x pad128(rows) doubles
// each) stay below a cap.  Two parts.  The arithmetic is plain C++17, nothing from HIP and nothing of the library,
// so that tests/row_chunks_check.cpp can walk every case on the host.  The frame behind it is what the three
// callers used to write out each: gather, basis, B^T, the caller's work, the wait before the basis goes away.
#pragma once
#include <algorithm>
#include <cstdint>

namespace obhip {

inline uint64_t pad128(uint64_t v) { return (v + 127) / 128 * 128; }

// rows of a chunk so that one block of pp x rows doubles stays within cap_bytes: a multiple of 128, at least 128
inline uint64_t chunk_rows_for(uint64_t pp, uint64_t cap_bytes) {
  return std::max<uint64_t>(128, (cap_bytes / (pp * sizeof(double))) / 128 * 128);
}

struct RowChunk {
  uint64_t r0, nr, npad;  // first row, rows, pad128(rows): the pitch of the chunk's term-major blocks
  bool whole;             // the chunk is the call: x needs no gather
};

// the chunks of n rows, cmax at a time, in ascending order: all but the last have cmax rows
struct RowChunks {
  uint64_t n, cmax;
  uint64_t count() const { return (n + cmax - 1) / cmax; }
  RowChunk at(uint64_t c) const {
    const uint64_t r0 = c * cmax, nr = std::min(cmax, n - r0);
    return {r0, nr, pad128(nr), r0 == 0 && nr == n};
  }
};

}  // namespace obhip

#if defined(__HIPCC__)
#include "obhip_internal.h"

namespace obhip {

// *xsrc = rows r0 .. r0 + nr - 1 of the column-major d_x (leading dimension ld, d columns) with leading dimension
// nr: d_x itself where the chunk is the call, else a compact copy in xc
inline int gather_rows(DevBuf<double> &xc, const double *d_x, uint64_t ld, uint64_t d, const RowChunk &c,
                       const double **xsrc) {
  *xsrc = d_x;
  if (c.whole) return 0;
  if (xc.n < c.nr * d) OB_TRY(xc.alloc(c.nr * d));  // (the last chunk is the short one)
  OB_HIP(hipMemcpy2DAsync(xc.p, c.nr * sizeof(double), d_x + c.r0, ld * sizeof(double), c.nr * sizeof(double), d,
                          hipMemcpyDeviceToDevice, cur_stream()));
  *xsrc = xc.p;
  return 0;
}

// fn(r0, nr, npad, Bcm) per chunk of the n rows of d_x (column-major n x d): Bcm = B^T of the chunk, term-major
// pp x npad with the rows contiguous and zeros behind row nr and term p; waits before the chunk's basis goes away
template <class Fn>
int for_row_chunks(const obhip_model &om, obhip_terms &t, const double *d_x, uint64_t n, uint64_t cmax, uint64_t pp,
                   Fn fn) {
  const RowChunks plan{n, cmax};
  DevBuf<double> Bcm, xc;
  for (uint64_t ci = 0; ci < plan.count(); ++ci) {
    const RowChunk c = plan.at(ci);
    const double *xsrc = nullptr;
    OB_TRY(gather_rows(xc, d_x, n, om.d, c, &xsrc));
    BasisGuard g;
    OB_TRY(obhip_basis_create_dev(&g.b, &om, xsrc, c.nr, t.maxlev.data()));
    OB_TRY(Bcm.alloc(pp * c.npad));
    OB_HIP(hipMemsetAsync(Bcm.p, 0, pp * c.npad * sizeof(double), cur_stream()));
    OB_TRY(launch_getmat(*g.b, t, Bcm.p, c.npad));
    OB_TRY(fn(c.r0, c.nr, c.npad, (const double *)Bcm.p));
    OB_HIP(hipStreamSynchronize(cur_stream()));
  }
  return 0;
}

}  // namespace obhip
#endif
