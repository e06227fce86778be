// The plan of the term-count path (term_path.cpp, kernels_term_path.hip): checkpoints, tile
// and group sizes, the layout of the sums, scratch bytes, the response block and the refusals.  Plain C++17,
// nothing from HIP and nothing of the library, like row_chunks.h, so that tests/term_path_check.cpp can walk every
// case on the host.  The launchers behind it are declared at the end for the two translation units that share them.
#pragma once
#include <algorithm>
#include <cstdint>

#include "row_chunks.h"

namespace obhip {

constexpr uint64_t kTpTileRows = 128;  // rows of a tile: one workgroup, one lane per row
constexpr uint64_t kTpTileCols = 32;   // columns of Z staged through LDS at a time
constexpr uint64_t kTpPitch = kTpTileCols + 1;  // doubles: odd, so that 32 lanes reading one column hit 64 banks
constexpr uint64_t kTpGroup = 64;      // tiles of a group of the second stage: fixed, whatever the chunks are
constexpr uint64_t kTpRespBlock = 4;   // responses a pass keeps in registers (m_j and y_j per lane)
constexpr uint64_t kTpMaxQ = 65534, kTpMaxP = 65535;
constexpr uint64_t kTpMaxRows = 1ull << 40;
constexpr uint64_t kTpMaxChunkRows = 1ull << 30;      // tiles of a chunk are the grid of a launch
constexpr uint64_t kTpZCapBytes = 1ull << 30;         // the stored Z of a chunk that chunk_rows = 0 stands for
static_assert(kTpRespBlock * kTpTileCols <= kTpTileRows, "one sweep of the tile's lanes stages U");
static_assert(kTpTileRows % kTpTileCols == 0 && 128 % kTpTileCols == 0, "Z is padded to 128 both ways");

// why a call is refused, or nullptr; everything here is known before the first launch
inline const char *term_path_refusal(uint64_t p, uint64_t q, uint64_t step, uint64_t n, uint64_t chunk_rows) {
  if (p == 0 || p > kTpMaxP) return "p must be between 1 and 65535";
  if (q == 0 || q > kTpMaxQ) return "q must be between 1 and 65534";
  if (step == 0) return "step must be at least 1";
  if (n > kTpMaxRows) return "more than 2^40 rows in one call";
  if (chunk_rows % 128 != 0) return "chunk_rows must be 0 or a positive multiple of 128";
  if (chunk_rows > kTpMaxChunkRows) return "chunk_rows above 2^30";
  return nullptr;
}

struct TermPathPlan {
  uint64_t p = 0, q = 0, step = 1, n = 0, cmax = 128;

  uint64_t pp() const { return pad128(p); }
  // checkpoints k_c = min((c + 1) step, p), c < K = ceil(p / step); step >= p: the one checkpoint k = p
  uint64_t K() const { return step >= p ? 1 : (p + step - 1) / step; }
  uint64_t checkpoint(uint64_t c) const { return c + 1 >= K() ? p : (c + 1) * step; }
  // the checkpoint after k (the kernel's walk): never past p, no overflow for any step
  uint64_t next_checkpoint(uint64_t k) const { return p - k > step ? k + step : p; }
  // one set of sums: [K][q][3] (sse, spe, lpd), then sumv [K]
  uint64_t score_entries() const { return K() * q * 3; }
  uint64_t entries() const { return K() * (3 * q + 1); }
  uint64_t score_at(uint64_t c, uint64_t j, uint64_t s) const { return (c * q + j) * 3 + s; }
  uint64_t sumv_at(uint64_t c) const { return score_entries() + c; }
  // tiles and groups of the whole call: a tile is rows [128 T, 128 T + 128) whatever the chunks are, because a
  // chunk is a multiple of 128 rows, and group g holds tiles [64 g, 64 g + 64)
  uint64_t tiles() const { return (n + kTpTileRows - 1) / kTpTileRows; }
  uint64_t groups() const { return (tiles() + kTpGroup - 1) / kTpGroup; }
  uint64_t passes() const { return (q + kTpRespBlock - 1) / kTpRespBlock; }
  // rows of the largest chunk and its tiles
  uint64_t chunk_rows_max() const { return std::min(cmax, pad128(std::max<uint64_t>(n, 1))); }
  // pooled scratch of a scores call: Z of a chunk, its tiles' partial sums and the group sums
  uint64_t scratch_bytes() const {
    const uint64_t cr = chunk_rows_max();
    return (cr * pp() + (cr / kTpTileRows) * entries() + groups() * entries()) * sizeof(double);
  }
};

inline TermPathPlan term_path_plan(uint64_t p, uint64_t q, uint64_t step, uint64_t n, uint64_t chunk_rows) {
  TermPathPlan t;
  t.p = p, t.q = q, t.step = step, t.n = n;
  t.cmax = chunk_rows ? chunk_rows : std::min(kTpMaxChunkRows, chunk_rows_for(pad128(p), kTpZCapBytes));
  return t;
}

}  // namespace obhip

#if defined(__HIPCC__)
namespace obhip {
// kernels_term_path.hip
// one pass of a chunk's tiles over responses j0 .. j0 + nresp - 1 (nresp <= kTpRespBlock): d_part[tile][entries]
int launch_term_path(const TermPathPlan &plan, const double *d_Z, uint64_t nr, uint64_t npad, const double *d_U,
                     uint64_t j0, uint64_t nresp, const double *d_Y, uint64_t ldy, const double *d_meansd, double nu,
                     int loo, double *d_part);
// the chunk's tile sums added to their groups' in ascending tile order; tile0 = the chunk's first tile of the call
int launch_term_path_fold(const TermPathPlan &plan, const double *d_part, uint64_t ctiles, uint64_t tile0,
                          double *d_groups);
// the group sums added in ascending order into d_scores (K q 3) and d_sumv (K)
int launch_term_path_final(const TermPathPlan &plan, const double *d_groups, double *d_scores, double *d_sumv);
// U = X^T G and Theta_k = X[:k,:k] U[:k] (zeros behind k), X pp x pp row-major, the others p x q column-major
int launch_term_path_coef(const double *d_X, uint64_t p, uint64_t pp, const double *d_G, uint64_t q, double *d_U);
int launch_term_path_theta(const double *d_X, uint64_t p, uint64_t pp, const double *d_U, uint64_t q, uint64_t k,
                           double *d_Theta);
}  // namespace obhip
#endif
