// The plan of the conditional moments (conditional.cpp, kernels_conditional.hip): the groups
// of terms by their levels on the noise dimensions, the row chunks and the workspace of a chunk, and the refusals.
// Plain C++17, nothing from HIP and nothing of the library, like term_path_plan.h and row_chunks.h, so that
// tests/conditional_plan_check.cpp can walk every case on the host.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "row_chunks.h"

namespace obhip {

constexpr uint64_t kCondMaxQ = 65535;             // the response limit of the Sobol passes
constexpr uint64_t kCondMaxP = 1ull << 24;        // their term limit
constexpr uint64_t kCondMaxRows = 1ull << 40;     // rows obhip_predict_grad_dev takes in one call
constexpr uint64_t kCondMaxChunkRows = 1ull << 28;  // keeps the workspace of the largest q and G inside 64 bits
constexpr uint64_t kCondCapBytes = 1ull << 28;    // one group-major block (c or Y) of a chunk that chunk_rows = 0 stands for
constexpr uint64_t kCondRC = 4;                   // responses a wave keeps in registers
constexpr uint64_t kCondMaxGroups = 16384;        // K is G x G doubles: 2 GiB at the limit

inline uint64_t pad16(uint64_t v) { return (v + 15) / 16 * 16; }

// why a set of noise dimensions is refused, or nullptr: 1 to d - 1 entries, strictly ascending, each below d
inline const char *cond_dims_refusal(const uint32_t *dims_e, uint64_t ndims_e, uint64_t d) {
  if (!dims_e) return "null dims_e";
  if (ndims_e < 1 || ndims_e + 1 > d) return "dims_e must name 1 to d - 1 dimensions";
  for (uint64_t k = 0; k < ndims_e; ++k) {
    if (dims_e[k] >= d) return "dims_e entry out of range";
    if (k > 0 && dims_e[k] <= dims_e[k - 1]) return "dims_e must be strictly ascending";
  }
  return nullptr;
}

// why the sizes of a call are refused, or nullptr; everything here is known before the first launch
inline const char *cond_sizes_refusal(uint64_t p, uint64_t d, uint64_t q, uint64_t n, uint64_t chunk_rows) {
  if (p == 0 || p > kCondMaxP) return "p must be between 1 and 2^24";
  if (d == 0 || d > 255) return "1 to 255 dimensions";
  if (q == 0 || q > kCondMaxQ) return "1 to 65535 responses";
  if (n > kCondMaxRows) return "more than 2^40 rows in one call";
  if (chunk_rows % 128 != 0) return "chunk_rows must be 0 or a positive multiple of 128";
  if (chunk_rows > kCondMaxChunkRows) return "chunk_rows above 2^28";
  return nullptr;
}

// The groups of p terms (levels lev[k * d + l]) by their level tuples on dims_e, numbered in the order of their
// first term.  order: the terms sorted by (group, term), off[g] .. off[g + 1] the entries of group g; first[g]: the
// first term of group g, whose levels stand for the group.
struct CondGroups {
  uint64_t G = 0;
  std::vector<uint32_t> group_of, order, off, first;
};

template <typename Lev>
inline CondGroups cond_groups(const Lev *lev, uint64_t p, uint64_t d, const uint32_t *dims_e, uint64_t ne) {
  CondGroups g;
  g.group_of.resize(p);
  // terms sorted by (tuple, term): equal tuples are neighbours, the first of a run is the group's first term
  std::vector<uint32_t> idx(p);
  for (uint64_t k = 0; k < p; ++k) idx[k] = (uint32_t)k;
  auto cmp3 = [&](uint32_t a, uint32_t b) {
    for (uint64_t e = 0; e < ne; ++e) {
      const auto va = lev[(uint64_t)a * d + dims_e[e]], vb = lev[(uint64_t)b * d + dims_e[e]];
      if (va != vb) return va < vb ? -1 : 1;
    }
    return 0;
  };
  std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
    const int c = cmp3(a, b);
    return c != 0 ? c < 0 : a < b;
  });
  // the first term of every run, then the runs numbered by ascending first term
  std::vector<uint32_t> run_first(p);
  std::vector<uint32_t> firsts;
  for (uint64_t s = 0; s < p;) {
    uint64_t e = s + 1;
    while (e < p && cmp3(idx[s], idx[e]) == 0) ++e;
    for (uint64_t i = s; i < e; ++i) run_first[idx[i]] = idx[s];
    firsts.push_back(idx[s]);
    s = e;
  }
  std::sort(firsts.begin(), firsts.end());
  g.G = firsts.size();
  g.first = firsts;
  std::vector<uint32_t> id_of_first(p, 0);
  for (uint64_t i = 0; i < g.G; ++i) id_of_first[firsts[i]] = (uint32_t)i;
  g.off.assign(g.G + 1, 0);
  for (uint64_t k = 0; k < p; ++k) {
    g.group_of[k] = id_of_first[run_first[k]];
    ++g.off[g.group_of[k] + 1];
  }
  for (uint64_t i = 0; i < g.G; ++i) g.off[i + 1] += g.off[i];
  g.order.resize(p);
  std::vector<uint32_t> at(g.off.begin(), g.off.end() - 1);
  for (uint64_t k = 0; k < p; ++k) g.order[at[g.group_of[k]]++] = (uint32_t)k;  // ascending term order within a group
  return g;
}

// The rows of a call, cmax at a time, and the workspace of a call, one block of doubles that conditional.cpp carves in
// this order: the padded group tables mE (Gp) and K (Gp x Gp), the group coefficients c and the product Y = c K of a
// chunk (q x Gp x npad each, group-major with the rows contiguous), the moments M and W of the chunk (q x npad each).
struct CondPlan {
  uint64_t G = 0, q = 0, n = 0, cmax = 128;
  uint64_t Gp() const { return pad16(G); }
  RowChunks chunks() const { return RowChunks{n, cmax}; }
  uint64_t chunk_rows_max() const { return std::min(cmax, pad128(std::max<uint64_t>(n, 1))); }
  uint64_t block_doubles() const { return q * Gp() * chunk_rows_max(); }
  uint64_t moment_doubles() const { return q * chunk_rows_max(); }
  uint64_t off_mE() const { return 0; }
  uint64_t off_K() const { return Gp(); }
  uint64_t off_C() const { return off_K() + Gp() * Gp(); }
  uint64_t off_Y() const { return off_C() + block_doubles(); }
  uint64_t off_M() const { return off_Y() + block_doubles(); }
  uint64_t off_W() const { return off_M() + moment_doubles(); }
  uint64_t workspace_doubles() const { return off_W() + moment_doubles(); }
  uint64_t workspace_bytes() const { return workspace_doubles() * sizeof(double); }
};

// chunk_rows = 0: the library's choice, a block of c within kCondCapBytes; no product here overflows for the sizes
// cond_sizes_refusal lets through (q Gp <= 2^16 2^24)
inline CondPlan cond_plan(uint64_t G, uint64_t q, uint64_t n, uint64_t chunk_rows) {
  CondPlan c;
  c.G = G, c.q = q, c.n = n;
  c.cmax = chunk_rows ? chunk_rows : std::min(kCondMaxChunkRows, chunk_rows_for(q * pad16(G), kCondCapBytes));
  return c;
}

}  // namespace obhip

#if defined(__HIPCC__)
#include "obhip_internal.h"

namespace obhip {
// kernels_conditional.hip
// whether the row kernels keep the tile of S (mu used columns, nside dimensions, lists of w columns) in LDS
bool cond_rows_supports(uint64_t mu, uint64_t nside, uint64_t w);
// dynamic LDS of k_cond_tables: A, C and m m^T of the noise dimensions, n_cov entries each and a neutral one
inline size_t cond_tables_lds(uint64_t n_cov) { return 3 * (n_cov + 1) * sizeof(double); }
// mE (G) and K (G x G, leading dimension ldk >= G); d_meta: [L][offset in the mean table][offset in the covariance
// table] of the ne noise dimensions in the compact tables d_mtab, d_ctab of those dimensions alone, d_glev: G x ne levels
int launch_cond_tables(const uint8_t *d_glev, const int *d_meta, uint64_t G, uint64_t ne, uint64_t n_cov,
                       const double *d_mtab, const double *d_ctab, double *d_mE, double *d_K, uint64_t ldk);
// one row chunk: coefficients, Y = c K, the moments and, where asked for, the gradients.  The argument block of the
// row kernels, filled by conditional.cpp
struct CondChunk {
  const DimDesc *dims;
  const double *ka, *kb, *kc, *rot, *tab, *dtab;
  const int *side;        // the dimensions of S; column s of x holds dimension side[s]
  int nside;
  const int *cpos;        // compact column -> used column of S or -1
  int mu;                 // used columns of S (column 0 = ones)
  const uint32_t *colsw;  // p x W2 words of two used-column indices, right-aligned
  int W2, p;
  const uint32_t *order, *goff, *gof;  // terms by (group, term); G + 1 offsets; the group of a term
  int G, Gp, q;
  const double *Theta;    // p x q
  const double *mE, *K;   // Gp and Gp x Gp, zeros in the padding
  const uint32_t *vw, *voff;  // the views of the dimensions of S: W2 words of the other columns, own column, term
  const double *x;        // the chunk's rows, column-major with leading dimension ldx
  uint64_t ldx, nr, ntiles, npad;  // ntiles = npad / 64
  double *C, *Y;          // q x Gp x npad
  double *Mw, *Ww;        // q x npad: the chunk's moments
  uint64_t row0, n;       // the chunk's first row in the call, the call's rows
  double *mean, *var;     // n x q or null
  double *gradmean, *gradvar;  // [(j nside + a) n + i] or null
  double *scratch;        // HBM tiles (set by the launcher)
  bool fused;             // the tile in LDS
};
int launch_cond_chunk(CondChunk c);
}  // namespace obhip
#endif
