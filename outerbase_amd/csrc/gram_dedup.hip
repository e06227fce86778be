// Which 128 x 128 tile pairs of G = B^T B hold nothing that is not somewhere else in G.
//
// A column of the design matrix is scale x the product over the dimensions of one level function
// each (level 0: no factor), so G[s][t] = sum_i scale_i^2 prod_k r_k,s_k r_k,t_k depends on the
// per-dimension UNORDERED level pairs {s_k, t_k} only: G is a moment matrix, and (s, t), (s', t')
// hold the same sum whenever a factor can move from one term to the other.  The panel Gram
// (kernels_gram_panel.hip) works in tile pairs; a tile pair all of whose entries occur in tile pairs
// nearer the diagonal gets no task, and k_gram_fill copies its entries from there afterwards.
//
// The analysis runs once per term set, on the device (p = 4096: 8.65 million entries):
//   k_dd_keys     one key per entry of every upper-triangle tile pair: a 64-bit hash of the d
//                 unordered level pairs.  The entries are numbered tile pair by tile pair in the
//                 order of PRIORITY (smallest J - I first, then the smallest tile index), so that
//   radix sort    a STABLE sort by key alone leaves every key's occurrences in priority order,
//   k_dd_heads /  the first of them -- the canonical occurrence -- found by a running maximum over
//   scan          the segment starts.
//   k_dd_resolve  every entry compares its actual level pairs with those of its segment's head:
//                 the hash never decides an equality.  Equal and in another tile pair: the head is
//                 its source.  Anything else (the head itself, the head's own tile pair, a
//                 collision) marks the entry's tile pair as kept.
// A source is a segment head, heads keep their tile pairs, so sources always lie in kept pairs.
// Diagonal tile pairs (their diagonal entries are unique, the prior and diagH live there) and
// tile pairs that touch the padding columns of the last tile are kept whatever the analysis says.
#include <string.h>  // (memset for rocprim's headers)

#include <rocprim/rocprim.hpp>

#include <algorithm>

#include "obhip_internal.h"
#include "vec_ops.h"

namespace obhip {

namespace {

constexpr int kGT = kGramTile;
constexpr uint32_t kTileEntries = kGT * kGT;
constexpr uint64_t kNoKey = ~0ull;  // padding, and the lower half of diagonal tiles
// entries of all tile pairs above which the analysis is not run (p = 8192: 34 million; its
// temporaries take 32 bytes an entry and the sort's own storage, budgeted as 36)
constexpr uint64_t kMaxEntries = 48ull << 20;

__device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64's finaliser
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// entry e = rank << 14 | row << 7 | column of the tile pair order[rank] = I | J << 16
__device__ __forceinline__ bool dd_entry(uint32_t e, const uint32_t *__restrict__ order, uint32_t p, uint32_t &s,
                                         uint32_t &t) {
  const uint32_t ij = order[e >> 14], I = ij & 0xffffu, J = ij >> 16;
  s = I * kGT + ((e >> 7) & 127u);
  t = J * kGT + (e & 127u);
  return s < p && t < p && s <= t;
}

__global__ void __launch_bounds__(256)
k_dd_keys(const uint16_t *__restrict__ lev, uint32_t p, uint32_t d, const uint32_t *__restrict__ order, uint32_t n,
          int hashbits, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n) return;
  uint32_t s, t;
  uint64_t key = kNoKey;
  if (dd_entry(e, order, p, s, t)) {
    const uint16_t *ls = lev + (size_t)s * d, *lt = lev + (size_t)t * d;
    uint64_t h = 0x9e3779b97f4a7c15ull;
    for (uint32_t k = 0; k < d; ++k) {
      const uint32_t a = ls[k], b = lt[k], lo = min(a, b), hi = max(a, b);
      h = mix64(h ^ (uint64_t)(hi << 16 | lo)) + k;
    }
    key = h >> (64 - hashbits);  // hashbits <= 63: never kNoKey
  }
  keys[e] = key;
  vals[e] = e;
}

__global__ void __launch_bounds__(256)
k_dd_heads(const uint64_t *__restrict__ keys, uint32_t n, uint32_t *__restrict__ head) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  head[i] = i > 0 && keys[i] != keys[i - 1] ? i : 0u;  // running maximum = start of the segment
}

__global__ void __launch_bounds__(256)
k_dd_resolve(const uint16_t *__restrict__ lev, uint32_t p, uint32_t d, const uint32_t *__restrict__ order, uint32_t n,
             const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, const uint32_t *__restrict__ head,
             uint8_t *__restrict__ keep, uint32_t *__restrict__ src) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t e = vals[i];
  src[e] = ~0u;
  if (keys[i] == kNoKey) return;  // (their tile pairs are kept by rule)
  const uint32_t h = vals[head[i]];
  bool same = false;
  uint32_t s, t, hs = 0, ht = 0;
  if ((h >> 14) != (e >> 14)) {  // stable sort: the head's tile pair comes first in priority
    dd_entry(e, order, p, s, t);
    dd_entry(h, order, p, hs, ht);
    const uint16_t *ls = lev + (size_t)s * d, *lt = lev + (size_t)t * d;
    const uint16_t *ms = lev + (size_t)hs * d, *mt = lev + (size_t)ht * d;
    // (a head on the diagonal of G -- a term set with a duplicate term -- is no source: a formed
    // sink holds e2 G + the prior precision there)
    same = hs != ht;
    for (uint32_t k = 0; k < d && same; ++k) {
      const uint32_t a = ls[k], b = lt[k], a2 = ms[k], b2 = mt[k];
      same = min(a, b) == min(a2, b2) && max(a, b) == max(a2, b2);
    }
  }
  if (same)
    src[e] = hs << 16 | ht;
  else
    keep[e >> 14] = 1;
}

// G[s][t] = G[t][s] = G[s'][t'] for every entry of the skipped tile pairs (row-major or packed sink)
__global__ void __launch_bounds__(256)
k_gram_fill(const uint32_t *__restrict__ pairs, const uint32_t *__restrict__ src, uint32_t p,
            double *__restrict__ G, int packed) {
  const uint32_t ij = pairs[blockIdx.x], I = ij & 0xffffu, J = ij >> 16;
  const uint32_t *tab = src + (size_t)blockIdx.x * kTileEntries;
  for (uint32_t w = blockIdx.y * 256u + threadIdx.x; w < kTileEntries; w += gridDim.y * 256u) {
    const uint32_t s = I * kGT + (w >> 7), t = J * kGT + (w & 127u);
    const uint32_t q = tab[w], ss = q >> 16, st = q & 0xffffu;
    if (s >= p || t >= p || ss >= p || st >= p || ss > st) continue;  // (never: skipped pairs hold no padding)
    if (packed) {
      G[tri_off(s, p) + (t - s)] = G[tri_off(ss, p) + (st - ss)];
    } else {
      const double v = G[(uint64_t)ss * p + st];
      G[(uint64_t)s * p + t] = v;
      G[(uint64_t)t * p + s] = v;
    }
  }
}

int dedup_hashbits() {
  const char *e = getenv("OBHIP_GRAM_DEDUP_HASHBITS");
  const int v = e ? atoi(e) : 63;
  return std::max(1, std::min(63, v));
}

int analyse(obhip_terms &t, GramDedup &dd) {
  const double t0 = HostTimer::now();
  const uint32_t p = (uint32_t)t.p, d = (uint32_t)t.d;
  const int nb = dd.nb, npairs = dd.npairs;
  const uint32_t n = (uint32_t)npairs * kTileEntries;
  hipStream_t st = cur_stream();
  // tile pairs in the order of priority
  std::vector<uint32_t> order;
  std::vector<int> slot_of_rank;
  for (int dist = 0; dist < nb; ++dist)
    for (int I = 0; I + dist < nb; ++I) {
      order.push_back((uint32_t)I | (uint32_t)(I + dist) << 16);
      slot_of_rank.push_back(pair_slot(nb, I, I + dist));
    }
  std::vector<uint16_t> lev16((size_t)p * d);
  for (size_t k = 0; k < lev16.size(); ++k) {
    if (t.lev[k] > 65535u) return 0;  // (no such model; nothing skipped)
    lev16[k] = (uint16_t)t.lev[k];
  }
  DevBuf<uint16_t> dlev;
  DevBuf<uint32_t> dorder;
  OB_TRY(dlev.upload(lev16.data(), lev16.size()));
  OB_TRY(dorder.upload(order.data(), order.size()));
  // the temporaries in ONE allocation (allocating and freeing eight took 12 of the analysis' 14 ms):
  // keys and values in and out, segment heads, sources (32 bytes an entry), a byte per tile pair,
  // the sort's own storage
  size_t sort_b = 0, scan_b = 0;
  OB_HIP(rocprim::radix_sort_pairs(nullptr, sort_b, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                   (uint32_t *)nullptr, (size_t)n, 0u, 64u, st));
  OB_HIP(rocprim::inclusive_scan(nullptr, scan_b, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n,
                                 rocprim::maximum<uint32_t>(), st));
  const size_t keep_b = ((size_t)npairs + 255) / 256 * 256;
  DevBuf<char> arena;
  OB_TRY(arena.alloc((size_t)n * 32 + keep_b + std::max(sort_b, scan_b) + 256));
  uint64_t *keys0 = (uint64_t *)arena.p, *keys1 = keys0 + n;  // (n is a multiple of 16384: all parts aligned)
  uint32_t *vals0 = (uint32_t *)(keys1 + n), *vals1 = vals0 + n, *head = vals1 + n, *src = head + n;
  uint8_t *keep = (uint8_t *)(src + n);
  char *tmp = (char *)keep + keep_b;
  OB_HIP(hipMemsetAsync(keep, 0, (size_t)npairs, st));
  const unsigned blocks = (n + 255u) / 256u;
  hipLaunchKernelGGL(k_dd_keys, dim3(blocks), dim3(256), 0, st, dlev.p, p, d, dorder.p, n, dd.hashbits, keys0,
                     vals0);
  OB_HIP(hipGetLastError());
  OB_HIP(rocprim::radix_sort_pairs(tmp, sort_b, keys0, keys1, vals0, vals1, (size_t)n, 0u, 64u, st));
  hipLaunchKernelGGL(k_dd_heads, dim3(blocks), dim3(256), 0, st, keys1, n, vals0);
  OB_HIP(hipGetLastError());
  OB_HIP(rocprim::inclusive_scan(tmp, scan_b, vals0, head, (size_t)n, rocprim::maximum<uint32_t>(), st));
  hipLaunchKernelGGL(k_dd_resolve, dim3(blocks), dim3(256), 0, st, dlev.p, p, d, dorder.p, n, keys1, vals1,
                     head, keep, src);
  OB_HIP(hipGetLastError());
  std::vector<uint8_t> keep_h((size_t)npairs);
  OB_TRY(d2h(keep_h.data(), keep, keep_h.size()));
  // never skipped: the diagonal, and the last tile's row and column when it holds padding
  std::vector<uint32_t> pairs;
  std::vector<int> ranks;
  for (int r = 0; r < npairs; ++r) {
    const int I = (int)(order[r] & 0xffffu), J = (int)(order[r] >> 16);
    if (keep_h[r] || I == J || (p % kGT != 0 && J == nb - 1)) continue;
    pairs.push_back(order[r]);
    ranks.push_back(r);
    dd.skip[slot_of_rank[r]] = 1;
  }
  dd.nskip = (int)pairs.size();
  if (dd.nskip > 0) {
    OB_TRY(dd.pairs.upload(pairs.data(), pairs.size()));
    OB_TRY(dd.skip_dev.upload(dd.skip.data(), dd.skip.size()));
    OB_TRY(dd.src.alloc((size_t)dd.nskip * kTileEntries));
    for (int k = 0; k < dd.nskip; ++k)
      OB_HIP(hipMemcpyAsync(dd.src.p + (size_t)k * kTileEntries, src + (size_t)ranks[k] * kTileEntries,
                            kTileEntries * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    OB_HIP(hipStreamSynchronize(st));
    static std::atomic<uint64_t> serial{0};  // exact key of the task tables built on this mask
    dd.sig = ++serial;
  }
  dd.analysis_ms = HostTimer::now() - t0;
  return 0;
}

}  // namespace

// The analysis of t's term set (run on first use, kept with the terms); *out = nullptr when
// nothing is skipped: OBHIP_GRAM_DEDUP=0, too few or too many tile pairs, or no redundant pair.
int gram_dedup_get(obhip_terms &t, const GramDedup **out) {
  *out = nullptr;
  if (const char *e = getenv("OBHIP_GRAM_DEDUP"))
    if (atoi(e) == 0) return 0;
  GramDedup &dd = t.dedup;
  const int hashbits = dedup_hashbits();
  if (!dd.tried || dd.hashbits != hashbits) {
    dd.nskip = 0;
    dd.sig = 0;
    dd.dealing = GramDedup::Dealing();
    dd.analysis_ms = 0.0;
    dd.tried = true;
    dd.hashbits = hashbits;
    dd.nb = (int)((t.p + kGT - 1) / kGT);
    dd.npairs = dd.nb * (dd.nb + 1) / 2;
    dd.skip.assign((size_t)dd.npairs, 0);
    const uint64_t n = (uint64_t)dd.npairs * kTileEntries;
    size_t free_b = 0, total_b = 0;
    // three tiles at least; temporaries (32 bytes an entry + the sort's, budgeted as 36) within an eighth of
    // the free memory (p = 16384: 2.2e9 entries, not analysed)
    const bool fits = n <= kMaxEntries && hipMemGetInfo(&free_b, &total_b) == hipSuccess && n * 36 <= free_b / 8;
    if (dd.nb >= 3 && fits) {
      const int rc = analyse(t, dd);
      if (rc) {
        dd.nskip = 0;
        return rc;
      }
    }
  }
  if (dd.nskip > 0) *out = &dd;
  return 0;
}

// the fill table as a p x p array of linear source indices (-1: not an entry of a skipped tile pair)
int dedup_table(const GramDedup &dd, uint64_t p, int64_t *d_src) {
  const uint32_t *pairs = dd.pairs.p, *src = dd.src.p;
  return vmap((uint64_t)dd.nskip * kTileEntries, [=] __device__(uint64_t w) {
    const uint32_t ij = pairs[w / kTileEntries], q = src[w];
    const uint64_t s = (uint64_t)(ij & 0xffffu) * kGT + ((w >> 7) & 127u), tt = (uint64_t)(ij >> 16) * kGT + (w & 127u);
    if (s < p && tt < p && q != ~0u) d_src[s * p + tt] = (int64_t)((uint64_t)(q >> 16) * p + (q & 0xffffu));
  });
}

int launch_gram_fill(const GramDedup &dd, int p, const GramSink &sink) {
  ProfScope ps("gram_fill");
  hipLaunchKernelGGL(k_gram_fill, dim3((unsigned)dd.nskip, 8), dim3(256), 0, cur_stream(), dd.pairs.p, dd.src.p,
                     (uint32_t)p, sink.out, sink.packed ? 1 : 0);
  OB_HIP(hipGetLastError());
  return 0;
}

}  // namespace obhip

using namespace obhip;

extern "C" {

int obhip_gram_dedup_info(const obhip_terms *tc, uint64_t *tile_pairs, uint64_t *skipped, double *analysis_ms) {
  if (!tc) return fail(OBHIP_ERR_INVALID, "gram_dedup_info: null argument");
  OB_TRY(require_device());
  obhip_terms &t = *const_cast<obhip_terms *>(tc);
  const GramDedup *dd = nullptr;
  OB_TRY(gram_dedup_get(t, &dd));
  const uint64_t nb = (t.p + kGT - 1) / kGT;
  if (tile_pairs) *tile_pairs = nb * (nb + 1) / 2;
  if (skipped) *skipped = dd ? (uint64_t)dd->nskip : 0;
  if (analysis_ms) *analysis_ms = t.dedup.tried ? t.dedup.analysis_ms : 0.0;
  return 0;
}

int obhip_gram_dedup_table_dev(const obhip_terms *tc, int64_t *d_src) {
  if (!tc || !d_src) return fail(OBHIP_ERR_INVALID, "gram_dedup_table_dev: null argument");
  OB_TRY(require_device());
  obhip_terms &t = *const_cast<obhip_terms *>(tc);
  const GramDedup *dd = nullptr;
  OB_TRY(gram_dedup_get(t, &dd));
  const uint64_t p = t.p;
  OB_HIP(hipMemsetAsync(d_src, 0xff, p * p * sizeof(int64_t), cur_stream()));  // -1
  if (!dd) return 0;
  return dedup_table(*dd, p, d_src);
}

}  // extern "C"
