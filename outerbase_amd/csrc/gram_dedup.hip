// Which 128 x 128 tile pairs of G = B^T B -- and, one level finer, which 64 x 64 wave tiles -- hold nothing
// that is not somewhere else in G.
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
//
// The same pipeline with a tile edge of 64 (`lg` = 6 in place of 7) numbers the entries by the 64 x 64 tile
// one WAVE of the kernel computes, in the same order of priority over the 2 nb column groups: one keep byte
// per wave tile, sources in kept wave tiles.  The wave tiles of the diagonal tile pairs and those that touch
// padding columns are kept by rule.  gram_plan.h packs what is kept into blocks (gram_quads_pack); a launch
// takes that plan when gram_quads_get says it pays.
#include <string.h>  // (memset for rocprim's headers)

#include <rocprim/rocprim.hpp>

#include <algorithm>

#include "obhip_internal.h"
#include "vec_ops.h"

namespace obhip {

namespace {

constexpr int kGT = kGramTile;
constexpr int kLgPair = 7, kLgWave = 6;  // log2 of the tile edge of either granularity
constexpr uint32_t kTileEntries = kGT * kGT;
constexpr uint64_t kNoKey = ~0ull;  // padding, and the lower half of diagonal tiles
// entries of all tile pairs above which the analysis is not run (p = 8192: 34 million; its
// temporaries take 32 bytes an entry and the sort's own storage, budgeted as 36)
constexpr uint64_t kMaxEntries = 48ull << 20;
// What the analysis at wave-tile granularity and the packing of its plan cost a term set, once, in host wall
// time: 2.0 ms measured at the headline set, half as much again for the run-to-run
// spread of such a figure.  The packed plan is taken when it is modelled to save more than this in ONE launch.
constexpr double kQuadsSetupMs = 3.0;
constexpr double kBlockTileMs = 0.0146;  // a block's time per row tile (gram_cost's unit), DESIGN.md section 8

__device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64's finaliser
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// entry e = rank << 2 lg | row << lg | column of the tile order[rank] = I | J << 16 (edge 1 << lg)
__device__ __forceinline__ bool dd_entry(uint32_t e, const uint32_t *__restrict__ order, uint32_t p, int lg, uint32_t &s,
                                         uint32_t &t) {
  const uint32_t ij = order[e >> (2 * lg)], I = ij & 0xffffu, J = ij >> 16, m = (1u << lg) - 1u;
  s = (I << lg) + ((e >> lg) & m);
  t = (J << lg) + (e & m);
  return s < p && t < p && s <= t;
}

__global__ void __launch_bounds__(256)
k_dd_keys(const uint16_t *__restrict__ lev, uint32_t p, uint32_t d, const uint32_t *__restrict__ order, uint32_t n,
          int lg, int hashbits, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n) return;
  uint32_t s, t;
  uint64_t key = kNoKey;
  if (dd_entry(e, order, p, lg, s, t)) {
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
             int lg, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
             const uint32_t *__restrict__ head, uint8_t *__restrict__ keep, uint32_t *__restrict__ src) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t e = vals[i];
  src[e] = ~0u;
  if (keys[i] == kNoKey) return;  // (their tiles are kept by rule)
  const uint32_t h = vals[head[i]];
  bool same = false;
  uint32_t s, t, hs = 0, ht = 0;
  if ((h >> (2 * lg)) != (e >> (2 * lg))) {  // stable sort: the head's tile comes first in priority
    dd_entry(e, order, p, lg, s, t);
    dd_entry(h, order, p, lg, hs, ht);
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
    keep[e >> (2 * lg)] = 1;
}

// ---- the sequential pass (gram_order.h has the serial definition) ------------------------------------------
// k_seq_classes  in place of k_dd_resolve: the class of an entry is the start of its segment after the sort.
//                An entry whose actual level pairs are those of its segment's head, the head no diagonal entry
//                of G, is counted in its class; any other (a collision, a duplicate term's class) makes its
//                tile stay and is no one's source.
// k_seq_single   a tile that holds the only occurrence of a class can never drop: it stays, and the walk does
//                not visit it (the walk would take its entries off, find a zero and put them back).
// k_seq_walk     ONE workgroup walks the other tiles from the largest b - a down: entries off the counts,
//                barrier, none of their classes at zero?, back on failure.  The counts sit in the L2 (atomics,
//                so the lanes of a tile that share a class count every occurrence); the read-back of a count
//                is an atomic too, so it sees what the L2 holds.
// k_seq_sources  a dropped entry's source: the first entry of its segment that is counted and whose tile
//                survived -- the stable sort left every segment in the order of priority.
constexpr uint32_t kNoClass = ~0u;
constexpr int kWalkThreads = 1024;

__global__ void __launch_bounds__(256)
k_seq_classes(const uint16_t *__restrict__ lev, uint32_t p, uint32_t d, const uint32_t *__restrict__ order, uint32_t n,
              const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, const uint32_t *__restrict__ head,
              uint32_t *__restrict__ cls, uint32_t *__restrict__ cnt, uint8_t *__restrict__ stays) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t e = vals[i];
  cls[e] = kNoClass;
  if (keys[i] == kNoKey) return;  // (padding, the lower half of diagonal tiles: kept by rule)
  uint32_t s, t, hs, ht;
  dd_entry(e, order, p, kLgWave, s, t);
  dd_entry(vals[head[i]], order, p, kLgWave, hs, ht);
  const uint16_t *ls = lev + (size_t)s * d, *lt = lev + (size_t)t * d;
  const uint16_t *ms = lev + (size_t)hs * d, *mt = lev + (size_t)ht * d;
  bool same = hs != ht;
  for (uint32_t k = 0; k < d && same; ++k) {
    const uint32_t a = ls[k], b = lt[k], a2 = ms[k], b2 = mt[k];
    same = min(a, b) == min(a2, b2) && max(a, b) == max(a2, b2);
  }
  if (same) {
    cls[e] = head[i];
    atomicAdd(&cnt[head[i]], 1u);
  } else {
    stays[e >> (2 * kLgWave)] = 1;
  }
}

__global__ void __launch_bounds__(256)
k_seq_single(const uint32_t *__restrict__ cls, const uint32_t *__restrict__ cnt, uint32_t n, uint8_t *__restrict__ stays) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n) return;
  const uint32_t c = cls[e];
  if (c != kNoClass && cnt[c] < 2u) stays[e >> (2 * kLgWave)] = 1;
}

__global__ void __launch_bounds__(kWalkThreads)
k_seq_walk(const uint32_t *__restrict__ cls, uint32_t *__restrict__ cnt, const uint8_t *__restrict__ stays, int ng,
           uint32_t p, uint8_t *__restrict__ gone) {
  constexpr int kPer = 64 * 64 / kWalkThreads;
  for (int dist = ng - 1; dist >= 1; --dist)
    for (int a = 0; a + dist < ng; ++a) {
      const int b = a + dist, rank = wave_rank(ng, a, b);
      if (a / 2 == b / 2 || (uint32_t)(b + 1) * 64u > p || stays[rank]) continue;  // (uniform)
      // (every entry of such a tile is counted: an uncounted one would have made it stay)
      const uint32_t *c = cls + ((size_t)rank << (2 * kLgWave));
      uint32_t mine[kPer];
#pragma unroll
      for (int k = 0; k < kPer; ++k) {
        mine[k] = c[threadIdx.x + k * kWalkThreads];
        atomicSub(&cnt[mine[k]], 1u);
      }
      __syncthreads();
      int ok = 1;
#pragma unroll
      for (int k = 0; k < kPer; ++k) ok &= atomicAdd(&cnt[mine[k]], 0u) >= 1u ? 1 : 0;
      if (__syncthreads_and(ok)) {
        if (threadIdx.x == 0) gone[rank] = 1;
      } else {
#pragma unroll
        for (int k = 0; k < kPer; ++k) atomicAdd(&cnt[mine[k]], 1u);
      }
      __syncthreads();
    }
}

__global__ void __launch_bounds__(256)
k_seq_sources(const uint32_t *__restrict__ ranks, uint32_t ndrop, uint32_t p, const uint32_t *__restrict__ order,
              uint32_t n, const uint32_t *__restrict__ vals, const uint32_t *__restrict__ head,
              const uint32_t *__restrict__ cls, const uint8_t *__restrict__ gone, uint32_t *__restrict__ src) {
  constexpr uint32_t kWaveEntries = 64 * 64;
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w >= ndrop * kWaveEntries) return;
  const uint32_t e = ranks[w / kWaveEntries] * kWaveEntries + w % kWaveEntries, c = cls[e];
  uint32_t q = ~0u;
  for (uint32_t j = c; c != kNoClass && j < n && head[j] == c; ++j) {
    const uint32_t f = vals[j];
    if (cls[f] != c || gone[f >> (2 * kLgWave)]) continue;
    uint32_t s, t;
    dd_entry(f, order, p, kLgWave, s, t);
    q = s << 16 | t;
    break;
  }
  src[w] = q;
}

// G[s][t] = G[t][s] = G[s'][t'] for every entry of the skipped tiles of edge 1 << LG: tile pairs, or wave
// tiles (row-major or packed sink).  PERM: the tiles and their sources are in Gram order (gram_order.h); entry
// and source go through perm to their terms, the packed sink takes (min, max) of either.
template <int LG, bool PERM>
__global__ void __launch_bounds__(256)
k_gram_fill(const uint32_t *__restrict__ pairs, const uint32_t *__restrict__ src, uint32_t p,
            double *__restrict__ G, int packed, const uint32_t *__restrict__ perm) {
  constexpr uint32_t edge = 1u << LG, entries = edge * edge;
  const uint32_t ij = pairs[blockIdx.x], I = ij & 0xffffu, J = ij >> 16;
  const uint32_t *tab = src + (size_t)blockIdx.x * entries;
  for (uint32_t w = blockIdx.y * 256u + threadIdx.x; w < entries; w += gridDim.y * 256u) {
    uint32_t s = I * edge + (w >> LG), t = J * edge + (w & (edge - 1u));
    uint32_t q = tab[w], ss = q >> 16, st = q & 0xffffu;
    if (s >= p || t >= p || ss >= p || st >= p || ss > st) continue;  // (never: skipped tiles hold no padding)
    if constexpr (PERM) {
      const uint32_t a = perm[s], b = perm[t], sa = perm[ss], sb = perm[st];
      s = min(a, b), t = max(a, b), ss = min(sa, sb), st = max(sa, sb);
    }
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

std::atomic<uint64_t> g_mask_serial{0};  // exact key of the task tables built on a mask

// One run of the pipeline over the tiles of edge 1 << lg that `order` lists by priority (I | J << 16).
// keep[rank] = 1: the tile holds a canonical occurrence (or a collision); src: the sources, rank-major, in
// the arena until it goes.  ok = false: levels beyond 16 bits (no such model), nothing analysed.
// seq (wave tiles only): the sequential pass in place of the parallel rule -- keep[rank] = 0: the tile dropped;
// its sources come from seq_sources afterwards, while the arena stands.
struct DdRun {
  bool ok = false;
  DevBuf<char> arena;
  DevBuf<uint16_t> dlev;
  DevBuf<uint32_t> dorder;
  uint32_t *src = nullptr;
  std::vector<uint8_t> keep;
  // the sequential pass: sorted values and segment starts, the class of every entry, the dropped tiles
  uint32_t n = 0;
  const uint32_t *vals = nullptr, *head = nullptr, *cls = nullptr;
  const uint8_t *gone = nullptr;
};
int run_pipeline(const uint32_t *lev, uint64_t p64, uint64_t d64, int lg, const std::vector<uint32_t> &order, int hashbits,
                 DdRun &run, bool seq = false) {
  const uint32_t p = (uint32_t)p64, d = (uint32_t)d64;
  const size_t ntile = order.size();
  const uint32_t n = (uint32_t)ntile << (2 * lg);
  hipStream_t st = cur_stream();
  std::vector<uint16_t> lev16((size_t)p * d);
  for (size_t k = 0; k < lev16.size(); ++k) {
    if (lev[k] > 65535u) return 0;  // (no such model; nothing skipped)
    lev16[k] = (uint16_t)lev[k];
  }
  DevBuf<uint16_t> &dlev = run.dlev;
  DevBuf<uint32_t> &dorder = run.dorder;
  OB_TRY(dlev.upload(lev16.data(), lev16.size()));
  OB_TRY(dorder.upload(order.data(), order.size()));
  // the temporaries in ONE allocation (allocating and freeing eight took 12 of the analysis' 14 ms):
  // keys and values in and out, segment heads, sources (32 bytes an entry), a byte per tile,
  // the sort's own storage
  size_t sort_b = 0, scan_b = 0;
  OB_HIP(rocprim::radix_sort_pairs(nullptr, sort_b, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                   (uint32_t *)nullptr, (size_t)n, 0u, 64u, st));
  OB_HIP(rocprim::inclusive_scan(nullptr, scan_b, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n,
                                 rocprim::maximum<uint32_t>(), st));
  const size_t keep_b = (ntile + 255) / 256 * 256 * 2;  // (the sequential pass: a second byte per tile)
  OB_TRY(run.arena.alloc((size_t)n * 32 + keep_b + std::max(sort_b, scan_b) + 256));
  uint64_t *keys0 = (uint64_t *)run.arena.p, *keys1 = keys0 + n;  // (n is a multiple of 4096: all parts aligned)
  uint32_t *vals0 = (uint32_t *)(keys1 + n), *vals1 = vals0 + n, *head = vals1 + n, *src = head + n;
  uint8_t *keep = (uint8_t *)(src + n);
  char *tmp = (char *)keep + keep_b;
  OB_HIP(hipMemsetAsync(keep, 0, ntile, st));
  const unsigned blocks = (n + 255u) / 256u;
  hipLaunchKernelGGL(k_dd_keys, dim3(blocks), dim3(256), 0, st, dlev.p, p, d, dorder.p, n, lg, hashbits, keys0,
                     vals0);
  OB_HIP(hipGetLastError());
  OB_HIP(rocprim::radix_sort_pairs(tmp, sort_b, keys0, keys1, vals0, vals1, (size_t)n, 0u, 64u, st));
  hipLaunchKernelGGL(k_dd_heads, dim3(blocks), dim3(256), 0, st, keys1, n, vals0);
  OB_HIP(hipGetLastError());
  OB_HIP(rocprim::inclusive_scan(tmp, scan_b, vals0, head, (size_t)n, rocprim::maximum<uint32_t>(), st));
  if (seq) {
    // keys0 and vals0 are free now: the counts by segment start, the class of every entry; the tile bytes are
    // "stays" and, behind them, "gone"
    uint32_t *cnt = (uint32_t *)keys0, *cls = vals0;
    uint8_t *stays = keep, *gone = keep + keep_b / 2;
    OB_HIP(hipMemsetAsync(cnt, 0, (size_t)n * sizeof(uint32_t), st));
    OB_HIP(hipMemsetAsync(gone, 0, ntile, st));
    hipLaunchKernelGGL(k_seq_classes, dim3(blocks), dim3(256), 0, st, dlev.p, p, d, dorder.p, n, keys1, vals1, head,
                       cls, cnt, stays);
    OB_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_seq_single, dim3(blocks), dim3(256), 0, st, cls, cnt, n, stays);
    OB_HIP(hipGetLastError());
    const int ng = (int)((p + kGT - 1) / kGT) * 2;
    hipLaunchKernelGGL(k_seq_walk, dim3(1), dim3(kWalkThreads), 0, st, cls, cnt, stays, ng, p, gone);
    OB_HIP(hipGetLastError());
    run.keep.resize(ntile);
    OB_TRY(d2h(run.keep.data(), gone, ntile));
    for (uint8_t &k : run.keep) k = k ? 0 : 1;
    run.src = src;
    run.n = n, run.vals = vals1, run.head = head, run.cls = cls, run.gone = gone;
    run.ok = true;
    return 0;
  }
  hipLaunchKernelGGL(k_dd_resolve, dim3(blocks), dim3(256), 0, st, dlev.p, p, d, dorder.p, n, lg, keys1, vals1,
                     head, keep, src);
  OB_HIP(hipGetLastError());
  run.keep.resize(ntile);
  OB_TRY(d2h(run.keep.data(), keep, ntile));
  run.src = src;
  run.ok = true;
  return 0;
}

int analyse(obhip_terms &t, GramDedup &dd) {
  const double t0 = HostTimer::now();
  const uint32_t p = (uint32_t)t.p;
  const int nb = dd.nb, npairs = dd.npairs;
  hipStream_t st = cur_stream();
  // tile pairs in the order of priority
  std::vector<uint32_t> order;
  std::vector<int> slot_of_rank;
  for (int dist = 0; dist < nb; ++dist)
    for (int I = 0; I + dist < nb; ++I) {
      order.push_back((uint32_t)I | (uint32_t)(I + dist) << 16);
      slot_of_rank.push_back(pair_slot(nb, I, I + dist));
    }
  DdRun run;
  OB_TRY(run_pipeline(t.lev.data(), t.p, t.d, kLgPair, order, dd.hashbits, run));
  if (!run.ok) return 0;
  // never skipped: the diagonal, and the last tile's row and column when it holds padding
  std::vector<uint32_t> pairs;
  std::vector<int> ranks;
  for (int r = 0; r < npairs; ++r) {
    const int I = (int)(order[r] & 0xffffu), J = (int)(order[r] >> 16);
    if (run.keep[r] || I == J || (p % kGT != 0 && J == nb - 1)) continue;
    pairs.push_back(order[r]);
    ranks.push_back(r);
    dd.skip[slot_of_rank[r]] = 1;
  }
  dd.nskip = (int)pairs.size();
  if (dd.nskip > 0) {
    OB_TRY(dd.pairs.upload(pairs.data(), pairs.size()));
    // (k_gram_reduce reads a bit per quadrant: all four of a skipped pair)
    std::vector<uint8_t> quadrants(dd.skip.size());
    for (size_t k = 0; k < quadrants.size(); ++k) quadrants[k] = dd.skip[k] ? 0x0f : 0;
    OB_TRY(dd.skip_dev.upload(quadrants.data(), quadrants.size()));
    OB_TRY(dd.src.alloc((size_t)dd.nskip * kTileEntries));
    for (int k = 0; k < dd.nskip; ++k)
      OB_HIP(hipMemcpyAsync(dd.src.p + (size_t)k * kTileEntries, run.src + (size_t)ranks[k] * kTileEntries,
                            kTileEntries * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    OB_HIP(hipStreamSynchronize(st));
    dd.sig = ++g_mask_serial;
  }
  dd.analysis_ms = HostTimer::now() - t0;
  return 0;
}

// the same at wave-tile granularity: q.keep, the dropped wave tiles with their sources, the quadrant bits of
// the reduction, and the blocks per split the packed plan needs
// lev: the p x d levels in the order the columns are staged in (the terms' own, or Gram order with seq = true:
// the sequential pass decides)
int analyse_quads(const uint32_t *lev, uint64_t p64, uint64_t d, GramDedup::Quads &q, int nb, bool seq = false) {
  const double t0 = HostTimer::now();
  const uint32_t p = (uint32_t)p64;
  const int ng = 2 * nb;
  constexpr uint32_t kWaveEntries = 64 * 64;
  hipStream_t st = cur_stream();
  std::vector<uint32_t> order;
  for (int dist = 0; dist < ng; ++dist)
    for (int a = 0; a + dist < ng; ++a) order.push_back((uint32_t)a | (uint32_t)(a + dist) << 16);
  DdRun run;
  OB_TRY(run_pipeline(lev, p64, d, kLgWave, order, q.hashbits, run, seq));
  if (!run.ok) return 0;
  // never dropped: the wave tiles of the diagonal tile pairs, and those that reach into the padding columns
  std::vector<uint32_t> tiles, ranks;
  for (size_t r = 0; r < order.size(); ++r) {
    const int a = (int)(order[r] & 0xffffu), b = (int)(order[r] >> 16);
    if (run.keep[r] || a / 2 == b / 2 || (uint32_t)(b + 1) * 64u > p) continue;
    tiles.push_back(order[r]);
    ranks.push_back((uint32_t)r);
    q.keep[(size_t)pair_slot(ng, a, b)] = 0;
  }
  q.ndrop = (int)tiles.size();
  if (q.ndrop > 0) {
    std::vector<uint8_t> quadrants(gram_npairs(nb), 0);
    for (uint32_t ab : tiles) {
      const int a = (int)(ab & 0xffffu), b = (int)(ab >> 16);
      quadrants[(size_t)pair_slot(nb, a / 2, b / 2)] |= (uint8_t)(1u << (2 * (a & 1) + (b & 1)));
    }
    DevBuf<uint32_t> dranks;
    OB_TRY(q.tiles.upload(tiles.data(), tiles.size()));
    OB_TRY(dranks.upload(ranks.data(), ranks.size()));
    OB_TRY(q.qskip_dev.upload(quadrants.data(), quadrants.size()));
    OB_TRY(q.src.alloc((size_t)q.ndrop * kWaveEntries));
    uint32_t *dst = q.src.p;
    const uint32_t *from = run.src, *rk = dranks.p;
    if (seq) {
      hipLaunchKernelGGL(k_seq_sources, dim3((unsigned)q.ndrop * (kWaveEntries / 256)), dim3(256), 0, st, rk,
                         (uint32_t)q.ndrop, p, run.dorder.p, run.n, run.vals, run.head, run.cls, run.gone, dst);
      OB_HIP(hipGetLastError());
    } else {
      OB_TRY(vmap((uint64_t)q.ndrop * kWaveEntries, [=] __device__(uint64_t w) {
        dst[w] = from[(uint64_t)rk[w / kWaveEntries] * kWaveEntries + w % kWaveEntries];
      }));
    }
    OB_HIP(hipStreamSynchronize(st));
    q.sig = ++g_mask_serial;
    std::vector<QuadBlock> blocks;
    gram_quads_pack(nb, q.keep.data(), blocks);
    q.blocks = (int)blocks.size();
  }
  q.setup_ms = HostTimer::now() - t0;
  return 0;
}

bool dedup_off() {
  const char *e = getenv("OBHIP_GRAM_DEDUP");
  return e && atoi(e) == 0;
}
// OBHIP_GRAM_DEDUP_QUADS: 1 forces the plan at wave-tile granularity, 0 forbids it, unset (-1) lets the model decide
int quads_mode() {
  const char *e = getenv("OBHIP_GRAM_DEDUP_QUADS");
  return e ? (atoi(e) != 0 ? 1 : 0) : -1;
}

// t's analysis at wave-tile granularity, run on first use and kept with the terms (ndrop = 0: nothing to
// drop, fewer than two tiles, or too many entries)
int quads_analysis(obhip_terms &t, GramDedup::Quads **out) {
  GramDedup::Quads &q = t.dedup.quads;
  *out = &q;
  const int hashbits = dedup_hashbits();
  if (q.tried && q.hashbits == hashbits) return 0;
  const int nb = (int)((t.p + kGT - 1) / kGT);
  q.ndrop = q.blocks = q.blocks_pairs = 0;
  q.sig = 0;
  q.setup_ms = 0.0;
  q.engaged = false;
  q.key = GramKey();
  q.tried = true;
  q.hashbits = hashbits;
  q.keep.assign(gram_npairs(2 * nb), 1);
  const uint64_t n = gram_npairs(2 * nb) * 64 * 64;
  size_t free_b = 0, total_b = 0;
  const bool fits = n <= kMaxEntries && hipMemGetInfo(&free_b, &total_b) == hipSuccess && n * 36 <= free_b / 8;
  if (nb >= 2 && fits) {
    const int rc = analyse_quads(t.lev.data(), t.p, t.d, q, nb);
    if (rc) {
      q.ndrop = 0;
      return rc;
    }
  }
  return 0;
}

// OBHIP_GRAM_ORDER: 1 forces the Gram's own column order, 0 forbids it, unset (-1) lets the model decide
int order_mode() {
  const char *e = getenv("OBHIP_GRAM_ORDER");
  return e ? (atoi(e) != 0 ? 1 : 0) : -1;
}

std::atomic<uint64_t> g_order_serial{0};

// t's Gram order and its analysis in Gram coordinates, built on first use and kept with the terms (quads.tried
// and nothing analysed: fewer than two tiles, or too many entries)
int order_analysis(obhip_terms &t) {
  GramOrder &o = t.order;
  GramDedup::Quads &q = o.quads;
  const int hashbits = dedup_hashbits();
  if (o.tried && q.tried && q.hashbits == hashbits) return 0;
  const double t0 = HostTimer::now();
  const int nb = (int)((t.p + kGT - 1) / kGT);
  if (!o.tried) {
    o.perm = gram_order_perm(t.lev.data(), t.p, t.d);
    o.identity = gram_perm_is_identity(o.perm);
    o.inv = gram_perm_inverse(o.perm);
    std::vector<uint32_t> padded(o.perm);
    for (uint64_t k = t.p; k < (uint64_t)nb * kGT; ++k) padded.push_back((uint32_t)k);  // the padding columns stay last
    OB_TRY(o.perm_dev.upload(padded.data(), padded.size()));
    o.serial = ++g_order_serial;
    o.tried = true;
  }
  q.ndrop = q.blocks = q.blocks_pairs = 0;
  q.sig = 0;
  q.setup_ms = 0.0;
  q.engaged = false;
  q.key = GramKey();
  q.tried = true;
  q.hashbits = hashbits;
  q.keep.assign(gram_npairs(2 * nb), 1);
  // (an earlier analysis' quadrant bits, tiles and sources must not outlive it: a forced order whose new
  // analysis drops nothing still runs, and the reduction would skip the quadrants of the old mask)
  q.qskip_dev.release();
  q.tiles.release();
  q.src.release();
  const uint64_t n = gram_npairs(2 * nb) * 64 * 64;
  size_t free_b = 0, total_b = 0;
  const bool fits = n <= kMaxEntries && hipMemGetInfo(&free_b, &total_b) == hipSuccess && n * 36 <= free_b / 8;
  if (nb >= 2 && fits) {
    const std::vector<uint32_t> lev = gram_perm_levels(t.lev.data(), t.d, o.perm);
    const int rc = analyse_quads(lev.data(), t.p, t.d, q, nb, true);
    if (rc) {
      q.ndrop = 0;
      return rc;
    }
    if (q.ndrop == 0) {  // (a forced order runs the packed plan of all wave tiles)
      q.sig = ++g_mask_serial;
      std::vector<QuadBlock> blocks;
      gram_quads_pack(nb, q.keep.data(), blocks);
      q.blocks = (int)blocks.size();
    }
  }
  q.setup_ms = HostTimer::now() - t0;
  return 0;
}

// The order's plan runs: the term set's latest Gram launch recorded that it did (GramOrder::last_launch), and the
// switch and the analysis still stand.  Forced and no launch yet: the next one will, if its analysis ran -- a launch
// that then cannot take the order (no staging kernel for it, another Gram back end) records that it did not.
int order_runs(obhip_terms &t, bool *runs) {
  *runs = false;
  const int mode = gram_order_mode();
  if (mode == 0 || t.order.last_launch == 0) return 0;
  if (mode == 1) OB_TRY(order_analysis(t));
  const GramDedup::Quads &q = t.order.quads;
  const bool stands = t.order.tried && q.tried && q.hashbits == dedup_hashbits() && q.sig != 0;
  *runs = stands && (mode == 1 || (q.engaged && t.order.last_launch == 1));
  return 0;
}

template <int LG>
int dedup_table(const uint32_t *tiles, const uint32_t *src, uint64_t ntile, uint64_t p, int64_t *d_src) {
  return vmap(ntile << (2 * LG), [=] __device__(uint64_t w) {
    const uint32_t ij = tiles[w >> (2 * LG)], q = src[w], m = (1u << LG) - 1u;
    const uint64_t s = ((uint64_t)(ij & 0xffffu) << LG) + ((w >> LG) & m), tt = ((uint64_t)(ij >> 16) << LG) + (w & m);
    if (s < p && tt < p && q != ~0u) d_src[s * p + tt] = (int64_t)((uint64_t)(q >> 16) * p + (q & 0xffffu));
  });
}

}  // namespace

// The analysis of t's term set (run on first use, kept with the terms); *out = nullptr when
// nothing is skipped: OBHIP_GRAM_DEDUP=0, too few or too many tile pairs, or no redundant pair.
int gram_dedup_get(obhip_terms &t, const GramDedup **out) {
  *out = nullptr;
  if (dedup_off()) return 0;
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

// Whether the launch of `shape` at `plan` (the split, and the dealing the whole-pair plan takes with its mask
// `skip`, may be null) runs the packed plan at wave-tile granularity instead.  Forced: whenever a wave tile can
// be dropped.  Otherwise only when the plan saves a block per split and, by gram_cost at kBlockTileMs a row tile,
// more time in this one launch than its set-up cost the term set; a launch whose whole modelled time is below
// that is not even analysed.  The decision is kept with the analysis until shape, split or mask change.
int gram_quads_get(obhip_terms &t, const GramShape &shape, const GramPlan &plan, const uint8_t *skip, uint64_t skip_sig,
                   const GramDedup::Quads **out) {
  *out = nullptr;
  GramDedup::Quads &q0 = t.dedup.quads;
  const int mode = dedup_off() ? 0 : quads_mode();
  if (mode == 0) {
    q0.engaged = false;
    q0.key = GramKey();
    return 0;
  }
  const GramKey key = {shape, plan.nsplit, skip_sig, 2 * mode + (plan.continuous ? 1 : 0)};
  if (q0.key == key) {
    if (q0.engaged) *out = &q0;
    return 0;
  }
  std::vector<uint64_t> tab;
  build_task_order(shape.nb, (int)plan.nsplit, shape.diag4, plan.continuous, skip, tab);
  const double cost_pairs = gram_table_cost(shape, plan.nsplit, plan.continuous, tab);
  if (mode < 0 && cost_pairs * kBlockTileMs <= kQuadsSetupMs) {
    q0.engaged = false;
    q0.key = key;
    return 0;
  }
  GramDedup::Quads *q = nullptr;
  OB_TRY(quads_analysis(t, &q));
  q->key = key;
  q->engaged = false;
  if (q->ndrop == 0) return 0;
  q->blocks_pairs = (int)((tab.size() - (size_t)std::count(tab.begin(), tab.end(), kAtbNoTask)) / plan.nsplit);
  double cost = 0.0;
  q->continuous = gram_quads_choose_dealing(shape, plan.nsplit, q->keep.data(), &cost);
  q->engaged = mode == 1 || (q->blocks + 1 <= q->blocks_pairs && (cost_pairs - cost) * kBlockTileMs > kQuadsSetupMs);
  if (getenv("OBHIP_GRAM_DBG") && atoi(getenv("OBHIP_GRAM_DBG")) != 0)
    fprintf(stderr, "[gram dbg] wave-tile plan: %d dropped, %d blocks per split (whole pairs %d), gram_cost %.1f -> %.1f, "
                    "set-up %.2f ms, %s\n", q->ndrop, q->blocks, q->blocks_pairs, cost_pairs, cost, q->setup_ms,
            q->engaged ? "engaged" : "not engaged");
  if (q->engaged) *out = q;
  return 0;
}

int gram_order_mode() { return dedup_off() ? 0 : order_mode(); }

// Whether the launch of `shape` at `plan` stages and multiplies its columns in Gram order.  Forced: whenever the
// analysis in Gram coordinates ran.  Unset: only beside an unset OBHIP_GRAM_DEDUP_QUADS (a forced or forbidden
// wave-tile plan runs as it always did), and only when gram_order_pays says so; a launch too short to pay is not
// even analysed.  The decision is kept with the order until shape, split, the competing plan or the switch change.
int gram_order_get(obhip_terms &t, const GramShape &shape, const GramPlan &plan, uint64_t other_sig,
                   const std::function<void(double &, int &)> &price_other, const GramOrder **out) {
  *out = nullptr;
  GramDedup::Quads &q = t.order.quads;
  const int mode = gram_order_mode();
  if (mode == 0 || (mode < 0 && quads_mode() >= 0)) {
    q.engaged = false;
    q.key = GramKey();
    return 0;
  }
  const GramKey key = {shape, plan.nsplit, other_sig, 2 * mode + (plan.continuous ? 1 : 0)};
  if (q.key == key && t.order.tried && q.hashbits == dedup_hashbits()) {
    if (q.engaged) *out = &t.order;
    return 0;
  }
  double cost_other = 0.0;
  int blocks_other = 0;
  price_other(cost_other, blocks_other);
  if (mode < 0 && !gram_order_worth_analysing(shape.nb, cost_other, kBlockTileMs)) {
    q.engaged = false;
    q.key = key;
    return 0;
  }
  OB_TRY(order_analysis(t));
  q.key = key;
  q.engaged = false;
  if (q.sig == 0) return 0;  // nothing analysed
  q.blocks_pairs = blocks_other;
  double cost = 0.0;
  q.continuous = gram_quads_choose_dealing(shape, plan.nsplit, q.keep.data(), &cost);
  q.engaged = mode == 1 || (!t.order.identity && gram_order_pays(shape.nb, cost_other, blocks_other, cost, q.blocks, kBlockTileMs));
  if (getenv("OBHIP_GRAM_DBG") && atoi(getenv("OBHIP_GRAM_DBG")) != 0)
    fprintf(stderr, "[gram dbg] Gram order: %d dropped, %d blocks per split (otherwise %d), gram_cost %.1f -> %.1f, "
                    "set-up %.2f ms, %s\n", q.ndrop, q.blocks, blocks_other, cost_other, cost, q.setup_ms,
            q.engaged ? "engaged" : "not engaged");
  if (q.engaged) *out = &t.order;
  return 0;
}

// obhip_terms::cols with its rows in Gram order, gathered anew before every staging (the table is rebuilt
// whenever the column layout changes; 64 KB at the headline)
int gram_order_cols(obhip_terms &t) {
  GramOrder &o = t.order;
  const uint64_t n = t.p_pad * t.W;
  if (o.cols.n < n) OB_TRY(o.cols.alloc(n));
  const uint16_t *from = t.cols.p;
  uint16_t *to = o.cols.p;
  const uint32_t *perm = o.perm_dev.p;
  const uint64_t W = t.W, p = t.p;
  return vmap(n, [=] __device__(uint64_t e) {
    const uint64_t k = e / W;
    to[e] = from[(k < p ? (uint64_t)perm[k] : k) * W + e % W];
  });
}

int launch_gram_fill(const GramDedup &dd, int p, const GramSink &sink) {
  ProfScope ps("gram_fill");
  hipLaunchKernelGGL((k_gram_fill<kLgPair, false>), dim3((unsigned)dd.nskip, 8), dim3(256), 0, cur_stream(), dd.pairs.p,
                     dd.src.p, (uint32_t)p, sink.out, sink.packed ? 1 : 0, nullptr);
  OB_HIP(hipGetLastError());
  return 0;
}

int launch_gram_fill_quads(const GramDedup::Quads &q, int p, const GramSink &sink, const uint32_t *perm) {
  if (q.ndrop == 0) return 0;  // (a forced order with nothing to drop)
  ProfScope ps("gram_fill");
  if (perm)
    hipLaunchKernelGGL((k_gram_fill<kLgWave, true>), dim3((unsigned)q.ndrop, 2), dim3(256), 0, cur_stream(), q.tiles.p,
                       q.src.p, (uint32_t)p, sink.out, sink.packed ? 1 : 0, perm);
  else
    hipLaunchKernelGGL((k_gram_fill<kLgWave, false>), dim3((unsigned)q.ndrop, 2), dim3(256), 0, cur_stream(), q.tiles.p,
                       q.src.p, (uint32_t)p, sink.out, sink.packed ? 1 : 0, nullptr);
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

int obhip_gram_dedup_quads_info(const obhip_terms *tc, uint64_t *wave_tiles, uint64_t *dropped, uint64_t *blocks_per_split,
                                int *engaged) {
  if (!tc) return fail(OBHIP_ERR_INVALID, "gram_dedup_quads_info: null argument");
  OB_TRY(require_device());
  obhip_terms &t = *const_cast<obhip_terms *>(tc);
  const uint64_t ng = 2 * ((t.p + kGT - 1) / kGT);
  bool ordered = false;
  OB_TRY(order_runs(t, &ordered));
  if (ordered) {  // the plan that runs is the order's
    if (wave_tiles) *wave_tiles = ng * (ng + 1) / 2;
    if (dropped) *dropped = (uint64_t)t.order.quads.ndrop;
    if (blocks_per_split) *blocks_per_split = (uint64_t)t.order.quads.blocks;
    if (engaged) *engaged = 1;
    return 0;
  }
  const int mode = dedup_off() ? 0 : quads_mode();
  GramDedup::Quads *q = &t.dedup.quads;
  if (mode == 1) OB_TRY(quads_analysis(t, &q));
  const bool known = mode != 0 && q->tried && q->hashbits == dedup_hashbits();
  if (wave_tiles) *wave_tiles = ng * (ng + 1) / 2;
  if (dropped) *dropped = known ? (uint64_t)q->ndrop : 0;
  if (blocks_per_split) *blocks_per_split = known ? (uint64_t)q->blocks : 0;
  if (engaged) *engaged = known && q->ndrop > 0 && (mode == 1 || q->engaged) ? 1 : 0;
  return 0;
}

int obhip_gram_order_info(const obhip_terms *tc, int *engaged, uint64_t *dropped, uint64_t *blocks_per_split,
                          double *setup_ms) {
  if (!tc) return fail(OBHIP_ERR_INVALID, "gram_order_info: null argument");
  OB_TRY(require_device());
  obhip_terms &t = *const_cast<obhip_terms *>(tc);
  bool ordered = false;
  OB_TRY(order_runs(t, &ordered));
  const GramDedup::Quads &q = t.order.quads;
  if (engaged) *engaged = ordered ? 1 : 0;
  if (dropped) *dropped = ordered ? (uint64_t)q.ndrop : 0;
  if (blocks_per_split) *blocks_per_split = ordered ? (uint64_t)q.blocks : 0;
  if (setup_ms) *setup_ms = q.tried ? q.setup_ms : 0.0;
  return 0;
}

int obhip_gram_dedup_table_dev(const obhip_terms *tc, int64_t *d_src) {
  if (!tc || !d_src) return fail(OBHIP_ERR_INVALID, "gram_dedup_table_dev: null argument");
  OB_TRY(require_device());
  obhip_terms &t = *const_cast<obhip_terms *>(tc);
  const uint64_t p = t.p;
  OB_HIP(hipMemsetAsync(d_src, 0xff, p * p * sizeof(int64_t), cur_stream()));  // -1
  bool ordered = false;
  OB_TRY(order_runs(t, &ordered));
  if (ordered) {  // tiles and sources are in Gram order: entry and source through perm, (min, max) of either
    const GramDedup::Quads &q = t.order.quads;
    const uint32_t *tiles = q.tiles.p, *src = q.src.p, *perm = t.order.perm_dev.p;
    return vmap((uint64_t)q.ndrop << (2 * kLgWave), [=] __device__(uint64_t w) {
      const uint32_t ij = tiles[w >> (2 * kLgWave)], v = src[w], m = (1u << kLgWave) - 1u;
      const uint64_t s = ((uint64_t)(ij & 0xffffu) << kLgWave) + ((w >> kLgWave) & m);
      const uint64_t tt = ((uint64_t)(ij >> 16) << kLgWave) + (w & m);
      if (s >= p || tt >= p || v == ~0u) return;
      const uint64_t a = perm[s], b = perm[tt], sa = perm[v >> 16], sb = perm[v & 0xffffu];
      d_src[min(a, b) * p + max(a, b)] = (int64_t)(min(sa, sb) * p + max(sa, sb));
    });
  }
  int engaged = 0;
  OB_TRY(obhip_gram_dedup_quads_info(tc, nullptr, nullptr, nullptr, &engaged));
  if (engaged) {
    const GramDedup::Quads &q = t.dedup.quads;
    return dedup_table<kLgWave>(q.tiles.p, q.src.p, (uint64_t)q.ndrop, p, d_src);
  }
  const GramDedup *dd = nullptr;
  OB_TRY(gram_dedup_get(t, &dd));
  if (!dd) return 0;
  return dedup_table<kLgPair>(dd->pairs.p, dd->src.p, (uint64_t)dd->nskip, p, d_src);
}

}  // extern "C"
