// Term views and pass groups of the hyper-gradient products (host code).  The reference's products are
//   d B[i,k] / d hyp_h = basescale_i . prod_{m != l} basemat[i, col(m, t_km)] . basemat_gradhyp[i, gest[h] + t_kl]
// (l = hypmatch[h]): the term product with dimension l's factor (the constant 1 at level 0) replaced
// by the gradient column.  So a *view* of the terms with l dropped and a pseudo-dimension of the
// gradient basis (kernels_grad_basis.hip) at level t_kl + 1 lets the value kernels k_mm / k_tmm /
// getmat compute them unchanged.  Also here: the hand-written tables of the fused pass (k_tmm_d3,
// kernels_grad_d3.hip).  Cached in obhip_terms::ge; who contracts what: kernels_grad.hip.
#include <map>
#include <numeric>
#include <set>

#include "obhip_internal.h"
#include "device_common.h"

namespace obhip {

// The terms ix of t (de dimensions with the pseudo-dimensions) with dimension l dropped and
// pseudo-dimension pd in its place, at the term's level in l plus `up`
static std::unique_ptr<obhip_terms> make_view(const obhip_terms &t, const std::vector<uint32_t> &ix, uint64_t de,
                                              uint64_t l, uint64_t pd, uint32_t up) {
  const uint64_t d = t.d;
  auto v = std::make_unique<obhip_terms>();
  v->no_share = true;  // (a view of the caller's terms: the per-hyper-parameter kernels take the plain tables)
  v->p = ix.size();
  v->d = de;
  v->lev.assign(v->p * de, 0);
  v->maxlev.assign(de, 0);
  for (uint64_t j = 0; j < v->p; ++j) {
    const uint64_t k = ix[j];
    uint64_t nnz = 1;
    for (uint64_t q = 0; q < d; ++q) {
      const uint32_t lv = q == l ? 0u : t.lev[k * d + q];
      v->lev[j * de + q] = lv;
      v->maxlev[q] = std::max<int64_t>(v->maxlev[q], lv);
      nnz += lv > 0;
    }
    const uint32_t gl = t.lev[k * d + l] + up;
    v->lev[j * de + pd] = gl;
    v->maxlev[pd] = std::max<int64_t>(v->maxlev[pd], gl);
    v->nnz_total += nnz;
    v->max_nnz = std::max(v->max_nnz, nnz);
  }
  return v;
}

// Views restricted to the terms whose level in hyper-parameter h's dimension is non-zero, the
// pseudo-dimension on the gradient block at level t + 1 (sviews) or on the delta block at level t
// (dviews), sidx their term indices; no view where no term has the dimension.
static void build_sparse_views(obhip_terms &t, const obhip_basis &b) {
  const obhip_model &m = *b.model;
  const uint64_t nh = m.nhyp(), d = t.d, de = d + 2 * nh;
  // (keyed by the dimension of every hyper-parameter: the same terms may meet a basis of another
  // model with as many hyper-parameters laid out differently)
  std::vector<uint64_t> sig(m.hypmatch.begin(), m.hypmatch.end());
  if (t.ge.sviews.size() == nh && t.ge.dviews.size() == nh && t.ge.sig == sig) return;
  t.ge.reset_views(sig, nh);
  for (uint64_t hh = 0; hh < nh; ++hh) {
    const uint64_t l = m.hypmatch[hh];
    std::vector<uint32_t> &ix = t.ge.sidx[hh];
    for (uint64_t k = 0; k < t.p; ++k)
      if (t.lev[k * d + l] > 0) ix.push_back((uint32_t)k);
    if (ix.empty()) continue;
    t.ge.sviews[hh] = make_view(t, ix, de, l, d + hh, 1);
    t.ge.dviews[hh] = make_view(t, ix, de, l, d + nh + hh, 0);
  }
  // The gradient views are contracted a few hyper-parameters at a time: their term lists
  // concatenated into groups whose used columns (the value columns of the other dimensions
  // plus the groups' own gradient columns) stay within what the term-per-lane kernel can
  // prefetch and keep two workgroups per CU on (128 columns).  One list of all of them
  // (round 1) put ~300 columns and 3 p terms into a single pass: one workgroup per CU, no
  // prefetch, 16.5 ms per call at p = 4096, 16 hyper-parameters.
  constexpr size_t kGroupMuCap = 128;
  auto group_views = [&](const std::vector<std::unique_ptr<obhip_terms>> &views,
                         std::vector<obhip_terms::GeGroup> &groups) {
    groups.clear();
    std::set<std::pair<uint32_t, uint32_t>> used;  // (dimension of the view, level > 0)
    auto close_group = [&](obhip_terms::GeGroup &g) {
      if (g.hyps.empty()) return;
      auto v = std::make_unique<obhip_terms>();
      v->no_share = true;  // (a view of the caller's terms: the per-hyper-parameter kernels take the plain tables)
      v->p = g.off.back();
      v->d = de;
      v->lev.resize(v->p * de);
      v->maxlev.assign(de, 0);
      for (size_t j = 0; j < g.hyps.size(); ++j) {
        const obhip_terms *sv = views[g.hyps[j]].get();
        std::copy(sv->lev.begin(), sv->lev.end(), v->lev.begin() + g.off[j] * de);
        for (uint64_t q = 0; q < de; ++q) v->maxlev[q] = std::max(v->maxlev[q], sv->maxlev[q]);
        v->nnz_total += sv->nnz_total;
        v->max_nnz = std::max(v->max_nnz, sv->max_nnz);
      }
      g.v = std::move(v);
      groups.push_back(std::move(g));
    };
    obhip_terms::GeGroup cur;
    cur.off.push_back(0);
    for (uint64_t hh = 0; hh < nh; ++hh) {
      const obhip_terms *sv = views[hh].get();
      if (!sv) continue;
      std::set<std::pair<uint32_t, uint32_t>> mine;
      for (uint64_t j = 0; j < sv->p; ++j)
        for (uint64_t q = 0; q < de; ++q)
          if (sv->lev[j * de + q] > 0) mine.insert({(uint32_t)q, sv->lev[j * de + q]});
      std::set<std::pair<uint32_t, uint32_t>> both = used;
      both.insert(mine.begin(), mine.end());
      if (!cur.hyps.empty() && both.size() + 1 > kGroupMuCap) {
        close_group(cur);
        cur = obhip_terms::GeGroup();
        cur.off.push_back(0);
        used = mine;
      } else {
        used.swap(both);
      }
      cur.hyps.push_back(hh);
      cur.off.push_back(cur.off.back() + sv->p);
    }
    close_group(cur);
  };
  group_views(t.ge.sviews, t.ge.sgroups);
  group_views(t.ge.dviews, t.ge.dgroups);  // the same for the delta views (grad_mm_dot_dev)
}

// (a view does not fit the kernel: more than 8 column slots, or a tile beyond the prefetch registers)
bool build_d3_groups(obhip_terms &t, const obhip_basis &b) {
  // OBHIP_GRAD_D3=0 (read per call: the tests switch it): the per-hyper-parameter passes
  const char *sw = getenv("OBHIP_GRAD_D3");
  if (sw && atoi(sw) == 0) return false;
  // the tables hold column numbers of the gradient basis: keyed by everything those depend on
  // (level caps, first column of every dimension, first delta column of every hyper-parameter)
  const obhip_model &m = *b.model;
  const obhip_gradbasis &g = *b.grad;
  const std::vector<DimDesc> &dims = b.md.dims_h;
  const uint64_t d = t.d;
  std::vector<int64_t> key = b.md.cap;
  for (uint64_t l = 0; l < d; ++l) key.push_back(dims[l].ccol0);
  for (const GradHyp &gh : g.hyps_h) {
    key.push_back(gh.dim);
    key.push_back(gh.dcol);
  }
  if (t.ge.d3_key == key) return t.ge.d3_ok;
  HostTimer ht("build_d3_groups (rebuild)");
  build_sparse_views(t, b);
  t.ge.d3.clear();
  t.ge.d3_key = key;
  t.ge.d3_ok = false;
  // two blocks per CU: 2 x Mu x 65 x 8 B <= 160 KB
  constexpr size_t kMuCap = 152;
  static_assert(kMuCap <= (size_t)kTlWaves * kD3Pre, "the tile is prefetched into registers");  // kD3Pre: obhip_internal.h
  struct Member {
    uint64_t l, h0;
    int nh;
    std::set<uint32_t> cols;
    uint64_t maxw = 0;
  };
  std::vector<Member> mem;
  for (uint64_t l = 0; l < d; ++l)
    for (uint64_t h0 = m.hypst[l]; h0 < m.hypst[l + 1]; h0 += 2) {
      Member M;
      M.l = l;
      M.h0 = h0;
      M.nh = (int)std::min<uint64_t>(2, m.hypst[l + 1] - h0);
      const std::vector<uint32_t> &ix = t.ge.sidx[h0];
      if (ix.empty()) continue;
      for (uint32_t k : ix) {
        uint64_t w = 1 + (uint64_t)M.nh;
        for (uint64_t q = 0; q < d; ++q) {
          const uint32_t lv = t.lev[(uint64_t)k * d + q];
          if (lv == 0) continue;
          // (bits 28-29: how the column is staged -- 0 as it is, 1 times the row's basescale (delta
          // columns), 2 times basescale x second weight (the dimension's OWN factor): k_tmm_d3)
          if (q == l) {
            M.cols.insert((uint32_t)(dims[q].ccol0 + lv - 1) | kD3Own);
            for (int j = 0; j < M.nh; ++j) M.cols.insert((uint32_t)(g.hyps_h[h0 + j].dcol + lv - 1) | kD3Delta);
          } else {
            M.cols.insert((uint32_t)(dims[q].ccol0 + lv - 1));
            ++w;
          }
        }
        M.maxw = std::max(M.maxw, w);
      }
      if (M.cols.size() + 1 > kMuCap || M.maxw > 8) return false;
      mem.push_back(std::move(M));
    }
  // consecutive members with the same number of delta columns share a launch while their columns fit
  size_t i = 0;
  while (i < mem.size()) {
    std::set<uint32_t> used = mem[i].cols;
    uint64_t maxw = mem[i].maxw;
    size_t j = i + 1;
    while (j < mem.size() && mem[j].nh == mem[i].nh) {
      std::set<uint32_t> both = used;
      both.insert(mem[j].cols.begin(), mem[j].cols.end());
      if (both.size() + 1 > kMuCap) break;
      used.swap(both);
      maxw = std::max(maxw, mem[j].maxw);
      ++j;
    }
    obhip_terms::GeD3 G;
    G.nh = mem[i].nh;
    G.off.push_back(0);
    for (size_t q = i; q < j; ++q) {
      G.hyp0.push_back(mem[q].h0);
      G.off.push_back(G.off.back() + t.ge.sidx[mem[q].h0].size());
    }
    auto v = std::make_unique<obhip_terms>();
    v->no_share = true;
    v->p = G.off.back();
    v->d = 0;
    v->p_pad = (v->p + 255) / 256 * 256;
    v->W = std::max<uint64_t>(4, (maxw + 1) / 2 * 2);
    std::vector<uint32_t> ul(1, 0u);  // the ones column first
    ul.insert(ul.end(), used.begin(), used.end());
    v->Mu = ul.size();
    std::map<uint32_t, uint16_t> pos;
    for (size_t u = 0; u < ul.size(); ++u) pos[ul[u]] = (uint16_t)u;
    const uint64_t W = v->W;
    std::vector<uint16_t> hc(v->p_pad * W, 0);
    std::vector<uint32_t> nz(v->p, 0), order(v->p_pad);
    for (size_t q = i; q < j; ++q) {
      const Member &M = mem[q];
      const std::vector<uint32_t> &ix = t.ge.sidx[M.h0];
      for (size_t e = 0; e < ix.size(); ++e) {
        const uint64_t k = ix[e], vt = G.off[q - i] + e;
        uint64_t others = 0;
        for (uint64_t a = 0; a < d; ++a) others += a != M.l && t.lev[k * d + a] > 0;
        uint64_t w = W - (others + 1 + (uint64_t)M.nh);
        nz[vt] = (uint32_t)(others + 1 + (uint64_t)M.nh);
        for (uint64_t a = 0; a < d; ++a) {  // the other factors keep their dimension order
          const uint32_t lv = t.lev[k * d + a];
          if (a != M.l && lv > 0) hc[vt * W + w++] = pos[(uint32_t)(dims[a].ccol0 + lv - 1)];
        }
        const uint32_t lv = t.lev[k * d + M.l];
        hc[vt * W + w++] = pos[(uint32_t)(dims[M.l].ccol0 + lv - 1) | kD3Own];
        for (int a = 0; a < M.nh; ++a)
          hc[vt * W + w++] = pos[(uint32_t)(g.hyps_h[M.h0 + a].dcol + lv - 1) | kD3Delta];
      }
    }
    for (uint64_t k = 0; k < v->p_pad; ++k) order[k] = (uint32_t)k;
    std::stable_sort(order.begin(), order.begin() + v->p, [&](uint32_t a, uint32_t c) { return nz[a] > nz[c]; });
    if (v->cols.upload(hc.data(), hc.size()) || v->sperm.upload(order.data(), order.size()) ||
        v->ucol.upload(ul.data(), ul.size()))
      return false;
    G.v = std::move(v);
    t.ge.d3.push_back(std::move(G));
    i = j;
  }
  t.ge.d3_ok = true;
  return true;
}

obhip_terms *grad_view_restricted(obhip_terms &t, const obhip_basis &b, uint64_t h, bool delta,
                                  const std::vector<uint32_t> **idx) {
  build_sparse_views(t, b);
  *idx = &t.ge.sidx[h];
  return (delta ? t.ge.dviews : t.ge.sviews)[h].get();
}

std::vector<obhip_terms::GeGroup> &grad_view_groups(obhip_terms &t, const obhip_basis &b, bool delta) {
  build_sparse_views(t, b);
  return delta ? t.ge.dgroups : t.ge.sgroups;
}

obhip_terms *grad_view(obhip_terms &t, const obhip_basis &b, uint64_t h) {
  const obhip_model &m = *b.model;
  const uint64_t nh = m.nhyp(), d = t.d;
  if (t.ge.full.size() != nh || t.ge.full_sig != m.hypmatch) {
    t.ge.full.clear();
    t.ge.full.resize(nh);
    t.ge.full_sig = m.hypmatch;
  }
  if (!t.ge.full[h]) {
    std::vector<uint32_t> all(t.p);
    std::iota(all.begin(), all.end(), 0u);
    t.ge.full[h] = make_view(t, all, d + 2 * nh, m.hypmatch[h], d + h, 1);
  }
  return t.ge.full[h].get();
}

}  // namespace obhip
