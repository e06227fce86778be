// Observed input gradients as rows of the normal equations: host side.  No reference counterpart.
//   ensure_dx_stage        the tables of the staging kernel (those of the input-gradient predictor plus
//                          the dimension of every used column)
//   grad_batch_normal_eq   sum_j w_j D_j^T D_j and sum_j w_j D_j^T g_j of one batch, over row chunks:
//                          stage sqrt(w_j) D_j (kernels_materialize_dx.hip), Gram of the staged rows
//   obhip_design_dx_dev    the staged blocks themselves
// Every check that can refuse a call runs before the first device call.
#include <algorithm>
#include <cmath>
#include <string>

#include "obhip_internal.h"

using namespace obhip;

namespace obhip {

int check_grad_dims(const char *who, uint64_t d, const uint32_t *dims, uint64_t ndims, const double *weights) {
  const std::string w(who);
  if (ndims == 0 || ndims > d)
    return fail(OBHIP_ERR_INVALID, w + ": ndims must be between 1 and the model's " + std::to_string(d) + " dimensions");
  for (uint64_t j = 0; j < ndims; ++j)
    for (uint64_t i = 0; i < j; ++i)
      if (dims[i] == dims[j]) return fail(OBHIP_ERR_INVALID, w + ": dimension " + std::to_string(dims[j]) + " is listed twice");
  for (uint64_t j = 0; j < ndims; ++j)
    if (dims[j] >= d)
      return fail(OBHIP_ERR_INVALID, w + ": dimension " + std::to_string(dims[j]) + " of a model with " + std::to_string(d));
  if (weights)
    for (uint64_t j = 0; j < ndims; ++j)
      if (!(weights[j] > 0.0) || !std::isfinite(weights[j]))
        return fail(OBHIP_ERR_INVALID, w + ": weights must be finite and positive");
  return 0;
}

int ensure_dx_stage(const obhip_model &m, obhip_terms &t) {
  OB_TRY(prepare_predict(m, t, true));
  obhip_terms::Dx &dx = t.dx;
  if (dx.udim.p && dx.udim_cap == t.cached_cap) return 0;
  std::vector<int32_t> h(t.Mu, -1);
  for (uint64_t l = 0; l < t.d; ++l)
    for (int64_t lv = 1; lv <= t.pred_md.cap[l]; ++lv) {
      const int32_t u = t.cpos_h[(size_t)t.pred_md.dims_h[l].ccol0 + lv - 1];
      if (u >= 1) h[u] = (int32_t)l;
    }
  OB_TRY(dx.udim.upload(h.data(), h.size()));
  dx.udim_cap = t.cached_cap;
  return 0;
}

namespace {

// dims and sqrt(weights) on the device
int upload_dims(const uint32_t *dims, const double *weights, uint64_t L, DevBuf<uint32_t> &d_dims, DevBuf<double> &d_sqw) {
  std::vector<double> sq(L, 1.0);
  if (weights)
    for (uint64_t j = 0; j < L; ++j) sq[j] = std::sqrt(weights[j]);
  OB_TRY(d_dims.upload(dims, L));
  return d_sqw.upload(sq.data(), L);
}

}  // namespace

int grad_batch_normal_eq(obhip_basis &holder, const obhip_model &m, obhip_terms &t, const double *d_x, uint64_t n,
                         const uint32_t *dims, const double *weights, uint64_t L, const double *d_dY, uint64_t lddy,
                         uint64_t q, double *d_tri, double *d_R) {
  OB_TRY(ensure_dx_stage(m, t));
  DevBuf<uint32_t> d_dims;
  DevBuf<double> d_sqw;
  OB_TRY(upload_dims(dims, weights, L, d_dims, d_sqw));
  // The staged blocks take n_pad L p_pad doubles (65 GB for 1e5 rows, d = 20, p = 4096): row chunks, each
  // within a quarter of the free HBM and 16 GB as launch_gram_panel's chunk path has them.
  const uint64_t ntiles = (n + kTileRows - 1) / kTileRows;
  size_t free_b = 0, total_b = 0;
  OB_HIP(hipMemGetInfo(&free_b, &total_b));
  const char *forced = getenv("OBHIP_GRAM_CHUNK_ROWS");  // tests
  const uint64_t ctiles = gram_chunk_tiles(free_b, (uint64_t)t.p_pad * kTileRows * L * sizeof(double), ntiles,
                                           forced ? std::max<uint64_t>(1, (uint64_t)atoll(forced)) : 0);
  if (!ctiles)
    return fail(OBHIP_ERR_HIP, "not enough free HBM for even one row chunk of the derivative design matrix");
  const uint64_t blk_rows = ctiles * kTileRows;
  DevBuf<double> staged, ypart, part;
  OB_TRY(staged.alloc((size_t)blk_rows * L * t.p_pad));
  OB_TRY(ypart.alloc((size_t)ctiles * t.p_pad));
  if (q > 1) OB_TRY(part.alloc(dx_aty_splits(blk_rows * L) * t.p_pad));
  GramSink sink;
  sink.out = d_tri;
  sink.packed = true;
  for (uint64_t t0 = 0; t0 < ntiles; t0 += ctiles) {
    const uint64_t nt = std::min(ctiles, ntiles - t0), r0 = t0 * kTileRows;
    const uint64_t nrows = std::min<uint64_t>(nt * kTileRows, n - r0);
    const uint64_t rows_blk = nt * kTileRows;  // the last chunk is shorter: its blocks lie closer
    DxStage s;
    s.x = d_x + r0, s.ldx = n, s.n = nrows;
    s.dims = d_dims.p, s.sqw = d_sqw.p, s.L = L;
    s.out = staged.p, s.pitch = t.p_pad, s.blk_rows = rows_blk, s.pcols = t.p_pad;
    s.pad_rows = true;
    s.g = d_dY + r0, s.ldg = lddy, s.ypart = ypart.p;
    OB_TRY(launch_materialize_dx(m, t, s));
    OB_TRY(launch_dx_colsum(ypart.p, nt, t.p_pad, t.p, t0 != 0, d_R));
    for (uint64_t r = 1; r < q; ++r)
      OB_TRY(launch_dx_aty(staged.p, t.p_pad, rows_blk, L, nrows, d_sqw.p, d_dY + r * L * lddy + r0, lddy, part.p, t.p,
                           t0 != 0, d_R + r * t.p));
    // The Gram de-duplication stays valid on these rows: a row of D_l is still `scale x one function of
    // the level per dimension`, level 0 included (its function in dimension l is rho_l instead of 1), so
    // an entry of D_l^T D_l depends on the per-dimension unordered level pairs only -- gram_dedup.hip's
    // premise; and so does a sum of such matrices over l.
    OB_TRY(gram_of_staged(holder, staged.p, nt * L, t, sink, t0 != 0, t0 + nt >= ntiles));
  }
  return 0;
}

}  // namespace obhip

extern "C" {

int obhip_design_dx_dev(const obhip_model *m, const obhip_terms *t, const double *d_x, uint64_t n, const uint32_t *dims,
                        uint64_t ndims, const double *weights, double *d_out, uint64_t ldo) {
  if (!m || !t || !dims || !d_out || (!d_x && n > 0))
    return fail(OBHIP_ERR_INVALID, "design_dx_dev: null model, terms, x, dims or out");
  OB_TRY(check_compat(m, t));
  OB_TRY(check_grad_dims("design_dx_dev", m->d, dims, ndims, weights));
  if (ldo < t->p) return fail(OBHIP_ERR_INVALID, "design_dx_dev: ldo below the number of terms");
  if (n > kMaxRowsPerCall) return fail(OBHIP_ERR_INVALID, "design_dx_dev: more than 2^40 rows in one call");
  if (n == 0) return 0;
  OB_TRY(require_device());
  obhip_terms &tt = *const_cast<obhip_terms *>(t);
  OB_TRY(ensure_dx_stage(*m, tt));
  DevBuf<uint32_t> d_dims;
  DevBuf<double> d_sqw;
  std::vector<double> sq(ndims, 1.0);
  if (weights)
    for (uint64_t j = 0; j < ndims; ++j) sq[j] = std::sqrt(weights[j]);
  OB_TRY(d_dims.upload(dims, ndims));
  OB_TRY(d_sqw.upload(sq.data(), ndims));
  DxStage s;
  s.x = d_x, s.ldx = n, s.n = n;
  s.dims = d_dims.p, s.sqw = d_sqw.p, s.L = ndims;
  s.out = d_out, s.pitch = ldo, s.blk_rows = n, s.pcols = t->p;
  return launch_materialize_dx(*m, tt, s);
}

}  // extern "C"
