// Internal declarations shared by the host logic and the HIP kernels of
// libobhip.  Nothing here is part of the ABI (include/obhip.h is).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/obhip.h"
#include "launch_plan.h"
#include "gram_plan.h"
#include "gram_order.h"

namespace obhip {

// ---- error plumbing ---------------------------------------------------------
int fail(int code, const std::string &msg);
int hip_fail(hipError_t e, const char *what, const char *file, int line);
#define OB_HIP(expr)                                                \
  do {                                                              \
    hipError_t _e = (expr);                                         \
    if (_e != hipSuccess) return obhip::hip_fail(_e, #expr, __FILE__, __LINE__); \
  } while (0)
#define OB_TRY(...)              \
  do {                           \
    int _rc = (__VA_ARGS__);     \
    if (_rc != 0) return _rc;    \
  } while (0)

int require_device();
hipStream_t cur_stream();
// model state stamps are drawn from one process-wide counter: device tables cached under
// (model address, stamp) can then never be taken for those of another model that came to live at
// the same address
uint64_t next_model_version();
int ensure_dyn_lds(const void *kernel, size_t bytes);  // dynamic LDS above 64 KB, granted once per kernel
int device_cus(int device);                            // compute units (cached per device)

// ---- profiling --------------------------------------------------------------
// every blocking wait of the library for the device goes through these (the macros below): counted,
// so that a caller can ask how many host round trips a call sequence made
// (obhip_profile_get("host_syncs"); bench.py reports it for the small-n obfit of configs[0])
extern std::atomic<uint64_t> g_host_syncs;
inline hipError_t counted_stream_sync(hipStream_t s) {
  g_host_syncs.fetch_add(1, std::memory_order_relaxed);
  return hipStreamSynchronize(s);
}
inline hipError_t counted_device_sync() {
  g_host_syncs.fetch_add(1, std::memory_order_relaxed);
  return hipDeviceSynchronize();
}
#define hipStreamSynchronize(s) obhip::counted_stream_sync(s)
#define hipDeviceSynchronize() obhip::counted_device_sync()

struct ProfScope {
  const char *name;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool active = false;
  explicit ProfScope(const char *n);
  ~ProfScope();
};

// host wall time of a scope, summed per name and printed at exit when OBHIP_HOST_TIMING is set
// (tuning aid: where an entry point spends its time between the kernels)
struct HostTimer {
  const char *name;
  double t0 = 0;
  static bool on() {
    static const bool v = getenv("OBHIP_HOST_TIMING") != nullptr;
    return v;
  }
  static double now() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
  }
  struct Table {
    std::map<std::string, std::pair<uint64_t, double>> t;
    ~Table() {
      for (auto &e : t)
        fprintf(stderr, "[host] %-36s %8llu x %10.3f ms = %10.1f ms\n", e.first.c_str(),
                (unsigned long long)e.second.first, e.second.second / e.second.first, e.second.second);
    }
  };
  static Table &table() {
    static Table tb;
    return tb;
  }
  explicit HostTimer(const char *n) : name(n) {
    if (on()) t0 = now();
  }
  ~HostTimer() {
    if (!on()) return;
    auto &e = table().t[name];
    e.first += 1;
    e.second += now() - t0;
  }
};

// ---- device memory pool -----------------------------------------------------------
// Every C-ABI call allocates its device temporaries (vectors of n or p doubles, an n x nhyp
// block, ...) and frees them on return; hipMalloc / hipFree cost far more than the kernels of
// a small call and hipFree synchronises the device.  Freed blocks are therefore kept, keyed
// by exact size, device and the stream they were last used on -- a block is handed out again
// only to work queued on that same stream, so stream order protects it -- up to
// OBHIP_POOL_MB (default: an eighth of the device's memory, at least 8192) of cached memory; larger blocks and the overflow go back to
// the driver, and a failed hipMalloc empties the pool and retries.
int pool_alloc(void **p, size_t bytes);
// stream: the one the block was allocated for (the tag under which it may be handed out again)
void pool_free(void *p, size_t bytes, hipStream_t stream);
void pool_trim();

// ---- device buffer ----------------------------------------------------------
template <typename T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  hipStream_t s = nullptr;  // stream current at allocation
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) {
      // used on another stream since (obhip_set_stream between allocation and release): let
      // that work finish, the block goes back under the stream it was allocated for
      if (cur_stream() != s) (void)hipStreamSynchronize(cur_stream());
      pool_free(p, n * sizeof(T), s);
    }
    p = nullptr;
    n = 0;
  }
  int alloc(size_t count) {
    if (count == n && p) return 0;
    release();
    if (count == 0) return 0;
    int rc = pool_alloc((void **)&p, count * sizeof(T));
    if (rc) return rc;
    n = count;
    s = cur_stream();
    return 0;
  }
  int upload(const T *src, size_t count) {
    int rc = alloc(count);
    if (rc) return rc;
    if (count == 0) return 0;
    hipError_t e = hipMemcpyAsync(p, src, count * sizeof(T),
                                  hipMemcpyHostToDevice, cur_stream());
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync", __FILE__, __LINE__);
    e = hipStreamSynchronize(cur_stream());
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__);
    return 0;
  }
};

// dst (host) <- src (device), waited for
int d2h(void *dst, const void *src, size_t bytes);
// d <- the rows x cols column-major host matrix src with leading dimension ld, compacted to ld = rows
int upload_cols(DevBuf<double> &d, const double *src, uint64_t rows, uint64_t cols, uint64_t ld);

// ---- covariance functions (host) --------------------------------------------
constexpr int kNumCov = 3;
struct CovInfo {
  int numhyp;
  double hyp0[2], hyplb[2], hypub[2], hypvar[2];
  double lowbnd, uppbnd;
};
const CovInfo &cov_info(int kind);
void cov_host(int kind, const double *hyp, const double *x1, uint64_t n1,
              const double *x2, uint64_t n2, double *out /* n1 x n2 col-major */);
void cov_gradhyp_host(int kind, const double *hyp, const double *x1, uint64_t n1, const double *x2,
                      uint64_t n2, double *out /* n1 x n2 x numhyp, col-major slices */);
double cov_hyplpdf_host(int kind, const double *hyp);

// symmetric eigen-decomposition (cyclic Jacobi), eigenvalues ascending like
// LAPACK dsyev / arma::eig_sym; a is n x n col-major (destroyed), v n x n.
void jacobi_eigh(int n, std::vector<double> &a, std::vector<double> &w,
                 std::vector<double> &v);

}  // namespace obhip

// ---- outermod -----------------------------------------------------------------
struct obhip_model {
  uint64_t d = 0;
  std::vector<int> kinds;
  std::vector<uint64_t> hypst;     // d+1
  std::vector<double> hyp;
  bool knots_set = false;
  std::vector<uint64_t> knotptst;  // d+1
  std::vector<double> knotpt;      // M
  uint64_t mmax = 0;
  std::vector<double> rotmat;      // mmax x M col-major
  std::vector<double> basisvar;    // M
  std::vector<int64_t> maxlevel;   // d
  uint64_t version = 0;            // bumped whenever build() runs
  // hyper-parameter gradients (modandbase.cpp:183-197,257-274): one block of m_l columns
  // per hyper-parameter; gest[h] = first column of hyper-parameter h, hypmatch[h] = its dim
  std::vector<uint64_t> hypmatch, gest;     // nhyp, nhyp + 1
  std::vector<double> rotmat_gradhyp;       // mmax x gest[nhyp] col-major
  std::vector<double> logbasisvar_gradhyp;  // gest[nhyp]
  uint64_t nhyp() const { return hypmatch.size(); }

  uint64_t M() const { return knotpt.size(); }
  uint64_t m_of(uint64_t l) const { return knotptst[l + 1] - knotptst[l]; }
  int build();
};

// ---- device view of a model restricted to per-dimension level caps ------------
namespace obhip {

struct DimDesc {
  int kind;
  int m;       // knots in this dim
  int koff;    // offset into the knot arrays
  int ncol;    // levels evaluated = cap+1 (level 0 included)
  int ncolp;   // ncol rounded up to a multiple of 8
  int rotoff;  // offset into rot (doubles)
  int ccol0;   // compact column of level 1 (level t -> ccol0 + t - 1)
  int tab;     // offset (doubles) of the dimension's interval tables in ModelDev::tab, -1: none
  int gwin;    // interval search of the tables: 0 = seven bisection steps; E > 0: the guess
               // J0 = floor((u - g0) ginv) + 1 is within E - 1 of the interval for every u (checked on
               // the host), so 2 E independent reads around it settle it in one round trip
  double p0, p1, p2;  // kernel constants (see kernels_basis.hip)
  double g0, ginv;    // the guess of gwin: first sorted knot (in u), (m - 1) / (last - first)
};

struct ModelDev {
  uint64_t model_version = ~0ull;
  const void *built_for = nullptr;  // the model the tables were built from
  std::vector<int64_t> cap;     // d
  std::vector<DimDesc> dims_h;
  uint64_t Mc = 0;              // compact columns incl. the ones column 0
  DevBuf<DimDesc> dims;
  DevBuf<double> ka, kb, kc;    // per-knot constants (M each)
  DevBuf<double> rot;           // per dim [m][ncolp]
  DevBuf<double> tab;           // per mat25 / mat25pow dim [m sorted u (even length)][m + 1][ncol][6]
  int build(const obhip_model &m, const std::vector<int64_t> &cap);
};

}  // namespace obhip

// ---- terms --------------------------------------------------------------------
// star tables of a term set (csrc/share.cpp): p_pad / 4 stars of four terms that share all
// factors but one (or, plain stars, nothing), in star-waves of 64
namespace obhip {
struct ShareTables {
  bool ok = false;
  uint64_t nstars = 0;       // 64 x (nsw_family + nsw_plain), the empty stars that fill the waves included
  uint64_t nsw_family = 0;   // star-waves of family stars (shape (P, 1)) -- they come first
  uint64_t nsw_plain = 0;    // star-waves of plain stars (shape (0, S)): the left-over terms four at a time
  uint64_t nleft = 0;        // left-over terms (no family with four free members)
  uint64_t reads = 0;        // column reads per row of the family star-waves: sum of P + 4
  uint64_t reads_left = 0;   // of the plain star-waves: sum of 4 S
  uint64_t reads_plain = 0;  // of the nnz-sorted scheme without sharing, 4 terms per lane (rounds 1-4)
  uint64_t lds_cycles = 0;   // LDS cycles of all star-waves' reads with their bank conflicts (2 per read at best)
  uint64_t lds_cycles0 = 0;  // the same before the half-wave / term-order search
  std::vector<uint16_t> cols;   // nstars x 4 W used-column indices, laid out for the star-wave's shape
  std::vector<uint32_t> term;   // nstars x 4 term indices (0xffffffff: none -- an empty star's)
  std::vector<uint32_t> shape;  // per star-wave: P | S << 8
  std::vector<uint32_t> left_term;  // nleft term indices
  std::vector<uint16_t> left_cols;  // nleft x W used-column indices, right-aligned (0 = ones)
  std::vector<uint16_t> relabel;    // used-column index the caller passed -> index the tables are written in
};
int build_share_tables(const uint16_t *hc, uint64_t p_pad, uint64_t W, ShareTables &out, bool renumber = false,
                       uint64_t ncol = 0);
bool share_wanted();  // OBHIP_SHARE=0: the kernels take the plain tables (A/B measurements)

// tile pairs of the panel Gram that hold repeats of other entries of G only (csrc/gram_dedup.hip):
// analysed once per term set, on the device
struct GramDedup {
  bool tried = false;
  int hashbits = 0;            // bits of the hash the analysis ran with (OBHIP_GRAM_DEDUP_HASHBITS)
  int nb = 0, npairs = 0, nskip = 0;
  double analysis_ms = 0.0;    // host wall time of the analysis, uploads and read-back included
  uint64_t sig = 0;            // serial number of the analysis (non-zero): key of the task tables built on the mask
  struct Dealing {             // dealing chosen for the mask (continuous or whole runs) ...
    GramKey key;               // ... at this shape and split (no shape: none chosen yet)
    bool continuous = false;
  } dealing;
  std::vector<uint8_t> skip;   // per tile pair (row-major slot in the upper triangle): 1 = no task
  DevBuf<uint8_t> skip_dev;    // the same on the device
  DevBuf<uint32_t> pairs;      // nskip skipped tile pairs, I | J << 16
  DevBuf<uint32_t> src;        // nskip x 128 x 128: the entry's source s' << 16 | t' (s' <= t', in a kept pair)
  // The same analysis at the granularity of a wave's 64 x 64 tile (gram_plan.h: the plan at wave-tile
  // granularity), run when a launch is long enough to pay for it or OBHIP_GRAM_DEDUP_QUADS=1 asks
  struct Quads {
    bool tried = false;
    int hashbits = 0;
    int ndrop = 0;               // dropped wave tiles
    int blocks = 0;              // blocks per row split of the packed plan ...
    int blocks_pairs = 0;        // ... and of the whole-pair plan (build_task_order under `skip`)
    double setup_ms = 0.0;       // host wall time of the analysis and the packing
    uint64_t sig = 0;
    GramKey key;                 // the launch the decision below was taken for: shape, split, the whole-pair mask and
                                 // dealing it competes with, the switch (no shape: none taken)
    bool engaged = false;        // that launch runs the packed plan ...
    bool continuous = false;     // ... dealt continuously or in whole runs
    std::vector<uint8_t> keep;   // per wave tile (slot pair_slot(2 nb, a, b)): 0 = dropped
    DevBuf<uint8_t> qskip_dev;   // per tile pair: bit 2 r + c set = its quadrant (r, c) is not computed
    DevBuf<uint32_t> tiles;      // ndrop dropped wave tiles, a | b << 16 (64-column groups)
    DevBuf<uint32_t> src;        // ndrop x 64 x 64 sources, in kept wave tiles
  } quads;
};
// The order in which the panel Gram stages and multiplies the columns of these terms (gram_order.h): a stable
// sort by the number of factors, under which more wave tiles repeat.  It belongs to the term set, is built on
// first use and changes nothing a caller sees: every result comes out in term coordinates.
struct GramOrder {
  bool tried = false;             // perm, inv and perm_dev are built
  bool identity = true;           // the sort changes nothing
  uint64_t serial = 0;            // non-zero once built: what obhip_basis::bmat_order records of a staged matrix
  int last_launch = -1;           // the term set's latest launch_gram_to ran in Gram order (1) or not (0); -1: none yet
  std::vector<uint32_t> perm;     // perm[k] = the term staged as column k
  std::vector<uint32_t> inv;      // inv[perm[k]] = k
  DevBuf<uint32_t> perm_dev;      // p_pad entries, the padding columns stay where they are (last)
  DevBuf<uint16_t> cols;          // obhip_terms::cols with its rows in Gram order (gathered before every staging)
  // the analysis at wave-tile granularity in Gram coordinates, dropped by the sequential pass; its key, engaged,
  // continuous, blocks and setup_ms are those of the order (blocks_pairs: of the plan it competes with)
  GramDedup::Quads quads;
};
}  // namespace obhip

struct obhip_terms {
  uint64_t uid = 0;                   // unique per object (caches keyed by terms use it)
  uint64_t p = 0, d = 0;
  std::vector<uint32_t> lev;          // p x d row-major levels
  std::vector<int64_t> maxlev;        // d
  uint64_t nnz_total = 0, max_nnz = 0;
  // device tables, rebuilt when the compact layout (caps) changes
  std::vector<int64_t> cached_cap;
  uint64_t W = 0;                     // padded column-list width
  uint64_t Mu = 0;                    // used compact columns
  obhip::DevBuf<uint16_t> cols;       // p_pad x W indices into the USED list
  obhip::DevBuf<uint32_t> ucol;       // Mu compact column ids (used list)
  obhip::DevBuf<uint32_t> sperm;      // p_pad: terms ordered by falling number of factors (stable)
  obhip::DevBuf<int32_t> cpos;        // compact column -> used index or -1 (Mc)
  std::vector<int32_t> cpos_h;        // host copy (the dimension views of the input-gradient predictor)
  uint64_t p_pad = 0;
  // star tables (shared sub-products, csrc/share.cpp); sh.ok false: the kernels take sperm / cols
  obhip::ShareTables sh;              // (host copies dropped after the upload; counts kept)
  bool no_share = false;              // views of another term set (gradient passes): no star tables
  obhip::DevBuf<uint16_t> sh_cols;    // nstars x 4 W
  obhip::DevBuf<uint32_t> sh_term;    // nstars x 4
  obhip::DevBuf<uint32_t> sh_shape;   // nstars / 64
  obhip::DevBuf<uint32_t> sh_left_term;  // nleft (at least one element)
  obhip::DevBuf<uint16_t> sh_left_cols;  // nleft x W
  // a few restricted views concatenated (one B^T pass for all of them), offsets per hyper-parameter
  struct GeGroup {
    std::unique_ptr<obhip_terms> v;  // the views of `hyps`, concatenated
    std::vector<uint64_t> hyps, off; // off[j]: first term of hyps[j] in v (off.size() = hyps.size() + 1)
  };
  // the fused gradient passes (k_tmm_d3, kernels_grad_d3.hip): per launch the terms that have one of a
  // few dimensions, each with that dimension's own factor moved to the END of its column list and
  // followed by the delta columns (level of the term) of up to two of the dimension's
  // hyper-parameters -- tables written by hand into v (no levels), keyed by the level caps
  struct GeD3 {
    std::unique_ptr<obhip_terms> v;
    int nh = 0;                       // delta columns per view-term (1 or 2)
    std::vector<uint64_t> hyp0, off;  // member j: hyper-parameters hyp0[j] .. hyp0[j] + nh - 1,
                                      // view-terms [off[j], off[j + 1]) = the terms sidx[hyp0[j]]
  };
  // per hyper-parameter views of these terms for the gradient products (grad_views.cpp), with their keys
  struct GradCache {
    // full views: dimension hypmatch[h] dropped, the gradient block at level t + 1 (grad_view)
    std::vector<std::unique_ptr<obhip_terms>> full;
    std::vector<uint64_t> full_sig;  // hypmatch of the model they were built for
    // restricted to the terms that HAVE the hyper-parameter's dimension (sidx[h]), its factor replaced
    // by the gradient column (sviews: transposed products, the other terms come from one dense pass)
    // or by the delta column (dviews: products B a); groups of each kind concatenated
    std::vector<std::unique_ptr<obhip_terms>> sviews, dviews;
    std::vector<std::vector<uint32_t>> sidx;
    std::vector<GeGroup> sgroups, dgroups;
    std::vector<uint64_t> sig;       // hypmatch of the model they were built for
    // the k_tmm_d3 groups, written from sidx
    std::vector<GeD3> d3;
    std::vector<int64_t> d3_key;     // column layout they were built for (build_d3_groups)
    bool d3_ok = false;              // false: some view does not fit the kernel
    // empty restricted views for nh hyper-parameters laid out as `s`; the d3 tables go with them
    void reset_views(const std::vector<uint64_t> &s, uint64_t nh) {
      sig = s;
      sviews.clear(), sviews.resize(nh), dviews.clear(), dviews.resize(nh);
      sidx.assign(nh, {}), sgroups.clear(), dgroups.clear();
      d3.clear(), d3_key.clear(), d3_ok = false;
    }
  } ge;
  // device view of the model capped at maxlev, for the fused predictor
  obhip::ModelDev pred_md;
  const obhip_model *pred_model = nullptr;
  // input-gradient predictor (kernels_predict_dx.hip, predict_dx.cpp): per dimension l the view of
  // the terms that have l -- entry = W / 2 words of the term's OTHER used columns (own slot = the
  // ones column), its own used column, its term index -- and the derivative interval tables
  struct Dx {
    std::vector<uint64_t> voff;      // d + 1: first view entry of every dimension (host; from lev alone)
    std::vector<uint32_t> vterm;     // term index of every view entry (host)
    std::vector<int64_t> cap;        // level caps (= column layout) the device tables were packed for
    obhip::DevBuf<uint32_t> vw;      // entries x (W / 2 + 2) words
    obhip::DevBuf<uint32_t> voff_dev;
    obhip::DevBuf<double> dtab;      // layout of ModelDev::tab, the sums of dk/du in place of those of k
    const obhip_model *tab_model = nullptr;
    uint64_t tab_version = ~0ull;
    std::vector<int64_t> tab_cap;
    // second-derivative interval tables (predict_hvp.cpp): the layout of dtab, the sums of d2k/du2
    obhip::DevBuf<double> d2tab;
    const obhip_model *tab2_model = nullptr;
    uint64_t tab2_version = ~0ull;
    std::vector<int64_t> tab2_cap;
    // staging of the derivative design matrix (kernels_materialize_dx.hip): used column -> dimension
    obhip::DevBuf<int32_t> udim;     // Mu (-1: the ones column)
    std::vector<int64_t> udim_cap;   // column layout it was made for
  } dx;
  // prior precisions 1 / (sd e^rho)^2 of these terms on the device, for the model state and rho
  // they were last asked for (the device-side Newton fit: no upload, no host sync per fit)
  obhip::DevBuf<double> prec_dev;
  const obhip_model *prec_model = nullptr;
  uint64_t prec_version = 0;
  double prec_rho = 0.0;
  obhip::GramDedup dedup;             // redundant tile pairs of the panel Gram (levels only: no cap in its key)
  obhip::GramOrder order;             // the column order of the panel Gram and its plan (levels only)
  // Sobol passes (sobol.cpp; levels only): the levels as bytes, [p][d], and per dimension l
  // L_l = maxlev[l] + 1, its offset in a packed mean table and in a packed cov table ([3][d] ints)
  obhip::DevBuf<uint8_t> sobol_lev;
  obhip::DevBuf<int> sobol_meta;
  // and per pair of dimensions i < j, in the order (0,1), (0,2), .. (0,d-1), (1,2), ..: i, j and the
  // offset of G_ij in a packed G ([d (d - 1) / 2][3] ints)
  obhip::DevBuf<int> sobol_pairs;
  // product of two input blocks (product.cpp, kernels_product.hip): the tables of the last split
  // (dims_b) asked for, against the column layout `cap`.  Each side has its own used columns (0 = the
  // ones column, then the used levels of its dimensions in ascending (dimension, level) order).
  struct Product {
    std::vector<uint32_t> dims_b;      // key: the split ...
    std::vector<int64_t> cap;          // ... and the level caps of pred_md the compact columns refer to
    uint64_t mu_a = 0, mu_b = 0;       // used columns of the sides
    uint64_t wa = 0, wb = 0;           // padded widths of the sides' column lists (even, >= 2)
    obhip::DevBuf<int> side_a, side_b;       // the sides' dimensions (A ascending, B in the order of dims_b)
    obhip::DevBuf<int> dim_src;              // d: column s of xa as s, column s of xb as -(s + 1)
    obhip::DevBuf<int32_t> cpos_a, cpos_b;   // compact column -> the side's used column or -1 (Mc each)
    obhip::DevBuf<uint16_t> cols_a, cols_b;  // p x wa, p x wb: right-aligned, padded with column 0
  } product;
  // gradient by xb on the product (product.cpp, kernels_product_dx.hip): per dimension of dims_b the view of
  // the terms that have it, against the tables of `product` for the same split and caps.  An entry is
  // wa / 2 words of the term's A columns, wb / 2 words of its OTHER B columns (own slot = the ones column),
  // its own used B column and its term index.
  struct ProductGrad {
    std::vector<uint32_t> dims_b;      // key, as in Product
    std::vector<int64_t> cap;
    std::vector<uint32_t> voff_h;      // |B| + 1: first entry of every B dimension
    obhip::DevBuf<uint32_t> voff;      // the same on the device
    obhip::DevBuf<uint32_t> vw;        // entries x (wa / 2 + wb / 2 + 2) words
  } product_grad;
  int prepare(const std::vector<int64_t> &cap, const std::vector<obhip::DimDesc> &dims);
};

// ---- hyper-parameter gradient tables (device) -------------------------------------
namespace obhip {
struct GradHyp {
  int dim;      // dimension of this hyper-parameter
  int which;    // its index within the dimension (0 or 1)
  int rotgoff;  // offset into rotg (doubles), block [m][ncolp] like ModelDev::rot
  int gecol;    // first gradient column of this hyper-parameter in the combined tile
  int dcol;     // first delta column: delta[t] = ge[t] - basemat[level t] ge[0], t >= 1
};
}  // namespace obhip

struct obhip_basis;
// gradient basis of an outerbase (outerbase::build with dograd, modandbase.cpp:547-626):
// a second tile-blocked array holding the basemat columns AND, behind them, for every
// hyper-parameter h the columns basemat_gradhyp[:, gest[h] + t], t = 0..cap -- laid out
// so that the ordinary product kernels can run on it with per-hyper-parameter term views.
struct obhip_gradbasis {
  uint64_t model_version = ~0ull;
  uint64_t id = 0;  // unique per build: tables derived from the column layout are keyed by it
  std::vector<obhip::GradHyp> hyps_h;
  obhip::DevBuf<obhip::GradHyp> hyps;
  obhip::DevBuf<int> ge0col;   // gecol of every hyper-parameter (the level-0 gradient columns), device
  obhip::DevBuf<double> rotg;  // per hyper-parameter [m][ncolp]
  obhip::DevBuf<double> kd;    // per knot: log(knot) * t(knot) (mat25pow), else 0
  std::unique_ptr<obhip_basis> gb;    // combined array + extended dimension table
  std::unique_ptr<obhip_basis> gbsq;  // its squared store (basematsq / basematsq_gradhyp)
};

// ---- outerbase ------------------------------------------------------------------
struct obhip_basis {
  const obhip_model *model = nullptr;
  uint64_t n = 0, n_pad = 0, d = 0;
  obhip::ModelDev md;
  obhip::DevBuf<double> x;      // column-major n x d (ld = n)
  obhip::DevBuf<double> bm;     // tile-blocked [n_pad/64][Mc][64]
  obhip::DevBuf<double> scale;  // n_pad (0 beyond n)
  obhip::DevBuf<char> work;     // scratch for split-reduction partials (grown on demand)
  obhip::DevBuf<double> bmat;   // row-major design matrix [n_pad][p_pad], staging of the
                                // materialised-B Gram kernel (allocated on first use)
  uint64_t bmat_terms = 0;      // uid of the terms bmat currently holds (0: none)
  uint64_t bmat_order = 0;      // GramOrder::serial of the column order it holds them in (0: the terms' own)
  struct GramTable {            // XCD-aware (tile pair, row split) task order of that kernel ...
    obhip::GramKey key;         // ... and what it was built for (no shape: no table)
    obhip::DevBuf<uint64_t> tab;
    obhip::DevBuf<uint32_t> wbytes;  // the four wave bytes of every task (packed plan; unused otherwise)
    bool packed = false;
  } gram_table;
  std::unique_ptr<obhip_gradbasis> grad;  // built on first *_gradhyp call, dropped on rebuild
  int device = 0;
  int workspace(size_t bytes, void **out) {
    if (work.n < bytes) {
      // the previous kernels may still be reading the old buffer
      if (work.p && hipStreamSynchronize(obhip::cur_stream()) != hipSuccess)
        return obhip::fail(OBHIP_ERR_HIP, "stream sync failed");
      int rc = work.alloc(bytes + bytes / 4);
      if (rc) return rc;
    }
    *out = work.p;
    return 0;
  }
};

namespace obhip {

// owns a basis that a call makes for itself
struct BasisGuard {
  obhip_basis *b = nullptr;
  ~BasisGuard() { obhip_basis_destroy(b); }
};
// rows of one call that the entries with 64-bit row indices and 32-bit tile counts take
constexpr uint64_t kMaxRowsPerCall = 1ull << 40;

constexpr int kTileRows = 64;
static_assert(kTileRows == kGramRowTile, "gram_plan.h sizes row chunks in these tiles");
// LDS of a workgroup on gfx950: what the fused kernels size their tiles against
constexpr size_t kLdsBudget = 160 * 1024;
// the largest tile the term-per-lane and star kernels were measured to run with: what their
// *_supports functions admit.  Not the budget above: the 4 KB between them are left to the
// compiler's own LDS and to the allocation granule
constexpr size_t kLdsTile = 156 * 1024;
// doubles of LDS k_build_basis has for one dimension's interval tables; ModelDev::build makes
// tables only for dimensions whose tables fit (larger ones would be per-lane global gathers, no
// faster than the knot loop, and cost the host O(knots^2 x levels) per hyper-parameter update)
constexpr int kIntervalTabMax = 2048;

// kernels_basis.hip
int launch_build_basis(obhip_basis &b);
int launch_getbase(const obhip_basis &b, uint64_t k, double *d_out /* n x m */);
// kernels_prod.hip
int launch_getmat(const obhip_basis &b, obhip_terms &t, double *d_out, uint64_t ld = 0);
int launch_mm(const obhip_basis &b, obhip_terms &t, const double *d_a,
              double *d_out, bool squared);
int launch_tmm(const obhip_basis &b, obhip_terms &t, const double *d_a,
               double *d_out, bool squared);
// d_out (p) = B^T (c_a B a + c_b y) in ONE pass over the basis; d_yhat (n) = B a and d_ss (1) =
// sum (B a - y)^2 when asked for.  Returns kNotFused (nothing done) when the terms do not fit the
// fused kernel: the caller then composes launch_mm / launch_tmm.
constexpr int kNotFused = -1;
// d_stop0 / d_stop1 (device scalars, may be null): the launch does nothing when either is non-zero
// at the time it RUNS -- for launches enqueued before the host knows whether they are needed; only
// where hessmult_fused_skippable says so
// then (may be null): q[k] = e2 d_out[k] + prec[k] pv[k] written by the reduction of the row-split
// partials as well -- the PCG's q = H pv (lpdfvec::hessmult, fit.cpp:382-392) without a launch of its own
struct HmThen {
  double e2;
  const double *prec, *pv;
  double *q;
};
int launch_hessmult_fused(const obhip_basis &b, obhip_terms &t, const double *d_a, const double *d_y,
                          double ca, double cb, double *d_out, double *d_yhat, double *d_ss,
                          const double *d_stop0 = nullptr, const double *d_stop1 = nullptr,
                          const HmThen *then = nullptr);
bool hessmult_fused_skippable(const obhip_basis &b, obhip_terms &t);
// d_out = B^T a and d_out2 = (B^2)^T a2 (a2 null: ones) in one pass; kNotFused: make two passes
int launch_tmm_dual(const obhip_basis &b, obhip_terms &t, const double *d_a, double *d_out, const double *d_a2,
                    double *d_out2);
// kernels_generic.hip: any number of used columns / factors, columns read from HBM
int launch_mm_generic(const obhip_basis &b, obhip_terms &t, const double *d_a, double *d_out, int mode,
                      uint64_t ld);
int launch_tmm_generic(const obhip_basis &b, obhip_terms &t, const double *d_a, double *d_out,
                       bool squared);
int launch_materialize_generic(const obhip_basis &b, obhip_terms &t, double *d_B);
// kernels_star.hip: the kernels on shared sub-products (stars of four terms), from 9 star-waves up
bool star_supports(const obhip_terms &t, bool one_block, bool dual = false);
int launch_star_hess(const obhip_basis &b, obhip_terms &t, const double *d_a, const double *d_y, double ca,
                     double cb, double *part, double *d_yhat, double *sspart, unsigned nsplit, uint64_t ntiles,
                     uint64_t tps, const double *stop0, const double *stop1);
int launch_star_tmm(const obhip_basis &b, obhip_terms &t, const double *d_a, bool squared, double *part,
                    const double *d_a2, double *part2, unsigned nsplit, uint64_t ntiles, uint64_t tps);
int launch_star_mm(const obhip_basis &b, obhip_terms &t, const double *d_a, bool squared, double *d_out,
                   double *mpart, unsigned nsplit, uint64_t ntiles, uint64_t tps);
bool star_predict_supports(const obhip_terms &t);
int launch_star_predict(const obhip_model &m, obhip_terms &t, const double *d_theta, const double *d_x, uint64_t n,
                        double *d_mean, const double *d_coeffvar, double e2sigma, double *d_var);
// kernels_hm.hip: the second-generation kernel (two tile buffers fed by LDS-direct loads, four
// waves per SIMD) and the terms it takes
bool hm2_supports(const obhip_terms &t, bool ro);
int launch_hm2(const obhip_basis &b, obhip_terms &t, const double *d_a, const double *d_y, double ca,
               double cb, double *part, double *d_yhat, double *sspart, unsigned nsplit, uint64_t ntiles,
               uint64_t tps, const double *stop0, const double *stop1);
// kernels_gram.hip
// where k_gram_reduce puts the summed tiles: full symmetric p x p (raw G, or with `form` the
// Hessian e2 G + diag(prec) and its diagonal) or the packed upper triangle of a row-sharded
// fit's exchange buffer
struct GramSink {
  double *out = nullptr;
  bool packed = false;
  bool form = false;
  double e2 = 1.0;
  const double *prec = nullptr;  // p, device
  double *diagH = nullptr;       // p, device, may be null
};
// a fit's request to take g = B^T y along when the design matrix is staged (the staging pass
// forms every entry of B anyway); `done` tells the caller whether that pass ran and did it --
// not when the staged matrix of these terms was still valid, nor on the chunked / fused paths
struct GramFuse {
  const double *y = nullptr;  // n, device
  double *g = nullptr;        // p, device
  bool done = false;
};
int launch_gram(const obhip_basis &b, obhip_terms &t, double *d_G);
int launch_gram_to(const obhip_basis &b, obhip_terms &t, const GramSink &sink, GramFuse *fuse = nullptr);
// skip (device, may be null): per tile pair one bit per quadrant (2 row + column) whose partials were never
// written and that is left alone (0x0f: the whole pair)
// perm (device, may be null): the partials are in Gram order, entry (gi, gj) belongs to terms perm[gi], perm[gj]
int launch_gram_reduce(const double *part, int npairs, int nsplit, int nb, int p, const GramSink &sink,
                       bool accumulate, bool last, const uint8_t *skip = nullptr, const uint32_t *perm = nullptr);
// gram_dedup.hip: *out = the redundant tile pairs of t's term set, nullptr when there are none (or
// OBHIP_GRAM_DEDUP=0); launch_gram_fill copies their entries from their sources in the sink
int gram_dedup_get(obhip_terms &t, const GramDedup **out);
int launch_gram_fill(const GramDedup &dd, int p, const GramSink &sink);
// the analysis at wave-tile granularity and its packed plan (OBHIP_GRAM_DEDUP_QUADS): *out = t.dedup.quads when the
// launch of this shape at this split is to run it (forced, or it saves a block per split and more modelled
// time than its set-up took), nullptr otherwise; launch_gram_fill_quads copies the dropped wave tiles' entries
int gram_quads_get(obhip_terms &t, const GramShape &shape, const GramPlan &plan, const uint8_t *skip, uint64_t skip_sig,
                   const GramDedup::Quads **out);
int launch_gram_fill_quads(const GramDedup::Quads &q, int p, const GramSink &sink, const uint32_t *perm = nullptr);
// the column order of t's Gram (OBHIP_GRAM_ORDER): *out = &t.order when the launch of this shape at this split is
// to stage and multiply its columns in Gram order -- forced, or the ordered packed plan saves a block per split
// against the plan the launch would otherwise take (price_other: its gram_cost and blocks per split, asked for only
// when a decision has to be taken) and kGramOrderLaunches launches save more modelled time than the set-up costs;
// nullptr otherwise
int gram_order_get(obhip_terms &t, const GramShape &shape, const GramPlan &plan, uint64_t other_sig,
                   const std::function<void(double &, int &)> &price_other, const GramOrder **out);
int gram_order_mode();  // 1 forced, 0 forbidden, -1 the model decides
int gram_order_cols(obhip_terms &t);  // t.order.cols = t.cols with its rows in Gram order
void set_gram_backend(int b);
int get_gram_backend();
// kernels_gram_panel.hip
// order (may be null): the columns in that order, and the fused B^T y scattered back to the terms
int launch_materialize_rows(const obhip_basis &b, obhip_terms &t, double *d_B, GramFuse *fuse = nullptr,
                            const GramOrder *order = nullptr);
// b.bmat = design matrix of (b, t) with its columns in `order` (null: the terms' own); staged anew when it holds
// other terms or another order
int ensure_bmat(obhip_basis &b, obhip_terms &t, GramFuse *fuse = nullptr, const GramOrder *order = nullptr);
bool gram_panel_supports(const obhip_basis &b, const obhip_terms &t);
// partial tiles of B^T B over the ntiles x 64 rows staged at d_B (pitch p_pad), reduced into the sink; holder
// lends its device, workspace and task table (grad_obs.cpp stages rows of its own)
// order: the one d_B was staged in (launch_gram_panel alone passes one: the other callers stage rows of their own)
int gram_of_staged(obhip_basis &holder, const double *d_B, uint64_t ntiles, obhip_terms &t, const GramSink &sink,
                   bool accumulate, bool last, const GramOrder *order = nullptr);
// C = A^T Bm on the matrix cores (kernels_gram_panel.hip): kAtbNorm = row norms of C into
// out[J * ldo + i] per 128-column tile J, kAtbStore = C stored row-major with ldo, kAtbStoreFixed = the same with
// every entry summed over k in one order wherever it stands (kAtbStore rotates a tile's start by its indices);
// kAtbGram is gram_of_staged's own
constexpr int kAtbGram = 0, kAtbNorm = 1, kAtbStore = 2, kAtbStoreFixed = 3;
int launch_atb(int mode, const double *A, uint64_t ldA, uint64_t M, const double *Bm, uint64_t ldB,
               uint64_t N, uint64_t K, bool tri, double *out, uint64_t ldo);
// kernels_trtri.hip: X (pp x pp, zeroed) = L^-T in its upper triangle; transpose of an n x n block
int launch_trtri_lt(const double *d_L, uint64_t ldl, uint64_t p, double *d_X, uint64_t pp,
                    double *d_dinv);
int launch_transpose(const double *d_in, uint64_t ldi, double *d_out, uint64_t ldo, uint64_t n);
// posterior.cpp: Cholesky factor of the total Hessian and X = L^-T for predr_std
struct PostFactor {
  uint64_t p = 0, pp = 0;  // pp = p rounded up to 128
  DevBuf<double> L;        // p x p row-major, lower triangle = L
  DevBuf<double> X;        // pp x pp row-major, upper triangle = L^-T, zero elsewhere
};
int post_factor_build(const double *d_H, uint64_t p, PostFactor &f, bool want_inverse);
// S (pp x pp, allocated here) = inv(H) = X X^T of a factor built with its inverse; waits for it
int post_factor_inverse(const PostFactor &f, DevBuf<double> &S);
int factor_logdet(const PostFactor &f, double *logdet);  // log det H from the diagonal of L; waits
int post_var_dev(const obhip_model &m, obhip_terms &t, const PostFactor &f, const double *d_x,
                 uint64_t n, double e2sigma, double *d_var);
// obhip_margadj_full in its two parts, so that a row-sharded likelihood can sum the first over its ranks:
// rows[l] = e^{-2 sigma} tr(inv(H) B^T Bge_l) for l < nhyp and rows[nhyp] = e^{-2 sigma} tr(inv(H) B^T B) over
// the rows of THIS basis, prior[l] = sum_k inv(H)_kk prec_k lvarge_kl and prior[nhyp] = sum_k inv(H)_kk prec_k
// (both may be null: val only)
int margadj_full_parts(const obhip_basis *b, const obhip_terms *t, const obhip_model *m, const double *H,
                       double sigma, double rho, double *val, double *rows, double *prior);
}  // namespace obhip
// posterior.cpp: the device-resident posterior of one model and term set (include/obhip.h)
struct obhip_posterior {
  const obhip_model *model = nullptr;
  const obhip_terms *terms = nullptr;
  uint64_t p = 0;
  double sigma = 0.0, logdet = 0.0;
  obhip::DevBuf<double> H;  // p x p, symmetric
  obhip::PostFactor f;
  // S = inv(H) = X X^T (pp x pp), built by the first call that needs it (posterior_inverse), freed with the handle
  mutable obhip::DevBuf<double> S;
  mutable std::mutex S_lock;
};
namespace obhip {
// *out = a new handle that takes the symmetric p x p d_H over (copied); waits for the factorisation
int posterior_from_hessian(obhip_posterior **out, const obhip_model *m, const obhip_terms *t, const double *d_H,
                           double sigma);
// posterior.cpp: *S = the handle's inv(H), formed by post_factor_inverse on first use and read-only from then on:
// launch_design_pspace downdates its S in place, so the selection entries work on a copy
int posterior_inverse(const obhip_posterior &post, const double **S);
// posterior.cpp: what the entries on a handle refuse, in the texts they have always had.  check_post_handle: a null
// handle, check_compat, then p (cap_p: "... disagree on p (or p > 65535)", else "the terms changed since ...")
int check_post_handle(const std::string &who, const obhip_posterior *post, bool cap_p);
int check_acq_criterion(const std::string &who, int criterion);                        // the range
int check_acq_params(const std::string &who, int criterion, const double *params);   // null, best, xi, kappa, level
// design.cpp / kernels_design.hip: one greedy step of the sequential design over the candidates (fused: the
// basis of a 64-row tile in LDS, a = B s and c = B h on the matrix cores, downdate, score and argmax in
// the epilogue) and the p-space work between two steps
// design.cpp: b_i^T Q b_i (norms false) or || X^T b_i ||^2 (norms true) at the n rows of d_x, a stored product
// and one ascending sum per row.  fixed_order: the stored product by launch_atb's kAtbStoreFixed, and only then do
// bit-identical rows get bit-identical results wherever they stand (without it: when their 128-row tiles of a
// chunk have the same index mod 8 -- what obhip_design_select has always returned)
int row_forms_dev(const obhip_model &m, obhip_terms &t, const double *d_Q, bool norms, uint64_t p, uint64_t pp,
                  const double *d_x, uint64_t n, double *d_out, bool fixed_order = false);
constexpr int kDesignScal = 8;  // doubles of the step's scalar block: gamma, tau, d_j, nu, -, nothing left, -, -
struct DesignStep {
  int crit = 0;
  bool replace = false;
  uint64_t n = 0;
  const double *x = nullptr;        // candidates, column-major n x d
  const double *w = nullptr;        // weights or null
  const double *sh = nullptr;       // [p][16] term-major: column 0 = s, column 1 = h, the rest zero
  const double *scal = nullptr;     // kDesignScal doubles the previous step wrote
  double *dvar = nullptr, *num = nullptr;  // n each (num: IMSE only)
  const uint8_t *picked = nullptr;  // n
  double *part_score = nullptr;     // per workgroup
  int64_t *part_idx = nullptr;
};
bool design_step_supports(const obhip_terms &t);
uint64_t design_step_parts(uint64_t n, bool fused);
int launch_design_step(const obhip_model &m, obhip_terms &t, const DesignStep &s);
// the same downdate, score and argmax with a = ac[i] and c = ac[n + i] read from HBM
int launch_design_update(const DesignStep &s, const double *d_ac);
// part[] -> the step's pick: index and score appended at slot `step`, x_j gathered into d_xj (1 x d), the row
// marked in picked; no eligible candidate: scal[5] = 1 and nothing else written
int launch_design_pick(const DesignStep &s, uint64_t nparts, uint64_t d, uint64_t step, int64_t *d_index,
                       double *d_score, double *d_xj, uint8_t *d_picked, double *d_scal);
// s = S b, h = T b (T null: h = 0), gamma = nu + b.s, tau = b.h into scal, trace[step + 1], the [p][16] block,
// then S -= s s^T / gamma and T -= (s h^T + h s^T) / gamma - s s^T tau / gamma^2
int launch_design_pspace(int crit, uint64_t p, uint64_t pp, const double *d_b, double *d_S, double *d_T, double *d_sv,
                         double *d_hv, double *d_sh, double *d_scal, double *d_trace, uint64_t step);
// design.cpp: the working set and the step loop that obhip_design_select_dev and obhip_acquire_dev share
struct GreedyPicks {
  obhip_terms *terms = nullptr;
  uint64_t p = 0, pp = 0, d = 0;
  DevBuf<double> S;        // pp x pp: a copy of the handle's inverse, downdated by every pick
  DevBuf<double> vec;      // s | h, the two columns launch_design_pspace writes
  DevBuf<double> sh;       // its [p][16] block
  DevBuf<double> scal;     // the step's scalar block, seeded from scal0 by run
  DevBuf<double> trace;    // k + 1
  DevBuf<double> bj, xj0;  // the picked row's basis (p) and where the pick kernels gather its x (d)
  DevBuf<double> pscore;   // nparts partial pairs
  DevBuf<int64_t> pidx;
  DevBuf<uint8_t> picked;  // m
  BasisGuard one;          // the one-row basis b_j is evaluated with
  std::vector<double> scal0;  // {1, 0, 0, nu, 0, ..}: gamma = 1, nothing to downdate; the entry may fill its own slots
  // allocates, zeroes and seeds all of the above for m candidates, k picks, nscal scalars and nparts partials
  int init(const obhip_posterior &post, const double *d_xcand, uint64_t m, uint64_t k, uint64_t nscal,
           uint64_t nparts);
  // k steps of pass(step), pick(step), the host wait for the nothing-left flag, b_j and the p-space kernels with
  // the criterion and T (null: no h), then pass(npicked) for the last pick's downdate; *npicked <= k
  int run(uint64_t k, int crit, double *d_T, const std::function<int(uint64_t)> &pass,
          const std::function<int(uint64_t)> &pick, uint64_t *npicked);
};
// acquire.cpp / kernels_acquire.hip: acquisition picks (include/obhip.h, "acquisition picks")
// the step's scalar block: the kDesignScal doubles launch_design_pspace writes, then delta = y* - mu_j and the
// incumbent (in the sign the criterion is scored with)
constexpr int kAcqDelta = kDesignScal, kAcqBest = kDesignScal + 1, kAcqScal = kDesignScal + 2;
struct AcqStep {
  int crit = 0, lie = 0;
  uint64_t n = 0;
  double sgn = 1.0, xi = 0.0, kappa = 0.0, level = 0.0, lie_value = 0.0;  // level: signed; lie_value: as given
  const double *x = nullptr;       // candidates, column-major n x d
  const double *a = nullptr;       // n: b_i^T s of the previous pick (zeros before the first)
  const uint8_t *elig = nullptr;   // n: launch_sample_elig's map
  uint8_t *picked = nullptr;       // n
  double *mu = nullptr, *dvar = nullptr;  // n each
  double *scal = nullptr;          // kAcqScal doubles
  double *part_score = nullptr;    // per workgroup of 256 rows
  int64_t *part_idx = nullptr;
};
constexpr uint64_t kAcqRows = 256;
// downdate of every candidate by the previous pick, its score, one (best score, lowest index) pair per workgroup;
// d_score0 (may be null): every row's score as formed
int launch_acq_update(const AcqStep &s, double *d_score0);
// the partial pairs -> the step's pick: index and score appended at slot `step`, the row marked, x_j gathered
// into d_xj, delta and the incumbent into scal; no eligible candidate: scal[5] = 1 and nothing else written
int launch_acq_pick(const AcqStep &s, uint64_t d, uint64_t step, int64_t *d_index, double *d_score, double *d_xj);
// acquire_multi.cpp / kernels_acquire_multi.hip: acquisition picks over several responses (include/obhip.h,
// "acquisition over several responses").  The state block of a call, in doubles: per response
// (16 slots each) delta = y* - mu_j, the sign g, the signed limit cs (a constraint's limit, an EHVI objective's
// reference coordinate), the lie value and the role; the signed incumbent of CEI / CPI; F; the front's first
// coordinates (ascending) and second coordinates, kMacqFrontCap + 1 slots each (acquire_front.h)
constexpr int kMacqDelta = 0, kMacqSign = 16, kMacqLimit = 32, kMacqLie = 48, kMacqRole = 64, kMacqBest = 80,
              kMacqF = 81, kMacqU = 82, kMacqC = kMacqU + 2048 + 1, kMacqState = kMacqC + 2048 + 1;
struct MacqStep {
  int crit = 0, lie = 0, q = 0, obj1 = -1, obj2 = -1;  // the objectives' response indices, -1: none
  uint64_t n = 0, front_cap = 0;   // front_cap: F never exceeds it during the call (the LDS of the update kernel)
  double xi = 0.0;
  const double *x = nullptr;       // candidates, column-major n x d
  const double *a = nullptr;       // n: b_i^T s of the previous pick (zeros before the first)
  const uint8_t *elig = nullptr;   // n: launch_sample_elig's map
  uint8_t *picked = nullptr;       // n
  double *mean = nullptr, *dvar = nullptr;  // n x q (leading dimension n), n
  double *scal = nullptr;          // kDesignScal doubles
  double *mst = nullptr;           // kMacqState doubles
  double *part_score = nullptr;    // per workgroup of 256 rows
  int64_t *part_idx = nullptr;
};
uint64_t macq_update_lds_bytes(int crit, uint64_t front_cap);
// downdate of every candidate by the previous pick (q means, one variance), its score, one (best score, lowest
// index) pair per workgroup; d_score0, d_pof0 (may be null): every row's score and feasibility factor as formed
int launch_macq_update(const MacqStep &s, double *d_score0, double *d_pof0);
// the partial pairs -> the step's pick as launch_acq_pick, the q deltas, the incumbent or the front into mst
int launch_macq_pick(const MacqStep &s, uint64_t d, uint64_t step, int64_t *d_index, double *d_score, double *d_xj);
// acquire_dx.cpp / kernels_acquire_dx.hip: input gradients of the latent variance and of the acquisition criteria
// (include/obhip.h, "acquisition gradients")
constexpr int kAdxNone = -1;  // no criterion: the variance and its gradient only
struct AcqDxArgs {
  double sgn = 1.0, best = 0.0, xi = 0.0, kappa = 0.0, level = 0.0;  // best, level: in the sign scored with
  double noise = 0.0;   // added to var
  uint64_t row0 = 0, ldo = 0;  // the chunk's first row and the leading dimension of every output
  double *score = nullptr, *gradscore = nullptr;  // n, n x d: required with a criterion
  double *mean = nullptr, *gradmean = nullptr, *var = nullptr, *gradvar = nullptr;  // may be null
};
bool acquire_dx_fused(const obhip_terms &t);  // predict_dx_supports and no OBHIP_FORCE_GENERIC
uint64_t acquire_dx_lds_bytes(const obhip_terms &t, uint64_t d, bool fused);
// one chunk: the n rows at d_x (column-major, leading dimension ldx) against their stored product d_Y = S B^T
// (term-major, pitch npad >= the rows' 64-row tiles, zeros behind row n); crit: kAdxNone or OBHIP_ACQ_*
int launch_acquire_dx(const obhip_model &m, obhip_terms &t, int crit, const double *d_theta, const double *d_Y,
                      uint64_t npad, const double *d_x, uint64_t ldx, uint64_t n, const AcqDxArgs &a);
// sample.cpp / kernels_sample.hip: draws from N(theta, inv(H)) and the per-draw extremum of their sample
// paths over a candidate set (include/obhip.h, "posterior draws")
constexpr uint64_t kDrawChunk = 64;  // draws of one launch of k_draw outside the fused pass (which takes up to 128)
// Theta_ks = theta_k + sum_{j >= k} X_kj z_js for the qc <= 128 columns of d_z, j ascending, theta added last:
// into the term-major [p][qw] block d_tht (columns qc .. qw - 1 zero; may be null) and the column-major
// p x qc d_Theta (leading dimension p; may be null)
int launch_draw(const PostFactor &f, const double *d_theta, const double *d_z, uint64_t ldz, int qc, uint64_t qw,
                double *d_tht, double *d_Theta);
// d_elig[i] = 1: row i of d_x (column-major n x d) is not skipped and all its coordinates are finite
int launch_sample_elig(const double *d_x, uint64_t n, uint64_t d, const uint8_t *d_skip, uint8_t *d_elig);
bool sample_ext_supports(const obhip_terms &t);
int sample_ext_nqb_max(const obhip_terms &t);  // widest pass (16 nqb draws, nqb <= 8) whose LDS fits
// One pass of the fused kernel over the n candidates for the 16 nqb columns of the term-major block d_tht:
// per workgroup (64 rows) and column the best key = sgn * value (sgn = +1: minimum, -1: maximum) among the
// eligible rows with a finite value and the lowest row that has it, into part_key / part_idx [block][16 nqb];
// no such row: +inf and INT64_MAX
int launch_sample_ext(const obhip_model &m, obhip_terms &t, const double *d_tht, int nqb, const double *d_x,
                      uint64_t n, const uint8_t *d_elig, double sgn, double *part_key, int64_t *part_idx);
constexpr uint64_t kColextRows = 256;  // rows per workgroup of k_sample_colext
// the same partials from nr rows of stored paths (d_path: nr x qc, leading dimension ld; global rows row0 ..),
// 256 rows per workgroup, into part_*[(row0 / 256 + block) * stride + column]
int launch_sample_colext(const double *d_path, uint64_t ld, uint64_t nr, uint64_t row0, int qc, const uint8_t *d_elig,
                         double sgn, uint64_t stride, double *part_key, int64_t *part_idx);
// per column the partials in ascending block order -> d_index[s] (-1: no eligible row), d_value[s] (NaN)
int launch_sample_pick(const double *part_key, const int64_t *part_idx, uint64_t nparts, uint64_t stride, int qc,
                       double sgn, int64_t *d_index, double *d_value);

// kernels_grad_basis.hip
int ensure_gradbasis(obhip_basis &b);     // b.grad = the gradient basis of b for the model's current state
int ensure_gradbasis_sq(obhip_basis &b);  // ... and b.grad->gbsq, its squared store
// grad_views.cpp: the views cached in t.ge, rebuilt when b's model lays its hyper-parameters out differently
// full view of hyper-parameter h (every term; level 0 picks up the gradient column too)
obhip_terms *grad_view(obhip_terms &t, const obhip_basis &b, uint64_t h);
// view of the terms that have h's dimension, its factor replaced by the gradient column (delta: the delta
// column); *idx = their term indices; null when no term has the dimension
obhip_terms *grad_view_restricted(obhip_terms &t, const obhip_basis &b, uint64_t h, bool delta,
                                  const std::vector<uint32_t> **idx);
// those views concatenated a few hyper-parameters at a time, at most 128 used columns per group
std::vector<obhip_terms::GeGroup> &grad_view_groups(obhip_terms &t, const obhip_basis &b, bool delta);
// t.ge.d3 = the k_tmm_d3 groups for b.grad's column layout; false: a view does not fit, or OBHIP_GRAD_D3=0
bool build_d3_groups(obhip_terms &t, const obhip_basis &b);
// kernels_grad_dense.hip: d_out (device, p x nhyp column-major) = sum_i a_i ge[h, 0]_i B_ik (squared: of
// the squared stores), enqueued on the current stream; t prepared for b, b.grad built
bool tmm_ge0_supports(const obhip_terms &t);  // at most 8 column slots and the tile within the LDS
// the launch geometry of launch_tmm_ge0: what it runs and what obhip_grad_plan_info reports
struct Ge0Pass {
  int h0, nh;  // hyper-parameters h0 .. h0 + nh - 1
  int n4;      // > 0: a 16-block and n4 groups of four; < 0: |n4| groups of four only; 0: the 16-block only
  int hs;      // hyper-parameter slots of the pass' partial sums
};
struct Ge0Geom {
  int nw;  // 8 | 16: k_tmm_ge0 with that many waves; 32: k_tmm_ge0_db (16 waves, two tile buffers)
  uint64_t pblocks, nsplit, tps;
  std::vector<Ge0Pass> passes;
};
Ge0Geom ge0_geometry(const obhip_basis &b, const obhip_terms &t);
int launch_tmm_ge0(obhip_basis &b, obhip_terms &t, bool squared, const double *d_a, double *d_out);
// (from the materialised design matrix; squared: b.grad->gbsq built)
struct BtuGeom {
  int nhb;  // hyper-parameters per pass
  unsigned gy;
  uint64_t nsplit, tps;
};
BtuGeom btu_geometry(const obhip_basis &b, const obhip_terms &t);
int launch_bt_times_ge0(obhip_basis &b, obhip_terms &t, bool squared, const double *d_a, double *d_out);
// kernels_grad.hip: device-level forms (inputs and n-sized results in HBM) for the likelihood classes
int grad_mm_dev(obhip_basis &b, obhip_terms &t, bool squared, const double *a_host, const double *d_a,
                double *d_M, DevBuf<double> &dge);
int grad_mm_dot_dev(obhip_basis &b, obhip_terms &t, const double *a_host, const double *d_M,
                    const double *d_w, double *out_host);
// staging class of a column of a k_tmm_d3 tile, in bits 28-29 of its entry in the group's ucol list
constexpr uint32_t kD3Delta = 1u << 28, kD3Own = 2u << 28, kD3ColMask = (1u << 28) - 1;
constexpr int kD3Pre = 20;  // k_tmm_d3: prefetch registers per thread => at most 8 * 20 columns per group
// one group of obhip_terms::ge.d3 (kernels_grad_d3.hip): d_out (device, [2 nh][v.p]) = u1 of the
// group's first hyper-parameter, of its second, u2 likewise; mode bit 0: u1, bit 1: u2
int launch_tmm_d3(obhip_basis &b, const obhip_terms::GeD3 &g, int mode, const double *d_w1, const double *d_w2,
                  double *d_out);
// its launch geometry: what it runs and what obhip_grad_plan_info reports
struct D3Geom {
  int nu;  // view-terms per lane: 2 (tile prefetched into registers) or 4 (two half-runs)
  uint64_t pblocks, nsplit, tps;
};
D3Geom d3_geometry(const obhip_basis &b, const obhip_terms::GeD3 &g);
int grad_dual_dev(obhip_basis &b, obhip_terms &t, const double *a_host, const double *d_M, const double *d_w1,
                  const double *d_w2, double *out_dot, double *out_sq);
int grad_wdot_dev(const double *d_G, const double *d_w, uint64_t n, uint64_t ncol, double *out_host);
int grad_tmm_host(obhip_basis &b, obhip_terms &t, bool squared, const double *d_a, double *out_host);
// kernels_chol.hip
uint64_t newton_workspace_bytes(uint64_t p);
bool materialize_tl_supports(const obhip_terms &t);
int launch_materialize_tl(const obhip_basis &b, obhip_terms &t, double *d_B, const double *d_y = nullptr,
                          double *d_g = nullptr, const GramOrder *order = nullptr);
int launch_newton_solve(uint64_t p, double *d_H, const double *d_rhs,
                        double *d_theta, void *d_ws, uint64_t ws_bytes);
int launch_form_hessian(uint64_t p, double *d_G, const double *d_prec,
                        double e2, double *d_diagH);
const double *newton_workspace_iinv(uint64_t p, const void *d_ws);
// kernels_multi.hip: the batched passes of the multi-response fit and predictor (fit_newton.cpp)
uint64_t multi_solve_scratch_bytes(uint64_t p);
// Fewest columns worth a batched pass of B^T Y or the predictor: one pass costs the same for 1 to 16
// columns (d=20, n=1e6, p=4096: 5.6 ms and 9.1 ms) where the single-column kernels take 0.77 ms and
// 1.14 ms per column, so below eight columns the column loop is the faster one.
constexpr uint64_t kMultiMinCols = 8;
int launch_aty_multi(obhip_basis &b, const obhip_terms &t, const double *d_Y, uint64_t ldy, uint64_t q,
                     double *d_out, uint64_t ldo);
int launch_trsm_multi(uint64_t p, const double *d_L, const double *d_Iinv, const double *d_R, uint64_t ldr,
                      uint64_t q, double e2, double *d_Theta, void *d_scratch);
bool predict_multi_supports(const obhip_terms &t);
// d_T ([p][qw], term-major) = the qc <= qw columns of d_Theta (p x qc, leading dimension p), zero beyond them:
// the B operand of the multi-response predictors
int launch_theta_term_major(const double *d_Theta, uint64_t p, int qc, uint64_t qw, double *d_T);
int launch_predict_multi(const obhip_model &m, obhip_terms &t, const double *d_Theta, uint64_t q,
                         const double *d_x, uint64_t n, double *d_mean);
// kernels_product.hip / product.cpp: the predictor on the product of two input blocks (include/obhip.h,
// "product of two input blocks").  One call of the fused kernel or of the row route:
struct ProductCall {
  const double *theta = nullptr;     // p x q, leading dimension p
  uint64_t q = 1;
  const double *xa = nullptr, *xb = nullptr;  // na x |A|, nb x |B|, column-major without padding
  uint64_t na = 0, nb = 0;
  const double *coeffvar = nullptr;  // p or null
  double sigma = 0.0;
  double *mean = nullptr;            // store epilogue: mean[(r nb + j) lda + i] ...
  uint64_t lda = 0;
  double *var = nullptr;             // ... and var[j lda + i] (needs coeffvar)
  const double *y = nullptr, *obsvar = nullptr;  // likelihood epilogue (mean == nullptr, q == 1): ...
  double *part = nullptr;            // ... part[(w tiles_a + A tile) nb + j], w = 0: sum r^2 / v, 1: sum log v
};
constexpr uint64_t kProductTile = 64;  // rows of a side per workgroup (= kTileRows)
size_t predict_product_lds(uint64_t mu_a, uint64_t mu_b, uint64_t wa, uint64_t wb);
// the fused kernel's domain: both side tiles and the staging within kLdsBudget, column lists of even width
bool predict_product_supports(uint64_t mu_a, uint64_t mu_b, uint64_t wa, uint64_t wb);
// t.product and t.pred_md are prepared for the split (product.cpp: ensure_product_tables)
int launch_predict_product(const obhip_model &m, obhip_terms &t, const ProductCall &c);
// rows [j0, j0 + nj) x [i0, i0 + ni) of the product as full-width rows: d_X[l rows + (j - j0) ni + (i - i0)]
int launch_product_expand(const obhip_terms &t, const double *d_xa, uint64_t na, const double *d_xb, uint64_t nb,
                          uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj, double *d_X);
// d_mean[(r nb + j0 + jj) lda + i0 + ii] = d_src[r rows + jj ni + ii], r < q
int launch_product_scatter(const double *d_src, uint64_t q, uint64_t nb, uint64_t lda, uint64_t i0, uint64_t ni,
                           uint64_t j0, uint64_t nj, double *d_dst);
// the likelihood terms of a chunk of rows (d_var null: e2sigma), reduced per A tile in the fused kernel's order
int launch_product_lik_rows(const double *d_mean, const double *d_var, double e2sigma, const double *d_y,
                            const double *d_obsvar, uint64_t na, uint64_t nb, uint64_t i0, uint64_t ni, uint64_t j0,
                            uint64_t nj, double *d_part);
// d_out[w nb + j] = the partials of the A tiles added in ascending order
int launch_product_sum_tiles(const double *d_part, uint64_t tiles_a, uint64_t nb, double *d_out);
// *bad_out != 0: an entry of d_v (n) is negative or not finite (waits for the device)
int launch_check_nonneg(const double *d_v, uint64_t n, int *bad_out);
// kernels_product_dx.hip: the gradient by xb on the product (include/obhip.h, "gradient by xb"; DESIGN.md
// section 28).  One response; L = |dims_b|.
struct ProductGradCall {
  const double *theta = nullptr;     // p
  const double *xa = nullptr, *xb = nullptr;
  uint64_t na = 0, nb = 0;
  const double *coeffvar = nullptr;  // p or null: no variance part
  double sigma = 0.0;
  double *dmean = nullptr;           // store epilogue: dmean[(l nb + j) lda + i] ...
  uint64_t lda = 0;
  double *dvar = nullptr;            // ... and dvar likewise (needs coeffvar)
  const double *y = nullptr, *obsvar = nullptr;  // likelihood epilogue (dmean == nullptr): ...
  double *part = nullptr;            // ... part[(w tiles_a + A tile) nb + j], w < 2 + 2 L: chi2, logdet,
                                     // d chi2 / d xb_l (w = 2 + l), d logdet / d xb_l (w = 2 + L + l)
};
size_t product_grad_lds(uint64_t mu_a, uint64_t mu_b, uint64_t nb_dims, uint64_t wa, uint64_t wb);
// the gradient kernel's domain: the A tile, the B tile with its derivative and rho columns and the staging
// within kLdsBudget, column lists of even width
bool product_grad_supports(uint64_t mu_a, uint64_t mu_b, uint64_t nb_dims, uint64_t wa, uint64_t wb);
// t.product, t.product_grad, t.pred_md and t.dx.dtab are prepared for the split (product.cpp)
int launch_product_grad(const obhip_model &m, obhip_terms &t, const ProductGradCall &c);
// the row route's reduction: the likelihood terms and their gradients of a chunk of expanded rows (d_grad,
// d_gradvar: rows x d as obhip_predict_grad_dev writes them; d_var, d_gradvar null: e2sigma, no variance part)
// per A tile in the fused kernel's order, into the partials of ProductGradCall::part
int launch_product_lik_grad_rows(const obhip_terms &t, const double *d_mean, const double *d_var, double e2sigma,
                                 const double *d_grad, const double *d_gradvar, const double *d_y,
                                 const double *d_obsvar, uint64_t na, uint64_t nb, uint64_t i0, uint64_t ni,
                                 uint64_t j0, uint64_t nj, double *d_part);
// d_out[w nb + j], w < ncols = the partials of the A tiles added in ascending order
int launch_product_sum_tile_cols(const double *d_part, uint64_t tiles_a, uint64_t nb, uint64_t ncols, double *d_out);
// product.cpp: the split of the dimensions and what follows from the levels alone (no device)
struct ProductSplit {
  std::vector<uint32_t> dims_b;
  std::vector<int> side_a, side_b, dim_src;
  std::vector<std::vector<char>> seen;  // per dimension: level used by some term
  uint64_t mu_a = 1, mu_b = 1, wa = 2, wb = 2;
  bool fused = false;
};
// dims_b: 1 to d - 1 entries, strictly ascending, each < d -- refused with OBHIP_ERR_INVALID otherwise
int make_split(const char *who, const obhip_terms &t, const uint32_t *dims_b, uint64_t ndims_b, ProductSplit &s);
// one side's tables against the column layout of t.pred_md (after prepare_predict): cpos maps a compact column to the
// side's used column or -1, cols holds p x w right-aligned used-column indices, padded with column 0
void side_tables(const obhip_terms &t, const ProductSplit &s, const std::vector<int> &side, uint64_t w,
                 std::vector<int32_t> &cpos, std::vector<uint16_t> &cols);
// the device tables of the split (t.product), cached on the terms for the last split and column layout asked for
int ensure_product_tables(const obhip_model &m, obhip_terms &t, const ProductSplit &s);
// kernels_product_fit.hip / product_fit.cpp: the Newton fit on gridded data (include/obhip.h, "Newton fit on
// the product of two input blocks").  One side's staged matrix:
struct SideStage {
  int side = 0;                     // 0: A (rows of xa), 1: B (rows of xb)
  const double *x = nullptr;        // device, column-major with leading dimension ldx, n rows from x on
  uint64_t ldx = 0, n = 0;
  double *out = nullptr;            // out[i * pitch + k] = s_i prod of term k's factors on the side; rows n ..
  uint64_t pitch = 0;               // 64 ceil(n / 64) and columns p .. pcols as zeros
  uint64_t pcols = 0;
  double *colpart = nullptr;        // optional: [ceil(n / 64)][pitch] column sums per tile
};
// the staging kernel keeps the side's tile in LDS: at most 8 factors per term on the side, tile within kLdsBudget
bool materialize_side_supports(uint64_t mu, uint64_t w);
// t.product and t.pred_md are prepared for the split (ensure_product_tables)
int launch_materialize_side(const obhip_model &m, obhip_terms &t, const SideStage &s);
// responses per GEMM of the right-hand sides: the product W2 of a block stays within 1 GB
constexpr uint64_t kFitRespBlock = 8;
inline uint64_t product_fit_resp_block(uint64_t na_pad, uint64_t p_pad, uint64_t q) {
  return std::max<uint64_t>(1, std::min<uint64_t>(std::min(q, kFitRespBlock), (1ull << 27) / (na_pad * p_pad)));
}
// where Y[r][j][i] - c_r stands in the shifted copy: response blocks of rb, within a block [j][r][i] with i
// padded to ldp and j to nbp rows (zeros), so that a block is the K x M operand of launch_atb with K = j
__host__ __device__ inline uint64_t product_fit_ys_at(uint64_t r, uint64_t j, uint64_t i, uint64_t q, uint64_t rb,
                                                     uint64_t nbp, uint64_t ldp) {
  const uint64_t r0 = r / rb * rb, rc = (q - r0 < rb) ? q - r0 : rb;
  return r0 * nbp * ldp + (j * rc + (r - r0)) * ldp + i;
}
// d_mom_batch[4 r] = the shift (the state's, or Y[r][0][0] for an empty state), d_Ys = Y - shift in the layout of
// product_fit_ys_at, padding zeroed, then (mu, M2, n = na nb) per response in launch_acc_batch_moments' order
// over the na nb values; the padding lda - na of Y is never read.  d_part: kSumBlocks q doubles
int launch_product_fit_moments(const double *d_Y, uint64_t lda, uint64_t na, uint64_t nb, uint64_t q, uint64_t rb,
                               uint64_t nbp, uint64_t ldp, bool empty, const double *d_mom_state, double *d_mom_batch,
                               double *d_Ys, double *d_part);
// d_part[(rr ns + s) pitch + k] = sum over the rows i of split s of A[i][k] W2[rr ldw + i][k] (rows ascending),
// then d_R[(rr) p + k] (+)= the splits in ascending order; rc <= kFitRespBlock responses per pass over A
uint64_t product_rhs_splits(uint64_t na);
int launch_product_rhs_dot(const double *d_A, const double *d_W2, uint64_t pitch, uint64_t na, uint64_t ldw,
                           uint64_t rc, uint64_t p, bool accumulate, double *d_part, double *d_R);
// d_tri[e] += sign GA[e] GB[e] over the packed triangle, d_b1[k] = a1[k] b1[k]
int launch_acc_fold_hadamard(uint64_t p, double *d_tri, const double *d_GA, const double *d_GB, double sign);
int launch_hadamard(uint64_t p, const double *d_a, const double *d_b, double *d_out);
// OBHIP_ERR_INVALID for a split with more than 65535 used columns on a side (the column lists are 16-bit)
int check_side_columns(const char *who, const ProductSplit &s);
// the normal equations of one grid batch: the two sides' Grams as packed triangles (d_GA, d_GB) and
// [R | b1 | moments] in the accumulator's layout behind the triangle (d_tail); holder as grad_batch_normal_eq's
int product_batch_normal_eq(obhip_basis &holder, const obhip_model &m, obhip_terms &t, const ProductSplit &s,
                            const double *d_xa, uint64_t na, const double *d_xb, uint64_t nb, const double *d_Y,
                            uint64_t lda, uint64_t q, bool empty, const double *d_mom_state, double *d_GA,
                            double *d_GB, double *d_tail);
// kernels_glm.hip: the row pass between two Newton steps of the GLM fit (glm.cpp) and the response scale
// of its predictor.  eta_i = (eta ? eta[i] : o ? o[i] : 0) + (deta ? alpha deta[i] : 0); scale, scale_w and
// u have n rounded up to a multiple of 64 entries; scale_w == nullptr: a trial pass, only the sums
constexpr int kGlmSums = 3;  // sum a l over the finite rows, the sum of its magnitudes, the rows left out
struct GlmRows {
  int family = 0;
  uint64_t n = 0;
  const double *eta = nullptr, *deta = nullptr;
  double alpha = 0.0;
  const double *y = nullptr, *a = nullptr, *o = nullptr;
  double e2 = 1.0;  // e^{-2 sigma}, Gaussian family only
  const double *scale = nullptr;
  double *eta_out = nullptr, *mu = nullptr, *scale_w = nullptr, *u = nullptr;
};
// d_sums: kGlmSums doubles; d_part: kSumBlocks (vec_ops.h) * kGlmSums doubles of scratch
int launch_glm_rows(const GlmRows &r, double *d_sums, double *d_part);
// d_eta (n, in/out) += o; d_mu = inverse link; d_varmu = (d mu / d eta)^2 d_vareta; o, mu, varmu may be null
int launch_glm_response(int family, uint64_t n, const double *d_o, double *d_eta, const double *d_vareta,
                        double *d_mu, double *d_varmu);
// kernels_sobol.hip: moment tables of the 1-D bases over a product measure and the variance
// decomposition of the fitted mean on them (sobol.cpp; include/obhip.h, "variance-based sensitivity")
constexpr int kSobolTW = 128;  // terms per tile of the pair sum (= threads of its blocks)
constexpr int kSobolRC = 2;    // responses per chunk of the pair sum
inline int sobol_dim_chunk(uint64_t d) { return d <= 8 ? 8 : 24; }  // accumulated dimensions per pass
size_t sobol_pairs_lds(uint64_t d, uint64_t n_cov);                  // dynamic LDS of k_sobol_pairs
uint64_t sobol_part_doubles(uint64_t p, uint64_t d, uint64_t q);     // partials of the pair sum
// d_mean / d_cov: the packed tables; *flag_out != 0: a bad weight or a weight column without mass
int launch_dim_moments(const obhip_model &m, obhip_terms &t, const double *d_nodes, uint64_t n, uint64_t ldx,
                       const double *d_w, uint64_t ldw, double *d_mean, double *d_cov, int *flag_out);
// meta: obhip_terms::sobol_meta; d_excl (p x d) and d_u (p): scratch
int launch_sobol_first(const uint8_t *d_lev, const int *d_meta, uint64_t p, uint64_t d, uint64_t q, uint64_t lmax,
                       uint64_t sum_l, const double *d_Theta, const double *d_mtab, const double *d_ctab, double *d_excl,
                       double *d_u, double *d_out, double *d_g);
int launch_sobol_pairs(const uint8_t *d_lev, const int *d_meta, uint64_t p, uint64_t d, uint64_t q, uint64_t n_cov,
                       const double *d_Theta, const double *d_mtab, const double *d_ctab, double *d_part, double *d_out);
int launch_main_effect(const obhip_model &m, obhip_terms &t, uint64_t dim, const double *d_g, uint64_t q,
                       const double *d_grid, uint64_t G, double *d_out);
// second-order and total-interaction variances and the interaction surface
constexpr int kSobol2T = 5;  // dimensions per block of the d x d triangle of outputs: T x T accumulators per pass
inline int sobol2_reg_dims(uint64_t d) { return d <= 8 ? 8 : 24; }  // dimensions whose row offsets stay in registers
size_t sobol2_pairs_lds(uint64_t n_cov);                             // dynamic LDS of k_block_pairs<Sobol2Op>
// pairs: obhip_terms::sobol_pairs; gmax: the largest L_i L_j; d_out q x 2 n_pairs (the V2 half), d_G may be null
int launch_sobol2_second(const uint8_t *d_lev, const int *d_meta, const int *d_pairs, uint64_t p, uint64_t d, uint64_t q,
                         uint64_t n_pairs, uint64_t n_G, uint64_t gmax, const double *d_Theta, const double *d_mtab,
                         const double *d_ctab, double *d_out, double *d_G);
// the VT2 half of d_out; d_part: pair_part_doubles (sens_plan.h) at kSobol2T, kSobolRC
int launch_sobol2_pairs(const uint8_t *d_lev, const int *d_meta, uint64_t p, uint64_t d, uint64_t q, uint64_t n_cov,
                        const double *d_Theta, const double *d_mtab, const double *d_ctab, double *d_part,
                        double *d_out);
// d_Gij: G of the pair (di, dj) of response 0, response j at j * n_G
int launch_interaction_effect(const obhip_model &m, obhip_terms &t, uint64_t di, uint64_t dj, const double *d_Gij,
                              uint64_t n_G, uint64_t q, const double *d_grid_i, uint64_t Gi, const double *d_grid_j,
                              uint64_t Gj, double *d_out);
// kernels_shapley.hip: Shapley effects of players (groups of dimensions), DESIGN.md section 29
constexpr int kShapMaxPlayers = 40;                   // = the register slots of the widest instantiation
constexpr int kShapMaxNodes = kShapMaxPlayers / 2;    // Gauss-Legendre nodes: ceil(P / 2)
inline int shapley_slots(uint64_t d) { return d <= 8 ? 8 : d <= 24 ? 24 : 40; }  // NS: register slots per pair
inline int shapley_rc(uint64_t d) { return d <= 24 ? 2 : 1; }                     // responses per chunk at that NS
// What the pair kernel sweeps, passed by value (kernel arguments: scalar loads).  The dimensions in sweep order
// `perm`, every player's dimensions contiguous; slot s < ns holds a run of that order, all of one player: its last
// dimension regdim[s], whose row offset is in a register of the lane, behind nmem (a byte per slot, four to a
// word) dimensions that are read per pair.  Bit s of lastmask: the player ends at slot s and its effect is
// accumulated there; slot[g]: that slot.
struct ShapPlan {
  double node[kShapMaxNodes], wt[kShapMaxNodes];
  unsigned long long lastmask;
  uint32_t nmem[kShapMaxPlayers / 4];
  int ns, nnode, nplayers;
  uint8_t perm[256], regdim[kShapMaxPlayers], slot[kShapMaxPlayers];
};
size_t shapley_pairs_lds(uint64_t d, uint64_t n_cov);               // dynamic LDS of k_shapley_pairs
uint64_t shapley_part_doubles(uint64_t p, uint64_t d, uint64_t q);  // partials of its pair sum
// d_out: q x nplayers row-major
int launch_shapley_pairs(const ShapPlan &plan, const uint8_t *d_lev, const int *d_meta, uint64_t p, uint64_t d,
                         uint64_t q, uint64_t n_cov, const double *d_Theta, const double *d_mtab, const double *d_ctab,
                         double *d_part, double *d_out);
// kernels_active.hip: E[grad f grad f^T] and E[grad f] of the fitted mean in closed form, DESIGN.md section 31
constexpr int kActiveT = 5;   // dimensions per block of the d x d triangle of outputs (diagonal included)
constexpr int kActiveRC = 2;  // responses per chunk of the pair sum
int active_moment_threads(uint64_t lmax);                           // threads per block of the derivative moments
size_t active_moments_lds(uint64_t lmax);                           // and their dynamic LDS (kernels_moments.hip)
size_t active_pairs_lds(uint64_t n_cov);                            // dynamic LDS of k_block_pairs<ActiveOp>
// the exclusion products of launch_sobol_first alone (kernels_sobol.hip): d_excl p x d, d_u p
int launch_sobol_excl(const uint8_t *d_lev, const int *d_meta, uint64_t p, uint64_t d, const double *d_mtab,
                      double *d_excl, double *d_u);
// d_dmean / d_cross / d_dd: the packed tables; *flag_out != 0: a bad weight or a weight column without mass
int launch_dim_grad_moments(const obhip_model &m, obhip_terms &t, const double *d_nodes, uint64_t n, uint64_t ldx,
                            const double *d_w, uint64_t ldw, double *d_dmean, double *d_cross, double *d_dd,
                            int *flag_out);
// d_out: q x (d + d (d + 1) / 2) row-major; d_excl (p x d), d_u (p) and d_part (pair_part_doubles at kActiveT,
// kActiveRC): scratch
int launch_active(const uint8_t *d_lev, const int *d_meta, uint64_t p, uint64_t d, uint64_t q, uint64_t n_cov,
                  const double *d_Theta, const double *d_mtab, const double *d_ctab, const double *d_dmtab,
                  const double *d_xtab, const double *d_ddtab, double *d_excl, double *d_u, double *d_part,
                  double *d_out);
// ---- runtime value -> template argument -----------------------------------------------------------
// pick_or<1, 2, 4, 8>(ng, miss, [&](auto NG) { ... NG() ... }): the lambda is called with the
// std::integral_constant of the listed value that v equals and its result returned; `miss` when v
// equals none.  Inside the lambda `if constexpr` on NG() keeps a combination that must not exist
// from being instantiated (no_kernel() is what such an arm returns).
template <int... Vs, typename F>
int pick_or(int v, int miss, F &&f) {
  int rc = miss;
  (void)((v == Vs ? (rc = f(std::integral_constant<int, Vs>{}), true) : false) || ...);
  return rc;
}
// the same, the LAST listed value standing in for every v that equals none (a switch's `default:`)
template <int... Vs, typename F>
int pick(int v, F &&f) {
  constexpr int vs[] = {Vs...};
  return pick_or<Vs...>(((v == Vs) || ...) ? v : vs[sizeof...(Vs) - 1], 0, f);
}
template <typename F>
int pick_bool(bool v, F &&f) {
  return v ? f(std::true_type{}) : f(std::false_type{});
}
inline int no_kernel() { return fail(OBHIP_ERR_STATE, "dispatch: no kernel for this combination"); }

// ---- what the product kernels share on the host ---------------------------------------------------
// (kernels_prod, _hm, _grad, _grad_d3: the kernels that stage a tile of the used columns of b in LDS)
// Their leading parameters, in their order.
struct ProdTabs {
  const double *bm, *scale;
  const uint32_t *ucol;
  int Mu;
  uint64_t Mc;
  const uint32_t *cols;
};
inline ProdTabs prod_tabs(const obhip_basis &b, const obhip_terms &t) {
  return {b.bm.p, b.scale.p, t.ucol.p, (int)t.Mu, b.md.Mc, (const uint32_t *)t.cols.p};
}
// kernel<<<grid, block, lds, current stream>>>(the tables as separate arguments, rest...), its dynamic
// LDS granted first (ensure_dyn_lds: nothing to do up to 64 KB) and the launch checked
template <typename Kernel, typename... Rest>
int launch_prod(Kernel kernel, dim3 grid, dim3 block, size_t lds, const ProdTabs &T, Rest... rest) {
  OB_TRY(ensure_dyn_lds((const void *)kernel, lds));
  hipLaunchKernelGGL(kernel, grid, block, lds, cur_stream(), T.bm, T.scale, T.ucol, T.Mu, T.Mc, T.cols, rest...);
  OB_HIP(hipGetLastError());
  return 0;
}

// ---- what the fused predictors share on the host -------------------------------------------------
// (kernels_predict, _star, _multi, _predict_dx, _materialize_dx, _predict_jac, _predict_hvp)
int ensure_dx_tables(const obhip_model &m, obhip_terms &t);  // predict_dx.cpp; after t.prepare(t.pred_md.cap, ...)
// Before any of their launches: the device view of the model capped at the terms' levels (rebuilt when
// the model or its state changed), the term tables packed against its column layout and, with_dx, the
// per-dimension views and derivative tables of the input-gradient kernels.
inline int prepare_predict(const obhip_model &m, obhip_terms &t, bool with_dx) {
  if (t.pred_model != &m || t.pred_md.model_version != m.version) {
    OB_TRY(t.pred_md.build(m, t.maxlev));
    t.pred_model = &m;
  }
  OB_TRY(t.prepare(t.pred_md.cap, t.pred_md.dims_h));
  if (with_dx) OB_TRY(ensure_dx_tables(m, t));
  return 0;
}
// The tables their kernels evaluate the basis from: the kernels' leading parameters, in their order
// (dtab: behind tab in the kernels that take it; null before ensure_dx_tables).
struct PredTabs {
  const DimDesc *dims;
  const double *ka, *kb, *kc, *rot, *tab, *dtab;
  const int *cpos;
  int d, Mu;
};
inline PredTabs pred_tabs(const obhip_model &m, const obhip_terms &t) {
  const ModelDev &md = t.pred_md;
  return {md.dims.p, md.ka.p, md.kb.p, md.kc.p, md.rot.p, md.tab.p, t.dx.dtab.p, t.cpos.p, (int)m.d, (int)t.Mu};
}
// kernel<<<grid, block, lds, current stream>>>(the tables as separate arguments, rest...); DX: with dtab
template <bool DX, typename Kernel, typename... Rest>
void launch_pred(Kernel kernel, dim3 grid, dim3 block, size_t lds, const PredTabs &T, Rest... rest) {
  if constexpr (DX)
    hipLaunchKernelGGL(kernel, grid, block, lds, cur_stream(), T.dims, T.ka, T.kb, T.kc, T.rot, T.tab, T.dtab, T.cpos,
                       T.d, T.Mu, rest...);
  else
    hipLaunchKernelGGL(kernel, grid, block, lds, cur_stream(), T.dims, T.ka, T.kb, T.kc, T.rot, T.tab, T.cpos, T.d,
                       T.Mu, rest...);
}
// blocks of a fallback kernel that keeps its tile of ncols columns in a per-block slice of pooled HBM
// scratch: at most `want`, at least 1, within 1 GB of scratch in all
inline uint64_t hbm_tile_blocks(uint64_t want, uint64_t ncols) {
  const uint64_t per = ncols * kTileRows * sizeof(double);
  return std::max<uint64_t>(1, std::min<uint64_t>(want, (1ull << 30) / per));
}
// kernels_predict.hip
int launch_predict(const obhip_model &m, obhip_terms &t, const double *d_theta,
                   const double *d_x, uint64_t n, double *d_mean,
                   const double *d_coeffvar, double e2sigma, double *d_var);
// kernels_predict_dx.hip / predict_dx.cpp: mean, variance and their gradients by the inputs
bool predict_dx_supports(const obhip_terms &t);
void build_dim_views_host(obhip_terms &t);               // t.dx.voff / vterm (no device needed)
int launch_predict_dx(const obhip_model &m, obhip_terms &t, const double *d_theta, const double *d_x, uint64_t n,
                      double *d_mean, double *d_grad, const double *d_coeffvar, double e2sigma, double *d_var,
                      double *d_gradvar);
// kernels_predict_jac.hip / predict_jac.cpp: Jacobian (d_W == nullptr, into d_jac) or vector-Jacobian
// product (with d_W, into d_out) of the multi-response predictor; q = 1 goes to launch_predict_dx
bool predict_jac_supports(const obhip_terms &t);
int launch_predict_jac(const obhip_model &m, obhip_terms &t, const double *d_Theta, uint64_t q, const double *d_x,
                       uint64_t n, double *d_mean, double *d_jac, const double *d_W, uint64_t ldw, double *d_out);
// kernels_predict_hvp.hip / predict_hvp.cpp: Hessian-vector and Jacobian-vector product of the
// multi-response predictor (any q >= 1); the fused kernel's domain and its LDS for NQB blocks of 16 responses
constexpr int kHvpRows = 32;  // rows of a tile
size_t predict_hvp_lds(uint64_t Mu, uint64_t d, int nqb, bool hbm);
bool predict_hvp_supports(const obhip_terms &t);
int ensure_d2_tables(const obhip_model &m, obhip_terms &t);  // after ensure_dx_stage
int launch_predict_hvp(const obhip_model &m, obhip_terms &t, const double *d_Theta, uint64_t q, const double *d_x,
                       uint64_t n, const double *d_W, uint64_t ldw, const double *d_V, double *d_mean, double *d_vjp,
                       double *d_jvp, double *d_hvp);
// kernels_materialize_dx.hip / grad_obs.cpp: the derivative design matrix as rows of the normal equations
struct DxStage {
  const double *x = nullptr;        // device, column-major with leading dimension ldx, n rows from x on
  uint64_t ldx = 0, n = 0;
  const uint32_t *dims = nullptr;   // device: the L differentiated dimensions
  const double *sqw = nullptr;      // device: sqrt(w_j)
  uint64_t L = 0;
  double *out = nullptr;            // out[(j * blk_rows + i) * pitch + k] = sqrt(w_j) dB[i,k] / dx_{dims[j]}
  uint64_t pitch = 0, blk_rows = 0;
  uint64_t pcols = 0;               // columns written per row: p .. pcols as zeros
  bool pad_rows = false;            // rows n .. next multiple of 64 written as zeros
  const double *g = nullptr;        // with ypart: g[j * ldg + i], one response's observed gradients (raw)
  uint64_t ldg = 0;
  double *ypart = nullptr;          // [ceil(n / 64)][pitch] partial (staged)^T sqrt(w) g per tile
};
// dims distinct and < d, 1 <= ndims <= d, weights (may be null) finite and > 0 -- refused in that order
int check_grad_dims(const char *who, uint64_t d, const uint32_t *dims, uint64_t ndims, const double *weights);
int ensure_dx_stage(const obhip_model &m, obhip_terms &t);  // prepare_predict + the staging kernel's own table
bool materialize_dx_supports(const obhip_terms &t);
int launch_materialize_dx(const obhip_model &m, obhip_terms &t, const DxStage &s);
uint64_t dx_aty_splits(uint64_t rows);
int launch_dx_aty(const double *d_B, uint64_t pitch, uint64_t blk_rows, uint64_t L, uint64_t n, const double *d_sqw,
                  const double *d_g, uint64_t ldg, double *d_part, uint64_t p, bool accumulate, double *d_out);
int launch_dx_colsum(const double *d_part, uint64_t nsplit, uint64_t pitch, uint64_t p, bool accumulate, double *d_out);
// sum_j w_j D_j^T D_j of the batch d_x (n x d, ld = n) into the packed triangle d_tri and, per response r,
// sum_j w_j D_j^T g_rj into d_R + r * p; holder: a basis that lends gram_of_staged its device, workspace
// and task-table cache (never its bmat)
int grad_batch_normal_eq(obhip_basis &holder, const obhip_model &m, obhip_terms &t, const double *d_x, uint64_t n,
                         const uint32_t *dims, const double *weights, uint64_t L, const double *d_dY, uint64_t lddy,
                         uint64_t q, double *d_tri, double *d_R);
// kernels_acc.hip: the streaming fit's batch moments, folds and right-hand sides (normal_acc.cpp)
// dst +/- src over the triangle and R only (a batch of gradient rows has no B^T 1 and no moments)
int launch_acc_fold_grad(uint64_t p, uint64_t q, double *d_dst, const double *d_src, double sign);
int launch_acc_batch_moments(const double *d_Y, uint64_t ldy, uint64_t n, uint64_t q, bool empty,
                             const double *d_mom_state, double *d_mom_batch, double *d_Ys, double *d_part);
int launch_acc_fold(uint64_t p, uint64_t q, double *d_dst, const double *d_src, bool dst_empty, double sign);
// launch_acc_fold behind the triangle: d_dst_tail / d_src_tail = [R | b1 | moments] of the two states
int launch_acc_fold_tail(uint64_t p, uint64_t q, double *d_dst_tail, const double *d_src_tail, bool dst_empty,
                         double sign);
int launch_acc_rhs(uint64_t p, uint64_t q, const double *d_state, const double *d_minus, double e2, double *d_rhs,
                   double *d_meansd);
int launch_cv_score(const double *d_mean, const double *d_Y, uint64_t n, uint64_t q, uint64_t ld,
                    const double *d_meansd, double *d_out, double *d_part);
// small vector kernels (kernels_misc.hip)
int launch_colnorm2(const double *d_Z, uint64_t ld, uint64_t p, uint64_t n, double add, double *d_out);
int launch_dot_cols(const double *d_A, const double *d_B, uint64_t ld, uint64_t p, uint64_t n, double *d_out,
                    double *d_part);
int quantile_max_targets();
int launch_count_le(const double *d_x, uint64_t n, uint64_t d, const uint64_t *d_mids, int T,
                    unsigned long long *d_counts);
int launch_u64_to_f64(const unsigned long long *d_in, uint64_t n, double *d_out);
int launch_synth(uint64_t seed, uint64_t row0, uint64_t n, uint64_t d,
                 const int *d_kinds, double *d_x, double *d_y);
int launch_sum_sumsq(const double *d_v, uint64_t n, double *d_out2,
                     double *d_part /* 2048 doubles of scratch */);
int launch_affine(double *d_v, uint64_t n, double cent, double sca);
int launch_resid(const double *d_yhat, const double *d_y, uint64_t n, double e2,
                 double *d_r, double *d_diff);
int launch_scale(double *d_v, uint64_t n, double c);
int launch_fill(double *d_v, uint64_t n, double c);
// kernels_comm.hip: the one-buffer exchange of the normal equations, and the packed upper triangle
// (row-major, row i from its diagonal on) in which a sharded fit exchanges G and a streaming fit keeps it
__host__ __device__ inline uint64_t tri_off(uint64_t i, uint64_t p) {
  return i * p - i * (i - 1) / 2;  // start of row i (entries j >= i)
}
uint64_t normal_eq_tail(uint64_t p);
int launch_pack_normal_eq(uint64_t p, bool with_tri, const double *d_G, const double *d_g, const double *d_b1,
                          const double *d_sum2, double nlocal, double *d_buf, uint64_t count);
int launch_unpack_normal_eq(uint64_t p, bool with_tri, const double *d_buf, double *d_G, double *d_g,
                            double *d_meansd);
// d_H (full symmetric p x p) = the packed triangle d_tri minus d_tri_minus (may be null); with `form`
// the Hessian e2 (T - T_minus) + diag(prec) and its diagonal (d_diagH may be null)
int launch_unpack_tri(uint64_t p, const double *d_tri, const double *d_tri_minus, double *d_H, bool form,
                      double e2 = 1.0, const double *d_prec = nullptr, double *d_diagH = nullptr);
// api.cpp: logpr_gauss::diaghess of the terms; model and terms belong together
std::vector<double> prior_prec(const obhip_model &m, const obhip_terms &t, double rho);
int check_compat(const obhip_model *m, const obhip_terms *t);
// fit_newton.cpp: the pieces of the one Newton-fit pipeline that the streaming fit uses as well.
// *d_prec = the prior precisions of t on the device, uploaded when the model state or rho changed
int terms_prec_dev(const obhip_model *m, obhip_terms &t, double rho, const double **d_prec);
// d_out (p x ncols, ld = p) = B^T Y for the columns that do not ride along with the Gram
int bty_columns(obhip_basis &b, obhip_terms &t, const double *d_Y, uint64_t ldy, uint64_t ncols, double *d_out);
// d_Theta (p x ncols) = inv(H) e2 R on the factor launch_newton_solve has just left in d_H
int solve_columns(uint64_t p, const double *d_H, const void *d_cholws, const double *d_R, uint64_t ncols, double e2,
                  double *d_Theta, void *d_scratch);
// comm.cpp: in-place sum over the ranks of c (no-op for c == nullptr or one rank)
int comm_allreduce(obhip_comm *c, double *d_buf, uint64_t count);
int comm_nranks(const obhip_comm *c);
// obhip_fit_cg_dev with the non-finite exit of fit.cpp:53-56 reported (finite_out = 0, val = -inf)
int fit_cg_dev_impl(const obhip_basis *b, const obhip_terms *t, const obhip_model *m, const double *d_y,
                    double sigma, double rho, double tol, uint64_t maxit, double *d_theta,
                    uint64_t *iters_out, double *d_diagH, double *val_out, obhip_comm *comm,
                    int *finite_out,
                    double *d_sqcolsums_out = nullptr);

}  // namespace obhip
