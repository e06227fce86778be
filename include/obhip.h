/*
 * obhip.h -- C ABI of the MI355X-native outerbase hot path.
 *
 * This is the drop-in boundary: every entry point below replaces one piece of
 * the reference's Rcpp-module surface (RCPP_MODULE(obmod),
 * src/interfaceR.cpp:661-793 of MattPlumlee/outerbase) or of the C++ objects
 * behind it.  The reference interface each function replaces is cited as
 * file:line relative to the reference checkout.  INTEGRATION.md shows the
 * Rcpp glue a maintainer would add on the reference side.
 *
 * Conventions
 *   - plain C, opaque handles, caller owns every host buffer, the library
 *     owns every device buffer behind a handle;
 *   - every function returns 0 on success, non-zero on failure; the message
 *     is in obhip_last_error() (thread-local).  Nothing throws across the ABI;
 *   - matrices that cross the ABI on the HOST side are column-major FP64,
 *     `terms` are column-major p x d unsigned 64-bit 0-based levels, exactly
 *     like the Armadillo mat / umat the reference marshals
 *     (SURVEY.md section 8b "Data marshalling");
 *   - functions with the suffix _dev take DEVICE pointers (HBM resident
 *     inputs/outputs) and enqueue on the stream set by obhip_set_stream();
 *     they do not synchronise.  Functions without the suffix take host
 *     pointers and return after the result is in the host buffer;
 *   - there is NO CPU fallback: without a visible gfx950 device every
 *     device-touching call fails with OBHIP_ERR_NO_DEVICE;
 *   - handles are NOT re-entrant: like the reference (one R main thread,
 *     SURVEY.md section 8b "Threading") a model / basis / terms / lpdf /
 *     communicator is used by one thread at a time.  Calls on a `const`
 *     handle may still fill caches behind it (device tables of the terms, the
 *     staged design matrix and task tables of a basis, the prior precisions);
 *     different handles may be used from different threads concurrently;
 *   - collective calls (anything taking an obhip_comm with more than one rank)
 *     must be made by every rank with the same sizes: an argument error on one
 *     rank returns on that rank while its peers wait in the collective.
 */
#ifndef OBHIP_H
#define OBHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OBHIP_OK 0
#define OBHIP_ERR_INVALID 1     /* bad argument (std::range_error / Armadillo
                                   size error in the reference) */
#define OBHIP_ERR_NO_DEVICE 2   /* no HIP device / kernels unavailable */
#define OBHIP_ERR_HIP 3         /* a HIP runtime call failed */
#define OBHIP_ERR_STATE 4       /* object not ready (e.g. knots not set) */
#define OBHIP_ERR_NUMERIC 5     /* non-finite / not positive definite */

/* covariance kinds: listcov() R/fitting.R:6-8, setcovfs
 * src/interfaceR.cpp:53-73 */
#define OBHIP_COV_MAT25 0
#define OBHIP_COV_MAT25POW 1
#define OBHIP_COV_MAT25ANG 2

typedef struct obhip_model obhip_model; /* class outermod, modandbase.h:9-54 */
typedef struct obhip_basis obhip_basis; /* class outerbase, modandbase.h:57-125 */
typedef struct obhip_terms obhip_terms; /* a umat `terms` resident on device */
typedef struct obhip_lpdf obhip_lpdf;   /* class lpdf and descendants, fit.h:23-361 */
typedef struct obhip_predictor obhip_predictor; /* class predictor, fit.h:352-361 */
typedef struct obhip_comm obhip_comm;   /* the ranks of a row-sharded job (no reference
                                           counterpart: the reference is one process,
                                           modandbase.cpp:464) */
typedef struct obhip_normal_acc obhip_normal_acc; /* the normal equations of the rows seen so far
                                                     (no reference counterpart: obfit takes all
                                                     rows at once, R/fitting.R:40-120) */
typedef struct obhip_posterior obhip_posterior;   /* the posterior covariance of the coefficients,
                                                     resident on the device (no reference
                                                     counterpart: predr_std inverts H per call,
                                                     loglik_std.cpp:227) */

/* ---- library ----------------------------------------------------------- */
/* 5.  (2 -> 3: obhip_standardise_dev, obhip_destandardise_dev, obhip_fit_newton_count,
 * obhip_fit_newton_sharded_dev, obhip_source_hash added; 3 -> 4: obhip_comm_selftest_dev,
 * obhip_comm_exchange_path, obhip_comm_init_sim added, obhip_standardise_dev accepts an empty
 * shard when it has a communicator; 4 -> 5: obhip_terms_share_tables added; nothing removed.) */
int obhip_abi_version(void);
const char *obhip_last_error(void);
/* 16 hex digits of the SHA-256 over the library's sources at build time: which = 0 all of
 * them, 1 the files the Gram kernel is built from.  Profiles record it, and bench.py prints
 * PMC counters only when they were collected from the kernel that is running. */
const char *obhip_source_hash(int which);
int obhip_device_count(int *count);
int obhip_set_device(int device);
/* hipStream_t to launch on (NULL = default stream). */
int obhip_set_stream(void *hip_stream);
int obhip_synchronize(void);
/* Device temporaries of the calls below are recycled through a size-keyed pool (at most
 * OBHIP_POOL_MB, default 8192, of cached memory); this hands the cached blocks back to the
 * driver. */
int obhip_trim_pool(void);
/* Per-kernel hipEvent timing (used by bench.py for the roofline line).  obhip_profile_get: the
 * launches and device time of one profiled scope ("gram", "cholesky", "hessmult", ...); "*" = all
 * scopes together; "host_syncs" = the number of times the library has blocked on the device
 * since it was loaded (launches; total_ms = 0): the host round trips of a call sequence are the
 * difference of two readings. */
int obhip_profile_enable(int on);
int obhip_profile_reset(void);
int obhip_profile_get(const char *kernel, uint64_t *launches, double *total_ms);

/* ---- covariance functions (classes covf_mat25 / covf_mat25pow /
 * covf_mat25ang, src/covfuncs.h:34-67; module rows interfaceR.cpp:764-791) */
int obhip_cov_numhyp(int kind, int *numhyp);
/* hyp0, hyplb, hypub, hypvar (numhyp each), lowbnd, uppbnd
 * (covfuncs.cpp:87-111,166-195,254-283) */
int obhip_cov_info(int kind, double *hyp0, double *hyplb, double *hypub,
                   double *hypvar, double *lowbnd, double *uppbnd);
/* covf::cov (covfuncs.cpp:113-126,197-212,285-310): out is n1 x n2
 * column-major.  Host arithmetic (knot-sized problems). */
int obhip_cov(int kind, const double *hyp, const double *x1, uint64_t n1,
              const double *x2, uint64_t n2, double *out);
/* covf::cov_gradhyp (covfuncs.cpp:134-150,220-243,318-347; module row interfaceR.cpp:775):
 * out is n1 x n2 x numhyp, column-major slices.  Host arithmetic. */
int obhip_cov_gradhyp(int kind, const double *hyp, const double *x1, uint64_t n1,
                      const double *x2, uint64_t n2, double *out);
/* covf::lpdf (covfuncs.cpp:35-50) */
int obhip_cov_hyplpdf(int kind, const double *hyp, double *out);

/* ---- outermod ---------------------------------------------------------- */
/* new(outermod) + setcovfs(om, covnames): interfaceR.cpp:53-73,
 * outermod::hyp_init modandbase.cpp:128-153 */
int obhip_model_create(obhip_model **out, uint64_t d, const int *kinds);
int obhip_model_destroy(obhip_model *m);
/* setknot(om, knotlist): interfaceR.cpp:94-149.  knotptst has d+1 entries
 * (modandbase.h:18), knotpt has knotptst[d]. Triggers outermod::build. */
int obhip_model_set_knots(obhip_model *m, const uint64_t *knotptst,
                          const double *knotpt);
/* the knots as set (fields knotptst / knotpt, modandbase.h:18-19); either pointer may be NULL */
int obhip_model_get_knots(const obhip_model *m, uint64_t *knotptst, double *knotpt);
/* om$updatehyp(hyp): outermod::hyp_set modandbase.cpp:161-202 */
int obhip_model_set_hyp(obhip_model *m, const double *hyp, uint64_t nhyp);
/* gethyp(om): interfaceR.cpp:167-180 */
int obhip_model_get_hyp(const obhip_model *m, double *hyp);
/* d, M = total knots, mmax = max knots per dim, nhyp */
int obhip_model_dims(const obhip_model *m, uint64_t *d, uint64_t *M,
                     uint64_t *mmax, uint64_t *nhyp);
/* results of outermod::build (modandbase.cpp:210-276): rotmat is
 * mmax x M column-major (modandbase.h:44), basisvar M (:12), maxlevel d
 * (:29). */
int obhip_model_get_rotation(const obhip_model *m, double *rotmat,
                             double *basisvar, int64_t *maxlevel);
/* Replace the eigen-decomposition results with caller-supplied ones (the
 * reference takes them from LAPACK via arma::eig_sym, modandbase.cpp:236;
 * parity tests inject the oracle's so that both sides share one rotation). */
int obhip_model_set_rotation(obhip_model *m, const double *rotmat,
                             const double *basisvar, const int64_t *maxlevel);
/* Hyper-parameter gradient layout (outermod::hyp_set, modandbase.cpp:183-197): nhyp
 * hyper-parameters in all; hyper-parameter h belongs to dimension hypmatch[h] and owns
 * the column block [gest[h], gest[h+1]) (m_l columns) of the *_gradhyp arrays.
 * hypmatch: nhyp entries, gest: nhyp + 1; any pointer may be NULL. */
int obhip_model_grad_layout(const obhip_model *m, uint64_t *nhyp, uint64_t *hypmatch,
                            uint64_t *gest);
/* gradient part of outermod::build (modandbase.cpp:257-274): rotmat_gradhyp is
 * mmax x gest[nhyp] column-major (modandbase.h:45), logbasisvar_gradhyp gest[nhyp] */
int obhip_model_get_rotation_grad(const obhip_model *m, double *rotmat_gradhyp,
                                  double *logbasisvar_gradhyp);
/* counterpart of obhip_model_set_rotation for the gradient arrays */
int obhip_model_set_rotation_grad(obhip_model *m, const double *rotmat_gradhyp,
                                  const double *logbasisvar_gradhyp);
/* om$getlvar_gradhyp(terms): modandbase.cpp:364-379; out p x nhyp column-major */
int obhip_model_term_lvar_gradhyp(const obhip_model *m, const uint64_t *terms, uint64_t p,
                                  double *out);
/* om$selectterms(numele): modandbase.cpp:387-440.  seed==0: the reference's
 * RNG shuffle (modandbase.cpp:408) is replaced by the identity permutation;
 * seed!=0: SplitMix64-driven pick among the near-best candidates.
 * terms_out: p x d column-major. */
int obhip_model_select_terms(const obhip_model *m, uint64_t p, uint64_t seed,
                             uint64_t *terms_out);
/* om$getvar(terms): modandbase.cpp:350-356 */
int obhip_model_term_var(const obhip_model *m, const uint64_t *terms,
                         uint64_t p, double *out);
/* om$hyplpdf(hyp): modandbase.cpp:89-99 */
int obhip_model_hyplpdf(const obhip_model *m, const double *hyp, uint64_t nhyp,
                        double *out);

/* om$hyplpdf_grad(hyp): modandbase.cpp:106-118 (covf::lpdf_gradhyp, covfuncs.cpp:53-70) */
int obhip_model_hyplpdf_grad(const obhip_model *m, const double *hyp, uint64_t nhyp,
                             double *out);

/* ---- terms ------------------------------------------------------------- */
/* Upload a umat `terms` (p x d, column-major, 0-based levels) once; the
 * reference passes it by value on every call (modandbase.cpp:649,677,700). */
int obhip_terms_create(obhip_terms **out, const obhip_model *m,
                       const uint64_t *terms, uint64_t p);
int obhip_terms_destroy(obhip_terms *t);
int obhip_terms_info(const obhip_terms *t, uint64_t *p, uint64_t *d,
                     uint64_t *nnz_total, uint64_t *max_nnz);
/* highest level used per dimension (d entries) */
int obhip_terms_maxlevels(const obhip_terms *t, int64_t *levels);
/* How the term-per-lane kernels share sub-products among these terms (host only, no device
 * needed).  The reference multiplies every term out on its own (prodmm_ / tprodmm_,
 * linalg.cpp:57-131,286-355); selectterms' output is downward-closed (modandbase.cpp:419-436), so
 * its terms come in families that differ in one factor, and the library groups the p_pad = p
 * rounded up to 256 terms (the padding terms have no factors) into *stars*: four terms whose P
 * shared factors are read and multiplied once (csrc/share.cpp).  Terms that find no family with
 * four free members are *left over* (any term set is accepted; one that is not downward-closed
 * just leaves more over): they are listed, and also packed four at a time into plain stars
 * (nothing shared) behind the family stars.  Stars come in star-waves of 64, filled up with empty
 * stars.  info (11 entries):
 *   [0] p_pad, [1] left-over terms, [2] column reads per row of the family star-waves (sum of
 *   P + 4), [3] of the scheme without sharing (4 terms per lane, terms by falling number of
 *   factors: rounds 1-4), [4] W, the column slots per term, [5] LDS cycles of all star-waves' reads
 *   with their bank conflicts (2 per read at best; column u of the [column][65] tile lies in bank
 *   pair u mod 32), [6] the same before the search over the stars' half-waves and term orders that
 *   minimises them, [7] family star-waves, [8] plain star-waves, [9] reads per row of the latter, [10] the LDS
 *   cycles of [5] once the library has also chosen which tile index (bank pair) every used column
 *   gets -- what it uploads; the tables returned here keep the level-based ids (11 entries).
 * With S = 64 ([7] + [8]) stars in all -- S <= p_pad / 4 + 128 -- the optional outputs are:
 * term (4 S entries): the four term indices of star 0, of star 1, ... (0xffffffff: none);
 * shape ([7] + [8] entries): per star-wave P | S << 8 (family star-waves first: S = 1);
 * factor (S * 4 W entries): per star its column slots in read order -- [P shared][own of term 0]
 * [own of term 1] ... -- as 1 + (levels of the dimensions before l) + (level - 1) for level >= 1
 * of dimension l (levels counted up to obhip_terms_maxlevels), 0 = unused;
 * left ([1] entries): the left-over terms. */
int obhip_terms_share_tables(const obhip_terms *t, uint64_t *info, uint32_t *term, uint32_t *shape,
                             uint16_t *factor, uint32_t *left);

/* ---- outerbase --------------------------------------------------------- */
/* new(outerbase, om, x): modandbase.cpp:459-480 + build :547-626.
 * x is n x d column-major with leading dimension ldx (host).  levelcap
 * (d entries, or NULL) bounds the levels evaluated per dimension; NULL = all
 * knots-1 levels as the reference does.  The basis is built on the current
 * device. */
int obhip_basis_create(obhip_basis **out, const obhip_model *m, const double *x,
                       uint64_t n, uint64_t ldx, const int64_t *levelcap);
/* same with x already in HBM (column-major, ld = n) */
int obhip_basis_create_dev(obhip_basis **out, const obhip_model *m,
                           const double *d_x, uint64_t n,
                           const int64_t *levelcap);
/* ob$build(): rebuild after the model's hyp/knots changed
 * (modandbase.cpp:547; vignettes/learning.Rmd:48-54) */
int obhip_basis_rebuild(obhip_basis *b);
int obhip_basis_destroy(obhip_basis *b);
int obhip_basis_dims(const obhip_basis *b, uint64_t *n, uint64_t *d,
                     uint64_t *ncols_stored);
/* ob$getbase(k), k 1-based: modandbase.cpp:634-639; out n x m_k col-major */
int obhip_basis_getbase(const obhip_basis *b, uint64_t k, double *out);
/* ob$getmat(terms): getm_ linalg.cpp:647-715; out n x p col-major */
int obhip_basis_getmat(const obhip_basis *b, const obhip_terms *t, double *out);
/* ob$matmul(terms, a) / outerbase::mm: prodmm_ linalg.cpp:57-131 (vector)
 * and :481-557 (matrix, ncol > 1; a is p x ncol, out n x ncol) */
int obhip_basis_mm(const obhip_basis *b, const obhip_terms *t, const double *a,
                   uint64_t ncol, double *out);
/* ob$tmatmul(terms, a) / outerbase::tmm: tprodmm_ linalg.cpp:286-355 and
 * :567-637 (a is n x ncol, out p x ncol) */
int obhip_basis_tmm(const obhip_basis *b, const obhip_terms *t, const double *a,
                    uint64_t ncol, double *out);
/* outerbase::sqmm modandbase.cpp:784-790, sqtmm/sqtmmm :816-837,
 * sqcolsums :863-867, residvar :889-895 */
int obhip_basis_sqmm(const obhip_basis *b, const obhip_terms *t,
                     const double *a, uint64_t ncol, double *out);
int obhip_basis_sqtmm(const obhip_basis *b, const obhip_terms *t,
                      const double *a, uint64_t ncol, double *out);
int obhip_basis_sqcolsums(const obhip_basis *b, const obhip_terms *t,
                          double *out);
int obhip_basis_residvar(const obhip_basis *b, const obhip_terms *t,
                         const obhip_model *m, double *out);

/* device-pointer forms (single vector) used by the fit drivers, the
 * benchmark and the multi-GPU path */
int obhip_basis_mm_dev(const obhip_basis *b, const obhip_terms *t,
                       const double *d_a, double *d_out, int squared);
int obhip_basis_tmm_dev(const obhip_basis *b, const obhip_terms *t,
                        const double *d_a, double *d_out, int squared);

/* ---- hyper-parameter gradients ------------------------- */
/* The gradient basis (outerbase::build with dograd, modandbase.cpp:547-626) is built on
 * the first call and kept until the basis is rebuilt.  nhyp and the block layout come
 * from obhip_model_grad_layout.  The basis must have been built after the last change of
 * the model (OBHIP_ERR_STATE otherwise).
 * ob$getmat_gradhyp(terms): modandbase.cpp:663-669 (getmge_, linalg.cpp:778-822);
 * out: n x p x nhyp, column-major slices. */
int obhip_basis_getmat_gradhyp(const obhip_basis *b, const obhip_terms *t, double *out);
/* ob$matmul_gradhyp(terms, a): modandbase.cpp:725-744 (prodmmge_, linalg.cpp:219-276);
 * out (n, may be NULL) = B a, out_gradhyp n x nhyp column-major. */
int obhip_basis_mm_gradhyp(const obhip_basis *b, const obhip_terms *t, const double *a,
                           double *out, double *out_gradhyp);
/* w^T d(B a)/dhyp (nhyp values) with the n x nhyp matrix left on the device: the form the
 * likelihoods use matmul_gradhyp in (src/lpdfs/loglik_gauss.cpp:127, loglik_std.cpp:143).
 * out (n, B a) may be NULL. */
int obhip_basis_mm_gradhyp_dot(const obhip_basis *b, const obhip_terms *t, const double *a,
                               const double *w, double *out, double *out_dot);
/* ob$tmatmul_gradhyp(terms, a): modandbase.cpp:755-776 (tprodmmge_, linalg.cpp:395-471);
 * out (p, may be NULL) = B^T a, out_gradhyp p x nhyp column-major. */
int obhip_basis_tmm_gradhyp(const obhip_basis *b, const obhip_terms *t, const double *a,
                            double *out, double *out_gradhyp);

/* ob$sqmm_gradhyp(terms, a) / ob$sqtmm_gradhyp(terms, a): the same on the squared stores
 * basematsq / basescalesq / basematsq_gradhyp (modandbase.cpp:798-809, 845-856);
 * out_gradhyp n x nhyp resp. p x nhyp, column-major */
int obhip_basis_sqmm_gradhyp(const obhip_basis *b, const obhip_terms *t, const double *a,
                             double *out_gradhyp);
int obhip_basis_sqtmm_gradhyp(const obhip_basis *b, const obhip_terms *t, const double *a,
                              double *out_gradhyp);
/* ob$sqcolsums_gradhyp(terms): modandbase.cpp:875-879; p x nhyp */
int obhip_basis_sqcolsums_gradhyp(const obhip_basis *b, const obhip_terms *t, double *out_gradhyp);
/* ob$residvar_gradhyp(terms): modandbase.cpp:904-925; n x nhyp */
int obhip_basis_residvar_gradhyp(const obhip_basis *b, const obhip_terms *t, const obhip_model *m,
                                 double *out_gradhyp);
/* What the hyper-gradient products above will launch for (b, t), read from the functions the launchers
 * take their geometry from; the gradient basis and the terms' device tables are prepared as the
 * products prepare them, nothing else runs (OBHIP_GRAD_D3 and OBHIP_GRAM_CHUNK_ROWS are read as there).
 * info (16 entries):
 *   [0] plan of the transposed products: 0 fused (dense pass + k_tmm_d3), 1 dense pass + restricted
 *       views, 2 k_bt_times_u on the materialised design matrix + restricted views, 3 full views;
 *   [1] k_tmm_d3 groups (0: the terms do not fit it, or it is switched off; matmul_gradhyp_dot takes
 *       them under any plan), [10] their members in all;
 *   the dense pass: [2] kernel (0 none, 1 k_tmm_ge0_db, 2 k_tmm_ge0 with 16 waves, 3 with 8 waves,
 *       4 k_bt_times_u), [6] blocks along the terms, [7] row splits, [8] row tiles per split, [9] passes;
 *   the terms' own tables: [3] W / 2 (column slots per term / 2), [4] used columns Mu, [5] p_pad;
 *   [11] groups of restricted views (plans 1 and 2), [12] of them those too wide for one pass, which
 *       go hyper-parameter by hyper-parameter;
 *   [13] hyper-parameters, [14] row tiles of the basis, [15] compute units of its device.
 * Optional outputs, sized from a first call without them:
 * groups (10 x [1]): per k_tmm_d3 group nh (delta columns per view-term), W, Mu, view-terms p, p_pad,
 *   NU (view-terms per lane: 2 or 4), blocks along the view-terms, row splits, row tiles per split,
 *   members;
 * members ([10] entries): the first hyper-parameter of every member, group after group;
 * passes (4 x [9]): per dense pass h0, nh, NHB (1: a 16-block), N4 (groups of four). */
int obhip_grad_plan_info(const obhip_basis *b, const obhip_terms *t, uint64_t *info, uint64_t *groups,
                         uint64_t *members, int64_t *passes);

/* ---- Gram / Newton ("back end A") -------------------------------------- */
/* G = B^T B (loglik_std::hess without its e^{-2 sigma}, loglik_std.cpp:
 * 170-173) and g = B^T y (loglik_std::update at coeff = 0, :100-120).
 * d_G: p x p (symmetric, full storage), d_g: p, both DEVICE buffers owned by
 * the caller so that a multi-GPU caller can all-reduce them.  d_y may be
 * NULL (then d_g is untouched). */
int obhip_gram_dev(const obhip_basis *b, const obhip_terms *t,
                   const double *d_y, double *d_G, double *d_g);
/* Which kernel forms G: 0 / 4 = FP64 matrix cores (v_mfma_f64_4x4x4_4b_f64) fed from a
 * row-major design matrix staged in HBM -- all n_pad x p_pad doubles at once (kept with the
 * basis) when that fits in half of the free memory, in row chunks otherwise; 3 = the same
 * matrix-core tiles with the operand panels generated inside the kernel (no staging memory;
 * terms of at most 8 factors on at most 128 used basis columns).  Both give the same G up to
 * summation order; DESIGN.md has the measurements. */
int obhip_set_gram_backend(int backend);
/* Entries of G repeat: G[s][t] depends on the per-dimension unordered level pairs {s_k, t_k} only.
 * The staged back end gives no task to a 128 x 128 tile pair all of whose entries occur in tile
 * pairs nearer the diagonal, and copies them from there after the reduction.  The term set is
 * analysed once, on the device, at its first Gram or at the first of these calls (which need a
 * device).  tile_pairs: pairs of the upper triangle; skipped: those without a task (0 with
 * OBHIP_GRAM_DEDUP=0 and where no analysis runs: fewer than three tiles, i.e. p <= 256, or more than
 * 48 Mi / 16384 = 3072 tile pairs); analysis_ms: host wall time the analysis took.  Any out pointer may be NULL. */
int obhip_gram_dedup_info(const obhip_terms *t, uint64_t *tile_pairs, uint64_t *skipped, double *analysis_ms);
/* d_src (device, p x p row-major int64): for an entry of a skipped tile pair the linear index
 * s' * p + t' of the entry it is copied from (s' <= t', in a tile pair that is computed), -1
 * everywhere else. */
int obhip_gram_dedup_table_dev(const obhip_terms *t, int64_t *d_src);
/* The same one level finer: a wave of the Gram kernel computes a 64 x 64 wave tile, and a wave tile outside
 * the diagonal tile pairs all of whose entries occur in wave tiles nearer the diagonal is dropped; the kept ones
 * are packed into blocks anew (the diagonal tiles' wave tiles fill the gaps).  A launch takes that plan when it
 * saves a block per row split and, by the launch's cost model, more time than its one-off analysis takes;
 * OBHIP_GRAM_DEDUP_QUADS=1 forces it wherever a wave tile can be dropped, =0 forbids it.  wave_tiles: those of
 * the upper triangle; dropped, blocks_per_split: of the analysis (both 0 while none has run: it runs at the first
 * launch long enough to pay for it, or here when forced); engaged: the term set's latest Gram launch ran the plan
 * (forced: the next one will).  While engaged, obhip_gram_dedup_table_dev reports the dropped wave tiles' sources
 * (in kept wave tiles) instead.  Any out pointer may be NULL. */
int obhip_gram_dedup_quads_info(const obhip_terms *t, uint64_t *wave_tiles, uint64_t *dropped, uint64_t *blocks_per_split,
                                int *engaged);
/* The panel Gram may stage and multiply its columns in an order of its own -- the terms in a stable sort by their
 * number of factors -- under which more wave tiles consist of repeats alone; which of them go is then decided by a
 * sequential pass from the farthest wave tile inwards.  Nothing a caller sees changes order: G, B^T y, the prior
 * diagonal and every report are in the caller's term coordinates.  A launch takes the order when its packed plan
 * saves a block per row split against the plan the launch would otherwise run and four launches save more modelled
 * time than the one-off set-up takes; OBHIP_GRAM_ORDER=1 forces it, =0 forbids it.  engaged: the term set's latest
 * Gram launch ran in Gram order (forced: the next one will); dropped, blocks_per_split: of its plan (0 while not
 * engaged); setup_ms: host wall time of the set-up, 0 while none has run.  While engaged,
 * obhip_gram_dedup_quads_info and obhip_gram_dedup_table_dev report this plan, in term coordinates.  Any out
 * pointer may be NULL. */
int obhip_gram_order_info(const obhip_terms *t, int *engaged, uint64_t *dropped, uint64_t *blocks_per_split,
                          double *setup_ms);
/* bytes of device workspace obhip_newton_solve_dev needs for p terms */
int obhip_newton_workspace_bytes(uint64_t p, uint64_t *bytes);
/* One Newton step from coeff = 0 of lpdfvec(loglik_std, logpr_gauss)
 * (lpdf::optnewton fit.cpp:98-131): H = e^{-2 sigma} G + diag(1/(sd e^rho)^2)
 * (loglik_std.cpp:170-173, logpr_gauss.cpp:153-158, fit.cpp:503-512),
 * theta = solve(H, e^{-2 sigma} g) by Cholesky + two triangular solves.
 * d_G is overwritten by the Cholesky factor (lower triangle, row-major).
 * d_theta: p (device).  d_diagH (p, may be NULL) receives diag(H)
 * (lpdfvec::diaghess_, fit.cpp:557-566). */
int obhip_newton_solve_dev(const obhip_model *m, const obhip_terms *t,
                           double *d_G, const double *d_g, double sigma,
                           double rho, double *d_theta, double *d_diagH,
                           void *d_workspace, uint64_t workspace_bytes);
/* host-buffer convenience: the whole back end A on one device.
 * theta (p), diagH (p, may be NULL), H_out (p x p col-major, may be NULL). */
int obhip_fit_newton(const obhip_basis *b, const obhip_terms *t,
                     const obhip_model *m, const double *y, double sigma,
                     double rho, double *theta, double *diagH, double *H_out);

/* ---- matrix-free PCG ("back end B", what obfit runs) -------------------- */
/* lpdf::optcg (fit.cpp:37-96) on lpdfvec(logpr_gauss, loglik_gauss)
 * (loglik_gauss.cpp:110-157), domargadj = false.  theta is in/out (host, p);
 * iters_out receives the iteration count; diagH (p, may be NULL) the
 * preconditioner (lpdfvec::diaghess_); val_out (may be NULL) the value of the
 * objective at the result -- asking for it costs one more evaluation (two passes
 * over the basis) when the last iteration advanced it by the recurrence. */
int obhip_fit_cg(const obhip_basis *b, const obhip_terms *t,
                 const obhip_model *m, const double *y, double sigma,
                 double rho, double tol, uint64_t maxit, double *theta,
                 uint64_t *iters_out, double *diagH, double *val_out);
/* same with y / theta / diagH in HBM.  comm (may be NULL = one rank): the rows are sharded
 * over comm's ranks and every B^T a pass sums one p-vector (+ 2 scalars) over them
 * (SURVEY.md section 8e); all ranks return the same theta. */
int obhip_fit_cg_dev(const obhip_basis *b, const obhip_terms *t,
                     const obhip_model *m, const double *d_y, double sigma,
                     double rho, double tol, uint64_t maxit, double *d_theta,
                     uint64_t *iters_out, double *d_diagH, double *val_out,
                     obhip_comm *comm);

/* ---- multi-GPU: rows sharded over ranks, one process per GPU ------------
 * No reference counterpart (one process, OpenMP threads: modandbase.cpp:464,480); this is
 * the partitioning BASELINE.json's north_star prescribes.  Every rank holds a contiguous row
 * block of x / y and its own outerbase; outermod and terms are replicated.  Back end A
 * exchanges ONE buffer per fit, back end B one p-vector per B^T a pass; prediction needs no
 * communication. */
#define OBHIP_UNIQUE_ID_BYTES 128
#define OBHIP_TRANSPORT_NONE 0
#define OBHIP_TRANSPORT_RCCL 1 /* ncclReduceScatter + ncclAllGather over xGMI */
#define OBHIP_TRANSPORT_HOST 2 /* caller-supplied sum of a host buffer (MPI, gloo) */
#define OBHIP_TRANSPORT_SIM 3  /* N virtual ranks holding this rank's shard: sum = N x, on the device */
/* what sums a buffer of a given size (obhip_comm_exchange_path) */
#define OBHIP_EXCHANGE_NONE 0
#define OBHIP_EXCHANGE_PAIR 1      /* ncclReduceScatter + ncclAllGather, in place */
#define OBHIP_EXCHANGE_ALLREDUCE 2 /* ncclAllReduce */
#define OBHIP_EXCHANGE_HOST 3
#define OBHIP_EXCHANGE_SIM 4
/* rank 0 draws the communicator id (ncclGetUniqueId); the launcher hands the 128 bytes to
 * every rank */
int obhip_comm_unique_id(void *id);
/* RCCL communicator over the current device of each of the nranks processes
 * (ncclCommInitRank; collective: every rank must call it).  librccl is loaded at run time. */
int obhip_comm_init(obhip_comm **out, int nranks, int rank, const void *id);
/* the same ranks with a caller-supplied transport: fn(user, host_buf, count) sums count
 * doubles in place over all ranks (MPI_Allreduce under R, gloo in the one-GPU rehearsals);
 * the library stages device buffers through pinned memory */
typedef int (*obhip_host_allreduce_fn)(void *user, double *host_buf, uint64_t count);
int obhip_comm_init_host(obhip_comm **out, int nranks, int rank, obhip_host_allreduce_fn fn,
                         void *user);
int obhip_comm_destroy(obhip_comm *c);
/* rccl_ranks: what ncclCommCount reports (0 for the host transport); rccl_version:
 * ncclGetVersion; any pointer may be NULL */
int obhip_comm_info(const obhip_comm *c, int *nranks, int *rank, int *transport, int *rccl_ranks,
                    int *rccl_version);
/* in-place sum of count doubles in HBM over the ranks, on the library's stream */
int obhip_comm_allreduce_dev(obhip_comm *c, double *d_buf, uint64_t count);
/* A communicator of nranks VIRTUAL ranks that all hold this process's shard: every sum is one
 * device pass buf *= nranks, nothing leaves the GPU.  For timing, on one GPU, the step one rank
 * of an nranks-GPU job runs (exchange-buffer layout, unpack, replicated solve); the result is
 * the fit of the shard's rows repeated nranks times. */
int obhip_comm_init_sim(obhip_comm **out, int nranks);
/* path: OBHIP_EXCHANGE_* a buffer of count doubles takes on this communicator (large buffers
 * in equal 16-byte blocks per rank: the reduce-scatter / all-gather pair, unless
 * OBHIP_RCCL_ALLREDUCE=1 was set on any rank when the communicator was made -- the flags are
 * summed over the ranks at init -- or the self-test switched it off); selftest: 0 not run,
 * 1 passed, 2 passed after switching the pair off.  Either pointer may be NULL. */
int obhip_comm_exchange_path(const obhip_comm *c, uint64_t count, int *path, int *selftest);
/* Collective self-test of the exchange on a buffer of count doubles (pass the size of the real
 * exchange, obhip_fit_newton_count): rank r fills (r + 1) w_i with small integers w_i, the sums
 * over the ranks are compared ON THE DEVICE with the closed form nranks (nranks + 1) / 2 w_i,
 * once through the reduce-scatter / all-gather pair (if a buffer of this size takes it) and
 * once through the plain all-reduce; the mismatch counts are summed over the ranks so that all
 * take the same decision.  Pair wrong, all-reduce right: the communicator switches to the
 * all-reduce for every size, in this process, and the call succeeds.  All-reduce wrong:
 * OBHIP_ERR_STATE.  result (4 values, may be NULL): OBHIP_EXCHANGE_* in use afterwards for this
 * size, mismatching elements of the pair (-1: not tried), of the all-reduce, 1 if the pair was
 * switched off by this call. */
int obhip_comm_selftest_dev(obhip_comm *c, uint64_t count, int64_t *result);
/* The one exchange of back end A.  Buffer layout (count doubles, obhip_normal_eq_count):
 * [upper triangle of G_r = B_r^T B_r, row-major packed, p (p + 1) / 2][B_r^T y_r : p]
 * [B_r^T 1 : p][sum y_r, sum y_r^2, n_r][zero padding to 2 nranks].  Pack -> sum over ranks ->
 * unpack: d_G becomes the global Gram (full symmetric storage), d_g the right-hand side of
 * the problem with y standardised over ALL rows like obfit does (R/fitting.R:55-57):
 * B^T ((y - cent) / sca) = (B^T y - cent B^T 1) / sca; d_meansd receives cent, sca, n
 * (device, 3 doubles).  comm may be NULL (one rank: only the standardisation happens and the
 * triangle part of the buffer is never touched, so d_buf may point count - tail doubles
 * before a tail-sized allocation). */
/* Exact sample quantiles (R's quantile(), type 7) of every column of a row-sharded x: what
 * obfit's knot placement needs of the data (.genknotlist, R/fitting.R:177-185).  d_x: this
 * rank's n x d rows, column-major (device); probs: q values in [0, 1] (host); out: d x q,
 * out[l * q + j] (host), identical on every rank.  comm may be NULL (one rank). */
int obhip_quantiles_dev(obhip_comm *comm, const double *d_x, uint64_t n, uint64_t d,
                        const double *probs, uint64_t q, double *out);
int obhip_normal_eq_count(uint64_t p, int nranks, uint64_t *count);
/* ---- row-sharded Newton fit, start to finish on the device (ABI 3) ----------------------
 * obfit's standardisation of y (R/fitting.R:55-57: (y - mean(y)) / sd(y), n - 1 denominator)
 * over the rows of ALL ranks, two-pass like R's sd(): (sum y, n) and sum (y - mean)^2 are
 * summed over the ranks (24 bytes in two exchanges), nothing returns to the host.
 * d_y_raw, d_y: n doubles (device; may be the same buffer); d_meansd: mean, sd, rows of all
 * ranks (device, 3 doubles).  comm may be NULL (one rank).  With a communicator n = 0 is a legal
 * shard (it still takes part in the two sums; d_y_raw / d_y may then be NULL); fewer than two
 * rows over all ranks give sd = NaN as R's sd() does. */
int obhip_standardise_dev(obhip_comm *comm, const double *d_y_raw, uint64_t n, double *d_y,
                          double *d_meansd);
/* obpred's de-standardisation (R/fitting.R:152): v = mean + sd v, in place, mean and sd read
 * from d_meansd on the device */
int obhip_destandardise_dev(double *d_v, uint64_t n, const double *d_meansd);
/* doubles of exchange buffer obhip_fit_newton_sharded_dev needs: the packed upper triangle of
 * G, then g = B^T y, padded to equal 16-byte blocks per rank */
int obhip_fit_newton_count(uint64_t p, int nranks, uint64_t *count);
/* lpdf::optnewton (fit.cpp:98-131) of lpdfvec(loglik_std, logpr_gauss) from coeff = 0 on a
 * row shard: G_r = B_r^T B_r by the Gram kernels, whose reduction writes the packed upper
 * triangle straight into d_exbuf, g_r = B_r^T y behind it; ONE sum over the ranks; the unpack
 * forms H = e^{-2 sigma} G + diag(1 / (sd e^rho)^2) (loglik_std.cpp:170-173,
 * logpr_gauss.cpp:153-158, fit.cpp:503-512) in full symmetric storage in d_H; Cholesky and
 * the two triangular solves (replicated on every rank) give d_theta.  d_y: this rank's rows,
 * already standardised.  d_H (p x p; on return its lower triangle is the Cholesky factor),
 * d_g (p: B^T y over all ranks), d_theta (p), d_diagH (p, may be NULL), d_exbuf
 * (obhip_fit_newton_count doubles whose padding the caller zeroed once), d_workspace
 * (obhip_newton_workspace_bytes): device memory of the caller.  comm = NULL: one rank, the
 * reduction writes H itself, d_exbuf is not used. */
int obhip_fit_newton_sharded_dev(obhip_comm *comm, const obhip_basis *b, const obhip_terms *t,
                                 const obhip_model *m, const double *d_y, double sigma, double rho,
                                 double *d_H, double *d_g, double *d_theta, double *d_diagH,
                                 double *d_exbuf, uint64_t exbuf_count, void *d_workspace,
                                 uint64_t workspace_bytes);
int obhip_normal_eq_exchange_dev(obhip_comm *comm, uint64_t p, uint64_t n_local, double *d_G,
                                 double *d_g, const double *d_b1, const double *d_sum2,
                                 double *d_buf, uint64_t buf_count, double *d_meansd);

/* ---- several responses over one design (no reference counterpart) ---------------------
 * The reference fits one y (obfit, R/fitting.R:40-120); what it has for several columns are the
 * matrix forms of prodmm_ / tprodmm_ (src/linalg.cpp:481-637).  Here q responses Y (n x q,
 * column-major, leading dimension ldy >= n) over one x share the model, the terms, sigma and
 * rho, hence G = B^T B, H and its Cholesky factor, which are formed ONCE; B^T Y, the
 * triangular solves and the predictor are batched over the responses in blocks of 16 columns
 * (64 per pass, so the scratch does not grow with q).  Theta is p x q, mean n_new x q, both
 * column-major without padding; any q >= 1.  Response 0 takes the single-response code path
 * throughout (with q = 1 every entry below gives the bits of its single-response twin).
 * obfit's standardisation (R/fitting.R:55-57) of every column on its own, like
 * obhip_standardise_dev: two passes, n - 1 denominator, summed over the ranks of comm in TWO
 * exchanges for the whole batch (2 q and q doubles).  d_Y_raw, d_Y: n x q with leading
 * dimension ldy (may be the same buffer); d_meansd: q triples (mean, sd, rows of all ranks).  A
 * constant column gets what obhip_standardise_dev gives it (sd = 0, NaN entries); the other
 * columns are not affected. */
int obhip_standardise_multi_dev(obhip_comm *comm, const double *d_Y_raw, uint64_t n, uint64_t q,
                                uint64_t ldy, double *d_Y, double *d_meansd);
/* obpred's de-standardisation (R/fitting.R:152) per column, in place: v = mean_j + sd_j v, or
 * with squared != 0 v = sd_j^2 v (variances).  d_V: n x q, leading dimension ldv. */
int obhip_destandardise_multi_dev(double *d_V, uint64_t n, uint64_t q, uint64_t ldv,
                                  const double *d_meansd, int squared);
/* doubles of exchange buffer obhip_fit_newton_multi_dev needs: [packed upper triangle of G :
 * p (p + 1) / 2][B^T Y : p q, column-major][zero padding to a multiple of 2 nranks]; with
 * q = 1 this is obhip_fit_newton_count */
int obhip_fit_newton_multi_count(uint64_t p, uint64_t q, int nranks, uint64_t *count);
/* bytes of device workspace of the two entries below: obhip_newton_workspace_bytes(p) plus the
 * right-hand sides of one pass of the batched substitutions (the same for every q) */
int obhip_newton_multi_workspace_bytes(uint64_t p, uint64_t q, uint64_t *bytes);
/* obhip_newton_solve_dev (lpdf::optnewton, fit.cpp:98-131) for q right-hand sides d_G_rhs
 * (p x q: B^T Y): H is formed from the caller's raw G and factorised once, d_Theta (p x q) =
 * solve(H, e^{-2 sigma} B^T Y) by blocked forward and backward substitution on the factor (no
 * inverse of L is formed).  d_G is overwritten by the factor; d_diagH (p) may be NULL. */
int obhip_newton_multi_solve_dev(const obhip_model *m, const obhip_terms *t, double *d_G,
                                 const double *d_G_rhs, uint64_t q, double sigma, double rho,
                                 double *d_Theta, double *d_diagH, void *d_workspace,
                                 uint64_t workspace_bytes);
/* obhip_fit_newton_sharded_dev with q right-hand sides, same contract and error codes
 * (OBHIP_ERR_NUMERIC for a Hessian that is not positive definite): d_Y this rank's rows,
 * already standardised; d_G_rhs (p x q) receives B^T Y over all ranks; on return the lower
 * triangle of d_H holds the Cholesky factor; d_exbuf: obhip_fit_newton_multi_count doubles
 * whose padding the caller zeroed once; d_workspace: obhip_newton_multi_workspace_bytes.
 * comm = NULL: one rank, d_exbuf is not used.  B^T Y is one pass over the staged design matrix
 * for up to 64 responses; where that matrix is not resident as a whole (row chunks, Gram
 * backend 3), or fewer than eight responses are left beside response 0 (a batched pass costs
 * the same for 1 to 16 columns), it is one pass over the basis per response. */
int obhip_fit_newton_multi_dev(obhip_comm *comm, const obhip_basis *b, const obhip_terms *t,
                               const obhip_model *m, const double *d_Y, uint64_t q, uint64_t ldy,
                               double sigma, double rho, double *d_H, double *d_G_rhs,
                               double *d_Theta, double *d_diagH, double *d_exbuf,
                               uint64_t exbuf_count, void *d_workspace, uint64_t workspace_bytes);
/* obhip_predict_dev for q coefficient vectors: column j of d_mean (n x q) = B(x) Theta[:, j],
 * the term products formed once per row and term for all responses.  d_var (n, may be NULL,
 * needs d_coeffvar) = B^2 coeffvar + e^{2 sigma} as obhip_predict_dev gives it: in standardised
 * units it is the same for every response.  Terms on more basis columns than the fused kernel's
 * LDS tile holds (and OBHIP_FORCE_GENERIC), and fewer than eight responses beside response 0,
 * take obhip_predict_dev's path column by column. */
int obhip_predict_multi_dev(const obhip_model *m, const obhip_terms *t, const double *d_Theta,
                            uint64_t q, const double *d_x, uint64_t n, double *d_mean,
                            const double *d_coeffvar, double sigma, double *d_var);
/* host-buffer conveniences like obhip_fit_newton / obhip_predict: Y (n x q, ldy; standardised
 * by the caller), Theta (p x q), diagH (p, may be NULL); x n x d with ldx, mean n x q, var n */
int obhip_fit_newton_multi(const obhip_basis *b, const obhip_terms *t, const obhip_model *m,
                           const double *Y, uint64_t q, uint64_t ldy, double sigma, double rho,
                           double *Theta, double *diagH);
int obhip_predict_multi(const obhip_model *m, const obhip_terms *t, const double *Theta,
                        uint64_t q, const double *x, uint64_t n, uint64_t ldx, double *mean,
                        const double *coeffvar, double sigma, double *var);

/* ---- weighted, binomial and Poisson responses: iteratively reweighted least squares ----------
 * (no reference counterpart: every fit of the reference, and every entry above, has a Gaussian
 * response with one noise level for all rows.)  For rows i with prior weights a_i > 0 (NULL: 1)
 * and offsets o_i (NULL: 0), eta = o + B theta and P = diag(prior precisions of the terms at
 * rho), the entries below maximise
 *     F(theta) = sum_i a_i l(y_i, eta_i) - theta^T P theta / 2
 *   family     link      l(y, eta)                       mu                  IRLS weight w      y
 *   GAUSSIAN   identity  -e^{-2 sigma} (y - eta)^2 / 2   eta                 a e^{-2 sigma}     finite
 *   BINOMIAL   logit     y eta - softplus(eta)           1 / (1 + e^{-eta})  a mu (1 - mu)      in [0, 1]
 *   POISSON    log       y eta - e^eta                   e^eta               a mu               >= 0
 * (binomial y: proportions, a = trials; sigma is read by the Gaussian family only; y standardised
 * by the caller as for obhip_fit_newton_multi_dev).  With e = exp(-|eta|) the binomial forms are
 * free of overflow: mu = eta >= 0 ? 1 / (1 + e) : e / (1 + e), mu (1 - mu) = e / (1 + e)^2,
 * softplus(eta) = max(eta, 0) + log1p(e).
 * Newton's method from theta = 0 (eta = o), or from the caller's theta with info->warm_start:
 *   1. row pass: mu, w, the weighted row factor scale_w = scale sqrt(w) of the basis, the working
 *      column u = a (y - mu) (Gaussian: e^{-2 sigma}) / sqrt(w), so that B_w^T u = B^T (a (y - mu)),
 *      and sum a l;
 *   2. H = B_w^T B_w + P, g = B_w^T u - P theta by the Gram pipeline of the fits above on the
 *      caller's basis with its row factors exchanged for scale_w for the length of that Gram (no
 *      copy of the basis; restored on every exit path, after which an unweighted use stages the
 *      design matrix again), Cholesky, delta = inv(H) g, dec = g^T delta;
 *   3. one B delta on the unweighted basis; a trial step alpha is then one row pass on
 *      eta + alpha B delta and a p-sized dot product;
 *   4. dec <= tol (1 + |F|): the full step is taken and the fit has converged (the last step is
 *      the one that brings theta to rounding level);
 *   5. otherwise alpha is halved from 1 until F(theta + alpha delta) is finite and not below
 *      F(theta) - slack, slack = (n + p + 16) 2^-53 (A(theta) + A(theta + alpha delta)), A = the
 *      sum of the magnitudes F is summed of: the rounding bound of the two sums, so that no step is
 *      refused on rounding noise alone.  30 halvings without a step: OBHIP_ERR_NUMERIC.
 * One response, all rows on one device: row sharding (obhip_comm), several responses and the
 * streaming accumulator are not offered, the weights change with every iteration and differ per
 * response. */
#define OBHIP_GLM_GAUSSIAN 0
#define OBHIP_GLM_BINOMIAL 1
#define OBHIP_GLM_POISSON 2
typedef struct obhip_glm_info {
  int warm_start;      /* in: non-zero = start from the theta the caller passed */
  int converged;       /* out: step 4 was reached within maxit iterations */
  uint64_t iterations; /* out: Newton steps taken, the last one included */
  uint64_t halvings;   /* out: halvings of alpha over all line searches */
  double dec;          /* out: g^T delta of the last step */
  double F;            /* out: the penalised log-likelihood at the returned theta */
  double deviance;     /* out: 2 sum a (l(y, saturated) - l(y, eta)) at the returned theta */
} obhip_glm_info;
/* bytes of device workspace of obhip_fit_glm_dev for p terms and n rows (host arithmetic) */
int obhip_glm_workspace_bytes(uint64_t p, uint64_t n, uint64_t *bytes);
/* The row pass on its own.  All vectors have n entries except d_scale, d_scale_w and d_u, which
 * have n rounded up to a multiple of 64 like the row factors of a basis.
 *   eta_i = (d_eta ? d_eta[i] : d_o ? d_o[i] : 0) + (d_deta ? alpha d_deta[i] : 0)
 * (d_eta holds o + B theta of an earlier pass, so d_o is read only where a pass starts from it);
 * d_a NULL: weights 1.  Written: d_eta_out (may be d_eta), d_mu (may be NULL), d_scale_w =
 * d_scale sqrt(w), d_u; rows >= n of d_scale_w and d_u are written as zeros whatever the inputs
 * hold there, and a row with w = 0 (binomial beyond |eta| = 745) or a non-finite w has u = 0.
 * With d_eta_out, d_mu, d_scale_w and d_u all NULL the pass is a trial: nothing but the sums is
 * written.  d_sums (3): sum a l over the rows whose l is finite, the sum of the magnitudes
 * a (|y eta| + |b(eta)|) (l = y eta - b(eta); Gaussian: a |l|), and the number of rows whose l is
 * not finite -- read that in place of a NaN-poisoned sum.  Fixed two-stage summation order, no
 * atomics: the same bits on every call. */
int obhip_glm_rows_dev(int family, uint64_t n, const double *d_eta, const double *d_deta,
                       double alpha, const double *d_y, const double *d_a, const double *d_o,
                       double sigma, const double *d_scale, double *d_eta_out, double *d_mu,
                       double *d_scale_w, double *d_u, double *d_sums);
/* The fit.  d_y, d_a, d_o: n rows of the basis (d_a, d_o may be NULL); d_H: p x p, on return its
 * lower triangle holds the Cholesky factor of the last Hessian and d_diagH (p, may be NULL) that
 * Hessian's diagonal; d_theta (p): out, in/out with info->warm_start; d_eta (n, may be NULL):
 * o + B theta at the returned theta; d_ws: obhip_glm_workspace_bytes(p, n).  maxit >= 1
 * iterations without convergence are no error (info->converged = 0).  OBHIP_ERR_NUMERIC: a
 * Hessian that is not positive definite, a start at which F is not finite, a line search that
 * finds no step; OBHIP_ERR_INVALID for argument errors, before the first launch. */
int obhip_fit_glm_dev(const obhip_basis *b, const obhip_terms *t, const obhip_model *m, int family,
                      const double *d_y, const double *d_a, const double *d_o, double sigma,
                      double rho, double tol, uint64_t maxit, double *d_H, double *d_theta,
                      double *d_diagH, double *d_eta, obhip_glm_info *info, void *d_ws,
                      uint64_t ws_bytes);
/* obhip_predict_dev's path without a noise term, then the response scale: d_eta (n) = o +
 * B(x) theta, d_vareta = B^2 coeffvar (needs d_coeffvar), d_mu = the inverse link of eta, d_varmu
 * = (d mu / d eta)^2 vareta (delta method).  Any output may be NULL; n = 0 is a no-op. */
int obhip_predict_glm_dev(const obhip_model *m, const obhip_terms *t, int family,
                          const double *d_theta, const double *d_x, uint64_t n, const double *d_o,
                          const double *d_coeffvar, double *d_eta, double *d_vareta, double *d_mu,
                          double *d_varmu);
/* host-buffer forms like obhip_fit_newton_multi / obhip_predict_multi.  They check, before any
 * device call, that y is in its family's domain and the weights are finite and > 0
 * (OBHIP_ERR_INVALID).  theta (p): out, in/out with info->warm_start; diagH, eta may be NULL. */
int obhip_fit_glm(const obhip_basis *b, const obhip_terms *t, const obhip_model *m, int family,
                  const double *y, const double *a, const double *o, double sigma, double rho,
                  double tol, uint64_t maxit, double *theta, double *diagH, double *eta,
                  obhip_glm_info *info);
int obhip_predict_glm(const obhip_model *m, const obhip_terms *t, int family, const double *theta,
                      const double *x, uint64_t n, uint64_t ldx, const double *o,
                      const double *coeffvar, double *eta, double *vareta, double *mu,
                      double *varmu);

/* ---- variance-based sensitivity of the fitted mean (no reference counterpart) ------------------
 * The fitted mean is f(x) = sum_k theta_k prod_l psi_{l, t_kl}(x_l), psi_l = getbase(l) (the raw
 * cov . rotmat).  Under independent inputs with a discrete measure per dimension -- nodes z_il with
 * weights w_il >= 0 normalised by their sum: the empirical marginals of a sample (no weights) or a
 * quadrature rule of a density -- every variance-based index is a closed-form sum over the moment
 * tables of the 1-D bases; no sampling is involved.  With L_l = 1 + obhip_terms_maxlevels[l]:
 *   mean table  m_l[t]    = sum_i w^_i psi_{l,t}(z_il)                       packed, sum L_l doubles,
 *                                                                            dimension l at sum_{i<l} L_i
 *   cov table   C_l[t,t'] = sum_i w^_i (psi_t - m_t)(psi_t' - m_t')          packed, sum L_l^2 doubles,
 *                                                                            row-major per dimension
 * (two passes: means, then centred products) and A_l = C_l + m_l m_l^T.  Per response column theta:
 *   mu   = sum_k theta_k prod_l m_l[t_kl]
 *   V1_l = g_l^T C_l g_l,  g_l[t] = sum_{k: t_kl = t} theta_k prod_{i != l} m_i[t_ki]   (Var E[f | x_l])
 *   VT_l = sum_{k,k'} theta_k theta_k' C_l[t,t'] prod_{i != l} A_i[t_ki, t_k'i]        (V - Var E[f | x_~l])
 *   V    = sum_{k,k'} theta_k theta_k' sum_l (prod_{i<l} A_i) C_l (prod_{i>l} m_i m_i)  (= prod A - prod m m)
 * and E[f | x_l = z] = sum_t g_l[t] psi_{l,t}(z).  All sums are taken in a fixed order without
 * atomics: the same bits on every call.  Levels beyond 255 in a dimension and tables beyond the LDS
 * of a workgroup are refused (OBHIP_ERR_INVALID).  Argument errors return OBHIP_ERR_INVALID before
 * any device call. */
/* *n_mean = sum L_l, *n_cov = sum L_l^2 (either may be NULL) */
int obhip_sobol_layout(const obhip_terms *t, uint64_t *n_mean, uint64_t *n_cov);
/* The tables of the measure.  d_nodes: n x d column-major with ldx >= n; d_weights: n x d
 * column-major with ldw >= n, or NULL (all 1); rows n .. ld are never read.  n = 0 is
 * OBHIP_ERR_INVALID (there is no measure).  A weight that is negative or not finite, or a column
 * of weights whose sum is not > 0: OBHIP_ERR_NUMERIC (found on the device; the call waits for it). */
int obhip_dim_moments_dev(const obhip_model *m, const obhip_terms *t, const double *d_nodes,
                          uint64_t n, uint64_t ldx, const double *d_weights, uint64_t ldw,
                          double *d_mean, double *d_cov);
int obhip_sobol_workspace_bytes(uint64_t p, uint64_t d, uint64_t q, uint64_t *bytes);
/* d_Theta: p x q column-major, ld = p.  d_mean_tab / d_cov_tab: tables in the layout above -- those
 * of obhip_dim_moments_dev or any others; every C_l must be symmetric (only the pairs k <= k' of
 * term tiles are visited).  d_out: q x (2 + 2 d) row-major, per response [mu, V, V1_0 .. V1_{d-1},
 * VT_0 .. VT_{d-1}].  d_g (may be NULL; d_out has the same bits either way): the g_l packed like a
 * mean table, response j at j * sum L_l.  d_ws: obhip_sobol_workspace_bytes(p, d, q). */
int obhip_sobol_dev(const obhip_terms *t, const double *d_Theta, uint64_t q,
                    const double *d_mean_tab, const double *d_cov_tab, double *d_out, double *d_g,
                    void *d_ws, uint64_t ws_bytes);
/* d_out (G x q column-major, ld = G) = psi_dim at the G points d_grid times the g_dim of every
 * response: E[f | x_dim = z], from which the caller subtracts mu.  d_g as obhip_sobol_dev writes it.
 * G = 0 is a no-op. */
int obhip_main_effect_dev(const obhip_model *m, const obhip_terms *t, uint64_t dim,
                          const double *d_g, uint64_t q, const double *d_grid, uint64_t G,
                          double *d_out);
/* host-buffer forms: nodes n x d with ldx, weights n x d with ldw or NULL, mean / cov the packed
 * tables; Theta p x q (ld = p), out q x (2 + 2 d), g (may be NULL) q x sum L_l */
int obhip_dim_moments(const obhip_model *m, const obhip_terms *t, const double *nodes, uint64_t n,
                      uint64_t ldx, const double *weights, uint64_t ldw, double *mean, double *cov);
int obhip_sobol(const obhip_terms *t, const double *Theta, uint64_t q, const double *mean_tab,
                const double *cov_tab, double *out, double *g);
/* Which inputs matter together: for every pair of dimensions i < j, in the order (0,1), (0,2), ..
 * (0,d-1), (1,2), .. -- n_pairs = d (d - 1) / 2 of them -- with t = t_ki, s = t_kj:
 *   G_ij[t,s] = sum_{k: t_ki = t, t_kj = s} theta_k prod_{l != i,j} m_l[t_kl]   (L_i x L_j, row-major; no division)
 *   V2_ij     = tr(C_i G_ij C_j G_ij^T)              = Var E[f | x_i, x_j] - V1_i - V1_j, the pure second order
 *   VT2_ij    = sum_{k,k'} theta_k theta_k' C_i[t,t'] C_j[s,s'] prod_{l != i,j} A_l[t_kl, t_k'l]
 *                                                    = the variances of all subsets that hold both i and j
 * and E[f | x_i = z, x_j = z'] = sum_{t,s} G_ij[t,s] psi_{i,t}(z) psi_{j,s}(z').  The limits are those of
 * obhip_sobol_dev, refused with a message before any device call; fixed summation order, no atomics. */
/* *n_pairs = d (d - 1) / 2, *n_G = sum_{i<j} L_i L_j: a packed G holds G_ij in pair order (either may be NULL) */
int obhip_sobol2_layout(const obhip_terms *t, uint64_t *n_pairs, uint64_t *n_G);
int obhip_sobol2_workspace_bytes(uint64_t p, uint64_t d, uint64_t q, uint64_t *bytes);
/* d_Theta and the tables as obhip_sobol_dev takes them (every C_l symmetric).  d_out: q x 2 n_pairs
 * row-major, per response [V2 of every pair, VT2 of every pair].  d_G (may be NULL; d_out has the same
 * bits either way): the packed G, response j at j * n_G.  d_ws: obhip_sobol2_workspace_bytes(p, d, q).
 * d = 1 has no pairs: nothing is written (d_out, d_G and d_ws are not looked at) and the call returns OK. */
int obhip_sobol2_dev(const obhip_terms *t, const double *d_Theta, uint64_t q,
                     const double *d_mean_tab, const double *d_cov_tab, double *d_out, double *d_G,
                     void *d_ws, uint64_t ws_bytes);
/* The conditional mean E[f | x_dim_i = z_a, x_dim_j = z'_b] on the grid d_grid_i (Gi) x d_grid_j (Gj):
 * d_out[(r Gi + a) Gj + b] for response r -- q slabs of Gi x Gj, row-major, b fastest.  d_G as
 * obhip_sobol2_dev writes it for q responses.  The caller subtracts the two main effects and mu for the
 * interaction surface.  Gi Gj = 0 is a no-op; dim_i == dim_j or a dimension out of range is
 * OBHIP_ERR_INVALID; dim_i > dim_j reads G transposed. */
int obhip_interaction_effect_dev(const obhip_model *m, const obhip_terms *t, uint64_t dim_i,
                                 uint64_t dim_j, const double *d_G, uint64_t q,
                                 const double *d_grid_i, uint64_t Gi, const double *d_grid_j,
                                 uint64_t Gj, double *d_out);
/* host-buffer form: out q x 2 n_pairs, G (may be NULL) q x n_G */
int obhip_sobol2(const obhip_terms *t, const double *Theta, uint64_t q, const double *mean_tab,
                 const double *cov_tab, double *out, double *G);
/* One number per input that sums to V: the Shapley effect Sh_l = sum_{u contains l} V_u / |u| (Owen 2014), V_u the
 * variance of the ANOVA term of the subset u.  Players are groups of dimensions, a partition of 0 .. d-1 into P
 * groups; per term pair (k, k'), with c_i = C_i[t,t'], mm_i = m_i[t] m_i[t'], A_i = c_i + mm_i, a player g has
 *   mm_g = prod_{i in g} mm_i,   c_g = prod_{i in g} A_i - prod_{i in g} mm_i   (by D <- c_i PA + mm_i D,
 *                                                                                PA <- PA A_i: no cancellation)
 *   Sh_g = sum_{k,k'} theta_k theta_k' c_g int_0^1 prod_{h != g} (mm_h + s c_h) ds,   sum_g Sh_g = V
 * The integrand is a polynomial of degree P - 1 in s: the Gauss-Legendre rule of ceil(P / 2) nodes on [0,1] is
 * exact, its weights are positive and nothing is divided.  The limits are those of obhip_sobol_dev and at most 40
 * players (more dimensions than that must be grouped), refused with a message before any device call; fixed
 * summation order, no atomics: the same bits on every call. */
/* Host only: the Gauss-Legendre rule of G nodes on [0,1], 1 <= G <= 128 (OBHIP_ERR_INVALID otherwise), nodes
 * ascending, weights summing to 1; computed in long double and rounded once. */
int obhip_gauss_legendre01(uint64_t G, double *nodes, double *weights);
/* groups: d player ids on the host, exactly 0 .. P-1 with every id used, or NULL: dimension l is player l.
 * *n_players = P, *n_nodes = ceil(P / 2) (either may be NULL); P > 40 is OBHIP_ERR_INVALID. */
int obhip_shapley_layout(const obhip_terms *t, const int32_t *groups, uint64_t *n_players,
                         uint64_t *n_nodes);
int obhip_shapley_workspace_bytes(uint64_t p, uint64_t d, uint64_t q, uint64_t *bytes);
/* d_Theta and the tables as obhip_sobol_dev takes them (every C_l symmetric).  d_out: q x P row-major, in
 * variance units, player g at column g.  d_ws: obhip_shapley_workspace_bytes(p, d, q). */
int obhip_shapley_dev(const obhip_terms *t, const int32_t *groups, const double *d_Theta, uint64_t q,
                      const double *d_mean_tab, const double *d_cov_tab, double *d_out, void *d_ws,
                      uint64_t ws_bytes);
/* host-buffer form: out q x P */
int obhip_shapley(const obhip_terms *t, const int32_t *groups, const double *Theta, uint64_t q,
                  const double *mean_tab, const double *cov_tab, double *out);

/* ---- active subspaces and derivative-based sensitivity (no reference counterpart) ------------------
 * C = E[grad f grad f^T] and gbar = E[grad f] of the fitted mean under the product measure above, in closed
 * form: the diagonal of C holds the derivative-based global sensitivity measures (DGSM, nu_l = C_ll), its
 * eigenvectors span the active subspace.  psi' = d psi / d x_l in raw input units, the raw (dcov/dx) . rotmat.
 * Three more tables per dimension, all raw moments -- nothing is centred and nothing subtracted:
 *   dm_l[t]   = sum_i w^_i psi'_{l,t}(z_il)                        packed like the mean table (sum L_l)
 *   X_l[a,b]  = sum_i w^_i psi'_{l,a}(z_il) psi_{l,b}(z_il)          packed like the cov table (sum L_l^2), NOT symmetric
 *   D_l[a,b]  = sum_i w^_i psi'_{l,a}(z_il) psi'_{l,b}(z_il)         packed like the cov table, exactly symmetric
 * Per response, with t = t_kl, t' = t_k'l, s = t_km, s' = t_k'm and A_l = C_l + m_l m_l^T of the tables above:
 *   gbar_l = sum_k theta_k dm_l[t] prod_{i != l} m_i[t_ki]                                   E[d f / d x_l]
 *   C_ll   = sum_{k,k'} theta_k theta_k' D_l[t,t'] prod_{i != l} A_i[t_ki,t_k'i]              = nu_l
 *   C_lm   = sum_{k,k'} theta_k theta_k' X_l[t,t'] X_m[s',s] prod_{i != l,m} A_i[t_ki,t_k'i]  l != m (X_m transposed)
 * Exchanging k and k' maps the summand of C_lm onto that of C_ml: the pair sum runs over the upper triangle of
 * term tiles and adds both orientations of every pair.  Fixed summation order, no atomics: the same bits on
 * every call.  The limits are those of obhip_sobol_dev with three tables of sum L_l^2 entries in the LDS of a
 * workgroup, refused with a message before any device call.  d = 1 is valid: one gbar and one C_00. */
/* *n_mean = sum L_l, *n_cov = sum L_l^2, *n_out = d + d (d + 1) / 2 (each may be NULL) */
int obhip_active_layout(const obhip_terms *t, uint64_t *n_mean, uint64_t *n_cov, uint64_t *n_out);
/* The gradient tables of the measure; nodes, weights, errors and layout as obhip_dim_moments_dev (a bad weight
 * or a column of weights without mass: OBHIP_ERR_NUMERIC).  d_dmean: sum L_l doubles; d_cross, d_dd: sum L_l^2
 * doubles each, row-major per dimension.  Neither the basis nor its derivative is written to memory. */
int obhip_dim_grad_moments_dev(const obhip_model *m, const obhip_terms *t, const double *d_nodes,
                               uint64_t n, uint64_t ldx, const double *d_weights, uint64_t ldw,
                               double *d_dmean, double *d_cross, double *d_dd);
int obhip_active_workspace_bytes(uint64_t p, uint64_t d, uint64_t q, uint64_t *bytes);
/* d_Theta and d_mean_tab / d_cov_tab as obhip_sobol_dev takes them (every C_l symmetric); d_dmean, d_cross,
 * d_dd: the tables above (D_l symmetric; X_l as it is).  d_out: q x (d + d (d + 1) / 2) row-major, per response
 * [gbar_0 .. gbar_{d-1}, C packed: the upper triangle with the diagonal, row-major -- C_00, C_01, .. C_0,d-1,
 * C_11, ..].  d_ws: obhip_active_workspace_bytes(p, d, q). */
int obhip_active_dev(const obhip_terms *t, const double *d_Theta, uint64_t q,
                     const double *d_mean_tab, const double *d_cov_tab, const double *d_dmean,
                     const double *d_cross, const double *d_dd, double *d_out, void *d_ws,
                     uint64_t ws_bytes);
/* host-buffer forms */
int obhip_dim_grad_moments(const obhip_model *m, const obhip_terms *t, const double *nodes, uint64_t n,
                           uint64_t ldx, const double *weights, uint64_t ldw, double *dmean,
                           double *cross, double *dd);
int obhip_active(const obhip_terms *t, const double *Theta, uint64_t q, const double *mean_tab,
                 const double *cov_tab, const double *dmean, const double *cross, const double *dd,
                 double *out);
/* Host only: the eigen-decomposition of the symmetric n x n matrix A (column-major; the upper triangle is
 * read), 1 <= n <= 4096 (OBHIP_ERR_INVALID otherwise; an entry that is not finite: OBHIP_ERR_NUMERIC), by the
 * cyclic Jacobi method.  w: the n eigenvalues, descending; V: n x n column-major, column j the unit
 * eigenvector of w[j], signed so that its component of largest magnitude is positive (the lowest index wins
 * a tie). */
int obhip_sym_eigh(uint64_t n, const double *A, double *w, double *V);

/* ---- streaming Newton fit: rows come and go, one pass over each (no reference counterpart) ----
 * obfit (R/fitting.R:40-120) and every fit entry above take all rows at once and form the whole
 * Gram again per call.  An obhip_normal_acc keeps, in HBM, the sufficient statistics of the Newton
 * step for the rows it has been given -- the algebra of "the one exchange of back end A" with the
 * shards spread over time instead of over ranks, standardising AFTER the sum:
 * B^T ((y - cent) / sd) = (B^T y - cent B^T 1) / sd.  State, obhip_normal_acc_bytes(p, q) / 8 doubles:
 *   [upper triangle of G = B^T B, row-major packed as in obhip_normal_eq_count : p (p + 1) / 2]
 *   [R = B^T (Y - c) : p x q, column-major][B^T 1 : p][per response c, mu, M2, n : 4 q]
 * c_j is a fixed shift of response j (its first row ever added), mu_j = mean(y_j) - c_j and
 * M2_j = sum (y_j - mean(y_j))^2 over the rows in the state; batches and accumulators merge by the
 * pairwise update of Chan, Golub and LeVeque and leave by its inverse, all in differences from c, so
 * a mean far from zero costs no digits.  Removal SUBTRACTS sums: its rounding error is that of the
 * rows that were ever in the state, not of those that remain.
 * An accumulator is bound to one model and one term set (the caller keeps both alive) and to the
 * model's hyper-parameters and knots as they are when its first rows come in: any later change
 * makes add / combine / solve fail with OBHIP_ERR_STATE until obhip_normal_acc_reset.  Argument
 * errors are OBHIP_ERR_INVALID, and every check runs before the first launch: a refused call leaves
 * the accumulator unchanged.  Handles are used by one thread at a time; the _dev entries enqueue on
 * the library's stream and do not synchronise, with one exception: obhip_normal_acc_solve_dev waits
 * for its factorisation like the other solve entries (that is how OBHIP_ERR_NUMERIC is reported),
 * and uploads the prior precisions when the model or rho differ from its last call.  q >= 1
 * responses (at most 65534). */
int obhip_normal_acc_create(obhip_normal_acc **out, const obhip_model *m, const obhip_terms *t,
                            uint64_t q);
int obhip_normal_acc_destroy(obhip_normal_acc *acc);
/* back to no rows (and free to follow the model's current hyper-parameters) */
int obhip_normal_acc_reset(obhip_normal_acc *acc);
/* terms, responses, rows in the state, batches added and not removed; any pointer may be NULL */
int obhip_normal_acc_info(const obhip_normal_acc *acc, uint64_t *p, uint64_t *q, uint64_t *rows,
                          uint64_t *batches);
/* bytes of device memory of one accumulator: 8 (p (p + 1) / 2 + p q + p + 4 q); host arithmetic */
int obhip_normal_acc_bytes(uint64_t p, uint64_t q, uint64_t *bytes);
/* the state as laid out above into d_out (device, count >= obhip_normal_acc_bytes / 8 doubles) */
int obhip_normal_acc_export_dev(const obhip_normal_acc *acc, double *d_out, uint64_t count);
/* sign = +1: add the rows of `basis` (built on the accumulator's model, after its last change;
 * another model: OBHIP_ERR_INVALID) with their RAW responses d_Y_raw (n_b x q, column-major, leading
 * dimension ldy); sign = -1: take out a batch that was added before (more rows than the state
 * holds: OBHIP_ERR_STATE; a state left without rows is reset).  The batch's Gram is formed by the
 * Gram kernels of obhip_gram_dev into a packed triangle in scratch, B^T [Y - c | 1] as
 * obhip_fit_newton_multi_dev forms B^T Y, and one pass folds both into the state: the cost is that
 * of a fit of n_b rows without its Cholesky.  Scratch: one more state's worth of pooled device
 * memory plus n_b (q + 1) doubles, for the duration of the call.  A basis of no rows cannot exist;
 * callers skip empty batches. */
int obhip_normal_acc_add_dev(obhip_normal_acc *acc, const obhip_basis *basis, const double *d_Y_raw,
                             uint64_t ldy, int sign);
/* dst = dst + sign src (sign = +1 / -1) for two accumulators of the same model, terms and q:
 * triangle, right-hand sides (src's moved to dst's shift) and moments; src is not written */
int obhip_normal_acc_combine_dev(obhip_normal_acc *dst, const obhip_normal_acc *src, int sign);
/* The Newton step of obhip_newton_multi_solve_dev (lpdf::optnewton, fit.cpp:98-131, from
 * coeff = 0) on the rows in acc -- with minus != NULL on the rows of acc without those of minus,
 * which must be among them -- every response standardised over exactly those rows as obfit does
 * (R/fitting.R:55-57, n - 1 denominator).  Neither accumulator is written.  d_H (p x p) receives
 * H = e^{-2 sigma} (T - T_minus) + diag(1 / (sd e^rho)^2) and then, in its lower triangle, the
 * Cholesky factor; d_Theta p x q; d_diagH (p) may be NULL; d_meansd: q triples (mean, sd, rows) as
 * from obhip_standardise_multi_dev; d_workspace: obhip_newton_multi_workspace_bytes(p, q).  Fewer
 * than two rows left: OBHIP_ERR_STATE; a Hessian that is not positive definite (possible after a
 * removal that cancels most of G): OBHIP_ERR_NUMERIC, as the other solve entries report it.  A
 * response that is constant over the rows that remain -- or whose M2 a removal has cancelled to
 * zero -- gets sd = 0 and non-finite coefficients without an error, as obhip_standardise_multi_dev
 * treats a constant column; d_meansd shows it. */
int obhip_normal_acc_solve_dev(const obhip_normal_acc *acc, const obhip_normal_acc *minus,
                               double sigma, double rho, double *d_H, double *d_Theta,
                               double *d_diagH, double *d_meansd, void *d_workspace,
                               uint64_t workspace_bytes);
/* Held-out score of a cross-validation fold: d_out[2 j] = sum over the n rows of
 * (mean_j + sd_j d_mean[i, j] - d_Y_raw[i, j])^2, the squared error in raw units of the
 * standardised predictions d_mean (d_meansd = NULL: d_mean is in raw units already), and
 * d_out[2 j + 1] = n.  d_mean, d_Y_raw: n x q, column-major, leading dimension ld.  One two-stage
 * reduction in a fixed order, no atomics: the same bits on every run. */
int obhip_cv_score_dev(const double *d_mean, const double *d_Y_raw, uint64_t n, uint64_t q,
                       uint64_t ld, const double *d_meansd, double *d_out);

/* ---- observed input gradients as rows of the Newton fit (no reference counterpart) ----
 * A computer code with an adjoint returns dy/dx with y: 1 + d equations per run.  With
 * y~ = (y - cent) / sd and g~_l = g_l / sd (the gradient has no offset: cent and sd come from the
 * value rows only), D_l[i,k] = dB[i,k] / dx_l and a weight w_l > 0 per differentiated dimension
 * (gradients carry the units of 1 / x_l, so their noise differs by dimension) the Newton step solves
 *   (e^{-2 sigma} (B^T B + sum_l w_l D_l^T D_l) + diag(prec)) theta
 *       = e^{-2 sigma} (B^T y~ + sum_l w_l D_l^T g~_l).
 * In the accumulator's state a gradient batch adds sum_l w_l D_l^T D_l to the triangle and
 * sum_l w_l D_l^T g_l (raw g) to R, nothing to B^T 1 and the moments; the solve's right-hand side
 * (R - (cent - c) B^T 1) / sd is then already the one above.  In the notation of
 * obhip_predict_grad_dev,
 *   D_l[i,k] = s_i (rho_l P_k + [t_kl > 0] E_kl r'_{l,t_kl}),
 * every entry non-zero through rho_l, the derivative of the row scale: D_l is dense.
 * The batch is staged in row chunks as L blocks sqrt(w_l) D_l (one kernel; fused while the terms
 * use at most 8 factors and the tile of 2 Mu - 1 + d columns plus its reduction space fits 160 KB of
 * LDS, from a pooled HBM tile per block beyond that and under OBHIP_FORCE_GENERIC: every term set
 * obhip_predict_grad_dev accepts) and goes through the Gram kernels of obhip_gram_dev; the right-hand
 * side of the first response rides along with the staging, the others take one pass over the staged
 * chunk each.  No atomics: two calls give the same bits.  Scratch: the packed triangle, p q doubles
 * and one staged chunk (at most a quarter of the free HBM and 16 GB; OBHIP_GRAM_CHUNK_ROWS sets the
 * batch rows per chunk for tests).
 * dims (host): ndims distinct dimensions, each < d, 1 <= ndims <= d.  weights (host, ndims): finite
 * and > 0, NULL = all 1.  Refused in this order, before any device call, with OBHIP_ERR_INVALID:
 * a null argument, ndims = 0 (or > d), a repeated dimension, a dimension >= d, a weight <= 0 or not
 * finite, lddy < n, ldo < p.  n = 0 is a no-op; at most 2^40 rows per call. */
/* out[(j*n + i)*ldo + k] = sqrt(w_j) dB[i,k]/dx_{dims[j]}; d_x column-major n x d (ld = n); ldo >= p;
 * nothing else of d_out is written */
int obhip_design_dx_dev(const obhip_model *m, const obhip_terms *t, const double *d_x, uint64_t n,
                        const uint32_t *dims, uint64_t ndims, const double *weights,
                        double *d_out, uint64_t ldo);
/* d_dY_raw[(r*ndims + j)*lddy + i] = d y_r / d x_{dims[j]} at row i (raw units), r < q; sign = +1
 * adds the n ndims gradient equations, sign = -1 takes out a batch added before (more equations than
 * the state holds: OBHIP_ERR_STATE).  Value rows (obhip_normal_acc_info) and the fewer-than-two-rows
 * rule of the solve count value rows only; gradient and value batches may come in any order, and the
 * tie to the model's state holds from the first batch of either kind.  A state without value rows
 * and gradient equations is reset.  obhip_normal_acc_combine_dev and the `minus` of the solve carry
 * the gradient rows with them. */
int obhip_normal_acc_add_grad_dev(obhip_normal_acc *acc, const double *d_x, uint64_t n,
                                  const uint32_t *dims, uint64_t ndims, const double *weights,
                                  const double *d_dY_raw, uint64_t lddy, int sign);
/* gradient equations in the state (rows x differentiated dimensions) and their batches; either
 * pointer may be NULL */
int obhip_normal_acc_grad_info(const obhip_normal_acc *acc, uint64_t *grad_equations,
                               uint64_t *grad_batches);

/* ---- Newton fit on the product of two input blocks (no reference counterpart) ----
 * Training data on a full grid: the na nb pairs (row i of xa, row j of xb) of "product of two input
 * blocks" below, one response value per pair.  A design-matrix entry of the pair separates,
 * B[(i,j),k] = At[i,k] Bt[j,k] with At = diag(sA) U (na x p) and Bt = diag(sB) V (nb x p), and so do
 * the normal equations:
 *   B^T B = (At^T At) o (Bt^T Bt)   (Hadamard product),   B^T 1 = (At^T 1) o (Bt^T 1),
 *   (B^T y)_k = sum_i At[i,k] (Y Bt)[i,k].
 * The two side matrices are staged (one kernel per side; fused while the side's terms use at most 8
 * factors and its tile fits 160 KB of LDS, from a pooled HBM tile per block beyond that and under
 * OBHIP_FORCE_GENERIC), go through the Gram kernels of obhip_gram_dev as na + nb rows, and Y Bt is one
 * matrix-core product with the long index j contracted in ascending row chunks.  Nothing of size
 * na nb d or na nb p exists.  Y - c is formed by one subtraction per entry before anything is
 * contracted; the batch moments are those of obhip_normal_acc_add_dev over the na nb values in the
 * order i fast, j slow.  No atomics: two equal calls give the same bits.  Scratch: two packed
 * triangles, the staged A side (64 ceil(na / 64) x p_pad doubles, whole), one staged chunk of the B
 * side (at most a quarter of the free HBM and 16 GB; OBHIP_GRAM_CHUNK_ROWS sets the rows per chunk for
 * tests), q copies of Y padded to multiples of (128, 64) and the product of one block of at most 8
 * responses (128 ceil(na / 128) x p_pad doubles each).  When na is far larger than nb, name the
 * complement as dims_b and swap the blocks: the B side is the one that is chunked.
 * Every check runs before the first device call and a refused call leaves the state unchanged:
 * OBHIP_ERR_INVALID for a null argument, a sign other than +1 / -1, dims_b not strictly ascending or
 * out of range or with fewer than 1 or more than d - 1 entries, na = 0 or nb = 0 (a batch without
 * rows cannot be told from a mistake here), lda < na, more than 2^31 rows in xa, 2^40 in xb or 2^48
 * pairs, more than 65535 used basis columns on a side; OBHIP_ERR_STATE as obhip_normal_acc_add_dev.
 * A batch is taken out with the dims_b it was added with: the accumulator does not remember the
 * split, that is the caller's business. */
/* sign = +1: add the na*nb observations of the grid (xa_i on the dimensions not in dims_b, xb_j on dims_b);
 * sign = -1: take out a grid batch added before.  d_xa: column-major na x |A|, d_xb: column-major nb x |B|,
 * dims_b (host) as obhip_predict_product_dev takes them (strictly ascending, 1..d-1 entries).
 * d_Y_raw[(r*nb + j)*lda + i], lda >= na: the layout obhip_predict_product_dev writes its mean in; the
 * padding lda - na is never read.  rows grows by na*nb and batches by 1; the shift of a fresh
 * accumulator is Y_raw[r][0][0].  obhip_normal_acc_combine_dev, the `minus` of the solve and
 * obhip_normal_acc_posterior_dev carry grid batches like any other rows.  No reference counterpart. */
int obhip_normal_acc_add_product_dev(obhip_normal_acc *acc, const double *d_xa, uint64_t na,
                                     const double *d_xb, uint64_t nb, const uint32_t *dims_b,
                                     uint64_t ndims_b, const double *d_Y_raw, uint64_t lda, int sign);
/* the staged side matrix itself: out[i*pitch + k] = s_i * prod of the term's factors on that side
 * (side 0 = A at rows of xa, 1 = B at rows of xb; d_x column-major n x |side|), k < p, zeros up to
 * pitch; d_out holds 64 ceil(n / 64) rows of pitch >= p doubles and the rows from n on are written as
 * zeros: the layout the Gram kernels read.  n = 0 is a no-op.  For tests and callers that want the
 * factors.  No reference counterpart. */
int obhip_product_side_dev(const obhip_model *m, const obhip_terms *t, const uint32_t *dims_b,
                           uint64_t ndims_b, int side, const double *d_x, uint64_t n,
                           double *d_out, uint64_t pitch);
/* host only: used columns of each side and whether the staging kernel keeps that side's tile in LDS
 * (any pointer may be NULL).  No reference counterpart. */
int obhip_product_fit_layout(const obhip_terms *t, const uint32_t *dims_b, uint64_t ndims_b,
                             uint64_t *mu_a, uint64_t *mu_b, int *fused_a, int *fused_b);

/* ---- predictor ---------------------------------------------------------- */
/* predictor$update(x) + $mean() (+ $var() of pred_gauss):
 * loglik_gauss.cpp:214-227, loglik_std.cpp:239-248.  The basis at xnew is
 * evaluated and contracted with theta in one fused kernel; it is never
 * written to HBM.  d_coeffvar (p) may be NULL; then d_var is untouched;
 * otherwise var = B^2 coeffvar + e^{2 sigma}. */
int obhip_predict_dev(const obhip_model *m, const obhip_terms *t,
                      const double *d_theta, const double *d_x, uint64_t n,
                      double *d_mean, const double *d_coeffvar, double sigma,
                      double *d_var);
int obhip_predict(const obhip_model *m, const obhip_terms *t,
                  const double *theta, const double *x, uint64_t n,
                  uint64_t ldx, double *mean, const double *coeffvar,
                  double sigma, double *var);
/* Gradients of the predictive mean and variance by the inputs, at new rows.  The reference has no
 * counterpart.  With R_l = cov_l(x_l, knots_l) . rotmat_l, R'_l = (dcov_l / dx_l) . rotmat_l and, per
 * row, s = prod_l R_l0, r_lt = R_lt / R_l0, rho_l = R'_l0 / R_l0, r'_lt = (R'_lt - r_lt R'_l0) / R_l0,
 * P_k = prod_{l: t_kl > 0} r_l,t_kl and E_kl = P_k without dimension l's factor (a product, never a
 * quotient):
 *   mean       = s sum_k theta_k P_k
 *   dmean/dx_l = s (rho_l sum_k theta_k P_k + sum_{k: t_kl > 0} theta_k E_kl r'_l,t_kl)
 *   var        = s^2 sum_k c_k P_k^2 + e^{2 sigma}
 *   dvar/dx_l  = 2 s^2 (rho_l sum_k c_k P_k^2 + sum_{k: t_kl > 0} c_k P_k E_kl r'_l,t_kl)
 * dcov/dx, with h2 = h (1 + |h|) e^{-|h|} and w = (1 + h) e^{-h}:
 *   mat25     u = x / e^{2 th0}, h = u - u_knot:                    -(1/3) h2 / e^{2 th0}
 *   mat25pow  a = e^{th1/4}, t = x^a / e^{2 th0 + th1/4}, h = t - t_knot:   -(1/3) h2 a t / x
 *   mat25ang  hs = (sin x - sin k) / e^{2 th0}, hc = (cos x - cos k) / e^{2 th1}, h = sqrt(hs^2 + hc^2):
 *             -(1/3) w (hs cos x / e^{2 th0} - hc sin x / e^{2 th1})   -- nothing divides by h
 * One fused kernel per call; neither the basis nor its derivative is written to HBM while the
 * terms use at most 8 factors and 2 Mu + d + 31 <= 320 (Mu used basis columns).  Beyond that, and
 * under OBHIP_FORCE_GENERIC, the same contraction runs from a pooled HBM tile per block (any term
 * set obhip_predict_dev accepts).  No atomics: two calls give the same bits.
 * d_grad, d_gradvar: n x d column-major, ld = n (the layout of d_x).  d_mean may be NULL.
 * d_coeffvar (p) NULL: d_var and d_gradvar are untouched (d_gradvar without d_coeffvar is an
 * error); with it each of d_var (n) and d_gradvar may be NULL.  n = 0 is a no-op; at most 2^40
 * rows per call.  Argument errors return OBHIP_ERR_INVALID before any device call. */
int obhip_predict_grad_dev(const obhip_model *m, const obhip_terms *t, const double *d_theta,
                           const double *d_x, uint64_t n, double *d_mean, double *d_grad,
                           const double *d_coeffvar, double sigma, double *d_var, double *d_gradvar);
/* the same on host buffers: x n x d with ldx, grad / gradvar n x d with ldg */
int obhip_predict_grad(const obhip_model *m, const obhip_terms *t, const double *theta, const double *x,
                       uint64_t n, uint64_t ldx, double *mean, double *grad, uint64_t ldg,
                       const double *coeffvar, double sigma, double *var, double *gradvar);
/* the terms that have dimension dim (0-based) at a level > 0, in term order: what the gradient by
 * x_dim sums over beside the dense part.  *count always; terms_out (count entries) may be NULL.
 * Host only. */
int obhip_terms_dimview(const obhip_terms *t, uint64_t dim, uint64_t *count, uint32_t *terms_out);
/* Jacobian and vector-Jacobian product of the predictor of q responses that share the model and the
 * terms (obhip_predict_multi_dev).  The reference has no counterpart.  In the notation of
 * obhip_predict_grad_dev, for response j with the coefficients Theta[:, j]:
 *   mean_ij        = s_i sum_k Theta_kj P_k(i)
 *   dmean_ij/dx_l  = s_i (rho_l(i) sum_k Theta_kj P_k(i) + sum_{k: t_kl > 0} Theta_kj E_kl(i) r'_l,t_kl(i))
 *   vjp_il         = sum_j W_ij dmean_ij/dx_l
 * P_k, E_kl, r', rho_l and s do not depend on j: for q >= 2 one fused kernel evaluates the basis and
 * its derivative once per 64-row tile, forms every product once and contracts it with a 4 x 16 slice
 * of Theta on the matrix cores, responses in blocks of 16 and chunks of at most 64 per launch.  The
 * VJP comes from the same kernel, which contracts each finished 64 x (responses of the chunk) block
 * with the tile's rows of W before it leaves the chip: the n x d x q Jacobian is never written, not
 * even as scratch.  q = 1 takes the kernel of obhip_predict_grad_dev and gives exactly its bits.
 * Fused while the padded width of the terms is even and the tile of 2 Mu - 1 + d columns plus the
 * staged block fits 160 KB of LDS; beyond that and under OBHIP_FORCE_GENERIC one
 * obhip_predict_grad_dev pass per response (any term set it accepts), the VJP accumulated as
 * out += W[:, j] o grad_j with one fma per entry, in response order, from n d doubles of pooled
 * scratch.  No atomics and a fixed summation order on both paths: two calls give the same bits, and
 * the bits of d_mean and d_jac do not depend on which optional outputs are passed.
 * d_Theta: p x q column-major, ld = p.  d_x: n x d column-major, ld = n.  d_mean: n x q column-major,
 * ld = n, may be NULL.  d_jac (required): jac[(j d + l) n + i] = dmean_ij/dx_l.  d_W: n x q
 * column-major, ldw >= n (the padding is not read).  d_out (required): n x d column-major, ld = n.
 * A null m, t, d_Theta, d_x, d_jac / d_W / d_out, q = 0, ldw < n, n > 2^40 and terms of another
 * model's dimension count return OBHIP_ERR_INVALID before any device call; n = 0 is a no-op. */
int obhip_predict_jac_multi_dev(const obhip_model *m, const obhip_terms *t, const double *d_Theta,
                                uint64_t q, const double *d_x, uint64_t n, double *d_mean,
                                double *d_jac);
int obhip_predict_vjp_multi_dev(const obhip_model *m, const obhip_terms *t, const double *d_Theta,
                                uint64_t q, const double *d_x, uint64_t n, const double *d_W,
                                uint64_t ldw, double *d_mean, double *d_out);
/* the Jacobian on host buffers: Theta p x q (ld = p), x n x d with ldx, mean n x q (ld = n, may be
 * NULL), jac as d_jac */
int obhip_predict_jac_multi(const obhip_model *m, const obhip_terms *t, const double *Theta,
                            uint64_t q, const double *x, uint64_t n, uint64_t ldx, double *mean,
                            double *jac);
/* Hessian-vector and Jacobian-vector product of the multi-response predictor by the inputs, for one
 * direction per row (row i of V is v).  The reference has no counterpart.  Notation of
 * obhip_predict_grad_dev, per row, standardised units; with R''_l = (d2cov_l/dx_l^2) . rotmat_l
 *   kappa_l = R''_l0 / R_l0        r''_lt = (R''_lt - 2 r'_lt R'_l0 - r_lt R''_l0) / R_l0   (t >= 1)
 * d2cov/dx2, with k'(h) = -(1/3) h (1 + |h|) e^{-|h|} and k''(h) = -(1/3) (1 + |h| - h^2) e^{-|h|}:
 *   mat25     u = x / e^{2 th0}:                                       k''(h) / e^{4 th0}
 *   mat25pow  a = e^{th1/4}, t = x^a / e^{2 th0 + th1/4}, dt/dx = a t / x, d2t/dx2 = a (a - 1) t / x^2:
 *             k''(h) (dt/dx)^2 + k'(h) d2t/dx2
 *   mat25ang  cx = cos x / e^{2 th0}, sx = sin x / e^{2 th1}, q = hs cx - hc sx,
 *             q' = cx^2 + sx^2 - hs sin x / e^{2 th0} - hc cos x / e^{2 th1}:
 *             -(1/3) e^{-h} ((1 + h) q' - q^2)                         -- nothing divides by h
 * For response j with the coefficients Theta[:, j], E_klm = P_k without the factors of l and m:
 *   rho.v     = sum_l v_l rho_l
 *   S_j       = sum_k Theta_kj P_k
 *   Sd_j      = sum_k Theta_kj sum_{m: t_km > 0} v_m E_km r'_m,t
 *   g_lj      = sum_{k: t_kl > 0} Theta_kj E_kl r'_l,t
 *   h_lj      = sum_{k: t_kl > 0} Theta_kj (v_l E_kl r''_l,t + r'_l,t sum_{m != l: t_km > 0} v_m E_klm r'_m,t)
 *   mean_ij   = s S_j
 *   jvp_ij    = sum_l v_l dmean_ij/dx_l = s ((rho.v) S_j + Sd_j)
 *   (H_j v)_l = sum_m v_m d2mean_ij/dx_l dx_m
 *             = s ((rho_l (rho.v) + v_l (kappa_l - rho_l^2)) S_j + rho_l Sd_j + (rho.v) g_lj + h_lj)
 *   hvp_il    = sum_j W_ij (H_j v)_l          vjp_il = sum_j W_ij s (rho_l S_j + g_lj)
 * Per (row, term) O(f) multiplies through products of (value, directional derivative) pairs; no d x d
 * block is formed.  One fused kernel per chunk of responses (blocks of 16, at most 32): per 32-row
 * tile the basis with both derivatives is evaluated once, S and Sd come from one dense pass and
 * (rho.v) g_l + h_l (and g_l when d_vjp is passed) from one pass per dimension over its view, all
 * contracted with Theta on the matrix cores; each finished block is contracted with the tile's rows of
 * W in response order before it leaves the chip.  Neither the Jacobian nor any n x d x q or n x d x d
 * array is written, not even as scratch; q = 1 takes the same kernel.  Fused while the tile of
 * 3 Mu + 3 d columns of 33 doubles, eight blocks of 16 x 33 doubles, 18 x 32 doubles and Mu ints fit
 * 160 KB of LDS (obhip_predict_hvp_layout); beyond that and under OBHIP_FORCE_GENERIC the same
 * contraction runs from a pooled HBM tile per block (any term set obhip_predict_grad_dev accepts).  No
 * atomics and one summation order: two calls give the same bits, and the bits of an output do not
 * depend on which optional outputs are passed.
 * d_Theta: p x q column-major, ld = p.  d_x, d_V, d_vjp, d_hvp: n x d column-major, ld = n.  d_mean,
 * d_jvp: n x q column-major, ld = n.  d_W: n x q column-major, ldw >= n (the padding is not read),
 * required when d_vjp or d_hvp is passed.  d_mean and d_vjp may be NULL; at least one of d_jvp and
 * d_hvp is required.  A null m, t, d_Theta, d_x or d_V, q = 0, ldw < n, n > 2^40, neither d_jvp nor
 * d_hvp, d_vjp or d_hvp without d_W and terms of another model's dimension count return
 * OBHIP_ERR_INVALID before any device call, nothing written; n = 0 is a no-op.  Runs on the stream
 * of obhip_set_stream. */
int obhip_predict_hvp_multi_dev(const obhip_model *m, const obhip_terms *t, const double *d_Theta,
                                uint64_t q, const double *d_x, uint64_t n, const double *d_W,
                                uint64_t ldw, const double *d_V, double *d_mean, double *d_vjp,
                                double *d_jvp, double *d_hvp);
/* the same on host buffers: x with ldx, W with ldw, the n x d arrays V, vjp and hvp with ldg, mean
 * and jvp n x q with ld = n */
int obhip_predict_hvp_multi(const obhip_model *m, const obhip_terms *t, const double *Theta, uint64_t q,
                            const double *x, uint64_t n, uint64_t ldx, const double *W, uint64_t ldw,
                            const double *V, uint64_t ldg, double *mean, double *vjp, double *jvp,
                            double *hvp);
/* what obhip_predict_hvp_multi_dev will do with these terms and q responses: the used basis columns,
 * the rows of a tile (32), the LDS bytes of a workgroup of the first launch and whether the tile
 * lives in LDS (1) or in pooled HBM scratch (0).  From the levels alone; every output may be NULL.
 * Host only. */
int obhip_predict_hvp_layout(const obhip_terms *t, uint64_t q, uint64_t *mu, uint64_t *tile_rows,
                             uint64_t *lds_bytes, int *fused);
/* predr_std (loglik_std.cpp:218-256), the predictor of the loglik_std model with the full
 * posterior covariance of the coefficients: mean = B theta, var_i = b_i^T inv(H) b_i +
 * e^{2 sigma} (:249-256; the reference uses arma::inv; here H = L L^T by the library's own
 * Cholesky, X = L^-T by a blocked triangular inversion and || L^-1 b_i ||^2 in one pass of the
 * matrix-core kernel, csrc/posterior.cpp -- no BLAS library is involved).  H: total Hessian,
 * p x p symmetric (host); var may be NULL (then H may be too). */
int obhip_predict_std(const obhip_model *m, const obhip_terms *t, const double *theta,
                      const double *H, const double *x, uint64_t n, uint64_t ldx, double *mean,
                      double sigma, double *var);

/* Marginal adjustment of lpdfvec(loglik_std, logpr_gauss) with the full Hessian
 * (lpdfvec::buildhess, fit.cpp:270-299): val = -1/2 log det H, gradhyp[l] =
 * -1/2 sum(dH/dhyp_l % inv(H)) (nhyp entries) and gradpara = {noisescale, coeffscale}
 * parts (loglik_std.cpp:180-203, logpr_gauss.cpp:165-186).  H: total Hessian (host);
 * gradhyp / gradpara may be NULL.  inv(H) = L^-T L^-1 on the library's own kernels, like
 * obhip_predict_std. */
int obhip_margadj_full(const obhip_basis *b, const obhip_terms *t, const obhip_model *m,
                       const double *H, double sigma, double rho, double *val, double *gradhyp,
                       double *gradpara);

/* ---- posterior handle and sequential design (no reference counterpart) -------------------
 * An obhip_posterior owns, for one model and term set, the total Hessian H (p x p), its factor
 * H = L L^T with X = L^-T, and sigma.  All variances are in standardised units, without the noise
 * e^{2 sigma} unless asked for.  d_x is column-major n x d (leading dimension n), on the device.
 * Every argument check runs before the first launch and a refused call changes nothing; a Hessian
 * that is not positive definite is OBHIP_ERR_NUMERIC, as the other solve entries report it (the
 * create entries wait for their factorisation).
 * The explicit S = inv(H) = X X^T (pad128(p)^2 doubles, pad128(p) = p rounded up to 128) is formed
 * by the handle's first design, acquisition or gradient call (obhip_design_select*, obhip_acquire*,
 * obhip_posterior_var_grad_dev, obhip_acquire_grad*) and stays on the handle until it is destroyed;
 * the selection entries downdate a copy of their own, the handle's S is never written again. */
/* d_H: symmetric p x p on the device, copied */
int obhip_posterior_create_dev(obhip_posterior **out, const obhip_model *m, const obhip_terms *t,
                               const double *d_H, double sigma);
int obhip_posterior_destroy(obhip_posterior *post);
/* p, sigma and log det H = 2 sum log L_kk; any pointer may be NULL */
int obhip_posterior_info(const obhip_posterior *post, uint64_t *p, double *sigma, double *logdet);
/* H formed exactly as obhip_normal_acc_solve_dev forms it: e^{-2 sigma} (T - T_minus) + diag(prec);
 * minus may be NULL.  Neither accumulator is written. */
int obhip_normal_acc_posterior_dev(const obhip_normal_acc *acc, const obhip_normal_acc *minus,
                                   double sigma, double rho, obhip_posterior **out);
/* d_var[i] = b_i^T inv(H) b_i (+ e^{2 sigma} when with_noise) at the n rows of d_x; n = 0: no-op */
int obhip_posterior_var_dev(const obhip_posterior *post, const double *d_x, uint64_t n,
                            double *d_var, int with_noise);
/* *out = a NEW handle for H + e^{-2 sigma} B^T B of the n rows of d_x (the Gram kernels): the
 * posterior once the simulator has been run at those rows, whatever it returns. */
int obhip_posterior_condition_dev(const obhip_posterior *post, const double *d_x, uint64_t n,
                                  obhip_posterior **out);

/* Greedy sequential design over m candidate rows d_xcand (column-major m x d).  With nu =
 * e^{2 sigma}, d_i = b_i^T inv(H) b_i and a run at j taking H to H + b_j b_j^T / nu:
 *   OBHIP_DESIGN_MAXVAR  picks argmax w_i d_i (greedy D-optimality: log det H grows by
 *                        log(1 + d_j / nu)); score = w_j d_j, trace[t] = the cumulative gain;
 *   OBHIP_DESIGN_IMSE    picks argmax w_i num_i / (nu + d_i), num_i = b_i^T S M S b_i, S = inv(H),
 *                        M = sum_r u_r b_r b_r^T / sum u over the r reference rows d_xref
 *                        (column-major r x d): the drop of the integrated variance tr(M S);
 *                        score = that weighted drop, trace[t] = tr(M S_t).
 * After every pick S, d and num are downdated by the rank-one formulas: per
 * step the candidates are passed over once, in one kernel, and the host waits for the device once.
 * The lowest index wins a tie; a candidate that is already picked (replace = 0), has weight 0 or
 * a score that is not finite is never picked.  d_weights (m) and d_uref (r) may be NULL: all ones;
 * d_xref, r, d_uref are ignored for MAXVAR.  Out: d_index (k, int64) and d_score (k), of which
 * *n_picked are written -- fewer than k when no eligible candidate is left, which is no error --
 * d_var (m, may be NULL): d_i after all picks; d_trace (k + 1, may be NULL): entries 0 .. *n_picked.
 * No atomics anywhere: two calls give the same bits.  u with a negative or non-finite entry or
 * without mass: OBHIP_ERR_NUMERIC. */
#define OBHIP_DESIGN_MAXVAR 0
#define OBHIP_DESIGN_IMSE 1
int obhip_design_select_dev(const obhip_posterior *post, const double *d_xcand, uint64_t m,
                            int criterion, const double *d_xref, uint64_t r, const double *d_uref,
                            const double *d_weights, uint64_t k, int replace, int64_t *d_index,
                            double *d_score, double *d_var, double *d_trace, uint64_t *n_picked);
/* the same on host buffers; xcand m x d and xref r x d column-major with leading dimensions m, r */
int obhip_design_select(const obhip_posterior *post, const double *xcand, uint64_t m, int criterion,
                        const double *xref, uint64_t r, const double *uref, const double *weights,
                        uint64_t k, int replace, int64_t *index, double *score, double *var,
                        double *trace, uint64_t *n_picked);

/* ---- posterior draws (no reference counterpart) -------------------------------------------
 * The posterior of the coefficients of one response is N(theta, inv(H)), so with z_s ~ N(0, I_p)
 * the draw Theta[:, s] = theta + L^-T z_s has exactly that law; its sample path at row i is
 * b_i^T Theta[:, s].  The library contains no random number generator: the caller supplies the
 * normals d_z, column-major p x S with leading dimension ldz >= p.  d_theta (p) is the posterior
 * mean of one response; everything is in standardised units.  The rules of the posterior block
 * hold: every argument check runs before the first launch, a refused call changes nothing.  No
 * atomics anywhere and one fixed order of summation: two calls give the same bits.
 *
 * draw      d_Theta (p x S, leading dimension p): Theta_ks = theta_k + sum_{j >= k} X_kj z_js from the
 *           handle's resident X = L^-T, j ascending, theta added last.
 * sample    d_path (n x S, leading dimension n) = B(d_x) Theta: the multi-response predictor's
 *           batched pass on the drawn coefficients (its bits); n = 0: no-op.
 * extremum  per draw s the row of d_xcand (column-major m x d) with the smallest path value
 *           (maximize != 0: the largest) and that value, the m x S paths never stored.  The lowest
 *           index wins among equal values (-0.0 and 0.0 are equal).  A candidate with d_skip[i] != 0
 *           (d_skip may be NULL), a coordinate that is not finite or a value that is not finite is
 *           never chosen; a draw without an eligible candidate gets index -1 and value NaN, which
 *           is no error.  The values carry the bits sample gives the same rows. */
int obhip_posterior_draw_dev(const obhip_posterior *post, const double *d_theta,
                             const double *d_z, uint64_t ldz, uint64_t S,
                             double *d_Theta /* p x S, ld = p */);
int obhip_posterior_sample_dev(const obhip_posterior *post, const double *d_theta,
                               const double *d_z, uint64_t ldz, uint64_t S,
                               const double *d_x, uint64_t n,
                               double *d_path /* n x S, ld = n */);
int obhip_posterior_extremum_dev(const obhip_posterior *post, const double *d_theta,
                                 const double *d_z, uint64_t ldz, uint64_t S,
                                 const double *d_xcand, uint64_t m,
                                 const uint8_t *d_skip /* m or NULL */, int maximize,
                                 int64_t *d_index /* S */, double *d_value /* S */);

/* ---- acquisition picks (no reference counterpart) -----------------------------------------
 * k of the m candidate rows d_xcand (column-major m x d), picked one after the other by a criterion
 * of the latent mean mu_i = b_i^T theta and the latent variance d_i = b_i^T inv(H) b_i (without the
 * noise; sd = sqrt(max(d, 0))), all in standardised units.  Written for minimisation; maximize != 0
 * applies the same to -mu, -best, -level and -lie_value.  With t = best - xi - mu, u = t / sd:
 *   OBHIP_ACQ_EI        t Phi(u) + sd phi(u)            (sd = 0: max(t, 0))   expected improvement
 *   OBHIP_ACQ_PI        Phi(u)                          (sd = 0: t > 0)       probability of improvement
 *   OBHIP_ACQ_LCB       kappa sd - mu                                         confidence bound
 *   OBHIP_ACQ_STRADDLE  kappa sd - |mu - level|                               contour f = level
 * params (host, 4 doubles): best, xi, kappa, level; what a criterion does not use is not looked at,
 * except that xi must be finite and kappa finite and >= 0 always.  The largest score is picked, the
 * lowest index among equal scores (EI and PI underflow to exact zeros far from the incumbent).  A
 * candidate with d_skip[i] != 0 (d_skip may be NULL), one that is picked already, one with a
 * coordinate that is not finite or a score that is not finite is never picked.  After pick j the
 * run there is given a value y* without being made -- OBHIP_LIE_BELIEVER: y* = mu_j, the mean does
 * not move; OBHIP_LIE_CONSTANT: y* = lie_value -- and with s = inv(H) b_j, gamma = e^{2 sigma} + b_j^T s,
 * a_i = b_i^T s every candidate's mu_i += a_i (y* - mu_j) / gamma, d_i -= a_i^2 / gamma; for EI and PI
 * best becomes min(best, y*).  Per pick the candidates are passed over by the one-response
 * predictor and one update kernel, and the host waits for the device once.
 * d_theta (p): the standardised coefficients of one response.  Out: d_index (k, int64) and d_score
 * (k), of which *n_picked are written -- fewer than k when no eligible candidate is left, which is
 * no error; d_score0 (m, may be NULL): every candidate's score at the first step, eligible or not;
 * d_mean, d_var (m each, may be NULL): mu_i and d_i after all fantasies.  No atomics anywhere: two
 * calls give the same bits.  The rules of the posterior block hold: every argument check runs
 * before the first launch and a refused call changes nothing. */
enum { OBHIP_ACQ_EI = 0, OBHIP_ACQ_PI = 1, OBHIP_ACQ_LCB = 2, OBHIP_ACQ_STRADDLE = 3 };
enum { OBHIP_LIE_BELIEVER = 0, OBHIP_LIE_CONSTANT = 1 };
int obhip_acquire_dev(const obhip_posterior *post, const double *d_theta, const double *d_xcand,
                      uint64_t m, int criterion, const double *params /* host: best, xi, kappa, level */,
                      int maximize, int lie, double lie_value, const uint8_t *d_skip /* m or NULL */,
                      uint64_t k, int64_t *d_index, double *d_score, double *d_score0,
                      double *d_mean, double *d_var, uint64_t *n_picked);
/* the same on host buffers; xcand m x d column-major with leading dimension m */
int obhip_acquire(const obhip_posterior *post, const double *theta, const double *xcand, uint64_t m,
                  int criterion, const double *params, int maximize, int lie, double lie_value,
                  const uint8_t *skip, uint64_t k, int64_t *index, double *score, double *score0,
                  double *mean, double *var, uint64_t *n_picked);

/* ---- acquisition over several responses (no reference counterpart) -------------------------
 * The picks of obhip_acquire_dev for q responses fitted from one Gram and one factor: d_Theta (p x q,
 * leading dimension p) holds their standardised coefficients.  They share H, hence the latent variance
 * d_i and the downdate vector a_i, and given the data their coefficient posteriors are independent:
 * feasibility probabilities multiply and a pick still costs one pass of the one-response predictor.
 * Per response r (host arrays of q entries): roles[r] OBHIP_ROLE_OBJECTIVE, _CONSTRAINT or _NONE
 * (carried along, not scored); signs[r] = +1 or -1 (an objective: -1 maximises; a constraint:
 * +1 is f_r <= limits[r], -1 is f_r >= limits[r]); limits[r]: a constraint's limit, the incumbent of the
 * CEI / CPI objective (signs[r] * limits[r] finite or +inf: "no feasible run yet"), the reference
 * coordinate of an EHVI objective (finite).  With ms_r = signs[r] mu_r, cs_r = signs[r] limits[r],
 * Psi(c; ms, d) = OBHIP_ACQ_EI's score at best = c, xi = 0 and P(c; ms, d) = OBHIP_ACQ_PI's likewise
 * (both with their sd = 0 branches):
 *   pof = prod over the constraints, ascending r from 1.0, of P(cs_r; ms_r, d)
 *   OBHIP_MACQ_CEI   one objective   EI(ms, d, best, xi) pof; while best = +inf: pof
 *   OBHIP_MACQ_CPI   one objective   PI(ms, d, best, xi) pof; likewise
 *   OBHIP_MACQ_POF   no objective, at least one constraint   pof
 *   OBHIP_MACQ_EHVI  two objectives (1) and (2) in response order, reference point (cs_(1), cs_(2)):
 *                    the expected improvement of the hypervolume the front dominates inside the box,
 *                    pof sum_{s=1..F+1} [Psi(u_s; ms_1, d) - Psi(u_{s-1}; ms_1, d)] Psi(c_s; ms_2, d),
 *                    u_1 < .. < u_F the front's first coordinates, u_{F+1} = r1, Psi(u_0) = 0, c_1 = r2,
 *                    c_{s+1} the second coordinate of front point s; the strips are summed in ascending s.
 * front0 (host, F0 x 2 row-major pairs in the caller's sign, any order, finite; EHVI only) is
 * normalised point by point by the front rule: a point not strictly inside the box or with a front
 * point <= it in both signed coordinates changes nothing; otherwise every front point >= it in both
 * leaves and it is inserted in order.  After pick j every response gets a value -- OBHIP_LIE_BELIEVER:
 * y*_r = mu_jr; OBHIP_LIE_CONSTANT: y*_r = lie_value[r] (host, q finite entries) -- and with gamma and a_i
 * of obhip_acquire_dev mu_ir += a_i (y*_r - mu_jr) / gamma for every r and d_i -= a_i^2 / gamma once.  The
 * pick is believed feasible when signs[r] y*_r <= cs_r for every constraint; only then CEI / CPI take
 * best = min(best, signs y*_obj) and EHVI enters the signed point into the front by the same rule.
 * Tie rule, eligibility, d_skip and non-finite scores are obhip_acquire_dev's; one host wait per pick;
 * no atomics: two calls give the same bits.  q = 1, CEI without a constraint and a finite incumbent
 * returns the bits of obhip_acquire_dev with OBHIP_ACQ_EI (CPI: OBHIP_ACQ_PI).
 * Out: d_index, d_score (k), *n_picked as obhip_acquire_dev; d_score0, d_pof0 (m, may be NULL): the
 * score and the feasibility factor at the first step; d_mean (m x q, leading dimension m) and d_var (m)
 * after all fantasies (may be NULL); front_out (host, 2 (F0 + k) doubles, pairs in the caller's sign,
 * ascending in the signed first coordinate) with *n_front, and *best_out (the final incumbent of CEI /
 * CPI in the caller's sign), each may be NULL.  Refused with OBHIP_ERR_INVALID before any device call:
 * q outside 1 .. 16, a number of objectives the criterion does not take, F0 + k > 2048, a reference
 * point, xi, front point or lie value that is not finite, an incumbent that is neither finite nor +inf
 * in the signed sense.  The rules of the posterior block hold. */
enum { OBHIP_MACQ_CEI = 0, OBHIP_MACQ_CPI = 1, OBHIP_MACQ_POF = 2, OBHIP_MACQ_EHVI = 3 };
enum { OBHIP_ROLE_OBJECTIVE = 0, OBHIP_ROLE_CONSTRAINT = 1, OBHIP_ROLE_NONE = 2 };
int obhip_acquire_multi_dev(const obhip_posterior *post, const double *d_Theta, uint64_t q,
                            const double *d_xcand, uint64_t m, int criterion, const int32_t *roles,
                            const double *signs, const double *limits, double xi,
                            const double *front0, uint64_t F0, int lie, const double *lie_value,
                            const uint8_t *d_skip /* m or NULL */, uint64_t k, int64_t *d_index,
                            double *d_score, double *d_score0, double *d_pof0, double *d_mean,
                            double *d_var, double *front_out, uint64_t *n_front, double *best_out,
                            uint64_t *n_picked);
/* the same on host buffers; Theta p x q with leading dimension p, xcand m x d column-major with leading
 * dimension m, mean m x q with leading dimension m */
int obhip_acquire_multi(const obhip_posterior *post, const double *Theta, uint64_t q, const double *xcand,
                        uint64_t m, int criterion, const int32_t *roles, const double *signs,
                        const double *limits, double xi, const double *front0, uint64_t F0, int lie,
                        const double *lie_value, const uint8_t *skip, uint64_t k, int64_t *index,
                        double *score, double *score0, double *pof0, double *mean, double *var,
                        double *front_out, uint64_t *n_front, double *best_out, uint64_t *n_picked);
/* host only: *lds_bytes = the LDS of one workgroup of the update kernel for q responses, this criterion
 * and a front of at most front_cap (= F0 + k) points; *max_q = 16, *max_front = 2048.  q, criterion or
 * front_cap outside those limits are refused.  Any pointer may be NULL. */
int obhip_acquire_multi_layout(uint64_t q, int criterion, uint64_t front_cap, uint64_t *lds_bytes,
                               uint64_t *max_q, uint64_t *max_front);

/* ---- acquisition gradients (no reference counterpart) --------------------------------------
 * The latent variance d_i = b_i^T inv(H) b_i (the full posterior covariance, what the design and
 * acquisition entries score with), the latent mean mu_i = b_i^T theta, an acquisition criterion and
 * the gradients of all three by the inputs, at the n rows d_x (column-major n x d), in standardised
 * units: what moves a point continuously to where a criterion is best.  Gradients are column-major
 * n x d with leading dimension n.  With S = inv(H), b_ik = s_i P_ik (s_i the row scale, P_ik the
 * term product; the names of obhip_predict_grad_dev), t_i = S b_i, rho_l = R'_l0 / R_l0, E_kl the
 * product of term k's columns other than that of dimension l and r'_l,t that column's derivative:
 *   d_i         = s sum_k t_ik P_k
 *   dd_i/dx_l   = 2 s (rho_l sum_k t_ik P_k + sum_{k has l} t_ik E_kl r'_l,t)      (S is symmetric)
 *   dmu_i/dx_l  =   s (rho_l sum_k theta_k P_k + sum_{k has l} theta_k E_kl r'_l,t)
 * and with sd = sqrt(max(d, 0)), dsd = dd / (2 sd), mu~ = mu (maximize != 0: -mu, with -best and
 * -level, as obhip_acquire_dev), t = best - xi - mu~, u = t / sd:
 *   OBHIP_ACQ_EI        score t Phi(u) + sd phi(u)       gradient -Phi(u) dmu~ + phi(u) dsd
 *   OBHIP_ACQ_PI        score Phi(u)                     gradient phi(u) (-dmu~ - u dsd) / sd
 *   OBHIP_ACQ_LCB       score kappa sd - mu~             gradient kappa dsd - dmu~
 *   OBHIP_ACQ_STRADDLE  score kappa sd - |mu~ - level|   gradient kappa dsd - sign(mu~ - level) dmu~
 * with sign(0) = 0.  Where d <= 0: dsd = 0 and the scores are obhip_acquire_dev's sd = 0 branches, so
 * the EI gradient is -dmu~ where t > 0 and 0 elsewhere and the PI gradient is 0.  A row with a
 * coordinate that is not finite gets NaN in every output.  criterion and params (host: best, xi,
 * kappa, level) are obhip_acquire_dev's, checked as there.
 *
 * inv(H) is formed by the first of these calls on a handle (as the design and acquisition entries
 * form theirs on every call), kept on the handle and freed with it; a handle from
 * obhip_posterior_condition_dev starts without one.  The rows are taken in chunks: per chunk the
 * stored product Y = S B^T (term-major, in pooled scratch, every entry summed in one fixed order) and
 * one fused kernel pass (csrc/kernels_acquire_dx.hip).  chunk_rows bounds the workspace -- two blocks
 * of pad128(p) x chunk_rows doubles: 0 = the library's choice (at most 1 GiB per block), otherwise a
 * positive multiple of 128; anything else is refused.  No atomics anywhere and a summation order that
 * does not depend on where a row stands: two calls give the same bits, a chunked call the bits of the
 * unchunked one, bit-identical rows bit-identical results.  The rules of the posterior block hold:
 * every argument check runs before the first launch and a refused call changes nothing; n = 0 is a
 * no-op; p <= 65535 and n <= 2^40.
 *
 * var_grad  d_var (n) = d_i (+ e^{2 sigma} when with_noise) and d_gradvar (n x d) = dd_i/dx_l; no
 *           theta, no criterion.  Both required. */
int obhip_posterior_var_grad_dev(const obhip_posterior *post, const double *d_x, uint64_t n,
                                 uint64_t chunk_rows, int with_noise, double *d_var,
                                 double *d_gradvar);
/* d_theta (p): the standardised coefficients of one response.  d_score (n) and d_gradscore (n x d)
 * are required; d_mean (n) = mu, d_gradmean (n x d) = dmu/dx (of mu, not of mu~), d_var (n) = d
 * without the noise and d_gradvar (n x d) = dd/dx may each be NULL: not wanted, not written. */
int obhip_acquire_grad_dev(const obhip_posterior *post, const double *d_theta, const double *d_x,
                           uint64_t n, int criterion,
                           const double *params /* host: best, xi, kappa, level */, int maximize,
                           uint64_t chunk_rows, double *d_score, double *d_gradscore,
                           double *d_mean, double *d_gradmean, double *d_var, double *d_gradvar);
/* the same on host buffers; x and every gradient n x d column-major with leading dimension n */
int obhip_acquire_grad(const obhip_posterior *post, const double *theta, const double *x, uint64_t n,
                       int criterion, const double *params, int maximize, uint64_t chunk_rows,
                       double *score, double *gradscore, double *mean, double *gradmean,
                       double *var, double *gradvar);
/* which kernel the two entries above run on this handle's terms: *fused = 1 the tile in LDS
 * (*lds_bytes of it per workgroup), 0 the tile in pooled scratch (more than 8 factors per term, a
 * tile beyond the LDS, or OBHIP_FORCE_GENERIC); *default_chunk_rows = what chunk_rows = 0 stands for.
 * Any pointer may be NULL. */
int obhip_acquire_grad_layout(const obhip_posterior *post, int *fused, uint64_t *lds_bytes,
                              uint64_t *default_chunk_rows);

/* ---- term-count path (no reference counterpart) --------------------------------------------
 * The terms of a handle stand in list order (selectterms: by prior variance), so the model of the
 * first k terms has H_k = H[:k,:k] with factor L_k = L[:k,:k]: the factor of the whole list nests
 * every prefix.  With G = e^{-2 sigma} B^T y (y standardised), U = L^-1 G = X^T G and, at a row with
 * basis b, z = X^T b (z_j depends on b_1 .. b_j only):
 *   theta_k = X[:k,:k] U[:k],   mean_k = sum_{j <= k} z_j U_j,   v_k = b_k^T inv(H_k) b_k = sum_{j <= k} z_j^2,
 *   log p(y | k) = -(n/2) log 2 pi - n sigma - 1/2 e^{-2 sigma} y^T y
 *                  + 1/2 sum_{j <= k} U_j^2 - sum_{j <= k} log L_jj + 1/2 sum_{j <= k} log prec_j.
 * Checkpoints are k_c = min((c + 1) step, p), c = 0 .. K - 1, K = ceil(p / step); step >= p gives the
 * one checkpoint k = p.  Row scores per checkpoint and response are sums over the n given rows, with
 * nu = e^{2 sigma}, r = y - mean_k, h = v_k / nu:
 *   loo = 0 (rows not in the fit):        e = r,           s2 = nu + v_k
 *   loo = 1 (rows of the fit, each once): e = r / (1 - h), s2 = nu / (1 - h)
 *   sse = sum r^2,  spe = sum e^2,  lpd = sum [-1/2 log(2 pi s2) - 1/2 e^2 / s2],  sumv = sum v_k.
 * No row is left out of any sum and a row that is not finite propagates as the formulas say.  The
 * leave-one-out scores hold the standardisation of the response (centre and scale) fixed: the row left
 * out still counts in them.  One factor and one pass over the rows give every prefix: per row chunk the
 * stored product Z = B X (the pass of obhip_posterior_var_dev, every entry summed in one fixed order)
 * and one kernel that walks a row's columns in ascending order (csrc/kernels_term_path.hip).  No
 * atomics: rows are summed per 128-row tile in a fixed order and tiles in ascending order in groups
 * whose size does not depend on the chunking, so two calls give the same bits and a chunked call the
 * bits of the unchunked one.  chunk_rows: 0 = the library's choice, otherwise a positive multiple of 128.
 * The rules of the posterior block hold: every argument check runs before the first launch and a
 * refused call changes nothing.  q <= 65534, p <= 65535, n <= 2^40. */
/* K, the rows of a chunk that chunk_rows stands for and the bytes of pooled scratch a scores call
 * takes (Z, the tile partials and the group sums); any output may be NULL.  Host only. */
int obhip_term_path_layout(uint64_t p, uint64_t q, uint64_t step, uint64_t n, uint64_t chunk_rows,
                           uint64_t *K, uint64_t *chunk_rows_used, uint64_t *scratch_bytes);
/* G = e^{-2 sigma} B^T y_std (p x q, column-major) of the rows acc holds (minus those of minus), standardised
   exactly as obhip_normal_acc_solve_dev does; d_meansd q triples */
int obhip_normal_acc_rhs_dev(const obhip_normal_acc *acc, const obhip_normal_acc *minus, double sigma,
                             double *d_G, double *d_meansd);
/* d_diag (p) = the diagonal of the handle's H, copied: what obhip_normal_acc_solve_dev returns as d_diagH for
   a handle made by obhip_normal_acc_posterior_dev of the same rows, sigma and rho */
int obhip_posterior_hessian_diag_dev(const obhip_posterior *post, double *d_diag);
/* d_U (p x q, column-major) = X^T G: U_jc = sum_{i <= j} X_ij G_ic, i ascending */
int obhip_posterior_path_coef_dev(const obhip_posterior *post, const double *d_G, uint64_t q, double *d_U);
/* Theta_k = X[:k,:k] U[:k]: Theta_ic = sum_{i <= j < k} X_ij U_jc, j ascending; zeros behind row k */
int obhip_posterior_path_theta_dev(const obhip_posterior *post, const double *d_U, uint64_t q, uint64_t k,
                                   double *d_Theta /* p x q */);
/* host in, host out: prec (p), yty (q, standardised), out K x q (out[c * q + j]); n_rows = the n of
 * the formula.  Host arithmetic over diag L, U and prec in one ascending order. */
int obhip_posterior_path_evidence(const obhip_posterior *post, const double *d_U, uint64_t q, const double *prec,
                                  const double *yty, uint64_t n_rows, uint64_t step, double *out);
/* d_Y n x q column-major (ldy); d_meansd NULL: Y is standardised already; d_scores K x q x 3 (sse, spe, lpd:
   d_scores[(c * q + j) * 3 + s]) in standardised units, d_sumv K; n = 0: zeros */
int obhip_posterior_path_scores_dev(const obhip_posterior *post, const double *d_U, uint64_t q, const double *d_x,
                                    uint64_t n, const double *d_Y, uint64_t ldy, const double *d_meansd,
                                    uint64_t step, int loo, uint64_t chunk_rows, double *d_scores, double *d_sumv);

/* ---- conditional moments (no reference counterpart) ----------------------------------------
 * The mean and the variance of the fitted mean over some inputs (the noise dimensions E) at fixed
 * values of the others (the control dimensions S, the complement of E), in closed form from the
 * moment tables of obhip_dim_moments_dev.  Notation of the sensitivity block and of
 * obhip_predict_grad_dev: f(x) = sum_k theta_k prod_l psi_{l,t_kl}(x_l), raw psi_l = R_l; tables m_l,
 * C_l, A_l = C_l + m_l m_l^T.  dims_e names E: 0-based, strictly ascending, 1 <= |E| <= d - 1 (the
 * convention of dims_b in the product block).  The noise inputs are independent and follow the
 * discrete product measure of the tables; only the tables of the dimensions in E are read.
 * For row i with control inputs x_i,S and response j:
 *   P_ik = prod_{l in S} R_{l,t_kl}(x_il)   (the A side of obhip_product_side_dev with dims_b = dims_e)
 *   M_ij = E[f_j | x_S]   = sum_k theta_kj P_ik prod_{l in E} m_l[t_kl]
 *   W_ij = Var[f_j | x_S] = sum_{k,k'} theta_kj theta_k'j P_ik P_ik'
 *                             sum_{l in E} (prod_{i in E, i<l} A_i) C_l (prod_{i in E, i>l} m_i m_i)
 * with the table entries at [t_kl, t_k'l]: the bracket prod A - prod m m is formed telescoped, as
 * obhip_sobol_dev forms V, never as a difference of two products.  Level 0 is not the constant
 * function: a term set whose terms all have level 0 on E still has a small positive variance.
 * The terms are grouped by their level tuples on E: G <= p groups, numbered in the order of their
 * first term, g(k) the group of term k.  With c_ij[g] = sum_{k in g} theta_kj P_ik (ascending k),
 * mE[g] = prod_{l in E} m_l[.] and K[g,g'] the bracket on the groups' tuples,
 *   M_ij = c_ij^T mE,   W_ij = c_ij^T K c_ij = sum_g c_ij[g] Y_ij[g],   Y_ij = K c_ij (g' ascending),
 * and for l in S, with rho_l, r'_lt and E_kl of obhip_predict_grad_dev restricted to S,
 *   dM_ij/dx_il = sum_k theta_kj mE[g(k)] dP_ik/dx_il,   dW_ij/dx_il = 2 sum_k theta_kj Y_ij[g(k)] dP_ik/dx_il.
 * A row costs O(p |S| + G^2), the G^2 part on the FP64 matrix cores; nothing of size n p exists
 * and the workspace is that of one row chunk.  Fixed summation order, no atomics: two calls give
 * the same bits, a chunked call those of the unchunked one, and each output requested alone the
 * bits it has when all are requested.  A row with a coordinate that is not finite gets NaN.
 * Refused with OBHIP_ERR_INVALID before any device call, nothing written: a NULL required
 * argument; dims_e unsorted, repeated, out of range, empty or naming all d dimensions; chunk_rows
 * not a multiple of 128 (or above 2^28); a level above 255, d above 255, q above 65535, p above 2^24
 * (the limits of the Sobol passes); tables of the noise dimensions beyond the LDS of a workgroup
 * (3 x 8 x (sum over E of L_l^2 + 1) bytes above 160 KB: only those tables are held); more than 2^31
 * (term, control dimension) pairs with a factor; n above 2^40 (that of
 * obhip_predict_grad_dev); more than 65535 used basis columns on S; more than 16384 groups.  n = 0
 * is a no-op. */
/* the number of groups, the group of every term (p entries, or NULL), the used columns of the S
 * side (the ones column included) and whether the row kernels keep the tile of S in LDS (at most 8
 * factors per term on S and a derivative tile within the LDS budget; otherwise, and under
 * OBHIP_FORCE_GENERIC, the same arithmetic runs from a pooled HBM tile).  Any output may be NULL.
 * Host only. */
int obhip_conditional_layout(const obhip_terms *t, const uint32_t *dims_e, uint64_t ndims_e, uint64_t *n_groups,
                             uint32_t *group_of, uint64_t *mu_s, int *fused);
/* d_mE (G) and d_K (G x G, leading dimension G): K is symmetric to the bit, every unordered pair of
 * groups is formed once and written to both places */
int obhip_conditional_tables_dev(const obhip_terms *t, const uint32_t *dims_e, uint64_t ndims_e,
                                 const double *d_mean_tab, const double *d_cov_tab, double *d_mE, double *d_K);
/* d_Theta p x q column-major; d_xs n x |S| column-major (leading dimension n), the columns in
 * ascending order of dimension -- what obhip_predict_product_dev takes for xa; d_mean, d_var n x q
 * column-major; d_gradmean, d_gradvar [(j |S| + a) n + i] for response j, the a-th dimension of S and
 * row i.  Any of the four outputs may be NULL.  chunk_rows: 0 = the library's choice, otherwise a
 * positive multiple of 128; it bounds the workspace and changes no bit of any output. */
int obhip_conditional_moments_dev(const obhip_model *m, const obhip_terms *t, const double *d_Theta, uint64_t q,
                                  const uint32_t *dims_e, uint64_t ndims_e, const double *d_mean_tab,
                                  const double *d_cov_tab, const double *d_xs, uint64_t n, uint64_t chunk_rows,
                                  double *d_mean, double *d_var, double *d_gradmean, double *d_gradvar);
/* host in, host out; xs with leading dimension ldx, the outputs compact as above */
int obhip_conditional_tables(const obhip_terms *t, const uint32_t *dims_e, uint64_t ndims_e, const double *mean_tab,
                             const double *cov_tab, double *mE, double *K);
int obhip_conditional_moments(const obhip_model *m, const obhip_terms *t, const double *Theta, uint64_t q,
                              const uint32_t *dims_e, uint64_t ndims_e, const double *mean_tab, const double *cov_tab,
                              const double *xs, uint64_t n, uint64_t ldx, uint64_t chunk_rows, double *mean,
                              double *var, double *gradmean, double *gradvar);

/* ---- the model layer: lpdf, loglik_*, logpr_gauss, lpdfvec, predictor ------------------
 * Module rows src/interfaceR.cpp:696-762; classes src/fit.h:23-361; arithmetic
 * src/fit.cpp:37-612 and src/lpdfs/{loglik_std,loglik_gauss,loglik_gda,logpr_gauss}.cpp.
 * One handle type for every descendant of class lpdf; y, yhat, the residuals and the
 * observation standard deviations of an object stay in HBM between calls, so a call moves
 * p-, nhyp- and npara-sized vectors only.  Objects reference each other like the C++
 * objects of the reference do (fit.h:133,153): the caller keeps the outermod alive as long
 * as a likelihood or prior built on it, and the two members as long as their lpdfvec. */
#define OBHIP_LPDF_LOGLIK_STD 0   /* class loglik_std,   src/lpdfs/loglik_std.cpp:41-203 */
#define OBHIP_LPDF_LOGLIK_GAUSS 1 /* class loglik_gauss, src/lpdfs/loglik_gauss.cpp:41-172 */
#define OBHIP_LPDF_LOGLIK_GDA 2   /* class loglik_gda,   src/lpdfs/loglik_gda.cpp:48-235 */
#define OBHIP_LPDF_LOGPR_GAUSS 3  /* class logpr_gauss,  src/lpdfs/logpr_gauss.cpp:41-186 */
#define OBHIP_LPDF_VEC 4          /* class lpdfvec,      src/fit.cpp:174-612 */
/* new(loglik_std | loglik_gauss | loglik_gda, om, terms, y, x): interfaceR.cpp:733-750.
 * terms p x d column-major, y n, x n x d column-major with leading dimension ldx (host). */
int obhip_loglik_create(obhip_lpdf **out, int kind, const obhip_model *om, const uint64_t *terms,
                        uint64_t p, const double *y, const double *x, uint64_t n, uint64_t ldx);
/* new(logpr_gauss, om, terms): interfaceR.cpp:752-756 */
int obhip_logpr_gauss_create(obhip_lpdf **out, const obhip_model *om, const uint64_t *terms,
                             uint64_t p);
/* new(lpdfvec, a, b): interfaceR.cpp:758-762, fit.cpp:174-200; para = [a.para, b.para] */
int obhip_lpdfvec_create(obhip_lpdf **out, obhip_lpdf *a, obhip_lpdf *b);
int obhip_lpdf_destroy(obhip_lpdf *l);
/* kind, nterms (field, interfaceR.cpp:709), npara, number of hyper-parameters of the model,
 * rows of the likelihood's data (0 for the prior); any pointer may be NULL */
int obhip_lpdf_dims(const obhip_lpdf *l, int *kind, uint64_t *nterms, uint64_t *npara,
                    uint64_t *nhyp, uint64_t *n);
/* boolean fields: compute_* (interfaceR.cpp:698-701; this ABI names them by what they do --
 * the reference module binds R's compute_gradpara to C++ compute_gradhyp and vice versa),
 * fullhess (read-only, :702), lpdfvec's domarg (:761), loglik_gda's dodiag (:748) */
#define OBHIP_FLAG_COMPUTE_VAL 0
#define OBHIP_FLAG_COMPUTE_GRAD 1
#define OBHIP_FLAG_COMPUTE_GRADHYP 2
#define OBHIP_FLAG_COMPUTE_GRADPARA 3
#define OBHIP_FLAG_FULLHESS 4
#define OBHIP_FLAG_DOMARG 5
#define OBHIP_FLAG_DODIAG 6
int obhip_lpdf_get_flag(const obhip_lpdf *l, int flag, int *value);
int obhip_lpdf_set_flag(obhip_lpdf *l, int flag, int value);
/* field val (interfaceR.cpp:703) */
int obhip_lpdf_get_val(const obhip_lpdf *l, double *val);
/* vector fields (interfaceR.cpp:704-708,737,743,749,755; para0 / paravar fit.h:59-60;
 * totdiaghess fit.h:33): out may be NULL to query the length */
#define OBHIP_VEC_COEFF 0
#define OBHIP_VEC_GRAD 1
#define OBHIP_VEC_GRADHYP 2
#define OBHIP_VEC_GRADPARA 3
#define OBHIP_VEC_PARA 4
#define OBHIP_VEC_PARA0 5
#define OBHIP_VEC_PARAVAR 6
#define OBHIP_VEC_TOTDIAGHESS 7
#define OBHIP_VEC_COEFFSD 8 /* logpr_gauss only */
#define OBHIP_VEC_YHAT 9    /* likelihoods only; copied from HBM */
int obhip_lpdf_get_vec(const obhip_lpdf *l, int which, double *out, uint64_t cap, uint64_t *len);
/* names of the parameters, getpara(lpdf): interfaceR.cpp:193-199 */
int obhip_lpdf_paraname(const obhip_lpdf *l, uint64_t i, const char **name);
/* the umat `terms` of the object (fit.h:31), p x d column-major */
int obhip_lpdf_terms(const obhip_lpdf *l, uint64_t *terms_out);
/* the outerbase a likelihood owns (member `ob`, fit.h:185,237,273) and the device form of
 * its terms; borrowed handles, valid until the next updateterms / destroy */
int obhip_lpdf_basis(obhip_lpdf *l, obhip_basis **b, obhip_terms **t);
/* Rows sharded over the ranks of comm (no reference counterpart): the
 * likelihood (loglik_gauss | loglik_std; given an lpdfvec, its likelihood) holds this
 * rank's rows, and every sum over rows -- val, grad, gradhyp, gradpara, hessmult,
 * diaghess*, hess, optcg, optnewton -- is summed over the ranks, so that all ranks see the
 * numbers of the whole data set; para0 = log(0.01 var(y)) takes var(y) over all rows.
 * Collective: every rank calls it, and afterwards the same methods in the same order.
 * loglik_gda refuses (obfit runs it on a subsample every rank holds); NULL detaches. */
int obhip_lpdf_set_comm(obhip_lpdf *l, obhip_comm *comm);
/* lpdf$setnthreads (interfaceR.cpp:710): accepted and ignored on the device */
int obhip_lpdf_setnthreads(obhip_lpdf *l, int nthreads);
/* lpdf$update(coeff): loglik_gauss.cpp:110-130, loglik_std.cpp:100-120, loglik_gda.cpp:117-153,
 * logpr_gauss.cpp:113-121, lpdfvec fit.cpp:323-380 (marginal adjustment included) */
int obhip_lpdf_update(obhip_lpdf *l, const double *coeff, uint64_t ncoeff);
/* lpdf$updateom() / updatepara(para) / updateterms(terms): interfaceR.cpp:714-716 */
int obhip_lpdf_updateom(obhip_lpdf *l);
int obhip_lpdf_updatepara(obhip_lpdf *l, const double *para, uint64_t npara);
int obhip_lpdf_updateterms(obhip_lpdf *l, const uint64_t *terms, uint64_t p);
/* lpdf$hessmult(g) -> p; diaghess() -> p; diaghessgradhyp() -> p x nhyp;
 * diaghessgradpara() -> p x npara (column-major): interfaceR.cpp:717-720 */
int obhip_lpdf_hessmult(obhip_lpdf *l, const double *g, double *out);
int obhip_lpdf_diaghess(obhip_lpdf *l, double *out);
int obhip_lpdf_diaghessgradhyp(obhip_lpdf *l, double *out);
int obhip_lpdf_diaghessgradpara(obhip_lpdf *l, double *out);
/* hess() (fit.h:81; loglik_std.cpp:170-173, logpr_gauss.cpp:167-172, lpdfvec::hess_
 * fit.cpp:503-512): p x p, formed on the device by the Gram kernels */
int obhip_lpdf_hess(obhip_lpdf *l, double *out);
/* lpdf$optcg(tol, maxepch) (fit.cpp:37-96; iters may be NULL) and lpdf$optnewton()
 * (fit.cpp:98-131) */
int obhip_lpdf_optcg(obhip_lpdf *l, double tol, uint64_t maxepch, uint64_t *iters);
int obhip_lpdf_optnewton(obhip_lpdf *l);
/* lpdf$paralpdf(para) / paralpdf_grad(para): fit.cpp:133-157, lpdfvec fit.cpp:470-496 */
int obhip_lpdf_paralpdf(const obhip_lpdf *l, const double *parap, uint64_t n, double *out);
int obhip_lpdf_paralpdf_grad(const obhip_lpdf *l, const double *parap, uint64_t n, double *out);

/* new(predictor, lpdf) (interfaceR.cpp:725-731, lpdf::pred fit.h:51-55): the predictor of the
 * likelihood -- predr_std (loglik_std.cpp:218-256), pred_gauss (loglik_gauss.cpp:196-227),
 * pred_gda (loglik_gda.cpp:247-281); an lpdfvec stands for its likelihood.  Starts at the
 * training inputs like the reference. */
int obhip_predictor_create(obhip_predictor **out, const obhip_lpdf *l);
int obhip_predictor_destroy(obhip_predictor *p);
int obhip_predictor_setnthreads(obhip_predictor *p, int nthreads);
/* predictor$update(x): x n x d column-major, leading dimension ldx (host) */
int obhip_predictor_update(obhip_predictor *p, const double *x, uint64_t n, uint64_t ldx);
int obhip_predictor_n(const obhip_predictor *p, uint64_t *n);
/* predictor$mean() / $var(): n values */
int obhip_predictor_mean(obhip_predictor *p, double *out);
int obhip_predictor_var(obhip_predictor *p, double *out);
/* d mean / d x at the rows of the last update(): n x d column-major (obhip_predict_grad_dev; no
 * reference counterpart).  The mean is the same B theta for all three likelihoods. */
int obhip_predictor_gradmean(obhip_predictor *p, double *out);
int obhip_predictor_d(const obhip_predictor *p, uint64_t *d); /* input dimensions of its model */

/* ---- product of two input blocks (no reference counterpart) -----------------------------------
 * The emulator at every pair (row i of xa, row j of xb): the dimensions dims_b (0-based, strictly
 * ascending, 1 <= ndims_b <= d - 1) take their inputs from xb (nb rows, one column per entry of
 * dims_b, in that order), all other dimensions, ascending, from xa (na rows).  In the notation of
 * obhip_predict_grad_dev a design-matrix entry is s prod_{l: t_kl > 0} r_{l,t_kl}, a product over
 * the dimensions, so with A the dimensions of xa and B those of xb
 *     mean[i, j] = sA_i sB_j sum_k theta_k U_ik V_jk
 *     var[i, j]  = sA_i^2 sB_j^2 sum_k c_k U_ik^2 V_jk^2 + e^{2 sigma}    (obhip_predict_dev's diagonal form)
 *     U_ik = prod_{l in A, t_kl > 0} r_{l,t_kl}(xa_i)      sA_i = prod_{l in A} R_l0(xa_i)     (V, sB likewise)
 * : a matrix product with inner dimension p whose operands are formed from two basis tiles on the
 * fly, on the matrix cores.  The na nb rows of the full-width input are never written.  Term sets
 * whose two side tiles do not fit the kernel's LDS (obhip_product_layout reports it), and
 * OBHIP_FORCE_GENERIC, are expanded in bounded row chunks and go through obhip_predict_multi_dev.
 * OBHIP_ERR_INVALID before any device call, nothing written: a dims_b entry out of range, repeated
 * or unsorted; lda < na; d_var without d_coeffvar.  na = 0 or nb = 0: nothing to do. */
/* host only: the used basis columns of the two sides (the ones column counted on both:
 * mu_a + mu_b = used columns of the terms + 1) and whether the fused kernel takes the split */
int obhip_product_layout(const obhip_terms *t, const uint32_t *dims_b, uint64_t ndims_b,
                         uint64_t *mu_a, uint64_t *mu_b, int *fused);
/* d_mean[(r nb + j) lda + i], r < q: response r (column r of d_Theta, p x q with leading dimension
 * p) at the pair (i, j); d_var[j lda + i] (may be NULL, needs d_coeffvar): the variance, the same for
 * every response in standardised units.  d_xa na x |A|, d_xb nb x |B|, column-major without padding. */
int obhip_predict_product_dev(const obhip_model *m, const obhip_terms *t, const double *d_Theta,
                              uint64_t q, const uint32_t *dims_b, uint64_t ndims_b,
                              const double *d_xa, uint64_t na, const double *d_xb, uint64_t nb,
                              double *d_mean, uint64_t lda, const double *d_coeffvar, double sigma,
                              double *d_var);
/* The sums of a Gaussian likelihood of field data y (na, standardised) at the settings xa for every
 * candidate row of xb, one response: with r_ij = y_i - mean_ij and v_ij = var_ij + obsvar_i (var_ij
 * = e^{2 sigma} without d_coeffvar, obsvar_i = 0 without d_obsvar) d_out (nb x 2, column-major) =
 * [chi2_j = sum_i r_ij^2 / v_ij, logdet_j = sum_i log v_ij].  The na x nb matrices are not written;
 * the sums run in a fixed order without atomics: two calls give the same bits.  A negative or
 * non-finite d_obsvar entry is found on the device: OBHIP_ERR_NUMERIC, d_out untouched. */
int obhip_product_loglik_dev(const obhip_model *m, const obhip_terms *t, const double *d_theta,
                             const uint32_t *dims_b, uint64_t ndims_b, const double *d_xa,
                             uint64_t na, const double *d_y, const double *d_obsvar,
                             const double *d_xb, uint64_t nb, const double *d_coeffvar, double sigma,
                             double *d_out);
/* host-buffer forms like obhip_predict_multi: xa, xb with leading dimensions ldxa, ldxb; they refuse
 * a negative or non-finite obsvar with OBHIP_ERR_INVALID before any device call */
int obhip_predict_product(const obhip_model *m, const obhip_terms *t, const double *Theta, uint64_t q,
                          const uint32_t *dims_b, uint64_t ndims_b, const double *xa, uint64_t na,
                          uint64_t ldxa, const double *xb, uint64_t nb, uint64_t ldxb, double *mean,
                          uint64_t lda, const double *coeffvar, double sigma, double *var);
int obhip_product_loglik(const obhip_model *m, const obhip_terms *t, const double *theta,
                         const uint32_t *dims_b, uint64_t ndims_b, const double *xa, uint64_t na,
                         uint64_t ldxa, const double *y, const double *obsvar, const double *xb,
                         uint64_t nb, uint64_t ldxb, const double *coeffvar, double sigma, double *out);

/* ---- gradient by xb on the product (no reference counterpart) ---------------------------------
 * The derivatives of the pair's mean and variance, and of the two likelihood sums, by the inputs of
 * block B: what an optimiser or an HMC / MALA sampler over the candidate rows of xb needs per step.
 * One response.  Notation of the section above and of obhip_predict_grad_dev; l runs over the L =
 * ndims_b dimensions of B, in the order of dims_b.  For B row j
 *     rho_jl = R'_l0 / R_l0        r'_{l,t} = (R'_lt - r_lt R'_l0) / R_l0
 *     E_jkl  = V_jk without dimension l's factor (a product, never a quotient)
 * and with S_ij = sum_k theta_k U_ik V_jk, Q_ij = sum_k c_k U_ik^2 V_jk^2, s = sA_i sB_j
 *     m'_ijl = d mean_ij / d xb_jl = s (rho_jl S_ij + D_ijl)
 *              D_ijl = sum_{k: t_kl > 0} theta_k U_ik E_jkl r'_{l,t_kl}(xb_j)
 *     v'_ijl = d var_ij / d xb_jl = 2 s^2 (rho_jl Q_ij + F_ijl)
 *              F_ijl = sum_{k: t_kl > 0} c_k U_ik^2 V_jk E_jkl r'_{l,t_kl}(xb_j)
 *     d chi2_j / d xb_jl   = sum_i ( -2 r_ij / v_ij m'_ijl - r_ij^2 / v_ij^2 v'_ijl )
 *     d logdet_j / d xb_jl = sum_i v'_ijl / v_ij
 * (v' = 0 without d_coeffvar).  D and F run over the VIEW of l only -- the terms that contain
 * dimension l -- as matrix products on the matrix cores after the dense pass: all L gradients cost
 * about view_terms / p more passes, view_terms = sum_l |view_l|, not L more.  Term sets whose tiles
 * (the B tile now with its derivative columns and L columns of rho) do not fit the kernel's LDS, and
 * OBHIP_FORCE_GENERIC, are expanded in bounded row chunks and go through obhip_predict_grad_dev.
 * Refusals as in the section above.  Fixed summation order, no atomics: two calls give the same bits. */
/* host only: obhip_product_layout's mu_a and mu_b, view_terms, and whether the fused gradient kernel
 * takes the split */
int obhip_product_grad_layout(const obhip_terms *t, const uint32_t *dims_b, uint64_t ndims_b,
                              uint64_t *mu_a, uint64_t *mu_b, uint64_t *view_terms, int *fused);
/* d_dmean[(l nb + j) lda + i] = m'_ijl; d_dvar (same shape; may be NULL, needs d_coeffvar) = v'_ijl.
 * The mean-only call gives the bits of the d_dmean of the call with the variance. */
int obhip_predict_product_grad_dev(const obhip_model *m, const obhip_terms *t, const double *d_theta,
                                   const uint32_t *dims_b, uint64_t ndims_b, const double *d_xa,
                                   uint64_t na, const double *d_xb, uint64_t nb, double *d_dmean,
                                   uint64_t lda, const double *d_coeffvar, double sigma,
                                   double *d_dvar);
/* obhip_product_loglik_dev with the gradients: d_out is nb x (2 + 2 L), column-major,
 * [chi2, logdet, d chi2 / d xb_0 .., d logdet / d xb_0 ..].  On the fused route the first two
 * columns carry the bits of obhip_product_loglik_dev (the same contraction).  A bad d_obsvar:
 * OBHIP_ERR_NUMERIC, d_out untouched. */
int obhip_product_loglik_grad_dev(const obhip_model *m, const obhip_terms *t, const double *d_theta,
                                  const uint32_t *dims_b, uint64_t ndims_b, const double *d_xa,
                                  uint64_t na, const double *d_y, const double *d_obsvar,
                                  const double *d_xb, uint64_t nb, const double *d_coeffvar,
                                  double sigma, double *d_out);
/* host-buffer forms, as above: dmean, dvar with leading dimension lda, out nb x (2 + 2 L) */
int obhip_predict_product_grad(const obhip_model *m, const obhip_terms *t, const double *theta,
                               const uint32_t *dims_b, uint64_t ndims_b, const double *xa, uint64_t na,
                               uint64_t ldxa, const double *xb, uint64_t nb, uint64_t ldxb,
                               double *dmean, uint64_t lda, const double *coeffvar, double sigma,
                               double *dvar);
int obhip_product_loglik_grad(const obhip_model *m, const obhip_terms *t, const double *theta,
                              const uint32_t *dims_b, uint64_t ndims_b, const double *xa, uint64_t na,
                              uint64_t ldxa, const double *y, const double *obsvar, const double *xb,
                              uint64_t nb, uint64_t ldxb, const double *coeffvar, double sigma,
                              double *out);

/* ---- synthetic workload of BASELINE.md section 3 (benchmark input) ------ */
/* rows [row0, row0+n) of the counter-based SplitMix64 stream; d_x is n x d
 * column-major, d_y n (raw, not standardised).  kinds: d entries. */
int obhip_synth_xy_dev(uint64_t seed, uint64_t row0, uint64_t n, uint64_t d,
                       const int *kinds, double *d_x, double *d_y);
/* sum and sum of squares of a device vector (for standardising y) */
int obhip_sum_sumsq_dev(const double *d_v, uint64_t n, double *d_out2);
/* v = (v - cent) / sca in place */
int obhip_affine_dev(double *d_v, uint64_t n, double cent, double sca);

/* ---- device memory helpers for non-torch callers (Rcpp glue) ------------ */
int obhip_malloc(void **d_ptr, uint64_t bytes);
int obhip_free(void *d_ptr);
int obhip_memcpy_h2d(void *d_dst, const void *src, uint64_t bytes);
int obhip_memcpy_d2h(void *dst, const void *d_src, uint64_t bytes);
int obhip_memcpy_d2d(void *d_dst, const void *d_src, uint64_t bytes); /* async */

#ifdef __cplusplus
}
#endif
#endif /* OBHIP_H */
