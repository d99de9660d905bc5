/* pygps_amd -- C ABI of the MI355X-native exact-GP core (drop-in for the hot path of
 * marionmari/pyGPs: Core/cov.py kernel-matrix construction + Core/inf.py Exact/EP inference +
 * Core/tools.py jitchol/solve_chol + Core/gp.py predict).  Covariance functions: the stationary kernels that are functions of
 * one squared distance, Sum / Product / Scale trees over them, and the spectral mixture kernel PGP_COV_SM, which has tile code
 * and a fused gradient pass of its own and travels through the same entry points.
 *
 * Plain C, caller-owned host buffers, fp64, numpy row-major unless stated.  No exception crosses
 * the ABI.  Every function returns an int status:
 *      0            ok
 *     >0            LAPACK-style info: 1-based index of the first non-positive pivot
 *                   (the shim raises numpy.linalg.LinAlgError, as Core/tools.py:66-77 does)
 *     -1 .. -99     bad argument (index of the offending argument; the shim raises the reference's
 *                   plain Exception with the reference's message)
 *     <= -100       HIP runtime failure (pgp_strerror gives the text; the shim raises RuntimeError)
 *
 * One pgp_ctx = one device + one HIP stream + one workspace pool; NOT thread-safe; calls are
 * synchronous (stream-synchronised before return).  Multi-GPU = one process / one ctx per GPU.
 *
 * The Python binding a pyGPs maintainer would add is pygps_amd/_lib.py (ctypes); see INTEGRATION.md.
 */
#ifndef PYGPS_AMD_H
#define PYGPS_AMD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgp_ctx pgp_ctx;
typedef struct pgp_factor pgp_factor;
/* device-resident posterior: factor R, alpha, sW, inputs */
typedef struct pgp_fitc pgp_fitc;     /* FITC posterior on the device (alpha, dense L, inducing coordinates) */

/* covariance kinds            reference class                      */
#define PGP_COV_RBF 0     /* Core/cov.py:786-828   hyp=[log ell, log sf]               */
#define PGP_COV_RBFARD 1  /* Core/cov.py:872-938   hyp=[log ell_1..log ell_D, log sf]   (any D with nhyp <= 255) */
#define PGP_COV_MATERN 2  /* Core/cov.py:1078-1182 hyp=[log ell, log sf], para=d in {1,3,5,7} */
#define PGP_COV_RBFUNIT 3 /* Core/cov.py:832-869   hyp=[log ell]                                  */
#define PGP_COV_RQ 4      /* Core/cov.py:1304-1347 hyp=[log ell, log sf, log alpha]               */
#define PGP_COV_PIECEPOLY 5 /* Core/cov.py:683-782 hyp=[log ell, log sf], para=v in {0,1,2,3}      */
#define PGP_COV_RQARD 6   /* Core/cov.py:1356-1425 hyp=[log ell_1..log ell_D, log sf, log alpha]     */
#define PGP_COV_GABOR 7   /* Core/cov.py:392-450   hyp=[log ell, log p]  (p = exp(2 hyp1), as the reference) */
#define PGP_COV_PERIODIC 8 /* Core/cov.py:1186-1250 hyp=[log ell, log p, log sf], 1-d inputs only    */
#define PGP_COV_NOISE 9   /* Core/cov.py:1254-1300 hyp=[log sf]                                      */
#define PGP_COV_CONST 10  /* Core/cov.py:941-982   hyp=[log sf]  (sf2 = exp(hyp0), as the reference) */
#define PGP_COV_SM 11     /* Core/cov.py:454-619   spectral mixture, para=Q, hyp=[log w (Q) | log m (D x Q) | log sqrt(v) (D x Q)],
                           * nhyp = Q (1 + 2 D) <= 255 and D <= 16 (else -13).  The product over the coordinates as documented
                           * (GPML covSM); the reference agrees for D = 1 and sums partial products for D > 1.  Own tile code:
                           * not a leaf of a composite program (pgp_set_composite stores any tokens; the pgp_cov / fit call that
                           * expands a program with such a leaf answers -2) */
#define PGP_COV_PRE 12    /* Core/cov.py:1429-1455 precomputed kernel matrix, no hypers: the value of element (row, col) is read from
                           * the matrices bound with pgp_set_pre.  Alone or as ONE leaf of a composite program (a second one: -13).
                           * Fits and pgp_predict only: pgp_cov answers -13 (the Python class slices its host arrays). */
/* Dot-product kernels, p = sum_k x_k z_k; J = 1e-10 on the training diagonal, 0 elsewhere.  k(x, x) differs from point to point:
 * SELF_TEST writes one value per point, pgp_predict computes k(z, z) per test point on the device, EP reads K_ii off the matrix.
 * The drivers built on one scalar k(x, x) -- pgp_fitc_* fits, pgp_sharded_exact_fit, pgp_gpmc_fit_predict -- answer -13 for these
 * kinds and for programs that hold them. */
#define PGP_COV_LINEAR 13 /* Core/cov.py:986-1024  hyp=[log sf]  sf2 (p + J), sf2 = exp(hyp0) (not squared, as the reference; derivative
                           * 2 sf2 p).  Alone (any D) or as a leaf of a composite program. */
#define PGP_COV_POLY 14   /* Core/cov.py:623-679   hyp=[log c, log sf], para=d >= 1 (else -12)  sf2 (c + p + J)^d, sf2 = exp(2 hyp1).
                           * der 2 ("the degree") gives zeros on the plain kind.  Alone (any D) or as a leaf of a program. */
#define PGP_COV_LINARD 15 /* Core/cov.py:1028-1074 hyp=[log ell_1..log ell_D]  sum_k x_k z_k / ell_k^2 + J (GPML covLINard; the reference
                           * agrees at ell = 1).  Plain kind only, any D with nhyp <= 255 (1 / ell_k folded into the coordinates); as
                           * a leaf of a composite program it answers -2. */
#define PGP_COV_NKIND 16
/* Sum / Product / Scale tree over primitives (Core/cov.py:230-328; up to two ARD leaves), registered with
 * pgp_set_composite and selected by kind = PGP_COV_COMPOSITE in pgp_cov / pgp_exact_fit / pgp_ep_fit.
 * hyp is the composite's flattened list in the reference's order (cov1.hyp + cov2.hyp; [scalar] + cov.hyp). */
#define PGP_COV_COMPOSITE 100
/* postfix program tokens */
#define PGP_PROG_LEAF 1    /* LEAF kind para flags first_hyp_index */
#define PGP_PROG_SUM 2
#define PGP_PROG_PRODUCT 3
#define PGP_PROG_SCALE 4   /* SCALE hyp_index */
/* modes of getCovMatrix / getDerMatrix (Core/cov.py:81-111) */
#define PGP_MODE_TRAIN 0
#define PGP_MODE_CROSS 1
#define PGP_MODE_SELF_TEST 2
/* flags */
#define PGP_FLAG_MATERN_REFERENCE_DER 1 /* reproduce the reference's derivative quirks: Matern Core/cov.py:1173-1177
                                         * (derivative of K, not t); RQard :1412-1418 (length-scale derivatives) */

/* ---- lifetime ---------------------------------------------------------------------------- */
int pgp_init(int device, pgp_ctx** ctx_out);
void pgp_destroy(pgp_ctx* ctx);
const char* pgp_strerror(int status);
const char* pgp_version(void);
int pgp_device_count(void);              /* visible HIP devices (0 when there is none or no driver) */
int pgp_device_info(pgp_ctx* ctx, int* n_cu, int* sclk_mhz, double* hbm_gib, char* name, int name_len);

/* ---- kernel plug-in: Kernel.getCovMatrix / getDerMatrix (Core/cov.py:81-111) ---------------
 * der < 0 : covariance value; der >= 0 : derivative w.r.t. hyper `der` (log-space).
 * TRAIN: x (n,d) -> out (n,n).  CROSS: x (n,d), z (m,d) -> out (n,m).  SELF_TEST: z (m,d) -> out (m,1).
 * Error codes: -3 unknown mode, -4 derivative index does not exist, -5/-7 missing x / z.        */
int pgp_cov(pgp_ctx* ctx, int kind, int mode, int der, const double* x, int64_t n, const double* z, int64_t m,
            int64_t d, const double* hyp, int nhyp, int para, int flags, double* out);

/* Composite kernels: ProductOfKernel / SumOfKernel / ScaleOfKernel (Core/cov.py:230-328).  prog is the tree in
 * postfix order (PGP_PROG_* tokens); it stays registered in the context until replaced.  Limits: 8 leaves, 8 Scale
 * nodes, 8 products after distributing products over sums; at most TWO ARD leaves (RBFard / RQard), each with D <= 64
 * (their 1 / ell_k^2 weights travel as kernel arguments); anything beyond returns -13 from the calls that use the program
 * -- the Python layer then takes the dense path (pgp_exact_fit_dense / pgp_ep_fit_dense).  The PLAIN kinds
 * PGP_COV_RBFARD / PGP_COV_RQARD take any D (the scales are folded into the coordinates).
 * Budget of accumulators: beside the shared r^2 a program carries at most TWO more.  Every ARD leaf takes one; all PGP_COV_LINEAR /
 * PGP_COV_POLY leaves together take one (the unweighted dot product, any D).  So: two ARD leaves, or one ARD leaf and any number of
 * dot-product leaves; two ARD leaves and a dot-product leaf: -13.  A program holds either a PGP_COV_PRE leaf or dot-product leaves
 * (both: -13).  Status of the calls that expand a program or a plain kind: -4 derivative index, -12 bad para (Poly d < 1),
 * -13 over these limits. */
int pgp_set_composite(pgp_ctx* ctx, const int32_t* prog, int nprog);

/* cov.Pre: bind the precomputed matrices of the (one) PGP_COV_PRE leaf to the context; they stay resident until replaced.
 * M2 (n, n) row-major, symmetric: the training matrix, n = the n of pgp_set_data at fit time (else the fit answers -14).
 * M1 (n + 1, ns) row-major: cross-covariances with ns test points, last row = their self-covariances; needed by pgp_predict
 * only (a posterior of a program with this leaf answers -15 when no M1 with ns columns is bound).  Either pointer may be NULL:
 * that matrix is kept as it is (a new M2 drops the M1 bound before).  -2: M1 without an M2 of this n. */
int pgp_set_pre(pgp_ctx* ctx, const double* M2, int64_t n, const double* M1, int64_t ns);

/* ---- graph node kernels and the k-NN graph (GraphExtensions/nodeKernels.py, graphUtil.py:29-46) -------------
 * A (n, n) row-major host: dense symmetric adjacency matrix without isolated nodes; K_out (n, n) row-major host.
 *   PGP_NODE_REGLAP  inv(I + p0^2 L), L the normalised Laplacian      PGP_NODE_VND   inv(I - p0 S), S = I - L
 *   PGP_NODE_RW      (p0 I - L)^p1, p1 an integer >= 1                PGP_NODE_DIFF  exp(p0 (A - D))
 * The inverses are a Cholesky factorisation with its inverse: a matrix that is not positive definite (VND with p0 >= 1)
 * answers the index of the first bad pivot (> 0) like the fits.  Powers and the exponential (scaled Taylor series of
 * degree 18 with repeated squaring) are products on the fp64 GEMM. */
#define PGP_NODE_REGLAP 0
#define PGP_NODE_VND 1
#define PGP_NODE_RW 2
#define PGP_NODE_DIFF 3
int pgp_node_kernel(pgp_ctx* ctx, int kind, const double* A, int64_t n, double p0, double p1, double* K_out);
/* pc (n, d) row-major host; A_out (n, n) row-major host: 0 / 1 adjacency of the k-nearest-neighbour graph by brute-force
 * squared distances, the point itself left out, ties broken by the lower index, symmetrised with max (1 <= k < n). */
int pgp_knn_graph(pgp_ctx* ctx, const double* pc, int64_t n, int64_t d, int k, double* A_out);

/* ---- propagation kernels between graphs (GraphExtensions/graphKernels.py:27-184) -------------------------------
 * n nodes in n_graphs graphs, k label classes (2 <= k <= PGP_PROP_MAX_LABELS).  All pointers are host memory.
 *   indptr (n + 1), indices (nnz), vals (nnz): CSR of the matrix applied in the update (the row-normalised adjacency T, or
 *       0.8 S for PGP_PROP_SPREAD), entries in the order they are to be summed; may be NULL for PGP_PROP_NONE.
 *   lab_prob (n, k) row-major: the initial label distributions.  lab_orig (n, k) or NULL, push_back (n) or NULL: rows with
 *       push_back[i] != 0 are read from lab_orig in every update ('label_propagation').
 *   perm (n): the nodes in graph-grouped order; seg (n_graphs + 1): graph g owns perm[seg[g] .. seg[g + 1]).
 *   V (h_max + 1, k) row-major and b (h_max + 1): projection and offset of every iteration; w > 0 the bin width.
 *   update: PGP_PROP_NONE, PGP_PROP_T (lab <- T lab) or PGP_PROP_SPREAD (lab <- T lab + orig_weight lab_orig).
 *   take_sqrt: lab <- sqrt(lab) in place before every hash (it carries into the next update, as in the reference).
 *   sum: slice h is K_0 + ... + K_h, else K_h.
 * K_out (n_graphs, n_graphs, h_max + 1) row-major; K_h[g1, g2] = number of node pairs (i in g1, j in g2) with
 * floor((lab_i . v_h + b_h) / w) equal.  Counts are summed in 64-bit integers.  lab_out (n, k) or NULL: lab after the last
 * iteration.  stage_ms_out (6) or NULL: device time of upload | update | hash | sort | gram | download in ms.
 * Every product and sum runs in a defined order without contraction: the update in the stored CSR order, the hash over
 * j = 0 .. k - 1.  Status: -1 ... -13 for the arguments in their order of mention (-6: CSR arrays missing or inconsistent,
 * -9: perm is no permutation or seg does not partition it); PGP_ERR_PROP_NONFINITE: some key is not finite (overflow, or an
 * infinite projection entry). */
#define PGP_PROP_NONE 0
#define PGP_PROP_T 1
#define PGP_PROP_SPREAD 2
#define PGP_PROP_MAX_LABELS 256
#define PGP_PROP_SORT_LDS 2048  /* keys of one graph sorted in LDS; longer graphs sort on a global scratch */
#define PGP_PROP_GRAM_LDS 5120  /* (key, count) pairs of the 32 graphs of a tile held in LDS; larger tiles read global memory */
#define PGP_ERR_PROP_NONFINITE (-91)
int pgp_propagation_kernel(pgp_ctx* ctx, int64_t n, int64_t k, int64_t n_graphs, const int64_t* indptr, const int32_t* indices,
                           const double* vals, const double* lab_prob, const double* lab_orig, const uint8_t* push_back,
                           const int32_t* perm, const int64_t* seg, int h_max, const double* V, const double* b, double w, int update,
                           double orig_weight, int take_sqrt, int sum, double* K_out, double* lab_out, double* stage_ms_out);

/* ---- data residency -------------------------------------------------------------------------
 * The optimiser calls the fit hundreds of times with identical (x, y) and only hyp changing
 * (Core/opt.py:70-75), so x and y are uploaded once.                                            */
int pgp_set_data(pgp_ctx* ctx, const double* x, int64_t n, int64_t d, const double* y);

/* ---- inference plug-in: Exact.evaluate (Core/inf.py:353-384) ---------------------------------
 * Uses the data of the last pgp_set_data.  mvec: prior mean m (n); dm: (nmean, n) rows = derivative
 * of m w.r.t. each mean hyper (NULL if nmean == 0).  want = nargout (1: post, 2: +nlZ, 3: +dnlZ).
 * alpha_out (n), nlZ_out (1), dnlZ_out (nmean + ncov + 1, order mean|cov|lik as Core/opt.py:77-80).
 * factor_out (optional): handle keeping R (upper, R'R = K/sn2 + I), alpha, sW on the device.   */
int pgp_exact_fit(pgp_ctx* ctx, int kind, const double* covhyp, int ncov, int para, int flags, double log_sn,
                  const double* mvec, const double* dm, int nmean, int want, double* alpha_out, double* nlZ_out,
                  double* dnlZ_out, pgp_factor** factor_out);

/* ---- leave-one-out inference (csrc/loo.hip; GPML's infLOO, Rasmussen & Williams 5.4.2; no reference counterpart) ---------
 * The exact fit's stages up to B^-1 = E E' (B = K/sn2 + I) and alpha, its posterior (alpha, factor handle: pgp_predict and the
 * joint / sampling entry points work on it unchanged), then with Kinv = B^-1 / sn2, c_i = Kinv_ii:
 *      loo_mu_i = y_i - alpha_i / c_i     loo_s2_i = 1 / c_i (noise included)     loo_lp_i = log N(y_i | loo_mu_i, loo_s2_i)
 *      nlZ_out[0] = nlZ_loo = -sum loo_lp_i          nlZ_out[1] = the marginal nlZ of pgp_exact_fit
 *      dnlZ_out (nmean + ncov + 1, want = 3) = the gradient of nlZ_loo: 1/2 sum(Q_loo o dK_h), sn2 tr Q_loo, -u' dm_h with
 *      w_i = (1 + alpha_i^2 / c_i) / (2 c_i), u = Kinv (alpha / c), Q_loo = 2 Kinv diag(w) Kinv - u alpha' - alpha u'
 * want: 1 = posterior only (no LOO output), 2 = plus the values, 3 = plus the gradient.  loo_*_out (n each) may be NULL.
 * want = 2 runs nothing O(n^3) beyond the factorisation: diag(B^-1) is read off the fused inverse rows; want = 3 reads the same
 * sums, so both return the same bits.  With the fused inverse switched off or refused (options fused_inverse 0,
 * fused_value_max_np; no scratch) a want = 2 call takes want = 3's route to B^-1 instead (triangular inverse + W'W), and its alpha
 * is that route's (W'z), equal to pgp_exact_fit's want = 2 alpha (back-substitution) to rounding only.
 * pgp_loo_fit_dense: the same from a caller-built K (as pgp_exact_fit_dense); only r = y - m is handed in, so loo_mu_out is
 * r_i - alpha_i / c_i: THE CALLER ADDS m BACK.  u_out (n, want = 3, may be NULL): the mean gradients are -u' dm_h, formed by the
 * caller.  After want = 3 the workspace holds sn2 Q_loo and a zero alpha: pgp_dense_grad_term(ctx, dK_h, n, log_sn, &g) directly
 * afterwards returns 1/2 sum(Q_loo o dK_h).
 * Out of scope: EP / Laplace cavity LOO, FITC, sharded fits.  Status as pgp_exact_fit / pgp_exact_fit_dense. */
int pgp_loo_fit(pgp_ctx* ctx, int kind, const double* covhyp, int ncov, int para, int flags, double log_sn, const double* mvec,
                const double* dm, int nmean, int want, double* alpha_out, double* loo_mu_out, double* loo_s2_out,
                double* loo_lp_out, double* nlZ_out, double* dnlZ_out, pgp_factor** factor_out);
int pgp_loo_fit_dense(pgp_ctx* ctx, const double* K, int64_t n, const double* r, double log_sn, int want, double* alpha_out,
                      double* loo_mu_out, double* loo_s2_out, double* loo_lp_out, double* nlZ_out, double* dnlZ_lik_out,
                      double* u_out, pgp_factor** factor_out);

/* post.L as numpy expects it: (n,n) row-major UPPER factor, exact zeros below the diagonal
 * (Core/gp.py:393 branches on that).                                                           */
int pgp_factor_to_host(pgp_ctx* ctx, pgp_factor* f, double* L_out);
int64_t pgp_factor_n(pgp_factor* f);
void pgp_factor_free(pgp_ctx* ctx, pgp_factor* f);

/* ---- GP.predict (Core/gp.py:349-437), Cholesky parametrisation -------------------------------
 * fmu = ms + Ks' alpha ; fs2 = max(kss - colsum((R'^-1 (sW o Ks))^2), 0).                       */
int pgp_predict(pgp_ctx* ctx, pgp_factor* f, const double* xs, int64_t ns, const double* ms, double* fmu,
                double* fs2);

/* ---- the joint posterior at the test points and draws from it (csrc/joint.hip; no reference counterpart: Core/gp.py:395-417
 * stops at the marginals).  With V = R'^-1 (sW o Ks):
 *      fmu  = ms + Ks' alpha                          as pgp_predict
 *      fcov = Kss - V'V                               Kss = k(xs, xs) in 'train' mode (cov.Noise: sf2 I); its diagonal is the
 *                                                     'self_test' one: diag(fcov) is pgp_predict's fs2, clipped at 0 like it
 *      A    = fcov + (noise + jitter) I = Lc Lc'      the matrix that is factorised
 *      F    = fmu 1' + Lc Z                           Z (ns, nsamp) row-major: standard normal draws, made by the caller
 * All ns <= PGP_JOINT_MAX_POINTS points are one batch; V takes the form (product or blocked solve) pgp_predict would take for
 * them.  Outputs, row-major: fmu (ns); cov_out (ns, ns), exactly symmetric (one triangle computed, then mirrored), or NULL;
 * chol_out (ns, ns), the lower factor Lc with exact zeros above the diagonal, or NULL; samples_out (ns, nsamp) or NULL (then Z
 * and nsamp are ignored).  The factorisation runs only when chol_out or samples_out is given.  stage_ms_out (5, optional):
 * device ms of cross block + V | Kss | V'V | factorisation | draws and the downloads of cov_out / chol_out / samples_out, from
 * the call's own events (pgp_last_timings is not touched).  The posterior handle keeps nothing beyond what pgp_predict may
 * leave on it.
 * The factor is the Cholesky sweep's after one Newton step L <- L + L Phi(Y), Y = L^-1 (A - L L') L^-T, which brings its
 * componentwise residual to a substitution-based Cholesky's on badly conditioned A.  The step is first order in Y and is taken
 * only where nsp^2 max|Y| <= 1 (nsp = ns rounded up to 128): on a barely positive definite A that the sweep got through with
 * pivots at rounding level Y is not small, and the sweep's own factor is returned as it is, with status 0.  Option
 * "joint_refine" 0 always returns the sweep's factor, at an eighth of the factorisation time.
 * Kss is assembled in the difference form at every size, like the cross block it is subtracted from; the Gram-form assembly of
 * the fits is gated by a bound on the resident TRAINING inputs (gram_assembly_applies), which says nothing about xs.
 * Status: > 0 the first non-positive pivot of A (1-based, at most ns); -4 ns < 1 or ns > PGP_JOINT_MAX_POINTS (nothing is
 * allocated); -8 samples_out with nsamp < 1 or without Z; -13 a program with a PGP_COV_PRE leaf (cov.Pre carries no k(xs, xs));
 * otherwise as pgp_predict.
 * pgp_predict_joint_dense: the same for posteriors of caller-built matrices (pgp_exact_fit_dense ...): Ks (n, ns) =
 * getCovMatrix(x, xs, 'cross'), Kss (ns, ns) = getCovMatrix(xs, 'train') with the 'self_test' values on its diagonal.
 * pgp_sample_mvn: factor and draws for a caller's symmetric matrix A (ns, ns) and mean (ns, or NULL): A + jitter I = Lc Lc',
 * F = mean 1' + Lc Z (GP.sample_prior). */
#define PGP_JOINT_MAX_POINTS 16384
int pgp_predict_joint(pgp_ctx* ctx, pgp_factor* f, const double* xs, int64_t ns, const double* ms, double noise, double jitter,
                      const double* Z, int64_t nsamp, double* fmu, double* cov_out, double* chol_out, double* samples_out,
                      double* stage_ms_out);
int pgp_predict_joint_dense(pgp_ctx* ctx, pgp_factor* f, const double* Ks, const double* Kss, int64_t ns, const double* ms,
                            double noise, double jitter, const double* Z, int64_t nsamp, double* fmu, double* cov_out,
                            double* chol_out, double* samples_out, double* stage_ms_out);
int pgp_sample_mvn(pgp_ctx* ctx, const double* A, int64_t ns, const double* mean, double jitter, const double* Z, int64_t nsamp,
                   double* chol_out, double* samples_out);

/* ---- the same path from CALLER-BUILT covariance matrices (csrc/dense.hip) ---------------------------------
 * For covariance functions that are not device programs (Core/cov.py:230-328 composes anything; a tree with more than two
 * ARD leaves or more than 8 leaves has getCovMatrix / getDerMatrix only): K (n,n) = getCovMatrix(x, 'train'), r = y - m.
 * pgp_exact_fit_dense: want as pgp_exact_fit; dnlZ_lik_out = sn2 tr Q.  pgp_dense_grad_term: 1/2 sum(Q o dK) for one
 * derivative matrix dK = getDerMatrix(x, 'train', h), with the Q of the dense fit that directly precedes it on this context
 * (Core/inf.py:373-377).  pgp_predict_dense: Ks (n,ns) = getCovMatrix(x, xs, 'cross'), kss (ns) = 'self_test'.        */
int pgp_exact_fit_dense(pgp_ctx* ctx, const double* K, int64_t n, const double* r, double log_sn, int want,
                        double* alpha_out, double* nlZ_out, double* dnlZ_lik_out, pgp_factor** factor_out);
int pgp_dense_grad_term(pgp_ctx* ctx, const double* dK, int64_t n, double log_sn, double* out);
int pgp_predict_dense(pgp_ctx* ctx, pgp_factor* f, const double* Ks, int64_t ns, const double* kss, const double* ms,
                      double* fmu, double* fs2);

/* ---- EP.evaluate with lik.Erf (Core/inf.py:731-806, 174-189; Core/lik.py:295-366) ----------
 * ttau/tnu (n): in = warm start (ignored if warm == 0), out = final site parameters.           */
int pgp_ep_fit(pgp_ctx* ctx, int kind, const double* covhyp, int ncov, int para, int flags, const double* mvec,
               const double* dm, int nmean, int want, int warm, double* ttau, double* tnu, double* alpha_out,
               double* sW_out, double* nlZ_out, double* dnlZ_out, int* sweeps_out, pgp_factor** factor_out);

/* EP.evaluate (Core/inf.py:723-806) from a CALLER-BUILT covariance matrix: the covariance trees of Core/cov.py:230-328 that are
 * not device programs.  K (n, n) symmetric row-major host; n, y as set by pgp_set_data (x is not used).  dnlZ_mean_out: nmean + 1
 * entries (mean gradients, then 0: lik.Erf has no hyper-parameter).  want = 3 leaves sW sW' o B^-1 and alpha in the context's
 * workspace: pgp_dense_grad_term(ctx, dK_h, n, 0.0, &g) directly afterwards gives dnlZ.cov[h] (Core/inf.py:780-786).
 * Other arguments and status codes as pgp_ep_fit. */
int pgp_ep_fit_dense(pgp_ctx* ctx, const double* K, const double* mvec, const double* dm, int nmean, int want, int warm,
                     double* ttau_io, double* tnu_io, double* alpha_out, double* sW_out, double* nlZ_out,
                     double* dnlZ_mean_out, int* sweeps_out, pgp_factor** factor_out);

/* EP.evaluate with a likelihood argument (lik, likhyp, nlik as pgp_laplace_fit): PGP_LIK_ERF (nlik = 0: the fit of pgp_ep_fit /
 * pgp_ep_fit_dense) or PGP_LIK_LAPLACE (nlik = 1, likhyp = [log sn]: lik.Laplace, Core/lik.py:370-512).  dnlZ_out: nmean + ncov + 1
 * entries (mean, cov, lik; the dense form: nmean + 1, the covariance gradients follow from pgp_dense_grad_term as after
 * pgp_ep_fit_dense).  dnlZ.lik = -sum dlZhyp over the cavities (Core/inf.py:796-798).  With lik.Laplace the mean and likelihood
 * gradients are evaluated at the cavity of f (nu_n / tau_n + m); ref_compat = 1 evaluates them at the reference's nu_n / tau_n,
 * which differs wherever the mean is not zero.  A bad (lik, likhyp, nlik) returns -15.  Other arguments and status codes as
 * pgp_ep_fit. */
int pgp_ep_fit_lik(pgp_ctx* ctx, int kind, const double* covhyp, int ncov, int para, int flags, int lik, const double* likhyp,
                   int nlik, int ref_compat, const double* mvec, const double* dm, int nmean, int want, int warm, double* ttau_io,
                   double* tnu_io, double* alpha_out, double* sW_out, double* nlZ_out, double* dnlZ_out, int* sweeps_out,
                   pgp_factor** factor_out);
int pgp_ep_fit_dense_lik(pgp_ctx* ctx, const double* K, int lik, const double* likhyp, int nlik, int ref_compat, const double* mvec,
                         const double* dm, int nmean, int want, int warm, double* ttau_io, double* tnu_io, double* alpha_out,
                         double* sW_out, double* nlZ_out, double* dnlZ_out, int* sweeps_out, pgp_factor** factor_out);

/* ---- Laplace.evaluate with lik.Erf or lik.Gauss (Core/inf.py:459-564; Core/lik.py:175-197, 274-293) -----------------------
 * The Newton iteration in f with Brent's line search (inf.py:466-512, tools.py:121-272: tol 1e-6, at most 20 steps, s in [0, 2],
 * at most 20 evaluations per line search, thr 1e-4), then the posterior (inf.py:514-529) and, for want = 3, the gradients with
 * their implicit part (inf.py:530-562).  lik: PGP_LIK_ERF (likhyp unused, nlik = 0) or PGP_LIK_GAUSS (likhyp = [log sn], nlik = 1).
 * alpha_io (n): in = the last alpha (Laplace.last_alpha; used only if warm != 0, and kept only if its objective beats the default
 * start f = m as inf.py:474-497 decides), out = the final alpha.  sW_out (n), nlZ_out (1), dnlZ_out (nmean + ncov + nlik, order
 * mean | cov | lik).  steps_out: Newton steps taken.  trace_out (optional, 3 x 20): per Newton step the line search's step size,
 * objective Psi and number of evaluations.  factor_out: the posterior handle, the same form as EP's (pgp_predict serves it).
 * PGP_ERR_LAPLACE_WNEG: some W_i = -d2lp_i < 0 (the reference's LU branch, inf.py:500-502 / 520-523, is not restated; it cannot
 * occur for Erf or Gauss).  Other status codes as pgp_ep_fit. */
#define PGP_LIK_ERF 0
#define PGP_LIK_GAUSS 1
#define PGP_LIK_LAPLACE 2  /* EP only (pgp_ep_fit_lik, pgp_ep_fit_dense_lik) */
#define PGP_ERR_LAPLACE_WNEG (-90)
int pgp_laplace_fit(pgp_ctx* ctx, int kind, const double* covhyp, int ncov, int para, int flags, int lik, const double* likhyp,
                    int nlik, const double* mvec, const double* dm, int nmean, int want, int warm, double* alpha_io,
                    double* sW_out, double* nlZ_out, double* dnlZ_out, int* steps_out, double* trace_out, pgp_factor** factor_out);
/* Laplace.evaluate from a CALLER-BUILT covariance matrix K (n, n) (the covariance trees of Core/cov.py:230-328 that are not device
 * programs); n, y as set by pgp_set_data.  dnlZ_out: nmean + nlik entries (mean, then lik).  want = 3 leaves
 * R = sW sW' o B^-1 - u dlp' - dlp u' and alpha in the context's workspace: pgp_dense_grad_term(ctx, dK_h, n, 0.0, &g) directly
 * afterwards gives dnlZ.cov[h] (inf.py:536-541).  Other arguments and status codes as pgp_laplace_fit. */
int pgp_laplace_fit_dense(pgp_ctx* ctx, const double* K, int lik, const double* likhyp, int nlik, const double* mvec,
                          const double* dm, int nmean, int want, int warm, double* alpha_io, double* sW_out, double* nlZ_out,
                          double* dnlZ_out, int* steps_out, double* trace_out, pgp_factor** factor_out);

/* ---- GPMC.fitAndPredict (Core/gp.py:829-863): one-vs-one multi-class classification on ONE shared covariance matrix -------------
 * Every pair (i, j), i < j, of the n_class classes is a binary GPC with lik.Erf on the rows of the two classes (class i first,
 * labelled +1, then class j, -1, each in data order: createBinaryClass, gp.py:905-928), and all pairs share mean, kernel and
 * hyper-parameters.  K_all = k(x_all, x_all) and, per batch of test points, Ks_all = k(x_all, xs) are assembled once on the
 * device; every pair's fit (cold start, want = 2) and predict work on gathered principal submatrices / row subsets, and the votes
 * (gp.py:854-862) are accumulated and normalised on the device.  x_all: the x of the last pgp_set_data (its y is not used).
 * kind / covhyp / ncov / para / flags as pgp_ep_fit_lik.  inference: 0 = EP, 1 = Laplace.  labels (n): integer class of every
 * row, each class in [0, n_class) with at least one row (-8 otherwise).  m_all (n) / ms (ns): the prior mean at x_all / xs (NULL:
 * zero).  xs (ns, d).  votes_out (ns, n_class) row-major, rows sum to 1.  pair_nlZ_out / pair_iters_out (n_class (n_class - 1) / 2,
 * optional): nlZ and EP sweeps / Newton steps per pair in the order (0,1), (0,2), ..., (n_class-2, n_class-1).  Returns > 0: the
 * first bad pivot of the pair written to bad_pair_out (2 ints, optional), which also names the pair of any other failure;
 * -1 .. -99 bad argument; <= -100 HIP failure.  pgp_last_timings afterwards: assemble = K_all + Ks_all, solve = the fits,
 * potrf = the pairs' predicts, grad = the vote kernels, total = the whole call (ms). */
int pgp_gpmc_fit_predict(pgp_ctx* ctx, int kind, const double* covhyp, int ncov, int para, int flags, int inference,
                         const int32_t* labels, int n_class, const double* m_all, const double* xs, int64_t ns, const double* ms,
                         double* votes_out, double* pair_nlZ_out, int32_t* pair_iters_out, int32_t* bad_pair_out);

/* ---- FITC sparse regression: FITC_Exact.evaluate (Core/inf.py:398-455) with FITCOfKernel (Core/cov.py:332-390)
 * x, y of the last pgp_set_data; xu (nu,d) inducing inputs.  alpha_out (nu), L_out (nu,nu) = post.L (dense,
 * symmetric; NULL to skip), dnlZ_out = [mean.., cov.., lik].  snu2 = 1e-6 sn2 like the reference (inf.py:410).
 * Returns >0 when a Cholesky pivot is not positive.  handle_out (optional) feeds pgp_fitc_predict.               */
int pgp_fitc_fit(pgp_ctx* ctx, int kind, const double* covhyp, int ncov, int para, int flags, double log_sn,
                 const double* xu, int64_t nu, const double* mvec, const double* dm, int nmean, int want,
                 double* alpha_out, double* L_out, double* nlZ_out, double* dnlZ_out, pgp_fitc** handle_out);
/* the dense-L branch of GP.predict (Core/gp.py:404-417): fmu = ms + Ks'alpha, fs2 = max(kss + colsum(Ks o (L Ks)), 0) */
int pgp_fitc_predict(pgp_ctx* ctx, pgp_fitc* f, const double* xs, int64_t ns, const double* ms, double* fmu,
                     double* fs2);
void pgp_fitc_free(pgp_ctx* ctx, pgp_fitc* f);

/* ---- FITC sparse classification: FITC_EP.evaluate (Core/inf.py:810-944) with lik.Erf and FITCOfKernel --------------------
 * EP on Kt = Q + diag(K - Q) in O(n nu) memory, snu2 = 1e-6 (Erf has no hyper-parameter, inf.py:837-841): tol 1e-4, 2 to 10
 * sweeps over the sites in order 0..n-1, 128-site blocks (csrc/fitc.hip), a refresh and _epfitcZ's nlZ after every sweep.
 * warm != 0: ttau_io / tnu_io (n) hold the previous call's site parameters and are tried against nlZ0 as inf.py:857-870 does;
 * on return they hold the final ones.  alpha_out (nu), L_out (nu x nu row-major), nlZ_out, dnlZ_out (nmean + ncov: mean,
 * then covariance gradients), sweeps_out.  Returns >0 when a Cholesky pivot is not positive.  handle_out (optional) feeds
 * pgp_fitc_predict. */
int pgp_fitc_ep_fit(pgp_ctx* ctx, int kind, const double* covhyp, int ncov, int para, int flags, const double* xu, int64_t nu,
                    const double* mvec, const double* dm, int nmean, int want, int warm, double* ttau_io, double* tnu_io,
                    double* alpha_out, double* L_out, double* nlZ_out, double* dnlZ_out, int* sweeps_out,
                    pgp_fitc** handle_out);
/* FITC_EP with a likelihood argument (lik, likhyp, nlik as pgp_ep_fit_lik): PGP_LIK_ERF (nlik = 0: the fit of pgp_fitc_ep_fit) or
 * PGP_LIK_LAPLACE (nlik = 1, likhyp = [log sn]; snu2 = 1e-6 sn2, inf.py:837-841).  dnlZ_out: nmean + ncov + 1 entries with
 * lik.Laplace (mean, cov, lik), nmean + ncov with lik.Erf.  dnlZ.lik = -sum dlZhyp + snu2 (covariance-like term), inf.py:925-936,
 * with dlZhyp at the cavity nu_n / tau_n; ref_compat = 1 evaluates it at the reference's nu_n / tau_n + m, which counts the
 * mean twice.  A bad (lik, likhyp, nlik) returns -15.  Other arguments and status codes as pgp_fitc_ep_fit. */
int pgp_fitc_ep_fit_lik(pgp_ctx* ctx, int kind, const double* covhyp, int ncov, int para, int flags, int lik, const double* likhyp,
                        int nlik, int ref_compat, const double* xu, int64_t nu, const double* mvec, const double* dm, int nmean,
                        int want, int warm, double* ttau_io, double* tnu_io, double* alpha_out, double* L_out, double* nlZ_out,
                        double* dnlZ_out, int* sweeps_out, pgp_fitc** handle_out);

/* ---- learned inducing inputs: the FITC fits with the gradient w.r.t. xu ------------------------------------------------------
 * pgp_fitc_fit / pgp_fitc_ep_fit_lik with one more output: dxu_out (nu, d) row-major like xu, d nlZ / d xu (NULL: exactly the
 * plain entry points, which forward here).  Written with want = 3 and dnlZ_out set; every other output is bit-identical to a call
 * without it.  One adjoint matrix serves all nu d coordinates: two more nu x n x nu GEMMs and one fused contraction (csrc/fitc_xu.hip).
 * Kernels that are a function k(s) of one scaled squared distance: RBF, RBFunit, RBFard, RQ, RQard, Matern d = 3, 5, 7.  Any other
 * kind (programs, Matern d = 1, PiecePoly, Periodic, Gabor, Const, Noise, SM, ...) with dxu_out set returns
 * PGP_ERR_XU_UNSUPPORTED before any device work. */
#define PGP_ERR_XU_UNSUPPORTED (-92)
int pgp_fitc_fit_xu(pgp_ctx* ctx, int kind, const double* covhyp, int ncov, int para, int flags, double log_sn,
                    const double* xu, int64_t nu, const double* mvec, const double* dm, int nmean, int want,
                    double* alpha_out, double* L_out, double* nlZ_out, double* dnlZ_out, pgp_fitc** handle_out, double* dxu_out);
int pgp_fitc_ep_fit_lik_xu(pgp_ctx* ctx, int kind, const double* covhyp, int ncov, int para, int flags, int lik, const double* likhyp,
                           int nlik, int ref_compat, const double* xu, int64_t nu, const double* mvec, const double* dm, int nmean,
                           int want, int warm, double* ttau_io, double* tnu_io, double* alpha_out, double* L_out, double* nlZ_out,
                           double* dnlZ_out, int* sweeps_out, pgp_fitc** handle_out, double* dxu_out);

/* ---- ONE fit over the GPUs of a node (no reference counterpart: Core/inf.py:353-384 runs on one host) ---
 * One process per GPU, every rank calls with the same data (pgp_set_data) and arguments.  The factorisation is 1-D
 * block-cyclic over column panels; panels are broadcast over `comm`, alpha / nlZ / dnlZ come back identical on every
 * rank (csrc/sharded.hip).  Transports:
 *   pgp_comm_init_rccl: RCCL bound at run time (rccl_path: the librccl to dlopen, NULL = the system's); rank 0 makes the
 *                       128-byte id with pgp_comm_unique_id and hands it to the other ranks (any side channel).
 *   pgp_comm_init_host: call-backs that broadcast / all-reduce HOST buffers (op: 0 sum, 1 max; return 0 on success); the
 *                       library stages device memory through pinned host memory.  For MPI / gloo style transports and for
 *                       tests in which several ranks share one GPU. */
typedef struct pgp_comm pgp_comm;
typedef int (*pgp_host_bcast_fn)(void* user, void* buf, int64_t bytes, int root);
typedef int (*pgp_host_allreduce_fn)(void* user, double* buf, int64_t count, int op);
int pgp_comm_unique_id(const char* rccl_path, char* id_out /* 128 bytes */);
int pgp_comm_init_rccl(pgp_ctx* ctx, int world, int rank, const char* id /* 128 bytes */, const char* rccl_path,
                       pgp_comm** comm_out);
int pgp_comm_init_host(pgp_ctx* ctx, int world, int rank, pgp_host_bcast_fn bcast, pgp_host_allreduce_fn allreduce,
                       void* user, pgp_comm** comm_out);
void pgp_comm_free(pgp_comm* comm);
int pgp_comm_world(pgp_comm* comm);
int pgp_comm_rank(pgp_comm* comm);
/* Host collectives on the communicator: what the sharded restart search (Core/opt.py:301-327: init table + data out, one record
 * per restart back), the sharded K-fold loop (Validation/valid.py:20-66) and a sum of nlZ / dnlZ over independent data sets
 * (Demo/Clustering/pyGP_extension.py:54-64) exchange.  Buffers are HOST doubles; every rank calls with the same count.
 * RCCL transport: staged through a device buffer on the communicator's stream (ncclBroadcast / ncclAllReduce / ncclAllGather);
 * host transport: the call-backs.  pgp_comm_init_host accepts ctx = NULL for a communicator that only ever serves these
 * three (no device is touched).  allgather: recv holds world * count doubles, rank r's at recv + r * count.  op: 0 sum, 1 max. */
int pgp_comm_bcast_host(pgp_comm* comm, double* buf, int64_t count, int root);
int pgp_comm_allreduce_host(pgp_comm* comm, double* buf, int64_t count, int op);
int pgp_comm_allgather_host(pgp_comm* comm, const double* send, int64_t count, double* recv);
/* Arguments and results as pgp_exact_fit.  timings_out (optional, 10): ms of assembly, sweep, epilogue, total; device bytes
 * this call held at its peak; device bytes the posterior handle keeps; [6] ms the compute stream stalled waiting for a panel
 * (sum over the panels), [7] ms of the panel broadcasts from enqueue to complete on this rank (sum), [8] bytes this rank moved
 * in them, [9] the slowest single broadcast (ms) -- [6..9] are 0 at world size 1.  L_out (optional, (n,n) row-major, zero-filled by the
 * caller): THIS rank's columns of the factor in post.L's form (upper R, R'R = K/sn2 + I); the sum over the ranks is the whole
 * factor.  factor_out (optional): this rank's part of the distributed posterior (its column panels of L and of L^-T, alpha, the
 * coordinates) for pgp_sharded_predict.  Per-rank memory is O(n^2 / world): the panels, and for want = 3 the rank's column
 * strips of B^-1.  A rank that fails (out of memory, a launch error) makes EVERY rank return an error: its flag rides in the
 * collectives the others wait in.  (A sticky device fault, after which no HIP call succeeds, cannot enqueue that collective: the
 * failing rank then aborts the RCCL communicator so that the peers' collectives return with an error.) */
typedef struct pgp_sfactor pgp_sfactor;
int pgp_sharded_exact_fit(pgp_ctx* ctx, pgp_comm* comm, int kind, const double* covhyp, int ncov, int para, int flags,
                          double log_sn, const double* mvec, const double* dm, int nmean, int want, double* alpha_out,
                          double* nlZ_out, double* dnlZ_out, double* timings_out, double* L_out, pgp_sfactor** factor_out);
/* GP.predict (Core/gp.py:395-417) on the distributed posterior; every rank calls with the same test points (ns, d) and
 * receives the same fmu / fs2.  One all-reduce of ns doubles per batch of test points. */
int pgp_sharded_predict(pgp_ctx* ctx, pgp_comm* comm, pgp_sfactor* f, const double* xs, int64_t ns, const double* ms,
                        double* fmu, double* fs2);
void pgp_sfactor_free(pgp_ctx* ctx, pgp_sfactor* f);
int64_t pgp_sfactor_bytes(pgp_sfactor* f);

/* ---- helper functions: tools.jitchol / tools.solve_chol (Core/tools.py:31-97) ----------------
 * pgp_potrf: A (n,n) symmetric row-major in -> lower Cholesky factor (row-major, zeros above) out.
 * pgp_potrs: R (n,n) UPPER factor row-major, Bm (n,nrhs) row-major in -> X = (R'R)^-1 Bm out.   */
int pgp_potrf(pgp_ctx* ctx, const double* A, int64_t n, double* L_out);
int pgp_potrs(pgp_ctx* ctx, const double* R, int64_t n, const double* Bm, int64_t nrhs, double* X_out);

/* ---- measurement ------------------------------------------------------------------------------
 * Stage timings (ms, HIP events on the ctx stream) of the last fit, and -- when profiling is on --
 * per-kernel-class totals (launches, ms, algorithmic flops, algorithmic bytes).                 */
#define PGP_STAGE_ASSEMBLE 0
#define PGP_STAGE_POTRF 1
#define PGP_STAGE_SOLVE 2
#define PGP_STAGE_TRTRI 3
#define PGP_STAGE_LAUUM 4
#define PGP_STAGE_GRAD 5
#define PGP_STAGE_TOTAL 6
#define PGP_NSTAGE 7
int pgp_last_timings(pgp_ctx* ctx, double* ms_out /* PGP_NSTAGE */);
int pgp_set_profiling(pgp_ctx* ctx, int on);
int pgp_profile_classes(void);
const char* pgp_profile_class_name(int cls);
int pgp_profile_read(pgp_ctx* ctx, int cls, int64_t* launches, double* ms, double* flops, double* bytes);
int pgp_profile_reset(pgp_ctx* ctx);
/* tuning knobs (outer panel width of the blocked Cholesky, look-ahead on/off ...) */
int pgp_set_option(pgp_ctx* ctx, const char* name, int value);

#ifdef __cplusplus
}
#endif
#endif
