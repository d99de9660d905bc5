/* Self-test / calibration hooks of libpygps_amd.so: NOT part of the drop-in boundary (include/pygps_amd.h).  They are
 * exported for tests/, tools/ and bench.py's calibration legs only (pygps_amd/_lib.py: TEST_SIGNATURES). */
#pragma once
#include <stdint.h>

#include "../../include/pygps_amd.h"
#ifdef __cplusplus
extern "C" {
#endif
/* Column-major GEMM on host buffers through the fp64 MFMA kernel. */
int pgp_test_gemm(pgp_ctx* ctx, int tile, int a_kc, int b_kc, int tri, int mask_diag, int kmode, int koff,
                  double alpha, double beta, const double* A, int64_t lda, const double* B, int64_t ldb,
                  double* C, int64_t ldc, int M, int N, int K, int iters, double* ms_out);
int pgp_test_gemm_shrink(pgp_ctx* ctx, const double* Y, int64_t ldy, int M, int K, int w, int nb, int dm, int zero_from,
                         double* C, int64_t ldc, int64_t sC);
/* C = beta Cin + alpha A B' (Cin NULL: in place) with the k-clip of the trailing updates: first-touch rows from zero_from on,
   upper-trapezoidal there when zf_upper is set. */
int pgp_test_gemm_zskip(pgp_ctx* ctx, int tile, int tri, int mask_diag, int zero_from, int zf_upper, double alpha, double beta,
                        const double* A, int64_t lda, const double* B, int64_t ldb, const double* Cin, double* C, int64_t ldc,
                        int M, int N, int K);
/* two products in ONE launch (gemm_f64_pair_kernel): Ca = beta Ca + alpha A[:, :Ka] B[:, :Ka]', Cb the same with depth Kb */
int pgp_test_gemm_pair(pgp_ctx* ctx, double alpha, double beta, const double* A, int64_t lda, const double* B, int64_t ldb, double* Ca,
                       double* Cb, int64_t ldc, int M, int N, int Ka, int Kb);
/* C -= A B' on the lower tiles (packed, masked diagonal tiles) but those whose first row and column lie in [skip_lo, skip_hi); with
   wait_ms > 0 every workgroup waits inside the kernel for a device counter that the second stream raises wait_ms later. */
int pgp_test_gemm_skip_wait(pgp_ctx* ctx, int tile, const double* A, const double* B, double* C, int n, int K, int skip_lo,
                            int skip_hi, int wait_ms, int* timed_out);
int pgp_test_probit_hazard(pgp_ctx* ctx, const double* z, double* out, int n);
/* the Laplace-mode likelihood derivatives of the device (csrc/erf_lik.h) at host (y, f): out (4, n) rows lp, dlp, d2lp, d3lp.
   lik: PGP_LIK_ERF or PGP_LIK_GAUSS (log_sn used for Gauss only) */
int pgp_test_laplace_lik(pgp_ctx* ctx, int lik, double log_sn, const double* y, const double* f, int n, double* out);
/* lik.Laplace, EP mode (csrc/laplace_lik.h) on the device at host (y, mu, s2, sn) per site: out (4, n) rows lZ, dlZ, d2lZ, dlZhyp. */
int pgp_test_laplace_ep_lik(pgp_ctx* ctx, const double* y, const double* mu, const double* s2, const double* sn, int n, double* out);
int pgp_test_valu_peak(pgp_ctx* ctx, int iters, int waves_per_simd, double* out2);
int pgp_test_mfma_peak(pgp_ctx* ctx, int iters, double* tflops_out);
int pgp_test_mfma_cycles(pgp_ctx* ctx, int iters, int nacc, int waves_per_simd, double* out3);
int pgp_test_leaf_ticks(pgp_ctx* ctx, double* ticks_out /* 24 */);
int pgp_test_wave_costs(pgp_ctx* ctx, double* out16);
int pgp_test_slot_probe(pgp_ctx* ctx, int nwg, int lds_kb, int hold_us, int reserve, int probe_lds_kb, int delay_us, double* out4);
int pgp_test_cumask_gemm(pgp_ctx* ctx, int M, int K, int reserve_per_xcd, int stride, int iters, double* out2);
int pgp_test_assemble(pgp_ctx* ctx, int kind, int mode, int64_t n, int64_t d, int iters, double* ms_out);
/* the stores of the 'train' assembly alone (out3[0], ms), hipMemsetAsync (out3[1]) and a linear fill (out3[2]) over 8 n^2 bytes */
/* phase stamps (100 MHz) of every workgroup of one trailing-update launch: 8 words per workgroup, see GemmArgs::trace */
int pgp_test_gemm_trace(pgp_ctx* ctx, int M, int K, int tri, int warm, int conc, long long* out, int64_t out_words, int64_t* nblk_out);
int pgp_test_read_gemm_trace(pgp_ctx* ctx, long long* out, int64_t words, int64_t* nwg);
int pgp_test_store_roof(pgp_ctx* ctx, int64_t n, int grid, int iters, double* out3);
/* the fits' gradient pass (hadamard_reduce_launch) over the resident data of pgp_set_data: host Binv (n x n, symmetric), alpha,
   optional per-point weights wv (NULL: 1 / sn2); out[h] = sum_ij Q_ij dK_h,ij for h < ncov, out[ncov] = sn2 tr(Q) */
int pgp_test_hadamard(pgp_ctx* ctx, int kind, const double* hyp, int ncov, int para, int flags, const double* Binv,
                      const double* alpha, const double* wv, double sn2, double* out);
/* out2[0] = 1 if the context's two streams ran concurrently (a spinner on the panel stream saw a flag set from the main stream), out2[1] = us waited */
int pgp_test_stream_concurrency(pgp_ctx* ctx, int wait_us, double* out2);
/* gather_sym_kernel (csrc/gpmc.hip) on a host matrix K (n x n, row-major): Kd_out (np x np, np = n_idx rounded up to 128) with
   Kd_out[r, c] = K[idx[r], idx[c]] on the live part and zeros on the padding; y_out / m_out (np, optional): +1 for the first n_pos
   rows, -1 for the other live ones, and m_all[idx[r]] (m_all NULL: zeros) */
int pgp_test_gather_sym(pgp_ctx* ctx, const double* K, int64_t n, const int32_t* idx, int64_t n_idx, int64_t n_pos,
                        const double* m_all, double* Kd_out, double* y_out, double* m_out);
/* vote_accumulate_kernel / vote_normalise_kernel (csrc/gpmc.hip) for ONE pair (ci, cj) at host fmu, fs2 (ns each): votes_out
   (ns x n_class) before the normalisation, norm_out (optional) after it */
int pgp_test_vote(pgp_ctx* ctx, const double* fmu, const double* fs2, int64_t ns, int n_class, int ci, int cj, double* votes_out,
                  double* norm_out);
/* the device's yield table (capi.hip: one per device, shared by every context on it; 4096 words, one per CU key) read back to
   out4096 once the context's own streams are idle.  Reads only, launches nothing.  -2: the context has no table */
int pgp_test_yield_table(pgp_ctx* ctx, uint32_t* out4096);
/* step 1 of pgp_predict_joint (csrc/joint.hip) alone: V = L^-1 (sW o Ks) for the ns points as one batch, read back.  product_out:
   1 = the product form, 0 = the blocked solve; nonzero_out (3): entries that are not exact zeros in the padding rows n .. np of the
   live columns, in the padding columns ns .. nsp, and in the live part */
int pgp_test_joint_vpad(pgp_ctx* ctx, pgp_factor* f, const double* xs, int64_t ns, int* product_out, int64_t* nonzero_out);
/* out9: idle bytes of the factor pool and of the scratch pool, their buffer counts, whether the handle f (may be NULL) holds
   Wd, Linv, the fit's inverse rows, and the scratch-pool bytes and buffers that are OUT (taken by a call or held by a posterior
   handle, not yet given back: a call that leaks scratch leaves them above their value before it).  Reads host state only. */
int pgp_test_pool_state(pgp_ctx* ctx, pgp_factor* f, int64_t* out9);
/* B^-1 as the last want = 3 fit on this context left it in the workspace (lower triangle, leading dimension ws_np), mirrored into a
   symmetric row-major (n, n) host matrix once the context's streams are idle.  Reads only, launches nothing but the copy.
   -3: n rounded up to 128 is not the workspace's size */
int pgp_test_read_binv(pgp_ctx* ctx, int64_t n, double* out);
/* fitc_xu_contract_kernel (csrc/fitc_xu.hip) alone with caller-given weights: out[j, k] = 2 scale_k sum_i A[j, i] k'(s_ji)
   (rows~[j, k] - cols~[i, k]) for host rows (nr, d), cols (ncols, d; NULL: the rows again) and A (nr, ncols) row-major; out (nr, d).
   Needs no resident data.  PGP_ERR_XU_UNSUPPORTED for kinds without cov_dvalue_ds */
int pgp_test_fitc_xu_contract(pgp_ctx* ctx, int kind, const double* hyp, int ncov, int para, int flags, int64_t d, const double* rows,
                              int64_t nr, const double* cols, int64_t ncols, const double* A, double* out);
#ifdef __cplusplus
}
#endif
