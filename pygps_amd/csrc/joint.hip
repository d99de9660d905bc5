// The joint posterior of the (alpha, sW, L) parametrisation (Core/gp.py:395-417 stops at the marginals): with V = L^-1 (sW o Ks)
//     fmu  = ms + Ks' alpha                       as pgp_predict
//     fcov = Kss - V'V                            Kss = k(xs, xs) in 'train' mode, diag(fcov) = pgp_predict's fs2
//     A    = fcov + (noise + jitter) I = Lc Lc'   potrf_blocked, then one guarded Newton step on the factor (joint_refine)
//     F    = fmu 1' + Lc Z                        Z (ns, nsamp) standard normal, drawn by the caller
// All ns <= PGP_JOINT_MAX_POINTS points are ONE batch of predict.hip's batch body (predict_batch: either form of V, np x nsp
// column-major with exact zeros on its padding), so fmu and the diagonal are the bits pgp_predict gives for the same batch.  The
// flops are three launches of the fp64 MFMA GEMM family (V, V'V, Lc Z) and one Cholesky sweep; the kernels of this file are the
// O(ns^2) passes between them.
#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "testhooks.h"

namespace {

// One pass over the 64 x 64 tiles of the nsp x nsp column-major C whose LOWER tiles hold Kss - V'V (or a caller's matrix); blockIdx =
// (tile row, tile column).  Lower tiles: the diagonal comes from dv (pgp_predict's fs2, clipped at 0; null: C's own), the tile is
// mirrored into the upper triangle of C (what cov_out downloads) and A = C + add I is written for the factorisation with identity on
// the padding diagonal and zeros on the padding rows and columns.  Strictly upper tiles: zeros in A.  A may be null (no factor wanted).
__global__ __launch_bounds__(256) void joint_finish_kernel(double* __restrict__ C, long ld, long ns, const double* __restrict__ dv, double add,
                                                           double* __restrict__ A) {
    const long i0 = 64L * blockIdx.x, j0 = 64L * blockIdx.y;
    const int a = threadIdx.x & 63, b = threadIdx.x >> 6;
    if (blockIdx.x < blockIdx.y) {
        if (A) for (int q = b; q < 64; q += 4) A[i0 + a + (j0 + q) * ld] = 0.0;
        return;
    }
    __shared__ double tile[64][65];
    for (int q = b; q < 64; q += 4) tile[q][a] = C[i0 + a + (j0 + q) * ld];          // tile[q][a] = C(i0 + a, j0 + q)
    __syncthreads();
    const bool diag = blockIdx.x == blockIdx.y;
    for (int q = b; q < 64; q += 4) {
        const long i = i0 + a, j = j0 + q;
        const bool live = i < ns && j < ns;
        double vc = live ? tile[q][a] : 0.0, va = vc;
        if (diag && a < q) { vc = live ? tile[a][q] : 0.0; va = 0.0; }             // above the diagonal: the mirror in C, zero in A
        else if (diag && a == q) {
            if (live) { vc = dv ? fmax(dv[i], 0.0) : vc; va = vc + add; }
            else va = 1.0;
        }
        C[i + j * ld] = vc;
        if (A) A[i + j * ld] = va;
    }
    if (diag) return;
    for (int q = b; q < 64; q += 4) {                                                // C(j0 + a, i0 + q) = C(i0 + q, j0 + a)
        const long i = j0 + a, j = i0 + q;
        C[i + j * ld] = (i < ns && j < ns) ? tile[a][q] : 0.0;
    }
}

// dv[i] = max(Kss_ii - s_i, 0): the clamp of pgp_predict_dense, on the device (s = the raw column sums of squares)
__global__ __launch_bounds__(256) void joint_diag_sub_kernel(const double* __restrict__ Kss, long ld, const double* __restrict__ s, long ns,
                                                             double* __restrict__ dv) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < ns) dv[i] = fmax(Kss[i + i * ld] - s[i], 0.0);
}

// the sweep leaves whatever it computed above the diagonal of a 128 x 128 diagonal block: zeros there (one block per workgroup),
// so that the k-clipped product Lc Z and the download read a clean lower triangle
__global__ __launch_bounds__(256) void joint_clean_diag_kernel(double* __restrict__ L, long ld) {
    double* D = L + 128L * blockIdx.x * (ld + 1);
    for (int e = threadIdx.x; e < 128 * 128; e += 256) {
        const int i = e & 127, j = e >> 7;
        if (i < j) D[i + (long)j * ld] = 0.0;
    }
}

// T (row-major lower, leading dimension ld) <- L (column-major lower): T[i ld + j] = L(i, j) for j <= i, zeros above.  64 x 64 tiles
// through LDS; blockIdx = (tile row, tile column) of L.
__global__ __launch_bounds__(256) void joint_lower_rowmajor_kernel(const double* __restrict__ L, long ld, double* __restrict__ T) {
    __shared__ double tile[64][65];
    const long i0 = 64L * blockIdx.x, j0 = 64L * blockIdx.y;
    const int a = threadIdx.x & 63, b = threadIdx.x >> 6;
    const bool lower = blockIdx.x >= blockIdx.y, diag = blockIdx.x == blockIdx.y;
    for (int q = b; q < 64; q += 4) tile[q][a] = (lower && (!diag || a >= q)) ? L[i0 + a + (j0 + q) * ld] : 0.0;     // L(i0 + a, j0 + q)
    __syncthreads();
    for (int q = b; q < 64; q += 4) T[(i0 + q) * ld + j0 + a] = tile[a][q];                                          // L(i0 + q, j0 + a)
}

// out (ns, nsamp) row-major = F (column-major, leading dimension ld) + mu 1'   (mu null: zero mean)
__global__ __launch_bounds__(256) void add_col_mean_kernel(const double* __restrict__ F, long ld, long ns, long nsamp, const double* __restrict__ mu,
                                                           double* __restrict__ out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= ns * nsamp) return;
    const long m = e / nsamp, j = e % nsamp;
    out[e] = F[m + j * ld] + (mu ? mu[m] : 0.0);
}

// E = C + add I on the live part, identity on the padding diagonal: the matrix that was factorised, whole (both triangles)
__global__ __launch_bounds__(256) void joint_refine_init_kernel(const double* __restrict__ C, long ld, long ns, double add, double* __restrict__ E) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= ld) return;
    E[i + j * ld] = C[i + j * ld] + (i == j ? (i < ns ? add : 1.0) : 0.0);
}
// T = X' (64 x 64 tiles through LDS; blockIdx = tile row, tile column of X)
__global__ __launch_bounds__(256) void joint_transpose_kernel(const double* __restrict__ X, long ld, double* __restrict__ T) {
    __shared__ double tile[64][65];
    const long i0 = 64L * blockIdx.x, j0 = 64L * blockIdx.y;
    const int a = threadIdx.x & 63, b = threadIdx.x >> 6;
    for (int q = b; q < 64; q += 4) tile[q][a] = X[i0 + a + (j0 + q) * ld];
    __syncthreads();
    for (int q = b; q < 64; q += 4) T[j0 + a + (i0 + q) * ld] = tile[a][q];
}
// *out = max |Y_ij| as the bit pattern of a non-negative double (they order like unsigned integers; a NaN sorts above every number)
__global__ __launch_bounds__(256) void joint_maxabs_kernel(const double* __restrict__ Y, long ld, unsigned long long* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    unsigned long long v = i < ld ? (unsigned long long)__double_as_longlong(fabs(Y[i + j * ld])) : 0ull;
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long w = __shfl_down(v, o); v = w > v ? w : v; }
    if ((threadIdx.x & 63) == 0 && v) atomicMax(out, v);
}
// Y <- Phi(Y): the strictly lower triangle, half the diagonal, zeros above
__global__ __launch_bounds__(256) void joint_phi_kernel(double* __restrict__ Y, long ld) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= ld) return;
    if (i < j) Y[i + j * ld] = 0.0;
    else if (i == j) Y[i + j * ld] *= 0.5;
}

struct JointEvents {                       // the call's own timing events: the fit's stage timers (c->ev, c->last_ms) stay as they are
    hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int init() { for (auto& x : e) HIP_TRY(hipEventCreate(&x)); return PGP_OK; }
    ~JointEvents() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
    void read(double* out) const {
        if (!out) return;
        for (int s = 0; s < 5; ++s) { float ms = 0.f; (void)hipEventElapsedTime(&ms, e[s], e[s + 1]); out[s] = ms; }
    }
};

struct JointOut {
    double noise, jitter; const double* Z; long nsamp;
    double *cov_out, *chol_out, *samples_out, *stage_ms_out;
};

int check_out(const JointOut& o) { return (o.samples_out && (o.nsamp < 1 || !o.Z)) ? -8 : PGP_OK; }

// C -= scale V'V on the lower tiles: the TN form of lauum_lower without its k-clip, K = np.  Profiled in lauum's class: the set of
// class names is pinned by the recorded launch census (tests/test_gpu_sweep_census.py), so the launch has no class of its own
int joint_vtv(pgp_ctx* c, const double* V, long np, double scale, double* Cd, long nsp) {
    GemmArgs g{};
    g.A = V; g.lda = np; g.a_kc = 1;
    g.B = V; g.ldb = np; g.b_kc = 1;
    g.C = Cd; g.ldc = nsp;
    g.M = (int)nsp; g.N = (int)nsp; g.K = (int)np; g.alpha = -scale; g.beta = 1.0;
    g.tri = 2; g.mask_diag = 1; g.kmode = KM_FULL;
    const long t128 = (nsp / 128) * (nsp / 128 + 1) / 2;
    g.tile = t128 < c->small_tile_below ? 64 : 128;
    g.flops = (double)nsp * (double)nsp * (double)np;
    return gemm_prof(c, PC_GEMM_LAUUM, g);
}

// One Newton step on the factor.  The sweep's panel solves multiply by explicit inverses of 16 x 16 pivot blocks, which on a badly
// conditioned matrix (a latent covariance with a jitter of 1e-8) leaves a componentwise residual |A - L L'| / |L| |L|' an order of
// magnitude above a substitution-based Cholesky's.  With E = A - L L' (fp64, as accurate as that residual can be measured),
//     L <- L + L Phi(L^-1 E L^-T),      Phi = strictly lower triangle + half the diagonal
// solves (L + dL)(L + dL)' = A to first order in E; the two triangular solves act on the small E, so their own error is of second
// order.  Four launches of GEMM size (E, two blocked solves, the update): ~12 x the flops of the sweep, at GEMM rates.
// A = C + add I (C symmetric, zero padding).  *Lio: in the clean lower factor, out the refined one (another scratch buffer).
int joint_refine(pgp_ctx* c, PoolScratch& tmp, const double* Cd, double add, long ns, long nsp, double** Lio) {
    hipStream_t st = c->st;
    const double* L = *Lio;
    double *E = nullptr, *T = nullptr, *Wd = nullptr;
    CHK(tmp.alloc(&E, (size_t)nsp * nsp * sizeof(double)));
    CHK(tmp.alloc(&T, (size_t)nsp * nsp * sizeof(double)));
    CHK(tmp.alloc(&Wd, (size_t)128 * nsp * sizeof(double)));
    const dim3 gridE((unsigned)((nsp + 255) / 256), (unsigned)nsp), grid64((unsigned)(nsp / 64), (unsigned)(nsp / 64));
    const int tile = (nsp / 128) * (nsp / 128) < c->small_tile_below ? 64 : 128;
    hipLaunchKernelGGL(joint_refine_init_kernel, gridE, dim3(256), 0, st, Cd, nsp, ns, add, E);
    if (hipGetLastError() != hipSuccess) return PGP_ERR_HIP;
    GemmArgs g{};                                  // E -= L L'   (L(j, k) = 0 for k > j: k clipped)
    g.A = L; g.lda = nsp; g.a_kc = 0;
    g.B = L; g.ldb = nsp; g.b_kc = 0;
    g.C = E; g.ldc = nsp;
    g.M = (int)nsp; g.N = (int)nsp; g.K = (int)nsp; g.alpha = -1.0; g.beta = 1.0;
    // 64-tiles whatever the size: E is what is left of A after the cancellation, and it has to be right to a few ulps of |L| |L|'.
    // Measured at ns = 300 (latent, jitter 1e-8): with E on 64-tiles the refined factor's residual is 1.9e-15 (numpy's: 1.8e-15), with
    // E on the LDS-DMA 128-tile 6.9e-14 -- above the unrefined 2.0e-14.  Why that tile's sum is less accurate is not known.
    g.kmode = KM_LT_J; g.koff = 0; g.tile = 64;
    g.flops = (double)nsp * (double)nsp * (double)nsp;
    CHK(gemm_prof(c, PC_GEMM_INNER, g));
    CHK(leaf_inv_launch(L, nsp, Wd, 128, 128L * 128L, (int)(nsp / 128), st));
    CHK(solve_lower_multi(c, L, nsp, Wd, E, nsp, nsp, (int)nsp, false));           // E <- L^-1 E
    hipLaunchKernelGGL(joint_transpose_kernel, grid64, dim3(256), 0, st, E, nsp, T);
    if (hipGetLastError() != hipSuccess) return PGP_ERR_HIP;
    CHK(solve_lower_multi(c, L, nsp, Wd, T, nsp, nsp, (int)nsp, false));           // T <- L^-1 (L^-1 E)' = L^-1 E L^-T
    // The guard: the step is first order in Y = L^-1 E L^-T and what it leaves behind is of size |Phi|^2 <= (nsp max|Y|)^2 relative to
    // A.  It is taken only where that is below the max|Y| it removes, nsp^2 max|Y| <= 1 (a factor of a well enough conditioned A:
    // max|Y| is 1e-15 ... 1e-11 on the cases measured); on a barely positive definite A, where the sweep came through with pivots at
    // rounding level and Y is not small, or on anything that is not finite, the sweep's own factor stays.
    unsigned long long* ymax = nullptr;
    CHK(tmp.alloc(&ymax, sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(ymax, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(joint_maxabs_kernel, gridE, dim3(256), 0, st, T, nsp, ymax);
    if (hipGetLastError() != hipSuccess) return PGP_ERR_HIP;
    unsigned long long bits = 0;
    HIP_TRY(hipMemcpyAsync(&bits, ymax, sizeof(bits), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    double ym;
    memcpy(&ym, &bits, sizeof(ym));
    if (!(ym * (double)nsp * (double)nsp <= 1.0)) return PGP_OK;          // (*Lio untouched)
    hipLaunchKernelGGL(joint_phi_kernel, gridE, dim3(256), 0, st, T, nsp);
    if (hipGetLastError() != hipSuccess) return PGP_ERR_HIP;
    GemmArgs h{};                                  // E <- L + L Phi   (B(j, k) = Phi(k, j) = T[k + j ld]; exact zeros above the diagonal)
    h.A = L; h.lda = nsp; h.a_kc = 0;
    h.B = T; h.ldb = nsp; h.b_kc = 1;
    h.C = E; h.ldc = nsp; h.Cin = L; h.ldcin = nsp;
    h.M = (int)nsp; h.N = (int)nsp; h.K = (int)nsp; h.alpha = 1.0; h.beta = 1.0;
    h.kmode = KM_LT_I; h.koff = 0; h.tile = tile;
    h.flops = (double)nsp * (double)nsp * (double)nsp;
    CHK(gemm_prof(c, PC_GEMM_INNER, h));
    *Lio = E;
    return PGP_OK;
}

// Steps 4 to 6 on C (nsp x nsp column-major, lower tiles valid; overwritten): finish, factorise, draw, download.  dv / mu: device
// vectors of ns doubles or null.  ev[3] has been recorded by the caller in front of this; ev[4], ev[5] are recorded here.
// h_z: pinned staging of ns * nsamp doubles (samples wanted).  Returns > 0: the first non-positive pivot, capped at ns.
int joint_tail(pgp_ctx* c, PoolScratch& tmp, double* Cd, long ns, long nsp, const double* dv, const double* mu, const JointOut& o,
               double* h_z, const JointEvents& ev) {
    hipStream_t st = c->st;
    const bool factor = o.chol_out || o.samples_out;
    double *Ad = nullptr, *pack = nullptr;
    if (factor) {
        CHK(tmp.alloc(&Ad, (size_t)nsp * nsp * sizeof(double)));
        CHK(tmp.alloc(&pack, (size_t)(nsp / 128) * PACK_DOUBLES * sizeof(double)));
    }
    const dim3 grid64((unsigned)(nsp / 64), (unsigned)(nsp / 64));
    hipLaunchKernelGGL(joint_finish_kernel, grid64, dim3(256), 0, st, Cd, nsp, ns, dv, o.noise + o.jitter, Ad);
    if (hipGetLastError() != hipSuccess) return PGP_ERR_HIP;
    auto fetch_cov = [&]() -> int {                 // behind the factorisation's event: stage 4 times the sweep alone
        if (o.cov_out)
            HIP_TRY(hipMemcpy2DAsync(o.cov_out, ns * sizeof(double), Cd, nsp * sizeof(double), ns * sizeof(double), ns, hipMemcpyDeviceToHost, st));
        return PGP_OK;
    };
    if (!factor) {
        HIP_TRY(hipEventRecord(ev.e[4], st));
        CHK(fetch_cov());
        HIP_TRY(hipEventRecord(ev.e[5], st));
        HIP_TRY(hipStreamSynchronize(st));
        return PGP_OK;
    }
    HIP_TRY(hipMemsetAsync(c->info_dev, 0, sizeof(int), st));
    double* pack_save = c->inv16;                  // the blocked driver takes the per-leaf operand images from the ctx
    c->inv16 = pack;
    SweepJob job{Ad, nsp, nsp, nsp};
    const int rc = potrf_blocked(c, job);
    c->inv16 = pack_save;
    CHK(rc);
    if (job.join) HIP_TRY(hipStreamWaitEvent(st, job.join, 0));
    int info = 0;
    HIP_TRY(hipMemcpyAsync(&info, c->info_dev, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (info != 0) {
        HIP_TRY(hipEventRecord(ev.e[4], st));
        CHK(fetch_cov());
        HIP_TRY(hipStreamSynchronize(st));         // (cov_out arrives whatever the pivots say)
        return info > (int)ns ? (int)ns : info;
    }
    hipLaunchKernelGGL(joint_clean_diag_kernel, dim3((unsigned)(nsp / 128)), dim3(256), 0, st, Ad, nsp);
    if (hipGetLastError() != hipSuccess) return PGP_ERR_HIP;
    if (c->joint_refine) CHK(joint_refine(c, tmp, Cd, o.noise + o.jitter, ns, nsp, &Ad));
    HIP_TRY(hipEventRecord(ev.e[4], st));
    CHK(fetch_cov());
    if (o.chol_out) {                              // C is free now: it takes the row-major image of Lc
        hipLaunchKernelGGL(joint_lower_rowmajor_kernel, grid64, dim3(256), 0, st, Ad, nsp, Cd);
        HIP_TRY(hipMemcpy2DAsync(o.chol_out, ns * sizeof(double), Cd, nsp * sizeof(double), ns * sizeof(double), ns, hipMemcpyDeviceToHost, st));
    }
    if (hipGetLastError() != hipSuccess) return PGP_ERR_HIP;
    if (o.samples_out) {
        const long nsamp = o.nsamp, nzp = round_up(nsamp, 128);
        double *Zd = nullptr, *Fd = nullptr, *Fo = nullptr;
        CHK(tmp.alloc(&Zd, (size_t)nsp * nzp * sizeof(double)));
        CHK(tmp.alloc(&Fd, (size_t)nsp * nzp * sizeof(double)));
        CHK(tmp.alloc(&Fo, (size_t)ns * nsamp * sizeof(double)));
        // Z (ns, nsamp) row-major is the GEMM's B operand as it stands, B(j, k) = Z[k nsamp + j]; zero padding in both directions
        memcpy(h_z, o.Z, (size_t)ns * nsamp * sizeof(double));
        HIP_TRY(hipMemsetAsync(Zd, 0, (size_t)nsp * nzp * sizeof(double), st));
        HIP_TRY(hipMemcpy2DAsync(Zd, nzp * sizeof(double), h_z, nsamp * sizeof(double), nsamp * sizeof(double), ns, hipMemcpyHostToDevice, st));
        GemmArgs g{};                              // F = Lc Z, k clipped to the triangle
        g.A = Ad; g.lda = nsp; g.a_kc = 0;
        g.B = Zd; g.ldb = nzp; g.b_kc = 0;
        g.C = Fd; g.ldc = nsp;
        g.M = (int)nsp; g.N = (int)nzp; g.K = (int)nsp; g.alpha = 1.0; g.beta = 0.0;
        g.kmode = KM_LT_I; g.koff = 0;
        g.tile = (nsp / 128) * (nzp / 128) < c->small_tile_below ? 64 : 128;
        g.flops = (double)nsp * (double)nsp * (double)nzp;
        CHK(gemm_prof(c, PC_GEMM_INNER, g));
        hipLaunchKernelGGL(add_col_mean_kernel, dim3((unsigned)((ns * nsamp + 255) / 256)), dim3(256), 0, st, Fd, nsp, ns, nsamp, mu, Fo);
        if (hipGetLastError() != hipSuccess) return PGP_ERR_HIP;
        HIP_TRY(hipStreamSynchronize(st));         // (h_z has been consumed: it takes the result)
        HIP_TRY(hipMemcpyAsync(h_z, Fo, (size_t)ns * nsamp * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipEventRecord(ev.e[5], st));
    HIP_TRY(hipStreamSynchronize(st));
    if (o.samples_out) memcpy(o.samples_out, h_z, (size_t)ns * o.nsamp * sizeof(double));
    return PGP_OK;
}

// Step 1 of pgp_predict_joint: every test point as ONE batch of predict.hip's batch body.  On return (work queued on c->st, nothing
// synchronised) *V is np x nsp column-major, o1 = fmu, o2 = fs2 and XcT the scaled coordinates (dpad x nsp).
struct CrossV { double *V = nullptr, *XcT = nullptr, *o1 = nullptr, *o2 = nullptr; bool product = false; CovSpec cp; };
int joint_cross_v(pgp_ctx* c, pgp_factor* f, PoolScratch& tmp, const double* xs, long ns, const double* ms, size_t extra_stage, CrossV& out) {
    hipStream_t st = c->st;
    const long np = f->np, nsp = round_up(ns, 128);
    const int d = f->d, dpad = f->dpad;
    out.product = predict_takes_product(c, f, ns);
    if (out.product) CHK(ensure_linv(c, f));
    else CHK(ensure_wd(c, f));
    double *xd = nullptr, *scd = nullptr, *Ks = nullptr, *Vp = nullptr, *part = nullptr, *msd = nullptr;
    CHK(tmp.alloc(&xd, (size_t)nsp * d * sizeof(double)));
    CHK(tmp.alloc(&out.XcT, (size_t)dpad * nsp * sizeof(double)));
    CHK(tmp.alloc(&scd, dpad * sizeof(double)));
    CHK(tmp.alloc(&Ks, (size_t)np * nsp * sizeof(double)));
    if (out.product) {
        CHK(tmp.alloc(&Vp, (size_t)np * nsp * sizeof(double)));
        CHK(tmp.alloc(&part, (size_t)16 * nsp * sizeof(double)));
    }
    CHK(tmp.alloc(&msd, nsp * sizeof(double)));
    CHK(tmp.alloc(&out.o1, nsp * sizeof(double)));
    CHK(tmp.alloc(&out.o2, nsp * sizeof(double)));
    CHK(pred_stage(c, (size_t)nsp * (d + 2) + d + extra_stage));
    double* const h_x = c->pred_host, *const h_ms = h_x + (size_t)nsp * d, *const h_sc = h_ms + 2 * nsp;      // (h_ms + nsp: fmu on its way back)
    memcpy(h_sc, f->cs.scale.data(), d * sizeof(double));
    HIP_TRY(hipMemcpyAsync(scd, h_sc, d * sizeof(double), hipMemcpyHostToDevice, st));
    memcpy(h_x, xs, (size_t)ns * d * sizeof(double));
    HIP_TRY(hipMemcpyAsync(xd, h_x, (size_t)ns * d * sizeof(double), hipMemcpyHostToDevice, st));
    if (ms) {
        memcpy(h_ms, ms, ns * sizeof(double));
        HIP_TRY(hipMemcpyAsync(msd, h_ms, ns * sizeof(double), hipMemcpyHostToDevice, st));
    } else HIP_TRY(hipMemsetAsync(msd, 0, ns * sizeof(double), st));
    CHK(scale_transpose_launch(xd, ns, d, scd, out.XcT, nsp, dpad, st));
    out.cp = f->cs;
    out.cp.cp.der = -1; out.cp.pg.der = -1;
    CHK(predict_batch(c, f, out.cp, out.product, 0, out.XcT, nsp, ns, (int)nsp, msd, Ks, Vp, part, out.o1, out.o2, st));
    out.V = out.product ? Vp : Ks;
    return PGP_OK;
}

}  // namespace

extern "C" {

int pgp_predict_joint(pgp_ctx* c, pgp_factor* f, const double* xs, int64_t ns, const double* ms, double noise, double jitter,
                      const double* Z, int64_t nsamp, double* fmu, double* cov_out, double* chol_out, double* samples_out,
                      double* stage_ms_out) {
    if (!c) return -1;
    GateShared device_gate_hold(c);
    if (!f) return -2;
    if (!xs) return -3;
    if (ns < 1 || ns > PGP_JOINT_MAX_POINTS) return -4;
    if (!fmu) return -6;
    const JointOut o{noise, jitter, Z, (long)nsamp, cov_out, chol_out, samples_out, stage_ms_out};
    CHK(check_out(o));
    if (f->cs.has_pre()) return -13;                  // cov.Pre carries no k(xs, xs)
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->st;
    const long np = f->np, nsp = round_up(ns, 128);
    JointEvents ev;
    CHK(ev.init());
    PoolScratch tmp(c);
    double* Cd = nullptr;
    CHK(tmp.alloc(&Cd, (size_t)nsp * nsp * sizeof(double)));
    const size_t nz = samples_out ? (size_t)ns * nsamp : 0;
    HIP_TRY(hipEventRecord(ev.e[0], st));
    CrossV cv;
    CHK(joint_cross_v(c, f, tmp, xs, ns, ms, nz, cv));
    double* const h_o1 = c->pred_host + (size_t)nsp * (f->d + 1), *const h_z = c->pred_host + (size_t)nsp * (f->d + 2) + f->d;
    HIP_TRY(hipMemcpyAsync(h_o1, cv.o1, ns * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ev.e[1], st));
    // Kss in 'train' mode on the batch's own scaled coordinates (cov.Noise: sf2 I); its diagonal is replaced by fs2 in the finish pass
    HIP_TRY(hipMemsetAsync(Cd, 0, (size_t)nsp * nsp * sizeof(double), st));
    {
        ProfScope ps(c, PC_ASSEMBLE, 0.0, 8.0 * (double)ns * ns);
        CHK(cov_sym_launch(cv.XcT, nsp, ns, f->dpad, cv.cp, Cd, st, nsp));
    }
    HIP_TRY(hipEventRecord(ev.e[2], st));
    CHK(joint_vtv(c, cv.V, np, f->sWv ? 1.0 : f->sw * f->sw, Cd, nsp));
    HIP_TRY(hipEventRecord(ev.e[3], st));
    const int rc = joint_tail(c, tmp, Cd, ns, nsp, cv.o2, cv.o1, o, h_z, ev);
    if (rc < 0) return rc;
    memcpy(fmu, h_o1, ns * sizeof(double));           // (joint_tail has synchronised the stream, also in front of a pivot status)
    if (rc == PGP_OK) ev.read(stage_ms_out);
    if (c->prof) prof_collect(c);
    return rc;
}

int pgp_predict_joint_dense(pgp_ctx* c, pgp_factor* f, const double* Ks_host, const double* Kss_host, int64_t ns, const double* ms,
                            double noise, double jitter, const double* Z, int64_t nsamp, double* fmu, double* cov_out, double* chol_out,
                            double* samples_out, double* stage_ms_out) {
    if (!c) return -1;
    GateShared device_gate_hold(c);
    if (!f) return -2;
    if (!Ks_host) return -3;
    if (!Kss_host) return -4;
    if (ns < 1 || ns > PGP_JOINT_MAX_POINTS) return -5;
    if (!fmu) return -11;
    const JointOut o{noise, jitter, Z, (long)nsamp, cov_out, chol_out, samples_out, stage_ms_out};
    CHK(check_out(o));
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->st;
    CHK(ensure_wd(c, f));
    const long np = f->np, n = f->n, nsp = round_up(ns, 128);
    JointEvents ev;
    CHK(ev.init());
    PoolScratch tmp(c);
    double *Ks = nullptr, *msd = nullptr, *o1 = nullptr, *o2 = nullptr, *dv = nullptr, *Cd = nullptr;
    CHK(tmp.alloc(&Ks, (size_t)np * nsp * sizeof(double)));
    CHK(tmp.alloc(&msd, nsp * sizeof(double)));
    CHK(tmp.alloc(&o1, nsp * sizeof(double)));
    CHK(tmp.alloc(&o2, nsp * sizeof(double)));
    CHK(tmp.alloc(&dv, nsp * sizeof(double)));
    CHK(tmp.alloc(&Cd, (size_t)nsp * nsp * sizeof(double)));
    CHK(pred_stage(c, (size_t)ns * (samples_out ? nsamp + 1 : 1)));
    double* const h_o1 = c->pred_host, *const h_z = h_o1 + ns;
    std::vector<double> blk((size_t)ns * n);                   // column j of the device block = test point j
    for (long i = 0; i < n; ++i)
        for (long j = 0; j < ns; ++j) blk[(size_t)j * n + i] = Ks_host[(size_t)i * ns + j];
    HIP_TRY(hipEventRecord(ev.e[0], st));
    HIP_TRY(hipMemsetAsync(Ks, 0, (size_t)np * nsp * sizeof(double), st));
    HIP_TRY(hipMemcpy2DAsync(Ks, np * sizeof(double), blk.data(), n * sizeof(double), n * sizeof(double), ns, hipMemcpyHostToDevice, st));
    if (ms) HIP_TRY(hipMemcpyAsync(msd, ms, ns * sizeof(double), hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemsetAsync(msd, 0, ns * sizeof(double), st));
    CHK(predict_dense_block(c, f, Ks, ns, (int)nsp, msd, o1, o2));      // Ks <- V, o2 = the raw column sums of squares
    HIP_TRY(hipMemcpyAsync(h_o1, o1, ns * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ev.e[1], st));
    // symmetric input: row-major == column-major
    HIP_TRY(hipMemsetAsync(Cd, 0, (size_t)nsp * nsp * sizeof(double), st));
    HIP_TRY(hipMemcpy2DAsync(Cd, nsp * sizeof(double), Kss_host, ns * sizeof(double), ns * sizeof(double), ns, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(joint_diag_sub_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st, Cd, nsp, o2, (long)ns, dv);
    if (hipGetLastError() != hipSuccess) return PGP_ERR_HIP;
    HIP_TRY(hipEventRecord(ev.e[2], st));
    CHK(joint_vtv(c, Ks, np, f->sWv ? 1.0 : f->sw * f->sw, Cd, nsp));
    HIP_TRY(hipEventRecord(ev.e[3], st));
    const int rc = joint_tail(c, tmp, Cd, ns, nsp, dv, o1, o, h_z, ev);
    if (rc < 0) return rc;
    memcpy(fmu, h_o1, ns * sizeof(double));
    if (rc == PGP_OK) ev.read(stage_ms_out);
    if (c->prof) prof_collect(c);
    return rc;
}

int pgp_sample_mvn(pgp_ctx* c, const double* A, int64_t ns, const double* mean, double jitter, const double* Z, int64_t nsamp,
                   double* chol_out, double* samples_out) {
    if (!c) return -1;
    GateShared device_gate_hold(c);
    if (!A) return -2;
    if (ns < 1 || ns > PGP_JOINT_MAX_POINTS) return -3;
    const JointOut o{0.0, jitter, Z, (long)nsamp, nullptr, chol_out, samples_out, nullptr};
    CHK(check_out(o));
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->st;
    const long nsp = round_up(ns, 128);
    JointEvents ev;
    CHK(ev.init());
    PoolScratch tmp(c);
    double *Cd = nullptr, *mu = nullptr;
    CHK(tmp.alloc(&Cd, (size_t)nsp * nsp * sizeof(double)));
    CHK(tmp.alloc(&mu, nsp * sizeof(double)));
    CHK(pred_stage(c, samples_out ? (size_t)ns * nsamp : 1));
    for (int s = 0; s < 4; ++s) HIP_TRY(hipEventRecord(ev.e[s], st));
    HIP_TRY(hipMemsetAsync(Cd, 0, (size_t)nsp * nsp * sizeof(double), st));
    HIP_TRY(hipMemcpy2DAsync(Cd, nsp * sizeof(double), A, ns * sizeof(double), ns * sizeof(double), ns, hipMemcpyHostToDevice, st));
    if (mean) HIP_TRY(hipMemcpyAsync(mu, mean, ns * sizeof(double), hipMemcpyHostToDevice, st));
    const int rc = joint_tail(c, tmp, Cd, ns, nsp, nullptr, mean ? mu : nullptr, o, c->pred_host, ev);
    if (c->prof && rc >= 0) prof_collect(c);
    return rc;
}

// ---- test hooks (testhooks.h) ------------------------------------------------------------------------------------------------
int pgp_test_joint_vpad(pgp_ctx* c, pgp_factor* f, const double* xs, int64_t ns, int* product_out, int64_t* nonzero_out) {
    if (!c || !f || !xs || ns < 1 || ns > PGP_JOINT_MAX_POINTS || !product_out || !nonzero_out) return -1;
    if (f->cs.has_pre()) return -13;
    GateShared device_gate_hold(c);
    HIP_TRY(hipSetDevice(c->device));
    const long np = f->np, n = f->n, nsp = round_up(ns, 128);
    PoolScratch tmp(c);
    CrossV cv;
    CHK(joint_cross_v(c, f, tmp, xs, ns, nullptr, 0, cv));
    std::vector<double> V((size_t)np * nsp);
    HIP_TRY(hipMemcpyAsync(V.data(), cv.V, V.size() * sizeof(double), hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    int64_t rows = 0, cols = 0, live = 0;
    for (long j = 0; j < nsp; ++j)
        for (long i = 0; i < np; ++i) {
            const bool zero = V[(size_t)j * np + i] == 0.0;
            if (j >= ns) cols += !zero;
            else if (i >= n) rows += !zero;
            else live += !zero;
        }
    *product_out = cv.product ? 1 : 0;
    nonzero_out[0] = rows; nonzero_out[1] = cols; nonzero_out[2] = live;
    return PGP_OK;
}

int pgp_test_pool_state(pgp_ctx* c, pgp_factor* f, int64_t* out9) {
    int64_t* out7 = out9;
    if (!c || !out9) return -1;
    out9[7] = (int64_t)c->scratch_out_bytes.load(); out9[8] = (int64_t)c->scratch_out_count.load();
    std::lock_guard<std::mutex> lk(c->pool_mu);
    out7[0] = (int64_t)c->pool_bytes; out7[1] = (int64_t)c->spool_bytes;
    out7[2] = (int64_t)c->pool.size(); out7[3] = (int64_t)c->spool.size();
    out7[4] = f && f->Wd; out7[5] = f && f->Linv; out7[6] = f && f->Eraw;
    return PGP_OK;
}

}  // extern "C"
