// Laplace's approximation on the device -- reference: Core/inf.py Laplace.evaluate :466-562, _Psi_line :224-233,
// Core/tools.py brentmin :121-272 (Numerical Recipes §10.2), Core/lik.py Erf / Gauss in Laplace mode :175-197, 274-293.
//
// The Newton iteration in f keeps everything on the device; per Newton step the host reads back one small record
// (Psi_new, the step size, the evaluation count, a W < 0 flag) for the convergence test:
//   B = I + sW sW' o K (ep_build_kernel on the resident K) -> blocked MFMA Cholesky (1024-wide panels, as ep_factor_only)
//   -> x = B^-1 (sW o K b) by solve_lower_multi forward / backward -> dalpha = b - sW o x - alpha, b = W o (f - m) + dlp
//   -> K dalpha ONCE: f(s) = f + s K dalpha, alpha(s) = alpha + s dalpha, so every line-search evaluation is one reduction
//      over n -> Brent's method in ONE single-workgroup kernel (lap_line_kernel), which leaves alpha, f, dlp, W in place.
// The posterior (alpha, sW, L) has EP's form, so the factor handle is built exactly like EP's and predict serves it unchanged.
// Gradients (inf.py:530-562), with Z = sW sW' o B^-1 and S = diag(sW):
//   g = diag(K - K Z K) / 2 = (K_ii - colsum((L^-1 S K)^2)) / 2: K diag(sW) rides as right-hand-side rows of the final
//   factorisation (SweepJob::R, EP's rhsp form), row i of it then holds column i of L^-1 S K;
//   u = dfhat - sW o B^-1 (sW o K dfhat), dfhat = g o d3lp;
//   dnlZ.cov[h] = 1/2 sum((R - alpha alpha') o dK_h), R = Z - u dlp' - dlp u' (the rank-2 term is the implicit part
//   u' dK_h dlp), written into c->Binv and summed by the exact fit's Hadamard reduce in one pass over every hyper-parameter.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "erf_lik.h"

namespace {

constexpr int LAP_LS = 1024;            // threads of the line-search / reduction workgroup
constexpr int LAP_MAXIT = 20;           // Newton steps (inf.py:470)

__device__ __forceinline__ void lap_lik(int lik, double sn2, double y, double f, double* lp, double* dlp, double* d2lp,
                                        double* d3lp) {
    if (lik == PGP_LIK_GAUSS) gauss_laplace_derivs(y, f, sn2, lp, dlp, d2lp, d3lp);
    else erf_laplace_derivs(y, f, lp, dlp, d2lp, d3lp);
}

// sum of v over the LAP_LS threads of the workgroup, fixed order, the result in every thread
__device__ __forceinline__ double lap_block_sum(double v, double* red /* LAP_LS / 64 */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < LAP_LS / 64; ++k) s += red[k];
    return s;
}

// The likelihood at f (one workgroup): dlp, W = -d2lp, optionally lp and d3lp; out[0] = sum lp, out[1] = alpha'(f - m)
// (alpha may be null: 0), out[2] = number of W_i < 0.  Padding entries (n <= i < np) of the vectors are set to 0.
__global__ __launch_bounds__(LAP_LS) void lap_eval_kernel(long n, long np, int lik, double sn2, const double* __restrict__ y,
                                                          const double* __restrict__ f, const double* __restrict__ m,
                                                          const double* __restrict__ alpha, double* __restrict__ lp_out,
                                                          double* __restrict__ dlp, double* __restrict__ W,
                                                          double* __restrict__ d3lp, double* __restrict__ out) {
    __shared__ double red[LAP_LS / 64];
    double slp = 0.0, saf = 0.0, nneg = 0.0;
    for (long i = threadIdx.x; i < np; i += LAP_LS) {
        if (i >= n) {
            dlp[i] = 0.0; W[i] = 0.0;
            if (lp_out) lp_out[i] = 0.0;
            if (d3lp) d3lp[i] = 0.0;
            continue;
        }
        double l, d1, d2, d3;
        lap_lik(lik, sn2, y[i], f[i], &l, &d1, &d2, d3lp ? &d3 : nullptr);
        dlp[i] = d1; W[i] = -d2;
        if (lp_out) lp_out[i] = l;
        if (d3lp) d3lp[i] = d3;
        slp += l;
        if (alpha) saf = fma(alpha[i], f[i] - m[i], saf);
        if (-d2 < 0.0) nneg += 1.0;
    }
    const double a = lap_block_sum(slp, red);
    const double b = lap_block_sum(saf, red);
    const double c = lap_block_sum(nneg, red);
    if (threadIdx.x == 0) { out[0] = a; out[1] = b; out[2] = c; }
}

// Newton step, O(n) head: sW = sqrt(W), b = W o (f - m) + dlp (inf.py:503-505); padding 0
__global__ __launch_bounds__(256) void lap_step_prep_kernel(long n, long np, const double* __restrict__ W, const double* __restrict__ f,
                                                            const double* __restrict__ m, const double* __restrict__ dlp,
                                                            double* __restrict__ sW, double* __restrict__ b) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    if (i >= n) { sW[i] = 0.0; b[i] = 0.0; return; }
    sW[i] = sqrt(W[i]);
    b[i] = fma(W[i], f[i] - m[i], dlp[i]);
}

// out = s o v on [0, np)
__global__ __launch_bounds__(256) void lap_scale_kernel(long np, const double* __restrict__ s, const double* __restrict__ v,
                                                        double* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < np) out[i] = s[i] * v[i];
}

// out = a - s o x - c  (c may be null): dalpha = b - sW o B^-1(sW o K b) - alpha (inf.py:505), u = dfhat - sW o B^-1(...)
__global__ __launch_bounds__(256) void lap_axpy_kernel(long np, const double* __restrict__ a, const double* __restrict__ s,
                                                       const double* __restrict__ x, const double* __restrict__ c,
                                                       double* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < np) out[i] = a[i] - s[i] * x[i] - (c ? c[i] : 0.0);
}

// Psi(s) = alpha(s)'(f(s) - m) / 2 - sum lp(y, f(s)), alpha(s) = alpha + s dalpha, f(s) = f + s K dalpha  (inf.py:224-233)
__device__ double lap_psi(double s, long n, int lik, double sn2, const double* __restrict__ y, const double* __restrict__ m,
                          const double* __restrict__ alpha, const double* __restrict__ f, const double* __restrict__ da,
                          const double* __restrict__ kda, double* red) {
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += LAP_LS) {
        const double ai = fma(s, da[i], alpha[i]);
        const double fi = fma(s, kda[i], f[i]);
        double l, d1, d2;
        lap_lik(lik, sn2, y[i], fi, &l, &d1, &d2, nullptr);
        acc += 0.5 * ai * (fi - m[i]) - l;
    }
    return lap_block_sum(acc, red);
}

// The line search of one Newton step: Brent's method on [0, smax] (Numerical Recipes §10.2, the method Core/tools.py:121-272
// states), with the reference's decision points -- both endpoints first, then the golden-section point; `fu <= fx` takes the new
// point; at most nmax evaluations; the endpoints checked against the minimum at the end.  Every thread runs the same scalar
// recurrence on the same broadcast sums.  As in the reference, the state handed on (alpha, f, dlp, W) is the one of the LAST
// point evaluated, the step size and objective returned are the minimum's.  res = [s, Psi(s), evaluations].
__global__ __launch_bounds__(LAP_LS) void lap_line_kernel(long n, long np, int lik, double sn2, const double* __restrict__ y,
                                                          const double* __restrict__ m, double* __restrict__ alpha,
                                                          double* __restrict__ f, const double* __restrict__ da,
                                                          const double* __restrict__ kda, double* __restrict__ dlp,
                                                          double* __restrict__ W, double smax, int nmax, double thr,
                                                          double* __restrict__ res) {
    __shared__ double red[LAP_LS / 64];
    auto psi = [&](double s) { return lap_psi(s, n, lik, sn2, y, m, alpha, f, da, kda, red); };
    const double eps = DBL_EPSILON, tol = fmax(thr, eps), seps = sqrt(eps);
    const double cg = 0.5 * (3.0 - sqrt(5.0));
    const double fa = psi(0.0), fb = psi(smax);
    int nf = 2;
    double a = 0.0, b = smax, v = a + cg * (b - a), w = v, x = v, d = 0.0, e = 0.0;
    double fx = psi(x);
    ++nf;
    double last = x;
    double fv = fx, fw = fx;
    double xm = 0.5 * (a + b), tol1 = seps * fabs(x) + tol / 3.0, tol2 = 2.0 * tol1;
    while (fabs(x - xm) > tol2 - 0.5 * (b - a)) {
        bool golden = true;
        if (fabs(e) > tol1) {                                 // try a parabola through x, w, v
            golden = false;
            double r = (x - w) * (fx - fv);
            double q = (x - v) * (fx - fw);
            double p = (x - v) * q - (x - w) * r;
            q = 2.0 * (q - r);
            if (q > 0.0) p = -p;
            q = fabs(q);
            const double etemp = e;
            e = d;
            if (fabs(p) < fabs(0.5 * q * etemp) && p > q * (a - x) && p < q * (b - x)) {
                d = p / q;
                const double u = x + d;
                if (u - a < tol2 || b - u < tol2) d = (xm - x >= 0.0 ? tol1 : -tol1);
            } else golden = true;
        }
        if (golden) {
            e = (x >= xm) ? a - x : b - x;
            d = cg * e;
        }
        const double u = x + (d >= 0.0 ? 1.0 : -1.0) * fmax(fabs(d), tol1);
        const double fu = psi(u);
        ++nf;
        last = u;
        if (fu <= fx) {
            if (u >= x) a = x; else b = x;
            v = w; fv = fw;
            w = x; fw = fx;
            x = u; fx = fu;
        } else {
            if (u < x) a = u; else b = u;
            if (fu <= fw || w == x) {
                v = w; fv = fw;
                w = u; fw = fu;
            } else if (fu <= fv || v == x || v == w) {
                v = u; fv = fu;
            }
        }
        xm = 0.5 * (a + b);
        tol1 = seps * fabs(x) + tol / 3.0;
        tol2 = 2.0 * tol1;
        if (nf >= nmax) break;
    }
    if (fa < fx && fa <= fb) { x = 0.0; fx = fa; }
    else if (fb < fx) { x = smax; fx = fb; }
    __syncthreads();                                          // every thread is through its last read of alpha and f
    for (long i = threadIdx.x; i < n; i += LAP_LS) {
        const double ai = fma(last, da[i], alpha[i]);
        const double fi = fma(last, kda[i], f[i]);
        double l, d1, d2;
        lap_lik(lik, sn2, y[i], fi, &l, &d1, &d2, nullptr);
        alpha[i] = ai; f[i] = fi; dlp[i] = d1; W[i] = -d2;
    }
    if (threadIdx.x == 0) { res[0] = x; res[1] = fx; res[2] = (double)nf; }
}

// g_i = (K_ii - sum_j Y(i, j)^2) / 2 with Y (column-major, ld np) = (L^-1 S K)' after the rhs sweep; dfhat = g o d3lp
__global__ __launch_bounds__(256) void lap_g_kernel(long n, long np, const double* __restrict__ K, const double* __restrict__ Y,
                                                    const double* __restrict__ d3lp, double* __restrict__ g,
                                                    double* __restrict__ dfhat) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    if (i >= n) { g[i] = 0.0; dfhat[i] = 0.0; return; }
    double s = 0.0;
    for (long j = 0; j < np; ++j) { const double t = Y[i + j * np]; s = fma(t, t, s); }
    const double gi = 0.5 * (K[i + i * np] - s);
    g[i] = gi;
    dfhat[i] = gi * d3lp[i];
}

// R = sW sW' o B^-1 - u dlp' - dlp u' in place of B^-1 (lower triangle, column-major, ld ldr)
__global__ __launch_bounds__(256) void lap_r_kernel(double* __restrict__ R, long ldr, long np, const double* __restrict__ sW,
                                                    const double* __restrict__ u, const double* __restrict__ dlp) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    const double si = sW[i], ui = u[i], di = dlp[i];
    for (long j = blockIdx.y; j <= i; j += gridDim.y)
        R[i + j * ldr] = fma(si * sW[j], R[i + j * ldr], -(ui * dlp[j] + di * u[j]));
}

struct LapWork {
    long n, np, ldf;
    double *Kd, *Vd, *F, *Wd, *rhs;
    double *alpha, *f, *m, *dlp, *W, *sW, *b, *da, *kda, *lp, *d3lp, *g, *dfhat, *u, *tmp, *res;
};

inline dim3 lap_grid1(long np) { return dim3((unsigned)((np + 255) / 256)); }
inline dim3 lap_grid2(long np) { return dim3((unsigned)((np + 255) / 256), (unsigned)std::min<long>(np, 65535)); }

// B = I + sW sW' o K into w.F and its Cholesky factor; with Y != nullptr K diag(sW) rides as right-hand-side rows (EP's rhsp
// form) and leaves (L^-1 S K)' in Y.  1024-wide panels for the plain factorisation (ep_factor_only).
int lap_factor(pgp_ctx* c, LapWork& w, double* Y) {
    hipStream_t st = c->st;
    const long np = w.np;
    HIP_TRY(hipMemsetAsync(c->info_dev, 0, sizeof(int), st));
    CHK(ep_build_launch(w.Kd, np, w.sW, w.F, w.ldf, Y, Y ? 1 : 0, st));
    if (Y) {
        CHK(zero_strip_launch(w.F, w.ldf, np, np, 128, st));
        SweepJob job{w.F, w.ldf, np, np + 128};
        job.R = Y; job.ldr = np; job.nrhs2 = np;
        CHK(potrf_blocked(c, job));
        CHK(zero_strip_launch(w.F, w.ldf, np, np, 128, st));         // the spare rows go back to the pool's contract
    } else {
        const int keep = c->nb_outer;
        if (keep == 0 && np >= 2048) c->nb_outer = 8;
        SweepJob job{w.F, w.ldf, np, np};
        const int prc = potrf_blocked(c, job);
        c->nb_outer = keep;
        CHK(prc);
    }
    return PGP_OK;
}

// x = B^-1 (s o v) into w.rhs column 0 (v, s device vectors of np): one matvec-free forward / backward solve pair
int lap_solve(pgp_ctx* c, LapWork& w, const double* s, const double* v) {
    hipStream_t st = c->st;
    const long np = w.np;
    HIP_TRY(hipMemsetAsync(w.rhs + np, 0, (size_t)127 * np * sizeof(double), st));
    hipLaunchKernelGGL(lap_scale_kernel, lap_grid1(np), dim3(256), 0, st, np, s, v, w.rhs);
    CHK(leaf_inv_launch(w.F, w.ldf, w.Wd, 128, 128L * 128L, (int)(np / 128), st));
    CHK(solve_lower_multi(c, w.F, w.ldf, w.Wd, w.rhs, np, np, 128, false));
    CHK(solve_lower_multi(c, w.F, w.ldf, w.Wd, w.rhs, np, np, 128, true));
    return PGP_OK;
}

}  // namespace

static int laplace_fit_core(pgp_ctx* c, const double* Kdense, int kind, const double* covhyp, int ncov, int para, int flags,
                            int lik, const double* likhyp, int nlik, const double* mvec, const double* dm, int nmean, int want,
                            int warm, double* alpha_io, double* sW_out, double* nlZ_out, double* dnlZ_out, int* steps_out,
                            double* trace_out, pgp_factor** factor_out, const GatherSrc* gk = nullptr) {
    if (!c) return -1;
    if (gk ? gk->n <= 0 : c->n <= 0) return -1;
    if (lik != PGP_LIK_ERF && lik != PGP_LIK_GAUSS) return -7;
    if (lik == PGP_LIK_GAUSS && (!likhyp || nlik != 1)) return -8;
    if (lik == PGP_LIK_ERF && nlik != 0) return -9;
    if (nmean > 0 && !dm) return -11;
    if (!alpha_io) return -14;
    GateShared gate(c);
    HIP_TRY(hipSetDevice(c->device));
    c->dense_ready = false;                          // the workspace (B^-1, alpha) is about to be rewritten
    hipStream_t st = c->st;
    // K: a device program over the resident x, a dense upload, or (gk) a principal submatrix gathered on the device (gpmc.hip)
    const long n = gk ? gk->n : c->n, d = c->d, np = gk ? round_up(n, 128) : c->np, ldf = gk ? np + 128 : c->ldf;
    const bool dense = Kdense != nullptr || gk != nullptr;
    const double* const y_dev = gk ? gk->y : c->y_dev;
    const double sn2 = lik == PGP_LIK_GAUSS ? exp(2.0 * likhyp[0]) : 1.0;
    CovSpec cp;
    if (dense) ncov = 0;
    else { const int rc = make_spec(c, kind, covhyp, ncov, para, flags, -1, d, cp); if (rc != PGP_OK) return rc == -11 ? -10 : rc; }
    CHK(ensure_workspace(c, np));
    double kss = 0.0;
    if (!dense && !cp.has_dot()) CHK(cov_point_value(c, cp, 2, &kss));          // only stored for predict (dot-product leaves: per point there)
    const long need = std::max<long>(hadamard_partial_count(np, ncov), np);
    if (want >= 3) CHK(ensure_partial(c, need));
    // phase times (host wall clock, every phase ends synchronised) and the factorisations' share of the Newton loop (events)
    double ph_ms[4] = {0.0, 0.0, 0.0, 0.0}, potrf_ms = 0.0;
    auto tlast = std::chrono::steady_clock::now();
    auto stamp = [&](int phase) {
        const auto now = std::chrono::steady_clock::now();
        ph_ms[phase] += std::chrono::duration<double, std::milli>(now - tlast).count();
        tlast = now;
    };
    struct Events {
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    HIP_TRY(hipEventCreate(&ev.e[0]));
    HIP_TRY(hipEventCreate(&ev.e[1]));
    LapWork w{};
    w.n = n; w.np = np; w.ldf = ldf;
    const size_t nn = (size_t)np * np * sizeof(double);
    PoolScratch pscr(c);
    CHK(pscr.alloc(&w.Kd, nn));
    if (want >= 3) CHK(pscr.alloc(&w.Vd, nn));
    CHK(pscr.alloc(&w.Wd, (size_t)128 * np * sizeof(double)));
    CHK(pscr.alloc(&w.rhs, (size_t)128 * np * sizeof(double)));
    double* vecs = nullptr;
    const int nvec = 17;
    CHK(pscr.alloc(&vecs, (size_t)nvec * np * sizeof(double)));
    HIP_TRY(hipMemsetAsync(vecs, 0, (size_t)nvec * np * sizeof(double), st));
    double** slots[] = {&w.alpha, &w.f, &w.m, &w.dlp, &w.W, &w.sW, &w.b, &w.da, &w.kda, &w.lp, &w.d3lp, &w.g, &w.dfhat, &w.u,
                        &w.tmp, &w.res};
    for (size_t k = 0; k < sizeof(slots) / sizeof(slots[0]); ++k) *slots[k] = vecs + (long)k * np;
    HIP_TRY(hipMemsetAsync(w.Kd, 0, nn, st));
    CHK(alloc_factor_buffer(c, np, ldf, &w.F));
    FactorGuard fguard(c, w.F, (size_t)ldf * np * sizeof(double), /*scrub=*/true);
    // ---- K (full symmetric, padded with zeros) --------------------------------------------------------------------
    CHK(assemble_train_k(c, cp, Kdense, gk, n, np, w.Kd, st));
    if (gk) HIP_TRY(hipMemcpyAsync(w.m, gk->m, n * sizeof(double), hipMemcpyDeviceToDevice, st));       // gathered with K
    else if (mvec) HIP_TRY(hipMemcpyAsync(w.m, mvec, n * sizeof(double), hipMemcpyHostToDevice, st));
    double red[4];
    auto eval = [&](const double* alpha_or_null, bool with_d3) -> int {
        hipLaunchKernelGGL(lap_eval_kernel, dim3(1), dim3(LAP_LS), 0, st, n, np, lik, sn2, y_dev, w.f, w.m, alpha_or_null,
                           w.lp, w.dlp, w.W, with_d3 ? w.d3lp : nullptr, w.res);
        HIP_TRY(hipMemcpyAsync(red, w.res, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return PGP_OK;
    };
    // ---- start (inf.py:474-497) ----------------------------------------------------------------------------------
    double Psi_new;
    bool cold = true;
    if (warm) {                                       // the last alpha: f = K alpha + m
        HIP_TRY(hipMemcpyAsync(w.alpha, alpha_io, n * sizeof(double), hipMemcpyHostToDevice, st));
        CHK(col_dot_full_launch(w.Kd, np, np, np, w.alpha, w.m, w.f, st));
        CHK(eval(w.alpha, false));
        Psi_new = 0.5 * red[1] - red[0];
        // the reference's "objective for default init f == m" (inf.py:486-487) is the first element of -lp(y, m): vargout[0] of
        // the negated vector, not its sum.  Restated as it is, so that a warm call takes the branches the reference takes.
        double lp0, d1, d2, y0;
        HIP_TRY(hipMemcpy(&y0, y_dev, sizeof(double), hipMemcpyDeviceToHost));
        const double m0 = mvec ? mvec[0] : 0.0;
        if (lik == PGP_LIK_GAUSS) gauss_laplace_derivs(y0, m0, sn2, &lp0, &d1, &d2, nullptr);
        else erf_laplace_derivs(y0, m0, &lp0, &d1, &d2, nullptr);
        cold = !std::isfinite(Psi_new) || -lp0 < Psi_new;
    }
    if (cold) {
        HIP_TRY(hipMemsetAsync(w.alpha, 0, np * sizeof(double), st));
        HIP_TRY(hipMemcpyAsync(w.f, w.m, np * sizeof(double), hipMemcpyDeviceToDevice, st));
        CHK(eval(nullptr, false));
        Psi_new = -red[0];
    }
    bool wneg = red[2] > 0.0;
    stamp(0);
    // ---- Newton iteration in f (inf.py:499-512) -------------------------------------------------------------------
    const double tol = pow(10.0, -c->laplace_tol_exp), smax = 2.0, thr = 1e-4;
    const int nline = 20;
    double Psi_old = INFINITY;
    int it = 0;
    while (Psi_old - Psi_new > tol && it < LAP_MAXIT) {
        if (wneg) return PGP_ERR_LAPLACE_WNEG;        // the reference's LU / clamped-W branch is not restated
        Psi_old = Psi_new;
        ++it;
        hipLaunchKernelGGL(lap_step_prep_kernel, lap_grid1(np), dim3(256), 0, st, n, np, w.W, w.f, w.m, w.dlp, w.sW, w.b);
        HIP_TRY(hipEventRecord(ev.e[0], st));
        CHK(lap_factor(c, w, nullptr));
        HIP_TRY(hipEventRecord(ev.e[1], st));
        CHK(col_dot_full_launch(w.Kd, np, np, np, w.b, nullptr, w.tmp, st));            // K b
        CHK(lap_solve(c, w, w.sW, w.tmp));                                              // B^-1 (sW o K b)
        hipLaunchKernelGGL(lap_axpy_kernel, lap_grid1(np), dim3(256), 0, st, np, w.b, w.sW, w.rhs, w.alpha, w.da);
        CHK(col_dot_full_launch(w.Kd, np, np, np, w.da, nullptr, w.kda, st));           // K dalpha, once per step
        hipLaunchKernelGGL(lap_line_kernel, dim3(1), dim3(LAP_LS), 0, st, n, np, lik, sn2, y_dev, w.m, w.alpha, w.f, w.da,
                           w.kda, w.dlp, w.W, smax, nline, thr, w.res);
        // the W < 0 test of the next step (inf.py:512) rides in the same read-back
        hipLaunchKernelGGL(lap_eval_kernel, dim3(1), dim3(LAP_LS), 0, st, n, np, lik, sn2, y_dev, w.f, w.m,
                           (const double*)nullptr, w.lp, w.dlp, w.W, (double*)nullptr, w.res + 4);
        double rec[8];
        HIP_TRY(hipMemcpyAsync(rec, w.res, 8 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (hipGetLastError() != hipSuccess) return PGP_ERR_HIP;
        int info = 0;
        HIP_TRY(hipMemcpy(&info, c->info_dev, sizeof(int), hipMemcpyDeviceToHost));
        if (info != 0) return info > (int)n ? (int)n : info;
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        potrf_ms += ms;
        Psi_new = rec[1];
        wneg = rec[6] > 0.0;
        if (trace_out) { trace_out[3 * (it - 1)] = rec[0]; trace_out[3 * (it - 1) + 1] = rec[1]; trace_out[3 * (it - 1) + 2] = rec[2]; }
    }
    stamp(1);
    if (steps_out) *steps_out = it;
    // ---- posterior and nlZ at the final f (inf.py:514-529) -----------------------------------------------------------
    CHK(eval(w.alpha, true));
    if (red[2] > 0.0) return PGP_ERR_LAPLACE_WNEG;
    const double sum_lp = red[0], af = red[1];
    hipLaunchKernelGGL(lap_step_prep_kernel, lap_grid1(np), dim3(256), 0, st, n, np, w.W, w.f, w.m, w.dlp, w.sW, w.b);
    CHK(lap_factor(c, w, want >= 3 ? w.Vd : nullptr));
    CHK(logdet_ztz_launch(w.F, ldf, n, w.F, 0, c->scal, st));
    double sc[2];
    int info = 0;
    HIP_TRY(hipMemcpyAsync(sc, c->scal, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&info, c->info_dev, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (info != 0) return info > (int)n ? (int)n : info;
    const double nlZ = 0.5 * af + sc[0] - sum_lp;
    std::vector<double> alpha(n), sW(np, 0.0);
    HIP_TRY(hipMemcpyAsync(alpha.data(), w.alpha, n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(sW.data(), w.sW, np * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(alpha_io, alpha.data(), n * sizeof(double));
    if (sW_out) memcpy(sW_out, sW.data(), n * sizeof(double));
    if (nlZ_out) *nlZ_out = nlZ;
    // ---- derivatives (inf.py:530-562) -----------------------------------------------------------------------------
    if (want >= 3 && dnlZ_out) {
        hipLaunchKernelGGL(lap_g_kernel, lap_grid1(np), dim3(256), 0, st, n, np, w.Kd, w.Vd, w.d3lp, w.g, w.dfhat);
        CHK(col_dot_full_launch(w.Kd, np, np, np, w.dfhat, nullptr, w.tmp, st));        // K dfhat
        CHK(lap_solve(c, w, w.sW, w.tmp));
        hipLaunchKernelGGL(lap_axpy_kernel, lap_grid1(np), dim3(256), 0, st, np, w.dfhat, w.sW, w.rhs, (const double*)nullptr, w.u);
        // R = sW sW' o B^-1 - u dlp' - dlp u' into c->Binv, alpha into c->alpha_dev
        CHK(trtri_lower(c, w.F, ldf, c->W, np, c->T, np));
        CHK(lauum_lower(c, c->W, np, c->Binv, np, np));
        hipLaunchKernelGGL(lap_r_kernel, lap_grid2(np), dim3(256), 0, st, c->Binv, np, np, w.sW, w.u, w.dlp);
        HIP_TRY(hipMemcpyAsync(c->alpha_dev, w.alpha, np * sizeof(double), hipMemcpyDeviceToDevice, st));
        std::vector<double> gc(ncov + 1, 0.0);
        if (!dense) {
            CHK(hadamard_reduce_launch(c->XsT, np, n, np, c->dpad, cp, ncov, 1.0, c->Binv, np, c->alpha_dev, c->partial,
                                       c->scal + 8, st, nullptr));
            HIP_TRY(hipMemcpyAsync(gc.data(), c->scal + 8, (ncov + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        std::vector<double> u(n), g(n), Ku(n), f(n), y(n);
        HIP_TRY(hipMemcpyAsync(u.data(), w.u, n * sizeof(double), hipMemcpyDeviceToHost, st));
        if (lik == PGP_LIK_GAUSS) {
            CHK(col_dot_full_launch(w.Kd, np, np, np, w.u, nullptr, w.tmp, st));        // K u
            HIP_TRY(hipMemcpyAsync(Ku.data(), w.tmp, n * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(g.data(), w.g, n * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(f.data(), w.f, n * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(y.data(), y_dev, n * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
        for (int i = 0; i < nmean; ++i) {                                               // -(alpha + u)' dm_i
            double s = 0.0;
            for (long j = 0; j < n; ++j) s += (alpha[j] + u[j]) * dm[(long)i * n + j];
            dnlZ_out[i] = -s;
        }
        for (int h = 0; h < ncov; ++h) dnlZ_out[nmean + h] = 0.5 * gc[h];
        if (lik == PGP_LIK_GAUSS) {
            // lp_dhyp = (y - f)^2 / sn2 - 1, dlp_dhyp = 2 (f - y) / sn2, d2lp_dhyp = 2 / sn2 (lik.py:190-193)
            double s = 0.0;
            for (long j = 0; j < n; ++j) {
                const double r = y[j] - f[j];
                s += g[j] * (2.0 / sn2) + (r * r / sn2 - 1.0) + Ku[j] * (-2.0 * r / sn2);
            }
            dnlZ_out[nmean + ncov] = -s;
        }
    }
    if (c->prof) prof_collect(c);
    HIP_TRY(hipStreamSynchronize(st));
    stamp(2);
    c->last_ms[PGP_STAGE_ASSEMBLE] = ph_ms[0]; c->last_ms[PGP_STAGE_SOLVE] = ph_ms[1]; c->last_ms[PGP_STAGE_POTRF] = potrf_ms;
    c->last_ms[PGP_STAGE_GRAD] = ph_ms[2]; c->last_ms[PGP_STAGE_TRTRI] = 0.0; c->last_ms[PGP_STAGE_LAUUM] = 0.0;
    c->last_ms[PGP_STAGE_TOTAL] = ph_ms[0] + ph_ms[1] + ph_ms[2];
    if (factor_out) {                                 // EP's posterior handle, from the device: predict serves it unchanged
        CHK(finish_factor(c, n, np, ldf, fguard, dense ? nullptr : &cp, kss, 1.0, w.alpha, w.sW, hipMemcpyDeviceToDevice, factor_out));
    } else {
        HIP_TRY(hipStreamSynchronize(st));
        fguard.scrub = false;                         // a finished factor honours the pool contract (zeros above the diagonal)
    }
    if (dense && want >= 3) { c->dense_ready = true; c->dense_n = n; }
    return PGP_OK;
}

// Laplace on a principal submatrix of a covariance matrix that is already on the device (gpmc.hip): lik.Erf, cold start, want = 2
int laplace_fit_gathered(pgp_ctx* c, const GatherSrc& g, double* nlZ_out, int* steps_out, pgp_factor** factor_out) {
    if (!g.K_all || !g.idx || !g.y || !g.m || !g.m_all) return -2;
    std::vector<double> alpha(g.n, 0.0);
    return laplace_fit_core(c, nullptr, 0, nullptr, 0, 0, 0, PGP_LIK_ERF, nullptr, 0, nullptr, nullptr, 0, 2, 0, alpha.data(), nullptr,
                            nlZ_out, nullptr, steps_out, nullptr, factor_out, &g);
}

extern "C" int pgp_laplace_fit(pgp_ctx* c, int kind, const double* covhyp, int ncov, int para, int flags, int lik,
                               const double* likhyp, int nlik, const double* mvec, const double* dm, int nmean, int want, int warm,
                               double* alpha_io, double* sW_out, double* nlZ_out, double* dnlZ_out, int* steps_out,
                               double* trace_out, pgp_factor** factor_out) {
    if (!covhyp) return -3;
    return laplace_fit_core(c, nullptr, kind, covhyp, ncov, para, flags, lik, likhyp, nlik, mvec, dm, nmean, want, warm, alpha_io,
                            sW_out, nlZ_out, dnlZ_out, steps_out, trace_out, factor_out);
}

extern "C" int pgp_laplace_fit_dense(pgp_ctx* c, const double* K, int lik, const double* likhyp, int nlik, const double* mvec,
                                     const double* dm, int nmean, int want, int warm, double* alpha_io, double* sW_out,
                                     double* nlZ_out, double* dnlZ_out, int* steps_out, double* trace_out,
                                     pgp_factor** factor_out) {
    if (!K) return -2;
    return laplace_fit_core(c, K, 0, nullptr, 0, 0, 0, lik, likhyp, nlik, mvec, dm, nmean, want, warm, alpha_io, sW_out, nlZ_out,
                            dnlZ_out, steps_out, trace_out, factor_out);
}
