// Gradients of the FITC objectives w.r.t. the inducing inputs xu (Snelson & Ghahramani's pseudo-inputs; GPML's hyp.xu).  The
// reference's FITCOfKernel never differentiates w.r.t. xu: nothing here restates it.
//
// Both FITC gradient passes (fitc.hip: FITC_Exact, FITC_EP) end, per hyper-parameter, in a formula that is linear in (dKuu, dKu):
//   dnlZ = 1/2 (dk0 Sigma - w'R al - sum_j v_j al_j^2 - sum_j cw_j v_j - <R W', B W'>),  R = 2 dKu - dKuu B,  v = ddiagK - colsum(R o B).
// For a coordinate of xu, ddiagK = 0, so dnlZ = <G, R> with the adjoint
//   G = 1/2 (-w al' + B diag(al^2 + cw) - (B W') W)            (nu x n)
// and, expanding R,  dnlZ = <2 G, dKu> + <C, dKuu>,  C = -G B'  (nu x nu).  With k a function of the scaled squared distance s,
//   d nlZ / d u_jk = 2 scale_k [ sum_i 2 G_ji k'(s(u_j, x_i)) (u~_jk - x~_ik) + sum_l (C_jl + C_lj) k'(s(u_j, u_l)) (u~_jk - u~_lk) ]
// in scaled coordinates u~, x~: all nu x D entries from ONE adjoint -- two more nu x n x nu GEMMs and one fused pass that
// recomputes the distance tiles, instead of a loop over nu D "hyper-parameters".
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "ctx.h"
#include "testhooks.h"

namespace {

constexpr int XU_CT = 8;        // column tiles (of 64 points) per workgroup: fixed, so that the order of every sum is fixed
constexpr int XU_KS = 8;        // coordinates accumulated per workgroup: 4 x 8 running sums per thread (16 took every VGPR)

// One workgroup: 64 row points x up to XU_CT * 64 column points x the XU_KS coordinates of slab blockIdx.z.  Per 64 x 64 tile the
// scaled squared distances are recomputed in sqdist_tile's layout (thread t: rows 4 (t / 16) + a, columns 2 (t % 16) + e + 32 b),
// the weights A o k' are formed in registers (A is read once, 16 bytes at a time; the weighted tile never goes to memory) and
// every coordinate of the slab accumulates sum_i wt_ji (r_jk - c_ik) in the difference form.  The 16 threads of a tile row are
// then summed by a fixed butterfly, and the chunk's partial sums go to part[(chunk * dpad + k) * ldr + j]: no atomics.
// With D <= 8 there is one slab and A is read exactly once; each further slab of 8 coordinates reads it again.
__global__ __launch_bounds__(256) void fitc_xu_contract_kernel(const double* __restrict__ XrT, long ldr, long nr,
                                                               const double* __restrict__ XcT, long ldc, long ncols, int d, int dpad,
                                                               CovParams p, const double* __restrict__ A, long lda,
                                                               double* __restrict__ part) {
    __shared__ double sm[2 * SKC * ST];
    const int t = threadIdx.x, tr = t >> 4, tc = t & 15;
    const long r0 = (long)blockIdx.x * ST;
    const int k0 = (int)blockIdx.z * XU_KS;
    const long nct = (ncols + ST - 1) / ST;
    const long ct0 = (long)blockIdx.y * XU_CT, ct1 = ct0 + XU_CT < nct ? ct0 + XU_CT : nct;
    double* xr = sm;
    double* xc = sm + SKC * ST;
    double acc[4][XU_KS];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int k = 0; k < XU_KS; ++k) acc[a][k] = 0.0;
    for (long ct = ct0; ct < ct1; ++ct) {
        const long c0 = ct * ST;
        double s[4][4], wt[4][4];
        sqdist_tile(XrT, ldr, r0, XcT, ldc, c0, dpad, sm, s);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long col = c0 + 2 * tc + (q & 1) + 32 * (q >> 1);
            double av[4] = {0.0, 0.0, 0.0, 0.0};
            if (col < ncols) {
                const double* ap = A + col * lda + r0 + 4 * tr;
                const double2_t a01 = *(const double2_t*)ap, a23 = *(const double2_t*)(ap + 2);
                av[0] = a01[0]; av[1] = a01[1]; av[2] = a23[0]; av[3] = a23[1];
            }
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const bool live = col < ncols && r0 + 4 * tr + a < nr;           // padding points carry no weight
                wt[a][q] = live ? av[a] * cov_dvalue_ds(p, s[a][q]) : 0.0;
            }
        }
        // the slab's coordinates again (sqdist_tile leaves its last slab behind a barrier: safe to overwrite).  Padding points are
        // staged as zeros whatever the buffers hold there: their weight is a SELECTED zero above (a NaN distance cannot reach it),
        // and fma(0, finite, acc) leaves the live sums alone -- nothing relies on what the padding of XrT / XcT contains
        {
            const int k = t >> 5, pr = t & 31;            // 8 coordinates x 32 pairs of points = 256 double2 per side
            double2_t rr = *(const double2_t*)(XrT + (long)(k0 + k) * ldr + r0 + 2 * pr);
            double2_t cc = *(const double2_t*)(XcT + (long)(k0 + k) * ldc + c0 + 2 * pr);
            rr[0] = r0 + 2 * pr < nr ? rr[0] : 0.0;
            rr[1] = r0 + 2 * pr + 1 < nr ? rr[1] : 0.0;
            cc[0] = c0 + 2 * pr < ncols ? cc[0] : 0.0;
            cc[1] = c0 + 2 * pr + 1 < ncols ? cc[1] : 0.0;
            *(double2_t*)(xr + k * ST + 2 * pr) = rr;
            *(double2_t*)(xc + k * ST + 2 * pr) = cc;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < XU_KS; ++k) {
            if (k0 + k < d) {
                const double2_t r01 = *(const double2_t*)(xr + k * ST + 4 * tr);
                const double2_t r23 = *(const double2_t*)(xr + k * ST + 4 * tr + 2);
                const double2_t c01 = *(const double2_t*)(xc + k * ST + 2 * tc);
                const double2_t c23 = *(const double2_t*)(xc + k * ST + 2 * tc + 32);
                const double rv[4] = {r01[0], r01[1], r23[0], r23[1]};
                const double cv[4] = {c01[0], c01[1], c23[0], c23[1]};
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[a][k] = fma(wt[a][q], rv[a] - cv[q], acc[a][k]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int k = 0; k < XU_KS; ++k) {
            double v = acc[a][k];
            v += __shfl_xor(v, 1, 64);
            v += __shfl_xor(v, 2, 64);
            v += __shfl_xor(v, 4, 64);
            v += __shfl_xor(v, 8, 64);
            if (tc == 0) part[((long)blockIdx.y * dpad + k0 + k) * ldr + r0 + 4 * tr + a] = v;
        }
}

// out[j, k] = (prev ? prev[j, k] : 0) + 2 scale_k sum_chunk part[(chunk * dpad + k) * ldr + j]   (chunks in order)
__global__ __launch_bounds__(256) void fitc_xu_finish_kernel(const double* __restrict__ part, long ldr, long nr, int d, int dpad,
                                                             int nchunk, const double* __restrict__ scale,
                                                             const double* __restrict__ prev, double* __restrict__ out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nr * d) return;
    const long j = idx / d;
    const int k = (int)(idx - j * d);
    double s = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) s += part[((long)ch * dpad + k) * ldr + j];
    const double res = 2.0 * scale[k] * s;
    out[idx] = prev ? prev[idx] + res : res;
}

// R(j, i) <- R(j, i) - w_j al_i + B(j, i) (al_i^2 + cw_i) on the live part, zero on the padding:  R = -(B W') W  becomes  2 G
__global__ __launch_bounds__(256) void fitc_xu_adjoint_kernel(double* __restrict__ R, const double* __restrict__ Bm, long ld, long nrows,
                                                              long nu, long n, const double* __restrict__ w,
                                                              const double* __restrict__ al, const double* __restrict__ cw) {
    const long i = blockIdx.y;
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= nrows) return;
    double v = 0.0;
    if (j < nu && i < n) {
        const double a = al[i];
        v = R[j + i * ld] + (Bm[j + i * ld] * fma(a, a, cw[i]) - w[j] * a);
    }
    R[j + i * ld] = v;
}

// S = C + C'
__global__ __launch_bounds__(256) void fitc_xu_symmetrise_kernel(const double* __restrict__ Cm, double* __restrict__ S, long ld, long nrows) {
    const long l = blockIdx.y;
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= nrows) return;
    S[j + l * ld] = Cm[j + l * ld] + Cm[l + j * ld];
}

}  // namespace

bool fitc_xu_supported(int kind, int para) {
    switch (kind) {
        case PGP_COV_RBF: case PGP_COV_RBFARD: case PGP_COV_RBFUNIT: case PGP_COV_RQ: case PGP_COV_RQARD: return true;
        case PGP_COV_MATERN: return para != 1;       // d = 1: k'(s) is unbounded at s = 0 (every other `para` runs as d = 3, 5 or 7)
        default: return false;
    }
}

long fitc_xu_partial_doubles(long ldr, long ncols, int dpad) {
    const long nct = (ncols + ST - 1) / ST;
    return ((nct + XU_CT - 1) / XU_CT) * (long)dpad * ldr;
}

int fitc_xu_contract_launch(const double* XrT, long ldr, long nr, const double* XcT, long ldc, long ncols, int d, int dpad,
                            const CovSpec& cs, const double* A, long lda, const double* scale_dev, double* part, const double* prev,
                            double* out, hipStream_t st) {
    if (cs.prog || cs.sm || nr <= 0 || ncols <= 0 || d <= 0 || dpad % SKC) return -2;
    // every tile the kernel touches lies inside the padded buffers
    if (round_up(nr, ST) > ldr || round_up(nr, ST) > lda || round_up(ncols, ST) > ldc) return -2;
    // ... and every 16-byte load is aligned: even leading dimensions, 16-byte aligned bases
    if (((lda | ldr | ldc) & 1) || (((uintptr_t)A | (uintptr_t)XrT | (uintptr_t)XcT) & 15)) return -2;
    const long nct = (ncols + ST - 1) / ST;
    const int nchunk = (int)((nct + XU_CT - 1) / XU_CT);
    CovParams p = cs.cp;
    p.der = -1;
    dim3 grid((unsigned)((nr + ST - 1) / ST), (unsigned)nchunk, (unsigned)((d + XU_KS - 1) / XU_KS));     // slabs that hold a coordinate
    hipLaunchKernelGGL(fitc_xu_contract_kernel, grid, dim3(256), 0, st, XrT, ldr, nr, XcT, ldc, ncols, d, dpad, p, A, lda, part);
    hipLaunchKernelGGL(fitc_xu_finish_kernel, dim3((unsigned)((nr * d + 255) / 256)), dim3(256), 0, st, part, ldr, nr, d, dpad, nchunk,
                       scale_dev, prev, out);
    return hipGetLastError() == hipSuccess ? PGP_OK : PGP_ERR_HIP;
}

int fitc_xu_grad(pgp_ctx* c, const CovSpec& cs, long nu, long nup, const double* XuT, const double* Bm, const double* W,
                 const double* BW, const double* al_d, const double* cw_d, const double* w_d, double* R, double* Cm, double* Sm,
                 double* dxu_out) {
    hipStream_t st = c->st;
    const long n = c->n, np = c->np;
    const int d = (int)c->d, dpad = c->dpad;
    PoolScratch tmp(c);
    double *part = nullptr, *o1 = nullptr, *o2 = nullptr;
    CHK(tmp.alloc(&part, (size_t)std::max(fitc_xu_partial_doubles(nup, n, dpad), fitc_xu_partial_doubles(nup, nu, dpad)) * sizeof(double)));
    CHK(tmp.alloc(&o1, (size_t)nu * d * sizeof(double)));
    CHK(tmp.alloc(&o2, (size_t)nu * d * sizeof(double)));
    CHK(fitc_gemm(c, BW, nup, 0, W, nup, 1, R, nup, nup, np, nup, -1.0, 0.0));            // -(B W') W
    hipLaunchKernelGGL(fitc_xu_adjoint_kernel, dim3((unsigned)((nup + 255) / 256), (unsigned)np), dim3(256), 0, st, R, Bm, nup, nup,
                       nu, n, w_d, al_d, cw_d);                                           // R = 2 G
    CHK(fitc_gemm(c, R, nup, 0, Bm, nup, 0, Cm, nup, nup, nup, np, -0.5, 0.0));           // C = -G B'
    hipLaunchKernelGGL(fitc_xu_symmetrise_kernel, dim3((unsigned)((nup + 255) / 256), (unsigned)nup), dim3(256), 0, st, Cm, Sm, nup,
                       nup);
    HIP_TRY(hipGetLastError());
    // data columns first, then the inducing columns on top: a fixed order
    // profiled with the other passes that recompute distance tiles under a weight matrix (bytes: the weights, read once per slab)
    const double slabs = (double)((d + XU_KS - 1) / XU_KS);
    { ProfScope ps(c, PC_HADAMARD, 0.0, 8.0 * slabs * (double)nu * n + 8.0 * (double)(nu + n) * d, st);
      CHK(fitc_xu_contract_launch(XuT, nup, nu, c->XsT, np, n, d, dpad, cs, R, nup, c->scale_dev, part, nullptr, o1, st)); }
    { ProfScope ps(c, PC_HADAMARD, 0.0, 8.0 * slabs * (double)nu * nu + 16.0 * (double)nu * d, st);
      CHK(fitc_xu_contract_launch(XuT, nup, nu, XuT, nup, nu, d, dpad, cs, Sm, nup, c->scale_dev, part, o1, o2, st)); }
    HIP_TRY(hipMemcpyAsync(dxu_out, o2, (size_t)nu * d * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PGP_OK;
}

// self-test hook: the contraction alone with caller-given weights.  rows (nr, d), cols (ncols, d; NULL: the row points again, the
// inducing-against-inducing call), A (nr, ncols) row-major, all on the host; out (nr, d).  Needs no resident data.
extern "C" int pgp_test_fitc_xu_contract(pgp_ctx* c, int kind, const double* hyp, int ncov, int para, int flags, int64_t d,
                                         const double* rows, int64_t nr, const double* cols, int64_t ncols, const double* A,
                                         double* out) {
    if (!c) return -1;
    GateShared device_gate_hold(c);
    if (!hyp || !rows || !A || !out || d <= 0 || nr <= 0) return -2;
    if (!fitc_xu_supported(kind, para)) return PGP_ERR_XU_UNSUPPORTED;
    if (!cols) ncols = nr;
    if (ncols <= 0) return -2;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->st;
    CovSpec cs;
    CHK(make_spec(c, kind, hyp, ncov, para, flags, -1, (long)d, cs));
    const int dpad = (int)round_up((long)d, SKC);
    const long nrp = round_up(nr, 128), ncp = round_up(ncols, 128);
    std::vector<double> hA((size_t)nrp * ncp, 0.0);
    for (long j = 0; j < nr; ++j)
        for (long i = 0; i < ncols; ++i) hA[(size_t)i * nrp + j] = A[(size_t)j * ncols + i];
    PoolScratch tmp(c);
    double *xr = nullptr, *xc = nullptr, *XrT = nullptr, *XcT = nullptr, *scd = nullptr, *Ad = nullptr, *part = nullptr, *od = nullptr;
    CHK(tmp.alloc(&xr, (size_t)nr * d * sizeof(double)));
    CHK(tmp.alloc(&XrT, (size_t)dpad * nrp * sizeof(double)));
    CHK(tmp.alloc(&scd, (size_t)dpad * sizeof(double)));
    CHK(tmp.alloc(&Ad, hA.size() * sizeof(double)));
    CHK(tmp.alloc(&part, (size_t)fitc_xu_partial_doubles(nrp, ncols, dpad) * sizeof(double)));
    CHK(tmp.alloc(&od, (size_t)nr * d * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(scd, cs.scale.data(), (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(xr, rows, (size_t)nr * d * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(Ad, hA.data(), hA.size() * sizeof(double), hipMemcpyHostToDevice, st));
    CHK(scale_transpose_launch(xr, nr, (int)d, scd, XrT, nrp, dpad, st));
    if (cols) {
        CHK(tmp.alloc(&xc, (size_t)ncols * d * sizeof(double)));
        CHK(tmp.alloc(&XcT, (size_t)dpad * ncp * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(xc, cols, (size_t)ncols * d * sizeof(double), hipMemcpyHostToDevice, st));
        CHK(scale_transpose_launch(xc, ncols, (int)d, scd, XcT, ncp, dpad, st));
    }
    CHK(fitc_xu_contract_launch(XrT, nrp, nr, cols ? XcT : XrT, cols ? ncp : nrp, ncols, (int)d, dpad, cs, Ad, nrp, scd, part, nullptr,
                                od, st));
    HIP_TRY(hipMemcpyAsync(out, od, (size_t)nr * d * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PGP_OK;
}
