// Leave-one-out (LOO) predictive of a Gaussian-likelihood GP in closed form (Rasmussen & Williams 5.4.2; GPML infLOO; no
// counterpart in the reference, whose Validation/valid.py refits once per fold).  Everything starts from what the exact fit
// leaves on the device: B^-1 = E E' (B = K/sn2 + I, E = L^-T the fused inverse rows) and alpha.  With Kinv = B^-1 / sn2 and
// c_i = Kinv_ii:
//      mu_i = y_i - alpha_i / c_i     s2_i = 1 / c_i     lp_i = -1/2 log(2 pi) + 1/2 log c_i - alpha_i^2 / (2 c_i)
//      nlZ_loo = -sum lp_i            w_i = (1 + alpha_i^2 / c_i) / (2 c_i)              u = Kinv (alpha / c)
//      Q_loo = 2 Kinv diag(w) Kinv - u alpha' - alpha u'     takes the place of  Q = Kinv - alpha alpha'  in every gradient sum
// The gradient kernels (grad.hip, dense.hip) evaluate q = Binv[r, c] / sn2 - alpha[r] alpha[c]: handed S = sn2 Q_loo where they
// expect B^-1 and a zero vector where they expect alpha, they return the LOO gradients unchanged.  S = G G' - sn2 (u alpha' +
// alpha u') with G = sym(B^-1) diag(g), g_k = sqrt(2 w_k / sn2): one symmetric product on the fp64 MFMA tile.
//
//   loo_diag_upper_kernel     diag(B^-1)_i = sum_{k >= i} E(i,k)^2, fixed-order partials (the value-only route: no E E')
//   loo_stats_kernel          mu, s2, lp, w, alpha / c, g (0 on the padding), nlZ_loo: one workgroup, fixed order
//   loo_symv_kernel           u = Kinv v from the lower-triangle storage of B^-1: each stored 64 x 64 tile serves (I, J) and (J, I)
//   loo_mirror_scale_kernel   G = sym(B^-1) diag(g), full np x np; upper tiles transposed through LDS
//   loo_rank2_kernel          S -= sn2 (u alpha' + alpha u') on the lower triangle
#include <cmath>

#include "ctx.h"

namespace {

constexpr int LT = 64;          // tile edge of the symmetric matvec and the mirror
constexpr int LTP = LT + 1;     // LDS row stride in doubles.  ds_read_b64 is served in groups of 32 lanes over 64 four-byte banks
                                // (bank = (byte address / 4) mod 64): a column read T[lane][k] strides LTP doubles = 130 dwords = 2 mod
                                // 64, so the 32 lanes of a group land on 32 distinct bank pairs; a stride of 64 doubles would put them all
                                // on one.  Row accesses T[k][lane] are contiguous either way.

__device__ __forceinline__ double loo_block_sum(double v, double* red /* 4 doubles */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// partial[c*np + i] = sum_{k in chunk c, k >= i} E(i,k)^2   (E column-major upper triangular: coalesced over i)
__global__ __launch_bounds__(256) void loo_diag_upper_kernel(const double* __restrict__ E, long lde, long np, double* __restrict__ partial,
                                                             int nchunk) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    const long kc = (np + nchunk - 1) / nchunk;
    const long k0 = c * kc, k1 = k0 + kc < np ? k0 + kc : np;
    if (i >= np) return;
    double a4[4] = {0.0, 0.0, 0.0, 0.0};
    long k = (k0 > i ? k0 : i);
    for (; k + 4 <= k1; k += 4) {
        double e[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) e[q] = E[i + (k + q) * lde];
#pragma unroll
        for (int q = 0; q < 4; ++q) a4[q] = fma(e[q], e[q], a4[q]);
    }
    for (; k < k1; ++k) { const double e = E[i + k * lde]; a4[0] = fma(e, e, a4[0]); }
    partial[(long)c * np + i] = (a4[0] + a4[1]) + (a4[2] + a4[3]);
}
// y[i] = scale * sum_c partial[c*np + i], c ascending
__global__ __launch_bounds__(256) void loo_chunk_reduce_kernel(const double* __restrict__ partial, long np, int nchunk, double scale,
                                                               double* __restrict__ y) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    double acc = 0.0;
    for (int c = 0; c < nchunk; ++c) acc += partial[(long)c * np + i];
    y[i] = scale * acc;
}

// One workgroup.  cB = diag(B^-1) (np), alpha (np), yv = y (or y - m: then mu lacks m).  Outputs are np long, zero on the padding.
__global__ __launch_bounds__(256) void loo_stats_kernel(const double* __restrict__ cB, const double* __restrict__ alpha,
                                                        const double* __restrict__ yv, long n, long np, double sn2,
                                                        double* __restrict__ mu, double* __restrict__ s2, double* __restrict__ lp,
                                                        double* __restrict__ w, double* __restrict__ aoc, double* __restrict__ g,
                                                        double* __restrict__ nlz) {
    __shared__ double red[4];
    double acc = 0.0;
    for (long i = threadIdx.x; i < np; i += 256) {
        double vmu = 0.0, vs2 = 0.0, vlp = 0.0, vw = 0.0, vq = 0.0, vg = 0.0;
        if (i < n) {
            const double c = cB[i] / sn2, a = alpha[i];
            vq = a / c;
            vmu = yv[i] - vq;
            vs2 = 1.0 / c;
            vlp = -0.5 * log(2.0 * M_PI) + 0.5 * log(c) - 0.5 * a * vq;
            vw = (1.0 + a * vq) / (2.0 * c);
            vg = sqrt(2.0 * vw / sn2);
            acc += vlp;
        }
        mu[i] = vmu; s2[i] = vs2; lp[i] = vlp; w[i] = vw; aoc[i] = vq; g[i] = vg;      // g = 0 on the padding: B^-1 carries an identity there
    }
    const double tot = loo_block_sum(acc, red);
    if (threadIdx.x == 0) nlz[0] = -tot;
}

// Tile (I, J), I >= J, of the lower-triangle storage B(i,j) at B[i + j*ld]:  partial[J*np + I*64 + r] = sum_c B(I r, J c) v[J c]
// and, for I > J, partial[I*np + J*64 + c] = sum_r B(I r, J c) v[I r] (the mirrored half).  Every (slot, segment) pair is written
// by exactly one workgroup; the reduce adds the np / 64 slots in ascending order.
__global__ __launch_bounds__(256) void loo_symv_kernel(const double* __restrict__ B, long ld, long np, const double* __restrict__ v,
                                                       double* __restrict__ partial) {
    const int I = blockIdx.x, J = blockIdx.y;
    if (I < J) return;
    __shared__ double T[LT * LTP];          // T[c * LTP + r]
    __shared__ double part[4 * LT];
    __shared__ double vi[LT], vj[LT];
    const int t = threadIdx.x, lane = t & 63, q = t >> 6;
    const long i0 = (long)I * LT, j0 = (long)J * LT;
    for (int c = q; c < LT; c += 4) {
        double x = B[(i0 + lane) + (j0 + c) * ld];
        if (I == J && lane < c) x = B[(i0 + c) + (j0 + lane) * ld];       // diagonal tile: the stored half, mirrored
        T[c * LTP + lane] = x;
    }
    if (t < LT) { vi[t] = v[i0 + t]; vj[t] = v[j0 + t]; }
    __syncthreads();
    double s = 0.0;
    for (int c = q * 16; c < q * 16 + 16; ++c) s = fma(T[c * LTP + lane], vj[c], s);
    part[q * LT + lane] = s;
    __syncthreads();
    if (t < LT) partial[(long)J * np + i0 + t] = (part[t] + part[LT + t]) + (part[2 * LT + t] + part[3 * LT + t]);
    if (I == J) return;
    __syncthreads();
    s = 0.0;
    for (int r = q * 16; r < q * 16 + 16; ++r) s = fma(T[lane * LTP + r], vi[r], s);
    part[q * LT + lane] = s;
    __syncthreads();
    if (t < LT) partial[(long)I * np + j0 + t] = (part[t] + part[LT + t]) + (part[2 * LT + t] + part[3 * LT + t]);
}

// G(i,k) = sym(B)(i,k) g[k], full np x np, column-major.  Tile (I, K): on or below the diagonal the source tile is read as it is
// stored; above it the stored tile (K, I) is read along its columns and written out transposed through LDS, so that the global
// reads and the global writes both run along contiguous addresses.
__global__ __launch_bounds__(256) void loo_mirror_scale_kernel(const double* __restrict__ B, long ld, long np, const double* __restrict__ g,
                                                               double* __restrict__ G) {
    const int I = blockIdx.x, K = blockIdx.y;
    __shared__ double T[LT * LTP];
    const int t = threadIdx.x, lane = t & 63, q = t >> 6;
    const long i0 = (long)I * LT, k0 = (long)K * LT;
    if (I > K) {
        for (int k = q; k < LT; k += 4) G[(i0 + lane) + (k0 + k) * np] = B[(i0 + lane) + (k0 + k) * ld] * g[k0 + k];
        return;
    }
    // source tile (K, I): rows k0 + a (contiguous), columns i0 + b;  T[b * LTP + a]
    for (int b = q; b < LT; b += 4) T[b * LTP + lane] = B[(k0 + lane) + (i0 + b) * ld];
    __syncthreads();
    for (int k = q; k < LT; k += 4) {
        double x = T[lane * LTP + k];                                      // B(k0 + k, i0 + lane)
        if (I == K && lane >= k) x = T[k * LTP + lane];                    // diagonal tile: the stored half where i >= k
        G[(i0 + lane) + (k0 + k) * np] = x * g[k0 + k];
    }
}

// S(i,j) -= sn2 (u_i a_j + a_i u_j),  n > i >= j: one workgroup per 64 x 64 tile on or below the diagonal, 16 entries per thread,
// coalesced along i
__global__ __launch_bounds__(256) void loo_rank2_kernel(double* __restrict__ S, long ld, long n, const double* __restrict__ u,
                                                        const double* __restrict__ a, double sn2) {
    const int I = blockIdx.x, J = blockIdx.y;
    if (I < J) return;
    __shared__ double uj[LT], aj[LT];
    const int t = threadIdx.x, lane = t & 63, q = t >> 6;
    const long i = (long)I * LT + lane, j0 = (long)J * LT;
    if (t < LT) { const long j = j0 + t; uj[t] = j < n ? u[j] : 0.0; aj[t] = j < n ? a[j] : 0.0; }
    __syncthreads();
    if (i >= n) return;
    const double ui = u[i], ai = a[i];
    for (int k = q; k < LT; k += 4) {
        const long j = j0 + k;
        if (j > i || j >= n) continue;
        const double tt = fma(ui, aj[k], ai * uj[k]);
        S[i + j * ld] = fma(-sn2, tt, S[i + j * ld]);
    }
}

}  // namespace

// the pinned host image of a LOO fit's results (grow-only)
int loo_stage(pgp_ctx* c, size_t doubles) {
    if (c->loo_host && c->loo_host_cap >= doubles) return PGP_OK;
    (void)hipStreamSynchronize(c->st);
    if (c->loo_host) { (void)hipHostFree(c->loo_host); c->loo_host = nullptr; c->loo_host_cap = 0; }
    HIP_TRY(hipHostMalloc((void**)&c->loo_host, doubles * sizeof(double), hipHostMallocDefault));
    c->loo_host_cap = doubles;
    return PGP_OK;
}

long loo_buffer_doubles(long np) { return LOO_DEV_VECS * np + LOO_SCAL; }
long loo_symv_partial_doubles(long np) { return (np / LT) * np; }

// Stages 1 of the LOO tail (values).  E (np x np, upper triangular, column-major) when the fit ran the fused inverse, else null:
// then c->Binv holds B^-1 and its diagonal is read.  partial: >= 32 np doubles.
int loo_values_launch(pgp_ctx* c, long n, long np, double sn2, const double* E, long lde, const double* yv, const double* alpha,
                      double* partial, double* buf, hipStream_t st) {
    ProfScope ps(c, PC_SMALL, 0.0, E ? 4.0 * (double)np * np : 0.0, st);
    double* cB = loo_vec(buf, np, LOO_CDIAG);
    if (E) {
        const int nchunk = 32;
        hipLaunchKernelGGL(loo_diag_upper_kernel, dim3((unsigned)((np + 255) / 256), nchunk), dim3(256), 0, st, E, lde, np, partial, nchunk);
        hipLaunchKernelGGL(loo_chunk_reduce_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, partial, np, nchunk, 1.0, cB);
    } else {
        CHK(gather_strided_launch(c->Binv, np + 1, np, cB, st));
    }
    hipLaunchKernelGGL(loo_stats_kernel, dim3(1), dim3(256), 0, st, cB, alpha, yv, n, np, sn2, loo_vec(buf, np, LOO_MU),
                       loo_vec(buf, np, LOO_S2), loo_vec(buf, np, LOO_LP), loo_vec(buf, np, LOO_W), loo_vec(buf, np, LOO_AOC),
                       loo_vec(buf, np, LOO_G), buf + LOO_HOST_VECS * np);
    return hipGetLastError() == hipSuccess ? PGP_OK : PGP_ERR_HIP;
}

// Stages 2 to 5: u, G, S = G G' - sn2 (u alpha' + alpha u') over c->Binv (lower triangle).  c->Binv holds B^-1 on entry; G is
// np x np of scratch, symv_partial loo_symv_partial_doubles(np).  The product is profiled in lauum's class, PC_GEMM_LAUUM, beside
// E E' (tests/test_gpu_sweep_census.py pins the set of class names): np^3 flops where the launches of E E' add up to np^3 / 3.
int loo_gradient_matrix(pgp_ctx* c, long n, long np, double sn2, const double* alpha, double* buf, double* G, double* symv_partial,
                        hipStream_t st) {
    const unsigned nt = (unsigned)(np / LT);
    double* u = loo_vec(buf, np, LOO_U);
    {
        ProfScope ps(c, PC_SMALL, 0.0, 4.0 * (double)np * np + 16.0 * (double)np * np, st);
        hipLaunchKernelGGL(loo_symv_kernel, dim3(nt, nt), dim3(256), 0, st, c->Binv, np, np, loo_vec(buf, np, LOO_AOC), symv_partial);
        hipLaunchKernelGGL(loo_chunk_reduce_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, symv_partial, np, (int)nt,
                           1.0 / sn2, u);
        hipLaunchKernelGGL(loo_mirror_scale_kernel, dim3(nt, nt), dim3(256), 0, st, c->Binv, np, np, loo_vec(buf, np, LOO_G), G);
        if (hipGetLastError() != hipSuccess) return PGP_ERR_HIP;
    }
    GemmArgs g{};
    g.A = G; g.lda = np; g.a_kc = 0;
    g.B = G; g.ldb = np; g.b_kc = 0;
    g.C = c->Binv; g.ldc = np;
    g.M = (int)np; g.N = (int)np; g.K = (int)np; g.alpha = 1.0; g.beta = 0.0;
    g.tri = 2; g.mask_diag = 1; g.kmode = KM_FULL; g.koff = 0;          // G is full: no structural zeros to clip, unlike eet_lower's E
    const long t128 = (np / 128) * (np / 128 + 1) / 2;
    g.tile = t128 < c->small_tile_below ? 64 : 128;
    g.flops = (double)np * np * np;
    CHK(gemm_prof(c, PC_GEMM_LAUUM, g, st));
    {
        ProfScope ps(c, PC_SMALL, 0.0, 8.0 * (double)n * n, st);                  // (bytes: the lower triangle read and written)
        const unsigned ntl = (unsigned)((n + LT - 1) / LT);
        hipLaunchKernelGGL(loo_rank2_kernel, dim3(ntl, ntl), dim3(256), 0, st, c->Binv, np, n, u, alpha, sn2);
    }
    return hipGetLastError() == hipSuccess ? PGP_OK : PGP_ERR_HIP;
}
