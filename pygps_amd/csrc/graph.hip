// Graph node kernels and the k-nearest-neighbour graph (pyGPs/GraphExtensions/nodeKernels.py, graphUtil.py:29-46) on the device.
//
// pgp_node_kernel: from the dense adjacency matrix A (n x n, symmetric, no isolated node)
//     PGP_NODE_REGLAP  inv(I + sigma^2 L),  L = I - S,  S = D^-1/2 A D^-1/2        (nodeKernels.py:42-52)   p0 = sigma
//     PGP_NODE_VND     inv(I - alpha S)                                            (nodeKernels.py:83-98)   p0 = alpha
//     PGP_NODE_RW      (a I - L)^p by repeated squaring                            (nodeKernels.py:101-119) p0 = a, p1 = p
//     PGP_NODE_DIFF    exp(beta H), H = A - diag(row sums)                         (nodeKernels.py:66-80)   p0 = beta
// The inverses are the blocked Cholesky, the recursive triangular inverse and W'W of the fits (potrf_blocked, trtri_lower,
// lauum_lower): both matrices are symmetric positive definite (spectrum of S in [-1, 1]; alpha >= 1 shows as a non-positive
// pivot, returned like every other one).  Powers and the exponential are products on the fp64 MFMA GEMM: every factor is a
// polynomial in one symmetric matrix, so X Y = X Y' and the NT product the GEMM offers is the product wanted.  The
// exponential scales by 2^-s, with s from the 1-norm bound 2 |beta| max degree such that the scaled norm is <= 1/2, takes the
// Taylor polynomial of degree 18 by Horner's rule (remainder 0.5^19 / 19! = 1.6e-23) and squares s times.  No eigensolver.
//
// pgp_knn_graph: brute-force squared distances sum_k (x_ik - x_jk)^2 (difference form, as the reference's KD-tree compares
// them), the k smallest per row (the point itself left out; ties broken by the lower index), symmetrised with max.
#include <cmath>
#include <vector>

#include "ctx.h"

namespace {

constexpr int TAYLOR_DEGREE = 18;
constexpr int KNN_ROWS = 4, KNN_CHUNK = 512;

// cs[j] = sum_i A[i n + j]   (axis 0; one thread per column, coalesced across the workgroup)
__global__ __launch_bounds__(256) void col_sum_kernel(const double* __restrict__ A, long n, double* __restrict__ cs) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (long i = 0; i < n; ++i) s += A[i * n + j];
    cs[j] = s;
}
// rs[i] = sum_j A[i n + j]   (axis 1; one workgroup per row, fixed order)
__global__ __launch_bounds__(256) void row_sum_kernel(const double* __restrict__ A, long n, double* __restrict__ rs) {
    __shared__ double r[256];
    const long i = blockIdx.x;
    double s = 0.0;
    for (long j = threadIdx.x; j < n; j += 256) s += A[i * n + j];
    r[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) r[threadIdx.x] += r[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) rs[i] = r[0];
}

// M (np x np, column-major == row-major: symmetric) from A; identity on the padding for the matrices that are inverted, zero
// for those that are multiplied (the n x n corner is closed under products either way)
__global__ __launch_bounds__(256) void node_build_kernel(int kind, const double* __restrict__ A, long n, const double* __restrict__ cs,
                                                         const double* __restrict__ rs, double p0, double scale,
                                                         double* __restrict__ M, long np) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long j = blockIdx.y;
    if (i >= np) return;
    for (long jj = j; jj < np; jj += gridDim.y) {
        const double eye = (i == jj) ? 1.0 : 0.0;
        double v;
        if (i < n && jj < n) {
            const double a = A[jj * n + i];                         // (coalesced in i; A is symmetric)
            if (kind == PGP_NODE_DIFF) v = scale * (p0 * (a - eye * rs[i]));
            else {
                const double S = (sqrt(1.0 / cs[i]) * a) * sqrt(1.0 / cs[jj]);
                const double L = eye - S;
                if (kind == PGP_NODE_REGLAP) v = eye + (p0 * p0) * L;
                else if (kind == PGP_NODE_VND) v = eye - p0 * S;
                else v = p0 * eye - L;
            }
        } else v = (kind == PGP_NODE_REGLAP || kind == PGP_NODE_VND) ? eye : 0.0;
        M[i + jj * np] = v;
    }
}

// X <- I + scale * X
__global__ __launch_bounds__(256) void scale_add_eye_kernel(double* __restrict__ X, long np, double scale) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    for (long j = blockIdx.y; j < np; j += gridDim.y) {
        const double v = scale * X[i + j * np];
        X[i + j * np] = (i == j) ? 1.0 + v : v;
    }
}

// out (n x n, row-major) from the n x n corner of X (ld np): the full matrix, or the lower triangle mirrored
__global__ __launch_bounds__(256) void node_out_kernel(const double* __restrict__ X, long np, long n, int lower, double* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (long j = blockIdx.y; j < n; j += gridDim.y) {
        const long r = (lower && i < j) ? j : i, q = (lower && i < j) ? i : j;
        out[j * n + i] = X[r + q * np];
    }
}

dim3 grid2(long rows, long cols) { return dim3((unsigned)((rows + 255) / 256), (unsigned)std::min<long>(cols, 65535)); }

// C = X Y for symmetric commuting X, Y (np x np): the NT product X Y'
int sym_product(pgp_ctx* c, const double* X, const double* Y, double* C, long np) {
    GemmArgs g{};
    g.A = X; g.lda = np; g.a_kc = 0;
    g.B = Y; g.ldb = np; g.b_kc = 0;
    g.C = C; g.ldc = np;
    g.M = (int)np; g.N = (int)np; g.K = (int)np; g.alpha = 1.0; g.beta = 0.0;
    g.kmode = KM_FULL;
    g.tile = (np / 128) * (np / 128) < c->small_tile_below ? 64 : 128;
    g.flops = 2.0 * (double)np * np * np;
    return gemm_prof(c, PC_GEMM_INNER, g);
}

// D[i n + j] = |x_i - x_j|^2, +inf at j == i.  XT is d x n (coordinate-major): the loads of a workgroup are contiguous in j.
__global__ __launch_bounds__(256) void knn_dist_kernel(const double* __restrict__ XT, long n, long d, double* __restrict__ D) {
    __shared__ double xi[KNN_ROWS][KNN_CHUNK];
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    const long i0 = (long)blockIdx.y * KNN_ROWS;
    double acc[KNN_ROWS];
#pragma unroll
    for (int r = 0; r < KNN_ROWS; ++r) acc[r] = 0.0;
    for (long k0 = 0; k0 < d; k0 += KNN_CHUNK) {
        const int kc = (d - k0 < KNN_CHUNK) ? (int)(d - k0) : KNN_CHUNK;
        __syncthreads();
        for (int t = threadIdx.x; t < KNN_ROWS * kc; t += 256) {
            const int r = t / kc, kk = t - r * kc;
            xi[r][kk] = (i0 + r < n) ? XT[(k0 + kk) * n + i0 + r] : 0.0;
        }
        __syncthreads();
        if (j < n)
            for (int kk = 0; kk < kc; ++kk) {
                const double xj = XT[(k0 + kk) * n + j];
#pragma unroll
                for (int r = 0; r < KNN_ROWS; ++r) {
                    const double t = xi[r][kk] - xj;
                    acc[r] = fma(t, t, acc[r]);
                }
            }
    }
    if (j >= n) return;
#pragma unroll
    for (int r = 0; r < KNN_ROWS; ++r)
        if (i0 + r < n) D[(i0 + r) * n + j] = (i0 + r == j) ? HUGE_VAL : acc[r];
}

// per row: the k smallest entries of D's row, one after the other (lower index wins a tie); Adj[i n + j] = 1 for each
__global__ __launch_bounds__(256) void knn_select_kernel(double* __restrict__ D, long n, int k, double* __restrict__ Adj) {
    __shared__ double bv[256];
    __shared__ long bi[256];
    double* row = D + (long)blockIdx.x * n;
    for (int t = 0; t < k; ++t) {
        double v = HUGE_VAL;
        long at = n;
        for (long j = threadIdx.x; j < n; j += 256) {
            const double x = row[j];
            if (x < v) { v = x; at = j; }                           // ascending j per thread: the first minimum stays
        }
        bv[threadIdx.x] = v; bi[threadIdx.x] = at;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) {
                const double v2 = bv[threadIdx.x + o];
                const long a2 = bi[threadIdx.x + o];
                if (v2 < bv[threadIdx.x] || (v2 == bv[threadIdx.x] && a2 < bi[threadIdx.x])) { bv[threadIdx.x] = v2; bi[threadIdx.x] = a2; }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0 && bi[0] < n) {
            Adj[(long)blockIdx.x * n + bi[0]] = 1.0;
            row[bi[0]] = HUGE_VAL;
        }
        __syncthreads();
    }
}

// out = max(Adj, Adj')
__global__ __launch_bounds__(256) void knn_sym_kernel(const double* __restrict__ Adj, long n, double* __restrict__ out) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    for (long i = blockIdx.y; i < n; i += gridDim.y) out[i * n + j] = fmax(Adj[i * n + j], Adj[j * n + i]);
}

}  // namespace

extern "C" {

int pgp_node_kernel(pgp_ctx* c, int kind, const double* A, int64_t n, double p0, double p1, double* K_out) {
    if (!c) return -1;
    GateShared device_gate_hold(c);
    if (kind < PGP_NODE_REGLAP || kind > PGP_NODE_DIFF) return -2;
    if (!A) return -3;
    if (n <= 0) return -4;
    if (kind == PGP_NODE_RW && !(p1 >= 1.0 && p1 <= 1073741824.0)) return -6;
    if (!K_out) return -7;
    HIP_TRY(hipSetDevice(c->device));
    const long np = round_up(n, 128);
    const size_t nn = (size_t)np * np * sizeof(double);
    hipStream_t st = c->st;
    PoolScratch scr(c);
    double *Ad = nullptr, *cs = nullptr, *rs = nullptr, *M = nullptr, *X = nullptr, *Y = nullptr, *Z = nullptr, *pack = nullptr;
    CHK(scr.alloc(&Ad, (size_t)n * n * sizeof(double)));
    CHK(scr.alloc(&cs, (size_t)n * sizeof(double)));
    CHK(scr.alloc(&rs, (size_t)n * sizeof(double)));
    CHK(scr.alloc(&M, nn));
    CHK(scr.alloc(&X, nn));
    CHK(scr.alloc(&Y, nn));
    HIP_TRY(hipMemcpyAsync(Ad, A, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(col_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, Ad, (long)n, cs);
    hipLaunchKernelGGL(row_sum_kernel, dim3((unsigned)n), dim3(256), 0, st, Ad, (long)n, rs);
    int squarings = 0;
    if (kind == PGP_NODE_DIFF) {                       // 2 |beta| max degree / 2^s <= 1/2
        double maxdeg = 0.0;
        for (int64_t i = 0; i < n; ++i) {
            double s = 0.0;
            for (int64_t j = 0; j < n; ++j) s += fabs(A[i * n + j]);
            maxdeg = std::max(maxdeg, s);
        }
        double bound = 2.0 * fabs(p0) * maxdeg;
        if (!(bound < 1e300)) return -5;
        while (bound > 0.5) { bound *= 0.5; ++squarings; }
    }
    hipLaunchKernelGGL(node_build_kernel, grid2(np, np), dim3(256), 0, st, kind, Ad, (long)n, cs, rs, p0, ldexp(1.0, -squarings), M, np);
    const double* result = nullptr;
    int lower = 0;
    if (kind == PGP_NODE_REGLAP || kind == PGP_NODE_VND) {
        CHK(scr.alloc(&Z, std::max<size_t>(nn / 4, 128 * 128 * sizeof(double))));
        CHK(scr.alloc(&pack, (size_t)(np / 128) * PACK_DOUBLES * sizeof(double)));
        HIP_TRY(hipMemsetAsync(X, 0, nn, st));         // W = L^-1: its strict upper triangle is never written
        HIP_TRY(hipMemsetAsync(c->info_dev, 0, sizeof(int), st));
        double* pack_save = c->inv16;                  // the blocked driver takes the per-leaf operand images from the ctx
        c->inv16 = pack;
        SweepJob job{M, np, np, np};
        const int rc = potrf_blocked(c, job);
        c->inv16 = pack_save;
        CHK(rc);
        int info = 0;
        HIP_TRY(hipMemcpyAsync(&info, c->info_dev, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (info != 0) return info > (int)n ? (int)n : info;
        CHK(trtri_lower(c, M, np, X, np, Z, np));
        CHK(lauum_lower(c, X, np, Y, np, np));
        result = Y; lower = 1;
    } else if (kind == PGP_NODE_RW) {
        CHK(scr.alloc(&Z, nn));
        long p = (long)p1;
        double *base = M, *spare = X, *acc = nullptr, *acc_spare = Y;      // acc (once set) and acc_spare alternate between Y and Z
        while (true) {
            if (p & 1) {
                if (!acc) {                                                // acc <- base (a copy: base goes on being squared)
                    HIP_TRY(hipMemcpyAsync(Z, base, nn, hipMemcpyDeviceToDevice, st));
                    acc = Z;
                } else {
                    CHK(sym_product(c, acc, base, acc_spare, np));
                    std::swap(acc, acc_spare);
                }
            }
            p >>= 1;
            if (!p) break;
            CHK(sym_product(c, base, base, spare, np));
            std::swap(base, spare);
        }
        result = acc;
    } else {
        // Horner: X_18 = I + H / 18;  X_k = I + (H X_{k+1}) / k;  exp(H) ~ X_1;  then s squarings
        double *cur = X, *nxt = Y;
        HIP_TRY(hipMemcpyAsync(cur, M, nn, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(scale_add_eye_kernel, grid2(np, np), dim3(256), 0, st, cur, np, 1.0 / TAYLOR_DEGREE);
        for (int k = TAYLOR_DEGREE - 1; k >= 1; --k) {
            CHK(sym_product(c, M, cur, nxt, np));
            hipLaunchKernelGGL(scale_add_eye_kernel, grid2(np, np), dim3(256), 0, st, nxt, np, 1.0 / k);
            std::swap(cur, nxt);
        }
        for (int s = 0; s < squarings; ++s) {
            CHK(sym_product(c, cur, cur, nxt, np));
            std::swap(cur, nxt);
        }
        result = cur;
    }
    hipLaunchKernelGGL(node_out_kernel, grid2(n, n), dim3(256), 0, st, result, np, (long)n, lower, Ad);
    if (hipGetLastError() != hipSuccess) return PGP_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(K_out, Ad, (size_t)n * n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (c->prof) prof_collect(c);
    return PGP_OK;
}

// pc (n x d, row-major host), A_out (n x n, row-major host): dense 0 / 1 adjacency of the symmetrised k-NN graph
int pgp_knn_graph(pgp_ctx* c, const double* pc, int64_t n, int64_t d, int k, double* A_out) {
    if (!c) return -1;
    GateShared device_gate_hold(c);
    if (!pc) return -2;
    if (n <= 1) return -3;
    if (d <= 0) return -4;
    if (k < 1 || k >= n) return -5;
    if (!A_out) return -6;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->st;
    std::vector<double> xt((size_t)n * d);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t q = 0; q < d; ++q) xt[(size_t)q * n + i] = pc[i * d + q];
    PoolScratch scr(c);
    double *XT = nullptr, *D = nullptr, *Adj = nullptr;
    const size_t nn = (size_t)n * n * sizeof(double);
    CHK(scr.alloc(&XT, (size_t)n * d * sizeof(double)));
    CHK(scr.alloc(&D, nn));
    CHK(scr.alloc(&Adj, nn));
    HIP_TRY(hipMemcpyAsync(XT, xt.data(), (size_t)n * d * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(Adj, 0, nn, st));
    const long rowblocks = (n + KNN_ROWS - 1) / KNN_ROWS;
    if (rowblocks > 65535) return -3;
    hipLaunchKernelGGL(knn_dist_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)rowblocks), dim3(256), 0, st, XT, (long)n, (long)d, D);
    hipLaunchKernelGGL(knn_select_kernel, dim3((unsigned)n), dim3(256), 0, st, D, (long)n, k, Adj);
    hipLaunchKernelGGL(knn_sym_kernel, grid2(n, n), dim3(256), 0, st, Adj, (long)n, D);
    if (hipGetLastError() != hipSuccess) return PGP_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(A_out, D, nn, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PGP_OK;
}

}  // extern "C"
