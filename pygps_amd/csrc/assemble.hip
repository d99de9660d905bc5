// Kernel-matrix construction (reference: Core/cov.py RBF :796-828, RBFard :887-938, Matern
// :1124-1182 -- scipy cdist('sqeuclidean') + numpy exp/sqrt passes, replaced by ONE fused tile kernel).
//
//   scale_transpose_kernel  x (n,d) row-major  ->  XsT (dpad, ldp) k-major, scaled by the kernel's
//                           length-scales (x/ell, x*(1/ell_k), sqrt(d) x/ell), zero padded.
//   cov_tile_kernel<MODE>   64x64 output tile per workgroup; X slabs staged through LDS with
//                           coalesced 512-byte runs; distance in difference form; scalar map
//                           (exp / Matern polynomial / derivative) fused; HBM-write bound:
//                           algorithmic bytes = 8 n m (+ 8 (n+m) d).
//        MODE_SYM    'train': only tiles on/above the diagonal are computed, each is stored twice
//                    (direct + mirrored) -> full symmetric (n,n) numpy array.
//        MODE_RECT   'cross': (n,m).
//        MODE_FACTOR fused assembly of B = K/sn2 + I straight into the (padded) factor buffer that
//                    the Cholesky overwrites: only the row-major upper triangle (= column-major
//                    lower) is written, padding rows/cols get the identity.
#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include <atomic>

#include "kernels.h"
#include "sqdist_tile.h"

namespace {

__global__ void scale_transpose_kernel(const double* __restrict__ x, long n, int d, const double* __restrict__ scale,
                                       double* __restrict__ XsT, long ldp, int dpad) {
    // one thread per (k, p); p fastest for coalesced stores.  x reads are strided but x is tiny (n*d).
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y;
    if (p >= ldp) return;
    double v = 0.0;
    if (p < n && k < d) v = x[p * d + k] * scale[k];
    XsT[(long)k * ldp + p] = v;
    (void)dpad;
}

enum { MODE_SYM = 0, MODE_RECT = 1, MODE_FACTOR = 2 };
#ifndef PGP_SUPER
#define PGP_SUPER 8
#endif
constexpr int SUPER = PGP_SUPER;          // super-tile edge in tiles (0: plain packed-triangular order)

// The scalar map of one 4x4 register tile with the kernel family and value/derivative choice fixed at compile time:
// the run-time switch sits OUTSIDE the unrolled element loop, so the executed path is 16 short copies of one functor
// (a few KB of code) instead of 16 copies of the whole kind chain (the unspecialised kernel was ~18k instructions,
// larger than the instruction cache).
template <int MODE, int KIND, bool DER>
__device__ __forceinline__ void tile_values(const CovParams& cp0, const double (&s)[4][4], double (&v)[4][4],
                                            const double* __restrict__ XrT, long ldr, const double* __restrict__ XcT,
                                            long ldc, long r0, long c0, long n, double inv_sn2) {
    CovParams cp = cp0;
    cp.kind = KIND;                                 // constant-folds the kind chains of cov_value / cov_deriv
    const int t = threadIdx.x, tr = t >> 4, tc = t & 15;
    const int ard_der = DER ? cov_ard_der(cp) : -1;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long r = r0 + 4 * tr + a;
            const long c = c0 + 2 * tc + (b & 1) + 32 * (b >> 1);
            double val;
            if (!DER) {
                val = cov_value(cp, s[a][b], MODE != MODE_RECT && r == c);
            } else {
                double dk2 = 0.0;
                if ((KIND == 1 || KIND == 6) && ard_der >= 0) {
                    const double dd = XrT[(long)ard_der * ldr + r] - XcT[(long)ard_der * ldc + c];
                    dk2 = dd * dd;
                }
                val = cov_deriv(cp, s[a][b], dk2, MODE != MODE_RECT && r == c);
            }
            if (MODE == MODE_FACTOR) {
                if (r < n && c < n) val = val * inv_sn2 + (r == c ? 1.0 : 0.0);
                else val = (r == c) ? 1.0 : 0.0;
            }
            v[a][b] = val;
        }
}

// overload selection: programs never call the functor path
template <int MODE, int KIND, bool DER>
__device__ __forceinline__ void tile_values_sel(const CovProgram&, const double (&)[4][4], double (&)[4][4], const double*, long,
                                                const double*, long, long, long, long, double) {}
template <int MODE, int KIND, bool DER>
__device__ __forceinline__ void tile_values_sel(const CovParams& cp, const double (&s)[4][4], double (&v)[4][4],
                                                const double* __restrict__ XrT, long ldr, const double* __restrict__ XcT,
                                                long ldc, long r0, long c0, long n, double inv_sn2) {
    tile_values<MODE, KIND, DER>(cp, s, v, XrT, ldr, XcT, ldc, r0, c0, n, inv_sn2);
}

__device__ __forceinline__ const double* prog_ardw(const CovProgram& P) { return P.ardw; }
__device__ __forceinline__ const double* prog_ardw(const CovParams&) { return nullptr; }
__device__ __forceinline__ const double* prog_ardw2(const CovProgram& P) { return P.ardw2; }
__device__ __forceinline__ const double* prog_ardw2(const CovParams&) { return nullptr; }
__device__ __forceinline__ const double* prog_der_w(const CovProgram& P) { return cov_ard_der_w(P); }
__device__ __forceinline__ const double* prog_der_w(const CovParams&) { return nullptr; }
__device__ __forceinline__ double prog_elem(const CovProgram& P, double s, double dk2, bool same, double s1, double s2, double pv) { return cov_elem(P, s, dk2, same, s1, s2, pv); }
__device__ __forceinline__ double prog_elem(const CovParams& p, double s, double dk2, bool same, double, double, double) { return cov_elem(p, s, dk2, same); }
// the DOT instantiations: the element's dot product pd beside the distances
__device__ __forceinline__ double prog_elem_dot(const CovProgram& P, double s, double dk2, bool same, double s1, double pd) { return cov_elem<true>(P, s, dk2, same, s1, 0.0, 0.0, pd); }
__device__ __forceinline__ double prog_elem_dot(const CovParams&, double, double, bool, double, double) { return 0.0; }
__device__ __forceinline__ int prog_dot_der(const CovProgram& P) { return cov_dot_der(P); }
__device__ __forceinline__ int prog_dot_der(const CovParams&) { return -1; }
__device__ __forceinline__ const double* prog_pre(const CovProgram& P) { return P.pre; }
__device__ __forceinline__ const double* prog_pre(const CovParams&) { return nullptr; }
__device__ __forceinline__ long prog_pre_ld(const CovProgram& P) { return P.pre_ld; }
__device__ __forceinline__ long prog_pre_ld(const CovParams&) { return 0; }

template <class COV> struct is_program { static constexpr bool value = false; };
template <> struct is_program<CovProgram> { static constexpr bool value = true; };
template <class COV> struct is_sm { static constexpr bool value = false; };
template <> struct is_sm<CovSM> { static constexpr bool value = true; };

// first-slab share of one thread: 2 double2 of the row slab, 2 of the column slab (same split as sqdist_tile)
struct SlabRegs { double2_t r[2], c[2]; };

__device__ __forceinline__ void slab_fetch(const double* __restrict__ XrT, long ldr, long r0,
                                           const double* __restrict__ XcT, long ldc, long c0, int k0, SlabRegs& g) {
    const int t = threadIdx.x;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int v = t + p * 256;                 // 0..511 : k = v / 32, pair = v % 32
        const int k = v >> 5, pr = v & 31;
        g.r[p] = *(const double2_t*)(XrT + (long)(k0 + k) * ldr + r0 + 2 * pr);
        g.c[p] = *(const double2_t*)(XcT + (long)(k0 + k) * ldc + c0 + 2 * pr);
    }
}

__device__ __forceinline__ void slab_stage(double* __restrict__ smx, const SlabRegs& g) {
    const int t = threadIdx.x;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int v = t + p * 256;
        const int k = v >> 5, pr = v & 31;
        *(double2_t*)(smx + k * ST + 2 * pr) = g.r[p];
        *(double2_t*)(smx + SKC * ST + k * ST + 2 * pr) = g.c[p];
    }
}

// same, plus the ARD-weighted distance of a program's ARD leaf: s1 += w[k] (a_k - b_k)^2
__device__ __forceinline__ void slab_accum2(const double* __restrict__ smx, double (&s)[4][4], double (&s1)[4][4],
                                            const double* __restrict__ w, int k0) {
    const int t = threadIdx.x, tr = t >> 4, tc = t & 15;
    const double* xr = smx;
    const double* xc = smx + SKC * ST;
#pragma unroll
    for (int k = 0; k < SKC; ++k) {
        const double wk = (k0 + k) < CP_MAXARD ? w[k0 + k] : 0.0;
        const double2_t r01 = *(const double2_t*)(xr + k * ST + 4 * tr);
        const double2_t r23 = *(const double2_t*)(xr + k * ST + 4 * tr + 2);
        const double2_t c01 = *(const double2_t*)(xc + k * ST + 2 * tc);
        const double2_t c23 = *(const double2_t*)(xc + k * ST + 2 * tc + 32);
        const double rv[4] = {r01[0], r01[1], r23[0], r23[1]};
        const double cv[4] = {c01[0], c01[1], c23[0], c23[1]};
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double df = rv[a] - cv[b];
                const double d2 = df * df;
                s[a][b] += d2;
                s1[a][b] = fma(wk, d2, s1[a][b]);
            }
    }
}

// two ARD leaves: s1 += w[k] d^2, s2 += w2[k] d^2
__device__ __forceinline__ void slab_accum3(const double* __restrict__ smx, double (&s)[4][4], double (&s1)[4][4],
                                            double (&s2)[4][4], const double* __restrict__ w,
                                            const double* __restrict__ w2, int k0) {
    const int t = threadIdx.x, tr = t >> 4, tc = t & 15;
    const double* xr = smx;
    const double* xc = smx + SKC * ST;
#pragma unroll
    for (int k = 0; k < SKC; ++k) {
        const double wk = (k0 + k) < CP_MAXARD ? w[k0 + k] : 0.0;
        const double wk2 = (k0 + k) < CP_MAXARD ? w2[k0 + k] : 0.0;
        const double2_t r01 = *(const double2_t*)(xr + k * ST + 4 * tr);
        const double2_t r23 = *(const double2_t*)(xr + k * ST + 4 * tr + 2);
        const double2_t c01 = *(const double2_t*)(xc + k * ST + 2 * tc);
        const double2_t c23 = *(const double2_t*)(xc + k * ST + 2 * tc + 32);
        const double rv[4] = {r01[0], r01[1], r23[0], r23[1]};
        const double cv[4] = {c01[0], c01[1], c23[0], c23[1]};
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double df = rv[a] - cv[b];
                const double d2 = df * df;
                s[a][b] += d2;
                s1[a][b] = fma(wk, d2, s1[a][b]);
                s2[a][b] = fma(wk2, d2, s2[a][b]);
            }
    }
}

// programs with dot-product leaves: pd += a_k b_k (fma, coordinate order) beside r^2 and, when ARD, the ARD leaf's weighted distance
template <bool ARD>
__device__ __forceinline__ void slab_accum_dot(const double* __restrict__ smx, double (&s)[4][4], double (&s1)[ARD ? 4 : 1][4],
                                               double (&pd)[4][4], const double* __restrict__ w, int k0) {
    const int t = threadIdx.x, tr = t >> 4, tc = t & 15;
    const double* xr = smx;
    const double* xc = smx + SKC * ST;
#pragma unroll
    for (int k = 0; k < SKC; ++k) {
        double wk = 0.0;
        if (ARD) wk = (k0 + k) < CP_MAXARD ? w[k0 + k] : 0.0;
        const double2_t r01 = *(const double2_t*)(xr + k * ST + 4 * tr);
        const double2_t r23 = *(const double2_t*)(xr + k * ST + 4 * tr + 2);
        const double2_t c01 = *(const double2_t*)(xc + k * ST + 2 * tc);
        const double2_t c23 = *(const double2_t*)(xc + k * ST + 2 * tc + 32);
        const double rv[4] = {r01[0], r01[1], r23[0], r23[1]};
        const double cv[4] = {c01[0], c01[1], c23[0], c23[1]};
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double df = rv[a] - cv[b];
                if (ARD) {
                    const double d2 = df * df;
                    s[a][b] += d2;
                    s1[a][b] = fma(wk, d2, s1[a][b]);
                } else s[a][b] = fma(df, df, s[a][b]);
                pd[a][b] = fma(rv[a], cv[b], pd[a][b]);
            }
    }
}

__device__ __forceinline__ void slab_accum(const double* __restrict__ smx, double (&s)[4][4]) {
    const int t = threadIdx.x, tr = t >> 4, tc = t & 15;
    const double* xr = smx;
    const double* xc = smx + SKC * ST;
#pragma unroll
    for (int k = 0; k < SKC; ++k) {
        const double2_t r01 = *(const double2_t*)(xr + k * ST + 4 * tr);
        const double2_t r23 = *(const double2_t*)(xr + k * ST + 4 * tr + 2);
        const double2_t c01 = *(const double2_t*)(xc + k * ST + 2 * tc);
        const double2_t c23 = *(const double2_t*)(xc + k * ST + 2 * tc + 32);
        const double rv[4] = {r01[0], r01[1], r23[0], r23[1]};
        const double cv[4] = {c01[0], c01[1], c23[0], c23[1]};
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double df = rv[a] - cv[b];
                s[a][b] = fma(df, df, s[a][b]);
            }
    }
}

// COV = CovParams (one functor, the hot path) or CovProgram (Sum/Product/Scale tree; elements are evaluated in a
// rolled loop over LDS-staged distances so that the eight leaf functors are instantiated once, not 16 times) or CovSM (spectral
// mixture: no distance tile; every element is evaluated from the staged coordinates themselves, in a rolled loop as well).
//
// Persistent workgroups, software-pipelined over tiles: the coordinates of tile i+1 are fetched into registers
// BEFORE the stores of tile i are issued (vmcnt retires in order on gfx9, so a load queued behind 32 KB of stores
// would wait for them), which lets the store bursts of one tile drain under the distance/exp arithmetic of the
// next.  One workgroup per tile ran the phases load -> VALU -> store of all resident workgroups in lock-step:
// HBM idle during the VALU phase, VALU idle (55 % busy by SQ_ACTIVE_INST_VALU) during the store phase.
__device__ double2_t g_trash[1];       // out-of-range lanes of the FAST store path write here
// nt (uniform): non-temporal stores, option "asm_nt" (default 0).  Round 4 first read them as a 3 % gain for outputs >= 1 GB; alternated
// in ONE process (tools/gpu_probe.py asm nt=1 nt=0 ...) they are neutral for RBF (0.423-0.432 ms either way at N = 16384) and cost
// Matern up to 15 % -- the earlier reading compared a process's first measurement (always ~10 % slow) with its second.  A kernel
// that only issues this tile pattern's stores takes 0.40 ms (pgp_test_store_roof): the assembly runs at 0.93 of that
#define TILE_STORE(dst, val) do { if (nt) __builtin_nontemporal_store((val), (dst)); else *(dst) = (val); } while (0)

// FAST: ldo, n and m are even -> every store is an aligned, *unconditional* double2 store (lanes outside the matrix
// are redirected to g_trash).  With a fixed number of stores per tile the compiler can wait for the prefetched
// coordinates with vmcnt(#stores) instead of vmcnt(0), i.e. without waiting for the stores themselves.
template <int MODE, class COV, int KIND, bool DER, bool FAST>
__global__ __launch_bounds__(256) void cov_tile_kernel(const double* __restrict__ XrT, long ldr, long n,
                                                       const double* __restrict__ XcT, long ldc, long m, int dpad,
                                                       COV cp, double inv_sn2, double* __restrict__ out,
                                                       long ldo, const int2* __restrict__ tiles, long ntiles, int nt) {
    constexpr int TS = ST + 2;                      // transpose-tile row stride (16-byte aligned rows)
    constexpr bool PROG = is_program<COV>::value;
    constexpr bool SMK = is_sm<COV>::value;         // D <= SKC: the one staged slab holds every coordinate of the tile
    constexpr bool PARD = PROG && (KIND & 3) >= 1;  // program with an ARD leaf: second (weighted) distance
    constexpr bool PARD2 = PROG && (KIND & 3) == 2; // two ARD leaves: a third distance, kept in registers
    constexpr bool PPRE = PROG && (KIND & 4) != 0;  // program with a precomputed-matrix leaf: its tile is loaded beside the distances
    constexpr bool PDOT = PROG && (KIND & 8) != 0;  // program with dot-product leaves (Linear / Poly / plain LINard): sum_k x_k z_k beside
                                                    // the distances, kept in registers; KIND 8 (no ARD leaf) and 9 (one) exist
    constexpr int SMT = PARD ? 2 * 16 * 256 : (MODE == MODE_SYM ? ST * TS : (PROG ? 16 * 256 : 2));
    // coordinate slabs (2 x 16 x 64 doubles) and the mirror-transpose tile share one region: 33.8 KB -> 4 WGs per CU
    constexpr int SMX = 2 * SKC * ST;
    __shared__ __attribute__((aligned(16))) double sm[SMT > SMX ? SMT : SMX];
    double* smx = sm;
    const int t = threadIdx.x, tr = t >> 4, tc = t & 15;
    long tile = blockIdx.x;
    if (tile >= ntiles) return;
    // (ti, tj) come from a host-built table through scalar loads: no per-tile index arithmetic on the VALU
    int2 tc2 = tiles[tile];
    long ti = tc2.x, tj = tc2.y;
    SlabRegs g;
    slab_fetch(XrT, ldr, ti * ST, XcT, ldc, tj * ST, 0, g);
    slab_stage(smx, g);
    __syncthreads();
    while (true) {
        const long r0 = ti * ST, c0 = tj * ST;
        const long next = tile + gridDim.x;
        long nti = 0, ntj = 0;
        if (next < ntiles) {
            const int2 nx = tiles[next];
            nti = nx.x; ntj = nx.y;
            slab_fetch(XrT, ldr, nti * ST, XcT, ldc, ntj * ST, 0, g);
        }
        double s[4][4], s1[PARD ? 4 : 1][4], s2[PARD2 ? 4 : 1][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) { s[a][b] = 0.0; if (PARD) s1[a][b] = 0.0; if (PARD2) s2[a][b] = 0.0; }
        double pd[PDOT ? 4 : 1][4];
        if constexpr (PDOT) {
#pragma unroll
            for (int e = 0; e < 16; ++e) pd[e >> 2][e & 3] = 0.0;
        }
        if constexpr (SMK) {
#pragma unroll 1
            for (int e = 0; e < 16; ++e) {
                const int rl = 4 * tr + (e >> 2), cl = 2 * tc + (e & 1) + 32 * ((e >> 1) & 1);
                put16(s, e, sm_elem(cp, smx + rl, smx + SKC * ST + cl));
            }
        } else if constexpr (PDOT) slab_accum_dot<PARD>(smx, s, s1, pd, prog_ardw(cp), 0);
        else if constexpr (PARD2) slab_accum3(smx, s, s1, s2, prog_ardw(cp), prog_ardw2(cp), 0);
        else if constexpr (PARD) slab_accum2(smx, s, s1, prog_ardw(cp), 0); else slab_accum(smx, s);
        for (int k0 = SKC; !SMK && k0 < dpad; k0 += SKC) {  // d > 16: further slabs, loaded in place
            SlabRegs h;
            slab_fetch(XrT, ldr, r0, XcT, ldc, c0, k0, h);
            __syncthreads();
            slab_stage(smx, h);
            __syncthreads();
            if constexpr (PDOT) slab_accum_dot<PARD>(smx, s, s1, pd, prog_ardw(cp), k0);
            else if constexpr (PARD2) slab_accum3(smx, s, s1, s2, prog_ardw(cp), prog_ardw2(cp), k0);
            else if constexpr (PARD) slab_accum2(smx, s, s1, prog_ardw(cp), k0); else slab_accum(smx, s);
        }

        double v[4][4];
        if constexpr (PROG) {
            __syncthreads();                            // slabs consumed; the staging area overlays them
            double* sv = sm + t;
            double* sv1 = sm + 16 * 256 + t;
#pragma unroll
            for (int e = 0; e < 16; ++e) { sv[e * 256] = s[e >> 2][e & 3]; if (PARD) sv1[e * 256] = s1[e >> 2][e & 3]; }
            const int pder = cov_ard_der(cp);           // derivative w.r.t. an ARD length-scale of the program's ARD leaf
            double pm[PPRE ? 4 : 1][4];
            if constexpr (PPRE) pre_tile_load(prog_pre(cp), prog_pre_ld(cp), r0, c0, pm);
            int ddk = -1;                               // plain LINard: the coordinate of the length-scale the derivative is taken in
            if constexpr (PDOT) ddk = prog_dot_der(cp);
#pragma unroll 1
            for (int e = 0; e < 16; ++e) {
                const int a = e >> 2, b = e & 3;
                const long r = r0 + 4 * tr + a;
                const long c = c0 + 2 * tc + (b & 1) + 32 * (b >> 1);
                double dk2 = 0.0;
                if (PARD && pder >= 0) {
                    const double dd = XrT[(long)pder * ldr + r] - XcT[(long)pder * ldc + c];
                    dk2 = prog_der_w(cp)[pder] * dd * dd;
                }
                double s2e = 0.0;
                if constexpr (PARD2) s2e = sel16(s2, e);
                double pve = 0.0;
                if constexpr (PPRE) pve = sel16(pm, e);
                if constexpr (PDOT) {
                    if (ddk >= 0) dk2 = XrT[(long)ddk * ldr + r] * XcT[(long)ddk * ldc + c];
                    sv[e * 256] = prog_elem_dot(cp, sv[e * 256], dk2, MODE != MODE_RECT && r == c, PARD ? sv1[e * 256] : 0.0, sel16(pd, e));
                } else
                sv[e * 256] = prog_elem(cp, sv[e * 256], dk2, MODE != MODE_RECT && r == c, PARD ? sv1[e * 256] : 0.0, s2e, pve);
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e >> 2][e & 3] = sv[e * 256];
        }
        if constexpr (!PROG && !SMK) tile_values_sel<MODE, KIND, DER>(cp, s, v, XrT, ldr, XcT, ldc, r0, c0, n, inv_sn2);
        else {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const long r = r0 + 4 * tr + a;
                    const long c = c0 + 2 * tc + (b & 1) + 32 * (b >> 1);
                    double val = s[a][b];
                    if (MODE == MODE_FACTOR) {
                        if (r < n && c < n) val = val * inv_sn2 + (r == c ? 1.0 : 0.0);
                        else val = (r == c) ? 1.0 : 0.0;
                    }
                    v[a][b] = val;
                }
        }
        // direct store: row-major, double2 along c
        if (FAST) {
            // uniform 64-bit tile base + 32-bit per-thread byte offsets (64 rows x ldo x 8 B < 4 GiB)
            char* base = (char*)(out + r0 * ldo + c0);
            const unsigned ldb = (unsigned)ldo * 8u;
            const unsigned off0 = (unsigned)(4 * tr) * ldb + (unsigned)(2 * tc) * 8u;
            const bool edge = MODE != MODE_FACTOR && (r0 + ST > n || c0 + ST > m);      // uniform
#pragma unroll
            for (int a = 0; a < 4; ++a) {
#pragma unroll
                for (int bh = 0; bh < 2; ++bh) {
                    double2_t val = double2_t{v[a][2 * bh], v[a][2 * bh + 1]};
                    double2_t* dst = (double2_t*)(base + (off0 + (unsigned)a * ldb + (unsigned)bh * 256u));
                    if (MODE == MODE_FACTOR) {      // padded buffer: every tile is full; exact zeros below the diagonal
                        if (ti == tj) {
                            const int rl = 4 * tr + a, cl = 2 * tc + 32 * bh;
                            if (cl < rl) val[0] = 0.0;
                            if (cl + 1 < rl) val[1] = 0.0;
                        }
                    } else if (edge) {
                        const long r = r0 + 4 * tr + a, c = c0 + 2 * tc + 32 * bh;
                        if (r >= n || c >= m) dst = g_trash;
                    }
                    TILE_STORE(dst, val);
                }
            }
        } else {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const long r = r0 + 4 * tr + a;
#pragma unroll
            for (int bh = 0; bh < 2; ++bh) {
                const long c = c0 + 2 * tc + 32 * bh;
                if (MODE == MODE_FACTOR) {
                    if (ti != tj) {
                        *(double2_t*)(out + r * ldo + c) = double2_t{v[a][2 * bh], v[a][2 * bh + 1]};
                    } else {                            // diagonal tile: keep exact zeros below the diagonal
                        if (c >= r) out[r * ldo + c] = v[a][2 * bh];
                        if (c + 1 >= r) out[r * ldo + c + 1] = v[a][2 * bh + 1];
                    }
                } else {
                    if (r < n) {
                        if (c + 1 < m && ((ldo & 1) == 0)) {
                            *(double2_t*)(out + r * ldo + c) = double2_t{v[a][2 * bh], v[a][2 * bh + 1]};
                        } else {
                            if (c < m) out[r * ldo + c] = v[a][2 * bh];
                            if (c + 1 < m) out[r * ldo + c + 1] = v[a][2 * bh + 1];
                        }
                    }
                }
            }
        }
        }
        if (MODE == MODE_SYM && (FAST || ti != tj)) {     // FAST: diagonal tiles too (same values) -> fixed store count
            // mirrored store out[c][r]: transpose the tile through LDS so that the global stores are 512-byte
            // contiguous runs (32 lanes x 16 B) instead of 32-byte pieces with a row stride between lanes
            __syncthreads();                            // the slabs (same LDS) have been consumed by every wave
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int cl = 2 * tc + (b & 1) + 32 * (b >> 1);
                *(double2_t*)(sm + cl * TS + 4 * tr) = double2_t{v[0][b], v[1][b]};
                *(double2_t*)(sm + cl * TS + 4 * tr + 2) = double2_t{v[2][b], v[3][b]};
            }
            __syncthreads();
            const int pr = t & 31, rw = t >> 5;         // 8 tile rows per pass, 32 double2 per row
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int cl = p * 8 + rw;
                const long c = c0 + cl, r = r0 + 2 * pr;
                if (FAST) {
                    const double2_t val = *(const double2_t*)(sm + cl * TS + 2 * pr);
                    char* mbase = (char*)(out + c0 * ldo + r0);
                    double2_t* dst = (double2_t*)(mbase + ((unsigned)cl * ((unsigned)ldo * 8u) + (unsigned)pr * 16u));
                    if ((r0 + ST > n || c0 + ST > m) && (c >= m || r >= n)) dst = g_trash;
                    TILE_STORE(dst, val);
                } else if (c < m) {
                    const double2_t val = *(const double2_t*)(sm + cl * TS + 2 * pr);
                    if (r + 1 < n && ((ldo & 1) == 0)) *(double2_t*)(out + c * ldo + r) = val;
                    else {
                        if (r < n) out[c * ldo + r] = val[0];
                        if (r + 1 < n) out[c * ldo + r + 1] = val[1];
                    }
                }
            }
        }
        if (next >= ntiles) break;
        __syncthreads();                                // everyone is done reading smx / sm
        // the wait for the prefetched coordinates sits right behind this tile's stores in straight-line code, so it
        // is a vmcnt(#stores) -- the stores keep draining while the next tile computes
        slab_stage(smx, g);
        __syncthreads();
        tile = next; ti = nti; tj = ntj;
    }
}

// ---- squared-exponential assembly in the GRAM form on the matrix cores (round 4) ---------------------------------------------
// r^2 = |a|^2 + |b|^2 - 2 a.b on CENTRED, scaled coordinates: one v_mfma_f64_16x16x4 per 4 coordinates and 16 x 16 outputs
// against two VALU instructions per element and coordinate of the difference form -- at d = 64 the difference form is bound by
// the vector ALU (0.40 of its peak executed, 0.27 of the HBM roof), this one by the stores.  The reference's cdist is the
// difference form; the Gram form's absolute error in r^2 is c eps (|a| + |b|)^2 instead of c' eps r^2, i.e. a RELATIVE error of
// that size in K.  The host therefore selects this kernel only when a bound on max |a|^2 (sum over the coordinates of
// (scale_k max_p |x_pk - mean_k|)^2, from the data and the length scales of the call) is <= 64: then K carries <= ~5e-14
// relative -- below what the difference form's own sqrt(d) eps r^2 leaves at d >= 32 -- otherwise the difference form runs.
// RBF / RBFard values only (K = sf2 exp(-r^2 / 2)).  Diagonal forced to r^2 = 0, round-off clamped.  Thread layout = MFMA
// accumulator layout: wave w, lane (l4, l15) holds rows 16 w + 4 a + l4, columns 16 q + l15 of the 64 x 64 tile.
constexpr int GSTP = ST + 2;
template <int NP>
__device__ __forceinline__ void gram_stage_pieces(const double* __restrict__ gp, long ldp, const double* __restrict__ mup,
                                                  double* __restrict__ slp) {
    double2_t g[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) g[i] = *(const double2_t*)(gp + (long)(4 * i) * ldp);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const double m_ = mup[4 * i];
        *(double2_t*)(slp + 4 * i * GSTP) = double2_t{g[i][0] - m_, g[i][1] - m_};
    }
}

typedef double gram4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ double gram_swap_adjacent(double v) {          // value of lane l ^ 1 (DPP quad_perm [1,0,3,2])
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0xB1, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0xB1, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

// NP > 0: dpad = 4 NP <= 64, ONE chunk per tile -- persistent workgroups, the next tile's coordinates and norms are fetched
// into registers before this tile's products are issued (like cov_tile_kernel).  NP == 0: any dpad, chunk by chunk, one tile per
// trip without the prefetch.
template <int MODE, int NP>
__global__ __launch_bounds__(256, 2) void cov_gram_kernel(const double* __restrict__ XT, long ldp, long n, int dpad, double sf2,
                                                          double inv_sn2, double* __restrict__ out, long ldo,
                                                          const int2* __restrict__ tiles, long ntiles, const double* __restrict__ mu,
                                                          const double* __restrict__ nrm, int nt) {
    extern __shared__ __attribute__((aligned(16))) double gsm[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l4 = lane >> 4, l15 = lane & 15;
    const int CH = dpad < 64 ? dpad : 64;
    double* xr = gsm;
    double* xc = gsm + CH * GSTP;
    const int spr = lane & 31, sside = lane >> 5;
    const int wvu = __builtin_amdgcn_readfirstlane(wave);
    double* slp = (sside ? xc : xr) + 2 * spr + wvu * GSTP;
    const double* mup = mu + wvu;
    constexpr int NPR = NP > 0 ? NP : 1;
    double2_t pg[NPR];                                // the next tile's staging pieces (NP > 0)
    double pm[NPR];                                   // the means of this thread's coordinates (tile-independent)
    double nr[4], nc[4], nnr[4], nnc[4];
    long tile = blockIdx.x;
    if (tile >= ntiles) return;
    int2 tc2 = tiles[tile];
    auto fetch = [&](int2 tl) {                       // NP > 0: pieces of tile tl -> pg, its norms -> nnr / nnc
        const double* gp = XT + (sside ? (long)tl.y * ST : (long)tl.x * ST) + 2 * spr + (long)wvu * ldp;
#pragma unroll
        for (int i = 0; i < NPR; ++i) pg[i] = *(const double2_t*)(gp + (long)(4 * i) * ldp);
#pragma unroll
        for (int a = 0; a < 4; ++a) nnr[a] = nrm[(long)tl.x * ST + 16 * wave + 4 * a + l4];
#pragma unroll
        for (int q = 0; q < 4; ++q) nnc[q] = nrm[(long)tl.y * ST + 16 * q + l15];
    };
    auto commit = [&]() {                             // pg -> LDS (centred), norms -> nr / nc
#pragma unroll
        for (int i = 0; i < NPR; ++i) *(double2_t*)(slp + 4 * i * GSTP) = double2_t{pg[i][0] - pm[i], pg[i][1] - pm[i]};
#pragma unroll
        for (int a = 0; a < 4; ++a) { nr[a] = nnr[a]; nc[a] = nnc[a]; }
    };
    if constexpr (NP > 0) {
#pragma unroll
        for (int i = 0; i < NPR; ++i) pm[i] = mup[4 * i];
        fetch(tc2);
        commit();
        __syncthreads();
    }
    while (true) {
        const long r0 = (long)tc2.x * ST, c0 = (long)tc2.y * ST;
        const long next = tile + gridDim.x;
        int2 nx = tc2;
        if constexpr (NP > 0) {
            if (next < ntiles) { nx = tiles[next]; fetch(nx); }
        }
        gram4_t acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = gram4_t{0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < dpad; k0 += 64) {
            const int kk = (dpad - k0) < 64 ? (dpad - k0) : 64;
            if constexpr (NP == 0) {
                __syncthreads();
                const double* gp = XT + (sside ? c0 : r0) + 2 * spr + (long)wvu * ldp + (long)k0 * ldp;
                switch (kk >> 4) {
                    case 1: gram_stage_pieces<4>(gp, ldp, mup + k0, slp); break;
                    case 2: gram_stage_pieces<8>(gp, ldp, mup + k0, slp); break;
                    case 3: gram_stage_pieces<12>(gp, ldp, mup + k0, slp); break;
                    default: gram_stage_pieces<16>(gp, ldp, mup + k0, slp); break;
                }
                __syncthreads();
            }
            const double* ap = xr + l4 * GSTP + 16 * wave + l15;
            const double* bp = xc + l4 * GSTP + l15;
            double fa0 = ap[0], fb0[4] = {bp[0], bp[16], bp[32], bp[48]};
            for (int ks = 0; ks < kk; ks += 8) {
                const double* a1 = ap + (ks + 4) * GSTP;
                const double* b1 = bp + (ks + 4) * GSTP;
                const double fa1 = a1[0], fb1[4] = {b1[0], b1[16], b1[32], b1[48]};
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa0, fb0[q], acc[q], 0, 0, 0);
                if (ks + 8 < kk) {
                    const double* a2 = ap + (ks + 8) * GSTP;
                    const double* b2 = bp + (ks + 8) * GSTP;
                    fa0 = a2[0]; fb0[0] = b2[0]; fb0[1] = b2[16]; fb0[2] = b2[32]; fb0[3] = b2[48];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa1, fb1[q], acc[q], 0, 0, 0);
            }
        }
        if constexpr (NP == 0) {
#pragma unroll
            for (int a = 0; a < 4; ++a) nr[a] = nrm[r0 + 16 * wave + 4 * a + l4];
#pragma unroll
            for (int q = 0; q < 4; ++q) nc[q] = nrm[c0 + 16 * q + l15];
        }
        double v[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long r = r0 + 16 * wave + 4 * a + l4, c = c0 + 16 * q + l15;
                double s2 = fmax(fma(-2.0, acc[q][a], nr[a] + nc[q]), 0.0);
                if (r == c) s2 = 0.0;
                double val = sf2 * exp_nonpos(-0.5 * s2);
                if (MODE == MODE_FACTOR) {
                    if (r < n && c < n) val = val * inv_sn2 + (r == c ? 1.0 : 0.0);
                    else val = (r == c) ? 1.0 : 0.0;
                    if (c < r) val = 0.0;              // diagonal tiles: exact zeros below the diagonal (row-major upper view)
                }
                v[a][q] = val;
            }
        // direct store, row-major.  Full tiles with an even leading dimension: adjacent lanes trade one value each (DPP), the even
        // lane stores columns (c, c + 1) of row a, the odd lane columns (c - 1, c) of row a + 1: 16-byte stores, half as many
        const bool full = MODE == MODE_FACTOR || (r0 + ST <= n && c0 + ST <= n);
        if (full && !(ldo & 1)) {
            const bool odd = l15 & 1;
#pragma unroll
            for (int a = 0; a < 4; a += 2)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double x0 = v[a][q], x1 = v[a + 1][q];
                    const double n0 = gram_swap_adjacent(x0), n1 = gram_swap_adjacent(x1);
                    const double2_t val = odd ? double2_t{n1, x1} : double2_t{x0, n0};
                    const long r = r0 + 16 * wave + 4 * (odd ? a + 1 : a) + l4, c = c0 + 16 * q + (l15 & ~1);
                    double2_t* dst = (double2_t*)(out + r * ldo + c);
                    if (nt) __builtin_nontemporal_store(val, dst); else *dst = val;
                }
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const long r = r0 + 16 * wave + 4 * a + l4, c = c0 + 16 * q + l15;
                    if (MODE == MODE_FACTOR || (r < n && c < n)) out[r * ldo + c] = v[a][q];
                }
        }
        if (MODE == MODE_SYM && tc2.x != tc2.y) {
            // mirrored store out[c][r]: transpose through LDS (this tile's coordinates are consumed), 64-double runs per column
            __syncthreads();
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int q = 0; q < 4; ++q) gsm[(16 * q + l15) * GSTP + 16 * wave + 4 * a + l4] = v[a][q];
            __syncthreads();
            const int pr = t & 31, rw = t >> 5;
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int cl = p * 8 + rw;
                const long c = c0 + cl, r = r0 + 2 * pr;
                if (c < n) {
                    const double2_t val = *(const double2_t*)(gsm + cl * GSTP + 2 * pr);
                    if (r + 1 < n && ((ldo & 1) == 0)) {
                        double2_t* dst = (double2_t*)(out + c * ldo + r);
                        if (nt) __builtin_nontemporal_store(val, dst); else *dst = val;
                    } else {
                        if (r < n) out[c * ldo + r] = val[0];
                        if (r + 1 < n) out[c * ldo + r + 1] = val[1];
                    }
                }
            }
        }
        if (next >= ntiles) break;
        tile = next;
        if constexpr (NP > 0) {
            __syncthreads();                            // every wave is done with the LDS image of this tile (and of its mirror)
            commit();
            __syncthreads();
            tc2 = nx;
        } else tc2 = tiles[tile];
    }
}

// ---- the same kernel for the common case, restructured around the memory pipeline (round 5) -------------------------------------
// dpad = 4 NP <= 64 (one chunk), every tile full (MODE_FACTOR: the padded buffer; MODE_SYM: n a multiple of 64), even leading
// dimension.  What the general kernel above loses per tile, found in its ISA:
//  * its loop body has run-time branches (edge tiles, non-temporal stores, "is there a next tile"), so the compiler cannot count
//    the memory operations between the prefetch of the next tile's coordinates and their use and falls back to s_waitcnt vmcnt(0)
//    -- on gfx9 that also waits for every STORE of the tile just finished (stores share the load counter): the workgroup drains
//    its stores before it may touch LDS again;
//  * __syncthreads() is a workgroup-scope fence + barrier: another vmcnt(0) at every barrier.
// Here the body is ONE basic block (the next tile is always fetched -- the last iteration re-fetches its own; diagonal tiles of
// MODE_SYM write their mirror too: same values), so the wait before the LDS commit is an exact vmcnt(#stores), and the barriers
// are bare s_barrier behind an lgkmcnt(0): the stores of a tile drain under the next tile's matrix products.
template <int V> struct GIC { static constexpr int value = V; };
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// HV = 2: the coordinates go through LDS in two halves of DP / 2 coordinates (half the LDS: four workgroups per CU instead of two,
// for the price of two more barriers per tile) -- more waves to hide the LDS / store-issue latencies behind.  The prefetch
// registers hold ONE half-step ahead: while half h of a tile is multiplied, the pieces of the next half-step are in flight.
// (Measured, N = 16384, d = 64, full symmetric: general kernel 0.635 ms, HV = 1 0.622, HV = 2 0.566 with 8192 persistent workgroups.
//  The kernel sits at the 128-register cliff of four workgroups per CU: SGPR-based addressing of the stores, a branch around the
//  diagonal-only selects and single-buffered fragments were all tried and all SPILLED -- check .private_segment_fixed_size.)
template <int MODE, int NP, int HV>
__global__ __launch_bounds__(256, HV == 2 ? 4 : 2) void cov_gram_fast_kernel(const double* __restrict__ XT, long ldp, long n, double sf2,
                                                                             double inv_sn2, double* __restrict__ out, long ldo,
                                                                             const int2* __restrict__ tiles, long ntiles,
                                                                             const double* __restrict__ mu, const double* __restrict__ nrm) {
    static_assert(NP >= 4 && NP <= 16 && NP % (2 * HV) == 0, "one chunk of 16 .. 64 coordinates, an even number of k-steps per half");
    constexpr int DP = 4 * NP, NPH = NP / HV, DPH = DP / HV;
    extern __shared__ __attribute__((aligned(16))) double gsm[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l4 = lane >> 4, l15 = lane & 15;
    double* xr = gsm;
    double* xc = gsm + DPH * GSTP;
    // round 6: the scalar map by table (sqdist_tile.h exp_nonpos_tab), pre-scaled by the prefactor of this mode
    constexpr int TAB_OFF = 2 * DPH * GSTP > ST * GSTP ? 2 * DPH * GSTP : ST * GSTP;
    const double* etab = gsm + TAB_OFF;
    const double cpre = MODE == MODE_FACTOR ? sf2 * inv_sn2 : sf2;
    exp_tab_fill(gsm + TAB_OFF, cpre, t);
    const int spr = lane & 31, sside = lane >> 5;
    const int wvu = __builtin_amdgcn_readfirstlane(wave);
    double* slp = (sside ? xc : xr) + 2 * spr + wvu * GSTP;
    double2_t pg[NPH];                                // the pieces of the NEXT half-step
    double pm[NP];
    double nr[4], nc[4], nnr[4], nnc[4];
    long tile = blockIdx.x;
    if (tile >= ntiles) return;
    int2 tc2 = tiles[tile];
    auto fetch = [&](int2 tl, auto hc, bool norms) {   // half hc of tile tl -> pg (and its norms -> nnr / nnc)
        constexpr int H = decltype(hc)::value;
        const double* gp = XT + (sside ? (long)tl.y * ST : (long)tl.x * ST) + 2 * spr + (long)(wvu + 4 * H * NPH) * ldp;
#pragma unroll
        for (int i = 0; i < NPH; ++i) pg[i] = *(const double2_t*)(gp + (long)(4 * i) * ldp);
        if (norms) {
#pragma unroll
            for (int a = 0; a < 4; ++a) nnr[a] = nrm[(long)tl.x * ST + 16 * wave + 4 * a + l4];
#pragma unroll
            for (int q = 0; q < 4; ++q) nnc[q] = nrm[(long)tl.y * ST + 16 * q + l15];
        }
    };
    auto commit = [&](auto hc) {                       // pg (half hc) -> LDS, centred
        constexpr int H = decltype(hc)::value;
#pragma unroll
        for (int i = 0; i < NPH; ++i)
            *(double2_t*)(slp + 4 * i * GSTP) = double2_t{pg[i][0] - pm[H * NPH + i], pg[i][1] - pm[H * NPH + i]};
    };
#pragma unroll
    for (int i = 0; i < NP; ++i) pm[i] = mu[wvu + 4 * i];
    fetch(tc2, GIC<0>{}, true);
    commit(GIC<0>{});
#pragma unroll
    for (int a = 0; a < 4; ++a) { nr[a] = -0.5 * nnr[a]; nc[a] = -0.5 * nnc[a]; }      // halved, negated: see the accumulators
    if (HV == 2) fetch(tc2, GIC<HV - 1>{}, false);    // the first tile's second half
    lds_barrier();
    const double* ap = xr + l4 * GSTP + 16 * wave + l15;
    const double* bp = xc + l4 * GSTP + l15;
    const bool odd = l15 & 1;
    const int pr = t & 31, rw = t >> 5;
    while (true) {
        const long r0 = (long)tc2.x * ST, c0 = (long)tc2.y * ST;
        const long next = tile + gridDim.x;
        const int2 nx = tiles[next < ntiles ? next : tile];       // always a valid tile: the body stays one basic block
        if (HV == 1) fetch(nx, GIC<0>{}, true);
        // the accumulators start at -(|a|^2 + |b|^2) / 2: what comes out of the products is x = -r^2 / 2 itself (the same terms
        // as |a|^2 + |b|^2 - 2 a.b, scaled by the exact factor -1/2; the diagonal is forced below)
        gram4_t acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int a = 0; a < 4; ++a) acc[q][a] = nr[a] + nc[q];
#pragma unroll
        for (int h = 0; h < HV; ++h) {
            if (h == 1) {
                lds_barrier();                         // every wave has read the first half
                commit(GIC<HV - 1>{});                 // this tile's second half (in flight since the previous tile's stores)
                lds_barrier();
                fetch(nx, GIC<0>{}, true);             // the next tile's first half: lands under this half's products and the epilogue
            }
            double fa0 = ap[0], fb0[4] = {bp[0], bp[16], bp[32], bp[48]};
#pragma unroll
            for (int ks = 0; ks < DPH; ks += 8) {
                const double* a1 = ap + (ks + 4) * GSTP;
                const double* b1 = bp + (ks + 4) * GSTP;
                const double fa1 = a1[0], fb1[4] = {b1[0], b1[16], b1[32], b1[48]};
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa0, fb0[q], acc[q], 0, 0, 0);
                if (ks + 8 < DPH) {
                    const double* a2 = ap + (ks + 8) * GSTP;
                    const double* b2 = bp + (ks + 8) * GSTP;
                    fa0 = a2[0]; fb0[0] = b2[0]; fb0[1] = b2[16]; fb0[2] = b2[32]; fb0[3] = b2[48];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa1, fb1[q], acc[q], 0, 0, 0);
            }
        }
        // The scalar map, the direct stores and the LDS writes of the mirror image are ONE pass over the accumulators, two values at
        // a time: the 8 direct store instructions go out spread over the ~1700 cycles of the map instead of as a burst behind it.
        // The exact entries -- K_ii = sf2 (r^2 = 0 by definition, not by cancellation), and in the factor form the unit diagonal, the
        // identity on the padding and the zeros below the diagonal -- only exist on diagonal tiles and on the last tile row / column:
        // a uniform branch per pair that touches the two values only (two separate code paths for the tile kinds SPILL: the
        // allocator keeps both alive).
        const int nrl = (int)(n - r0 < ST ? n - r0 : ST), ncl = (int)(n - c0 < ST ? n - c0 : ST);    // live rows / columns of this tile
        const bool dtile = tc2.x == tc2.y;
        const bool special = dtile || (MODE == MODE_FACTOR && (nrl < ST || ncl < ST));
        auto exact = [&](double val, int a, int q) -> double {
            const int rl = 16 * wave + 4 * a + l4, cl = 16 * q + l15;
            const bool same = dtile && rl == cl;
            val = same ? cpre : val;
            if (MODE == MODE_FACTOR) {
                const double live = val + (same ? 1.0 : 0.0), pad = same ? 1.0 : 0.0;
                val = (rl < nrl && cl < ncl) ? live : pad;
                val = (dtile && cl < rl) ? 0.0 : val;              // exact zeros below the diagonal (row-major upper view)
            }
            return val;
        };
        if (MODE == MODE_SYM) lds_barrier();           // every wave has read this tile's coordinates: the region takes the mirror image
        {
            double* rowp = out + (r0 + 16 * wave + (odd ? 4 : 0) + l4) * ldo + c0 + (l15 & ~1);
#pragma unroll
            for (int a = 0; a < 4; a += 2) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    double x0 = exp_nonpos_tab(clamp_exp_arg(acc[q][a]), etab), x1 = exp_nonpos_tab(clamp_exp_arg(acc[q][a + 1]), etab);
                    if (special) { x0 = exact(x0, a, q); x1 = exact(x1, a + 1, q); }
                    if (MODE == MODE_SYM) {
                        gsm[(16 * q + l15) * GSTP + 16 * wave + 4 * a + l4] = x0;
                        gsm[(16 * q + l15) * GSTP + 16 * wave + 4 * (a + 1) + l4] = x1;
                    }
                    const double n0 = gram_swap_adjacent(x0), n1 = gram_swap_adjacent(x1);
                    *(double2_t*)(rowp + 16 * q) = odd ? double2_t{n1, x1} : double2_t{x0, n0};
                    __builtin_amdgcn_sched_barrier(0);
                }
                rowp += 8 * ldo;
            }
        }
        if (MODE == MODE_SYM) {
            // mirrored store out[c][r]: the transposed image in LDS, 8 x 16 bytes per lane
            lds_barrier();
            double* colp = out + (c0 + rw) * ldo + r0 + 2 * pr;
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                *(double2_t*)colp = *(const double2_t*)(gsm + (p * 8 + rw) * GSTP + 2 * pr);
                colp += 8 * ldo;
            }
        }
        if (next >= ntiles) break;
        tile = next;
        lds_barrier();                                 // every wave is done with the LDS image of this tile (and of its mirror)
        commit(GIC<0>{});                              // (the wait for pg is an exact vmcnt(#stores issued since): the stores keep draining)
#pragma unroll
        for (int a = 0; a < 4; ++a) { nr[a] = -0.5 * nnr[a]; nc[a] = -0.5 * nnc[a]; }      // halved, negated: see the accumulators
        if (HV == 2) fetch(nx, GIC<HV - 1>{}, false);
        lds_barrier();
        tc2 = nx;
    }
}

__global__ void self_fill_kernel(double* out, long m, double val) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) out[i] = val;
}

}  // namespace

int scale_transpose_launch(const double* x, long n, int d, const double* scale_dev, double* XsT, long ldp, int dpad,
                           hipStream_t st) {
    dim3 grid((unsigned)((ldp + 255) / 256), (unsigned)dpad);
    hipLaunchKernelGGL(scale_transpose_kernel, grid, dim3(256), 0, st, x, n, d, scale_dev, XsT, ldp, dpad);
    return hipGetLastError() == hipSuccess ? PGP_OK : PGP_ERR_HIP;
}

// (ti, tj) lists, cached per device and shape.  kind 0: row-major ntr x ntc ('cross'); kind 1: upper-triangular tiles of
// an nt x nt grid walked in SUPER x SUPER super-tiles (tiles in flight together cover 512 x 512 blocks: both the direct
// and the mirrored stores land in 4 KB runs per matrix row).
static std::mutex g_tab_mu;
static std::map<std::vector<long>, std::pair<int2*, long>> g_tabs;
static int tile_table(int tri, long ntr, long ntc, const int2** tab, long* cnt) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return PGP_ERR_HIP;
    std::lock_guard<std::mutex> lk(g_tab_mu);
    const std::vector<long> key = {dev, tri, ntr, ntc};
    auto it = g_tabs.find(key);
    if (it == g_tabs.end()) {
        std::vector<int2> h;
        if (!tri) {
            for (long i = 0; i < ntr; ++i) for (long j = 0; j < ntc; ++j) h.push_back(make_int2((int)i, (int)j));
        } else {
            const long S = SUPER > 0 ? SUPER : 1, nst = (ntr + S - 1) / S;
            for (long SI = 0; SI < nst; ++SI)
                for (long SJ = SI; SJ < nst; ++SJ)
                    for (long i = SI * S; i < std::min(ntr, SI * S + S); ++i)
                        for (long j = std::max(i, SJ * S); j < std::min(ntr, SJ * S + S); ++j) h.push_back(make_int2((int)i, (int)j));
        }
        int2* d = nullptr;
        if (hipMalloc((void**)&d, std::max<size_t>(1, h.size()) * sizeof(int2)) != hipSuccess) return PGP_ERR_HIP;
        if (!h.empty() && hipMemcpy(d, h.data(), h.size() * sizeof(int2), hipMemcpyHostToDevice) != hipSuccess) return PGP_ERR_HIP;
        it = g_tabs.emplace(key, std::make_pair(d, (long)h.size())).first;
    }
    *tab = it->second.first; *cnt = it->second.second;
    return PGP_OK;
}

// kind 3: the tiles of the column-major lower panel of tile columns [t0, t1) of an nt x nt factor: (i, j) with i in
// [t0, t1), j >= i (the kernel's "row" index i is the factor's COLUMN: row-major upper == column-major lower)
static int panel_tile_table(long nt, long t0, long t1, const int2** tab, long* cnt) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return PGP_ERR_HIP;
    std::lock_guard<std::mutex> lk(g_tab_mu);
    const std::vector<long> key = {dev, 3, nt, t0, t1};
    auto it = g_tabs.find(key);
    if (it == g_tabs.end()) {
        std::vector<int2> h;
        for (long i = t0; i < t1; ++i)
            for (long j = i; j < nt; ++j) h.push_back(make_int2((int)i, (int)j));
        int2* d = nullptr;
        if (hipMalloc((void**)&d, std::max<size_t>(1, h.size()) * sizeof(int2)) != hipSuccess) return PGP_ERR_HIP;
        if (!h.empty() && hipMemcpy(d, h.data(), h.size() * sizeof(int2), hipMemcpyHostToDevice) != hipSuccess) return PGP_ERR_HIP;
        it = g_tabs.emplace(key, std::make_pair(d, (long)h.size())).first;
    }
    *tab = it->second.first; *cnt = it->second.second;
    return PGP_OK;
}

                                                   // (round 4, three alternations on one box, full symmetric RBF d = 16: N = 16384 56-58 % of the HBM peak
                                                   //  at 2048 workgroups, 62-64 % at 4096; N = 8192 61-62 % / 62-65 %)

template <int MODE>
static int cov_tile_dispatch(const CovSpec& cs, int train, long ntr, long ntc_, hipStream_t st, const double* XrT, long ldr,
                             long n, const double* XcT, long ldc, long m, int dpad, double inv_sn2, double* out,
                             long ldo, const int2* tiles = nullptr, long ntiles = 0) {
    if (!tiles) { const int rc = tile_table(MODE != MODE_RECT, ntr, ntc_, &tiles, &ntiles); if (rc != PGP_OK) return rc; }
    if (ntiles == 0) return PGP_OK;
    const unsigned nblk = cs.asm_grid > 0 ? (unsigned)std::min<long>(ntiles, cs.asm_grid) : (unsigned)ntiles;
    const int nt_ = cs.asm_nt >= 0 ? cs.asm_nt : ((MODE != MODE_FACTOR && (double)n * (double)m * 8.0 >= 1073741824.0) ? 1 : 0);
    if (cs.sm) {
        const CovSM P = sm_resolved(cs);
        hipLaunchKernelGGL((cov_tile_kernel<MODE, CovSM, 0, false, false>), dim3(nblk), dim3(256), 0, st, XrT, ldr, n, XcT, ldc, m,
                           dpad, P, inv_sn2, out, ldo, tiles, ntiles, nt_);
    } else if (cs.prog) {
        CovProgram pg = cs.pg;
        for (int l = 0; l < pg.nleaf; ++l) pg.leaf[l].train = train;
        for (int la : {pg.ard_leaf, pg.ard_leaf2})
            if (la >= 0 && pg.leaf[la].kind == 6 && pg.leaf[la].ref_der)
                pg.leaf[la].gb = train == 1 ? 0.0 : cs.ell4;                      // Core/cov.py:1415-1418 as returned
        if (pg.pre_leaf >= 0) {
            // the leaf's matrix: M2 on 'train', the caller's block of the transposed M1 on 'cross' (CovSpec::pre_cross, predict.hip)
            pg.pre = train == 1 ? cs.pre_train : cs.pre_cross;
            pg.pre_ld = cs.pre_ld;
            if (!pg.pre || pg.pre_ld <= 0) return -14;
            // every tile the kernel visits lies inside the padded resident matrix
            if (train == 1 ? ntr * ST > cs.pre_rows || ntc_ * ST > cs.pre_ld : ntr * ST > cs.pre_cross_rows || ntc_ * ST > cs.pre_ld) return -14;
#define PRE_LAUNCH(K) hipLaunchKernelGGL((cov_tile_kernel<MODE, CovProgram, K, false, false>), dim3(nblk), dim3(256), 0, st, XrT, ldr, n, \
                                         XcT, ldc, m, dpad, pg, inv_sn2, out, ldo, tiles, ntiles, nt_)
            if (pg.ard_leaf2 >= 0) PRE_LAUNCH(6); else if (pg.ard_leaf >= 0) PRE_LAUNCH(5); else PRE_LAUNCH(4);
#undef PRE_LAUNCH
        } else if (pg.dot_mask) {
            if (pg.ard_leaf2 >= 0) return -13;        // the dot product is the second extra accumulator (make_spec refuses this too)
            if (pg.ard_leaf >= 0)
                hipLaunchKernelGGL((cov_tile_kernel<MODE, CovProgram, 9, false, false>), dim3(nblk), dim3(256), 0, st, XrT, ldr, n,
                                   XcT, ldc, m, dpad, pg, inv_sn2, out, ldo, tiles, ntiles, nt_);
            else
                hipLaunchKernelGGL((cov_tile_kernel<MODE, CovProgram, 8, false, false>), dim3(nblk), dim3(256), 0, st, XrT, ldr, n,
                                   XcT, ldc, m, dpad, pg, inv_sn2, out, ldo, tiles, ntiles, nt_);
        } else if (pg.ard_leaf2 >= 0)
            hipLaunchKernelGGL((cov_tile_kernel<MODE, CovProgram, 2, false, false>), dim3(nblk), dim3(256), 0, st, XrT, ldr, n,
                               XcT, ldc, m, dpad, pg, inv_sn2, out, ldo, tiles, ntiles, nt_);
        else if (pg.ard_leaf >= 0)
            hipLaunchKernelGGL((cov_tile_kernel<MODE, CovProgram, 1, false, false>), dim3(nblk), dim3(256), 0, st, XrT, ldr, n,
                               XcT, ldc, m, dpad, pg, inv_sn2, out, ldo, tiles, ntiles, nt_);
        else
            hipLaunchKernelGGL((cov_tile_kernel<MODE, CovProgram, 0, false, false>), dim3(nblk), dim3(256), 0, st, XrT, ldr, n,
                               XcT, ldc, m, dpad, pg, inv_sn2, out, ldo, tiles, ntiles, nt_);
    } else {
        CovParams cp = cs.cp;
        cp.train = train;
        if (cp.kind == 6 && cp.ref_der) cp.gb = train == 1 ? 0.0 : cs.ell4;       // Core/cov.py:1415-1418 as returned
        // kernel family and value/derivative choice are compile-time parameters of the kernel: one functor's code
        // and constants per instantiation (the persistent tile loop keeps hoisted constants live)
        const bool fast = ((ldo | n | m) & 1) == 0;
#define LAUNCH(K, D, F) hipLaunchKernelGGL((cov_tile_kernel<MODE, CovParams, K, D, F>), dim3(nblk), dim3(256), 0, st, XrT, ldr, \
                                           n, XcT, ldc, m, dpad, cp, inv_sn2, out, ldo, tiles, ntiles, nt_)
#define LAUNCH_K(K) do { if (cp.der < 0) { if (fast) LAUNCH(K, false, true); else LAUNCH(K, false, false); } \
                         else LAUNCH(K, true, false); } while (0)
        switch (cp.kind) {
            case 0: LAUNCH_K(0); break;
            case 1: LAUNCH_K(1); break;
            case 2: LAUNCH_K(2); break;
            case 3: LAUNCH_K(3); break;
            case 4: LAUNCH_K(4); break;
            case 5: LAUNCH_K(5); break;
            case 6: LAUNCH_K(6); break;
            default: return -2;
        }
#undef LAUNCH_K
#undef LAUNCH
    }
    return hipGetLastError() == hipSuccess ? PGP_OK : PGP_ERR_HIP;
}

int cov_sym_launch(const double* XT, long ldp, long n, int dpad, const CovSpec& cs, double* out, hipStream_t st,
                   long ldo) {
    const long nt = (n + ST - 1) / ST;
    return cov_tile_dispatch<MODE_SYM>(cs, 1, nt, nt, st, XT, ldp, n, XT, ldp, n, dpad, 0.0, out, ldo > 0 ? ldo : n);
}

int cov_rect_launch(const double* XrT, long ldr, long n, const double* XcT, long ldc, long m, int dpad,
                    const CovSpec& cs, double* out, long ldo, hipStream_t st) {
    const long ntr = (n + ST - 1) / ST, ntc = (m + ST - 1) / ST;
    return cov_tile_dispatch<MODE_RECT>(cs, 0, ntr, ntc, st, XrT, ldr, n, XcT, ldc, m, dpad, 0.0, out, ldo);
}

int cov_factor_launch(const double* XT, long ldp, long n, long np, int dpad, const CovSpec& cs, double inv_sn2,
                      double* Bf, long ldf, hipStream_t st) {
    const long nt = np / ST;
    return cov_tile_dispatch<MODE_FACTOR>(cs, 1, nt, nt, st, XT, ldp, n, XT, ldp, n, dpad, inv_sn2, Bf, ldf);
}

// Gram-form assembly (cov_gram_kernel): RBF / RBFard values, 'train' only.  prep = [coordinate means (HADAMARD-prep layout:
// HADAMARD_PREP_MU doubles) | squared norms of the centred points (np)], produced by hadamard_prepare_launch for the same XT.
static int cov_gram_dispatch(int mode, const double* XT, long ldp, long n, long nt, int dpad, const CovSpec& cs, double inv_sn2,
                             double* out, long ldo, const double* prep, hipStream_t st) {
    const int2* tiles = nullptr;
    long ntiles = 0;
    { const int rc = tile_table(1, nt, nt, &tiles, &ntiles); if (rc != PGP_OK) return rc; }
    if (ntiles == 0) return PGP_OK;
    const int CH = dpad < 64 ? dpad : 64;
    const size_t shm = std::max<size_t>((size_t)2 * CH * GSTP, (size_t)ST * GSTP) * sizeof(double);
    const int nt_ = cs.asm_nt >= 0 ? cs.asm_nt : ((mode != MODE_FACTOR && (double)n * (double)n * 8.0 >= 1073741824.0) ? 1 : 0);
    const unsigned grid = (unsigned)std::min<long>(ntiles, cs.gram_grid > 0 ? cs.gram_grid : 2048);   // persistent: 2 resident per CU, the rest queue
#define GRAM_LAUNCH(M, NPV) do {                                                                                                  \
        func_max_dynamic_lds((const void*)cov_gram_kernel<M, NPV>, 70000);   /* once per instantiation and device */              \
        hipLaunchKernelGGL((cov_gram_kernel<M, NPV>), dim3(grid), dim3(256), shm, st, XT, ldp, n, dpad, cs.cp.sf2, inv_sn2, out, ldo,  \
                           tiles, ntiles, prep, prep + HADAMARD_PREP_MU, nt_);                                                     \
    } while (0)
#define GRAM_MODE(M) do { switch (dpad) { case 32: GRAM_LAUNCH(M, 8); break; case 48: GRAM_LAUNCH(M, 12); break;                  \
                                          case 64: GRAM_LAUNCH(M, 16); break; default: GRAM_LAUNCH(M, 0); } } while (0)
    // the restructured kernel: one chunk of coordinates, full tiles only, even leading dimension, ordinary stores (option "gram_fast")
    const bool fast = cs.gram_fast && (dpad == 32 || dpad == 48 || dpad == 64) && !(ldo & 1) && !nt_ &&
                      (mode == MODE_FACTOR || n % ST == 0);
#define GRAM_FAST(M, NPV) do {                                                                                                    \
        func_max_dynamic_lds((const void*)cov_gram_fast_kernel<M, NPV, 1>, 70000);                                                 \
        if (cs.gram_fast == 2 && (NPV) == 16)            /* two halves, four workgroups per CU: d = 64 (the smaller ones spill) */   \
            hipLaunchKernelGGL((cov_gram_fast_kernel<M, NPV, ((NPV) == 16 ? 2 : 1)>), dim3(grid), dim3(256),                       \
                               ((size_t)ST * GSTP + 64) * sizeof(double), st, XT, ldp, n, cs.cp.sf2, inv_sn2, out, ldo, tiles, ntiles, prep, \
                               prep + HADAMARD_PREP_MU);                                                                           \
        else                                                                                                                       \
        hipLaunchKernelGGL((cov_gram_fast_kernel<M, NPV, 1>), dim3(grid), dim3(256), shm + 64 * sizeof(double), st, XT, ldp, n, cs.cp.sf2, inv_sn2, out, ldo, \
                           tiles, ntiles, prep, prep + HADAMARD_PREP_MU);                                                          \
    } while (0)
#define GRAM_FAST_MODE(M) do { switch (dpad) { case 32: GRAM_FAST(M, 8); break; case 48: GRAM_FAST(M, 12); break;                 \
                                               default: GRAM_FAST(M, 16); } } while (0)
    if (fast) { if (mode == MODE_FACTOR) GRAM_FAST_MODE(MODE_FACTOR); else GRAM_FAST_MODE(MODE_SYM); }
    else if (mode == MODE_FACTOR) GRAM_MODE(MODE_FACTOR); else GRAM_MODE(MODE_SYM);
#undef GRAM_FAST_MODE
#undef GRAM_FAST
#undef GRAM_MODE
#undef GRAM_LAUNCH
    return hipGetLastError() == hipSuccess ? PGP_OK : PGP_ERR_HIP;
}
bool cov_gram_applies(const CovSpec& cs, int dpad) {
    // dpad <= HADAMARD_PREP_MU: the prep buffer holds that many coordinate means in front of the norms (plain RBF has no cap on d)
    return !cs.prog && !cs.sm && (cs.cp.kind == 0 || cs.cp.kind == 1) && cs.cp.der < 0 && dpad >= 32 && dpad <= HADAMARD_PREP_MU;
}
int cov_factor_gram_launch(const double* XT, long ldp, long n, long np, int dpad, const CovSpec& cs, double inv_sn2, double* Bf,
                           long ldf, const double* prep, hipStream_t st) {
    return cov_gram_dispatch(MODE_FACTOR, XT, ldp, n, np / ST, dpad, cs, inv_sn2, Bf, ldf, prep, st);
}
int cov_sym_gram_launch(const double* XT, long ldp, long n, int dpad, const CovSpec& cs, double* out, long ldo, const double* prep,
                        hipStream_t st) {
    return cov_gram_dispatch(MODE_SYM, XT, ldp, n, (n + ST - 1) / ST, dpad, cs, 0.0, out, ldo > 0 ? ldo : n, prep, st);
}

// The same fused assembly for ONE column panel of the factor: columns [col0, col0 + ncols) (multiples of 64) of B = K/sn2 + I,
// rows >= the column, written column-major into `panel` (leading dimension ldpanel) with the panel's first diagonal entry at
// panel[0] -- the storage of one owned panel of the block-cyclic sweep (csrc/sharded.hip).
int cov_factor_panel_launch(const double* XT, long ldp, long n, long np, int dpad, const CovSpec& cs, double inv_sn2,
                            long col0, long ncols, double* panel, long ldpanel, hipStream_t st) {
    const long nt = np / ST;
    const int2* tiles = nullptr;
    long ntiles = 0;
    { const int rc = panel_tile_table(nt, col0 / ST, (col0 + ncols) / ST, &tiles, &ntiles); if (rc != PGP_OK) return rc; }
    // element (row r, column c) of the factor is written at out[c * ldo + r]: shift the base so that it lands at
    // panel[(c - col0) * ldpanel + (r - col0)]
    double* out = panel - col0 * ldpanel - col0;
    return cov_tile_dispatch<MODE_FACTOR>(cs, 1, nt, nt, st, XT, ldp, n, XT, ldp, n, dpad, inv_sn2, out, ldpanel, tiles, ntiles);
}

// k(z,z) and its derivatives at zero distance ('self_test' mode): one evaluation of the functor
template <class COV>
__global__ void cov_self_kernel(COV cp, int same, double* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = cov_elem(cp, 0.0, 0.0, same != 0);
}

// Programs with a precomputed-matrix leaf: the diagonal differs from point to point.  out[j] = k_jj with the leaf's value
// pre[j * stride] (train = 1: diag(M2), stride ld + 1; train = 2: the last row of M1, 'self_test');
// sub: out[j] = max(k_jj - out[j], 0) -- the predictive variance from the column sums of squares already in out.
// Programs with dot-product leaves (DOT): k_jj from |x_j|^2 = sum_k x_jk^2 of the point's own coordinates XT[k * ld + j] (k-major,
// dpad rows, zero-padded), summed by fma in coordinate order like the tiles' dot product; pre is not read.  With a derivative
// selected (P.der >= 0) out[j] is that derivative's k_jj.
template <bool DOT>
__global__ __launch_bounds__(256) void cov_self_vec_kernel(CovProgram P, int same, const double* __restrict__ pre, long stride,
                                                           long m, double* __restrict__ out, int sub,
                                                           const double* __restrict__ XT, long ld, int dpad) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    double k;
    if constexpr (DOT) {
        double pd = 0.0;
        for (int q = 0; q < dpad; ++q) { const double v = XT[(long)q * ld + j]; pd = fma(v, v, pd); }
        const int ddk = cov_dot_der(P);
        double dk = 0.0;
        if (ddk >= 0) { const double v = XT[(long)ddk * ld + j]; dk = v * v; }
        k = cov_elem<true>(P, 0.0, dk, same != 0, 0.0, 0.0, 0.0, pd);
    } else k = cov_elem(P, 0.0, 0.0, same != 0, 0.0, 0.0, pre[j * stride]);
    out[j] = sub ? fmax(k - out[j], 0.0) : k;
}
int cov_self_vec_launch(const CovSpec& cs, int train, const double* pre, long stride, long m, double* out_dev, int sub,
                        hipStream_t st) {
    if (!cs.has_pre() || !pre) return -14;
    if (m <= 0) return PGP_OK;
    CovProgram pg = cs.pg;
    for (int l = 0; l < pg.nleaf; ++l) pg.leaf[l].train = train;
    hipLaunchKernelGGL(cov_self_vec_kernel<false>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, pg, train == 1, pre, stride, m,
                       out_dev, sub, (const double*)nullptr, 0L, 0);
    return hipGetLastError() == hipSuccess ? PGP_OK : PGP_ERR_HIP;
}
// XT: the m points' scaled, transposed coordinates (dpad x ld, ld >= m)
int cov_self_dot_launch(const CovSpec& cs, int train, const double* XT, long ld, int dpad, long m, double* out_dev, int sub,
                        hipStream_t st) {
    if (!cs.has_dot() || cs.has_pre() || !XT || ld < m) return -14;
    if (m <= 0) return PGP_OK;
    CovProgram pg = cs.pg;
    for (int l = 0; l < pg.nleaf; ++l) pg.leaf[l].train = train;
    hipLaunchKernelGGL(cov_self_vec_kernel<true>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, pg, train == 1,
                       (const double*)nullptr, 0L, m, out_dev, sub, XT, ld, dpad);
    return hipGetLastError() == hipSuccess ? PGP_OK : PGP_ERR_HIP;
}

// train = 1: a diagonal entry of the training matrix; train = 2: 'self_test'
int cov_self_launch(const CovSpec& cs, int train, double* out_dev, hipStream_t st) {
    if (cs.sm) {                                      // t = 0: sum_q w_q; d / d log w_q = w_q, every other derivative 0
        const CovSM P = sm_resolved(cs);
        return self_fill_launch(out_dev, 1, P.dt < 0 ? cs.cp.sf2 : (P.dt == 0 ? P.h[P.dq] : 0.0), st);
    }
    if (cs.prog) {
        CovProgram pg = cs.pg;
        for (int l = 0; l < pg.nleaf; ++l) pg.leaf[l].train = train;
        hipLaunchKernelGGL((cov_self_kernel<CovProgram>), dim3(1), dim3(64), 0, st, pg, train == 1, out_dev);
    } else {
        CovParams cp = cs.cp;
        cp.train = train;
        hipLaunchKernelGGL((cov_self_kernel<CovParams>), dim3(1), dim3(64), 0, st, cp, train == 1, out_dev);
    }
    return hipGetLastError() == hipSuccess ? PGP_OK : PGP_ERR_HIP;
}

int self_fill_launch(double* out, long m, double val, hipStream_t st) {
    hipLaunchKernelGGL(self_fill_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, out, m, val);
    return hipGetLastError() == hipSuccess ? PGP_OK : PGP_ERR_HIP;
}
