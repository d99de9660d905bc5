// Propagation kernels between whole graphs (pyGPs/GraphExtensions/graphKernels.py:27-184; Neumann et al., ECML/PKDD 2012) on the
// device: pgp_propagation_kernel.  One upload, h_max + 1 iterations without a host round trip, one download.
//
// Per iteration h:
//   update   (h > 0)  lab <- T lab: CSR times dense (n x k), summed in the stored CSR order with a separate multiply and add.  The
//                     push-back of 'label_propagation' (rows of the mask read lab_orig) and the term of 'label_spreading'
//                     (+ orig_weight lab_orig) are folded into the same kernel; two buffers alternate.
//   hash              sqrt in place (Hellinger), dot = sum_j lab_ij v_j over j in order, key = floor((dot + b) / w) with -0.0
//                     made 0.0, stored as its 64-bit pattern at the node's place in graph-grouped order.  A non-finite key sets
//                     the context's error word.
//   sort              one workgroup per graph: bitonic network over its keys (in LDS up to PGP_PROP_SORT_LDS keys, the same
//                     network on a global scratch beyond), then run-length encoding into (key, count) pairs.
//   gram              K_h[g1, g2] = sum over equal keys of c1 c2: a 16 x 16 tile of graph pairs per workgroup, the 32 lists in
//                     LDS (read from global memory when they do not fit), one thread per pair merging two sorted lists, 64-bit
//                     integer sums in registers.  Lower triangle only, mirrored on the store.  No atomics anywhere: every
//                     output element has one owner.  Work: sum over pairs of (L1 + L2) = N n.
// Every floating-point step has a defined order and no contraction, so a host restatement with the same order gives the same
// keys bit for bit; the counts are integers, exact and independent of order.
#include <cmath>
#include <cstdint>
#include <vector>

#include "ctx.h"

#pragma clang fp contract(off)

namespace {

constexpr int SORT_LDS = PGP_PROP_SORT_LDS;
constexpr int GRAM_LDS = PGP_PROP_GRAM_LDS;
constexpr int GT = 16;                                  // graphs per tile edge: 256 threads, one pair each
constexpr unsigned long long PAD_KEY = ~0ull;           // sorts last; a NaN pattern, so no finite key equals it

// out[i, :] = sum_e vals[e] src(cols[e], :) (+ orig_weight orig[i, :]), src(c) = orig[c] where mask[c], else lab[c].
// kw lanes (a power of two, <= 64) share a row and stride over its k columns.
__global__ __launch_bounds__(256) void prop_update_kernel(const long long* __restrict__ indptr, const int* __restrict__ cols,
                                                          const double* __restrict__ vals, const double* __restrict__ lab,
                                                          const double* __restrict__ orig, const unsigned char* __restrict__ mask,
                                                          int spread, double orig_weight, long n, int k, int kw,
                                                          double* __restrict__ out) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long i = t / kw;
    const int j0 = (int)(t - i * kw);
    if (i >= n) return;
    const long long e0 = indptr[i], e1 = indptr[i + 1];
    for (int j = j0; j < k; j += kw) {
        double acc = 0.0;
        for (long long e = e0; e < e1; ++e) {
            const long c = cols[e];
            const double* src = (mask && mask[c]) ? orig : lab;
            const double prod = vals[e] * src[c * k + j];
            acc = acc + prod;
        }
        if (spread) {
            const double keep = orig_weight * orig[i * k + j];
            acc = acc + keep;
        }
        out[i * k + j] = acc;
    }
}

// one thread per node, in grouped order: p -> node perm[p]
__global__ __launch_bounds__(256) void prop_hash_kernel(double* __restrict__ lab, const int* __restrict__ perm, const double* __restrict__ v,
                                                        double b, double w, int take_sqrt, long n, int k,
                                                        unsigned long long* __restrict__ keys, int* __restrict__ err) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    double* row = lab + (long)perm[p] * k;
    double dot = 0.0;
    for (int j = 0; j < k; ++j) {
        double x = row[j];
        if (take_sqrt) {
            x = __dsqrt_rn(x);
            row[j] = x;
        }
        const double prod = x * v[j];
        dot = dot + prod;
    }
    const double shifted = dot + b;
    double key = floor(shifted / w);
    if (key == 0.0) key = 0.0;                          // -0.0 and 0.0 are one bin
    if (!(fabs(key) <= 1.79769313486231570815e308)) *err = 1;      // (every thread that stores, stores the same word)
    keys[p] = (unsigned long long)__double_as_longlong(key);
}

// ascending bitonic network over s[0 .. P), P a power of two, by the 256 threads of the workgroup
__device__ __forceinline__ void bitonic_sort(unsigned long long* s, long P) {
    for (long size = 2; size <= P; size <<= 1)
        for (long stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (long t = threadIdx.x; t < P / 2; t += 256) {
                const long lo = 2 * t - (t & (stride - 1));
                const long hi = lo + stride;
                const unsigned long long a = s[lo], c = s[hi];
                if ((a > c) == ((lo & size) == 0)) { s[lo] = c; s[hi] = a; }
            }
        }
    __syncthreads();
}

// s[0 .. L) sorted -> (key, count) pairs at uk / uc, their number at *ulen.  Heads are numbered by a scan over rounds of 256;
// a run's length is the distance to the upper bound of its key.
__device__ __forceinline__ void run_lengths(const unsigned long long* s, long L, unsigned long long* uk, int* uc, int* ulen, int* wtot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long base = 0;
    for (long i0 = 0; i0 < L; i0 += 256) {
        const long i = i0 + threadIdx.x;
        const bool head = i < L && (i == 0 || s[i] != s[i - 1]);
        const unsigned long long m = __ballot(head);
        if (lane == 0) wtot[wave] = __popcll(m);
        __syncthreads();
        long pos = base + __popcll(m & ((1ull << lane) - 1ull));
        for (int q = 0; q < wave; ++q) pos += wtot[q];
        base += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        __syncthreads();
        if (head) {
            const unsigned long long key = s[i];
            long lo = i + 1, hi = L;                    // first index in (i, L] whose key is greater
            while (lo < hi) {
                const long mid = lo + ((hi - lo) >> 1);
                if (s[mid] > key) hi = mid; else lo = mid + 1;
            }
            uk[pos] = key;
            uc[pos] = (int)(lo - i);
        }
    }
    if (threadIdx.x == 0) *ulen = (int)base;
}

// one workgroup per graph g: keys[seg[g] .. seg[g + 1]) -> sorted (key, count) pairs at the same offset, ulen[g] of them
__global__ __launch_bounds__(256) void prop_sort_kernel(const unsigned long long* __restrict__ keys, const long long* __restrict__ seg,
                                                        const long long* __restrict__ long_off, unsigned long long* __restrict__ long_buf,
                                                        unsigned long long* __restrict__ uk, int* __restrict__ uc, int* __restrict__ ulen) {
    __shared__ unsigned long long sl[SORT_LDS];
    __shared__ int wtot[4];
    const long g = blockIdx.x;
    const long s0 = seg[g], L = seg[g + 1] - s0;
    if (L <= 0) {
        if (threadIdx.x == 0) ulen[g] = 0;
        return;
    }
    long P = 1;
    while (P < L) P <<= 1;
    if (L <= SORT_LDS) {
        for (long i = threadIdx.x; i < P; i += 256) sl[i] = i < L ? keys[s0 + i] : PAD_KEY;
        bitonic_sort(sl, P);
        run_lengths(sl, L, uk + s0, uc + s0, ulen + g, wtot);
    } else {
        unsigned long long* s = long_buf + long_off[g];
        for (long i = threadIdx.x; i < P; i += 256) s[i] = i < L ? keys[s0 + i] : PAD_KEY;
        bitonic_sort(s, P);
        run_lengths(s, L, uk + s0, uc + s0, ulen + g, wtot);
    }
}

// sum of c1 c2 over the keys two sorted lists share
template <typename KP, typename CP>
__device__ __forceinline__ long long merge_dot(KP k1, CP c1, int L1, KP k2, CP c2, int L2) {
    long long acc = 0;
    int i = 0, j = 0;
    while (i < L1 && j < L2) {
        const unsigned long long a = k1[i], b = k2[j];
        if (a == b) acc += (long long)c1[i] * (long long)c2[j];
        i += (a <= b);
        j += (b <= a);
    }
    return acc;
}

// tile (blockIdx.y, blockIdx.x) of the lower triangle; thread (r, c) owns the pair (ty GT + r, tx GT + c) and its mirror image.
// out is (N, N, H1) row-major; ksum (N x N, lower triangle used) carries the running sum when `sum` is set.
__global__ __launch_bounds__(256) void prop_gram_kernel(const unsigned long long* __restrict__ uk, const int* __restrict__ uc,
                                                        const int* __restrict__ ulen, const long long* __restrict__ seg, long N, int h,
                                                        int H1, int sum, long long* __restrict__ ksum, double* __restrict__ out) {
    __shared__ unsigned long long sk[GRAM_LDS];
    __shared__ int sc[GRAM_LDS];
    __shared__ int off[2 * GT + 1];
    __shared__ int len[2 * GT];
    if (blockIdx.x > blockIdx.y) return;
    const long g1_0 = (long)blockIdx.y * GT, g2_0 = (long)blockIdx.x * GT;
    if (threadIdx.x < 2 * GT) {
        const long g = threadIdx.x < GT ? g1_0 + threadIdx.x : g2_0 + (threadIdx.x - GT);
        len[threadIdx.x] = g < N ? ulen[g] : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long total = 0;                                 // (long: 32 lists of up to 2^31 - 1 entries)
        for (int s = 0; s < 2 * GT; ++s) {
            off[s] = total <= GRAM_LDS ? (int)total : GRAM_LDS + 1;
            total += len[s];
        }
        off[2 * GT] = total <= GRAM_LDS ? (int)total : GRAM_LDS + 1;
    }
    __syncthreads();
    const bool in_lds = off[2 * GT] <= GRAM_LDS;
    if (in_lds) {
        const int s = threadIdx.x >> 3;                 // eight threads per list
        const long g = s < GT ? g1_0 + s : g2_0 + (s - GT);
        if (g < N) {
            const long src = seg[g];
            for (int e = threadIdx.x & 7; e < len[s]; e += 8) {
                sk[off[s] + e] = uk[src + e];
                sc[off[s] + e] = uc[src + e];
            }
        }
    }
    __syncthreads();
    const int r = threadIdx.x >> 4, c = threadIdx.x & 15;
    const long g1 = g1_0 + r, g2 = g2_0 + c;
    if (g1 >= N || g2 > g1) return;
    long long acc;
    if (in_lds)
        acc = merge_dot(sk + off[r], sc + off[r], len[r], sk + off[GT + c], sc + off[GT + c], len[GT + c]);
    else
        acc = merge_dot(uk + seg[g1], uc + seg[g1], len[r], uk + seg[g2], uc + seg[g2], len[GT + c]);
    if (sum) {
        if (h > 0) acc += ksum[g1 * N + g2];
        ksum[g1 * N + g2] = acc;
    }
    const double val = (double)acc;
    out[(g1 * N + g2) * H1 + h] = val;
    out[(g2 * N + g1) * H1 + h] = val;
}

enum { ST_UPLOAD = 0, ST_UPDATE, ST_HASH, ST_SORT, ST_GRAM, ST_DOWNLOAD, ST_COUNT };

// stage clock for tools/propagation_time.py: events on the stream at the stage boundaries, read after the last synchronisation
struct StageClock {
    hipStream_t st;
    bool on;
    std::vector<std::pair<int, hipEvent_t>> marks;      // (stage that ENDS here, event); the first mark only opens
    StageClock(hipStream_t st_, bool on_) : st(st_), on(on_) {}
    ~StageClock() { for (auto& m : marks) (void)hipEventDestroy(m.second); }
    int mark(int stage) {
        if (!on) return PGP_OK;
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        marks.push_back({stage, e});
        HIP_TRY(hipEventRecord(e, st));
        return PGP_OK;
    }
    int read(double* ms) {
        for (int s = 0; s < ST_COUNT; ++s) ms[s] = 0.0;
        for (size_t i = 1; i < marks.size(); ++i) {
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, marks[i - 1].second, marks[i].second));
            ms[marks[i].first] += t;
        }
        return PGP_OK;
    }
};

}  // namespace

extern "C" {

int pgp_propagation_kernel(pgp_ctx* c, int64_t n, int64_t k, int64_t n_graphs, const int64_t* indptr, const int32_t* indices,
                           const double* vals, const double* lab_prob, const double* lab_orig, const uint8_t* push_back,
                           const int32_t* perm, const int64_t* seg, int h_max, const double* V, const double* b, double w, int update,
                           double orig_weight, int take_sqrt, int sum, double* K_out, double* lab_out, double* stage_ms_out) {
    if (!c) return -1;
    GateShared device_gate_hold(c);
    if (n <= 0 || n > 2147483647LL) return -2;
    if (k < 2 || k > PGP_PROP_MAX_LABELS) return -3;
    if (n_graphs <= 0 || n_graphs > n) return -4;
    if (update < PGP_PROP_NONE || update > PGP_PROP_SPREAD) return -5;
    if (update != PGP_PROP_NONE && (!indptr || !indices || !vals)) return -6;
    if (!lab_prob) return -7;
    if ((update == PGP_PROP_SPREAD || push_back) && !lab_orig) return -8;
    if (!perm || !seg) return -9;
    if (h_max < 0 || h_max > 1000000) return -10;
    if (!V || !b) return -11;
    if (!(w > 0.0) || !(w <= 1.79769313486231570815e308)) return -12;
    if (!K_out) return -13;
    // everything a kernel indexes with is checked here: row pointers, column indices, the permutation, the segments
    int64_t nnz = 0;
    if (update != PGP_PROP_NONE) {
        if (indptr[0] != 0) return -6;
        for (int64_t i = 0; i < n; ++i)
            if (indptr[i + 1] < indptr[i]) return -6;
        nnz = indptr[n];
        for (int64_t e = 0; e < nnz; ++e)
            if (indices[e] < 0 || indices[e] >= n) return -6;
    }
    {
        std::vector<char> seen((size_t)n, 0);
        for (int64_t p = 0; p < n; ++p) {
            if (perm[p] < 0 || perm[p] >= n || seen[(size_t)perm[p]]) return -9;
            seen[(size_t)perm[p]] = 1;
        }
        if (seg[0] != 0 || seg[n_graphs] != n) return -9;
        for (int64_t g = 0; g < n_graphs; ++g)
            if (seg[g + 1] < seg[g]) return -9;
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->st;
    const long N = (long)n_graphs;
    const int H1 = h_max + 1;
    const size_t nk = (size_t)n * (size_t)k * sizeof(double);
    const size_t kbytes = (size_t)N * (size_t)N * (size_t)H1 * sizeof(double);

    // segments longer than the LDS sort: a power-of-two scratch each
    std::vector<long long> long_off((size_t)N, -1);
    size_t long_total = 0;
    for (long g = 0; g < N; ++g) {
        const int64_t L = seg[g + 1] - seg[g];
        if (L > SORT_LDS) {
            size_t P = 1;
            while ((int64_t)P < L) P <<= 1;
            long_off[(size_t)g] = (long long)long_total;
            long_total += P;
        }
    }

    PoolScratch scr(c);
    long long *indptr_d = nullptr, *seg_d = nullptr, *long_off_d = nullptr, *ksum = nullptr;
    int *cols_d = nullptr, *perm_d = nullptr, *uc = nullptr, *ulen = nullptr;
    double *vals_d = nullptr, *lab0 = nullptr, *lab1 = nullptr, *orig_d = nullptr, *V_d = nullptr, *K_d = nullptr;
    unsigned char* mask_d = nullptr;
    unsigned long long *keys = nullptr, *uk = nullptr, *long_buf = nullptr;
    CHK(scr.alloc(&lab0, nk));
    CHK(scr.alloc(&perm_d, (size_t)n * sizeof(int)));
    CHK(scr.alloc(&seg_d, (size_t)(N + 1) * sizeof(long long)));
    CHK(scr.alloc(&long_off_d, (size_t)N * sizeof(long long)));
    CHK(scr.alloc(&V_d, (size_t)H1 * (size_t)k * sizeof(double)));
    CHK(scr.alloc(&keys, (size_t)n * sizeof(unsigned long long)));
    CHK(scr.alloc(&uk, (size_t)n * sizeof(unsigned long long)));
    CHK(scr.alloc(&uc, (size_t)n * sizeof(int)));
    CHK(scr.alloc(&ulen, (size_t)N * sizeof(int)));
    CHK(scr.alloc(&K_d, kbytes));
    if (sum) CHK(scr.alloc(&ksum, (size_t)N * (size_t)N * sizeof(long long)));
    if (long_total) CHK(scr.alloc(&long_buf, long_total * sizeof(unsigned long long)));
    if (update != PGP_PROP_NONE) {
        CHK(scr.alloc(&lab1, nk));
        CHK(scr.alloc(&indptr_d, (size_t)(n + 1) * sizeof(long long)));
        CHK(scr.alloc(&cols_d, (size_t)nnz * sizeof(int)));
        CHK(scr.alloc(&vals_d, (size_t)nnz * sizeof(double)));
        if (lab_orig) CHK(scr.alloc(&orig_d, nk));
        if (push_back) CHK(scr.alloc(&mask_d, (size_t)n));
    }

    StageClock clock(st, stage_ms_out != nullptr);
    CHK(clock.mark(ST_UPLOAD));
    static_assert(sizeof(long long) == sizeof(int64_t), "row pointers and segments are uploaded as they are");
    HIP_TRY(hipMemcpyAsync(lab0, lab_prob, nk, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(perm_d, perm, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(seg_d, seg, (size_t)(N + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(long_off_d, long_off.data(), (size_t)N * sizeof(long long), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(V_d, V, (size_t)H1 * (size_t)k * sizeof(double), hipMemcpyHostToDevice, st));
    if (update != PGP_PROP_NONE) {
        HIP_TRY(hipMemcpyAsync(indptr_d, indptr, (size_t)(n + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
        if (nnz) {
            HIP_TRY(hipMemcpyAsync(cols_d, indices, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(vals_d, vals, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, st));
        }
        if (orig_d) HIP_TRY(hipMemcpyAsync(orig_d, lab_orig, nk, hipMemcpyHostToDevice, st));
        if (mask_d) HIP_TRY(hipMemcpyAsync(mask_d, push_back, (size_t)n, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemsetAsync(c->info_dev, 0, sizeof(int), st));
    CHK(clock.mark(ST_UPLOAD));

    int kw = 1;
    while (kw < k && kw < 64) kw <<= 1;
    const long tiles = (N + GT - 1) / GT;
    if (tiles > 65535) return -4;
    double *cur = lab0, *nxt = lab1;
    for (int h = 0; h < H1; ++h) {
        if (h > 0 && update != PGP_PROP_NONE) {
            hipLaunchKernelGGL(prop_update_kernel, dim3((unsigned)(((long)n * kw + 255) / 256)), dim3(256), 0, st, indptr_d, cols_d, vals_d,
                               cur, orig_d, mask_d, update == PGP_PROP_SPREAD ? 1 : 0, orig_weight, (long)n, (int)k, kw, nxt);
            std::swap(cur, nxt);
            CHK(clock.mark(ST_UPDATE));
        }
        hipLaunchKernelGGL(prop_hash_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cur, perm_d, V_d + (size_t)h * k, b[h], w,
                           take_sqrt ? 1 : 0, (long)n, (int)k, keys, c->info_dev);
        CHK(clock.mark(ST_HASH));
        hipLaunchKernelGGL(prop_sort_kernel, dim3((unsigned)N), dim3(256), 0, st, keys, seg_d, long_off_d, long_buf, uk, uc, ulen);
        CHK(clock.mark(ST_SORT));
        hipLaunchKernelGGL(prop_gram_kernel, dim3((unsigned)tiles, (unsigned)tiles), dim3(256), 0, st, uk, uc, ulen, seg_d, N, h, H1,
                           sum ? 1 : 0, ksum, K_d);
        CHK(clock.mark(ST_GRAM));
        if (hipGetLastError() != hipSuccess) return PGP_ERR_HIP;
    }
    int info = 0;
    HIP_TRY(hipMemcpyAsync(&info, c->info_dev, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (info != 0) return PGP_ERR_PROP_NONFINITE;
    HIP_TRY(hipMemcpyAsync(K_out, K_d, kbytes, hipMemcpyDeviceToHost, st));
    if (lab_out) HIP_TRY(hipMemcpyAsync(lab_out, cur, nk, hipMemcpyDeviceToHost, st));
    CHK(clock.mark(ST_DOWNLOAD));
    HIP_TRY(hipStreamSynchronize(st));
    if (stage_ms_out) CHK(clock.read(stage_ms_out));
    return PGP_OK;
}

}  // extern "C"
