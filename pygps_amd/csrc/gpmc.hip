// GPMC.fitAndPredict on the device (reference: Core/gp.py:829-863, 905-928): the one-vs-one pairs of a multi-class problem share
// mean, kernel and hyper-parameters, so every pair's training covariance is a principal submatrix of ONE K_all = k(x_all, x_all)
// and every pair's cross-covariance a row subset of ONE Ks_all = k(x_all, xs).  Both are assembled once with the tile code of the
// fits and of predict; per pair a gather kernel copies the submatrix into the padded buffer the dense EP / Laplace drivers factor
// from (ep.hip / laplace.hip: GatherSrc), a second one the rows of Ks_all into the block of pgp_predict_dense's device core, and
// the votes (gp.py:854-862) are accumulated and normalised on the device.  Nothing of size n^2 or n ns crosses PCIe.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <vector>

#include "ctx.h"
#include "erf_lik.h"
#include "testhooks.h"

namespace {

// Two rows of one gathered column: dst[r], dst[r + 1] = src[idx[r]], src[idx[r + 1]] (rows >= n: zero).  r is even and dst a column
// of a buffer whose leading dimension is a multiple of 128, so the store is one 16-byte access; the load is one too where the two
// source rows are neighbours at a 16-byte boundary (inside an ascending run of consecutive rows).
__device__ __forceinline__ void gather_two(const double* __restrict__ src, const int* __restrict__ idx, long n, long r,
                                           double* __restrict__ dst) {
    double2 v = make_double2(0.0, 0.0);
    if (r + 1 < n) {
        const int i0 = idx[r], i1 = idx[r + 1];
        const double* p = src + i0;
        if (i1 == i0 + 1 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) v = *reinterpret_cast<const double2*>(p);
        else { v.x = p[0]; v.y = src[i1]; }
    } else if (r < n) v.x = src[idx[r]];
    *reinterpret_cast<double2*>(dst + r) = v;
}

// Kd[r, c] = K_all[idx[r], idx[c]] (K_all full symmetric: column idx[c], rows idx[.], contiguous along r), zeros on the padding;
// the workgroups of the first grid row also write the labels (+1 for the first n_pos rows, -1 for the others) and gather the mean
__global__ __launch_bounds__(256) void gather_sym_kernel(const double* __restrict__ K_all, long ld, const int* __restrict__ idx, long n,
                                                         long n_pos, const double* __restrict__ m_all, double* __restrict__ Kd, long np,
                                                         double* __restrict__ y, double* __restrict__ m) {
    const long r = 2 * ((long)blockIdx.x * 256 + threadIdx.x);
    if (r >= np) return;
    for (long c = blockIdx.y; c < np; c += gridDim.y) {
        if (c < n) gather_two(K_all + (long)idx[c] * ld, idx, n, r, Kd + c * np);
        else *reinterpret_cast<double2*>(Kd + c * np + r) = make_double2(0.0, 0.0);
    }
    if (blockIdx.y == 0 && y)
        for (long q = r; q < r + 2; ++q) {
            y[q] = q < n ? (q < n_pos ? 1.0 : -1.0) : 0.0;
            m[q] = q < n ? m_all[idx[q]] : 0.0;
        }
}

// Kp[r, j] = Ks_all[idx[r], j] for the nb live test points of the batch, zeros on the padding rows and columns (nrhs columns in all)
__global__ __launch_bounds__(256) void gather_rows_kernel(const double* __restrict__ Ks_all, long ld, const int* __restrict__ idx, long n,
                                                          double* __restrict__ Kp, long np, long nb, long nrhs) {
    const long r = 2 * ((long)blockIdx.x * 256 + threadIdx.x);
    if (r >= np) return;
    for (long j = blockIdx.y; j < nrhs; j += gridDim.y) {
        if (j < nb) gather_two(Ks_all + j * ld, idx, n, r, Kp + j * np);
        else *reinterpret_cast<double2*>(Kp + j * np + r) = make_double2(0.0, 0.0);
    }
}

// One pair's votes (gp.py:854-862): p = Phi(fmu / sqrt(1 + fs2)) as lik.Erf's prediction mode has it (exp(logphi), lik.py:251-269),
// ym = 2 p - 1, votes[:, i] += ym + 1, votes[:, j] += 2 - (ym + 1); fs2 = max(kss - s2, 0).  votes is class-major (one contiguous
// run of nt test points per class); launches on one stream are ordered, so a plain read-modify-write per test point suffices.
__global__ __launch_bounds__(256) void vote_accumulate_kernel(long nb, const double* __restrict__ fmu, const double* __restrict__ s2,
                                                              double kss, double* __restrict__ votes, long nt, int ci, int cj) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nb) return;
    const double fs2 = fmax(kss - s2[t], 0.0);
    const double p = exp(erf_logphi(fmu[t] / sqrt(1.0 + fs2)));
    const double a = (2.0 * p - 1.0) + 1.0;
    votes[(long)ci * nt + t] += a;
    votes[(long)cj * nt + t] += 2.0 - a;
}

// out (nt x n_class, row-major) = votes / row sums
__global__ __launch_bounds__(256) void vote_normalise_kernel(long nt, int n_class, const double* __restrict__ votes, double* __restrict__ out) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    double s = 0.0;
    for (int k = 0; k < n_class; ++k) s += votes[(long)k * nt + t];
    for (int k = 0; k < n_class; ++k) out[t * n_class + k] = votes[(long)k * nt + t] / s;
}

inline dim3 gather_grid(long np, long ncols) { return dim3((unsigned)((np / 2 + 255) / 256), (unsigned)std::min<long>(ncols, 65535)); }

int gather_rows_launch(const double* Ks_all, long ld, const int* idx, long n, double* Kp, long np, long nb, long nrhs, hipStream_t st) {
    hipLaunchKernelGGL(gather_rows_kernel, gather_grid(np, nrhs), dim3(256), 0, st, Ks_all, ld, idx, n, Kp, np, nb, nrhs);
    return hipGetLastError() == hipSuccess ? PGP_OK : PGP_ERR_HIP;
}

int vote_accumulate_launch(long nb, const double* fmu, const double* s2, double kss, double* votes, long nt, int ci, int cj, hipStream_t st) {
    hipLaunchKernelGGL(vote_accumulate_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, nb, fmu, s2, kss, votes, nt, ci, cj);
    return hipGetLastError() == hipSuccess ? PGP_OK : PGP_ERR_HIP;
}

struct FactorList {                      // the pairs' posterior handles: freed on every way out
    pgp_ctx* c; std::vector<pgp_factor*> f;
    explicit FactorList(pgp_ctx* c_) : c(c_) {}
    ~FactorList() { for (pgp_factor* h : f) if (h) pgp_factor_free(c, h); }
};
struct EventList {
    std::vector<hipEvent_t> e;
    ~EventList() { for (hipEvent_t x : e) (void)hipEventDestroy(x); }
};

}  // namespace

int gather_sym_launch(const GatherSrc& g, double* Kd, long np, hipStream_t st) {
    hipLaunchKernelGGL(gather_sym_kernel, gather_grid(np, np), dim3(256), 0, st, g.K_all, g.ld, g.idx, g.n, g.n_pos, g.m_all, Kd, np,
                       g.y, g.m);
    return hipGetLastError() == hipSuccess ? PGP_OK : PGP_ERR_HIP;
}

extern "C" {

int pgp_gpmc_fit_predict(pgp_ctx* c, int kind, const double* covhyp, int ncov, int para, int flags, int inference,
                         const int32_t* labels, int n_class, const double* m_all, const double* xs, int64_t ns, const double* ms,
                         double* votes_out, double* pair_nlZ_out, int32_t* pair_iters_out, int32_t* bad_pair_out) {
    if (!c) return -1;
    if (c->n <= 0) return -1;
    if (!covhyp) return -3;
    if (inference != 0 && inference != 1) return -7;
    if (!labels) return -8;
    if (n_class < 2) return -9;
    if (!xs) return -11;
    if (ns <= 0) return -12;
    if (!votes_out) return -14;
    const long n = c->n, d = c->d, np = c->np;
    // createBinaryClass (gp.py:905-928): per class its rows in data order; a pair is class i's rows, then class j's
    std::vector<std::vector<int>> members(n_class);
    for (long r = 0; r < n; ++r)
        if (labels[r] >= 0 && labels[r] < n_class) members[labels[r]].push_back((int)r);
    for (int k = 0; k < n_class; ++k)
        if (members[k].empty()) return -8;
    const int npairs = n_class * (n_class - 1) / 2;
    std::vector<int> idx_h, off(npairs + 1, 0), pi(npairs), pj(npairs);
    long npair_max = 0;
    {
        int p = 0;
        for (int i = 0; i < n_class; ++i)
            for (int j = i + 1; j < n_class; ++j, ++p) {
                pi[p] = i; pj[p] = j;
                idx_h.insert(idx_h.end(), members[i].begin(), members[i].end());
                idx_h.insert(idx_h.end(), members[j].begin(), members[j].end());
                off[p + 1] = (int)idx_h.size();
                npair_max = std::max<long>(npair_max, round_up(off[p + 1] - off[p], 128));
            }
    }
    hipStream_t st = c->st;
    CovSpec cp;
    double kss = 0.0;
    PoolScratch scr(c);
    FactorList fl(c);
    fl.f.assign(npairs, nullptr);
    double *K_all = nullptr, *m_d = nullptr, *yp = nullptr, *mp = nullptr, *votes = nullptr;
    int* idx_d = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto ms_since = [](std::chrono::steady_clock::time_point a) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
    };
    double t_assemble = 0.0, t_fit = 0.0, t_predict = 0.0, t_votes = 0.0;
    // ---- 1. K_all, once (the assembly of the EP / Laplace fits, over the resident x_all) ----------------------------------------
    {
        GateShared gate(c);
        HIP_TRY(hipSetDevice(c->device));
        { const int rc = make_spec(c, kind, covhyp, ncov, para, flags, -1, d, cp); if (rc != PGP_OK) return rc == -11 ? -10 : rc; }
        CHK(cov_point_value(c, cp, 2, &kss));
        CHK(scr.alloc(&K_all, (size_t)np * np * sizeof(double)));
        CHK(scr.alloc(&m_d, np * sizeof(double)));
        CHK(scr.alloc(&yp, npair_max * sizeof(double)));
        CHK(scr.alloc(&mp, npair_max * sizeof(double)));
        CHK(scr.alloc(&idx_d, idx_h.size() * sizeof(int)));
        CHK(scr.alloc(&votes, (size_t)n_class * ns * sizeof(double)));
        HIP_TRY(hipMemsetAsync(K_all, 0, (size_t)np * np * sizeof(double), st));
        HIP_TRY(hipMemsetAsync(m_d, 0, np * sizeof(double), st));
        HIP_TRY(hipMemsetAsync(votes, 0, (size_t)n_class * ns * sizeof(double), st));
        if (m_all) HIP_TRY(hipMemcpyAsync(m_d, m_all, n * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(idx_d, idx_h.data(), idx_h.size() * sizeof(int), hipMemcpyHostToDevice, st));
        CHK(upload_scaled(c, c->x_dev, n, d, cp.scale, c->XsT, np, c->dpad, c->scale_dev));
        if (gram_assembly_applies(c, cp)) {
            double* prep = nullptr;
            CHK(scr.alloc(&prep, (size_t)hadamard_prep_count(np) * sizeof(double)));
            CHK(hadamard_prepare_launch(c->XsT, np, n, np, c->dpad, cp, prep, st, /*force=*/true));
            CHK(cov_sym_gram_launch(c->XsT, np, n, c->dpad, cp, K_all, np, prep, st));
        } else
            CHK(cov_sym_launch(c->XsT, np, n, c->dpad, cp, K_all, st, np));
        HIP_TRY(hipStreamSynchronize(st));
        t_assemble = ms_since(t0);
    }
    // ---- 2. the pairs' fits, in the reference's order, each from a cold start (a fresh GPC per pair, gp.py:846) ---------------------
    // (the drivers hold the device gate themselves: shared for the fit, exclusive during each EP block sweep)
    const auto t1 = std::chrono::steady_clock::now();
    for (int p = 0; p < npairs; ++p) {
        GatherSrc g;
        g.n = off[p + 1] - off[p]; g.n_pos = (long)members[pi[p]].size();
        g.K_all = K_all; g.ld = np; g.idx = idx_d + off[p]; g.m_all = m_d; g.y = yp; g.m = mp;
        double nlZ = 0.0;
        int iters = 0;
        const int rc = inference == 0 ? ep_fit_gathered(c, g, &nlZ, &iters, &fl.f[p]) : laplace_fit_gathered(c, g, &nlZ, &iters, &fl.f[p]);
        if (rc != PGP_OK) {
            if (bad_pair_out) { bad_pair_out[0] = pi[p]; bad_pair_out[1] = pj[p]; }
            return rc;
        }
        if (pair_nlZ_out) pair_nlZ_out[p] = nlZ;
        if (pair_iters_out) pair_iters_out[p] = iters;
    }
    t_fit = ms_since(t1);
    // ---- 3. Ks_all per batch of test points, once; per pair its rows, pgp_predict_dense's core and the votes -----------------------
    const auto t2 = std::chrono::steady_clock::now();
    {
        GateShared gate(c);
        const int dpad = c->dpad;
        const long NSB = predict_batch_points(c->predict_batch, ns, np);
        double *xd = nullptr, *XcT = nullptr, *Ks_all = nullptr, *Kp = nullptr, *msd = nullptr, *o1 = nullptr, *o2 = nullptr, *out_d = nullptr;
        CHK(scr.alloc(&xd, NSB * d * sizeof(double)));
        CHK(scr.alloc(&XcT, (size_t)dpad * NSB * sizeof(double)));
        CHK(scr.alloc(&Ks_all, (size_t)np * NSB * sizeof(double)));
        CHK(scr.alloc(&Kp, (size_t)npair_max * NSB * sizeof(double)));
        CHK(scr.alloc(&msd, NSB * sizeof(double)));
        CHK(scr.alloc(&o1, NSB * sizeof(double)));
        CHK(scr.alloc(&o2, NSB * sizeof(double)));
        CHK(scr.alloc(&out_d, (size_t)n_class * ns * sizeof(double)));
        CovSpec cq = cp;
        cq.cp.der = -1; cq.pg.der = -1;
        EventList ev;
        double ks_ms = 0.0;
        for (long a = 0; a < ns; a += NSB) {
            const long nb = std::min<long>(NSB, ns - a);
            const long nrhs = round_up(nb, 128);
            const auto tb = std::chrono::steady_clock::now();
            HIP_TRY(hipMemcpyAsync(xd, xs + a * d, nb * d * sizeof(double), hipMemcpyHostToDevice, st));
            if (ms) HIP_TRY(hipMemcpyAsync(msd, ms + a, nb * sizeof(double), hipMemcpyHostToDevice, st));
            else HIP_TRY(hipMemsetAsync(msd, 0, nb * sizeof(double), st));
            CHK(scale_transpose_launch(xd, nb, (int)d, c->scale_dev, XcT, NSB, dpad, st));
            // one column per test point, contiguous over the training index: rows = test points, columns = training points in the
            // tile kernel's view (as pgp_predict's blocked form)
            HIP_TRY(hipMemsetAsync(Ks_all, 0, (size_t)np * nrhs * sizeof(double), st));
            CHK(cov_rect_launch(XcT, NSB, nb, c->XsT, np, n, dpad, cq, Ks_all, np, st));
            HIP_TRY(hipStreamSynchronize(st));
            ks_ms += ms_since(tb);
            for (int p = 0; p < npairs; ++p) {
                pgp_factor* f = fl.f[p];
                CHK(gather_rows_launch(Ks_all, np, idx_d + off[p], f->n, Kp, f->np, nb, nrhs, st));
                CHK(predict_dense_block(c, f, Kp, nb, (int)nrhs, msd, o1, o2));
                hipEvent_t e0, e1;
                HIP_TRY(hipEventCreate(&e0)); ev.e.push_back(e0);
                HIP_TRY(hipEventCreate(&e1)); ev.e.push_back(e1);
                HIP_TRY(hipEventRecord(e0, st));
                CHK(vote_accumulate_launch(nb, o1, o2, kss, votes + a, (long)ns, pi[p], pj[p], st));
                HIP_TRY(hipEventRecord(e1, st));
            }
            HIP_TRY(hipStreamSynchronize(st));                       // (xd, msd and Ks_all are rewritten by the next batch)
        }
        hipLaunchKernelGGL(vote_normalise_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st, (long)ns, n_class, votes, out_d);
        if (hipGetLastError() != hipSuccess) return PGP_ERR_HIP;
        HIP_TRY(hipMemcpyAsync(votes_out, out_d, (size_t)n_class * ns * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t k = 0; k + 1 < ev.e.size(); k += 2) {
            float v = 0.f;
            if (hipEventElapsedTime(&v, ev.e[k], ev.e[k + 1]) == hipSuccess) t_votes += v;
        }
        t_assemble += ks_ms;
        t_predict = ms_since(t2) - ks_ms - t_votes;
        if (c->prof) prof_collect(c);
    }
    // pgp_last_timings after this call: assemble = K_all + Ks_all, solve = the pairs' fits, potrf = the pairs' predicts (gathers and
    // triangular solves), grad = the vote kernels (device time), total = host wall clock of the whole call
    for (double& v : c->last_ms) v = 0.0;
    c->last_ms[PGP_STAGE_ASSEMBLE] = t_assemble; c->last_ms[PGP_STAGE_SOLVE] = t_fit; c->last_ms[PGP_STAGE_POTRF] = t_predict;
    c->last_ms[PGP_STAGE_GRAD] = t_votes; c->last_ms[PGP_STAGE_TOTAL] = ms_since(t0);
    return PGP_OK;
}

// self-test hook: Kd (np x np, np = n_idx rounded up to 128) gathered from a host matrix K (n x n, column-major = row-major for a
// symmetric one) through gather_sym_kernel; y_out / m_out (np) the labels and the gathered mean (m_all may be NULL: zeros)
int pgp_test_gather_sym(pgp_ctx* c, const double* K, int64_t n, const int32_t* idx, int64_t n_idx, int64_t n_pos, const double* m_all,
                        double* Kd_out, double* y_out, double* m_out) {
    if (!c || !K || !idx || !Kd_out || n <= 0 || n_idx <= 0 || n_pos < 0 || n_pos > n_idx) return -1;
    for (int64_t r = 0; r < n_idx; ++r)
        if (idx[r] < 0 || idx[r] >= n) return -2;
    GateShared gate(c);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->st;
    const long ld = round_up(n, 2), np = round_up(n_idx, 128);
    PoolScratch scr(c);
    double *Ka = nullptr, *Kd = nullptr, *md = nullptr, *yd = nullptr, *mg = nullptr;
    int* id = nullptr;
    CHK(scr.alloc(&Ka, (size_t)ld * n * sizeof(double)));
    CHK(scr.alloc(&Kd, (size_t)np * np * sizeof(double)));
    CHK(scr.alloc(&md, n * sizeof(double)));
    CHK(scr.alloc(&yd, np * sizeof(double)));
    CHK(scr.alloc(&mg, np * sizeof(double)));
    CHK(scr.alloc(&id, n_idx * sizeof(int)));
    HIP_TRY(hipMemsetAsync(Ka, 0, (size_t)ld * n * sizeof(double), st));
    HIP_TRY(hipMemcpy2DAsync(Ka, ld * sizeof(double), K, n * sizeof(double), n * sizeof(double), n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(md, 0, n * sizeof(double), st));
    if (m_all) HIP_TRY(hipMemcpyAsync(md, m_all, n * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(id, idx, n_idx * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(Kd, 0xff, (size_t)np * np * sizeof(double), st));        // (the kernel writes every element, padding included)
    GatherSrc g;
    g.n = n_idx; g.n_pos = n_pos; g.K_all = Ka; g.ld = ld; g.idx = id; g.m_all = md; g.y = yd; g.m = mg;
    CHK(gather_sym_launch(g, Kd, np, st));
    HIP_TRY(hipMemcpyAsync(Kd_out, Kd, (size_t)np * np * sizeof(double), hipMemcpyDeviceToHost, st));
    if (y_out) HIP_TRY(hipMemcpyAsync(y_out, yd, np * sizeof(double), hipMemcpyDeviceToHost, st));
    if (m_out) HIP_TRY(hipMemcpyAsync(m_out, mg, np * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PGP_OK;
}

// self-test hook: the votes of ONE pair (ci, cj) from host fmu, fs2 (ns each) through vote_accumulate_kernel and
// vote_normalise_kernel: votes_out (ns x n_class, row-major) before the normalisation, norm_out (optional) after it
int pgp_test_vote(pgp_ctx* c, const double* fmu, const double* fs2, int64_t ns, int n_class, int ci, int cj, double* votes_out,
                  double* norm_out) {
    if (!c || !fmu || !fs2 || !votes_out || ns <= 0 || n_class < 2 || ci < 0 || cj < 0 || ci >= n_class || cj >= n_class || ci == cj) return -1;
    GateShared gate(c);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->st;
    PoolScratch scr(c);
    double *fd = nullptr, *sd = nullptr, *vd = nullptr, *od = nullptr;
    CHK(scr.alloc(&fd, ns * sizeof(double)));
    CHK(scr.alloc(&sd, ns * sizeof(double)));
    CHK(scr.alloc(&vd, (size_t)n_class * ns * sizeof(double)));
    CHK(scr.alloc(&od, (size_t)n_class * ns * sizeof(double)));
    std::vector<double> neg(ns), vh((size_t)n_class * ns);
    for (int64_t t = 0; t < ns; ++t) neg[t] = -fs2[t];                              // fs2 = max(kss - s2, 0) with kss = 0, s2 = -fs2
    HIP_TRY(hipMemcpyAsync(fd, fmu, ns * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(sd, neg.data(), ns * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(vd, 0, (size_t)n_class * ns * sizeof(double), st));
    CHK(vote_accumulate_launch((long)ns, fd, sd, 0.0, vd, (long)ns, ci, cj, st));
    hipLaunchKernelGGL(vote_normalise_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st, (long)ns, n_class, vd, od);
    if (hipGetLastError() != hipSuccess) return PGP_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(vh.data(), vd, vh.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    if (norm_out) HIP_TRY(hipMemcpyAsync(norm_out, od, vh.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int64_t t = 0; t < ns; ++t)
        for (int k = 0; k < n_class; ++k) votes_out[t * n_class + k] = vh[(size_t)k * ns + t];
    return PGP_OK;
}

}  // extern "C"
