// C ABI (include/pygps_amd.h) + host-side drivers: the exact fit around the Cholesky sweep (sweep.hip), GEMM launch
// bookkeeping and tile-order tables, recursive triangular inverse, W^T W, fused gradient reduce.  See DESIGN.md for the pipeline.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <mutex>
#include <vector>

#include "ctx.h"

// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void pgp_set_last_hip_error(hipError_t e, const char* what, const char* file, int line) {
    snprintf(g_err, sizeof(g_err), "HIP error %d (%s) in %s at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
    (void)hipGetLastError();      // clear the runtime's sticky "last error": the launch wrappers test hipGetLastError()
}

static void ctx_register(pgp_ctx* c);
static void ctx_unregister(pgp_ctx* c);

void prof_collect(pgp_ctx* c) {
    if (c->recs.empty()) return;
    (void)hipStreamSynchronize(c->st);
    for (auto& r : c->recs) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, r.e0, r.e1);
        c->pc_ms[r.cls] += ms; c->pc_flops[r.cls] += r.flops; c->pc_bytes[r.cls] += r.bytes; c->pc_launch[r.cls]++;
        if (r.shadow >= 0) { c->pc_ms[r.shadow] += ms; c->pc_flops[r.shadow] += r.flops; c->pc_launch[r.shadow]++; }
        if (getenv("PGP_PROF_DUMP"))
            fprintf(stderr, "prof %-34s %8.4f ms %10.3f GF %7.2f TF\n", kProfNames[r.cls], ms, r.flops * 1e-9,
                    ms > 0 ? r.flops / (ms * 1e-3) * 1e-12 : 0.0);
        c->ev_pool.push_back(r.e0); c->ev_pool.push_back(r.e1);
    }
    c->recs.clear();
}

// ------------------------------------------------------------------------------------------------
DeviceGate& device_gate(int device) {
    static DeviceGate gates[64];
    return gates[(unsigned)device % 64u];
}
int& device_gate_depth(int device) {
    static thread_local int depth[64] = {0};
    return depth[(unsigned)device % 64u];
}

extern "C" {

const char* pgp_version(void) { return "pygps_amd 0.1 (gfx950)"; }
int pgp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

const char* pgp_strerror(int status) {
    if (status == 0) return "ok";
    if (status > 0) return "kernel matrix not positive definite";
    if (status <= PGP_ERR_HIP) return g_err[0] ? g_err : "HIP runtime failure";
    if (status == PGP_ERR_XU_UNSUPPORTED) return "the gradient w.r.t. the inducing inputs is not built for this covariance function";
    return "bad argument";
}

__global__ void pgp_noop_kernel() {}
static int alloc_result_buffer(pgp_ctx* c, long np);

// one yield table per device (4096 words, zeroed once): every context on the device polls / marks the same words
static unsigned* yield_table(int device) {
    static std::mutex mu;
    static unsigned* tab[64] = {nullptr};
    std::lock_guard<std::mutex> lk(mu);
    if (device < 0 || device >= 64) return nullptr;
    if (!tab[device]) {
        if (hipMalloc((void**)&tab[device], 4096 * sizeof(unsigned)) != hipSuccess) { (void)hipGetLastError(); tab[device] = nullptr; return nullptr; }
        (void)hipMemset(tab[device], 0, 4096 * sizeof(unsigned));
    }
    return tab[device];
}

int pgp_init(int device, pgp_ctx** ctx_out) { GateShared device_gate_hold(device);
    if (!ctx_out) return -2;
    HIP_TRY(hipSetDevice(device));
    {
        // Prime the device's default (null-stream) hardware queue before creating our own streams.  Measured on
        // MI355X / ROCm 7.2: when the FIRST hardware queue a process creates carries one of the fit streams, two
        // concurrent fit contexts reach 81 fits/s; when that first queue belongs to the (idle) null stream they
        // reach 91 fits/s -- the placement a process also gets by accident when torch has touched the GPU first.
        static std::mutex mu;
        static bool primed[64] = {false};
        std::lock_guard<std::mutex> lk(mu);
        if (device >= 0 && device < 64 && !primed[device]) {
            hipLaunchKernelGGL(pgp_noop_kernel, dim3(1), dim3(64), 0, 0);
            HIP_TRY(hipDeviceSynchronize());
            primed[device] = true;
        }
    }
    pgp_ctx* c = new pgp_ctx();
    c->device = device;
    // process-wide defaults of two options that model code has no handle on (the contexts of fit streams are made inside the
    // searches): PYGPS_AMD_PREDICT_INVERSE = 0 / 1 / 2, PYGPS_AMD_KEEP_INVERSE = 0 / 1 (pgp_set_option still wins per context)
    if (const char* e = getenv("PYGPS_AMD_PREDICT_INVERSE")) { const int v = atoi(e); if (v >= 0 && v <= 2) c->predict_inverse = v; }
    if (const char* e = getenv("PYGPS_AMD_KEEP_INVERSE")) c->keep_inverse = atoi(e) != 0;
    HIP_TRY(hipGetDeviceProperties(&c->prop, device));
    HIP_TRY(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
    {
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        HIP_TRY(hipStreamCreateWithPriority(&c->st2, hipStreamNonBlocking, hi));   // panel chain = critical path
        // EP's resident sweep kernel (st2) and the bulk launches (st) must run CONCURRENTLY: two streams of different priority
        // never share a hardware queue.  A device without a priority range gives no such guarantee: the reference's per-site
        // sweep then (slow, but it cannot wait for a kernel queued behind itself)
        if (lo == hi) c->ep_block = 0;
    }
    for (auto& e : c->ev) HIP_TRY(hipEventCreate(&e));
    memset(c->last_ms, 0, sizeof(c->last_ms));
    memset(c->pc_ms, 0, sizeof(c->pc_ms)); memset(c->pc_flops, 0, sizeof(c->pc_flops));
    memset(c->pc_bytes, 0, sizeof(c->pc_bytes)); memset(c->pc_launch, 0, sizeof(c->pc_launch));
    CHK(alloc_result_buffer(c, 0));
    c->yield_flags = yield_table(device);
    HIP_TRY(hipMalloc((void**)&c->Dk, (size_t)2048 * 1024 * sizeof(double)));       // 2w x w, w <= 1024
    HIP_TRY(hipMalloc((void**)&c->dpack, (size_t)8 * PACK_DOUBLES * sizeof(double)));
    HIP_TRY(hipMemset(c->Dk, 0, (size_t)2048 * 1024 * sizeof(double)));
    ctx_register(c);
    *ctx_out = c;
    return PGP_OK;
}

// the result buffer of a fit (layout: ctx.h RES_HEAD / RES_INFO)
static int alloc_result_buffer(pgp_ctx* c, long np) {
    const size_t bytes = (size_t)(RES_HEAD + np) * sizeof(double);
    if (c->res_dev) (void)hipFree(c->res_dev);
    if (c->res_host) (void)hipHostFree(c->res_host);
    c->res_dev = c->res_host = c->res_host_dev = nullptr; c->scal = c->alpha_dev = nullptr; c->info_dev = nullptr; c->res_cap = 0;
    HIP_TRY(hipMalloc((void**)&c->res_dev, bytes));
    HIP_TRY(hipMemset(c->res_dev, 0, bytes));
    HIP_TRY(hipHostMalloc((void**)&c->res_host, bytes, hipHostMallocMapped | hipHostMallocCoherent));
    c->res_host_dev = nullptr;
    if (hipHostGetDevicePointer((void**)&c->res_host_dev, c->res_host, 0) != hipSuccess) { (void)hipGetLastError(); c->res_host_dev = nullptr; }
    c->scal = c->res_dev; c->info_dev = (int*)(c->res_dev + RES_INFO); c->alpha_dev = c->res_dev + RES_HEAD;
    c->res_cap = bytes;
    return PGP_OK;
}

void pgp_destroy(pgp_ctx* c) { if (!c) return; GateShared device_gate_hold(c);
    if (!c) return;
    ctx_unregister(c);
    (void)hipSetDevice(c->device);
    // every stream of the context may still carry work of the last call (the panel stream runs the last E E^T product)
    (void)hipStreamSynchronize(c->st);
    if (c->st2) (void)hipStreamSynchronize(c->st2);
    for (auto& kv : c->pool) (void)hipFree(kv.second);
    for (auto& kv : c->spool) (void)hipFree(kv.second);
    for (auto& kv : c->orders) (void)hipFree(kv.second.first);
    void* bufs[] = {c->x_dev, c->y_dev, c->XsT, c->scale_dev, c->W, c->T, c->Binv, c->inv16, c->m_dev,
                    c->rvec, c->zvec, c->partial, c->Dk, c->dpack, c->Xs, c->res_dev, c->prep, c->pre2, c->pre1t, c->pre1s};
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (c->res_host) (void)hipHostFree(c->res_host);
    if (c->in_host) (void)hipHostFree(c->in_host);
    if (c->pred_host) (void)hipHostFree(c->pred_host);
    if (c->loo_host) (void)hipHostFree(c->loo_host);
    if (c->gemm_trace) (void)hipFree(c->gemm_trace);
    for (auto& e : c->ev) (void)hipEventDestroy(e);
    for (auto& e : c->ev_pool) (void)hipEventDestroy(e);
    for (auto& r : c->recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    for (auto& e : c->la_ev) (void)hipEventDestroy(e);
    for (auto& e : c->tm_ev) (void)hipEventDestroy(e);
    for (auto& e : c->fill_ev) (void)hipEventDestroy(e);
    for (auto& e : c->ep_ev) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(c->st);
    if (c->st2) (void)hipStreamDestroy(c->st2);
    delete c;
}

int pgp_device_info(pgp_ctx* c, int* n_cu, int* sclk_mhz, double* hbm_gib, char* name, int name_len) {
    if (!c) return -1;
    if (n_cu) *n_cu = c->prop.multiProcessorCount;
    if (sclk_mhz) *sclk_mhz = c->prop.clockRate / 1000;
    if (hbm_gib) *hbm_gib = (double)c->prop.totalGlobalMem / (1024.0 * 1024.0 * 1024.0);
    if (name && name_len > 0) { strncpy(name, c->prop.name, name_len - 1); name[name_len - 1] = 0; }
    return PGP_OK;
}

int pgp_set_option(pgp_ctx* c, const char* name, int value) {
    if (!c || !name) return -1;
    if (!strcmp(name, "nb_outer")) { if (value < 0) return -3; c->nb_outer = value; return PGP_OK; }
    if (!strcmp(name, "joint_refine")) { c->joint_refine = value != 0; return PGP_OK; }
    if (!strcmp(name, "small_tile_below")) { c->small_tile_below = value; return PGP_OK; }
    if (!strcmp(name, "trtri_small_tile_below")) { c->trtri_small_tile_below = value; return PGP_OK; }
    if (!strcmp(name, "xcd_order")) { c->xcd_order = value; return PGP_OK; }
    if (!strcmp(name, "gemm_dbg")) { if (value & ~(64 | 256 | 512)) return -2; c->gemm_dbg = value; return PGP_OK; }
    if (!strcmp(name, "tile_ring")) { if (value < 0 || value > 1) return -2; c->tile_ring = value; return PGP_OK; }
    if (!strcmp(name, "lookahead")) { c->lookahead = value; return PGP_OK; }
    if (!strcmp(name, "leaf_first")) { c->leaf_first = value; return PGP_OK; }
    if (!strcmp(name, "leaf_pivot")) { if (value < 0 || value > 2) return -2; c->leaf_pivot = value; return PGP_OK; }
    if (!strcmp(name, "sched")) { if (value < -1 || value > 2) return -2; c->sched = value < 0 ? PGP_SCHED_DEFAULT : value; c->sched_explicit = value >= 0; return PGP_OK; }
    if (!strcmp(name, "concurrent_streams")) { c->concurrent_streams = value != 0; return PGP_OK; }   // a HINT: an explicit "sched" wins
    if (!strcmp(name, "tud_tile")) { if (value != 64 && value != 128) return -2; c->tud_tile = value; return PGP_OK; }
    if (!strcmp(name, "tur_tile")) { if (value != 0 && value != 64 && value != 128 && value != 1264) return -2; c->tur_tile = value; return PGP_OK; }
    if (!strcmp(name, "s_pan")) { if (value < -1 || value > 2) return -2; c->s_pan = value; return PGP_OK; }
    if (!strcmp(name, "s_pan_direct")) { c->s_pan_direct = value != 0; return PGP_OK; }
    if (!strcmp(name, "s_pan_out")) { c->s_pan_out = value != 0; return PGP_OK; }
    if (!strcmp(name, "skip_zeros")) { c->skip_zeros = value != 0; return PGP_OK; }
    if (!strcmp(name, "tud_mark")) { c->tud_mark = value != 0; return PGP_OK; }
    if (!strcmp(name, "sched2_wide")) { c->sched2_wide = value != 0; return PGP_OK; }
    if (!strcmp(name, "gram_assembly")) { if (value < 0 || value > 2) return -2; c->gram_assembly = value; return PGP_OK; }
    if (!strcmp(name, "yield")) { c->yield = value; return PGP_OK; }
    if (!strcmp(name, "ep_fused")) { c->ep_fused = value; return PGP_OK; }
    if (!strcmp(name, "ep_tol_exp")) { if (value < 1 || value > 16) return -3; c->ep_tol_exp = value; return PGP_OK; }
    if (!strcmp(name, "ep_max_sweep")) { if (value < 2 || value > 1000) return -3; c->ep_max_sweep = value; return PGP_OK; }
    if (!strcmp(name, "laplace_tol_exp")) { if (value < 1 || value > 16) return -3; c->laplace_tol_exp = value; return PGP_OK; }
    if (!strcmp(name, "ep_r_direct")) { c->ep_r_direct = value; return PGP_OK; }
    if (!strcmp(name, "ep_alpha_direct")) { c->ep_alpha_direct = value; return PGP_OK; }
    if (!strcmp(name, "ep_sym")) { c->ep_sym = value; return PGP_OK; }
    if (!strcmp(name, "ep_wait_kernel")) { c->ep_wait_kernel = value; return PGP_OK; }
    if (!strcmp(name, "ep_sigma_under")) { c->ep_sigma_under = value; return PGP_OK; }
    if (!strcmp(name, "ep_recompute")) { c->ep_recompute = value; return PGP_OK; }
    if (!strcmp(name, "ep_final_rebuild")) { c->ep_final_rebuild = value; return PGP_OK; }
    if (!strcmp(name, "ep_block")) { c->ep_block = value; return PGP_OK; }
    if (!strcmp(name, "xcd_max_k")) { c->xcd_max_k = value; return PGP_OK; }
    if (!strcmp(name, "xcd_min_tiles")) { c->xcd_min_tiles = value; return PGP_OK; }
    if (!strcmp(name, "xcd_super")) { c->xcd_super = value; return PGP_OK; }
    if (!strcmp(name, "solve_outer")) { if (value < 1) return -2; c->solve_outer = value; return PGP_OK; }
    if (!strcmp(name, "keep_inverse")) { c->keep_inverse = value != 0; return PGP_OK; }
    if (!strcmp(name, "predict_inverse")) { if (value < 0 || value > 2) return -2; c->predict_inverse = value; return PGP_OK; }
    if (!strcmp(name, "predict_batch")) { if (value < 128 || value % 128) return -2; c->predict_batch = value; return PGP_OK; }
    if (!strcmp(name, "s_tile")) { if (value != 0 && value != 64 && value != 128) return -2; c->s_tile = value; return PGP_OK; }
    if (!strcmp(name, "eet_overlap")) { if (value != 0 && value != 2 && value != 3) return -2; c->eet_overlap = value; return PGP_OK; }
    if (!strcmp(name, "eet_max_panels")) { c->eet_max_panels = value; return PGP_OK; }
    if (!strcmp(name, "eet_first")) { if (value < -1) return -2; c->eet_first = value; return PGP_OK; }
    if (!strcmp(name, "eet_tile")) { if (value != 64 && value != 128) return -2; c->eet_tile = value; return PGP_OK; }
    if (!strcmp(name, "fused_inverse")) { c->fused_inverse = value; return PGP_OK; }
    if (!strcmp(name, "trsm_lean")) { if (value < 0 || value > 2) return -2; c->trsm_lean = value; return PGP_OK; }
    if (!strcmp(name, "ep_merge12")) { c->ep_merge12 = value != 0; return PGP_OK; }
    if (!strcmp(name, "publish")) { c->publish = value != 0; return PGP_OK; }
    if (!strcmp(name, "fused_value_max_np")) { c->fused_value_max_np = value; return PGP_OK; }
    if (!strcmp(name, "asm_grid")) { c->asm_grid = value; return PGP_OK; }
    if (!strcmp(name, "gram_fast")) { if (value < 0 || value > 2) return -2; c->gram_fast = value; return PGP_OK; }
    if (!strcmp(name, "gram_grid")) { if (value < 0) return -2; c->gram_grid = value; return PGP_OK; }
    if (!strcmp(name, "asm_nt")) { c->asm_nt = value; return PGP_OK; }
    if (!strcmp(name, "pair_launch")) { c->pair_launch = value != 0; return PGP_OK; }
    if (!strcmp(name, "gemm_trace")) {               // diagnostic: see ctx.h
        GateShared device_gate_hold(c);
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipDeviceSynchronize());
        if (c->gemm_trace) { (void)hipFree(c->gemm_trace); c->gemm_trace = nullptr; }
        c->gemm_trace_cap = 0; c->gemm_trace_pos = 0;
        if (value > 0) {
            const long cap = (long)value * 1024;
            HIP_TRY(hipMalloc((void**)&c->gemm_trace, (size_t)cap * 64));
            HIP_TRY(hipMemset(c->gemm_trace, 0, (size_t)cap * 64));
            c->gemm_trace_cap = cap;
        }
        return PGP_OK;
    }
    if (!strcmp(name, "ard_grad_form")) { if (value < 0 || value > 2) return -3; c->ard_grad_form = value; return PGP_OK; }
    return -2;
}

int pgp_last_timings(pgp_ctx* c, double* ms_out) {
    if (!c || !ms_out) return -1;
    memcpy(ms_out, c->last_ms, sizeof(c->last_ms));
    return PGP_OK;
}
int pgp_set_profiling(pgp_ctx* c, int on) { if (!c) return -1; c->prof = on != 0; return PGP_OK; }
int pgp_profile_classes(void) { return PC_COUNT; }
const char* pgp_profile_class_name(int cls) { return (cls >= 0 && cls < PC_COUNT) ? kProfNames[cls] : "?"; }
int pgp_profile_read(pgp_ctx* c, int cls, int64_t* launches, double* ms, double* flops, double* bytes) {
    if (!c || cls < 0 || cls >= PC_COUNT) return -1;
    prof_collect(c);
    if (launches) *launches = c->pc_launch[cls];
    if (ms) *ms = c->pc_ms[cls];
    if (flops) *flops = c->pc_flops[cls];
    if (bytes) *bytes = c->pc_bytes[cls];
    return PGP_OK;
}
int pgp_profile_reset(pgp_ctx* c) {
    if (!c) return -1;
    prof_collect(c);
    memset(c->pc_ms, 0, sizeof(c->pc_ms)); memset(c->pc_flops, 0, sizeof(c->pc_flops));
    memset(c->pc_bytes, 0, sizeof(c->pc_bytes)); memset(c->pc_launch, 0, sizeof(c->pc_launch));
    return PGP_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// host-side helpers
// ------------------------------------------------------------------------------------------------

static int matern_d(int para) { return (para == 1 || para == 3 || para == 5 || para == 7) ? para : 3; }

// number of hyperparameters of a primitive kernel (-1: unknown kind)
static int leaf_nhyp(int kind, long d) {
    switch (kind) {
        case PGP_COV_RBF: case PGP_COV_MATERN: case PGP_COV_PIECEPOLY: case PGP_COV_GABOR: return 2;
        case PGP_COV_RBFARD: return (int)d + 1;
        case PGP_COV_RQARD: return (int)d + 2;
        case PGP_COV_RBFUNIT: case PGP_COV_NOISE: case PGP_COV_CONST: return 1;
        case PGP_COV_RQ: case PGP_COV_PERIODIC: return 3;
        case PGP_COV_PRE: return 0;
        case PGP_COV_LINEAR: return 1;
        case PGP_COV_POLY: return 2;
        case PGP_COV_LINARD: return (int)d;
        default: return -1;
    }
}

// One primitive functor.  iso = isotropic factor c with (scaled distance)^2 = c^2 |x-z|^2 of the reference:
// RBF x/ell (cov.py:804); Matern sqrt(d) x/ell (:1141); RBFunit :847, RQ :1318, PiecePoly :742, Gabor :420 x/ell;
// Periodic, Noise, Const take the raw distance.  ARD kinds (RBFard x*(1/ell_k) :893-899, RQard :1378) have no iso.
static int make_leaf(int kind, const double* hyp, int nhyp, int para, int flags, long d, CovParams& cp, double& iso) {
    const int want = leaf_nhyp(kind, d);
    if (want < 0) return -2;
    if (nhyp != want) return -11;
    cp = CovParams{};
    cp.kind = kind; cp.der = -1; cp.md = matern_d(para); cp.D = (int)d; cp.train = 1;
    cp.ref_der = (flags & PGP_FLAG_MATERN_REFERENCE_DER) ? 1 : 0;
    cp.sf2 = 1.0; cp.alpha = 1.0; cp.ppv = 0; cp.ppj = 1.0; cp.ga = 0.0; cp.gb = 0.0;
    iso = 1.0;
    switch (kind) {
        case PGP_COV_RBF: iso = 1.0 / exp(hyp[0]); cp.sf2 = exp(2.0 * hyp[1]); break;
        case PGP_COV_RBFARD: cp.sf2 = exp(2.0 * hyp[d]); break;
        case PGP_COV_MATERN: iso = sqrt((double)cp.md) / exp(hyp[0]); cp.sf2 = exp(2.0 * hyp[1]); break;
        case PGP_COV_RBFUNIT: iso = 1.0 / exp(hyp[0]); break;
        case PGP_COV_RQ: iso = 1.0 / exp(hyp[0]); cp.sf2 = exp(2.0 * hyp[1]); cp.alpha = exp(hyp[2]); break;
        case PGP_COV_PIECEPOLY:
            if (para < 0 || para > 3) return -12;                                // Core/cov.py:737 assert
            iso = 1.0 / exp(hyp[0]); cp.sf2 = exp(2.0 * hyp[1]);
            cp.ppv = para; cp.ppj = floor(0.5 * (double)d) + para + 1.0;
            break;
        case PGP_COV_RQARD: cp.sf2 = exp(2.0 * hyp[d]); cp.alpha = exp(hyp[d + 1]); cp.gb = 1.0; break;
        case PGP_COV_GABOR: {
            const double ell = exp(hyp[0]), p = exp(2.0 * hyp[1]);               // cov.py:415-416
            iso = 1.0 / ell; cp.ga = 2.0 * M_PI * ell / p;
            break;
        }
        case PGP_COV_PERIODIC:
            if (d != 1) return -12;                                              // cov.py:1201-1204 asserts
            cp.gb = 1.0 / exp(hyp[0]); cp.ga = M_PI / exp(hyp[1]); cp.sf2 = exp(2.0 * hyp[2]);
            break;
        case PGP_COV_NOISE: cp.sf2 = exp(2.0 * hyp[0]); break;                   // cov.py:1268
        case PGP_COV_CONST: cp.sf2 = exp(hyp[0]); break;                         // cov.py:951 (not squared)
        // dot-product kernels (sqdist_tile.h dot_value): functions of sum_k x_k z_k, no iso
        case PGP_COV_LINEAR: cp.sf2 = exp(hyp[0]); break;                        // cov.py:997 (not squared)
        case PGP_COV_POLY:
            if (para < 1) return -12;                                            // cov.py:642 assert
            cp.alpha = exp(hyp[0]); cp.sf2 = exp(2.0 * hyp[1]); cp.md = para;    // c, sf2, the degree (cov.py:637-643)
            break;
        case PGP_COV_LINARD: break;                                              // 1 / ell_k folded into the coordinates (make_spec)
    }
    return PGP_OK;
}

// A program with a cov.Pre leaf reads the context's resident M2 (pgp_set_pre), which must belong to the resident x
static int bind_pre(pgp_ctx* c, CovSpec& cs) {
    if (cs.pg.pre_leaf < 0) return PGP_OK;
    if (!c || !c->pre2 || c->pre_n != c->n || c->n <= 0) return -14;
    cs.pre_train = c->pre2; cs.pre_ld = c->pre_ld; cs.pre_rows = c->pre_ld;
    return PGP_OK;
}

// Describe the covariance function of one call.  kind < PGP_COV_NKIND: a primitive; PGP_COV_COMPOSITE: the
// postfix program registered with pgp_set_composite, expanded here into a sum of products.
int make_spec(pgp_ctx* c, int kind, const double* hyp, int nhyp, int para, int flags, int der, long d, CovSpec& cs) {
    cs = CovSpec{};
    if (c) { cs.asm_grid = c->asm_grid; cs.asm_nt = c->asm_nt; cs.gram_fast = c->gram_fast; cs.gram_grid = c->gram_grid; }
    if (!hyp && nhyp > 0) return -10;
    if (kind == PGP_COV_SM) {
        // spectral mixture: a description of its own (sqdist_tile.h CovSM), unscaled coordinates.  Before the one-leaf-program
        // branch below, which would otherwise take every kind from PGP_COV_GABOR up
        const long Q = para;
        if (Q < 1) return -12;
        if (d > SM_MAXD || Q * (1 + 2 * d) > SM_MAXHYP) return -13;
        if ((long)nhyp != Q * (1 + 2 * d)) return -11;
        if (der >= nhyp) return -4;
        CovSM& P = cs.smp;
        P = CovSM{};
        P.Q = (int)Q; P.D = (int)d; P.dt = -1; P.dj = -1; P.dq = 0;
        const long double pi = 3.14159265358979323846264338327950288L;
        long double sw = 0.0L;
        for (long q = 0; q < Q; ++q) { P.h[q] = (double)expl((long double)hyp[q]); sw += expl((long double)hyp[q]); }
        for (long i = 0; i < d * Q; ++i) {                                        // each rounded once
            P.h[Q + i] = (double)(2.0L * pi * expl((long double)hyp[Q + i]));
            P.h[Q + d * Q + i] = (double)(2.0L * pi * pi * expl(2.0L * (long double)hyp[Q + d * Q + i]));
        }
        cs.sm = true; cs.scale.assign(d, 1.0); cs.ncov = nhyp; cs.nder = nhyp;
        cs.cp = CovParams{};
        cs.cp.kind = kind; cs.cp.der = der; cs.cp.D = (int)d; cs.cp.train = 1; cs.cp.sf2 = (double)sw;   // k(x,x) = sum_q w_q
        return PGP_OK;
    }
    if (kind >= PGP_COV_GABOR && kind < PGP_COV_NKIND) {
        // trigonometric / index-dependent primitives run as one-leaf programs (see sqdist_tile.h cov_value<EXT>)
        CovProgram& P = cs.pg;
        P = CovProgram{};
        double iso;
        CHK(make_leaf(kind, hyp, nhyp, para, flags, d, P.leaf[0], iso));
        // Poly accepts der == 2 ("derivative w.r.t. the degree" = zeros, cov.py:675-676)
        const int nder = kind == PGP_COV_POLY ? 3 : nhyp;
        if (der >= nder) return -4;
        if (kind == PGP_COV_LINARD && nhyp > 255) return -13;
        P.nleaf = 1; P.nterm = 1; P.nscale = 0; P.is2[0] = iso * iso; P.hyp0[0] = 0; P.nh[0] = nhyp; P.ard_leaf = -1; P.ard_leaf2 = -1;
        P.pre_leaf = kind == PGP_COV_PRE ? 0 : -1;
        P.dot_mask = (kind == PGP_COV_LINEAR || kind == PGP_COV_POLY || kind == PGP_COV_LINARD) ? 1u : 0u;
        P.coef[0] = 1.0; P.tl[0] = 1u; P.ts[0] = 0u;
        P.der = der; P.der_leaf = der >= 0 ? 0 : -1; P.der_j = der; P.der_scale = -1;
        cs.prog = true; cs.scale.assign(d, 1.0); cs.ncov = nhyp; cs.nder = nder;
        if (kind == PGP_COV_LINARD)                                              // x_k / ell_k, as plain RBFard folds its scales
            for (long k = 0; k < d; ++k) cs.scale[k] = 1.0 / exp(hyp[k]);
        return bind_pre(c, cs);
    }
    if (kind != PGP_COV_COMPOSITE) {
        double iso;
        CHK(make_leaf(kind, hyp, nhyp, para, flags, d, cs.cp, iso));
        cs.scale.assign(d, iso);
        if (kind == PGP_COV_RBFARD || kind == PGP_COV_RQARD) {
            for (long k = 0; k < d; ++k) cs.scale[k] = 1.0 / exp(hyp[k]);
            // the gradient pass weights its sums with K in the Gram form (hadamard_ard_kernel): relative error eps (|a|^2 + |b|^2) of
            // the scaled, centred points.  Beyond |a|^2 ~ 1e6 (2e-10 in K; dnlZ is held to 1e-7 and the Hadamard sum can cancel) the difference-form kernel runs
            // instead -- data spread over a thousand length scales; the statistics are those of the resident x (pgp_set_data)
            double bound = 0.0;
            if (c && (long)c->xdev2.size() == d)
                for (long k = 0; k < d; ++k) bound += cs.scale[k] * cs.scale[k] * c->xdev2[k];
            cs.ard_grad_diff = !(bound <= ARD_GRAM_GRAD_BOUND) || (c && c->ard_grad_form == 2);
            if (c && c->ard_grad_form == 1) cs.ard_grad_diff = false;
        }
        cs.ncov = nhyp;
        // Matern and PiecePoly accept der == 2 ("derivative w.r.t. the order" = zeros, cov.py:1178, 778)
        cs.nder = (kind == PGP_COV_MATERN || kind == PGP_COV_PIECEPOLY) ? 3 : nhyp;
        if (der >= cs.nder) return -4;
        cs.cp.der = der;
        cs.ell4 = (kind == PGP_COV_RQARD && cs.cp.ref_der && der >= 0 && der < d) ? exp(4.0 * hyp[der]) : 1.0;
        return PGP_OK;
    }
    const std::vector<int>& tok = c->composite;
    if (tok.empty()) return -2;
    struct Term { unsigned leaves, scales; };
    std::vector<std::vector<Term>> stack;
    CovProgram& P = cs.pg;
    P = CovProgram{};
    P.der = der; P.der_leaf = P.der_j = P.der_scale = -1;
    P.ard_leaf = -1; P.ard_leaf2 = -1; P.pre_leaf = -1;
    int used = 0;
    for (size_t i = 0; i < tok.size();) {
        const int op = tok[i];
        if (op == PGP_PROG_LEAF) {
            if (i + 5 > tok.size()) return -2;
            const int lk = tok[i + 1], lpara = tok[i + 2], lflags = tok[i + 3], h0 = tok[i + 4];
            i += 5;
            const bool ard = lk == PGP_COV_RBFARD || lk == PGP_COV_RQARD;
            if (ard && (P.ard_leaf2 >= 0 || d > CP_MAXARD)) return -13;           // at most two ARD leaves (own weighted distances), D <= 64
            if (lk == PGP_COV_LINARD) return -2;                                  // plain kind only: its scales live in the coordinates
            const bool dot = lk == PGP_COV_LINEAR || lk == PGP_COV_POLY;
            if (dot) P.dot_mask |= 1u << P.nleaf;
            const int nh = leaf_nhyp(lk, d);
            if (nh < 0) return -2;
            if (h0 < 0 || h0 + nh > nhyp) return -11;
            if (P.nleaf >= CP_MAXLEAF) return -13;
            if (lk == PGP_COV_PRE) {
                if (P.pre_leaf >= 0) return -13;                                   // one precomputed-matrix leaf per program
                P.pre_leaf = P.nleaf;
            }
            double iso;
            CHK(make_leaf(lk, hyp + h0, nh, lpara, lflags, d, P.leaf[P.nleaf], iso));
            P.is2[P.nleaf] = iso * iso; P.hyp0[P.nleaf] = h0; P.nh[P.nleaf] = nh;
            if (ard) {
                double* aw = P.ard_leaf < 0 ? P.ardw : P.ardw2;
                (P.ard_leaf < 0 ? P.ard_leaf : P.ard_leaf2) = P.nleaf;
                for (long k = 0; k < d; ++k) aw[k] = exp(-2.0 * hyp[h0 + k]);      // 1 / ell_k^2 (cov.py:893, 1378)
                if (lk == PGP_COV_RQARD && P.leaf[P.nleaf].ref_der && der >= h0 && der < h0 + d) cs.ell4 = exp(4.0 * hyp[der]);
            }
            if (der >= h0 && der < h0 + nh) { P.der_leaf = P.nleaf; P.der_j = der - h0; }
            stack.push_back({Term{1u << P.nleaf, 0u}});
            ++P.nleaf; used += nh;
        } else if (op == PGP_PROG_SUM || op == PGP_PROG_PRODUCT) {
            ++i;
            if (stack.size() < 2) return -2;
            std::vector<Term> b = stack.back(); stack.pop_back();
            std::vector<Term> a = stack.back(); stack.pop_back();
            std::vector<Term> r;
            if (op == PGP_PROG_SUM) { r = a; r.insert(r.end(), b.begin(), b.end()); }
            else for (const Term& x : a) for (const Term& y : b) r.push_back(Term{x.leaves | y.leaves, x.scales | y.scales});
            if (r.size() > (size_t)CP_MAXTERM) return -13;
            stack.push_back(r);
        } else if (op == PGP_PROG_SCALE) {
            if (i + 1 >= tok.size()) return -2;
            const int h = tok[i + 1];
            i += 2;
            if (stack.empty()) return -2;
            if (h < 0 || h >= nhyp) return -11;
            if (P.nscale >= CP_MAXSCALE) return -13;
            for (Term& t : stack.back()) t.scales |= 1u << P.nscale;
            P.shyp[P.nscale] = h;
            if (der == h) P.der_scale = P.nscale;
            ++P.nscale; ++used;
        } else {
            return -2;
        }
    }
    if (stack.size() != 1 || used != nhyp) return -11;
    // beside r^2 at most two more accumulators: one per ARD leaf, one for all dot-product leaves; and no Pre tile beside the dot product
    if (P.dot_mask && (P.ard_leaf2 >= 0 || P.pre_leaf >= 0)) return -13;
    P.nterm = (int)stack[0].size();
    for (int t = 0; t < P.nterm; ++t) {
        P.tl[t] = stack[0][t].leaves; P.ts[t] = stack[0][t].scales;
        double cf = 1.0;
        for (int k = 0; k < P.nscale; ++k)
            if ((P.ts[t] >> k) & 1u) cf *= exp(hyp[P.shyp[k]]);                   // cov.py:315 sf2 = exp(hyp[0])
        P.coef[t] = cf;
    }
    if (der >= nhyp) return -4;
    cs.prog = true;
    cs.scale.assign(d, 1.0);
    cs.ncov = nhyp; cs.nder = nhyp;
    cs.cp = CovParams{};
    if (P.ard_leaf >= 0 && c && (long)c->xdev2.size() == d) {          // as for the plain ARD kinds: per-coordinate sums in the difference form
        double b1 = 0.0, b2 = 0.0;                                   // when a leaf's weighted, centred points lie too far out
        for (long k = 0; k < d && k < CP_MAXARD; ++k) { b1 += P.ardw[k] * c->xdev2[k]; if (P.ard_leaf2 >= 0) b2 += P.ardw2[k] * c->xdev2[k]; }
        cs.ard_grad_diff = !(std::max(b1, b2) <= ARD_GRAM_GRAD_BOUND);
    }
    if (c && P.ard_leaf >= 0 && c->ard_grad_form) cs.ard_grad_diff = c->ard_grad_form == 2;
    return bind_pre(c, cs);
}

// value of the functor at zero distance: train = 1 -> K_ii (training diagonal), train = 2 -> k(z,z) of 'self_test'
int cov_point_value(pgp_ctx* c, const CovSpec& cs, int train, double* out) {
    // a cov.Pre leaf: K_ii and k(z,z) are vectors.  The fits read the training diagonal off the assembled K, pgp_predict takes
    // k(z,z) from the last row of the bound M1 (cov_self_vec_launch); the one number is not used
    if (cs.has_pre()) { *out = 0.0; return PGP_OK; }
    // dot-product leaves have no such scalar either, and nobody may ask for one: the exact, EP and Laplace fits skip the call,
    // pgp_cov and pgp_predict take the per-point vector (cov_self_dot_launch); the drivers built on one k(x, x) for all points
    // (FITC, the sharded fit, GPMC's shared engine) end here
    if (cs.has_dot()) return -13;
    if (!cs.prog && cs.cp.der < 0) {          // every functor primitive has k(x,x) = sf2 (RBFunit: sf2 = 1)
        (void)train;
        *out = cs.cp.sf2;
        return PGP_OK;
    }
    double* dv = c->scal + 6;
    CHK(cov_self_launch(cs, train, dv, c->st));
    HIP_TRY(hipMemcpyAsync(out, dv, sizeof(double), hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return PGP_OK;
}

// upload host x (n,d) scaled+transposed into a fresh device buffer XsT (dpad x ldp)
int upload_scaled(pgp_ctx* c, const double* x_dev, long n, long d, const std::vector<double>& sc, double* XsT,
                         long ldp, int dpad, double* scale_dev) {
    HIP_TRY(hipMemcpyAsync(scale_dev, sc.data(), d * sizeof(double), hipMemcpyHostToDevice, c->st));
    return scale_transpose_launch(x_dev, n, (int)d, scale_dev, XsT, ldp, dpad, c->st);
}

// Tile order for a GEMM launch.  Tiles are enumerated in 8x8 super-tiles (row-major over super-tiles, so
// for k-clipped triangular products the long-K rows come first = LPT), the list is cut into 8 contiguous
// chunks and chunk x is handed to the blocks with blockIdx % 8 == x -- the blocks the dispatcher places on
// XCD x.  The ~64 workgroups resident on one XCD then share 8 A and 8 B operand slabs through that XCD's
// private 4 MiB L2 instead of streaming 64 + 8 distinct slabs through all eight L2s.  Speed only: any
// placement computes the same result.
static int tile_order(pgp_ctx* c, int mt, int nt, int tri, int off_tiles, const int** out, int* n) {
    std::vector<int> key = {mt, nt, tri ? 1 : 0, off_tiles, c->xcd_super};
    auto it = c->orders.find(key);
    if (it != c->orders.end()) { *out = it->second.first; *n = it->second.second; return PGP_OK; }
    // super-tiles (S x S tiles: S A slabs + S B slabs serve S^2 tiles out of one XCD's L2), biggest first, each handed to
    // the XCD with the least work so far (LPT): the triangular edge makes partial super-tiles, and a plain round-robin
    // left one XCD up to a whole super-tile = one full round of its 64 slots behind (measured: -46 % FETCH but +13 % time)
    const int S = c->xcd_super > 0 ? c->xcd_super : 8;
    std::vector<std::vector<int>> sts;
    for (int SI = 0; SI * S < mt; ++SI)
        for (int SJ = 0; SJ * S < nt; ++SJ) {
            std::vector<int> st;
            for (int ti = SI * S; ti < std::min(mt, SI * S + S); ++ti)
                for (int tj = SJ * S; tj < std::min(nt, SJ * S + S); ++tj)
                    if (!tri || ti + off_tiles >= tj) { st.push_back(ti); st.push_back(tj); }
            if (!st.empty()) sts.push_back(std::move(st));
        }
    std::stable_sort(sts.begin(), sts.end(), [](const std::vector<int>& a, const std::vector<int>& b) { return a.size() > b.size(); });
    std::vector<std::vector<int>> seq(8);
    for (auto& st : sts) {
        int best = 0;
        for (int x = 1; x < 8; ++x) if (seq[x].size() < seq[best].size()) best = x;
        seq[best].insert(seq[best].end(), st.begin(), st.end());
    }
    // level the eight sequences to within one tile: single tiles move from the end of the longest to the shortest (a few
    // tiles per launch lose their super-tile's locality; an XCD that is a partial super-tile behind costs a whole tail)
    for (;;) {
        int lo = 0, hi = 0;
        for (int x = 1; x < 8; ++x) { if (seq[x].size() < seq[lo].size()) lo = x; if (seq[x].size() > seq[hi].size()) hi = x; }
        if (seq[hi].size() < seq[lo].size() + 4) break;
        const int tj = seq[hi].back(); seq[hi].pop_back();
        const int ti = seq[hi].back(); seq[hi].pop_back();
        seq[lo].push_back(ti); seq[lo].push_back(tj);
    }
    size_t maxlen = 0;
    for (auto& q : seq) maxlen = std::max(maxlen, q.size() / 2);
    const int nb = (int)maxlen * 8;
    std::vector<int> ord(2 * (size_t)nb, -1);
    for (int b = 0; b < nb; ++b) {
        const int x = b % 8, idx = b / 8;
        if ((size_t)idx < seq[x].size() / 2) { ord[2 * b] = seq[x][2 * idx]; ord[2 * b + 1] = seq[x][2 * idx + 1]; }
    }
    int* dev = nullptr;
    HIP_TRY(hipMalloc((void**)&dev, ord.size() * sizeof(int)));
    HIP_TRY(hipMemcpyAsync(dev, ord.data(), ord.size() * sizeof(int), hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));          // ord goes out of scope
    c->orders[key] = {dev, nb};
    *out = dev; *n = nb;
    return PGP_OK;
}

// Valid tiles of a lower-triangular (trapezoidal) tile grid, column-major like the plain 2-D grid but without
// the empty upper tiles (a 64x64-tile grid over N=8192 would otherwise dispatch 2016 workgroups that exit at once).
static int tri_tile_list(pgp_ctx* c, int mt, int nt, int off_tiles, const int** out, int* n) {
    std::vector<int> key = {mt, nt, 2, off_tiles};
    auto it = c->orders.find(key);
    if (it != c->orders.end()) { *out = it->second.first; *n = it->second.second; return PGP_OK; }
    std::vector<int> ord;
    for (int tj = 0; tj < nt; ++tj)
        for (int ti = 0; ti < mt; ++ti)
            if (ti + off_tiles >= tj) { ord.push_back(ti); ord.push_back(tj); }
    int* dev = nullptr;
    HIP_TRY(hipMalloc((void**)&dev, ord.size() * sizeof(int)));
    HIP_TRY(hipMemcpyAsync(dev, ord.data(), ord.size() * sizeof(int), hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    c->orders[key] = {dev, (int)ord.size() / 2};
    *out = dev; *n = (int)ord.size() / 2;
    return PGP_OK;
}

// Tiles of a SHRINKING batch of lower-trapezoidal products (GemmArgs::batch_dm: product z has mt0 - z dmt tile rows, nt tile
// columns, the top nt x nt tile block lower-triangular), product by product, column-major inside a product; ti carries z in
// its bits 16.. (GemmArgs::order_z).
int batch_tile_list(pgp_ctx* c, int mt0, int nt, int nb, int dmt, const int** out, int* n) {
    std::vector<int> key = {mt0, nt, nb, dmt, 7777};
    auto it = c->orders.find(key);
    if (it != c->orders.end()) { *out = it->second.first; *n = it->second.second; return PGP_OK; }
    std::vector<int> ord;
    for (int z = 0; z < nb; ++z)
        for (int tj = 0; tj < nt; ++tj)
            for (int ti = tj; ti < mt0 - z * dmt; ++ti) { ord.push_back(ti | (z << 16)); ord.push_back(tj); }
    if (ord.empty()) { ord.push_back(-1); ord.push_back(-1); }
    int* dev = nullptr;
    HIP_TRY(hipMalloc((void**)&dev, ord.size() * sizeof(int)));
    HIP_TRY(hipMemcpyAsync(dev, ord.data(), ord.size() * sizeof(int), hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    c->orders[key] = {dev, (int)ord.size() / 2};
    *out = dev; *n = (int)ord.size() / 2;
    return PGP_OK;
}

// RBF / RBFard values at d >= 32: the Gram form on the matrix cores (csrc/assemble.hip cov_gram_kernel) when a bound on the centred,
// scaled points' squared norms -- sum_k (scale_k max_p |x_pk - mean_k|)^2, from the statistics pgp_set_data took and the scales
// of this call -- keeps its extra rounding error below ~5e-14 relative in K; else the reference's difference form.
bool gram_assembly_applies(pgp_ctx* c, const CovSpec& cs) {
    if (!c->gram_assembly || !cov_gram_applies(cs, c->dpad) || (long)c->xdev2.size() != c->d || (long)cs.scale.size() < c->d) return false;
    if (c->gram_assembly == 2) return true;
    double bound = 0.0;
    for (long k = 0; k < c->d; ++k) bound += cs.scale[k] * cs.scale[k] * c->xdev2[k];
    return bound <= 64.0;
}

// everything gemm_prof decides about a launch before it goes out: tile order lists, the yield role, the trace slot
static int gemm_prepare(pgp_ctx* c, GemmArgs& g) {
    if (g.batch < 1) g.batch = 1;
    g.dbg |= c->gemm_dbg;
    // XCD-aware order only for bulk launches (>= xcd_min_tiles 128-tiles, unbatched): a latency-bound grid of a few
    // tiles would be serialised on one or two XCDs by it; and only up to K = xcd_max_k (measured: N = 8192, K = 512:
    // same speed, -40 % FETCH_SIZE per launch; N = 16384, K = 1024: 6 % slower)
    bool xcd = false;
    if (c->xcd_order && !g.order && g.tile != 64 && g.tile != 1264 && g.batch == 1 && g.K <= c->xcd_max_k) {
        const long mt = g.M / 128, nt = g.N / 128;
        const long tiles = g.tri == 2 ? mt * (mt + 1) / 2 : (g.tri == 1 ? mt * nt - nt * (nt - 1) / 2 : mt * nt);
        xcd = tiles >= c->xcd_min_tiles;
    }
    if (g.tri == 1 && !g.order && !xcd) {
        const int T = g.tile == 64 ? 64 : 128;
        CHK(tri_tile_list(c, g.M / T, g.N / T, g.tri_off / T, &g.order, &g.norder));
    }
    if (xcd) CHK(tile_order(c, g.M / 128, g.N / 128, g.tri, g.tri ? g.tri_off / 128 : 0, &g.order, &g.norder));
    if (c->yield && c->yield_flags) {
        g.yield_flags = c->yield_flags;
        // the chain's own small products mark their CUs (the caller presets role 2); every bulk (128-tile, LDS-DMA) launch polls
        if (g.yield_role != 2) g.yield_role = gemm_f64_uses_dma(g) ? 1 : 0;
    } else g.yield_role = 0;
    g.ring = c->tile_ring && gemm_f64_uses_dma(g) ? 1 : 0;      // the context's option decides, for every launch that goes through here
    if (c->gemm_trace && gemm_f64_uses_dma128(g) && g.batch == 1) {
        const long mt = g.M / 128, nt = g.N / 128;
        const long nb = g.order ? g.norder : (g.tri == 2 ? mt * (mt + 1) / 2 : mt * nt);
        if (c->gemm_trace_pos + nb <= c->gemm_trace_cap) { g.trace = c->gemm_trace + 8 * c->gemm_trace_pos; c->gemm_trace_pos += nb; }
    }
    return PGP_OK;
}

int gemm_prof(pgp_ctx* c, int cls, GemmArgs g, hipStream_t st) {
    if (!st) st = c->st;
    CHK(gemm_prepare(c, g));
    ProfScope ps(c, cls, g.flops, 0.0, st, gemm_f64_uses_dma128(g) ? PC_KERNEL_DMA128 : -1);
    return gemm_f64_launch(g, st);
}

// two independent bulk products as ONE launch when the kernel family allows it (gemm_f64_pair_ok), else one after the other
int gemm_prof_pair(pgp_ctx* c, int cls_a, GemmArgs a, int cls_b, GemmArgs b, hipStream_t st) {
    if (!st) st = c->st;
    CHK(gemm_prepare(c, a));
    CHK(gemm_prepare(c, b));
    if (c->pair_launch && gemm_f64_pair_ok(a, b)) {
        ProfScope ps(c, cls_a, a.flops + b.flops, 0.0, st, PC_KERNEL_DMA128);
        return gemm_f64_launch_pair(a, b, st);
    }
    { ProfScope ps(c, cls_a, a.flops, 0.0, st, gemm_f64_uses_dma128(a) ? PC_KERNEL_DMA128 : -1);
      CHK(gemm_f64_launch(a, st)); }
    ProfScope ps(c, cls_b, b.flops, 0.0, st, gemm_f64_uses_dma128(b) ? PC_KERNEL_DMA128 : -1);
    return gemm_f64_launch(b, st);
}

// W = L^-1 (column-major lower, np x np).  Level 0: batched inversion of the 128-blocks; then the
// recursion  W21 = -W22 (L21 W11)  bottom-up.  Levels whose nodes all share one shape run as ONE
// batched launch per product.
struct TriNode { int lo, mid, hi, depth; };
static void tri_nodes(int lo, int hi, int depth, std::vector<TriNode>& out) {
    if (hi - lo <= 1) return;
    int half = 1;
    while (half * 2 < hi - lo) half *= 2;          // largest power of two < size  (== size/2 for powers of two)
    const int mid = lo + half;
    out.push_back({lo, mid, hi, depth});
    tri_nodes(lo, mid, depth + 1, out);
    tri_nodes(mid, hi, depth + 1, out);
}

int trtri_lower(pgp_ctx* c, const double* L, long ldl, double* W, long ldw, double* T, long np) {
    const int nblk = (int)(np / 128);
    {
        ProfScope ps(c, PC_LEAFINV, (double)nblk * 128.0 * 128.0 * 128.0 / 3.0, 0.0);
        CHK(leaf_inv_launch(L, ldl, W, ldw, 128L * (1 + ldw), nblk, c->st));
    }
    std::vector<TriNode> nodes;
    tri_nodes(0, nblk, 0, nodes);
    int maxd = -1;
    for (auto& nd : nodes) maxd = std::max(maxd, nd.depth);
    for (int dep = maxd; dep >= 0; --dep) {
        std::vector<TriNode> lv;
        for (auto& nd : nodes) if (nd.depth == dep) lv.push_back(nd);
        if (lv.empty()) continue;
        std::sort(lv.begin(), lv.end(), [](const TriNode& a, const TriNode& b) { return a.lo < b.lo; });
        bool uniform = true;
        const int h1 = lv[0].mid - lv[0].lo, h2 = lv[0].hi - lv[0].mid;
        const int step = lv.size() > 1 ? lv[1].lo - lv[0].lo : 0;
        for (size_t i = 0; i < lv.size(); ++i)
            if (lv[i].mid - lv[i].lo != h1 || lv[i].hi - lv[i].mid != h2 || lv[i].lo != lv[0].lo + (int)i * step)
                uniform = false;
        const size_t ngroups = uniform ? 1 : lv.size();
        for (size_t gi = 0; gi < ngroups; ++gi) {
            const TriNode& nd = lv[gi];
            const int a1 = (nd.mid - nd.lo) * 128, a2 = (nd.hi - nd.mid) * 128;
            const long o1 = (long)nd.lo * 128, o2 = (long)nd.mid * 128;
            const int batch = uniform ? (int)lv.size() : 1;
            const long bstep = (long)step * 128;
            const long t128 = (long)(a2 / 128) * (a1 / 128) * batch;
            // T (a2 x a1) = L21 * W11            k >= j0 (W11 lower triangular)
            GemmArgs g{};
            g.A = L + o2 + o1 * ldl; g.lda = ldl; g.a_kc = 0;
            g.B = W + o1 + o1 * ldw; g.ldb = ldw; g.b_kc = 1;
            g.C = T; g.ldc = a2;
            g.M = a2; g.N = a1; g.K = a1; g.alpha = 1.0; g.beta = 0.0;
            g.kmode = KM_GE_J; g.koff = 0;
            g.batch = batch; g.sA = bstep * (1 + ldl); g.sB = bstep * (1 + ldw); g.sC = (long)a1 * a2;
            g.tile = t128 < c->trtri_small_tile_below ? 64 : 128;
            g.flops = (double)batch * (double)a2 * a1 * a1;
            CHK(gemm_prof(c, PC_GEMM_TRTRI, g));
            // W21 = -W22 * T                     k < i0 + TM (W22 lower triangular)
            GemmArgs h{};
            h.A = W + o2 + o2 * ldw; h.lda = ldw; h.a_kc = 0;
            h.B = T; h.ldb = a2; h.b_kc = 1;
            h.C = W + o2 + o1 * ldw; h.ldc = ldw;
            h.M = a2; h.N = a1; h.K = a2; h.alpha = -1.0; h.beta = 0.0;
            h.kmode = KM_LT_I; h.koff = 0;
            h.batch = batch; h.sA = bstep * (1 + ldw); h.sB = (long)a1 * a2; h.sC = bstep * (1 + ldw);
            h.tile = g.tile;
            h.flops = (double)batch * (double)a2 * a2 * a1;
            CHK(gemm_prof(c, PC_GEMM_TRTRI, h));
        }
    }
    return PGP_OK;
}

// Binv (lower) = W^T W
int lauum_lower(pgp_ctx* c, const double* W, long ldw, double* Binv, long ldb, long np) {
    GemmArgs g{};
    g.A = W; g.lda = ldw; g.a_kc = 1;
    g.B = W; g.ldb = ldw; g.b_kc = 1;
    g.C = Binv; g.ldc = ldb;
    g.M = (int)np; g.N = (int)np; g.K = (int)np; g.alpha = 1.0; g.beta = 0.0;
    g.tri = 2; g.mask_diag = 1; g.kmode = KM_GE_I; g.koff = 0;
    const long t128 = (np / 128) * (np / 128 + 1) / 2;
    g.tile = t128 < c->small_tile_below ? 64 : 128;
    g.flops = (double)np * np * np / 3.0;
    return gemm_prof(c, PC_GEMM_LAUUM, g);
}

// B^-1 (lower) = E E^T with E = W^T upper triangular (column-major, lde): NT product, k >= i0
int eet_lower(pgp_ctx* c, const double* E, long lde, double* Binv, long ldb, long np) {
    GemmArgs g{};
    g.A = E; g.lda = lde; g.a_kc = 0;
    g.B = E; g.ldb = lde; g.b_kc = 0;
    g.C = Binv; g.ldc = ldb;
    g.M = (int)np; g.N = (int)np; g.K = (int)np; g.alpha = 1.0; g.beta = 0.0;
    g.tri = 2; g.mask_diag = 1; g.kmode = KM_GE_I; g.koff = 0;
    const long t128 = (np / 128) * (np / 128 + 1) / 2;
    g.tile = t128 < c->small_tile_below ? 64 : 128;
    g.flops = (double)np * np * np / 3.0;
    return gemm_prof(c, PC_GEMM_LAUUM, g);
}

int ensure_workspace(pgp_ctx* c, long np) {
    if (c->ws_np == np) return PGP_OK;
    (void)hipStreamSynchronize(c->st);
    void* olds[] = {c->W, c->T, c->Binv, c->inv16, c->m_dev, c->rvec, c->zvec, c->prep};
    for (void* b : olds) if (b) (void)hipFree(b);
    c->W = c->T = c->Binv = c->inv16 = c->m_dev = c->rvec = c->zvec = c->prep = nullptr;
    if (c->in_host) { (void)hipHostFree(c->in_host); c->in_host = nullptr; c->in_cap = 0; }
    c->ws_np = 0;          // committed again only once EVERY allocation below has succeeded
    c->dense_ready = false;
    const size_t nn = (size_t)np * np * sizeof(double);
    HIP_TRY(hipMalloc((void**)&c->W, nn));
    HIP_TRY(hipMemsetAsync(c->W, 0, nn, c->st));
    HIP_TRY(hipMalloc((void**)&c->Binv, nn));
    HIP_TRY(hipMemsetAsync(c->Binv, 0, nn, c->st));
    HIP_TRY(hipMalloc((void**)&c->T, std::max<size_t>(nn / 4, 128 * 128 * sizeof(double))));
    HIP_TRY(hipMalloc((void**)&c->inv16, (size_t)(np / 128) * PACK_DOUBLES * sizeof(double)));
    CHK(alloc_result_buffer(c, np));                          // scalars | alpha: one device buffer, one pinned host image
    HIP_TRY(hipMalloc((void**)&c->m_dev, np * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&c->rvec, np * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&c->zvec, np * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&c->prep, (size_t)hadamard_prep_count(np) * sizeof(double)));
    HIP_TRY(hipMemsetAsync(c->rvec, 0, np * sizeof(double), c->st));
    c->in_cap = (size_t)(np + 1024) * sizeof(double);
    HIP_TRY(hipHostMalloc((void**)&c->in_host, c->in_cap, hipHostMallocDefault));
    c->ws_np = np;
    return PGP_OK;
}

int alloc_factor_buffer(pgp_ctx* c, long np, long ldf, double** F) {
    const size_t bytes = (size_t)ldf * np * sizeof(double);
    bool fresh = false;
    CHK(pool_alloc(c, bytes, (void**)F, &fresh));
    if (fresh) HIP_TRY(hipMemsetAsync(*F, 0, bytes, c->st));     // strict-upper tiles and augmented rows stay 0 forever
    return PGP_OK;
}

// ---- registry of live contexts (per-device idle caps, cross-context eviction on out-of-memory) ------------------
static std::mutex g_ctx_mu;
static std::vector<pgp_ctx*> g_ctxs;
int pgp_ctx_count_on_device(int device) {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    int n = 0;
    for (pgp_ctx* c : g_ctxs) n += c->device == device;
    return n;
}
void pgp_drop_idle_pools(int device) { GateShared device_gate_hold(device);
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    for (pgp_ctx* c : g_ctxs) {
        if (c->device != device) continue;
        std::lock_guard<std::mutex> lp(c->pool_mu);
        for (auto& kv : c->pool) (void)hipFree(kv.second);
        for (auto& kv : c->spool) (void)hipFree(kv.second);
        c->pool.clear(); c->pool_bytes = 0;
        c->spool.clear(); c->spool_bytes = 0;
    }
}
static void ctx_register(pgp_ctx* c) { std::lock_guard<std::mutex> lk(g_ctx_mu); g_ctxs.push_back(c); }
static void ctx_unregister(pgp_ctx* c) {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    g_ctxs.erase(std::remove(g_ctxs.begin(), g_ctxs.end(), c), g_ctxs.end());
}

extern "C" {

int pgp_set_composite(pgp_ctx* c, const int32_t* prog, int nprog) { if (!c) return -1; GateShared device_gate_hold(c);
    if (!c) return -1;
    if (nprog < 0 || (nprog > 0 && !prog)) return -2;
    c->composite.assign(prog, prog + nprog);
    return PGP_OK;
}

// cov.Pre (Core/cov.py:1429-1455): the precomputed matrices of the leaf, resident until replaced.  M2 (n, n) row-major goes into a
// zero-padded np x np buffer (np = n rounded up to 128: every 64-tile the kernels visit is in bounds and 16-byte aligned);
// M1 (n + 1, ns) is stored transposed, test-major -- row j = the n cross-covariances of test point j, the layout pgp_predict's
// cross block reads along -- with its last row (the test self-covariances) as a vector of its own.  Either may be NULL: it is kept.
int pgp_set_pre(pgp_ctx* c, const double* M2, int64_t n, const double* M1, int64_t ns) { if (!c) return -1; GateShared device_gate_hold(c);
    if (!c) return -1;
    if (n <= 0) return -3;
    if (M1 && ns <= 0) return -5;
    HIP_TRY(hipSetDevice(c->device));
    (void)hipStreamSynchronize(c->st);
    const long np = round_up(n, 128);
    if (M2) {
        if (c->pre2) (void)hipFree(c->pre2);
        c->pre2 = nullptr; c->pre_n = 0;
        if (c->pre1t) (void)hipFree(c->pre1t);                    // an M1 of another training set no longer applies
        if (c->pre1s) (void)hipFree(c->pre1s);
        c->pre1t = c->pre1s = nullptr; c->pre_ns = 0;
        HIP_TRY(hipMalloc((void**)&c->pre2, (size_t)np * np * sizeof(double)));
        HIP_TRY(hipMemsetAsync(c->pre2, 0, (size_t)np * np * sizeof(double), c->st));
        HIP_TRY(hipMemcpy2DAsync(c->pre2, np * sizeof(double), M2, n * sizeof(double), n * sizeof(double), n, hipMemcpyHostToDevice, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
        c->pre_n = n; c->pre_ld = np;
    }
    if (M1) {
        if (!c->pre2 || c->pre_n != n) return -2;
        if (c->pre1t) (void)hipFree(c->pre1t);
        if (c->pre1s) (void)hipFree(c->pre1s);
        c->pre1t = c->pre1s = nullptr; c->pre_ns = 0;
        const long nsp = round_up(ns, 128);
        HIP_TRY(hipMalloc((void**)&c->pre1t, (size_t)nsp * np * sizeof(double)));
        HIP_TRY(hipMalloc((void**)&c->pre1s, (size_t)nsp * sizeof(double)));
        HIP_TRY(hipMemsetAsync(c->pre1t, 0, (size_t)nsp * np * sizeof(double), c->st));
        HIP_TRY(hipMemsetAsync(c->pre1s, 0, (size_t)nsp * sizeof(double), c->st));
        std::vector<double> blk;                                     // transposed on the host, 1024 test points at a time
        for (int64_t a = 0; a < ns; a += 1024) {
            const int64_t nb = std::min<int64_t>(1024, ns - a);
            blk.resize((size_t)nb * n);
            for (int64_t i = 0; i < n; ++i)
                for (int64_t j = 0; j < nb; ++j) blk[(size_t)j * n + i] = M1[(size_t)i * ns + a + j];
            HIP_TRY(hipMemcpy2DAsync(c->pre1t + a * np, np * sizeof(double), blk.data(), n * sizeof(double), n * sizeof(double), nb,
                                     hipMemcpyHostToDevice, c->st));
            HIP_TRY(hipStreamSynchronize(c->st));                    // blk is reused
        }
        HIP_TRY(hipMemcpyAsync(c->pre1s, M1 + (size_t)n * ns, ns * sizeof(double), hipMemcpyHostToDevice, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
        c->pre_ns = ns; c->pre_nsp = nsp;
    }
    return PGP_OK;
}

int pgp_set_data(pgp_ctx* c, const double* x, int64_t n, int64_t d, const double* y) { if (!c) return -1; GateShared device_gate_hold(c);
    if (!c) return -1;
    if (!x) return -2;
    if (n <= 0) return -3;
    if (d <= 0) return -4;
    HIP_TRY(hipSetDevice(c->device));
    (void)hipStreamSynchronize(c->st);
    void* olds[] = {c->x_dev, c->y_dev, c->XsT, c->scale_dev};
    for (void* b : olds) if (b) (void)hipFree(b);
    c->x_dev = c->y_dev = c->XsT = c->scale_dev = nullptr;
    c->n = 0;              // "no data" until every allocation and copy below has succeeded
    const long np = round_up(n, 128);
    const int dpad = (int)round_up(d, SKC);
    HIP_TRY(hipMalloc((void**)&c->x_dev, n * d * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&c->y_dev, np * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&c->XsT, (size_t)dpad * np * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&c->scale_dev, dpad * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(c->x_dev, x, n * d * sizeof(double), hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipMemsetAsync(c->y_dev, 0, np * sizeof(double), c->st));
    if (y) HIP_TRY(hipMemcpyAsync(c->y_dev, y, n * sizeof(double), hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    {   // per coordinate: the largest squared deviation from the mean (the bound behind the choice of the Gram-form assembly)
        std::vector<double> mean((size_t)d, 0.0);
        for (int64_t p = 0; p < n; ++p) for (int64_t k = 0; k < d; ++k) mean[k] += x[p * d + k];
        for (int64_t k = 0; k < d; ++k) mean[k] /= (double)n;
        c->xdev2.assign((size_t)d, 0.0);
        for (int64_t p = 0; p < n; ++p)
            for (int64_t k = 0; k < d; ++k) { const double v = x[p * d + k] - mean[k]; if (v * v > c->xdev2[k]) c->xdev2[k] = v * v; }
    }
    c->n = n; c->d = d; c->np = np; c->ldf = np + 128;
    // ^ factor rows | 128 augmented rhs rows.  (The np rows of the fused inverse live in pooled scratch, not in the
    //   factor buffer: a posterior handle keeps (np + 128) np doubles, not (2 np + 128) np.)
    c->dpad = dpad;
    return PGP_OK;
}

}  // extern "C"

// ---- the blocks every fit driver shares (ctx.h) -----------------------------------------------------------------------------
int ensure_partial(pgp_ctx* c, long need) {
    if (c->partial_cap >= need) return PGP_OK;
    if (c->partial) (void)hipFree(c->partial);
    c->partial = nullptr; c->partial_cap = 0;      // a failed realloc must not leave a dangling pointer behind
    HIP_TRY(hipMalloc((void**)&c->partial, need * sizeof(double)));
    c->partial_cap = need;
    return PGP_OK;
}

int assemble_train_k(pgp_ctx* c, const CovSpec& cp, const double* Kdense, const GatherSrc* gk, long n, long np, double* Kd, hipStream_t st) {
    if (gk) return gather_sym_launch(*gk, Kd, np, st);                                  // already on the device, gathered
    if (Kdense) {
        HIP_TRY(hipMemcpy2DAsync(Kd, np * sizeof(double), Kdense, n * sizeof(double), n * sizeof(double), n, hipMemcpyHostToDevice, st));
        return PGP_OK;
    }
    CHK(upload_scaled(c, c->x_dev, n, c->d, cp.scale, c->XsT, np, c->dpad, c->scale_dev));
    if (!gram_assembly_applies(c, cp)) return cov_sym_launch(c->XsT, np, n, c->dpad, cp, Kd, st, np);
    // RBF / RBFard at d >= 32 (cfg 5: d = 32): the Gram form on the matrix cores
    CHK(hadamard_prepare_launch(c->XsT, np, n, np, c->dpad, cp, c->prep, st, /*force=*/true));
    return cov_sym_gram_launch(c->XsT, np, n, c->dpad, cp, Kd, np, c->prep, st);
}

int finish_factor(pgp_ctx* c, long n, long np, long ldf, FactorGuard& fguard, const CovSpec* cs, double kss, double sn2,
                  const double* alpha, const double* sW, hipMemcpyKind from, pgp_factor** out) {
    hipStream_t st = c->st;
    FactorHandleGuard hg(c, new pgp_factor());
    pgp_factor* f = hg.f;
    f->n = n; f->np = np; f->ldf = ldf; f->F = fguard.release(); f->dpad = cs ? c->dpad : 0; f->d = cs ? (int)c->d : 0; f->kss = kss;
    if (cs) f->cs = *cs;
    f->sn2 = sn2; f->sw = 1.0 / sqrt(sn2); f->Wd = nullptr; f->XsT = nullptr;
    const bool host = from == hipMemcpyHostToDevice;             // a host alpha has n entries: the padding is zeroed here
    CHK(spool_take(c, np * sizeof(double), (void**)&f->alpha));
    if (host) HIP_TRY(hipMemsetAsync(f->alpha, 0, np * sizeof(double), st));
    HIP_TRY(hipMemcpyAsync(f->alpha, alpha, (host ? n : np) * sizeof(double), from, st));
    if (sW) {
        CHK(spool_take(c, np * sizeof(double), (void**)&f->sWv));
        HIP_TRY(hipMemcpyAsync(f->sWv, sW, np * sizeof(double), from, st));
    }
    if (cs) {
        CHK(spool_take(c, (size_t)c->dpad * np * sizeof(double), (void**)&f->XsT));
        HIP_TRY(hipMemcpyAsync(f->XsT, c->XsT, (size_t)c->dpad * np * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    *out = hg.release();
    return PGP_OK;
}

void loo_copy_out(pgp_ctx* c, LooOut* loo, long n, long np, int want) {
    const double* v = c->loo_host;
    if (loo->mu) memcpy(loo->mu, v + LOO_MU * np, n * sizeof(double));
    if (loo->s2) memcpy(loo->s2, v + LOO_S2 * np, n * sizeof(double));
    if (loo->lp) memcpy(loo->lp, v + LOO_LP * np, n * sizeof(double));
    if (loo->u && want >= 3) memcpy(loo->u, v + LOO_U * np, n * sizeof(double));
    loo->nlZ_loo = v[LOO_HOST_VECS * np];
}

// Exact.evaluate, and with `loo` its leave-one-out variant (loo.hip): the same stages up to B^-1 and alpha, the same posterior;
// the LOO tail then replaces B^-1 by S = sn2 Q_loo and hands the gradient pass a zero vector for alpha.  nlZ_out receives the
// marginal likelihood either way (loo->nlZ_loo the LOO objective); dnlZ_out the gradient of the one the call is about.
// A value-only LOO call (want < 3) reads diag(B^-1) off the fused inverse rows (row sums of squares of E) and runs nothing
// O(n^3) beyond the factorisation; want = 3 reads the SAME sums, so that both return the same bits.  Where the fused inverse is
// switched off or refused (fused_inverse 0, fused_value_max_np, no scratch), a value-only LOO call takes want = 3's route to
// B^-1 (triangular inverse + W'W) and reads its diagonal.
static int exact_fit_run(pgp_ctx* c, int kind, const double* covhyp, int ncov, int para, int flags, double log_sn,
                         const double* mvec, const double* dm, int nmean, int want, double* alpha_out, double* nlZ_out,
                         double* dnlZ_out, pgp_factor** factor_out, LooOut* loo) {
    if (!c) return -1;
    GateShared device_gate_hold(c);
    if (!c) return -1;
    if (c->n <= 0) return -1;
    if (!covhyp) return -3;
    if (want < 1 || want > 3) return -11;
    if (ncov < 0 || 8 + ncov + 1 > RES_INFO) return -4;
    HIP_TRY(hipSetDevice(c->device));
    c->dense_ready = false;                          // the workspace (B^-1, alpha) is about to be rewritten
    const long n = c->n, d = c->d, np = c->np;
    // value-only fits (want < 3) take the fused-inverse sweep too (round 5): alpha = E z / sn2 is one matvec, whereas the blocked
    // back-substitution without E is a chain of np / 128 dependent steps (3.3 ms at N = 8192: an nlZ-only fit cost as much as one
    // with all gradients).  They skip E E' and the gradient pass.
    // with all gradients).  They skip E E' and the gradient pass.  That is a win while the sweep is bound by its dependent chain
    // (measured at N <= 8192); the inverse rows double the sweep's flops and need np x np of scratch, so beyond
    // `fused_value_max_np` (default 12288, where the sweep turns compute-bound) -- or when that scratch cannot be had -- a
    // value-only fit takes the plain factorisation + blocked back-substitution again.
    bool fused = c->fused_inverse != 0;
    if (want < 3 && fused && c->fused_value_max_np >= 0 && np > c->fused_value_max_np) fused = false;
    const long ldf = c->ldf;                         // factor buffer = factor rows + rhs rows; the inverse rows are scratch
    CovSpec cp;
    { const int rc = make_spec(c, kind, covhyp, ncov, para, flags, -1, d, cp); if (rc != PGP_OK) return rc == -11 ? -10 : rc; }
    const std::vector<double>& sc = cp.scale;
    CHK(ensure_workspace(c, np));
    double kss = 0.0;
    if (factor_out && !cp.has_dot()) CHK(cov_point_value(c, cp, 2, &kss));      // (dot-product leaves: predict takes k(z,z) per point)
    const long need = std::max(hadamard_partial_count(np, ncov), 32L * np);       // also the partials of upper_matvec
    if (want >= 3 || fused || loo) CHK(ensure_partial(c, need));
    const double sn2 = exp(2.0 * log_sn);
    double* F = nullptr;
    CHK(alloc_factor_buffer(c, np, ldf, &F));
    FactorGuard fguard(c, F, (size_t)ldf * np * sizeof(double), /*scrub=*/true);   // back to the pool on every early return
    PoolScratch pscr(c);
    double* E = nullptr;                             // E(i,j) at E[i + j*lde]: ends up as W^T = L^-T (upper triangular)
    const long lde = np;
    if (fused) {
        const int erc = pscr.alloc(&E, (size_t)np * np * sizeof(double));
        if (erc != PGP_OK) {
            if (want >= 3) return erc;
            (void)hipGetLastError(); fused = false; E = nullptr;      // value-only: the plain sweep needs no inverse rows
        }
    }
    const int rwant = (loo && want >= 2 && !fused) ? 3 : want;    // the route to B^-1 and alpha (see above); == want for every plain fit
    hipStream_t st = c->st;
    HIP_TRY(hipMemsetAsync(c->info_dev, 0, sizeof(int), st));
    if (mvec) {                                      // through pinned memory: an async copy from pageable memory is staged
        memcpy(c->in_host, mvec, n * sizeof(double));             // and synchronised by the runtime
        HIP_TRY(hipMemcpyAsync(c->m_dev, c->in_host, n * sizeof(double), hipMemcpyHostToDevice, st));
    } else HIP_TRY(hipMemsetAsync(c->m_dev, 0, n * sizeof(double), st));

    // ---- S1': fused assembly of B = K/sn2 + I into the factor buffer --------------------------
    HIP_TRY(hipEventRecord(c->ev[0], st));
    CHK(upload_scaled(c, c->x_dev, n, d, sc, c->XsT, np, c->dpad, c->scale_dev));
    const bool gram = gram_assembly_applies(c, cp);
    if (gram) CHK(hadamard_prepare_launch(c->XsT, np, n, np, c->dpad, cp, c->prep, st, /*force=*/true));
    {
        ProfScope ps(c, PC_ASSEMBLE, 0.0, 8.0 * (double)np * (np + 1) / 2.0 + 8.0 * (double)n * d);
        if (gram) CHK(cov_factor_gram_launch(c->XsT, np, n, np, c->dpad, cp, 1.0 / sn2, F, ldf, c->prep, st));
        else CHK(cov_factor_launch(c->XsT, np, n, np, c->dpad, cp, 1.0 / sn2, F, ldf, st));
    }
    CHK(aug_rhs_launch(c->y_dev, c->m_dev, n, F, ldf, np, c->rvec, st));
    // ---- S2: Cholesky (forward substitution of the augmented row -- and L^-T -- ride along) ----------
    HIP_TRY(hipEventRecord(c->ev[1], st));
    SweepJob job{F, ldf, np, np + 128, fused, E, lde};
    if (fused && want >= 3) { job.eet_out = c->Binv; job.eet_ld = np; }
    const int prc = potrf_blocked(c, job);
    if (prc != PGP_OK) (void)hipDeviceSynchronize();                              // queued products still read the scratch E
    CHK(prc);
    HIP_TRY(hipEventRecord(c->ev[2], st));
    // scalars first: logdet, z'z  (one small workgroup; it runs beside the last E E^T product instead of behind alpha)
    CHK(logdet_ztz_launch(F, ldf, n, F + np, ldf, c->scal, st));
    // ---- S5a/S3: W = L^-1, alpha = W^T z / sn2 (or blocked back-substitution when W is not needed)
    CHK(gather_strided_launch(F + np, ldf, np, c->zvec, st));
    if (fused) {
        HIP_TRY(hipEventRecord(c->ev[3], st));
        { ProfScope ps(c, PC_SMALL, 0.0, 4.0 * (double)np * np);                      // alpha = W^T z / sn2 = E z / sn2
          CHK(upper_matvec_launch(E, lde, np, c->zvec, 1.0 / sn2, c->partial, c->alpha_dev, st)); }
    } else if (rwant >= 3) {
        CHK(trtri_lower(c, F, ldf, c->W, np, c->T, np));
        HIP_TRY(hipEventRecord(c->ev[3], st));
        { ProfScope ps(c, PC_SMALL, 0.0, 4.0 * (double)np * np);
          CHK(col_dot_launch(c->W, np, np, c->zvec, 1, 1.0 / sn2, c->alpha_dev, st)); }
    } else {
        { ProfScope ps(c, PC_LEAFINV, 0.0, 0.0);
          CHK(leaf_inv_launch(F, ldf, c->W, np, 128L * (1 + np), (int)(np / 128), st)); }
        HIP_TRY(hipEventRecord(c->ev[3], st));
        { ProfScope ps(c, PC_SMALL, 0.0, 4.0 * (double)np * np);
          CHK(trsv_bwd_launch(F, ldf, c->W, np, c->zvec, c->alpha_dev, (int)(np / 128), st)); }
    }
    HIP_TRY(hipEventRecord(c->ev[4], st));
    // ---- S5b: B^-1 = W^T W ; S6: gradient reduce ------------------------------------------------
    double* lbuf = nullptr;                          // LOO: [mu | s2 | lp | u | nlZ_loo ...] and the tail's device-only vectors
    if (rwant >= 3) {
        if (fused && job.join) HIP_TRY(hipStreamWaitEvent(st, job.join, 0));        // accumulated under the sweep
        else if (fused) CHK(eet_lower(c, E, lde, c->Binv, np, np));                   // B^-1 = W^T W = E E^T
        else CHK(lauum_lower(c, c->W, np, c->Binv, np, np));
    }
    HIP_TRY(hipEventRecord(c->ev[5], st));
    // alpha currently holds W^T z / sn2 = B^-1 r / sn2  (already the final alpha)
    const double* grad_alpha = c->alpha_dev;
    if (loo && want >= 2) {
        CHK(pscr.alloc(&lbuf, (size_t)loo_buffer_doubles(np) * sizeof(double)));
        CHK(loo_values_launch(c, n, np, sn2, fused ? E : nullptr, lde, c->y_dev, c->alpha_dev, c->partial, lbuf, st));
        if (want >= 3) {
            double *G = c->W, *svp = nullptr;        // W is free once W'W is formed; beside the fused inverse it was never used
            if (fused) CHK(pscr.alloc(&G, (size_t)np * np * sizeof(double)));         // (E goes on to the posterior handle)
            CHK(pscr.alloc(&svp, (size_t)loo_symv_partial_doubles(np) * sizeof(double)));
            HIP_TRY(hipMemsetAsync(loo_vec(lbuf, np, LOO_ZERO), 0, np * sizeof(double), st));
            CHK(loo_gradient_matrix(c, n, np, sn2, c->alpha_dev, lbuf, G, svp, st));   // c->Binv <- S = sn2 Q_loo
            grad_alpha = loo_vec(lbuf, np, LOO_ZERO);
        }
        CHK(loo_stage(c, (size_t)loo_host_doubles(np)));
    }
    if (want >= 3) {
        ProfScope ps(c, PC_HADAMARD, 0.0, 8.0 * (double)np * (np + 1) / 2.0 + 8.0 * (double)n * d);
        CHK(hadamard_reduce_launch(c->XsT, np, n, np, c->dpad, cp, ncov, sn2, c->Binv, np, grad_alpha, c->partial,
                                   c->scal + 8, st, nullptr, gram ? c->prep : nullptr));
    }
    HIP_TRY(hipEventRecord(c->ev[6], st));
    if (lbuf) HIP_TRY(hipMemcpyAsync(c->loo_host, lbuf, (size_t)loo_host_doubles(np) * sizeof(double), hipMemcpyDeviceToHost, st));   // pinned: queued, not staged
    // ---- results to host: ONE copy of [scalars | status | alpha] into pinned memory ---------------------
    // (round 6) the LAST KERNEL of the fit writes them into the pinned buffer through its device-side address: a copy command
    // behind the last kernel cost a lone chain ~100 us (final_reduce's end to the copy's start in the kernel trace); option publish = 0
    if (c->publish && c->res_host_dev) CHK(publish_launch(c->res_dev, c->res_host_dev, RES_HEAD + n, st));
    else HIP_TRY(hipMemcpyAsync(c->res_host, c->res_dev, (size_t)(RES_HEAD + n) * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const double* sc_host = c->res_host;
    double* alpha_h = c->res_host + RES_HEAD;
    int info = 0;
    memcpy(&info, c->res_host + RES_INFO, sizeof(int));
    if (rwant < 3 && !fused) for (long j = 0; j < n; ++j) alpha_h[j] /= sn2;   // the back-substitution produced L^-T z
    {
        float ms;
        const int map[6][2] = {{0, 1}, {1, 2}, {3, 4}, {2, 3}, {4, 5}, {5, 6}};   // assemble, potrf, solve, trtri, lauum, grad
        for (int i = 0; i < 6; ++i) { (void)hipEventElapsedTime(&ms, c->ev[map[i][0]], c->ev[map[i][1]]); c->last_ms[i] = ms; }
        (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[6]); c->last_ms[PGP_STAGE_TOTAL] = ms;
    }
    if (c->prof) prof_collect(c);
    if (info != 0) return info > (int)n ? (int)n : info;     // the buffer now holds NaNs: fguard scrubs it for the pool
    if (alpha_out) memcpy(alpha_out, alpha_h, n * sizeof(double));
    if (want >= 2 && nlZ_out) {
        const double logdet = sc_host[0], ztz = sc_host[1];
        *nlZ_out = 0.5 * ztz / sn2 + logdet + 0.5 * (double)n * log(2.0 * M_PI * sn2);
    }
    if (lbuf) loo_copy_out(c, loo, n, np, want);
    if (want >= 3 && dnlZ_out) {
        const double* gv = lbuf ? c->loo_host + LOO_U * np : alpha_h;        // LOO: -u' dm_h takes the place of -alpha' dm_h
        for (int i = 0; i < nmean; ++i) {                 // Core/inf.py:378-381
            double s = 0.0;
            for (long j = 0; j < n; ++j) s += dm[(long)i * n + j] * gv[j];
            dnlZ_out[i] = -s;
        }
        for (int h = 0; h < ncov; ++h) dnlZ_out[nmean + h] = 0.5 * sc_host[8 + h];      // inf.py:377
        dnlZ_out[nmean + ncov] = sc_host[8 + ncov];                                     // inf.py:374
    }
    if (factor_out) {
        CHK(finish_factor(c, n, np, ldf, fguard, &cp, kss, sn2, alpha_h, nullptr, hipMemcpyHostToDevice, factor_out));
        // (round 6) the fused inverse rows E = L^-T are what GP.predict's product form needs (W = L^-1 = E'): the handle keeps the
        // scratch buffer instead of the pool, the first predict transposes it (predict.hip ensure_linv) -- no trtri
        if (fused && E && c->keep_inverse && np <= 16384) {
            const size_t eb = pscr.release(E);
            if (eb) { (*factor_out)->Eraw = E; (*factor_out)->Eraw_bytes = eb; }
        }
    }
    fguard.scrub = false;                             // a finished factor honours the pool contract as it is
    return PGP_OK;
}

extern "C" {

int pgp_exact_fit(pgp_ctx* c, int kind, const double* covhyp, int ncov, int para, int flags, double log_sn,
                  const double* mvec, const double* dm, int nmean, int want, double* alpha_out, double* nlZ_out,
                  double* dnlZ_out, pgp_factor** factor_out) {
    return exact_fit_run(c, kind, covhyp, ncov, para, flags, log_sn, mvec, dm, nmean, want, alpha_out, nlZ_out, dnlZ_out, factor_out,
                         nullptr);
}

int pgp_loo_fit(pgp_ctx* c, int kind, const double* covhyp, int ncov, int para, int flags, double log_sn, const double* mvec,
                const double* dm, int nmean, int want, double* alpha_out, double* loo_mu_out, double* loo_s2_out, double* loo_lp_out,
                double* nlZ_out, double* dnlZ_out, pgp_factor** factor_out) {
    LooOut lo{loo_mu_out, loo_s2_out, loo_lp_out, nullptr, 0.0};
    double nlz = 0.0;
    const int rc = exact_fit_run(c, kind, covhyp, ncov, para, flags, log_sn, mvec, dm, nmean, want, alpha_out, &nlz, dnlZ_out,
                                 factor_out, &lo);
    if (rc == PGP_OK && want >= 2 && nlZ_out) { nlZ_out[0] = lo.nlZ_loo; nlZ_out[1] = nlz; }
    return rc;
}

int64_t pgp_factor_n(pgp_factor* f) { return f ? f->n : 0; }

int pgp_factor_to_host(pgp_ctx* c, pgp_factor* f, double* L_out) {
    if (!c) return -1;
    GateShared device_gate_hold(c);
    if (!c || !f) return -1;
    if (!L_out) return -3;
    HIP_TRY(hipSetDevice(c->device));
    // row-major upper R(r, c) lives at F[r*ldf + c]; copy the n x n corner
    HIP_TRY(hipMemcpy2DAsync(L_out, f->n * sizeof(double), f->F, f->ldf * sizeof(double), f->n * sizeof(double), f->n,
                             hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return PGP_OK;
}

void pgp_factor_free(pgp_ctx* c, pgp_factor* f) { GateShared device_gate_hold(c);
    if (!f) return;
    if (c) {
        (void)hipSetDevice(c->device);
        // augmented rows / upper tiles of a pooled buffer must be zero when it is reused: the factor only ever
        // wrote the lower triangle + row np, and row np is rewritten by every fit, so it can go back as is.
        pool_free(c, (size_t)f->ldf * f->np * sizeof(double), f->F);
        if (f->Linv) pool_free(c, (size_t)f->ldf * f->np * sizeof(double), f->Linv);    // (lower triangle only, zero augmented rows: the pool contract holds)
    }
    spool_give(c, (size_t)f->np * sizeof(double), f->alpha);
    spool_give(c, (size_t)f->dpad * f->np * sizeof(double), f->XsT);
    spool_give(c, (size_t)128 * f->np * sizeof(double), f->Wd);
    spool_give(c, (size_t)f->np * sizeof(double), f->sWv);
    if (f->Eraw) spool_give(c, f->Eraw_bytes, f->Eraw);
    delete f;
}

// ---- kernel plug-in ------------------------------------------------------------------------------
int pgp_cov(pgp_ctx* c, int kind, int mode, int der, const double* x, int64_t n, const double* z, int64_t m,
            int64_t d, const double* hyp, int nhyp, int para, int flags, double* out) {
    if (!c) return -1;
    GateShared device_gate_hold(c);
    if (!c) return -1;
    if (mode < 0 || mode > 2) return -3;
    if (!hyp) return -10;
    if (!out) return -14;
    if (mode != PGP_MODE_SELF_TEST && !x) return -5;
    if (mode != PGP_MODE_TRAIN && !z) return -7;
    if (d <= 0) return -9;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->st;
    CovSpec cp;
    CHK(make_spec(c, kind, hyp, nhyp, para, flags, der, d, cp));
    if (cp.has_pre()) return -13;                    // cov.Pre: getCovMatrix / getDerMatrix are host slices and sums (pygps_amd/cov.py)
    if (mode == PGP_MODE_SELF_TEST && cp.diag_per_point()) {
        // dot-product leaves: k(z_j, z_j) (or the selected derivative of it) differs from point to point -- one value per point from
        // the point's own coordinates (Core/cov.py:644-646, 998-1000)
        const int dpad = (int)round_up(d, SKC);
        const long ldc = round_up(m, 128);
        PoolScratch tmp(c);
        double *zd = nullptr, *XcT = nullptr, *scd = nullptr, *od = nullptr;
        CHK(tmp.alloc(&zd, m * d * sizeof(double)));
        CHK(tmp.alloc(&XcT, (size_t)dpad * ldc * sizeof(double)));
        CHK(tmp.alloc(&scd, dpad * sizeof(double)));
        CHK(tmp.alloc(&od, m * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(zd, z, m * d * sizeof(double), hipMemcpyHostToDevice, st));
        CHK(upload_scaled(c, zd, m, d, cp.scale, XcT, ldc, dpad, scd));
        CHK(cov_self_dot_launch(cp, 2, XcT, ldc, dpad, m, od, 0, st));
        HIP_TRY(hipMemcpyAsync(out, od, m * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return PGP_OK;
    }
    if (mode == PGP_MODE_SELF_TEST) {
        // zero distance: the functor itself gives value and derivatives (Core/cov.py:815-817, 924-925, 1163-1177,
        // SURVEY Q6), including the Matern derivative quirk and Noise = 0 on 'self_test' (cov.py:1271)
        double val = 0.0;                              // cov_point_value only needs c->scal: the fit workspace stays as it is
        CHK(cov_point_value(c, cp, 2, &val));
        for (int64_t i = 0; i < m; ++i) out[i] = val;
        return PGP_OK;
    }
    const std::vector<double>& sc = cp.scale;
    const int dpad = (int)round_up(d, SKC);
    const long ldr = round_up(n, 128), ldc = (mode == PGP_MODE_CROSS) ? round_up(m, 128) : 0;
    const long mm = (mode == PGP_MODE_CROSS) ? m : n;
    PoolScratch tmp(c);
    double *xd = nullptr, *zd = nullptr, *XrT = nullptr, *XcT = nullptr, *scd = nullptr, *od = nullptr;
    CHK(tmp.alloc(&xd, n * d * sizeof(double)));
    CHK(tmp.alloc(&XrT, (size_t)dpad * ldr * sizeof(double)));
    CHK(tmp.alloc(&scd, dpad * sizeof(double)));
    CHK(tmp.alloc(&od, (size_t)n * mm * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(xd, x, n * d * sizeof(double), hipMemcpyHostToDevice, st));
    CHK(upload_scaled(c, xd, n, d, sc, XrT, ldr, dpad, scd));
    if (mode == PGP_MODE_CROSS) {
        CHK(tmp.alloc(&zd, m * d * sizeof(double)));
        CHK(tmp.alloc(&XcT, (size_t)dpad * ldc * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(zd, z, m * d * sizeof(double), hipMemcpyHostToDevice, st));
        CHK(scale_transpose_launch(zd, m, (int)d, scd, XcT, ldc, dpad, st));
    }
    {
        ProfScope ps(c, PC_ASSEMBLE, 0.0, 8.0 * (double)n * mm + 8.0 * (double)(n + (mode == PGP_MODE_CROSS ? m : 0)) * d);
        // getCovMatrix('train') of RBF / RBFard at d >= 32 and n >= 4096 (cfg 3's size): the Gram form on the matrix cores under the
        // same host-side norm bound as the fit's assembly (gram_assembly_applies; K within ~5e-14 relative of the difference form --
        // kernel-matrix parity is held to 1e-13); the statistics of THIS x are taken here on the host (n d operations)
        bool gram = false;
        if (mode == PGP_MODE_TRAIN && der < 0 && n >= 4096 && c->gram_assembly && cov_gram_applies(cp, dpad) && (long)sc.size() >= d) {
            gram = c->gram_assembly == 2;
            if (!gram) {
                double bound = 0.0;
                for (int64_t k = 0; k < d; ++k) {
                    double mean = 0.0, dev = 0.0;
                    for (int64_t p = 0; p < n; ++p) mean += x[p * d + k];
                    mean /= (double)n;
                    for (int64_t p = 0; p < n; ++p) dev = std::max(dev, fabs(x[p * d + k] - mean));
                    bound += sc[k] * sc[k] * dev * dev;
                }
                gram = bound <= 64.0;
            }
        }
        if (gram) {
            double* prep = nullptr;
            CHK(tmp.alloc(&prep, (size_t)hadamard_prep_count(ldr) * sizeof(double)));
            CHK(hadamard_prepare_launch(XrT, ldr, n, ldr, dpad, cp, prep, st, /*force=*/true));
            CHK(cov_sym_gram_launch(XrT, ldr, n, dpad, cp, od, n, prep, st));
        } else if (mode == PGP_MODE_TRAIN) CHK(cov_sym_launch(XrT, ldr, n, dpad, cp, od, st));
        else CHK(cov_rect_launch(XrT, ldr, n, XcT, ldc, m, dpad, cp, od, m, st));
    }
    HIP_TRY(hipMemcpyAsync(out, od, (size_t)n * mm * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (c->prof) prof_collect(c);
    return PGP_OK;
}

// ---- helper functions ------------------------------------------------------------------------------
int pgp_potrf(pgp_ctx* c, const double* A, int64_t n, double* L_out) {
    if (!c) return -1;
    GateShared device_gate_hold(c);
    if (!c) return -1;
    if (!A) return -2;
    if (n <= 0) return -3;
    if (!L_out) return -4;
    HIP_TRY(hipSetDevice(c->device));
    const long np = round_up(n, 128);
    hipStream_t st = c->st;
    PoolScratch tmp(c);
    double *F = nullptr, *pack = nullptr;
    CHK(tmp.alloc(&F, (size_t)np * np * sizeof(double)));
    CHK(tmp.alloc(&pack, (size_t)(np / 128) * PACK_DOUBLES * sizeof(double)));
    HIP_TRY(hipMemsetAsync(F, 0, (size_t)np * np * sizeof(double), st));
    // symmetric input: row-major == column-major; copy the n x n corner, identity on the padding
    HIP_TRY(hipMemcpy2DAsync(F, np * sizeof(double), A, n * sizeof(double), n * sizeof(double), n, hipMemcpyHostToDevice, st));
    std::vector<double> ones(np - n + 1, 1.0);
    if (np > n)
        HIP_TRY(hipMemcpy2DAsync(F + n + n * np, (np + 1) * sizeof(double), ones.data(), sizeof(double), sizeof(double),
                                 np - n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(c->info_dev, 0, sizeof(int), st));
    double* pack_save = c->inv16;                  // the blocked driver takes the per-leaf operand images from the ctx
    c->inv16 = pack;
    SweepJob job{F, np, np, np};
    const int rc = potrf_blocked(c, job);
    c->inv16 = pack_save;
    CHK(rc);
    int info = 0;
    HIP_TRY(hipMemcpyAsync(&info, c->info_dev, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (c->prof) prof_collect(c);
    if (info != 0) return info > (int)n ? (int)n : info;
    // device holds column-major lower L; numpy wants row-major lower => transpose on the host
    std::vector<double> host((size_t)n * n);
    HIP_TRY(hipMemcpy2D(host.data(), n * sizeof(double), F, np * sizeof(double), n * sizeof(double), n,
                        hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < n; ++j) L_out[i * n + j] = (j <= i) ? host[(size_t)j * n + i] : 0.0;
    return PGP_OK;
}

}  // extern "C"
