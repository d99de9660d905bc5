#!/usr/bin/env python3
"""Benchmark of the exact-GP hot path on MI355X (metric of BASELINE.json).

One "step" = one GP fit = Exact.evaluate(..., nargout=3): kernel assembly -> Cholesky -> alpha -> nlZ
-> all hyper-gradients, with x, y resident in HBM and only the hyper-parameters changing (what the
optimiser does, Core/opt.py:70-75); outputs returned to the host per step: nlZ, dnlZ, alpha.
Workload at N GPUs: BASELINE configs[1] (GPR + RBF, N=8192, d=16, fp64, synthetic recipe of SURVEY
8(d)) on EVERY rank with rank-specific hyper-parameters -- i.e. independent objective evaluations of
the restart search (configs[3]) sharded one stream of fits per GPU; RCCL is used only for the
broadcast of (x, y) before and the all-gather of results after the timed region ("weak" scaling).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times ONE window of exactly K steps (bracketed by
barrier + synchronize), optionally writes the last step's outputs (--dump-outputs) and prints the headline:
`value` = K / window time, `ms_per_step` = window time / K.  Everything below is measured only with --full,
which also times the K-step window `--windows` times (default 5; `value` is K / median window time, every
window is listed).  `roofline` is for the dominant
kernel (gemm_f64_kernel, the fp64 MFMA GEMM behind the Cholesky trailing updates, the panel solves, the
fused triangular inverse and E E'): ALGORITHMIC flops of a fit that run in it (N^3: Cholesky N^3/3 +
inverse N^3/3 + E E' N^3/3) / its launches / their average duration, measured with HIP events on the
library's own stream in a single-stream profiled pass over the same steps (profiles/README.md says which
rocprofv3 CSV reproduces it); the executed/algorithmic flop ratio and the aggregate rate of the timed
(multi-stream) window are reported beside it.  `cpu_baseline` (N=1 only) times the oracle's
reference-faithful CPU path (scipy cdist + LAPACK dpotrf + general-LU solve_chol + one derivative matrix
per hyper, call-for-call what pyGPs does) on this host's cores: ONE full fit at the benchmark size.

Schema notes.  `per_rank_fits_per_s` lists every rank's own rate, `value` the aggregate (the slowest rank's window).  The
collective extras of --full (`cfg4_restarts_N8192`, `sharded_fit`) run after the timed region behind a 300 s watchdog:
`collective_extras_ok` is false -- and `collective_extras_error` says why -- when they did not finish; the line (and rc 0)
still goes out so that the headline survives a stall on hardware the collective path has never seen.  With `--gpus N > 1`
and no launcher environment the script re-executes itself under `python -m torch.distributed.run --nproc-per-node N`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("PYGPS_AMD_TORCH_FIRST", "1")   # this process runs torch.distributed beside the library (pygps_amd/_lib.py)

PEAK_FP64_MFMA_TF = 78.6      # MI355X fp64 matrix peak: 128 flop/clk/CU x 256 CU x 2.4 GHz (measured issue rate 77.6)
PEAK_HBM_GBS = 8000.0


def synth_reg(N, d, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.randn(N, d)
    w = rng.randn(d, 1)
    y = np.sin(x @ w / np.sqrt(d)) + 0.1 * rng.randn(N, 1)
    return x, y


def hyp_for(step, rank, d):
    """Hyper-parameters of one objective evaluation: the cfg-2 point, nudged so that no two steps repeat."""
    eps = 1e-3 * ((step * 7 + rank * 13) % 101) / 101.0
    return np.array([np.log(np.sqrt(d)) + eps, 0.0 - eps]), float(np.log(0.1) + 0.5 * eps)


def usable_cpus():
    """Cores this process may actually use: the affinity mask, capped by the container's CFS quota (cgroup v2 cpu.max / v1
    cfs_quota_us).  The GPU boxes show 256 cores and grant 16: a BLAS pool of 128-256 threads is throttled there, not faster."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(np.ceil(float(q) / float(p)))))
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, int(np.ceil(q / p))))
        except Exception:
            pass
    return n


def cpu_baseline(N, d, budget_s=150.0):
    """Reference-faithful CPU path (oracle) on the host cores: ONE full fit at (N, d) unless a half-size fit predicts more
    than budget_s (then the half-size time is scaled and labelled as such).  Also returns the measured exponent between
    N/2 and N (SURVEY section 6 measured x5.5 for 4096 -> 8192 on 8 cores, i.e. not a clean N^3)."""
    from oracle import gp_oracle as O
    ncpu = usable_cpus()
    try:
        from threadpoolctl import threadpool_info, threadpool_limits
        # one BLAS thread per core the container may use (kept for the rest of the process: the CPU legs run after the timed region)
        cpu_baseline._limit = threadpool_limits(limits=ncpu)
        thr = max([p.get("num_threads", 1) for p in threadpool_info()] or [1])
    except Exception:
        thr = ncpu

    def one(n, faithful=True):
        x, y = synth_reg(n, d)
        c = float(y.mean())
        t = time.perf_counter()
        O.exact_fit(O.RBF, np.array([np.log(np.sqrt(d)), 0.0]), 0, np.log(0.1), x, y, c * np.ones_like(y),
                    np.ones_like(y), nargout=3, faithful=faithful)
        return time.perf_counter() - t

    one(512)                                            # warm the BLAS threads
    th = one(N // 2)
    out = {"unit": "fits/s", "cores": int(thr), "kind": "port", "host_cpu_count": os.cpu_count(), "usable_cpus": ncpu,
           "half_size_fit_s": th}
    if th * 8 <= budget_s:
        t = one(N)
        out["sample"] = ("1 full fit at N=%d d=%d (%.1f s), oracle reference-faithful path (cdist + dpotrf + LU solve_chol x2 + "
                         "one derivative matrix per hyper); N=%d took %.1f s" % (N, d, t, N // 2, th))
        out["exponent_N_half_to_N"] = float(np.log(t / th) / np.log(2.0))
    else:
        t = th * 8
        out["sample"] = ("1 fit at N=%d d=%d took %.1f s; scaled by 2^3 to N=%d because the full fit would exceed the %.0f s "
                         "budget (EXTRAPOLATED, not measured)" % (N // 2, d, th, N, budget_s))
    out["value"] = 1.0 / t
    ts = one(N // 2, faithful=False)                    # same maths with triangular solves + potri, half size, scaled
    out["value_sane_linear_algebra"] = 1.0 / (ts * 8)
    out["sane_sample"] = "N=%d in %.1f s, scaled by 2^3" % (N // 2, ts)
    return out


def cpu_baseline_other_configs(cfg2_fits_per_s):
    """CPU baselines of BASELINE configs[2], [3], [4] on this host, bounded samples of the same workloads through the oracle's
    reference-faithful path, scaled to the configured size by the stated model and LABELLED as extrapolations.  Beside them:
    the wall times the reference itself took in the build container (8 cores) when the fixtures were recorded."""
    from oracle import gp_oracle as O
    out = {}
    # cfg 3: GPR + SEard, N = 16384, d = 64.  Sample: one faithful fit at N = 2048 (67 gradients: 65 derivative matrices).
    try:
        n, d = 2048, 64
        x, y = synth_reg(n, d)
        c = float(y.mean())
        hyp = np.concatenate([np.full(d, np.log(np.sqrt(d))), [0.0]])
        t = time.perf_counter()
        O.exact_fit(O.RBFARD, hyp, 0, np.log(0.1), x, y, c * np.ones_like(y), np.ones_like(y), nargout=3, faithful=True)
        t3 = time.perf_counter() - t
        # model: dense linear algebra ~ N^3, derivative assembly 65 N^2 d; both terms grow by >= 64 from N = 2048
        # to 16384 -- the N^2 d term by 64, the N^3 term by 512: the bracket [x64, x512] is reported, the headline uses x512
        # only for the share the N = 2048 fit spends outside getDerMatrix (timed separately below)
        t = time.perf_counter()
        O.der_matrix(O.RBFARD, hyp, 0, x=x, mode="train", der=0)
        tder = (time.perf_counter() - t) * (d + 1)
        tder = min(tder, t3)
        est = (t3 - tder) * 512.0 + tder * 64.0
        out["cfg3"] = {"value": 1.0 / est, "unit": "fits/s", "kind": "port", "extrapolated": True,
                       "sample": "1 faithful oracle fit at N=2048 d=64 (%.1f s, of which ~%.1f s in 65 getDerMatrix calls), scaled to "
                                 "N=16384 as x512 on the N^3 part and x64 on the 65 N^2 d part => %.0f s per fit (EXTRAPOLATED)"
                                 % (t3, tder, est),
                       "reference_recorded": "the reference itself, build container, 8 cores: N=16384 d=64 getPosterior 2969 s "
                                             "(tests/golden/G7_rbfard_d64_N16384.npz ref_seconds); N=4096: 160 s"}
    except Exception as e:           # pragma: no cover
        out["cfg3"] = {"error": repr(e)}
    # cfg 5: GPC + RBF, infEP, N = 4096, d = 32.  Sample: oracle EP (the reference's per-site full-matrix update) at N = 512.
    try:
        n, d = 512, 32
        rng = np.random.RandomState(0)
        x = rng.randn(n, d); w = rng.randn(d, 1)
        y = np.sign(x @ w / np.sqrt(d) + 0.3 * rng.randn(n, 1)); y[y == 0] = 1
        t = time.perf_counter()
        r = O.ep_fit(O.RBF, np.array([np.log(np.sqrt(d)), 0.0]), 0, x, y, np.zeros_like(y))
        t5 = time.perf_counter() - t
        sw = int(r.get("sweeps", 4))
        est = t5 * 8.0 ** 3                      # per sweep: N sites x O(N^2) each + an N^3 rebuild; same sweep count (4) at N = 4096
        out["cfg5"] = {"value": 1.0 / est, "unit": "fits/s", "kind": "port", "extrapolated": True,
                       "sample": "1 oracle EP fit at N=512 d=32 (%.1f s, %d sweeps), scaled by 8^3 to N=4096 => %.0f s per fit "
                                 "(EXTRAPOLATED; N^3 per sweep, 4 sweeps at both sizes)" % (t5, sw, est),
                       "reference_recorded": "the reference itself, build container, 8 cores: N=4096 ~43 min per fit (G8ii N=4096), "
                                             "N=512 4.1 s"}
    except Exception as e:           # pragma: no cover
        out["cfg5"] = {"error": repr(e)}
    # cfg 4 = the cfg-2 fit, 8 restarts x minimize.run: the optimiser's cost is the fits it asks for
    out["cfg4"] = {"value": cfg2_fits_per_s, "unit": "fits/s", "kind": "port", "extrapolated": True,
                   "sample": "derived: every objective evaluation of the restart search is one cfg-2 fit (N=8192 d=16), so the CPU "
                             "rate is the cfg-2 figure of this run; a cfg-4 search of ~374 fits would take %.1f h on this host"
                             % (374.0 / cfg2_fits_per_s / 3600.0)}
    return out


def _fit_args(lib, _lib, h, kind, hyp, log_sn, m, dm, out):
    alpha, nlZ, g = out
    return lib.pgp_exact_fit(h, kind, _lib.ptr(hyp), len(hyp), 0, 0, log_sn, _lib.ptr(m), _lib.ptr(dm), 1, 3,
                             _lib.ptr(alpha), _lib.ptr(nlZ), _lib.ptr(g), None)


def extras(lib, _lib, local, d, roof):
    """Driver-run figures of the other single-GPU configs, OUTSIDE the timed region, a few seconds in total."""
    import ctypes
    # ---- north-star assembly figure: full symmetric K (getCovMatrix 'train'), N=16384, device-resident coordinates,
    #      algorithmic bytes 8 N^2 + 8 N d, HIP-event time over 100 launches: RBF d=16 and SEard d=64
    ctx = _lib.ctx(local)
    na = 16384
    for key, kind, dd in (("assembly_full_N16384", _lib.COV_RBF, 16), ("assembly_full_N16384_SEard_d64", _lib.COV_RBFARD, 64)):
        ms_a = ctypes.c_double()
        if lib.pgp_test_assemble(ctx, kind, 0, na, dd, 100, ctypes.byref(ms_a)) == 0 and ms_a.value > 0:
            ba = 8.0 * na * na + 8.0 * na * dd
            roof[key] = {"ms": ms_a.value, "GBs": ba / ms_a.value / 1e6, "bound": "hbm",
                         "frac_of_hbm_peak": ba / ms_a.value / 1e6 / PEAK_HBM_GBS}
            if dd == 16:
                # the same box's answer to "what do the stores alone cost": the 'train' tiles written twice in the same order by a
                # kernel without any arithmetic (csrc/testhooks.hip pgp_test_store_roof; no symmetric tile pattern of
                # tools/store_roof.hip writes faster), hipMemsetAsync and a one-store-per-thread linear fill over the same bytes
                o3 = (ctypes.c_double * 3)()
                if lib.pgp_test_store_roof(ctx, na, 0, 50, o3) == 0 and min(o3) > 0:
                    roof[key].update({"stores_alone_same_pattern_ms": o3[0], "frac_of_stores_alone": o3[0] / ms_a.value,
                                      "stores_alone_frac_of_hbm_peak": 8.0 * na * na / o3[0] / 1e6 / PEAK_HBM_GBS,
                                      "memset_frac_of_hbm_peak": 8.0 * na * na / o3[1] / 1e6 / PEAK_HBM_GBS,
                                      "linear_fill_frac_of_hbm_peak": 8.0 * na * na / o3[2] / 1e6 / PEAK_HBM_GBS})
            if dd == 64:
                # d = 64 (round 4): this is the form a FIT picks for such data -- squared distances in the Gram form on the matrix
                # cores (csrc/assemble.hip cov_gram_kernel; the per-call means and norms are inside the timed loop), chosen by the
                # host's norm bound; getCovMatrix keeps the reference's difference form (0.27 of the HBM roof, 0.40 of the fp64
                # vector roof executed: rounds 2-3 quoted that kernel here).  MFMA flops 2 d per output on the tiles computed
                # (upper triangle, each stored twice): far from the matrix roof -- the kernel is bound by its stores.
                nt = -(-na // 64)
                mf = 2.0 * dd * 64.0 * 64.0 * nt * (nt + 1) / 2.0
                roof[key].update({"bound": "hbm (write): %.2f of the HBM peak; MFMA Gram products %.1f TFLOP/s"
                                           % (ba / ms_a.value / 1e6 / PEAK_HBM_GBS, mf / ms_a.value / 1e9),
                                  "form": "Gram form on centred coordinates (v_mfma_f64_16x16x4), selected by the host's norm bound",
                                  "mfma_TFLOPs": mf / ms_a.value / 1e9,
                                  # the other roof (SURVEY 7 allows both for d = 64): issue cycles of the fp64 pipe per 64 x 64 tile and
                                  # wave, read off the ISA of cov_gram_fast_kernel<SYM, 16, 2> (round 6): 64 v_mfma_f64_16x16x4 (64 cycles
                                  # each) + 244 fp64 VALU instructions (4 cycles each), over the tiles computed, at the 2.4 GHz peak clock
                                  "fp64_pipe_cycles_per_tile_wave": 64 * 64 + 244 * 4,
                                  "frac_of_fp64_pipe": (64 * 64 + 244 * 4) * (nt * (nt + 1) / 2.0 * 4.0 / 1024.0) / (ms_a.value * 1e-3 * 2.4e9)})
    out = {}
    # ---- cfg 3 (GPR + SEard, N=16384 d=64, nlZ + 67 gradients) and the N=16384 RBF Cholesky figure ----------------
    for key, kind, dd in (("cholesky_sweep_N16384", _lib.COV_RBF, d), ("cfg3_seard_N16384_d64", _lib.COV_RBFARD, 64)):
        hb = ctypes.c_void_p()
        nb_ = 16384
        if lib.pgp_init(local, ctypes.byref(hb)) != 0:
            continue
        try:
            xb, yb = synth_reg(nb_, dd)
            ybv = np.ascontiguousarray(yb).ravel()
            mb, dmb = np.full(nb_, ybv.mean()), np.ones((1, nb_))
            nh = 2 if kind == _lib.COV_RBF else dd + 1
            bufs = (np.empty(nb_), np.zeros(1), np.zeros(nh + 2))
            if lib.pgp_set_data(hb, _lib.ptr(np.ascontiguousarray(xb)), nb_, dd, _lib.ptr(ybv)) != 0:
                continue
            def run_fits(count, first=0):
                res = []
                for it in range(first, first + count):
                    eps = 1e-3 * it
                    hyp_b = (np.array([np.log(np.sqrt(dd)) + eps, -eps]) if kind == _lib.COV_RBF
                             else np.concatenate([np.full(dd, np.log(np.sqrt(dd)) + eps), [-eps]]))
                    if _fit_args(lib, _lib, hb, kind, hyp_b, float(np.log(0.1)), mb, dmb, bufs) != 0:
                        return None
                    st_b = np.zeros(len(_lib.STAGES))
                    lib.pgp_last_timings(hb, _lib.ptr(st_b))
                    res.append(dict(zip(_lib.STAGES, st_b.tolist())))
                return res
            tb = run_fits(3)                                       # default schedule (E E^T folded into the sweep)
            ts = None
            if tb and lib.pgp_set_option(hb, b"eet_overlap", 0) == 0:
                ts = run_fits(2, 3)                                # E E^T as one product after the sweep: the sweep-alone figure
                lib.pgp_set_option(hb, b"eet_overlap", 3)
            if tb and ts:
                pm = min(t["potrf"] for t in ts)
                ft = min(t["total"] for t in tb[1:])
                fm = min(t["potrf"] + t["solve"] + t["trtri"] + t["lauum"] for t in tb[1:])
                rec = {"ms": pm, "TFLOPs": (2.0 * nb_ ** 3 / 3.0) / (pm * 1e-3) / 1e12, "bound": "mfma",
                       "frac_of_peak": (2.0 * nb_ ** 3 / 3.0) / (pm * 1e-3) / 1e12 / PEAK_FP64_MFMA_TF,
                       "what": "sweep + fused inverse alone (option eet_overlap=0): 2 N^3 / 3 flops / potrf stage time",
                       "fit_ms": ft, "fit_TFLOPs": float(nb_) ** 3 / (ft * 1e-3) / 1e12,
                       "factor_inverse_EEt_ms": fm, "factor_inverse_EEt_frac_of_peak": float(nb_) ** 3 / (fm * 1e-3) / 1e12 / PEAK_FP64_MFMA_TF,
                       "EEt_alone_ms": min(t["lauum"] for t in ts),
                       "stage_ms": tb[-1]}
                if kind == _lib.COV_RBF:
                    roof[key] = rec
                else:
                    rec = {"fit_ms": ft, "fit_TFLOPs": rec["fit_TFLOPs"], "fits_per_s": 1e3 / ft, "n_gradients": dd + 3,
                           "cholesky_sweep_ms": pm, "cholesky_sweep_frac_of_peak": rec["frac_of_peak"],
                           "assembly_fused_ms": tb[-1]["assemble"], "hadamard_reduce_ms": tb[-1]["grad"],
                           "EEt_alone_ms": rec["EEt_alone_ms"], "factor_inverse_EEt_ms": rec["factor_inverse_EEt_ms"],
                           "factor_inverse_EEt_frac_of_peak": rec["factor_inverse_EEt_frac_of_peak"], "stage_ms": tb[-1],
                           "workload": "BASELINE configs[2]: GPR + SEard, N=16384 d=64 fp64 synthetic, infExact nlZ + all hyper-gradients"}
                    out[key] = rec
        finally:
            lib.pgp_destroy(hb)
    # ---- cfg 5 (GPC + RBF, infEP, N=4096 d=32) through the drop-in API ------------------------------------------------
    try:
        import pygps_amd as pyGPs
        n5, d5 = 4096, 32
        rng = np.random.RandomState(0)
        x5 = rng.randn(n5, d5); w5 = rng.randn(d5, 1)
        y5 = np.sign(x5 @ w5 / np.sqrt(d5) + 0.3 * rng.randn(n5, 1)); y5[y5 == 0] = 1
        ts, sw = [], 0
        for it in range(2):
            m5 = pyGPs.GPC()
            m5.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(np.log(np.sqrt(d5)), 0.0))
            t = time.perf_counter()
            nlz5 = m5.getPosterior(x5, y5)[0]
            ts.append(time.perf_counter() - t)
            sw = int(m5.inffunc.sweeps)
            ph5 = _lib.last_timings(local)            # EP phases (host wall clock, each phase ends synchronised): see csrc/ep.hip
        t5 = min(ts)
        # block sweep: per block of 128 sites the strip Sigma(:, B) is copied (8 N 128 B read + written), U = strip W written and
        # read (2 x 8 N 128), and ONE K = 128 fold touches the lower triangle of Sigma (read + write 8 N^2 B: every row -- the
        # posterior is carried through the sweeps, not rebuilt after each)
        nblk5 = n5 // 128
        bytes_sweep = nblk5 * (4 * 8.0 * n5 * 128 + 8.0 * n5 * n5)
        rebuilds = 1                                   # ONE factorisation after the sweeps (post.L of the converged site parameters)
        out["cfg5_ep_N4096_d32"] = {
            "fit_ms": t5 * 1e3, "sweeps": sw, "ms_per_sweep_incl_params": t5 * 1e3 / max(sw, 1), "nlZ": float(nlz5),
            "algorithmic_bytes_per_sweep_blocked": bytes_sweep,
            "reference_algorithm_bytes_per_sweep": 16.0 * n5 ** 3,
            "site_sweep_GB_per_sweep": bytes_sweep / 1e9,
            # round 4: Sigma, mu, log det B are carried AND returned from; after the sweeps only post.L = chol(I + sW sW' o K) is
            # computed afresh (N^3 / 3 flops; a full _epComputeParams is 8 N^3 / 3: option ep_final_rebuild=1)
            "final_factor_flops": n5 ** 3 / 3.0,
            "epComputeParams_calls_per_fit": 0,
            "schedule": "Sigma, mu, log det B carried through the sweeps by exact identities (Woodbury folds per block of 128 sites, "
                        "determinant lemma per site); alpha, nlZ and the gradients come from the carried state, post.L from ONE plain "
                        "Cholesky after the sweeps (options: ep_final_rebuild=1 one full _epComputeParams instead, ep_recompute=1 a rebuild "
                        "after every sweep = the reference's schedule, inf.py:772).  One resident kernel per sweep (1 chain + 36 prep "
                        "workgroups) beside the bulk stream's folds; hand-overs through device counters, no launch per block",
            # the split the site sweep / parameter recomputation figures are read from (last of the two fits)
            "site_sweep_ms": ph5["solve"] / max(sw, 1), "site_sweep_GBs": bytes_sweep / (ph5["solve"] / max(sw, 1)) / 1e6,
            "site_sweep_frac_of_hbm_peak": bytes_sweep / (ph5["solve"] / max(sw, 1)) / 1e6 / PEAK_HBM_GBS,
            "site_sweep_bound": "4096 sequentially dependent site updates per sweep (~0.7 us each inside ep_chain_kernel) + a ~22 us hand-over per block of 128, not bandwidth",
            "params_ms": ph5["potrf"] / rebuilds, "params_what": "the final factorisation (chain of diagonal blocks bound at N = 4096)",
            "params_TFLOPs": n5 ** 3 / 3.0 / (ph5["potrf"] / rebuilds) / 1e9,
            "params_frac_of_mfma_peak": n5 ** 3 / 3.0 / (ph5["potrf"] / rebuilds) / 1e9 / PEAK_FP64_MFMA_TF,
            "first_params_and_K_ms": ph5["assemble"], "alpha_and_gradients_ms": ph5["grad"],
            "workload": "BASELINE configs[4]: GPC + RBF, infEP, N=4096 d=32 (cold start, nlZ + gradients, through model.getPosterior)"}
    except Exception as e:           # pragma: no cover
        out["cfg5_ep_N4096_d32"] = {"error": repr(e)}
    # ---- SURVEY 8(f) rows 1 and 3 through the drop-in API: predict throughput on the cfg-2 posterior, one FITC fit -----
    try:
        import pygps_amd as pyGPs
        n6, d6, ns = 8192, 16, 65536
        x6, y6 = synth_reg(n6, d6)
        m6 = pyGPs.GPR()
        m6.setPrior(kernel=pyGPs.cov.RBF(np.log(np.sqrt(d6)), 0.0)); m6.setNoise(np.log(0.1))
        m6.getPosterior(x6, y6)
        xs6 = np.random.RandomState(1).randn(ns, d6)
        m6.predict(xs6[:4096])
        # round 6: every call of this shape is timed, wall AND device (pgp_predict's own events, _lib.last_timings: assemble = host ms
        # spent getting scratch, solve = wall of the library call, total = device ms).  The FIRST call at a batch shape allocates its
        # scratch (4 GiB here) and meets a cool chip; later calls take the scratch from the pool and run ~25 % slower on the device (a
        # 100 ms burst of fp64 MFMA at full power).  `ms` is the median of the warm calls; the first call is reported beside it.
        calls = []
        for it in range(4):
            t = time.perf_counter(); m6.predict(xs6); wall = (time.perf_counter() - t) * 1e3
            lt = _lib.last_timings(local)
            calls.append({"wall_ms": wall, "device_ms": lt["total"], "library_call_ms": lt["solve"], "scratch_alloc_ms": lt["assemble"]})
        warm = sorted(calls[1:], key=lambda c_: c_["wall_ms"])[len(calls[1:]) // 2]
        tp = warm["wall_ms"] * 1e-3
        out["predict_N8192_ns65536"] = {
            "ms": warm["wall_ms"], "device_ms": warm["device_ms"], "host_share": 1.0 - warm["device_ms"] / warm["wall_ms"],
            "first_call_ms": calls[0]["wall_ms"], "first_call_device_ms": calls[0]["device_ms"],
            "first_call_scratch_alloc_ms": calls[0]["scratch_alloc_ms"], "calls": calls,
            "test_points_per_s": ns / tp,
            "TFLOPs": (1.0 * n6 * n6 * ns) / tp / 1e12,     # fs2 needs V = L^-1 Ks: a triangular solve, N^2 flops per test point
            "what": "GP.predict (ym, ys2, fm, fs2, lp) of 65536 test points on the N=8192 posterior; host arrays in and out; median of "
                    "3 warm calls (wall), device time from the library's own events"}
        # round 6: the product form (V = L^-1 Ks as one fold-rows MFMA product with the posterior's cached W = L^-1; the default for
        # batches >= 1024 points) beside the blocked triangular solve, at the reference's own batch size (1000 points, gp.py:395) and
        # at 8192; the 65536-point figure above is the same for both (a sustained full-chip fp64 burst settles at the power limit)
        sm = {}
        for mode, tag in ((1, "product_form"), (0, "blocked_solve")):
            _lib.check(lib.pgp_set_option(_lib.ctx(local), b"predict_inverse", mode))
            for pts in (1000, 8192):
                m6.predict(xs6[:pts])
                ts_ = []
                for it in range(5):
                    t = time.perf_counter(); m6.predict(xs6[:pts]); ts_.append((time.perf_counter() - t) * 1e3)
                sm["ns%d_%s_ms" % (pts, tag)] = float(np.median(ts_))
        _lib.check(lib.pgp_set_option(_lib.ctx(local), b"predict_inverse", 1))
        out["predict_N8192_small_batches"] = sm
        nf, nuf, df = 131072, 1024, 16
        rng = np.random.RandomState(0)
        xf = rng.randn(nf, df); wf = rng.randn(df, 1)
        yf = np.sin(xf @ wf / np.sqrt(df)) + 0.1 * rng.randn(nf, 1)
        uf = xf[rng.choice(nf, nuf, replace=False)] + 0.01 * rng.randn(nuf, df)
        mf = pyGPs.GPR_FITC()
        mf.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(np.log(np.sqrt(df)), 0.0), inducing_points=uf)
        mf.setNoise(np.log(0.1))
        mf.getPosterior(xf, yf)
        tsf = []
        for it in range(3):
            mf.covfunc.hyp = [np.log(np.sqrt(df)) + 1e-3 * it, 0.0]
            t = time.perf_counter(); mf.getPosterior(xf, yf); tsf.append(time.perf_counter() - t)
        tf = min(tsf)
        out["fitc_n131072_nu1024"] = {
            "fit_ms": tf * 1e3, "TFLOPs_on_nu2n_products": 2.0 * nuf * nuf * nf * 8 / tf / 1e12,
            "what": "GPR_FITC.getPosterior (nlZ + 3 gradients), n=131072, 1024 inducing points, d=16; "
                    "flop model: 8 products of 2 nu^2 n (V, V V', B, W, B W' and two per hyper)"}
    except Exception as e:           # pragma: no cover
        out["predict_fitc_error"] = repr(e)
    return out


# The driver's record keeps only the leading scalar members of `roofline` (24 of them in BENCH_r05.json): the contract members and
# the north-star figures of every config come FIRST, in this order; `tests/test_gpu_api.py::test_bench_line_contract_small` asserts it.
ROOFLINE_HEAD = (
    "kernel", "bound", "achieved", "peak", "unit", "frac", "traffic",
    "assembly_full_N16384_frac_of_hbm_peak", "assembly_SEard_d64_N16384_frac_of_hbm_peak",
    "assembly_SEard_d64_N16384_frac_of_fp64_pipe", "cholesky_sweep_N16384_frac_of_peak", "cholesky_sweep_frac_of_peak",
    "single_stream_ms_per_fit", "cfg4_as_written_fits_per_s_per_gpu", "two_stream_fits_per_s_per_gpu",
    "cfg3_fit_ms", "cfg5_fit_ms", "predict_ns65536_ms", "predict_ns65536_device_ms", "sharded_fit_wait_share",
    "timed_window_frac_of_peak", "assembly_fused_frac_of_hbm_peak")
ROOFLINE_KERNEL_SHORT = "gemm_tile<128,128> fp64 MFMA (rows gemm_f64_kernel<128,128,0,0,1,1> + gemm_f64_pair_kernel<1>)"


def flatten_roofline(out):
    """(flat, detail): `roofline` with scalars only, ROOFLINE_HEAD first -- the contract members, then the north-star figures of
    every config -- and everything long or nested (`kernel` in full, `how`, `traffic_source`, `*_what`, the sched-0 diagnostics, the
    nested objects) in `roofline_detail`."""
    roof = out["roofline"]
    rest, detail = {}, {}
    for k, v in roof.items():
        if isinstance(v, (dict, list, tuple)) or isinstance(v, str) and len(v) > 120 or k.endswith("_what") or k.endswith("_sched0"):
            detail[k] = v
        else:
            rest[k] = v

    def get(obj, *path):
        for p_ in path:
            if not isinstance(obj, dict) or p_ not in obj:
                return None
            obj = obj[p_]
        return obj if isinstance(obj, (int, float, str, bool)) or obj is None else None
    tw = detail.get("timed_window") or {}
    fe = detail.get("factor_inverse_EEt") or {}
    rest.update({
        "kernel": ROOFLINE_KERNEL_SHORT,
        # cfg 2 (the headline): two-stream window, ONE dependent chain, cfg 4 as written (one chain per GPU)
        "timed_window_frac_of_peak": tw.get("frac_of_peak"), "timed_window_streams": tw.get("streams"),
        "factor_inverse_EEt_ms": fe.get("ms"), "factor_inverse_EEt_frac_of_peak": fe.get("frac_of_peak"),
        "all_gemm_f64_frac": get(detail, "all_gemm_f64_instantiations", "frac"),
        "single_stream_ms_per_fit": out.get("single_stream_ms_per_fit"),
        "single_stream_fits_per_s": out.get("single_stream_fits_per_s"),
        "cfg4_as_written_fits_per_s_per_gpu": out.get("cfg4_as_written_fits_per_s_per_gpu"),
        "cfg4_as_written_fits_per_s": out.get("cfg4_as_written_fits_per_s"),
        "two_stream_fits_per_s_per_gpu": out.get("per_gpu_fits_per_s"),
        "api_fits_per_s": out.get("api_fits_per_s"),
        # north star: ">= 60 % of HBM peak on kernel assembly at N = 16384", ">= 50 % of the fp64-MFMA roofline on the Cholesky panel"
        "assembly_full_N16384_ms": get(detail, "assembly_full_N16384", "ms"),
        "assembly_full_N16384_frac_of_hbm_peak": get(detail, "assembly_full_N16384", "frac_of_hbm_peak"),
        "assembly_stores_alone_frac_of_hbm_peak": get(detail, "assembly_full_N16384", "stores_alone_frac_of_hbm_peak"),
        "assembly_SEard_d64_N16384_ms": get(detail, "assembly_full_N16384_SEard_d64", "ms"),
        "assembly_SEard_d64_N16384_frac_of_hbm_peak": get(detail, "assembly_full_N16384_SEard_d64", "frac_of_hbm_peak"),
        "assembly_SEard_d64_N16384_frac_of_fp64_pipe": get(detail, "assembly_full_N16384_SEard_d64", "frac_of_fp64_pipe"),
        "cholesky_sweep_N16384_ms": get(detail, "cholesky_sweep_N16384", "ms"),
        "cholesky_sweep_N16384_frac_of_peak": get(detail, "cholesky_sweep_N16384", "frac_of_peak"),
        "fit_N16384_RBF_ms": get(detail, "cholesky_sweep_N16384", "fit_ms"),
        # cfg 3 / cfg 5 / cfg 4 / the sharded fit / predict / FITC
        "cfg3_fit_ms": get(out, "cfg3_seard_N16384_d64", "fit_ms"),
        "cfg3_hadamard_reduce_ms": get(out, "cfg3_seard_N16384_d64", "hadamard_reduce_ms"),
        "cfg3_assembly_fused_ms": get(out, "cfg3_seard_N16384_d64", "assembly_fused_ms"),
        "cfg3_cholesky_sweep_frac_of_peak": get(out, "cfg3_seard_N16384_d64", "cholesky_sweep_frac_of_peak"),
        "cfg5_fit_ms": get(out, "cfg5_ep_N4096_d32", "fit_ms"), "cfg5_sweeps": get(out, "cfg5_ep_N4096_d32", "sweeps"),
        "cfg5_site_sweep_ms": get(out, "cfg5_ep_N4096_d32", "site_sweep_ms"),
        "cfg5_final_factor_ms": get(out, "cfg5_ep_N4096_d32", "params_ms"),
        "cfg4_fits_per_s": get(out, "cfg4_restarts_N8192", "fits_per_s"), "cfg4_fits": get(out, "cfg4_restarts_N8192", "fits"),
        "cfg4_wall_s": get(out, "cfg4_restarts_N8192", "wall_s"), "cfg4_n_gpus": get(out, "cfg4_restarts_N8192", "n_gpus"),
        "sharded_fit_n": get(out, "sharded_fit", "n"), "sharded_fit_world": get(out, "sharded_fit", "world"),
        "sharded_fit_seconds": get(out, "sharded_fit", "seconds"),
        "sharded_fit_frac_of_peak_per_gpu": get(out, "sharded_fit", "frac_of_peak_per_gpu"),
        "sharded_fit_peak_bytes_per_rank": get(out, "sharded_fit", "peak_bytes_per_rank"),
        "sharded_fit_wait_share": get(out, "sharded_fit", "wait_share"),
        "sharded_fit_bcast_GBs_per_rank": get(out, "sharded_fit", "bcast_GBs_per_rank"),
        "predict_ns65536_ms": get(out, "predict_N8192_ns65536", "ms"),
        "predict_ns65536_device_ms": get(out, "predict_N8192_ns65536", "device_ms"),
        "fitc_n131072_nu1024_fit_ms": get(out, "fitc_n131072_nu1024", "fit_ms"),
        "kfold_K10_N8192_wall_s": get(out, "kfold_K10_N8192", "wall_s"),
    })
    detail["kernel"] = roof.get("kernel")
    flat = {k: rest.get(k) for k in ROOFLINE_HEAD}
    flat.update({k: v for k, v in rest.items() if k not in flat})
    assert all(not isinstance(v, (dict, list, tuple)) for v in flat.values())
    assert list(flat)[:len(ROOFLINE_HEAD)] == list(ROOFLINE_HEAD)
    return flat, detail


def api_rate(N, d, x, y, steps):
    """fits/s through the drop-in API, the way minimize.run drives it: model.getPosterior() with hyp changing every call
    (hashes x / y for the residency check, builds postStruct / dnlZStruct, keeps post.L as a device handle)."""
    import pygps_amd as pyGPs
    m = pyGPs.GPR()
    m.setPrior(kernel=pyGPs.cov.RBF(np.log(np.sqrt(d)), 0.0))
    m.setNoise(np.log(0.1))
    m.setData(x, y)
    for s in range(2):
        m.getPosterior()
    t = time.perf_counter()
    for s in range(steps):
        hyp, log_sn = hyp_for(s, 0, d)
        m.covfunc.hyp = [float(hyp[0]), float(hyp[1])]
        m.likfunc.hyp = [log_sn]
        m.getPosterior()
    dt = time.perf_counter() - t
    return {"fits_per_s": steps / dt, "ms_per_fit": dt / steps * 1e3, "steps": steps,
            "what": "loop of model.getPosterior() (nlZ, dnlZ, post with device-resident L), one fit stream"}


def cfg4_extra(torch, dist, world, n4=8192):
    """BASELINE configs[3] through the drop-in optimiser: GPR.optimize with ShardedMinimize, 8 restarts x 10 line searches of
    minimize.run at N=8192 d=16, restart r on rank r % world (one broadcast of the start table + data, one all-gather of the
    results: pygps_amd/opt.py).  On one GPU the 8 restarts are dealt to two fit streams; on 8 GPUs it is one restart per
    GPU, one fit stream each.  Collective: every rank calls this."""
    import threading
    import pygps_amd as pyGPs
    d4 = 16
    x4, y4 = synth_reg(n4, d4)
    m4 = pyGPs.GPR()
    m4.setPrior(kernel=pyGPs.cov.RBF(np.log(np.sqrt(d4)), 0.0)); m4.setNoise(np.log(0.1))
    m4.setData(x4, y4)
    m4.setOptimizer("ShardedMinimize", num_restarts=8)
    calls, lock, orig = [0], threading.Lock(), pyGPs.inf.Exact.evaluate

    def counted(self_, *a, **k):                          # count the fits the optimiser asks for (all restart threads)
        with lock:
            calls[0] += 1
        return orig(self_, *a, **k)
    pyGPs.inf.Exact.evaluate = counted
    try:
        np.random.seed(7)
        m4.optimize(x4, y4, numIterations=2)              # builds the fit-stream contexts and their workspaces (one-off cost)
        calls[0] = 0
        np.random.seed(7)
        if dist:
            dist.barrier()
        t = time.perf_counter()
        m4.optimize(x4, y4, numIterations=10)
        t4 = time.perf_counter() - t
    finally:
        pyGPs.inf.Exact.evaluate = orig
    fits = float(calls[0])
    if dist:
        dev = torch.device("cuda", torch.cuda.current_device())
        tt = torch.tensor([t4], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        ft = torch.tensor([fits], dtype=torch.float64, device=dev)
        dist.all_reduce(ft)
        t4, fits = float(tt.item()), float(ft.item())
    runs = m4.optimizer.runs or []
    return {"n_gpus": world, "N": n4, "restarts": 8, "line_searches_per_restart": 10, "wall_s": t4,
            "line_searches_total": int(sum(r.nls for r in runs)), "fits": int(fits), "fits_per_s": fits / t4,
            "nlZ_best": float(m4.nlZ), "fit_streams_per_gpu": min(2, -(-8 // world)),
            "what": "BASELINE configs[3]: GPR.optimize with ShardedMinimize, 8 restarts x 10 line searches of minimize.run at "
                    "N=8192 d=16, restart r on rank r % n_gpus over RCCL; fits = Exact.evaluate calls on all ranks (nlZ + "
                    "gradients each), wall time of the whole optimize() call of a warmed-up model (max over ranks)"}


def kfold_extra(world, n=8192, K=10):
    """The other half of north_star's multi-GPU sentence ("shards independent restarts / CV folds across the 8 GPUs"): the
    reference's K-fold loop (Validation/valid.py:20-66 as Demo/JHUI/demo_Validation.py:70-90 drives it) on the cfg-2 data, fold f on
    rank f % world -- per fold one fit (nlZ + gradients) of N (K-1)/K points and predictions on the held-out N/K; ONE all-gather
    of K records.  Collective: every rank calls this."""
    import pygps_amd as pyGPs
    from pygps_amd import valid
    d = 16
    x, y = synth_reg(n, d)

    def make():
        m = pyGPs.GPR()
        m.setPrior(kernel=pyGPs.cov.RBF(np.log(np.sqrt(d)), 0.0)); m.setNoise(np.log(0.1))
        return m
    valid.sharded_k_fold(make, x, y, K=K)                   # builds the fit-stream contexts (one-off cost)
    t = time.perf_counter()
    res = valid.sharded_k_fold(make, x, y, K=K)
    wall = time.perf_counter() - t
    return {"n_gpus": world, "N": n, "K": K, "wall_s": wall, "folds_per_s": K / wall, "rmse_mean": float(np.mean(res["RMSE"])),
            "nlpd_mean": float(np.mean(res["NLPD"])), "folds_per_rank": np.bincount(res["owner"], minlength=world).tolist(),
            "what": "10-fold validation of GPR + RBF on the cfg-2 data (N=8192 d=16): per fold a fit of 7372-7373 points (nlZ + gradients) "
                    "and predict on 819-820, folds sharded over the ranks (two fit streams per GPU), one all-gather of 10 records"}


def sharded_fit_extra(torch, dist, n, d=16):
    """SURVEY 8(f) row 4, measured: ONE exact-GP fit (RBF, d = 16: assembly, Cholesky + fused inverse, alpha, nlZ, E E' and all
    gradients) spread over ALL ranks -- pgp_sharded_exact_fit (csrc/sharded.hip): 1-D block-cyclic column panels, panel
    broadcasts by RCCL driven from C (no host synchronisation inside the sweep), two small all-reduces.  The same n at every
    world size (a strong-scaling series).  Checked in place: the normal equations (K + sn2 I) alpha = y - m on a sample of
    rows, K rebuilt on the host from the coordinates.  Collective: every rank calls this."""
    import pygps_amd as pyGPs
    from pygps_amd import sharded
    rank, world = dist.get_rank(), dist.get_world_size()
    x, y = synth_reg(n, d, seed=5)
    comm = sharded.Comm()
    m = pyGPs.GPR()
    m.setPrior(kernel=pyGPs.cov.RBF(np.log(np.sqrt(d)), 0.0))
    m.setNoise(np.log(0.1))
    m.setData(x, y)
    m.inffunc = pyGPs.inf.Exact(sharded=comm)
    times, stages = [], None
    for rep in range(2):                                     # the first pass also warms pools, kernels, RCCL
        dist.barrier(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        nlZ, dnlZ, post = m.getPosterior()
        torch.cuda.synchronize(); dist.barrier()
        # wall time of the call (it includes the first-touch allocation of the panel storage: 35 GB per rank at world 1) and the
        # device time of the fit itself (HIP events on the compute stream: first kernel of the assembly to the last all-reduce)
        tt = torch.tensor([time.perf_counter() - t0, 1e-3 * float(m.inffunc.last_ms[3])], dtype=torch.float64, device="cuda")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        times.append((float(tt[0].item()), float(tt[1].item())))
        stages = [float(v) for v in m.inffunc.last_ms]
    wall, dt = times[-1]
    sn2, c = float(np.exp(2 * m.likfunc.hyp[0])), float(m.meanfunc.hyp[0])
    idx = np.arange(0, n, max(1, n // 64))[:64]
    ell2 = float(np.exp(2 * m.covfunc.hyp[0]))
    d2 = ((x[idx, None, :] - x[None, :, :]) ** 2).sum(-1)
    lhs = np.exp(-0.5 * d2 / ell2) @ post.alpha + sn2 * post.alpha[idx]
    res = float(np.abs(lhs - (y[idx] - c)).max() / np.abs(y - c).max())
    w = 1024 if n >= 12288 else 512
    npad = -(-n // w) * w
    sweep_s = stages[1] * 1e-3
    # per-rank device memory (max over ranks) against the panel storage the layout needs, and predict on the distributed posterior
    lb = m.inffunc.last_bytes
    bt = torch.tensor([float(lb["peak_device_bytes"]), float(lb["factor_device_bytes"])], dtype=torch.float64, device="cuda")
    dist.all_reduce(bt, op=dist.ReduceOp.MAX)
    panel_bytes = 2.0 * (npad + 128) * npad / world * 8
    # the multi-rank timers of the library (pgp_sharded_exact_fit timings_out[6..9]), worst rank: how long the compute stream stalled
    # for panels, how long the broadcasts took from enqueue to complete, the rate they moved their bytes at
    lc = getattr(m.inffunc, "last_comm", None) or {}
    ct = torch.tensor([float(lc.get("wait_panel_ms", 0.0)), float(lc.get("bcast_ms", 0.0)), float(lc.get("bcast_max_ms", 0.0))],
                      dtype=torch.float64, device="cuda")
    dist.all_reduce(ct, op=dist.ReduceOp.MAX)
    wait_ms, bcast_ms, bcast_max_ms = (float(v) for v in ct.tolist())
    bcast_bytes = float(lc.get("bcast_bytes", 0.0))
    ns_p = 16384
    xs_p = np.random.RandomState(9).randn(ns_p, d)
    m.predict(xs_p[:1024])
    dist.barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    fm_p = m.predict(xs_p)[2]
    tp = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device="cuda")
    dist.all_reduce(tp, op=dist.ReduceOp.MAX)
    comm.close()
    return {"what": "ONE exact-GP fit (nlZ + all gradients) over all ranks: pgp_sharded_exact_fit, 1-D block-cyclic column panels "
                    "of %d (factor | rhs | fused-inverse rows), depth-1 look-ahead, panel broadcasts by RCCL driven from C, "
                    "every rank accumulates ITS column strips of B^-1 = E E' from the broadcast panels (no N^2 reduction, "
                    "np^2 / (2 world) doubles per rank) and runs the gradient reduce on them" % w,
            "n": n, "d": d, "world": world, "panels": npad // w, "transport": comm.transport,
            "seconds": dt, "seconds_what": "device time of the fit (max over ranks)", "wall_seconds": wall,
            "wall_seconds_first_pass": times[0][0], "stage_ms": dict(zip(("assemble", "sweep_and_EEt", "epilogue", "total"), stages)),
            "flops": float(n) ** 3, "TFLOPs": float(n) ** 3 / dt / 1e12, "TFLOPs_per_gpu": float(n) ** 3 / dt / 1e12 / world,
            "frac_of_peak_per_gpu": float(n) ** 3 / dt / 1e12 / world / PEAK_FP64_MFMA_TF,
            "sweep_frac_of_peak_per_gpu": float(npad) ** 3 / sweep_s / 1e12 / world / PEAK_FP64_MFMA_TF,
            "bytes_broadcast_per_rank": float((npad + 128) * npad * 8) * (world > 1),
            "wait_panel_ms": wait_ms, "wait_share": wait_ms / max(stages[1], 1e-9), "bcast_ms": bcast_ms, "bcast_max_ms": bcast_max_ms,
            "bcast_GBs_per_rank": bcast_bytes / max(bcast_ms, 1e-9) / 1e6 if bcast_ms > 0 else 0.0,
            "bcast_bytes_over_fit_seconds_GBs": float((npad + 128) * npad * 8) * (world > 1) / dt / 1e9,
            "comm_what": "worst rank: ms the compute stream stalled waiting for a panel (sum over panels; wait_share = / sweep ms), ms "
                         "inside the panel broadcasts from enqueue to complete (they overlap compute), bytes / that time",
            "nlZ": float(nlZ), "residual_normal_equations": res,
            "peak_bytes_per_rank": float(bt[0].item()), "factor_bytes_per_rank": float(bt[1].item()),
            "peak_bytes_over_2x_panel_storage": float(bt[0].item()) / panel_bytes,
            "bytes_what": "device bytes one call of pgp_sharded_exact_fit holds at its peak (max over ranks: panels + spare + two "
                          "receive buffers + strips of B^-1 + scratch) / 2 (np + 128) np / world * 8; what the posterior handle keeps",
            "predict_ns16384_ms": float(tp[0].item()) * 1e3, "predict_finite": bool(np.all(np.isfinite(fm_p))),
            "predict_what": "GP.predict of 16384 test points on the distributed posterior (pgp_sharded_predict: V = E' Ks on the "
                            "owners, one all-reduce of ns doubles per batch)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--windows", type=int, default=None,
                    help="the K-step window is timed this many times; value = K / median (default 1: exactly K timed steps; "
                         "5 with --full)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure everything else: single-stream latency, the roofline / kernel-class "
                         "profiled passes, the cfg 3 / cfg 5 / N=16384 / predict / FITC extras, the collective extras and the "
                         "CPU baselines.  --prof-steps, --no-cpu-baseline, --cpu-budget, --no-extras, --collective-extras-only, "
                         "--cfg4-n and --sharded-n act only with --full")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (rank 0) as DIR/alpha.npy (N), DIR/nlZ.npy (1) and "
                         "DIR/dnlZ.npy (mean | cov | lik hypers), float64")
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--prof-steps", type=int, default=6)
    ap.add_argument("--streams", type=int, default=2,
                    help="independent fit streams per GPU (one pgp_ctx + one host thread each); the K timed steps are "
                         "split over them.  2 overlaps one fit's latency-bound panel phases with the other's GEMMs")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-budget", type=float, default=150.0)
    ap.add_argument("--no-extras", action="store_true", help="skip cfg 3 / cfg 5 / N=16384 figures (used by the rocprof passes)")
    ap.add_argument("--option", action="append", default=[], help="library option name=value (experiments)")
    ap.add_argument("--collective-extras-only", action="store_true",
                    help="skip rank 0's single-GPU extras but run the collective ones (cfg 4 over the ranks, one Cholesky over "
                         "the ranks): the 2-rank self-test")
    ap.add_argument("--cfg4-n", type=int, default=8192, help="N of the cfg-4 restart-search extra")
    ap.add_argument("--sharded-n", type=int, default=-1,
                    help="size of the one-Cholesky-over-all-ranks extra (SURVEY 8(f)4); -1 = 65536 (34 GB over the ranks); "
                         "0 = skip")
    args = ap.parse_args()
    if args.windows is None:
        args.windows = 5 if args.full else 1

    # `python3 bench.py --gpus N` with N > 1 and no launcher around it: become the launcher (one rank per GPU under
    # torch.distributed.run, rendezvous on 127.0.0.1) and hand its output through -- rank 0 of the children prints the line
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        import random
        import socket
        import subprocess
        # a rendezvous port BELOW the kernel's ephemeral range: one obtained by bind(0) may be handed to an outgoing connection of
        # another process before the ranks (which first import torch) get to listen on it (EADDRINUSE, seen once in the GPU suite)
        try:
            eph_lo = int(open("/proc/sys/net/ipv4/ip_local_port_range").read().split()[0])
        except Exception:
            eph_lo = 32768
        rnd = random.Random(os.getpid() * 1000003 + time.time_ns())
        port = None
        for _ in range(500):
            cand = rnd.randrange(20000, max(20100, min(eph_lo, 32000) - 32))
            ok = True
            for q in (cand, cand + 17):                       # (+ 17: hostgroup's side channel)
                with socket.socket() as sk:
                    try:
                        sk.bind(("127.0.0.1", q))
                    except OSError:
                        ok = False
            if ok:
                port = cand
                break
        if port is None:
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd))

    # stdout carries exactly ONE line (the JSON).  Native libraries print there too (RCCL writes its version banner to
    # the C stdout when the first communicator is made), so fd 1 is pointed at stderr for the life of the process and
    # the JSON line goes out through a private duplicate of the original stdout.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    import torch
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    # self-test hook only: PYGPS_BENCH_BACKEND=gloo lets N ranks share fewer GPUs (collectives through host memory)
    backend = os.environ.get("PYGPS_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local = local % torch.cuda.device_count()
        os.environ["LOCAL_RANK"] = str(local)              # pygps_amd._lib.default_device() reads it
    torch.cuda.set_device(local)
    cdev = torch.device("cuda", local) if backend == "nccl" else torch.device("cpu")
    # The process group is created at EVERY world size, 1 included: the RCCL broadcast / all-reduce / all-gather below
    # are then the same code on one GPU as on eight.
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    rccl_note = None
    try:
        if backend == "nccl":
            dist.init_process_group(backend="nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", local))              # RCCL (over xGMI for N > 1)
        else:
            dist.init_process_group(backend=backend, rank=rank, world_size=world)
    except Exception as e:
        if world > 1:
            raise
        rccl_note = "process group not available at world size 1: %r" % (e,)
        dist = None
    assert world == args.gpus, "--gpus must equal WORLD_SIZE (launch with torch.distributed.run for N > 1)"

    from pygps_amd import _lib
    lib = _lib.load()
    ctx = _lib.ctx(local)
    N, d = args.n, args.d

    # ---- data: rank 0 generates, RCCL broadcast (configs[3]: "trivial RCCL broadcast/gather") ------
    if rank == 0:
        x, y = synth_reg(N, d)
    else:
        x, y = np.zeros((N, d)), np.zeros((N, 1))
    if dist:
        xt = torch.from_numpy(x).to(cdev)
        yt = torch.from_numpy(y).to(cdev)
        dist.broadcast(xt, src=0)
        dist.broadcast(yt, src=0)
        x, y = xt.cpu().numpy(), yt.cpu().numpy()
    x = np.ascontiguousarray(x)
    yv = np.ascontiguousarray(y).ravel()
    m = np.full(N, yv.mean())
    dm = np.ones((1, N))
    # one context (own HIP streams + workspace) per fit stream; x, y resident in HBM in each
    import ctypes
    import threading
    S = max(1, args.streams)
    ctxs = [ctx]
    for _ in range(1, S):
        h = ctypes.c_void_p()
        _lib.check(lib.pgp_init(local, ctypes.byref(h)), "pgp_init")
        ctxs.append(h)
    for h in ctxs:
        _lib.check(lib.pgp_set_data(h, _lib.ptr(x), N, d, _lib.ptr(yv)))
        for o in args.option:
            k_, v_ = o.split("=")
            _lib.check(lib.pgp_set_option(h, k_.encode(), int(v_)), "pgp_set_option")
    # several fit streams side by side: the schedule ShardedMinimize / sharded_k_fold select for their fit streams
    # (pygps_amd._lib.concurrent_fit_streams: option sched = 1, bit-identical results; an explicit --option sched=... wins)
    sched_multi = S >= 2 and "sched" not in dict(o.split("=") for o in args.option)
    if sched_multi:
        for h in ctxs:
            _lib.check(lib.pgp_set_option(h, b"sched", 1), "pgp_set_option")
    eet_default = int(dict(o.split("=") for o in args.option).get("eet_overlap", 3))
    bufs = [(np.empty(N), np.zeros(1), np.zeros(4)) for _ in range(S)]

    def fit(step, k=0):
        hyp, log_sn = hyp_for(step, rank, d)
        alpha, nlZ, g = bufs[k]
        rc = lib.pgp_exact_fit(ctxs[k], _lib.COV_RBF, _lib.ptr(hyp), 2, 0, 0, log_sn, _lib.ptr(m), _lib.ptr(dm), 1, 3,
                               _lib.ptr(alpha), _lib.ptr(nlZ), _lib.ptr(g), None)
        _lib.check(rc, "pgp_exact_fit")
        return float(nlZ[0])

    def run_steps(first, count):
        """`count` fits, split round-robin over the S fit streams (ctypes releases the GIL during a fit)."""
        res = [None] * count
        if S == 1:
            for s in range(count):
                res[s] = fit(first + s)
            return res

        def work(k):
            for s in range(k, count, S):
                res[s] = fit(first + s, k)
        ths = [threading.Thread(target=work, args=(k,)) for k in range(S)]
        [t.start() for t in ths]
        [t.join() for t in ths]
        return res

    def fence():
        if dist:
            dist.barrier()
        torch.cuda.synchronize()

    run_steps(0, max(args.warmup, S))
    windows, own_windows = [], []
    vals = None
    for wdw in range(max(1, args.windows)):           # EXACTLY K steps per window, barrier + synchronize on both sides
        fence()
        t0 = time.perf_counter()
        vals = run_steps(args.warmup, args.steps)
        fence()
        wt = time.perf_counter() - t0
        own_windows.append(wt)
        if dist:
            tt = torch.tensor([wt], dtype=torch.float64, device=cdev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)                                # slowest rank defines the window
            wt = float(tt.item())
        windows.append(wt)
    dt = float(np.median(windows))
    if rank == 0 and args.dump_outputs:
        # what the caller of the last timed step received: its fit stream's buffers, before a later fit reuses them
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in zip(("alpha", "nlZ", "dnlZ"), bufs[(args.steps - 1) % S]):
            np.save(os.path.join(args.dump_outputs, name + ".npy"), a)
    # every rank's own rate (its median window, before the max over ranks): the 1/2/4/8 table shows stragglers directly
    own = float(np.median(own_windows))
    rank_rates = [args.steps / own]
    if dist:
        rr = torch.tensor([args.steps / own], dtype=torch.float64, device=cdev)
        parts_r = [torch.empty_like(rr) for _ in range(world)]
        dist.all_gather(parts_r, rr)
        rank_rates = [float(p_.item()) for p_ in parts_r]
    if args.full:
        # single-stream latency of one fit in a dependent chain (what cfg 4's one-restart-per-GPU minimize.run sees): the lone-chain schedule
        if sched_multi:
            lib.pgp_set_option(ctxs[0], b"sched", -1)          # the library's default for a lone chain (sched 2 since round 5)
        t1 = time.perf_counter()
        lat_stage = []
        for s in range(6):
            fit(args.warmup + s)
            lat_stage.append(_lib.last_timings(local))
        lat_ms = (time.perf_counter() - t1) / 6 * 1e3
        single_rates = [1e3 / lat_ms]                     # every rank's ONE-chain rate: cfg 4 as written (8 restarts on 8 GPUs) runs one chain per GPU
        if dist:
            sr = torch.tensor([1e3 / lat_ms], dtype=torch.float64, device=cdev)
            parts_s = [torch.empty_like(sr) for _ in range(world)]
            dist.all_gather(parts_s, sr)
            single_rates = [float(p_.item()) for p_ in parts_s]
        # the same with E E^T kept OUT of the sweep (option eet_overlap=0): the stage time of the sweep + fused inverse alone,
        # the figure rounds 1-2 quote as cholesky_sweep_* (2 N^3 / 3 flops); the default schedule folds E E^T into the sweep
        sweep_stage = []
        if lib.pgp_set_option(ctxs[0], b"eet_overlap", 0) == 0:
            for s in range(6):
                fit(args.warmup + s)
                sweep_stage.append(_lib.last_timings(local))
            lib.pgp_set_option(ctxs[0], b"eet_overlap", eet_default)
    if dist:
        res = torch.tensor(vals, dtype=torch.float64, device=cdev)
        parts = [torch.empty_like(res) for _ in range(world)]
        dist.all_gather(parts, res)                                              # RCCL gather of results
        vals_all = torch.stack(parts).cpu().numpy()
        assert np.all(np.isfinite(vals_all)) and vals_all.shape == (world, args.steps)

    # the extra fit-stream contexts of the timed region are done: give their HIP streams back before the extras create
    # their own (beyond four streams of one priority the runtime maps streams onto SHARED hardware queues, and two fit
    # streams that land on one queue serialise: cfg 4 below measured 92 instead of 105 fits/s with them alive)
    for h in ctxs[1:]:
        lib.pgp_destroy(h)
    ctxs = ctxs[:1]
    # ---- roofline of the dominant kernel: single-stream profiled pass over the same steps (HIP events per launch,
    #      recorded on the library's own stream) -------------------------------------------------------------------
    roof = None
    classes = {}
    extra = {}
    if rank == 0 and args.full:
        lib.pgp_profile_reset(ctx)
        lib.pgp_set_profiling(ctx, 1)
        prof_stage = []
        for s in range(args.prof_steps):
            fit(args.warmup + s)
            prof_stage.append(_lib.last_timings(local))
        lib.pgp_set_profiling(ctx, 0)
        prof = _lib.profile(local)
        nfit = float(args.prof_steps)
        gl = gm = gf = 0.0
        for name, v in prof.items():
            if v["launches"]:
                classes[name] = {"launches_per_fit": v["launches"] / nfit, "ms_per_fit": v["ms"] / nfit,
                                 "us_per_launch": v["ms"] / v["launches"] * 1e3,
                                 "executed_TFLOPs": v["flops"] / max(v["ms"], 1e-12) / 1e9 if v["flops"] else None,
                                 "GBs": v["bytes"] / max(v["ms"], 1e-12) / 1e6 if v["bytes"] else None}
            if name.startswith("gemm_f64"):
                gl += v["launches"]; gm += v["ms"]; gf += v["flops"]
        alg = float(N) ** 3                                    # algorithmic flops of one fit that run in gemm_f64_kernel
        achieved_all = alg * nfit / max(gm, 1e-12) / 1e9
        # the dominant kernel = ONE tile code (two rows of the rocprofv3 kernel-stats CSV since round 4: gemm_f64_kernel<128,128,false,false,
        # true,true> and gemm_f64_pair_kernel<true>, the same gemm_tile behind a second entry point): the LDS-DMA 128 x 128 tile
        # kernel that runs every trailing update and E E^T product.  Its algorithmic flops: N^3 per fit minus everything
        # the OTHER gemm_f64 instantiations execute (panel solves, 64-tile updates of the leaf chain; executed >= algorithmic
        # there, so this is a lower bound)
        kd = next((v for k_, v in prof.items() if k_.startswith("kernel gemm_f64_kernel<128,128,false,false,true")), None)
        if kd and kd["launches"]:
            alg_dom = alg * nfit - (gf - kd["flops"])
            dom_ms, dom_l = kd["ms"], kd["launches"]
        else:
            alg_dom, dom_ms, dom_l = alg * nfit, gm, gl
        achieved = alg_dom / max(dom_ms, 1e-12) / 1e9
        # stage time of the UN-profiled single-stream fits (the per-launch HIP events of the profiled pass stretch the chain)
        potrf_ms = float(np.median([t["potrf"] for t in (sweep_stage or lat_stage)]))
        fact_ms = float(np.median([t["potrf"] + t["solve"] + t["trtri"] + t["lauum"] for t in lat_stage]))
        traffic, tsrc = None, None
        import glob
        import hashlib
        cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_gemm_f64_hbm_traffic.json")))
        if cands:            # the newest tracked PMC measurement -- only if it was taken on THIS kernel (fingerprint of its sources)
            try:
                tj = json.load(open(cands[-1]))
                hh = hashlib.sha256()
                for fsrc in ("gemm_f64.hip", "gemm_tile.h", "common.h"):
                    hh.update(open(os.path.join(ROOT, "pygps_amd", "csrc", fsrc), "rb").read())
                cur = hh.hexdigest()[:16]
                if tj.get("kernel_source_sha16") == cur:
                    traffic = tj.get("bytes_per_launch")
                    tsrc = ("profiles/%s: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes (separate runs) of this command line, measured on "
                            "commit %s, kernel sources %s = the ones of this run -- a static file, not re-measured in this run"
                            % (os.path.basename(cands[-1]), tj.get("measured_on_commit"), cur))
                else:
                    tsrc = ("STALE: profiles/%s was measured on kernel sources %s (commit %s), this run's gemm_f64 sources are %s -- "
                            "traffic withheld; re-run tools/make_profiles.sh" % (os.path.basename(cands[-1]), tj.get("kernel_source_sha16"),
                                                                              tj.get("measured_on_commit"), cur))
            except Exception as e:
                tsrc = "traffic file unreadable: %r" % (e,)
        roof = {"kernel": "gemm_f64_kernel<128,128,false,false,true,true> + gemm_f64_pair_kernel<true>: ONE tile code (gemm_tile<128,128>, fp64 MFMA, "
                          "LDS-DMA operand staging, yield poll) behind two entry points -- one product per launch, or the trailing update "
                          "TU_b(p) and panel p's share of E E^T in one launch; every trailing update of the Cholesky sweep incl. the fused "
                          "inverse, and the E E^T products; in a rocprofv3 kernel-stats CSV: the sum of these two rows",
                "bound": "mfma", "achieved": achieved, "peak": PEAK_FP64_MFMA_TF, "unit": "TFLOP/s",
                "frac": achieved / PEAK_FP64_MFMA_TF, "traffic": traffic, "traffic_source": tsrc,
                "how": "algorithmic flops of this instantiation's launches (N^3 per fit minus what the other gemm_f64 "
                       "instantiations execute) / summed HIP-event durations of its launches, %d single-stream fits" % args.prof_steps,
                "launches_per_fit": dom_l / nfit, "flops_per_launch": alg_dom / max(dom_l, 1), "avg_launch_ms": dom_ms / max(dom_l, 1),
                "algorithmic_flops_per_fit": alg_dom / nfit,
                "all_gemm_f64_instantiations": {
                    "achieved": achieved_all, "frac": achieved_all / PEAK_FP64_MFMA_TF, "launches_per_fit": gl / nfit,
                    "avg_launch_ms": gm / max(gl, 1),
                    "what": "rounds 1-2 definition: N^3 per fit / summed durations of EVERY gemm_f64 launch, the 64-tile "
                            "updates of the latency-bound leaf chain included (their event durations overlap the bulk kernels)"},
                "executed_over_algorithmic_flops": gf / (alg * nfit),
                "timed_window": {"streams": S, "TFLOPs_end_to_end": alg / (dt / args.steps) / 1e12,
                                 "frac_of_peak": alg / (dt / args.steps) / 1e12 / PEAK_FP64_MFMA_TF,
                                 "what": "N^3 x K fits / window time: every kernel and every gap of the timed region included"},
                # the Cholesky sweep also produces L^-T (fused triangular inverse): 2 N^3 / 3 algorithmic flops in that stage
                "factor_inverse_EEt": {"ms": fact_ms, "TFLOPs": alg / (fact_ms * 1e-3) / 1e12,
                                       "frac_of_peak": alg / (fact_ms * 1e-3) / 1e12 / PEAK_FP64_MFMA_TF,
                                       "what": "default schedule, one fit stream: Cholesky sweep + fused inverse + E E^T (accumulated "
                                               "panel by panel under the sweep; the last product overlaps the O(N^2) alpha / log det "
                                               "kernels) = N^3 flops / (potrf + solve + lauum stage times)"},
                "cholesky_sweep_what": "sweep + fused inverse alone (2 N^3 / 3 flops), 6 single-stream fits with option eet_overlap=0",
                "cholesky_sweep_ms": potrf_ms,
                "cholesky_sweep_TFLOPs": (2.0 * N ** 3 / 3.0) / (potrf_ms * 1e-3) / 1e12,
                "cholesky_sweep_frac_of_peak": (2.0 * N ** 3 / 3.0) / (potrf_ms * 1e-3) / 1e12 / PEAK_FP64_MFMA_TF}
        # the same profiled pass under the round 2-4 schedule (sched 0: TU_a as ONE 254-tile launch alone on the chip).  The default since
        # round 5 (sched 2) moves the diagonal-block piece of TU_a to the panel stream and lets D(p+1)'s first kernels run beside the
        # rectangle that is left: the fit is faster (single_stream_ms_per_fit), but that rectangle's launch of THIS kernel lasts ~100 us
        # instead of ~77 (its CUs' workgroups give way to the chain), which lowers `frac` -- both are in the line so that the kernel's
        # own rate is not confused with the schedule's
        try:
            if lib.pgp_set_option(ctx, b"sched", 0) == 0:
                lib.pgp_profile_reset(ctx)
                t0s = time.perf_counter()
                for s_ in range(4):
                    fit(args.warmup + s_)
                s0_ms = (time.perf_counter() - t0s) / 4 * 1e3
                lib.pgp_set_profiling(ctx, 1)
                for s_ in range(args.prof_steps):
                    fit(args.warmup + s_)
                lib.pgp_set_profiling(ctx, 0)
                prof0 = _lib.profile(local)
                kd0 = next((v for k_, v in prof0.items() if k_.startswith("kernel gemm_f64_kernel<128,128,false,false,true")), None)
                gf0 = sum(v["flops"] for k_, v in prof0.items() if k_.startswith("gemm_f64"))
                if kd0 and kd0["launches"]:
                    ach0 = (alg * nfit - (gf0 - kd0["flops"])) / max(kd0["ms"], 1e-12) / 1e9
                    roof["frac_sched0"] = ach0 / PEAK_FP64_MFMA_TF
                    roof["avg_launch_ms_sched0"] = kd0["ms"] / kd0["launches"]
                    roof["single_stream_ms_per_fit_sched0"] = s0_ms
        finally:
            lib.pgp_set_option(ctx, b"sched", int(dict(o.split("=") for o in args.option).get("sched", -1)))
            lib.pgp_profile_reset(ctx)
        asm = prof.get("cov_tile_kernel(assemble)")
        if asm and asm["launches"]:
            roof["assembly_fused_GBs"] = asm["bytes"] / asm["ms"] / 1e6
            roof["assembly_fused_frac_of_hbm_peak"] = asm["bytes"] / asm["ms"] / 1e6 / PEAK_HBM_GBS
        if not args.no_extras and not args.collective_extras_only:
            try:
                extra = extras(lib, _lib, local, d, roof)
            except Exception as e:         # pragma: no cover
                extra = {"error": repr(e)}
            try:
                extra["api"] = api_rate(N, d, x, y, 20)
            except Exception as e:         # pragma: no cover
                extra["api"] = {"error": repr(e)}

    if rank == 0:
        total_fits = world * args.steps
        out = {
            "metric": "GP fits/sec (nlZ+grad, RBF, N=%d d=%d)" % (N, d),
            "value": total_fits / dt, "unit": "fits/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": "GPR+RBF, N=%d d=%d fp64 synthetic (SURVEY 8d recipe, seed 0), infExact nlZ + dnlZ "
                                   "(BASELINE configs[1]); x,y resident in HBM, hyp changes every step; outputs "
                                   "nlZ, dnlZ(4), alpha(N) to host per step" % (N, d),
                       "fits_per_rank": args.steps, "fit_streams_per_gpu": S, "sched": 1 if sched_multi else int(dict(o.split("=") for o in args.option).get("sched", 2)),
                       "parallelism": "independent fits (restart evaluations) per GPU, %d concurrent fit streams per "
                                      "GPU; RCCL broadcast + all-reduce(max) + all-gather only%s"
                                      % (S, "" if dist else " (no process group at world size 1)")},
            "per_rank_fits_per_s": rank_rates, "per_gpu_fits_per_s": (total_fits / dt) / world,
            "timed_windows_s": windows, "window_spread": (max(windows) - min(windows)) / dt,
            "flops_per_fit": float(N) ** 3,
            "fit_TFLOPs": float(N) ** 3 / (dt / args.steps) / 1e12,
            "device": _lib.device_info(local),
        }
        if args.full:
            out.update({"single_stream_ms_per_fit": lat_ms, "single_stream_fits_per_s": 1e3 / lat_ms,
                        "stage_ms_single_stream_median": {k: float(np.median([t[k] for t in lat_stage])) for k in lat_stage[0]},
                        "roofline": roof, "kernel_classes": classes})
        if rccl_note:
            out["rccl_note"] = rccl_note
        out.update({k: v for k, v in extra.items() if k != "api"})
        if "api" in extra:
            out["api_fits_per_s"] = extra["api"].get("fits_per_s")
            out["api"] = extra["api"]
    # ---- collective extras, after the timed region and outside `value`: BASELINE configs[3] through the drop-in optimiser
    #      (restarts sharded over the ranks) and SURVEY 8(f) row 4 (one factorisation over ALL ranks).  A watchdog keeps
    #      the contract if the collective path stalls on a node this code has never run on: the JSON line goes out without
    #      the figures and the process leaves.
    sn = args.sharded_n if args.sharded_n >= 0 else 65536     # the same size at every world size: a strong-scaling series
    if args.full and dist and not args.no_extras:
        dist.barrier()                                       # rank 0 arrives after its single-GPU extras; the clock starts here
        partial = {}

        def bail():                                          # pragma: no cover
            if rank == 0:
                out.update(partial)
                out["collective_extras_error"] = "no result within 300 s (world %d)" % world
                out["collective_extras_ok"] = False
                os.write(json_fd, (json.dumps(out) + "\n").encode())
            os._exit(0)
        dog = threading.Timer(300.0, bail)
        dog.daemon = True
        dog.start()
        try:
            partial["cfg4_restarts_N8192"] = cfg4_extra(torch, dist, world, args.cfg4_n)
        except Exception as e:                               # pragma: no cover
            partial["cfg4_restarts_N8192"] = {"error": repr(e), "n_gpus": world}
        try:
            partial["kfold_K10_N8192"] = kfold_extra(world, args.cfg4_n)
        except Exception as e:                               # pragma: no cover
            partial["kfold_K10_N8192"] = {"error": repr(e), "n_gpus": world}
        if sn > 0:
            try:
                partial["sharded_fit"] = sharded_fit_extra(torch, dist, sn)
            except Exception as e:                           # pragma: no cover
                partial["sharded_fit"] = {"error": repr(e), "n": sn, "world": world}
        dog.cancel()
        if rank == 0:
            out.update(partial)
            out["collective_extras_ok"] = all("error" not in v for v in partial.values())
    if rank == 0:
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(N, d, args.cpu_budget)
            out["gpu_over_cpu"] = out["value"] / out["cpu_baseline"]["value"]
            if not args.no_extras:
                others = cpu_baseline_other_configs(out["cpu_baseline"]["value"])
                out["cpu_baseline"]["other_configs"] = others
                for key, cfg in (("cfg3_seard_N16384_d64", "cfg3"), ("cfg5_ep_N4096_d32", "cfg5"), ("cfg4_restarts_N8192", "cfg4")):
                    if isinstance(out.get(key), dict) and cfg in others:
                        out[key]["cpu_baseline"] = others[cfg]
        # The driver's parser keeps the contract keys, `config`, `cpu_baseline` and the SCALAR members of `roofline` (nested
        # objects are dropped): every north-star figure rides in `roofline` as a flat scalar, the nested detail objects move to
        # `roofline_detail` at top level, strings are cut to 120 characters (the full texts stay in `roofline_detail`).
        if out.get("roofline") is not None:
            out["single_stream_fits_per_s_per_rank"] = single_rates
            out["cfg4_as_written_fits_per_s"] = float(sum(single_rates))
            out["cfg4_as_written_fits_per_s_per_gpu"] = float(sum(single_rates)) / world
            out["roofline"], out["roofline_detail"] = flatten_roofline(out)
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    if dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
