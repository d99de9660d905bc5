#!/usr/bin/env python3
"""Exact GPR fits with gradients (nargout = 3) under the spectral mixture kernel cov.SM next to the same fit under cov.RBF, same
N, same process, alternated over several rounds: the `assemble` and `grad` stages of _lib.last_timings() (the two stages that run
SM's own kernels: cov_tile_kernel<.., CovSM, ..> and hadamard_sm_kernel) and the remaining stages, which run the same code for
both kernels and should agree within noise -- the sanity check of the comparison.  Inputs: x uniform in [0, 4]^D scaled so that N
points keep unit spacing on average in D = 1, two sinusoids plus noise; SM hypers drawn once per configuration.

    python tools/sm_time.py [N] [D:Q ...]          (default 8192 1:1 1:4 1:10 4:4)
    python tools/sm_time.py cpu [N] [Q]            (default 2048 3: the CPU baseline, no GPU needed)
    rocprofv3 --kernel-trace --stats -d OUT -o sm -- python tools/sm_time.py 8192 1:10

`cpu` times a numpy restatement of what the reference does per fit with gradients at D = 1 (Core/cov.py:521-619 SM.getCovMatrix,
Core/inf.py:353-384 Exact: K, Cholesky, alpha, then ONE n x n derivative matrix and one Hadamard sum per hyper) on the host
cores of the box it runs on, as BASELINE.md does for the other configurations (reference source never travels to the GPU box).
It is leaner than the reference (no cdist, components reused across the derivative matrices): a lower bound for the reference's
time, not the reference's time (DESIGN.md has both on one host).
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

OTHER = ("potrf", "solve", "trtri", "lauum")


def data(n, D, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.rand(n, D) * (n / 100.0 if D == 1 else 4.0)
    y = np.sin(2 * np.pi * 0.4 * x[:, [0]]) + 0.5 * np.cos(2 * np.pi * 1.1 * x[:, [-1]]) + 0.1 * rng.randn(n, 1)
    return x, y


def sm_hyp(Q, D, seed=1):
    rng = np.random.RandomState(seed)
    return [float(v) for v in np.concatenate([np.log(rng.uniform(0.2, 0.6, Q)), np.log(rng.uniform(0.1, 0.9, D * Q)),
                                              np.log(rng.uniform(0.02, 0.1, D * Q))])]


def gpu(n, configs, rounds=5):
    import pygps_amd as pyGPs
    from pygps_amd import _lib
    for D, Q in configs:
        x, y = data(n, D)
        models = {}
        for name, k in (("SM", pyGPs.cov.SM(Q, sm_hyp(Q, D))), ("RBF", pyGPs.cov.RBF(0.0, 0.0))):
            m = pyGPs.GPR()
            m.setPrior(mean=pyGPs.mean.Zero(), kernel=k)
            m.setNoise(np.log(0.1))
            m.setData(x, y)
            m.getPosterior()                                # warm-up (code objects, pools)
            models[name] = m
        rows = {"SM": [], "RBF": []}
        for _ in range(rounds):
            for name in ("SM", "RBF"):
                t0 = time.perf_counter()
                models[name].getPosterior()
                wall = (time.perf_counter() - t0) * 1e3
                t = _lib.last_timings()
                rows[name].append((t["assemble"], t["grad"], sum(t[s] for s in OTHER), t["total"], wall))
        for name in ("SM", "RBF"):
            a = np.array(rows[name])
            lo, md = a.min(axis=0), np.median(a, axis=0)
            print("N=%d D=%d Q=%2d %-3s  assemble %8.3f (med %8.3f)  grad %8.3f (med %8.3f)  other stages %8.3f (med %8.3f)  "
                  "total %8.3f  wall %8.3f ms" % (n, D, Q if name == "SM" else 0, name, lo[0], md[0], lo[1], md[1], lo[2], md[2],
                                                  lo[3], lo[4]), flush=True)


def cpu(n, Q, reps=3):
    import scipy.linalg as sla
    x, y = data(n, 1)
    h = np.array(sm_hyp(Q, 1))
    sn2 = 0.01
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        w, m, v = np.exp(h[:Q]), np.exp(h[Q:2 * Q]), np.exp(2 * h[2 * Q:])
        d2 = (x - x.T) ** 2
        d = np.sqrt(d2)
        comp = [w[q] * np.exp(-2 * np.pi ** 2 * d2 * v[q]) * np.cos(2 * np.pi * d * m[q]) for q in range(Q)]
        K = sum(comp)
        L = sla.cholesky(K / sn2 + np.eye(n), lower=False)
        alpha = sla.cho_solve((L, False), y) / sn2
        nlZ = (y.T @ alpha).item() / 2 + np.log(np.diag(L)).sum() + n * np.log(2 * np.pi * sn2) / 2
        Qm = sla.cho_solve((L, False), np.eye(n)) / sn2 - alpha @ alpha.T
        g = []
        for q in range(Q):                                  # one derivative matrix and one Hadamard sum per hyper, as the reference
            g.append((Qm * comp[q]).sum() / 2)
        for q in range(Q):
            a = 2 * np.pi * d * m[q]
            g.append((Qm * (-a * np.tan(a) * comp[q])).sum() / 2)
        for q in range(Q):
            g.append((Qm * (-(2 * np.pi) ** 2 * d2 * v[q] * comp[q])).sum() / 2)
        ts.append((time.perf_counter() - t0) * 1e3)
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    print("CPU restatement N=%d D=1 Q=%d: %.1f ms per fit with gradients (best of %d; %s host cores visible, BLAS threads %s), "
          "nlZ %.6g" % (n, Q, min(ts), reps, ncpu, os.environ.get("OMP_NUM_THREADS", "default"), nlZ), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "cpu":
        cpu(int(args[1]) if len(args) > 1 else 2048, int(args[2]) if len(args) > 2 else 3)
        return
    n = int(args[0]) if args else 8192
    configs = [tuple(int(v) for v in a.split(":")) for a in args[1:]] or [(1, 1), (1, 4), (1, 10), (4, 4)]
    gpu(n, configs)


if __name__ == "__main__":
    main()
