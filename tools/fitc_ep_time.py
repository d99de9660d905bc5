#!/usr/bin/env python3
"""GPC_FITC + FITC_EP fit times (nargout = 3, cold start) on the synthetic classification recipe of the G21 fixtures
(d = 8, RBF(log sqrt d, 0), Zero mean, nu inducing points drawn from the data), next to FITC_Exact (GPR_FITC, noise 0.1)
on the same inputs.  Per size: warm-up, then the best of several calls; ms per fit, sweeps and ms per sweep.  The split of a
sweep into chain (fitc_ep_chain_kernel), fold and refresh comes from a kernel trace of the same run:

    python tools/fitc_ep_time.py [n:nu ...]        (default 16384:256 65536:512 131072:1024)
    rocprofv3 --kernel-trace --stats -d OUT -o fitc_ep -- python tools/fitc_ep_time.py 65536:512
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import pygps_amd as pyGPs  # noqa: E402


def synth_cls(N, d, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.randn(N, d)
    w = rng.randn(d, 1)
    y = np.sign(x @ w / np.sqrt(d) + 0.3 * rng.randn(N, 1))
    y[y == 0] = 1
    return x, y


def best(model, reps):
    ts, sweeps = [], None
    for _ in range(reps):
        model.inffunc = type(model.inffunc)()                   # cold start every call (no warm-start state)
        t0 = time.perf_counter()
        model.inffunc.evaluate(model.meanfunc, model.covfunc, model.likfunc, model.x, model.y, 3)
        ts.append((time.perf_counter() - t0) * 1e3)
        sweeps = getattr(model.inffunc, "sweeps", None)
    return min(ts), sweeps


def main():
    sizes = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:]] or [(16384, 256), (65536, 512), (131072, 1024)]
    d = 8
    for n, nu in sizes:
        x, y = synth_cls(n, d)
        u = x[np.random.RandomState(1).choice(n, nu, replace=False)]
        reps = 3 if n <= 65536 else 2
        m = pyGPs.GPC_FITC()
        m.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(np.log(np.sqrt(d)), 0.0), inducing_points=u)
        m.setData(x, y)
        best(m, 1)                                              # warm-up (code objects, pools)
        ms, sweeps = best(m, reps)
        r = pyGPs.GPR_FITC()
        r.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(np.log(np.sqrt(d)), 0.0), inducing_points=u)
        r.setNoise(np.log(0.1))
        r.setData(x, y)
        best(r, 1)
        ms_exact, _ = best(r, reps)
        print("n=%6d nu=%4d FITC_EP: %9.2f ms/fit  sweeps %d  %8.2f ms/sweep   FITC_Exact: %8.2f ms/fit"
              % (n, nu, ms, sweeps, ms / max(sweeps, 1), ms_exact), flush=True)


if __name__ == "__main__":
    main()
