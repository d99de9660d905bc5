#!/usr/bin/env python3
"""GPR + lik.Laplace (EP) fit times (nargout = 3, cold start) next to GPC + lik.Erf (EP) at the same size: d = 32,
RBF(log sqrt d, 0), Zero mean; regression targets with Student-t noise for Laplace, their signs for Erf.  Then the FITC
pair: GPR_FITC + lik.Laplace (FITC_EP) next to GPC_FITC + lik.Erf (FITC_EP), d = 8, nu inducing points drawn from the data.
Per size: warm-up, then the best of several calls; ms per fit, sweeps and ms per sweep.  What the heavier moments cost per
site in the single-workgroup chains (ep_chain_kernel, fitc_ep_chain_kernel) comes from a kernel trace of the same run:

    python tools/lik_laplace_time.py [n ...] [fitc n:nu ...]     (default 4096 fitc 65536:512)
    rocprofv3 --kernel-trace --stats -d OUT -o lik_laplace -- python tools/lik_laplace_time.py 4096 fitc 65536:512
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import pygps_amd as pyGPs  # noqa: E402


def best(model, reps):
    ts, sweeps = [], None
    for _ in range(reps):
        model.inffunc = type(model.inffunc)()                   # cold start every call (no warm-start state)
        t0 = time.perf_counter()
        model.inffunc.evaluate(model.meanfunc, model.covfunc, model.likfunc, model.x, model.y, 3)
        ts.append((time.perf_counter() - t0) * 1e3)
        sweeps = model.inffunc.sweeps
    return min(ts), sweeps


def main():
    args = sys.argv[1:] or ["4096", "fitc", "65536:512"]
    k = args.index("fitc") if "fitc" in args else len(args)
    sizes = [int(a) for a in args[:k]]
    fitc_sizes = [tuple(int(v) for v in a.split(":")) for a in args[k + 1:]]
    d = 32
    for n in sizes:
        rng = np.random.RandomState(0)
        x = rng.randn(n, d)
        w = rng.randn(d, 1)
        f = np.sin(x @ w / np.sqrt(d))
        y = f + 0.1 * rng.standard_t(3, size=(n, 1))
        out = []
        for name, yy in (("Laplace", y), ("Erf", np.where(f + 0.3 * rng.randn(n, 1) >= 0, 1.0, -1.0))):
            m = pyGPs.GPR() if name == "Laplace" else pyGPs.GPC()
            if name == "Laplace":
                m.useLikelihood("Laplace")
            m.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(np.log(np.sqrt(d)), 0.0))
            m.setData(x, yy)
            best(m, 1)                                          # warm-up (code objects, pools)
            out.append(best(m, 5))
        (ms, sw), (ms_e, sw_e) = out
        print("n=%6d d=%d  EP+Laplace: %8.2f ms/fit  sweeps %d  %7.2f ms/sweep   EP+Erf: %8.2f ms/fit  sweeps %d  %7.2f ms/sweep"
              % (n, d, ms, sw, ms / max(sw, 1), ms_e, sw_e, ms_e / max(sw_e, 1)), flush=True)
    d = 8
    for n, nu in fitc_sizes:
        rng = np.random.RandomState(0)
        x = rng.randn(n, d)
        f = np.sin(x @ rng.randn(d, 1) / np.sqrt(d))
        u = x[np.random.RandomState(1).choice(n, nu, replace=False)]
        out = []
        for name, yy in (("Laplace", f + 0.1 * rng.standard_t(3, size=(n, 1))), ("Erf", np.where(f >= 0, 1.0, -1.0))):
            m = pyGPs.GPR_FITC() if name == "Laplace" else pyGPs.GPC_FITC()
            if name == "Laplace":
                m.useLikelihood("Laplace")
            m.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(np.log(np.sqrt(d)), 0.0), inducing_points=u)
            m.setData(x, yy)
            best(m, 1)
            out.append(best(m, 3))
        (ms, sw), (ms_e, sw_e) = out
        print("n=%6d nu=%4d d=%d  FITC_EP+Laplace: %8.2f ms/fit  sweeps %d  %7.2f ms/sweep   FITC_EP+Erf: %8.2f ms/fit  sweeps %d  "
              "%7.2f ms/sweep" % (n, nu, d, ms, sw, ms / max(sw, 1), ms_e, sw_e, ms_e / max(sw_e, 1)), flush=True)


if __name__ == "__main__":
    main()
