#!/usr/bin/env python3
"""GPC + Laplace fit times (nargout = 3) on the synthetic classification recipe of the G20 fixtures (d = 32, RBF(log sqrt d, 0),
Zero mean), next to EP on the same data.  Per size: warm-up, then the best of several calls; ms per fit, Newton steps, ms per
step and the share of the Newton loop spent in the Cholesky factorisations of B (pgp_last_timings: 'solve' = the Newton loop,
'potrf' = its factorisations, event-timed).

    python tools/laplace_time.py [N ...]        (default 4096 8192)
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import pygps_amd as pyGPs  # noqa: E402
from pygps_amd import _lib  # noqa: E402


def synth_cls(N, d, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.randn(N, d)
    w = rng.randn(d, 1)
    y = np.sign(x @ w / np.sqrt(d) + 0.3 * rng.randn(N, 1))
    y[y == 0] = 1
    return x, y


def best(model, x, y, reps):
    ts, tm = [], None
    for _ in range(reps):
        model.inffunc = type(model.inffunc)()                   # cold start every call (no warm-start state)
        t0 = time.perf_counter()
        model.inffunc.evaluate(model.meanfunc, model.covfunc, model.likfunc, x, y, 3)
        ts.append((time.perf_counter() - t0) * 1e3)
        if ts[-1] == min(ts):
            tm = (_lib.last_timings(), getattr(model.inffunc, "newton_steps", None), getattr(model.inffunc, "sweeps", None))
    return min(ts), tm


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [4096, 8192]
    d = 32
    for N in sizes:
        x, y = synth_cls(N, d)
        reps = 5 if N <= 4096 else 3
        for name in ("Laplace", "EP"):
            m = pyGPs.GPC()
            m.useInference(name)
            m.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(np.log(np.sqrt(d)), 0.0))
            m.setData(x, y)
            best(m, m.x, m.y, 1)                                # warm-up (code objects, pools)
            ms, (tim, steps, sweeps) = best(m, m.x, m.y, reps)
            if name == "Laplace":
                loop, fac = tim["solve"], tim["potrf"]
                print("N=%5d Laplace: %8.2f ms/fit  Newton steps %d  %6.2f ms/step  factorisation %.1f %% of the Newton loop "
                      "(loop %.2f ms, start %.2f ms, posterior + gradients %.2f ms)"
                      % (N, ms, steps, loop / max(steps, 1), 100.0 * fac / max(loop, 1e-9), loop, tim["assemble"], tim["grad"]),
                      flush=True)
            else:
                print("N=%5d EP:      %8.2f ms/fit  sweeps %d" % (N, ms, sweeps), flush=True)


if __name__ == "__main__":
    main()
