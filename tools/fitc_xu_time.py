"""What learning the inducing inputs costs: one GPR_FITC fit with gradients, flag off (the code path before the gradient w.r.t. xu
existed) against flag on, alternated in one process, and the two contraction passes alone (the library's profile class "hadamard_reduce_kernel",
which no other kernel of a FITC fit uses) with the bytes of the adjoint G they read per second against the HBM peak.

    python tools/fitc_xu_time.py [--reps 9] [--out profiles/fitc_xu_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pygps_amd as pyGPs                                            # noqa: E402
from pygps_amd import _lib                                           # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s, HBM3E of the MI355X (spec; a float4 copy reaches 6.3e12)
CASES = ((65536, 512, 8, "RBF"), (65536, 512, 8, "RBFard"), (8192, 256, 8, "RBF"), (8192, 256, 8, "RBFard"))


def model(n, nu, d, kind, learn):
    rng = np.random.RandomState(0)
    x = rng.randn(n, d)
    w = rng.randn(d, 1)
    y = np.sin(x @ w / np.sqrt(d)) + 0.1 * rng.randn(n, 1)
    u = x[rng.choice(n, nu, replace=False)] + 0.01 * rng.randn(nu, d)
    ell = float(np.log(np.sqrt(d)))
    k = pyGPs.cov.RBF(ell, 0.0) if kind == "RBF" else pyGPs.cov.RBFard(log_ell_list=[ell] * d, log_sigma=0.0)
    m = pyGPs.GPR_FITC()
    m.setPrior(mean=pyGPs.mean.Zero(), kernel=k, inducing_points=u)
    m.setNoise(np.log(0.1))
    m.learnInducing(learn)
    return m, x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["fitc_xu_time: %s, %s (python tools/fitc_xu_time.py --reps %d)" % (time.strftime("%Y-%m-%d"),
                                                                                _lib.device_info()["name"] or "MI355X", a.reps),
             "one GPR_FITC fit with all gradients, host clock around the synchronous call, median of %d alternated repeats" % a.reps]
    dll, ctx = _lib.load(), _lib.ctx()
    for n, nu, d, kind in CASES:
        off, x, y = model(n, nu, d, kind, False)
        on, _, _ = model(n, nu, d, kind, True)
        for m in (off, on, off, on):                                 # warm-up: code objects, pools, the resident data
            m.getPosterior(x, y)
        t = {False: [], True: []}
        for _ in range(a.reps):
            for flag, m in ((False, off), (True, on)):
                t0 = time.perf_counter()
                m.getPosterior(x, y)
                t[flag].append(time.perf_counter() - t0)
        t_off, t_on = float(np.median(t[False])), float(np.median(t[True]))
        _lib.check(dll.pgp_set_profiling(ctx, 1))
        _lib.check(dll.pgp_profile_reset(ctx))
        for _ in range(a.reps):
            on.getPosterior(x, y)
        p = _lib.profile()["hadamard_reduce_kernel"]
        dll.pgp_set_profiling(ctx, 0)
        ms = p["ms"] / a.reps
        gbytes = 8.0 * nu * n * ((d + 7) // 8)
        lines.append("n=%d nu=%d D=%d %s: flag off %.2f ms (min %.2f), flag on %.2f ms (min %.2f), ratio %.3f; contraction passes "
                     "%.3f ms, G read at %.2f TB/s = %.0f %% of the %.1f TB/s HBM peak"
                     % (n, nu, d, kind, t_off * 1e3, min(t[False]) * 1e3, t_on * 1e3, min(t[True]) * 1e3, t_on / t_off, ms,
                        gbytes / (ms * 1e-3) / 1e12, 100 * gbytes / (ms * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
