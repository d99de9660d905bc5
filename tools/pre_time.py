#!/usr/bin/env python3
"""Exact GPR fits with gradients (nargout = 3) at N training points, per-fit time of

    rbf      GPR + RBF                               (the plain hot path, for scale)
    program  GPR + (Pre * s + RBF), Pre a resident leaf of the device program: M2 is uploaded once and read by the
             assembly and the gradient tile kernels on every fit
    dense    the same model with cov.Pre.device_leaf = False: K and every derivative matrix are built on the host
             and cross PCIe on every fit (three derivative matrices + K = four n^2 uploads per evaluation)

    python tools/pre_time.py [N]            (default 8192) runs the three steps one after the other, each in a child
                                            process of its own under a time limit; the first failure ends the run
    python tools/pre_time.py step NAME N    one step in this process

M2 is a synthetic SPD matrix (a squared-exponential kernel of random 2-d points, scaled by 0.5): the timing does not
depend on what the matrix holds.  Prints best and median wall time per fit over `rounds` fits after a warm-up, and the
`assemble` / `grad` / `total` device stages of _lib.last_timings() for the two device-program steps."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

LIMIT = {"rbf": 300, "program": 420, "dense": 900}        # seconds per step


def data(n, d=8, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.randn(n, d)
    y = np.sin(x.sum(axis=1, keepdims=True) / np.sqrt(d)) + 0.1 * rng.randn(n, 1)
    u = rng.rand(n, 2) * np.sqrt(n) / 8.0
    sq = (u * u).sum(axis=1)
    M2 = 0.5 * np.exp(-0.5 * np.maximum(sq[:, None] + sq[None, :] - 2.0 * (u @ u.T), 0.0))
    M2 = 0.5 * (M2 + M2.T)
    return x, y, M2


def step(name, n, rounds=7):
    import pygps_amd as pyGPs
    from pygps_amd import _lib
    cov = pyGPs.cov
    x, y, M2 = data(n)
    if name == "rbf":
        k = cov.RBF(np.log(2.0), 0.0)
    else:
        k = cov.Pre(None, M2) * -0.5 + cov.RBF(np.log(2.0), 0.0)
        if name == "dense":
            cov.Pre.device_leaf = False
            rounds = 3
    m = pyGPs.GPR()
    m.setPrior(mean=pyGPs.mean.Zero(), kernel=k)
    m.setNoise(np.log(0.1))
    m.setData(x, y)
    nlZ = m.getPosterior()[0]                              # warm-up: code objects, pools, the one upload of M2
    rows = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        m.getPosterior()
        wall = (time.perf_counter() - t0) * 1e3
        t = _lib.last_timings() if name != "dense" else dict(assemble=np.nan, grad=np.nan, total=np.nan)
        rows.append((wall, t["assemble"], t["grad"], t["total"]))
    a = np.array(rows)
    lo, md = a.min(axis=0), np.median(a, axis=0)
    print("N=%d %-8s wall %9.3f ms (median %9.3f)   assemble %7.3f  grad %7.3f  device total %8.3f   nlZ %.10g"
          % (n, name, lo[0], md[0], lo[1], lo[2], lo[3], nlZ), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "step":
        step(args[1], int(args[2]))
        return 0
    n = int(args[0]) if args else 8192
    for name in ("rbf", "program", "dense"):
        rc = subprocess.call(["timeout", "-k", "10", str(LIMIT[name]), sys.executable, os.path.abspath(__file__), "step", name, str(n)])
        if rc != 0:
            print("step %s ended with status %d: stopping" % (name, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
