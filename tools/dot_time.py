#!/usr/bin/env python3
"""Exact GPR fits with gradients (nargout = 3) at N training points, d = 16, per-fit time of

    rbf      GPR + RBF                               (the plain hot path, for scale)
    program  GPR + (Linear + RBF) as ONE device program: the dot product is accumulated beside r^2 in the assembly and
             in the fused gradient pass
    dense    the same model forced down the dense route: K and the three derivative matrices are built by pgp_cov, come
             back to the host and cross PCIe again for every evaluation
    gram     getCovMatrix('train') of Linear at N points, d = 256, against numpy's x @ x.T on the host

    python tools/dot_time.py [N]            (default 8192) runs the steps one after the other, each in a child process of
                                            its own under a time limit; the first failure ends the run
    python tools/dot_time.py step NAME N    one step in this process

Prints best and median wall time per fit over `rounds` fits after a warm-up, and the `assemble` / `grad` / `total` device
stages of _lib.last_timings() for the two device-program steps."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

LIMIT = {"rbf": 300, "program": 300, "dense": 600, "gram": 300}        # seconds per step


def data(n, d=16, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.randn(n, d)
    y = np.sin(x.sum(axis=1, keepdims=True) / np.sqrt(d)) + 0.2 * x[:, :1] + 0.1 * rng.randn(n, 1)
    return x, y


def gram(n, rounds=5):
    import pygps_amd as pyGPs
    x = np.random.RandomState(1).randn(n, 256)
    k = pyGPs.cov.Linear(0.0)
    K = k.getCovMatrix(x=x, mode="train")                  # warm-up
    dev, host = [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        K = k.getCovMatrix(x=x, mode="train")
        dev.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        H = x @ x.T
        host.append((time.perf_counter() - t0) * 1e3)
    err = float(np.max(np.abs(K - H - 1e-10 * np.eye(n))) / np.max(np.abs(H)))
    print("N=%d d=256 Linear getCovMatrix('train') %9.3f ms (median %9.3f)   numpy x @ x.T %9.3f ms (median %9.3f)   "
          "max rel diff %.2g" % (n, min(dev), np.median(dev), min(host), np.median(host), err), flush=True)


def step(name, n, rounds=7):
    import pygps_amd as pyGPs
    from pygps_amd import _lib
    cov = pyGPs.cov
    if name == "gram":
        return gram(n)
    x, y = data(n)
    if name == "rbf":
        k = cov.RBF(np.log(4.0), 0.0)
    else:
        k = cov.Linear(np.log(0.05)) + cov.RBF(np.log(4.0), 0.0)
        if name == "dense":
            k._tokens = lambda: None                       # no device program: inf.Exact takes the dense route
            rounds = 3
    m = pyGPs.GPR()
    m.setPrior(mean=pyGPs.mean.Zero(), kernel=k)
    m.setNoise(np.log(0.1))
    m.setData(x, y)
    nlZ = m.getPosterior()[0]                              # warm-up: code objects, pools
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
    for name in ("rbf", "program", "dense", "gram"):
        rc = subprocess.call(["timeout", "-k", "10", str(LIMIT[name]), sys.executable, os.path.abspath(__file__), "step", name, str(n)])
        if rc != 0:
            print("step %s ended with status %d: stopping" % (name, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
