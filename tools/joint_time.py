#!/usr/bin/env python3
"""The joint posterior of GPR + RBF at N training points, d = 16: covariance of ns test points, its Cholesky factor and nsamp draws

    device   pgp_predict_joint per stage (its own events): cross block + V | Kss | V'V | factor | draws + downloads, with the factor's
             Newton step (the default) and without it (option joint_refine 0: the sweep alone); the rate of the V'V launch
             (2 ns (ns + 128) / 2 N flops on the lower tiles) and of the sweep (ns^3 / 3) as a share of the fp64 MFMA peak of
             DESIGN.md, and the wall time of the call with fcov, Lc and F downloaded
    host     what a user pays without it: download post.L, scipy solve_triangular, V.T @ V, numpy.linalg.cholesky, Lc @ Z on the
             host's BLAS threads

    python tools/joint_time.py [N]            (default 8192) runs the steps one after the other, each in a child process of
                                              its own under a time limit; the first failure ends the run
    python tools/joint_time.py step NAME N NS one step in this process
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PEAK_TF = 78.6                 # fp64 MFMA peak of the MI355X
NSAMP = 16
LIMIT = {"device": 300, "host": 420}


def model(n, d=16, seed=0):
    import pygps_amd as pyGPs
    rng = np.random.RandomState(seed)
    x = rng.randn(n, d)
    y = np.sin(x.sum(axis=1, keepdims=True) / np.sqrt(d)) + 0.1 * rng.randn(n, 1)
    m = pyGPs.GPR()
    m.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(np.log(4.0), 0.0))
    m.setNoise(np.log(0.1))
    m.setData(x, y)
    m.getPosterior()
    return m, rng.randn(16384, d)


def device(n, ns, rounds=5):
    from pygps_amd import _lib
    m, pool = model(n)
    xs = _lib.f64(pool[:ns])
    z = _lib.f64(np.random.default_rng(0).standard_normal((ns, NSAMP)))
    L = m.posterior.L
    dll = _lib.load()
    ms = np.zeros(ns)
    fmu, fcov, Lc, F, st = np.empty(ns), np.empty((ns, ns)), np.empty((ns, ns)), np.empty((ns, NSAMP)), np.zeros(5)
    sn2 = float(np.exp(2.0 * m.likfunc.hyp[0]))
    for refine in (1, 0):
        _lib.check(dll.pgp_set_option(L.ctx, b"joint_refine", refine))
        _device_rounds(dll, L, xs, ms, sn2, z, fmu, fcov, Lc, F, st, n, ns, rounds, refine)
    _lib.check(dll.pgp_set_option(L.ctx, b"joint_refine", 1))


def _device_rounds(dll, L, xs, ms, sn2, z, fmu, fcov, Lc, F, st, n, ns, rounds, refine):
    from pygps_amd import _lib
    rows, walls = [], []
    for r in range(rounds + 1):                             # the first round warms up: code objects, pools, W = L^-1
        t0 = time.perf_counter()
        rc = dll.pgp_predict_joint(L.ctx, L.handle, _lib.ptr(xs), ns, _lib.ptr(ms), sn2, 0.0, _lib.ptr(z), NSAMP, _lib.ptr(fmu),
                                   _lib.ptr(fcov), _lib.ptr(Lc), _lib.ptr(F), _lib.ptr(st))
        wall = (time.perf_counter() - t0) * 1e3
        assert rc == 0, rc
        if r:
            rows.append(st.copy())
            walls.append(wall)
    a = np.array(rows).min(axis=0)
    npad, nsp = (n + 127) // 128 * 128, (ns + 127) // 128 * 128
    vtv_tf = 2.0 * npad * nsp * (nsp + 128) / 2 / (a[2] * 1e-3) / 1e12
    chol_tf = nsp ** 3 / 3.0 / (a[3] * 1e-3) / 1e12
    what = "factor (sweep + Newton step)" if refine else "factor (sweep alone, joint_refine 0)"
    print("N=%d ns=%d nsamp=%d device ms: cross+V %8.3f  Kss %7.3f  V'V %8.3f  %s %8.3f  draws + downloads %7.3f  sum %8.3f   "
          "call wall %9.3f (median %9.3f)" % (n, ns, NSAMP, a[0], a[1], a[2], what, a[3], a[4], a.sum(),
                                              min(walls), np.median(walls)), flush=True)
    print("N=%d ns=%d V'V %.1f TF = %.1f %% of %.1f TF%s" % (n, ns, vtv_tf, 100 * vtv_tf / PEAK_TF, PEAK_TF,
          "" if refine else "   sweep %.1f TF = %.1f %%" % (chol_tf, 100 * chol_tf / PEAK_TF)), flush=True)


def host(n, ns, rounds=2):
    from scipy.linalg import solve_triangular
    import pygps_amd as pyGPs  # noqa: F401
    m, pool = model(n)
    xs = pool[:ns]
    z = np.random.default_rng(0).standard_normal((ns, NSAMP))
    sn2 = float(np.exp(2.0 * m.likfunc.hyp[0]))
    best = None
    for _ in range(rounds):
        m.posterior.L._host = None                          # every round pays the download, as a first use does
        t = [time.perf_counter()]
        R = np.asarray(m.posterior.L)
        t.append(time.perf_counter())
        Ks = m.covfunc.getCovMatrix(x=m.x, z=xs, mode="cross")
        Kss = m.covfunc.getCovMatrix(x=xs, mode="train")
        t.append(time.perf_counter())
        V = solve_triangular(R, Ks / np.sqrt(sn2), trans="T", lower=False)
        t.append(time.perf_counter())
        fcov = Kss - V.T @ V
        t.append(time.perf_counter())
        Lc = np.linalg.cholesky(fcov + sn2 * np.eye(ns))
        t.append(time.perf_counter())
        F = Lc @ z
        t.append(time.perf_counter())
        d = np.diff(np.array(t)) * 1e3
        best = d if best is None or d.sum() < best.sum() else best
    print("N=%d ns=%d nsamp=%d host ms (%s BLAS threads): download post.L %9.1f  Ks, Kss (device) %8.1f  solve_triangular %9.1f  "
          "V.T @ V %9.1f  cholesky %9.1f  Lc @ Z %7.1f  sum %9.1f" % (n, ns, NSAMP, os.environ.get("OMP_NUM_THREADS", "?"), best[0],
                                                                      best[1], best[2], best[3], best[4], best[5], best.sum()),
          flush=True)
    assert np.all(np.isfinite(F))


def main():
    args = sys.argv[1:]
    if args and args[0] == "step":
        {"device": device, "host": host}[args[1]](int(args[2]), int(args[3]))
        return 0
    n = int(args[0]) if args else 8192
    for ns in (1024, 8192):
        for name in ("device", "host"):
            rc = subprocess.call(["timeout", "-k", "10", str(LIMIT[name]), sys.executable, os.path.abspath(__file__), "step", name,
                                  str(n), str(ns)])
            if rc != 0:
                print("step %s ns=%d ended with status %d: stopping" % (name, ns, rc), flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
