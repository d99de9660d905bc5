#!/usr/bin/env python3
"""Leave-one-out inference of GPR + RBF at N training points, d = 16 (inf.LOO, GPR.predict_loo) against what it replaces

    fit      inf.LOO with gradients against inf.Exact with gradients; a value-only LOO call (predict_loo) against a value-only
             exact fit: device ms of a whole fit from the fit's own HIP events (pgp_last_timings, best of the timed rounds) and the
             wall time of the call
    product  the symmetric product S = G G' of the LOO gradient matrix (np^3 flops on the lower tiles) as a rate and as a share
             of the fp64 MFMA peak of DESIGN.md.  It is profiled in the class of B^-1 = E E' ("gemm_f64(lauum W^T W)", np^3 / 3
             flops: E is triangular), so its time and flops are the class's in a LOO fit minus the class's in an exact fit with
             gradients on the same context; the E E' launches' own rate is printed beside it
    kfold    valid.k_fold_validation with K = 10: ten fits on 9/10 of the data + ten predicts (wall), the loop LOO replaces

    python tools/loo_time.py [N]            (default 8192) runs the steps one after the other, each in a child process of its own
                                            under a time limit; the first failure ends the run
    python tools/loo_time.py step NAME N    one step in this process
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PEAK_TF = 78.6                 # fp64 MFMA peak of the MI355X
LIMIT = {"fit": 300, "product": 200, "kfold": 400}


def model(n, d=16, seed=0, loo=False):
    import pygps_amd as pyGPs
    rng = np.random.RandomState(seed)
    x = rng.randn(n, d)
    y = np.sin(x.sum(axis=1, keepdims=True) / np.sqrt(d)) + 0.1 * rng.randn(n, 1)
    m = pyGPs.GPR()
    m.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(np.log(4.0), 0.0))
    m.setNoise(np.log(0.1))
    m.setData(x, y)
    if loo:
        m.useInference("LOO")
    return m, x, y


def _timed(fn, rounds):
    from pygps_amd import _lib
    dev, wall = [], []
    for r in range(rounds + 1):                             # the first round warms up: code objects, pools
        t0 = time.perf_counter()
        fn()
        w = (time.perf_counter() - t0) * 1e3
        if r:
            dev.append(_lib.last_timings()["total"])
            wall.append(w)
    return min(dev), min(wall), float(np.median(wall))


def fit(n, rounds=5):
    rows = {}
    for name, loo in (("Exact", False), ("LOO", True)):
        m, x, y = model(n, loo=loo)
        rows[name + " with gradients"] = _timed(lambda: m.getPosterior(), rounds)
        rows[name + " value-only"] = _timed((lambda: m.predict_loo()) if loo else (lambda: m.getPosterior(der=False)), rounds)
    for k, (d, w, wm) in rows.items():
        print("N=%d %-22s device %9.3f ms   call wall %9.3f ms (median %9.3f)" % (n, k, d, w, wm), flush=True)
    print("N=%d LOO / Exact: with gradients %.2f x (device), value-only %.2f x (device)" % (
        n, rows["LOO with gradients"][0] / rows["Exact with gradients"][0], rows["LOO value-only"][0] / rows["Exact value-only"][0]),
        flush=True)


def product(n, rounds=3):
    from pygps_amd import _lib
    cls = "gemm_f64(lauum W^T W)"
    dll, ctx = _lib.load(), _lib.ctx()
    rows = {}
    for name, loo in (("exact", False), ("loo", True)):
        m, x, y = model(n, loo=loo)
        m.getPosterior()
        _lib.check(dll.pgp_set_profiling(ctx, 1))
        _lib.check(dll.pgp_profile_reset(ctx))
        for _ in range(rounds):
            m.getPosterior()
        rows[name] = _lib.profile()[cls]
        dll.pgp_set_profiling(ctx, 0)
    e, l = rows["exact"], rows["loo"]
    for what, ms, fl, k in (("S = G G' (LOO - Exact)", l["ms"] - e["ms"], l["flops"] - e["flops"], l["launches"] - e["launches"]),
                            ("B^-1 = E E' (Exact)", e["ms"], e["flops"], e["launches"])):
        tf = fl / (ms * 1e-3) / 1e12 if ms > 0 else float("nan")
        print("N=%d %-26s %3d launches  %9.3f ms per fit  %6.1f TF = %5.1f %% of %.1f TF" % (
            n, what, k, ms / rounds, tf, 100 * tf / PEAK_TF, PEAK_TF), flush=True)


def kfold(n, K=10):
    import pygps_amd as pyGPs
    from pygps_amd import valid
    m, x, y = model(n)
    best = None
    for _ in range(2):                                      # the first pass warms up
        t0 = time.perf_counter()
        rmse = []
        for x_tr, x_te, y_tr, y_te in valid.k_fold_validation(x, y, K=K):
            f = pyGPs.GPR()
            f.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(np.log(4.0), 0.0))
            f.setNoise(np.log(0.1))
            f.getPosterior(x_tr, y_tr.reshape(-1, 1), der=False)
            ym = f.predict(x_te)[0]
            rmse.append(valid.RMSE(ym, y_te.reshape(-1, 1)))
        best = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    rec = valid.loo_validation(m)
    t1 = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    rec = valid.loo_validation(m)
    t1 = min(t1, (time.perf_counter() - t0) * 1e3)
    print("N=%d k_fold_validation K=%d (value-only fits + predicts) wall %9.1f ms, RMSE %.4f   loo_validation wall %9.1f ms, RMSE %.4f" % (
        n, K, best, float(np.mean(rmse)), t1, rec["RMSE"]), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "step":
        {"fit": fit, "product": product, "kfold": kfold}[args[1]](int(args[2]))
        return 0
    n = int(args[0]) if args else 8192
    for name in ("fit", "product", "kfold"):
        rc = subprocess.call(["timeout", "-k", "10", str(LIMIT[name]), sys.executable, os.path.abspath(__file__), "step", name, str(n)])
        if rc != 0:
            print("step %s ended with status %d: stopping" % (name, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
