#!/usr/bin/env python3
"""GPMC.fitAndPredict times: the shared-kernel engine (pgp_gpmc_fit_predict) and the per-pair route next to the
reference's loop written over pyGPs.GPC and numpy votes inside this script (`baseline`).  The baseline uses nothing of
GPMC, so the script runs unchanged on a commit that has no GPMC: that is where the baseline figure is recorded.

Shapes (synthetic, Gaussian blobs in permuted order, the draw order of tests/gpmc_data.py):
    usps     C = 10, d = 256, n = 7291 (the class sizes of the USPS training set), ns = 2007, RBF(log 16, 0)
    c10_d64  the G24 fixture fit_c10_d64: C = 10, 200 per class, d = 64, ns = 1000, RBF(log 8, 0)

Per shape and route: one warm-up call (code objects, pools), then `--reps` timed calls (host clock around the call,
which ends synchronised); the median, the fastest and the slowest in ms.  For the shared route also the split of the
last call from pgp_last_timings: assembly (K_all + Ks_all), fits, predict (gathers + solves), votes.

    python tools/gpmc_time.py [--shapes usps,c10_d64] [--routes baseline,shared,pairs] [--reps 5] [--json FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import pygps_amd as pyGPs  # noqa: E402
from pygps_amd import _lib  # noqa: E402

USPS_COUNTS = [1194, 1005, 731, 658, 652, 556, 664, 645, 542, 644]          # digits 0..9 of the USPS training set: 7291
SHAPES = {
    "usps": dict(seed=2407, counts=USPS_COUNTS, d=256, ns=2007, sep=0.2, hyp=(np.log(16.0), 0.0)),
    "c10_d64": dict(seed=2401, counts=[200] * 10, d=64, ns=1000, sep=0.5, hyp=(np.log(8.0), 0.0)),
}


def blobs(seed, counts, d, ns, sep):
    """tests/gpmc_data.py's generator, repeated here so that the script stands alone."""
    rng = np.random.RandomState(seed)
    C = len(counts)
    centres = sep * rng.randn(C, d)
    x = np.concatenate([centres[k] + rng.randn(counts[k], d) for k in range(C)])
    y = np.concatenate([np.full(counts[k], k, dtype=float) for k in range(C)])
    perm = rng.permutation(x.shape[0])
    x, y = x[perm], y[perm].reshape(-1, 1)
    ks = rng.randint(0, C, size=ns)
    return x, y, centres[ks] + rng.randn(ns, d)


def baseline(x_all, y_all, xs, C, hyp):
    """The reference's fitAndPredict (Core/gp.py:829-863, 905-928) over pyGPs.GPC; returns votes and the sweeps per pair."""
    votes = np.zeros((xs.shape[0], C))
    t = y_all.reshape(-1)
    sweeps = []
    for i in range(C):
        for j in range(i + 1, C):
            ci, cj = np.flatnonzero(t == i), np.flatnonzero(t == j)
            x = x_all[np.concatenate([ci, cj])]
            y = np.concatenate([np.ones(len(ci)), -np.ones(len(cj))]).reshape(-1, 1)
            model = pyGPs.GPC()
            model.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(*hyp))
            model.getPosterior(x, y)
            ym = model.predict(xs)[0] + 1
            votes[:, i:i + 1] += ym
            votes[:, j:j + 1] += 2 - ym
            sweeps.append(int(model.inffunc.sweeps))
    return votes / votes.sum(axis=1)[:, np.newaxis], sweeps


def gpmc(x_all, y_all, xs, C, hyp, shared):
    m = pyGPs.GPMC(C, shared_kernel=shared)
    m.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(*hyp))
    m.setData(x_all, y_all)
    votes = m.fitAndPredict(xs)
    assert m.last_route == ("shared" if shared else "pairs"), m.last_route
    return votes, [m.pair_iters[p] for p in m.pairs()]


def timed(fn, reps):
    fn()                                                    # warm-up
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="usps,c10_d64")
    ap.add_argument("--routes", default="baseline,shared,pairs")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    have = hasattr(pyGPs, "GPMC")
    results = []
    for name in a.shapes.split(","):
        s = SHAPES[name]
        x, y, xs = blobs(s["seed"], s["counts"], s["d"], s["ns"], s["sep"])
        C = len(s["counts"])
        votes = {}
        for route in a.routes.split(","):
            if route != "baseline" and not have:
                print("%-8s %-8s not available on this commit (no GPMC)" % (name, route), flush=True)
                continue
            fn = ((lambda: baseline(x, y, xs, C, s["hyp"])) if route == "baseline"
                  else (lambda: gpmc(x, y, xs, C, s["hyp"], route == "shared")))
            ts, (v, iters) = timed(fn, a.reps)
            votes[route] = v
            rec = dict(shape=name, route=route, n=int(x.shape[0]), d=s["d"], ns=s["ns"], n_class=C, reps=a.reps,
                       median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), all_ms=[float(t) for t in ts],
                       sweeps=[int(min(iters)), int(max(iters))])
            line = "%-8s %-8s median %9.1f ms  (min %9.1f, max %9.1f, %d calls)  sweeps %d..%d" % (
                name, route, rec["median_ms"], rec["min_ms"], rec["max_ms"], a.reps, min(iters), max(iters))
            if route == "shared":
                lt = _lib.last_timings()
                rec["split_ms"] = dict(assembly=lt["assemble"], fits=lt["solve"], predict=lt["potrf"], votes=lt["grad"], total=lt["total"])
                line += "   split of the last call: assembly %.1f  fits %.1f  predict %.1f  votes %.2f  (total %.1f ms)" % (
                    lt["assemble"], lt["solve"], lt["potrf"], lt["grad"], lt["total"])
            print(line, flush=True)
            results.append(rec)
        if "baseline" in votes:
            for route in votes:
                if route != "baseline":
                    dv = float(np.max(np.abs(votes[route] - votes["baseline"]) / votes["baseline"]))
                    print("%-8s %-8s votes vs baseline: max relative difference %.2e" % (name, route, dv), flush=True)
                    results.append(dict(shape=name, route=route, votes_vs_baseline=dv))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
