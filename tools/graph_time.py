#!/usr/bin/env python3
"""Wall time of the device graph helpers against their host counterparts:

    knn      graphUtil.formKnnGraph at n = 7291, d = 256, k = 3 (USPS-shaped) against scipy's KD-tree query (the reference's route)
    reglap   nodeKernels.regLapKernel at n = 4096 against numpy's inverse
    diff     nodeKernels.diffKernel at n = 4096 against numpy's eigh route

    python tools/graph_time.py             runs the three steps one after the other, each in a child process of its own under
                                           a time limit; the first failure ends the run
    python tools/graph_time.py step NAME   one step in this process

Device times include the upload of the input and the download of the n x n result; best of 3 after a warm-up call."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

LIMIT = {"knn": 600, "reglap": 300, "diff": 300}


def best(fn, rounds):
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return min(out), r


def knn_graph_host(pts, k):
    """graphUtil.py:29-46 restated: KD-tree query for k + 1 neighbours, the first dropped, symmetrised with max."""
    from scipy import spatial
    n = pts.shape[0]
    nn = spatial.KDTree(pts).query(pts, k + 1)[1][:, 1:]
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), k), nn.reshape(-1)] = 1.0
    return np.maximum(A, A.T)


def step(name):
    from pygps_amd.GraphExtensions import graphUtil, nodeKernels
    if name == "knn":
        pts = np.tanh(np.random.RandomState(0).randn(7291, 256))
        graphUtil.formKnnGraph(pts[:512], 3)
        td, A = best(lambda: graphUtil.formKnnGraph(pts, 3), 3)
        th, Ah = best(lambda: knn_graph_host(pts, 3), 1)
        print("knn n=7291 d=256 k=3: device %.1f ms, host KD-tree %.1f ms, equal %s" % (td, th, np.array_equal(A, Ah)), flush=True)
        return
    n = 4096
    pts = np.random.RandomState(1).randn(n, 8)
    A = graphUtil.formKnnGraph(pts, 3)
    if name == "reglap":
        dev, host = (lambda: nodeKernels.regLapKernel(A, 1)), (lambda: np.linalg.inv(np.identity(n) + nodeKernels.normLap(A)))
    else:
        def host():
            w, Q = np.linalg.eigh(A - np.diag(A.sum(axis=1)))
            return (Q * np.exp(0.5 * w)) @ Q.T
        dev = lambda: nodeKernels.diffKernel(A, 0.5)  # noqa: E731
    dev()
    td, K = best(dev, 3)
    th, Kh = best(host, 1)
    print("%s n=%d: device %.1f ms, numpy %.1f ms, max difference / max|K| %.2e"
          % (name, n, td, th, np.max(np.abs(K - Kh)) / np.max(np.abs(Kh))), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "step":
        step(args[1])
        return 0
    for name in ("knn", "reglap", "diff"):
        rc = subprocess.call(["timeout", "-k", "10", str(LIMIT[name]), sys.executable, os.path.abspath(__file__), "step", name])
        if rc != 0:
            print("step %s ended with status %d: stopping" % (name, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
