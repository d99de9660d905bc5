#!/usr/bin/env python3
"""Wall time of GraphExtensions.graphKernels.propagationKernel and the device time of its stages:

    mutag      the demo's call: MUTAG (3371 nodes, 188 graphs, k = 7), h_max = 10, w = 1e-4, 'tv', 'label_diffusion'
    synthetic  N = 1500 graphs of 120 nodes (n = 180 000): a ring plus 3 random in-graph edges per node, k = 8, h_max = 10,
               w = 1e-4, 'tv', 'label_diffusion'

    python tools/propagation_time.py             runs the two steps one after the other, each in a child process of its own
                                                 under a time limit; the first failure ends the run
    python tools/propagation_time.py step NAME   one step in this process
    python tools/propagation_time.py host NAME   the numpy restatement (tests/propagation_cpu.py) of the step, for comparison

Wall times include the host's set-up (CSR, grouping, draws), the upload and the download of the (N, N, h_max + 1) result; best of 3
after a warm-up call.  Stage times are the device's (events on the stream), from one further call."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import scipy.sparse as spsp  # noqa: E402

LIMIT = {"mutag": 300, "synthetic": 600}
H_MAX, W = 10, 1e-4


def problem(name):
    if name == "mutag":
        d = np.load(os.path.join(ROOT, "tests", "golden", "G26_mutag.npz"))
        A = spsp.csc_matrix((d["adj_data"], d["adj_indice"], d["adj_indptr"]), shape=d["adj_shape"])
        return A, d["responses"], d["graph_ind"]
    import propagation_cpu as P
    return P.synthetic([120] * 1500, 8, 0, extra=3)


def step(name):
    from pygps_amd import _lib
    from pygps_amd.GraphExtensions import graphKernels
    A, l, gr = problem(name)

    def call():
        np.random.seed(1)
        return graphKernels.propagationKernel(A, l, gr, H_MAX, W, "tv", "label_diffusion")
    call()
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        K = call()
        wall.append((time.perf_counter() - t0) * 1e3)
    np.random.seed(1)
    stages = graphKernels._propagation(A, l, gr, H_MAX, W, "tv", "label_diffusion", True, want_stages=True)[2]
    print("%s: n = %d, N = %d, nnz = %d, h_max = %d: wall %.1f ms (best of 3: %s); K[:, :, -1] sums to %d"
          % (name, A.shape[0], K.shape[0], A.nnz, H_MAX, min(wall), " ".join("%.1f" % t for t in wall), K[:, :, -1].sum()), flush=True)
    print("   device stages, ms: " + "  ".join("%s %.2f" % (s, t) for s, t in zip(_lib.PROP_STAGES, stages))
          + "  (sum %.2f)" % stages.sum(), flush=True)


def host(name):
    import propagation_cpu as P
    A, l, gr = problem(name)
    np.random.seed(1)
    t0 = time.perf_counter()
    r = P.propagation_cpu(A, l, gr, H_MAX, W, "tv", "label_diffusion")
    print("%s: numpy restatement %.1f ms; K[:, :, -1] sums to %d" % (name, (time.perf_counter() - t0) * 1e3, r["K"][:, :, -1].sum()),
          flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] in ("step", "host"):
        (step if args[0] == "step" else host)(args[1])
        return 0
    for name in ("mutag", "synthetic"):
        rc = subprocess.call(["timeout", "-k", "10", str(LIMIT[name]), sys.executable, os.path.abspath(__file__), "step", name])
        if rc != 0:
            print("step %s ended with status %d: stopping" % (name, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
