#!/usr/bin/env python3
"""Generate the G26 golden vectors (propagation kernels between graphs) under tests/golden/ by importing the REFERENCE
(marionmari/pyGPs) in the build container.

Run by hand, where a checkout of the reference is at hand:

    PYGPS_REFERENCE=<checkout> MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_propagation.py [ids...]

Same set-up as make_golden_graph.py (the `past` shim in tests/golden/_shim, pyGPs imported unmodified).  Two repairs are made at
the call, not in the reference: `graph_ind` is passed as integers (stored as float, it fails as an index under current numpy), and
label matrices are passed as copies (the reference writes into them).

MUTAG is data of the reference (Demo/GraphData/graphData/MUTAG.npz): its seven arrays are stored as G26_mutag.  Kernel matrices
are stored as int32 lower triangles (every entry is an integer count): all slices for the demo configuration, for every other
case the last slice plus, per slice, its sum, its trace and K_h u for a stored integer vector u.

For every case the recorder checks that
  * the numpy restatement tests/propagation_cpu.py equals the reference EXACTLY, and
  * the case is not decided by rounding: the smallest distance of any (lab . v + b) / w to an integer, in bins, is at least 100
    times eps (k + h_max (maxdeg + 2)) sum|v_j| / w (the reference's BLAS sums the hash in an order we do not know).
Where a seed fails either, the next seed is taken; the seed used is stored.  The demo's seed is the demo's (1) and must pass.

Reference call sites exercised: GraphExtensions/graphKernels.py:27-184 (propagationKernel), Demo/GraphData/demo_GraphKernel.py,
GraphExtensions/graphUtil.py:49-63 (formKernelMatrix), Core/cov.py (Pre), Core/inf.py (EP), Core/gp.py (getPosterior, predict).
"""
import os
import sys
import time

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
if "PYGPS_REFERENCE" not in os.environ:
    sys.exit("set PYGPS_REFERENCE to a checkout of the reference (marionmari/pyGPs)")
REF = os.environ["PYGPS_REFERENCE"]
sys.path.insert(0, os.path.join(HERE, "_shim"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import scipy  # noqa: E402
from scipy.sparse import csc_matrix  # noqa: E402
import pyGPs  # noqa: E402  (the reference)
import pyGPs.Core.tools as ref_tools  # noqa: E402
from pyGPs.GraphExtensions import graphUtil, graphKernels  # noqa: E402

import propagation_cpu as P  # noqa: E402  (tests/propagation_cpu.py)

ref_tools.cmp = lambda a, b: int(a > b) - int(a < b)

META = dict(numpy=np.__version__, scipy=scipy.__version__, reference="marionmari/pyGPs v1.3.5",
            note="graph_ind passed as int; label matrices passed as copies")
MUTAG_KEYS = ("labels", "responses", "adj_data", "adj_indptr", "adj_indice", "adj_shape", "graph_ind")
W = 1e-4


def save(name, **arrs):
    arrs["meta"] = np.array(repr(META))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrs)
    print("wrote", name, os.path.getsize(path), "bytes", flush=True)
    assert os.path.getsize(path) < 1 << 20


def mutag():
    data = np.load(os.path.join(REF, "pyGPs", "Demo", "GraphData", "graphData", "MUTAG.npz"))
    return {k: data[k] for k in MUTAG_KEYS}


def demo_inputs(d):
    A = csc_matrix((d["adj_data"], d["adj_indice"], d["adj_indptr"]), shape=d["adj_shape"])
    return A, d["responses"], d["graph_ind"]


def partial_labels(d):
    l = d["responses"].astype(np.int64)
    l[np.random.RandomState(3).rand(l.shape[0]) < 0.4, 0] = -1
    return l


def label_matrix(l):
    k = int(l.max())
    M = np.zeros((l.shape[0], k))
    on = np.nonzero(l[:, 0] > 0)[0]
    M[on, l[on, 0] - 1] = 1
    return M


def record(A, l, gr_id, h_max, p, ktype, seed, search=True):
    """(seed used, reference K, restatement's dict) for the first seed from `seed` on that passes both checks."""
    while True:
        np.random.seed(seed)
        K_ref = graphKernels.propagationKernel(A, np.array(l), gr_id.astype(np.int64), h_max, W, p, ktype, SUM=True)
        np.random.seed(seed)
        r = P.propagation_cpu(A, np.array(l), gr_id, h_max, W, p, ktype, SUM=True)
        k = r["V"].shape[1]
        bound = P.rounding_bound(A, k, h_max, r["V"], W)
        equal, clear = np.array_equal(K_ref, r["K"]), r["edge"] >= 100 * bound
        print("   %-18s %-10s h_max %2d seed %d: restatement == reference %s, edge %.3g bins, bound %.3g, max|key| %.3g"
              % (ktype, p, h_max, seed, equal, r["edge"], bound, r["max_key"]), flush=True)
        if equal and clear:
            r["bound"] = bound
            return seed, K_ref, r
        if not search:
            raise SystemExit("the demo's seed does not pass: equal %s, clear %s" % (equal, clear))
        seed += 1


def summary(tag, seed, K, r, u):
    return {tag + "_seed": np.array(seed), tag + "_last": P.lower(K[:, :, -1:])[0], tag + "_sums": K.sum(axis=(0, 1)),
            tag + "_traces": np.trace(K, axis1=0, axis2=1), tag + "_Ku": np.einsum("ijh,j->hi", K, u.astype(float)),
            tag + "_edge": np.array(r["edge"]), tag + "_bound": np.array(r["bound"])}


def data():
    save("G26_mutag", **mutag())


def demo():
    d = mutag()
    A, l, gr = demo_inputs(d)
    seed, K, r = record(A, l, gr, 10, "tv", "label_diffusion", 1, search=False)
    save("G26_demo_K", seed=np.array(seed), h_max=np.array(10), w=np.array(W), tri=P.lower(K), edge=np.array(r["edge"]),
         bound=np.array(r["bound"]), V=r["V"], b=r["b"])
    # one fold of the demo's flow on slice 10
    y = np.where(d["labels"] == 0, -1, d["labels"]).astype(np.int8)
    N = y.shape[0]
    test = np.arange(0, N, 10)
    train = np.setdiff1d(np.arange(N), test)
    M1, M2 = graphUtil.formKernelMatrix(K[:, :, 10], train, test)
    model = pyGPs.GPC()
    model.setPrior(kernel=pyGPs.cov.Pre(M1, M2))
    nlZ, _, _ = model.getPosterior(np.zeros((len(train), 1)), y[train, :])
    ym, ys2, fm, fs2, lp = model.predict(np.zeros((len(test), 1)))
    acc = float(np.mean(np.sign(ym) == y[test, :]))
    print("   fold: nlZ %.6f accuracy %.2f" % (nlZ, acc), flush=True)
    save("G26_demo_fold", test=test, train=train, nlZ=np.array(nlZ), ym=ym, ys2=ys2, accuracy=np.array(acc))


def cases():
    d = mutag()
    A, l, gr = demo_inputs(d)
    N = int(gr.max())
    u = np.random.RandomState(7).randint(-3, 4, N).astype(np.int64)
    out = dict(u=u, w=np.array(W))
    for ktype in ("label_diffusion", "label_propagation"):                       # (b)
        for p in ("tv", "hellinger", "L2"):
            tag = "b_%s_%s" % (ktype, p)
            out[tag + "_h_max"] = np.array(4)
            out.update(summary(tag, *record(A, l, gr, 4, p, ktype, 1), u=u))
    lp = partial_labels(d)
    out["c_labels"] = lp
    for ktype in ("label_diffusion", "label_propagation"):                       # (c), (d)
        for form, lab in (("c", lp), ("d", label_matrix(lp))):
            tag = "%s_%s" % (form, ktype)
            out[tag + "_h_max"] = np.array(6)
            out.update(summary(tag, *record(A, lab, gr, 6, "tv", ktype, 1), u=u))
    save("G26_cases", **out)


CASES = {"data": data, "demo": demo, "cases": cases}

if __name__ == "__main__":
    for i in sys.argv[1:] or list(CASES):
        t = time.time()
        CASES[i]()
        print("  %s done in %.1fs" % (i, time.time() - t), flush=True)
