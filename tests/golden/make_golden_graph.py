#!/usr/bin/env python3
"""Generate the G25 golden vectors (cov.Pre, graph node kernels) under tests/golden/ by importing the REFERENCE
(marionmari/pyGPs, read-only at /root/reference) in the build container.

Run by hand, here only:

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_graph.py [ids...]

Same set-up as make_golden_laplace.py (the `past` shim in tests/golden/_shim, pyGPs imported unmodified, `cmp` in the
reference's tools module rebound for the Laplace fits, plain arrays stored).  The points and labels of every case come
from seeds (tests/graph_cpu.py graph_problem draws them); every matrix -- adjacency, node kernel, M1, M2 -- comes from the
reference's own functions.

Reference call sites exercised: GraphExtensions/graphUtil.py:29-82 (formKnnGraph, formKernelMatrix, normalizeKernel),
GraphExtensions/nodeKernels.py:28-131 (all six node kernels and normLap), Core/cov.py:1429-1455 (Pre) inside
Core/cov.py:230-328 (Sum, Product, Scale), Core/inf.py:345-384 (Exact), :459-564 (Laplace), :723-806 (EP),
Core/gp.py:251-285 (optimize), :349-437 (predict).
"""
import os
import sys
import time

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "_shim"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import scipy  # noqa: E402
import pyGPs  # noqa: E402  (the reference)
import pyGPs.Core.tools as ref_tools  # noqa: E402
from pyGPs.GraphExtensions import graphUtil, nodeKernels  # noqa: E402

import graph_cpu  # noqa: E402  (tests/graph_cpu.py: the seeds -> points / labels recipe only)

ref_tools.cmp = lambda a, b: int(a > b) - int(a < b)

META = dict(numpy=np.__version__, scipy=scipy.__version__,
            reference="marionmari/pyGPs v1.3.5 @ /root/reference", note="Core.tools.cmp rebound (numpy bools)")


def save(name, **arrs):
    arrs["meta"] = np.array(repr(META))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrs)
    print("wrote", name, os.path.getsize(os.path.join(HERE, name + ".npz")), "bytes", flush=True)


def dn(d):
    return dict(dnlZ_mean=np.array(d.mean, dtype=float), dnlZ_cov=np.array(d.cov, dtype=float),
                dnlZ_lik=np.array(d.lik, dtype=float))


def edges(A):
    i, j = np.nonzero(A)
    return np.stack([i, j]).astype(np.int32)


# ----------------------------------------------------------------------------- graph helpers
def knn():
    out = {}
    for tag, (n, d, k, seed) in (("a", (400, 8, 3, 0)), ("usps", (300, 256, 2, 1))):
        pts = np.random.RandomState(seed).randn(n, d)
        if tag == "usps":                                  # USPS-shaped: 16 x 16 grey values in [-1, 1]
            pts = np.tanh(pts)
        A = graphUtil.formKnnGraph(pts, k)
        out.update({tag + "_ndks": np.array([n, d, k, seed]), tag + "_edges": edges(A), tag + "_degree": A.sum(axis=0)})
    save("G25_knn_graphs", **out)


def node_kernels():
    n, d, k, seed = 120, 4, 3, 2
    pts = np.random.RandomState(seed).randn(n, d)
    A = graphUtil.formKnnGraph(pts, k)
    save("G25_node_kernels_a", ndks=np.array([n, d, k, seed]), edges=edges(A), normLap=nodeKernels.normLap(A),
         regLap=nodeKernels.regLapKernel(A, 1), regLap_s07=nodeKernels.regLapKernel(A, 0.7), diff=nodeKernels.diffKernel(A, 0.5))
    save("G25_node_kernels_b", ndks=np.array([n, d, k, seed]), psInv=nodeKernels.psInvLapKernel(A),
         VND=nodeKernels.VNDKernel(A, 0.5), rw_p3_a2=nodeKernels.rwKernel(A, 3, 2), rw_p2_a1=nodeKernels.rwKernel(A, 2.7, 0.5),
         cos=nodeKernels.cosKernel(A))
    K = nodeKernels.diffKernel(A, 0.5)
    rng = np.random.RandomState(3)
    perm = rng.permutation(n)
    tr, te = np.sort(perm[:100]), np.sort(perm[100:])
    M1, M2 = graphUtil.formKernelMatrix(K, tr, te)
    save("G25_kernel_matrix_helpers", ndks=np.array([n, d, k, seed]), train=tr, test=te, M1=M1, M2=M2,
         normalized=graphUtil.normalizeKernel(K))


def node_kernels_device():
    """The sizes the device node kernels are tested at (tests/test_gpu_graph.py): n = 200 with the full matrices, one file per
    kernel (a file stays below the size of the largest fixture committed before), and n = 1500 with the diagonal, K v for a
    fixed random v and 3000 sampled entries per kernel.  Points: randn(n, 8) from seed 5, 3-NN graph."""
    for n in (200, 1500):
        A = graphUtil.formKnnGraph(np.random.RandomState(5).randn(n, 8), 3)
        Ks = dict(regLap=nodeKernels.regLapKernel(A, 0.7), VND=nodeKernels.VNDKernel(A, 0.5), rw=nodeKernels.rwKernel(A, 3, 2),
                  diff=nodeKernels.diffKernel(A, 0.5))
        if n == 200:
            for name, K in Ks.items():
                save("G25_node_n200_" + name, ndks=np.array([n, 8, 3, 5]), edges=edges(A), K=K)
            continue
        rng = np.random.RandomState(9)
        v = rng.randn(n)
        ii, jj = rng.randint(0, n, 3000), rng.randint(0, n, 3000)
        out = dict(ndks=np.array([n, 8, 3, 5]), edges=edges(A), v=v, ii=ii, jj=jj)
        for name, K in Ks.items():
            out.update({name + "_diag": np.diag(K).copy(), name + "_Kv": K @ v, name + "_entries": K[ii, jj],
                        name + "_absmax": np.array(np.max(np.abs(K)))})
        save("G25_node_kernels_n1500", **out)


# ----------------------------------------------------------------------------- fits with cov.Pre
N_TRAIN, N_TEST, DIM, SEED = 300, 20, 8, 0


def problem():
    p = graph_cpu.graph_problem(N_TRAIN, N_TEST, DIM, SEED)
    A = graphUtil.formKnnGraph(p["pts"], 3)
    K = nodeKernels.diffKernel(A, 0.5)
    M1, M2 = graphUtil.formKernelMatrix(K, p["train"], p["test"])
    p.update(A=A, K=K, M1=M1, M2=M2)
    return p


def count_sweeps(m):
    calls = []
    orig = type(m.inffunc)._epComputeParams

    def spy(self, *a, **k):
        out = orig(self, *a, **k)
        calls.append(float(out[2]))
        return out
    type(m.inffunc)._epComputeParams = spy
    try:
        res = m.getPosterior()
    finally:
        type(m.inffunc)._epComputeParams = orig
    return res, len(calls)


def fit_dict(tag, nlZ, dnlZ, post, pred, **extra):
    ym, ys2, fm, fs2, lp = pred
    out = dict(nlZ=nlZ, alpha=post.alpha, sW=post.sW, L_diag=np.diag(post.L).copy(), pred_ym=ym, pred_ys2=ys2, pred_fm=fm,
               pred_fs2=fs2, **dn(dnlZ))
    out.update(extra)
    return {tag + "_" + k: v for k, v in out.items()}


def fits():
    cov = pyGPs.cov
    p = problem()
    x, y, xs, M1, M2 = p["x"], p["y"], p["xs"], p["M1"], p["M2"]
    n = x.shape[0]
    out = dict(ntds=np.array([N_TRAIN, N_TEST, DIM, SEED]), M1=M1, M2_diag=np.diag(M2).copy(), M2_row0=M2[0].copy(),
               eig_min=np.linalg.eigvalsh(p["K"])[0])
    # GPC, Pre alone (demo_NodeKernel's second model): dummy inputs
    m = pyGPs.GPC()
    m.setPrior(kernel=cov.Pre(M1, M2))
    m.setData(np.zeros((n, 1)), y)
    (nlZ, dnlZ, post), sw = count_sweeps(m)
    out.update(fit_dict("pre_ep", nlZ, dnlZ, post, m.predict(np.zeros((N_TEST, 1))), n_sweeps=sw))
    # GPC, Pre + RBFunit (the demo's third model): EP and Laplace
    for tag in ("sum_ep", "sum_laplace"):
        m = pyGPs.GPC()
        if tag == "sum_laplace":
            m.useInference("Laplace")
        m.setPrior(kernel=cov.Pre(M1, M2) + cov.RBFunit(np.log(2.5)))
        m.setData(x, y)
        if tag == "sum_ep":
            (nlZ, dnlZ, post), sw = count_sweeps(m)
            extra = dict(n_sweeps=sw)
        else:
            nlZ, dnlZ, post = m.getPosterior()
            extra = {}
        out.update(fit_dict(tag, nlZ, dnlZ, post, m.predict(xs), **extra))
    # GPR on a smooth target: Pre * s + RBF (the Scale gradient) and Pre * RBF
    yr = np.sin(p["pts"] @ np.ones((DIM, 1)) / np.sqrt(DIM))[p["train"]] + 0.1 * np.random.RandomState(5).randn(n, 1)
    out["yr"] = yr
    for tag, k in (("scale_sum", cov.Pre(M1, M2) * 0.4 + cov.RBF(np.log(2.0), -0.3)),
                   ("prod", cov.Pre(M1, M2) * cov.RBF(np.log(3.0), 0.2))):
        m = pyGPs.GPR()
        m.setPrior(mean=pyGPs.mean.Zero(), kernel=k)
        m.setNoise(np.log(0.2))
        m.setData(x, yr)
        nlZ, dnlZ, post = m.getPosterior()
        out.update(fit_dict(tag, nlZ, dnlZ, post, m.predict(xs), cov_hyp=np.array(m.covfunc.hyp)))
    save("G25_pre_fits_N300", **out)


def optimize():
    cov = pyGPs.cov
    p = problem()
    m = pyGPs.GPC()
    m.setPrior(kernel=cov.Pre(p["M1"], p["M2"]) + cov.RBFunit(np.log(2.5)))
    m.setData(p["x"], p["y"])
    t0 = time.time()
    m.optimize(numIterations=8)
    print("   optimize: %.1f s" % (time.time() - t0), flush=True)
    ym, ys2, fm, fs2, lp = m.predict(p["xs"])
    save("G25_pre_optimize_N300", ntds=np.array([N_TRAIN, N_TEST, DIM, SEED]), iters=8, cov_hyp0=np.array([np.log(2.5)]),
         cov_hyp=np.array(m.covfunc.hyp), opt_nlZ=np.array(m.nlZ, dtype=float), pred_ym=ym, pred_fs2=fs2)


CASES = {"knn": knn, "node_kernels": node_kernels, "node_kernels_device": node_kernels_device, "fits": fits, "optimize": optimize}

if __name__ == "__main__":
    for i in sys.argv[1:] or list(CASES):
        t = time.time()
        CASES[i]()
        print("  %s done in %.1fs" % (i, time.time() - t), flush=True)
