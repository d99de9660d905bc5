#!/usr/bin/env python3
"""Generate the G24 golden vectors (GPMC, one-vs-one multi-class classification) under tests/golden/ by importing the
REFERENCE (marionmari/pyGPs, read-only at /root/reference) in the build container.

Run by hand, here only:

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gpmc.py [ids...]

Same set-up as make_golden_fitc_ep.py (the `past` shim in tests/golden/_shim, pyGPs imported unmodified, plain arrays
stored).  The USPS file of the reference's demo is not part of the reference tree, so the data come from the seeded
generator tests/gpmc_data.py, which the tests import too: a fixture stores seeds and results, not inputs.

Added from outside, no reference source is copied:
- Inference._epComputeParams is wrapped to count calls: a cold EP fit calls it once per sweep (inf.py:772).
- GPC.predict is wrapped: GPMC's loops call it exactly once per pair, right after the pair's fit (gp.py:854, 892), so the
  wrapper records that pair's nlZ, hyper-parameters and the sweeps / Newton steps since the previous pair.
- `fit_laplace`: the reference's GPMC.useInference stores self.inffunc, but its loops test self.newInf, which nothing sets
  (gp.py:776-785, 849).  The fixture is what the reference computes once that attribute is set from outside
  (m.newInf = "Laplace"): its own loop, its own GPC.useInference("Laplace") per pair, its own vote arithmetic.  Core.tools.cmp is
  rebound and Core.inf.brentmin counted exactly as make_golden_laplace.py does.

Before a fixture is written the recipe asserts that no pair reached the reference's cap of 10 sweeps and that every vote is
above 1e-3 (so that relative errors mean something).

Reference call sites exercised: Core/gp.py:738-932 (GPMC), 641-732 (GPC), Core/inf.py:723-806 (EP), 459-564 (Laplace).
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
import pyGPs.Core.gp as ref_gp  # noqa: E402
import pyGPs.Core.inf as ref_inf  # noqa: E402
import pyGPs.Core.tools as ref_tools  # noqa: E402

import gpmc_data  # noqa: E402

ref_tools.cmp = lambda a, b: int(a > b) - int(a < b)

META = dict(numpy=np.__version__, scipy=scipy.__version__, reference="marionmari/pyGPs v1.3.5 @ /root/reference",
            note="data from tests/gpmc_data.py; _epComputeParams / brentmin counted; GPC.predict wrapped to record each pair")


class Rec(object):
    calls = 0            # _epComputeParams calls (EP sweeps) or brentmin calls (Newton steps) since the last pair
    pairs = []           # per pair: (nlZ, iterations of its LAST evaluate, cov hyp)


_orig_cp = ref_inf.Inference._epComputeParams
_orig_brent = ref_inf.brentmin
_orig_predict = ref_gp.GPC.predict
_orig_eval = {cls: cls.evaluate for cls in (ref_inf.EP, ref_inf.Laplace)}


def _cp(self, *a, **k):
    Rec.calls += 1
    return _orig_cp(self, *a, **k)


def _brent(*a, **k):
    Rec.calls += 1
    return _orig_brent(*a, **k)


def _evaluate(cls):
    def ev(self, *a, **k):
        Rec.calls = 0                      # the count that is recorded is that of the pair's LAST evaluate (its final posterior)
        return _orig_eval[cls](self, *a, **k)
    return ev


def _predict(self, *a, **k):
    Rec.pairs.append((float(self.nlZ), int(Rec.calls), np.array(self.covfunc.hyp, dtype=float)))
    return _orig_predict(self, *a, **k)


ref_inf.Inference._epComputeParams = _cp
ref_inf.brentmin = _brent
ref_gp.GPC.predict = _predict
for _cls in _orig_eval:
    _cls.evaluate = _evaluate(_cls)


def save(name, **arrs):
    arrs["meta"] = np.array(repr(META))
    path = os.path.join(HERE, "G24_" + name + ".npz")
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    assert size < 490 * 1024, size
    print("wrote G24_%s: %d bytes" % (name, size), flush=True)


def run(name, optimize=False, laplace=False):
    shape = gpmc_data.SHAPES[name]
    x, y, xs = gpmc_data.blobs(**shape)
    C = len(shape["counts"])
    m = pyGPs.GPMC(C)
    mean, kernel = gpmc_data.prior(name, pyGPs.cov, pyGPs.mean)
    if kernel is not None or mean is not None:
        m.setPrior(mean=mean, kernel=kernel)
    if laplace:
        m.useInference("Laplace")          # stores self.inffunc only (gp.py:782-783) ...
        m.newInf = "Laplace"               # ... this is what its loops test (gp.py:849)
    m.setData(x, y)
    Rec.pairs = []
    t0 = time.time()
    votes = m.optimizeAndPredict(xs) if optimize else m.fitAndPredict(xs)
    secs = time.time() - t0
    npairs = C * (C - 1) // 2
    assert len(Rec.pairs) == npairs
    nlZ = np.array([p[0] for p in Rec.pairs])
    iters = np.array([p[1] for p in Rec.pairs], dtype=np.int64)
    hyp = np.array([p[2] for p in Rec.pairs])
    if not laplace:
        assert iters.max() < 10, iters     # no pair reached the reference's cap
    assert votes.min() > 1e-3, votes.min()
    print("   %s: %.1f s, iterations %d..%d, smallest vote %.2e" % (name, secs, iters.min(), iters.max(), votes.min()), flush=True)
    # createBinaryClass's index order for one pair: the reference's own method on a model whose "inputs" are the row numbers
    pi, pj = 1, C - 1
    probe = pyGPs.GPMC(C)
    probe.setData(np.arange(x.shape[0], dtype=float), y)
    bx, by = probe.createBinaryClass(pi, pj)
    META["note_" + name] = ("inference Laplace through newInf set from outside (see the recipe's docstring)" if laplace else "EP")
    save(name, votes=votes, pair_nlZ=nlZ, pair_iters=iters, pair_hyp=hyp, binary_pair=np.array([pi, pj]),
         binary_index=bx.reshape(-1).astype(np.int64), binary_y=by.reshape(-1), n_class=C, ref_seconds=secs,
         final_cov_hyp=np.array(m.covfunc.hyp, dtype=float), final_mean_hyp=np.array(m.meanfunc.hyp, dtype=float),
         **{"shape_" + k: np.array(v) for k, v in shape.items()})


JOBS = dict(fit_default=lambda: run("fit_default"), fit_c5_uneven=lambda: run("fit_c5_uneven"),
            fit_ard_const=lambda: run("fit_ard_const"), fit_program=lambda: run("fit_program"),
            fit_laplace=lambda: run("fit_laplace", laplace=True), opt_default=lambda: run("opt_default", optimize=True),
            opt_prior=lambda: run("opt_prior", optimize=True), fit_c10_d64=lambda: run("fit_c10_d64"))

if __name__ == "__main__":
    for j in (sys.argv[1:] or list(JOBS)):
        t0 = time.time()
        JOBS[j]()
        print("%s: %.1f s" % (j, time.time() - t0), flush=True)
