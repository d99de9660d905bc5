#!/usr/bin/env python3
"""Generate the G23 golden vectors (spectral mixture kernel cov.SM, D = 1) under tests/golden/ by importing the REFERENCE
(marionmari/pyGPs, read-only at /root/reference) in the build container.

Run by hand, here only:

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sm.py [ids...]

Same set-up as make_golden_lik_laplace.py (the `past` shim in tests/golden/_shim, pyGPs imported unmodified, `cmp` in the
reference's tools module rebound for numpy bools, EP gets a `logger`; no reference source is copied).

D = 1 ONLY: for D > 1 the reference's SM sums partial products instead of taking the product over the coordinates and decodes
`der` against a transposed layout (Core/cov.py:558-560, 598-618), so there is nothing coherent to record; D > 1 is tested
against tests/sm_ref_ld.py.  All frequencies and ranges keep |2 pi m t| <= 200.

Reference call sites exercised: Core/cov.py:521-619 (SM.getCovMatrix / getDerMatrix), Core/inf.py:353-384 (Exact), 723-806 (EP),
459-564 (Laplace), 386-455 (FITC_Exact), Core/gp.py predict / optimize.
"""
import logging
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "_shim"))
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import scipy  # noqa: E402
import pyGPs  # noqa: E402  (the reference)
import pyGPs.Core.tools as ref_tools  # noqa: E402

ref_tools.cmp = lambda a, b: int(a > b) - int(a < b)

META = dict(numpy=np.__version__, scipy=scipy.__version__,
            reference="marionmari/pyGPs v1.3.5 @ /root/reference", note="Core.tools.cmp rebound (numpy bools); EP.logger set")


def save(name, **arrs):
    arrs["meta"] = np.array(repr(META))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrs)
    print("wrote", name, os.path.getsize(os.path.join(HERE, name + ".npz")), "bytes", flush=True)


def dn(d):
    return dict(dnlZ_mean=np.array(d.mean, dtype=float), dnlZ_cov=np.array(d.cov, dtype=float),
                dnlZ_lik=np.array(d.lik, dtype=float))


def sm(w, m, s):
    """Reference SM for D = 1 from weights, frequencies and spectral standard deviations."""
    hyp = [float(v) for v in np.log(np.concatenate([w, m, s]))]
    return pyGPs.cov.SM(len(w), hyp)


def series(n, hi, seed, noise=0.1):
    """1-d series of two sinusoids (0.4 and 1.1 cycles per unit) plus noise on sorted uniform inputs in [0, hi]."""
    rng = np.random.RandomState(seed)
    x = np.sort(rng.uniform(0, hi, (n, 1)), axis=0)
    y = np.sin(2 * np.pi * 0.4 * x) + 0.5 * np.cos(2 * np.pi * 1.1 * x) + noise * rng.randn(n, 1)
    return x, y


Q3 = (np.array([0.8, 0.35, 0.1]), np.array([0.41, 1.08, 0.15]), np.array([0.03, 0.05, 0.2]))
Q2 = (np.array([1.2, 0.4]), np.array([0.4, 0.9]), np.array([0.05, 0.15]))


def kernels():
    rng = np.random.RandomState(23)
    x = rng.uniform(0, 10, (60, 1))
    z = rng.uniform(0, 10, (37, 1))
    z[5] = x[7]                                            # one coincident pair (t = 0)
    for nm, k in (("q1", sm(np.array([0.7]), np.array([0.9]), np.array([0.08]))),
                  ("q3", sm(np.array([0.5, 1.0, 0.3]), np.array([0.3, 1.1, 2.5]), np.array([0.05, 0.1, 0.2])))):
        out = dict(x=x, z=z, hyp=np.array(k.hyp, dtype=float))
        for mode, kw in (("train", dict(x=x)), ("cross", dict(x=x, z=z)), ("self_test", dict(z=z))):
            out["K_%s" % mode] = k.getCovMatrix(mode=mode, **kw)
            for i in range(len(k.hyp)):
                out["dK%d_%s" % (i, mode)] = k.getDerMatrix(mode=mode, der=i, **kw)
        save("G23_sm_kernels_" + nm, **out)


def fit300():
    x, y = series(300, 12.0, 3)
    xs = np.linspace(11, 14, 7).reshape(-1, 1)
    m = pyGPs.GPR()
    m.setPrior(mean=pyGPs.mean.Zero(), kernel=sm(*Q3))
    m.setNoise(np.log(0.1))
    m.setData(x, y)
    nlZ, dnlZ, post = m.getPosterior()
    ym, ys2, fm, fs2, lp = m.predict(xs)
    rec = dict(x=x, y=y, Q=3, nlZ=nlZ, alpha=post.alpha, L_diag=np.diag(post.L).copy(), cov_hyp=np.array(m.covfunc.hyp),
               lik_hyp=np.array(m.likfunc.hyp), pred_xs=xs, pred_ym=ym, pred_ys2=ys2, pred_fs2=fs2, **dn(dnlZ))
    m.optimize(x, y, numIterations=10)
    ym2, ys22, _, _, _ = m.predict(xs)
    rec.update(opt_iters=10, opt_nlZ=m.nlZ, opt_hyp=np.array(m.covfunc.hyp + m.likfunc.hyp), opt_ym=ym2, opt_ys2=ys22)
    save("G23_sm_fit_N300", **rec)


def fit2048():
    x, y = series(2048, 30.0, 4)
    xs = np.linspace(28, 32, 9).reshape(-1, 1)
    m = pyGPs.GPR()
    m.setPrior(mean=pyGPs.mean.Zero(), kernel=sm(*Q3))
    m.setNoise(np.log(0.1))
    m.setData(x, y)
    nlZ, dnlZ, post = m.getPosterior()
    ym, ys2, fm, fs2, lp = m.predict(xs)
    save("G23_sm_fit_N2048", x=x, y=y, Q=3, nlZ=nlZ, alpha_16=post.alpha[::16].copy(), cov_hyp=np.array(m.covfunc.hyp),
         lik_hyp=np.array(m.likfunc.hyp), pred_xs=xs, pred_ym=ym, pred_ys2=ys2, pred_fs2=fs2, **dn(dnlZ))


def cls_data():
    rng = np.random.RandomState(5)
    x = np.sort(rng.uniform(0, 10, (200, 1)), axis=0)
    y = np.sign(np.sin(2 * np.pi * 0.4 * x) + 0.4 * rng.randn(200, 1))
    y[y == 0] = 1
    return x, y, np.linspace(9, 11, 5).reshape(-1, 1)


def ep200():
    x, y, xs = cls_data()
    m = pyGPs.GPC()
    m.inffunc.logger = logging.getLogger("reference.EP")
    m.setPrior(kernel=sm(*Q2))
    nlZ, dnlZ, post = m.getPosterior(x, y)
    ym, ys2, fm, fs2, lp = m.predict(xs, ys=np.ones((5, 1)))
    save("G23_sm_ep_N200", x=x, y=y, Q=2, nlZ=nlZ, alpha=post.alpha, sW=post.sW, cov_hyp=np.array(m.covfunc.hyp),
         pred_xs=xs, pred_ym=ym, pred_fs2=fs2, pred_lp=lp, **dn(dnlZ))


def laplace200():
    x, y, xs = cls_data()
    m = pyGPs.GPC()
    m.useInference("Laplace")
    m.setPrior(kernel=sm(*Q2))
    nlZ, dnlZ, post = m.getPosterior(x, y)
    ym, ys2, fm, fs2, lp = m.predict(xs, ys=np.ones((5, 1)))
    save("G23_sm_laplace_N200", x=x, y=y, Q=2, nlZ=nlZ, alpha=post.alpha, sW=post.sW, cov_hyp=np.array(m.covfunc.hyp),
         pred_xs=xs, pred_ym=ym, pred_fs2=fs2, pred_lp=lp, **dn(dnlZ))


def fitc1500():
    x, y = series(1500, 30.0, 6)
    rng = np.random.RandomState(7)
    u = np.linspace(0, 30, 160).reshape(-1, 1) + 0.01 * rng.randn(160, 1)
    m = pyGPs.GPR_FITC()
    m.setData(x, y)
    m.setPrior(mean=pyGPs.mean.Zero(), kernel=sm(*Q2), inducing_points=u)
    m.setNoise(np.log(0.1))
    nlZ, dnlZ, post = m.getPosterior()
    xt = np.linspace(1, 31, 6).reshape(-1, 1)
    ym, ys2, fm, fs2, lp = m.predict(xt)
    save("G23_sm_fitc_N1500_nu160", x=x, y=y, Q=2, u=u, nlZ=nlZ, alpha=post.alpha, L=post.L, cov_hyp=np.array(m.covfunc.hyp),
         lik_hyp=np.array(m.likfunc.hyp), pred_xs=xt, pred_ym=ym, pred_fs2=fs2, **dn(dnlZ))


ALL = dict(kernels=kernels, fit300=fit300, fit2048=fit2048, ep200=ep200, laplace200=laplace200, fitc1500=fitc1500)

if __name__ == "__main__":
    for name in (sys.argv[1:] or list(ALL)):
        ALL[name]()
