#!/usr/bin/env python3
"""Generate the G22 golden vectors (lik.Laplace with EP) under tests/golden/ by importing the REFERENCE
(marionmari/pyGPs, read-only at /root/reference) in the build container.

Run by hand, here only:

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lik_laplace.py [ids...]

Same set-up as make_golden_laplace.py (the `past` shim in tests/golden/_shim, pyGPs imported unmodified, `cmp` in the
reference's tools module rebound for numpy bools; no reference source is copied).  EP gets a `logger`, which the reference's
EP.evaluate uses at 10 sweeps without ever setting it.  The sweeps are counted from the likelihood's per-site calls
(nargout = 3, one per site and sweep, Core/inf.py:762).

What the reference cannot evaluate is not recorded: value mode in the "idlik" regime (IndexError) and anything in the
"idgau" regime (TypeError).  Its mean gradient with lik.Laplace takes the first site's dlZ for every site (recorded as is;
the tests compare the device's mean gradient with central differences instead).

FITC: GPR_FITC.useLikelihood("Laplace") with FITC_EP; FITC_EP gets a `logger` too.  Its sweeps are counted the same way.

Reference call sites exercised: Core/gp.py:624-635, 1104-1114 (GPR / GPR_FITC.useLikelihood), Core/inf.py:723-806
(EP.evaluate), 174-189 (_epComputeParams), 810-944 (FITC_EP.evaluate), Core/lik.py:370-580 (Laplace).
"""
import logging
import os
import sys
import time

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "_shim"))
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import scipy  # noqa: E402
import pyGPs  # noqa: E402  (the reference)
import pyGPs.Core.inf as ref_inf  # noqa: E402
import pyGPs.Core.lik as ref_lik  # noqa: E402
import pyGPs.Core.tools as ref_tools  # noqa: E402

ref_tools.cmp = lambda a, b: int(a > b) - int(a < b)

META = dict(numpy=np.__version__, scipy=scipy.__version__,
            reference="marionmari/pyGPs v1.3.5 @ /root/reference", note="Core.tools.cmp rebound (numpy bools); EP.logger set")


class Count(object):
    sites = 0


_orig_eval = ref_lik.Laplace.evaluate


def _counting(self, y=None, mu=None, s2=None, inffunc=None, der=None, nargout=1):
    if isinstance(inffunc, ref_inf.EP) and der is None and nargout == 3:
        Count.sites += 1
    return _orig_eval(self, y, mu, s2, inffunc, der, nargout)


ref_lik.Laplace.evaluate = _counting


def save(name, **arrs):
    arrs["meta"] = np.array(repr(META))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrs)
    print("wrote", name, os.path.getsize(os.path.join(HERE, name + ".npz")), "bytes", flush=True)


def ep():
    f = ref_inf.EP()
    f.logger = logging.getLogger("reference.EP")
    return f


def model(x, y, zero_mean=False):
    m = pyGPs.GPR()
    m.useLikelihood("Laplace")
    m.inffunc = ep()
    if zero_mean:
        m.setPrior(mean=pyGPs.mean.Zero())
    m.setData(x, y)
    return m


def synth_t(N, d=3, seed=0):
    """Regression data with Student-t (3 degrees of freedom) noise: outliers for the robust likelihood."""
    rng = np.random.RandomState(seed)
    x = rng.randn(N, d)
    w = rng.randn(d, 1)
    y = np.sin(x @ w / np.sqrt(d)) + 0.1 * rng.standard_t(3, size=(N, 1))
    return x, y


def dn(d):
    return dict(dnlZ_mean=np.array(d.mean, dtype=float), dnlZ_cov=np.array(d.cov, dtype=float),
                dnlZ_lik=np.array(d.lik, dtype=float))


def fit(m, n):
    Count.sites = 0
    nlZ, dnlZ, post = m.getPosterior()
    sweeps = Count.sites // n
    assert Count.sites == sweeps * n
    return dict(nlZ=nlZ, sweeps=sweeps, ttau=m.inffunc.last_ttau.copy(), tnu=m.inffunc.last_tnu.copy(), alpha=post.alpha,
                sW=post.sW, L_diag=np.diag(post.L).copy(), mean_hyp=np.array(m.meanfunc.hyp, dtype=float),
                cov_hyp=np.array(m.covfunc.hyp, dtype=float), lik_hyp=np.array(m.likfunc.hyp, dtype=float), **dn(dnlZ))


def moments():
    """Per-site moments (scalar calls, as EP makes them) on a grid over the interior, and dlZhyp (one vector call) over the
    interior and the idlik regime."""
    rng = np.random.RandomState(3)
    k = 400
    sn = np.exp(rng.uniform(np.log(1e-2), np.log(3.0), k))
    s2 = sn ** 2 * np.exp(rng.uniform(np.log(2e-6), np.log(5e5), k))     # sqrt(s2) / sn from 1.4e-3 to 7e2: interior
    y = rng.randn(k)
    z = rng.uniform(-40, 40, k)                                           # (mu - y) / sqrt(s2)
    mu = y + z * np.sqrt(s2)
    lZ, dlZ, d2lZ, dh = (np.zeros(k) for _ in range(4))
    for i in range(k):
        L = ref_lik.Laplace(np.log(sn[i]))
        a = L.evaluate(np.array([y[i]]), np.array([mu[i]]), np.array([s2[i]]), ref_inf.EP(), None, 3)
        lZ[i], dlZ[i], d2lZ[i] = [float(np.ravel(v)[0]) for v in a]
        dh[i] = float(np.ravel(L.evaluate(np.array([y[i]]), np.array([mu[i]]), np.array([s2[i]]), ref_inf.EP(), 0))[0])
    # idlik: dlZhyp only (value mode raises in the reference)
    kl = 40
    sl = 0.05
    s2l = (sl * 1e3) ** 2 * np.exp(rng.uniform(0.01, 3.0, kl))
    yl = rng.randn(kl)
    mul = yl + rng.randn(kl) * np.sqrt(s2l)
    L = ref_lik.Laplace(np.log(sl))
    dhl = np.ravel(L.evaluate(yl.reshape(-1, 1), mul.reshape(-1, 1), s2l.reshape(-1, 1), ref_inf.EP(), 0))
    save("G22_lik_laplace_moments", y=y, mu=mu, s2=s2, sn=sn, lZ=lZ, dlZ=dlZ, d2lZ=d2lZ, dlZhyp=dh,
         idlik_y=yl, idlik_mu=mul, idlik_s2=s2l, idlik_sn=np.array(sl), idlik_dlZhyp=dhl)


def demo():
    data = np.load("/root/reference/pyGPs/Demo/Regression/regression_data.npz")
    x, y, xs = data["x"], data["y"], data["xstar"]
    m = model(x, y)
    out = dict(x=x, y=y, xstar=xs, **fit(m, x.shape[0]))
    ym, ys2, fm, fs2, lp = m.predict(xs, ys=np.sin(xs))
    out.update(pred_ym=ym, pred_ys2=ys2, pred_fm=fm, pred_fs2=fs2, pred_lp=lp)
    m2 = model(x, y)
    t0 = time.time()
    m2.optimize()
    ym2, ys22, fm2, fs22, lp2 = m2.predict(xs, ys=np.sin(xs))
    print("   optimize %.1f s" % (time.time() - t0), flush=True)
    out.update(opt_nlZ=m2.nlZ, opt_mean_hyp=np.array(m2.meanfunc.hyp), opt_cov_hyp=np.array(m2.covfunc.hyp),
               opt_lik_hyp=np.array(m2.likfunc.hyp), opt_ym=ym2, opt_ys2=ys22, opt_fm=fm2, opt_fs2=fs22, opt_lp=lp2)
    save("G22_lik_laplace_demo", **out)


def synth(N, zero_mean=False, sample=None):
    x, y = synth_t(N)
    m = model(x, y, zero_mean)
    m.covfunc.hyp = [np.log(1.3), np.log(0.9)]
    m.likfunc.hyp = [np.log(0.15)]
    r = fit(m, N)
    xs = np.random.RandomState(5).randn(50, x.shape[1])
    ym, ys2, fm, fs2, lp = m.predict(xs, ys=np.sin(xs[:, :1]))
    out = dict(x=x, y=y, pred_xs=xs, pred_ym=ym, pred_ys2=ys2, pred_fm=fm, pred_fs2=fs2, pred_lp=lp, **r)
    save("G22_lik_laplace_%s_N%d" % ("zero" if zero_mean else "const", N), **out)


def warm():
    """A warm-start pair: the second fit starts from the first one's site parameters (inf.py:744-753), once where they are
    kept and once where the zero start wins."""
    x, y = synth_t(200, seed=1)
    m = model(x, y)
    r1 = fit(m, 200)
    m.covfunc.hyp = [np.log(1.2), np.log(1.1)]
    r2 = fit(m, 200)                                  # nearby: warm start kept
    m.covfunc.hyp = [np.log(0.05), np.log(8.0)]
    m.likfunc.hyp = [np.log(2.0)]
    r3 = fit(m, 200)                                  # far away
    out = dict(x=x, y=y)
    for tag, r in (("a", r1), ("b", r2), ("c", r3)):
        out.update({tag + "_" + k: v for k, v in r.items()})
    save("G22_lik_laplace_warm_N200", **out)


def fitc(N, nu, zero_mean, d=4):
    x, y = synth_t(N, d, seed=4)
    u = np.random.RandomState(6).randn(nu, d)
    m = pyGPs.GPR_FITC()
    m.useLikelihood("Laplace")
    f = ref_inf.FITC_EP()
    f.logger = logging.getLogger("reference.FITC_EP")
    m.inffunc = f
    m.setPrior(kernel=pyGPs.cov.RBF(np.log(1.4), np.log(0.9)), inducing_points=u)
    if zero_mean:
        m.setPrior(mean=pyGPs.mean.Zero())
    m.setData(x, y)
    m.likfunc.hyp = [np.log(0.15)]
    Count.sites = 0
    t0 = time.time()
    nlZ, dnlZ, post = m.getPosterior(x, y)
    secs = time.time() - t0
    sweeps = Count.sites // N
    assert Count.sites == sweeps * N
    xs = np.random.RandomState(5).randn(50, d)
    ym, ys2, fm, fs2, lp = m.predict(xs, ys=np.sin(xs[:, :1]))
    L = np.asarray(post.L)
    save("G22_fitc_lik_laplace_%s_N%d_nu%d" % ("zero" if zero_mean else "const", N, nu), x=x, y=y, u=u, nlZ=nlZ, sweeps=sweeps,
         ttau=m.inffunc.last_ttau, tnu=m.inffunc.last_tnu, mean_hyp=np.array(m.meanfunc.hyp, dtype=float),
         cov_hyp=np.array(m.covfunc.hyp, dtype=float), lik_hyp=np.array(m.likfunc.hyp, dtype=float), alpha=post.alpha,
         L_diag=np.diag(L).copy(), L_stride=97, L_sample=L.ravel()[::97].copy(), ref_seconds=secs, pred_xs=xs, pred_ym=ym,
         pred_ys2=ys2, pred_fm=fm, pred_fs2=fs2, pred_lp=lp, **dn(dnlZ))


JOBS = dict(moments=moments, demo=demo, warm=warm, fitc_const_1500=lambda: fitc(1500, 100, False),
            const_200=lambda: synth(200), zero_200=lambda: synth(200, True), const_1000=lambda: synth(1000))

if __name__ == "__main__":
    for j in (sys.argv[1:] or list(JOBS)):
        t0 = time.time()
        JOBS[j]()
        print("%s: %.1f s" % (j, time.time() - t0), flush=True)
