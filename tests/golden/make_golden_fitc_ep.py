#!/usr/bin/env python3
"""Generate the G21 golden vectors (FITC_EP inference, GPC_FITC) under tests/golden/ by importing the REFERENCE
(marionmari/pyGPs, read-only at /root/reference) in the build container.

Run by hand, here only:

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fitc_ep.py [ids...]

Same set-up as make_golden_laplace.py (the `past` shim in tests/golden/_shim, pyGPs imported unmodified, plain arrays
stored).  Two things are added from outside, no reference source is copied:
- FITC_EP.__init__ never sets self.logger, so a call that reaches 10 sweeps raises AttributeError (inf.py:897-898).  Every
  FITC_EP instance used here gets a logger attribute; the fixtures are chosen so that no call reaches 10 sweeps (the
  recorded sweep counts say so).
- Inference._epfitcUpdate and _epfitcRefresh are wrapped to count site updates and refreshes: sweeps = updates / n, and a
  warm start that fell back to zero costs one refresh more (inf.py:866-872).

Reference call sites exercised: Core/gp.py:934-983 (GP_FITC.setData), 1117-1202 (GPC_FITC), Core/inf.py:235-297
(_epfitcZ / Refresh / Update), 810-944 (FITC_EP.evaluate), Core/cov.py:332-390 (FITCOfKernel).
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

META = dict(numpy=np.__version__, scipy=scipy.__version__,
            reference="marionmari/pyGPs v1.3.5 @ /root/reference", note="FITC_EP.logger set; updates/refreshes counted")


class Count(object):
    upd = 0
    ref = 0


_orig_upd = ref_inf.Inference._epfitcUpdate
_orig_ref = ref_inf.Inference._epfitcRefresh


def _upd(self, *a):
    Count.upd += 1
    return _orig_upd(self, *a)


def _ref(self, *a):
    Count.ref += 1
    return _orig_ref(self, *a)


ref_inf.Inference._epfitcUpdate = _upd
ref_inf.Inference._epfitcRefresh = _ref


def fitc_ep():
    f = ref_inf.FITC_EP()
    f.logger = logging.getLogger("reference.FITC_EP")
    return f


def counted(fn, n):
    Count.upd = Count.ref = 0
    out = fn()
    sweeps = Count.upd // n
    assert Count.upd == sweeps * n
    return out, sweeps, Count.ref - sweeps     # refreshes before the first sweep: 1 (cold / warm kept) or 2 (warm rejected)


def save(name, **arrs):
    arrs["meta"] = np.array(repr(META))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrs)
    print("wrote", name, os.path.getsize(os.path.join(HERE, name + ".npz")), "bytes", flush=True)


def synth_cls(N, d, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.randn(N, d)
    w = rng.randn(d, 1)
    y = np.sign(x @ w / np.sqrt(d) + 0.3 * rng.randn(N, 1))
    y[y == 0] = 1
    return x, y


def inducing(nu, d, seed=1):
    return np.random.RandomState(seed).randn(nu, d)


def dn(d):
    return dict(dnlZ_mean=np.array(d.mean, dtype=float), dnlZ_cov=np.array(d.cov, dtype=float),
                dnlZ_lik=np.array(d.lik, dtype=float))


def post_arrays(post, nu):
    L = np.asarray(post.L)
    out = dict(alpha=post.alpha, sW=post.sW, L_diag=np.diag(L).copy())
    if nu <= 64:
        out["L"] = L
    else:                                      # strided sample of the flattened L, like G20
        out.update(L_stride=97, L_sample=L.ravel()[::97].copy())
    return out


def demo():
    data = np.load("/root/reference/pyGPs/Demo/Classification/classification_data.npz")
    x, y, xs = data["x"], data["y"], data["xstar"]
    m = pyGPs.GPC_FITC()
    m.inffunc = fitc_ep()
    m.setData(x, y)
    (nlZ, dnlZ, post), sweeps, _ = counted(lambda: m.getPosterior(), x.shape[0])
    ttau, tnu = m.inffunc.last_ttau.copy(), m.inffunc.last_tnu.copy()
    ym, ys2, fm, fs2, lp = m.predict(xs, ys=np.ones((xs.shape[0], 1)))
    out = dict(x=x, y=y, xstar=xs, u=m.u, nlZ=nlZ, sweeps=sweeps, ttau=ttau, tnu=tnu, mean_hyp=np.array(m.meanfunc.hyp),
               cov_hyp=np.array(m.covfunc.hyp), alpha=post.alpha, L=post.L, sW=post.sW, pred_ym=ym, pred_ys2=ys2,
               pred_fm=fm, pred_fs2=fs2, pred_lp=lp, **dn(dnlZ))
    m2 = pyGPs.GPC_FITC()
    m2.inffunc = fitc_ep()
    m2.setData(x, y)
    t0 = time.time()
    m2.optimize()
    ym2, ys22, fm2, fs22, lp2 = m2.predict(xs[::81], ys=np.ones((xs[::81].shape[0], 1)))
    print("   optimize %.1f s" % (time.time() - t0), flush=True)
    out.update(opt_nlZ=m2.nlZ, opt_mean_hyp=np.array(m2.meanfunc.hyp), opt_cov_hyp=np.array(m2.covfunc.hyp),
               opt_xs=xs[::81], opt_ym=ym2, opt_fs2=fs22, opt_lp=lp2)
    save("G21_fitc_ep_demo", **out)


def kernel(name, d):
    cov = pyGPs.cov
    if name == "rbf":
        return cov.RBF(np.log(np.sqrt(d)), 0.0)
    if name == "rbfard":
        return cov.RBFard(log_ell_list=list(np.log(np.sqrt(d)) + np.linspace(-0.3, 0.3, d)), log_sigma=0.2)
    if name == "matern5":
        return cov.Matern(np.log(np.sqrt(d)), d=5, log_sigma=0.1)
    if name == "sum":
        return cov.RBF(np.log(np.sqrt(d)) + 0.3, -0.2) + cov.Matern(np.log(np.sqrt(d)), d=3, log_sigma=-0.5)
    raise KeyError(name)


def synth(name, N, nu, d=4):
    x, y = synth_cls(N, d)
    u = inducing(nu, d)
    m = pyGPs.GPC_FITC()
    m.inffunc = fitc_ep()
    m.setPrior(mean=pyGPs.mean.Zero(), kernel=kernel(name, d), inducing_points=u)
    m.setData(x, y)
    t0 = time.time()
    (nlZ, dnlZ, post), sweeps, _ = counted(lambda: m.getPosterior(x, y), N)
    secs = time.time() - t0
    print("   %s N=%d nu=%d: %d sweeps, %.1f s" % (name, N, nu, sweeps, secs), flush=True)
    xs = x[:64] + 0.05
    ym, ys2, fm, fs2, lp = m.predict(xs, ys=np.ones((64, 1)))
    save("G21_fitc_ep_%s_N%d_nu%d" % (name, N, nu), N=N, nu=nu, d=d, seed=0, u=u, nlZ=nlZ, sweeps=sweeps,
         ttau=m.inffunc.last_ttau, tnu=m.inffunc.last_tnu, cov_hyp=np.array(m.covfunc.hyp), ref_seconds=secs,
         pred_xs=xs, pred_ym=ym, pred_ys2=ys2, pred_fm=fm, pred_fs2=fs2, pred_lp=lp, **post_arrays(post, nu), **dn(dnlZ))


def warm():
    """One model, three calls: cold at h0, warm at h1 near h0 (the previous sites are kept), warm at h2 with the labels
    flipped (the previous sites are worse than zero and are dropped)."""
    d, N, nu = 4, 512, 64
    x, y = synth_cls(N, d, seed=3)
    u = inducing(nu, d, seed=4)
    hyps = [[np.log(2.0), 0.0], [np.log(2.0) + 0.05, 0.02], [np.log(2.0), 0.5]]
    m = pyGPs.GPC_FITC()
    m.inffunc = fitc_ep()
    m.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(*hyps[0]), inducing_points=u)
    m.setData(x, y)
    out = dict(x=x, y=y, u=u, hyps=np.array(hyps), flip=np.array([0, 0, 1]))
    for k, h in enumerate(hyps):
        m.covfunc.hyp = list(h)
        yk = -y if k == 2 else y
        (nlZ, dnlZ, post), sweeps, pre = counted(lambda: m.getPosterior(x, yk), N)
        print("   call %d: %d sweeps, %d initial refreshes" % (k, sweeps, pre), flush=True)
        out.update({"nlZ%d" % k: nlZ, "sweeps%d" % k: sweeps, "pre_refresh%d" % k: pre, "ttau%d" % k: m.inffunc.last_ttau.copy(),
                    "tnu%d" % k: m.inffunc.last_tnu.copy(), "alpha%d" % k: post.alpha, "dnlZ_cov%d" % k: np.array(dnlZ.cov)})
    save("G21_fitc_ep_warm_N512_nu64", **out)


def const_mean():
    d, N, nu = 3, 300, 30
    x, y = synth_cls(N, d, seed=5)
    u = inducing(nu, d, seed=6)
    m = pyGPs.GPC_FITC()
    m.inffunc = fitc_ep()
    m.setPrior(mean=pyGPs.mean.Const(0.3), kernel=pyGPs.cov.RBF(np.log(1.5), 0.3), inducing_points=u)
    m.setData(x, y)
    (nlZ, dnlZ, post), sweeps, _ = counted(lambda: m.getPosterior(x, y), N)
    xs = x[:32] + 0.05
    ym, ys2, fm, fs2, lp = m.predict(xs, ys=np.ones((32, 1)))
    save("G21_fitc_ep_const_mean_N300_nu30", x=x, y=y, u=u, nlZ=nlZ, sweeps=sweeps, ttau=m.inffunc.last_ttau,
         tnu=m.inffunc.last_tnu, mean_hyp=np.array(m.meanfunc.hyp), cov_hyp=np.array(m.covfunc.hyp), pred_xs=xs, pred_ym=ym,
         pred_fm=fm, pred_fs2=fs2, pred_lp=lp, **post_arrays(post, nu), **dn(dnlZ))


JOBS = dict(demo=demo, warm=warm, const_mean=const_mean,
            rbf_128=lambda: synth("rbf", 128, 25), rbf_1500=lambda: synth("rbf", 1500, 160),
            rbfard_1500=lambda: synth("rbfard", 1500, 160), matern5_1500=lambda: synth("matern5", 1500, 160),
            sum_1500=lambda: synth("sum", 1500, 160), rbf_4096=lambda: synth("rbf", 4096, 256))

if __name__ == "__main__":
    for j in (sys.argv[1:] or list(JOBS)):
        t0 = time.time()
        JOBS[j]()
        print("%s: %.1f s" % (j, time.time() - t0), flush=True)
