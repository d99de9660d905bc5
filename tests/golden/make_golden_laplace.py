#!/usr/bin/env python3
"""Generate the G20 golden vectors (Laplace inference) under tests/golden/ by importing the REFERENCE
(marionmari/pyGPs, read-only at /root/reference) in the build container.

Run by hand, here only:

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_laplace.py [ids...]

Same set-up as make_golden.py (the `past` shim in tests/golden/_shim, pyGPs imported unmodified, plain arrays stored).
One thing differs: the reference's line search (Core/tools.py brentmin) calls `cmp`, which the shim defines for
plain numbers only; under numpy >= 1.13 it fails on the numpy bools that reach it.  After import, `cmp` in the
reference's tools module is rebound to a three-way comparison that accepts them -- no reference source is copied.
`Core.inf.brentmin` is wrapped to record every Newton step's step size s, objective Psi and number of evaluations.

Reference call sites exercised: Core/gp.py:611-622, 708-717 (useInference), Core/inf.py:459-564 (Laplace.evaluate),
Core/lik.py:175-197 (Gauss, Laplace mode), 274-293 (Erf, Laplace mode), Core/tools.py:121-272 (brentmin).
"""
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
import pyGPs.Core.tools as ref_tools  # noqa: E402

ref_tools.cmp = lambda a, b: int(a > b) - int(a < b)

META = dict(numpy=np.__version__, scipy=scipy.__version__,
            reference="marionmari/pyGPs v1.3.5 @ /root/reference", note="Core.tools.cmp rebound (numpy bools)")


def save(name, **arrs):
    arrs["meta"] = np.array(repr(META))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrs)
    print("wrote", name, flush=True)


def synth_reg(N, d, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.randn(N, d)
    w = rng.randn(d, 1)
    y = np.sin(x @ w / np.sqrt(d)) + 0.1 * rng.randn(N, 1)
    return x, y


def synth_cls(N, d, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.randn(N, d)
    w = rng.randn(d, 1)
    y = np.sign(x @ w / np.sqrt(d) + 0.3 * rng.randn(N, 1))
    y[y == 0] = 1
    return x, y


def dn(d):
    return dict(dnlZ_mean=np.array(d.mean, dtype=float), dnlZ_cov=np.array(d.cov, dtype=float),
                dnlZ_lik=np.array(d.lik, dtype=float))


class Steps(object):
    """Wraps Core.inf.brentmin: per Newton step (s, Psi, function evaluations)."""

    def __init__(self):
        self.s, self.psi, self.nfun = [], [], []
        self.orig = ref_inf.brentmin

    def __enter__(self):
        def spy(*a, **k):
            out = self.orig(*a, **k)
            self.s.append(float(np.asarray(out[0]).ravel()[0]))
            self.psi.append(float(np.asarray(out[1]).ravel()[0]))
            self.nfun.append(int(out[2]))
            return out
        ref_inf.brentmin = spy
        return self

    def __exit__(self, *exc):
        ref_inf.brentmin = self.orig

    def arrays(self):
        return dict(step_s=np.array(self.s), step_psi=np.array(self.psi), step_nfun=np.array(self.nfun, dtype=np.int64),
                    newton_steps=len(self.s))


# ----------------------------------------------------------------------------- likelihood modes
def lik_modes():
    lap = ref_inf.Laplace()
    f = np.concatenate([np.linspace(-40, 40, 321), np.linspace(-6.3, -4.9, 57), -np.linspace(-6.3, -4.9, 57),
                        np.array([0.0, 1e-8, -1e-8, 5.5, -5.5, 6.0, -6.0, 6.2, -6.2])]).reshape(-1, 1)
    n = f.shape[0]
    out = dict(f=f)
    for tag, yv in (("pos", 1.0), ("neg", -1.0)):
        y = yv * np.ones((n, 1))
        lp, dlp, d2lp, d3lp = pyGPs.lik.Erf().evaluate(y, f, None, lap, None, 4)
        out.update({"erf_%s_lp" % tag: lp, "erf_%s_dlp" % tag: dlp, "erf_%s_d2lp" % tag: d2lp, "erf_%s_d3lp" % tag: d3lp})
    out["erf_der"] = np.array(len(pyGPs.lik.Erf().evaluate(np.ones((n, 1)), f, None, lap, 0, 3)))
    yg = np.sin(f) + 0.3
    g = pyGPs.lik.Gauss(np.log(0.3))
    lp, dlp, d2lp, d3lp = g.evaluate(yg, f, None, lap, None, 4)
    a, b, c = g.evaluate(yg, f, None, lap, 0, 3)
    out.update(gauss_y=yg, gauss_log_sn=np.array(np.log(0.3)), gauss_lp=lp, gauss_dlp=dlp, gauss_d2lp=d2lp, gauss_d3lp=d3lp,
               gauss_lp_dhyp=a, gauss_dlp_dhyp=b, gauss_d2lp_dhyp=c)
    save("G20_lik_laplace_modes", **out)


# ----------------------------------------------------------------------------- fits
def demo():
    data = np.load("/root/reference/pyGPs/Demo/Classification/classification_data.npz")
    x, y, xs = data["x"], data["y"], data["xstar"]
    m = pyGPs.GPC()
    m.useInference("Laplace")
    with Steps() as st:
        nlZ, dnlZ, post = m.getPosterior(x, y)
    ym, ys2, fm, fs2, lp = m.predict(xs[:5])
    save("G20_laplace_demo", x=x, y=y, xstar5=xs[:5], nlZ=nlZ, alpha=post.alpha, L=post.L, sW=post.sW,
         cov_hyp=np.array(m.covfunc.hyp), pred_ym=ym, pred_ys2=ys2, pred_fm=fm, pred_fs2=fs2, **st.arrays(), **dn(dnlZ))


def d32(N):
    d = 32
    x, y = synth_cls(N, d)
    m = pyGPs.GPC()
    m.useInference("Laplace")
    m.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(np.log(np.sqrt(d)), 0.0))
    t0 = time.time()
    with Steps() as st:
        nlZ, dnlZ, post = m.getPosterior(x, y)
    print("   N=%d: %d Newton steps, %.1f s" % (N, len(st.s), time.time() - t0), flush=True)
    extra = {}
    if N > 512:     # strided L sample of the flattened upper factor, like G6 / G8ii: every 257th entry, every 4112th (= 16 x 257)
        stride = 257 if N <= 4096 else 4112     # at N = 8192, where 257 would make a 2 MB fixture
        extra = dict(L_stride=stride, L_sample=np.asarray(post.L).ravel()[::stride].copy())
    save("G20_laplace_d32_N%d" % N, N=N, d=d, seed=0, nlZ=nlZ, alpha=post.alpha, sW=post.sW,
         L_diag=np.diag(post.L).copy(), cov_hyp=np.array(m.covfunc.hyp), ref_seconds=time.time() - t0,
         **extra, **st.arrays(), **dn(dnlZ))


def const_mean():
    cov = pyGPs.cov
    x, y = synth_cls(200, 3)
    m = pyGPs.GPC()
    m.useInference("Laplace")
    m.setPrior(mean=pyGPs.mean.Const(0.3), kernel=cov.RBF(np.log(1.5), 0.3) * cov.RQ(0.6, 0.0, 0.2) + cov.Const(-1.0))
    with Steps() as st:
        nlZ, dnlZ, post = m.getPosterior(x, y)
    ym, ys2, fm, fs2, lp = m.predict(x[:5] + 0.05, ys=np.ones((5, 1)))
    save("G20_laplace_const_mean_N200", x=x, y=y, nlZ=nlZ, alpha=post.alpha, sW=post.sW, L_diag=np.diag(post.L).copy(),
         mean_hyp=np.array(m.meanfunc.hyp), cov_hyp=np.array(m.covfunc.hyp), pred_xs=x[:5] + 0.05, pred_ym=ym,
         pred_fs2=fs2, **st.arrays(), **dn(dnlZ))


def dense():
    cov = pyGPs.cov
    x, y = synth_cls(200, 3)
    m = pyGPs.GPC()
    m.useInference("Laplace")
    m.setPrior(kernel=cov.RBFard(log_ell_list=[0.4, 0.6, 0.5], log_sigma=0.3) * cov.RBFard(log_ell_list=[0.9, 0.8, 1.0], log_sigma=0.0)
               + cov.RBFard(log_ell_list=[1.1, 0.7, 0.9], log_sigma=-0.4))
    with Steps() as st:
        nlZ, dnlZ, post = m.getPosterior(x, y)
    ym, ys2, fm, fs2, lp = m.predict(x[:5] + 0.05, ys=np.ones((5, 1)))
    save("G20_laplace_dense_N200", x=x, y=y, nlZ=nlZ, alpha=post.alpha, sW=post.sW, L_diag=np.diag(post.L).copy(),
         cov_hyp=np.array(m.covfunc.hyp), pred_xs=x[:5] + 0.05, pred_ym=ym, pred_fs2=fs2, **st.arrays(), **dn(dnlZ))


def gauss():
    x, y = synth_reg(300, 4)
    out = {}
    for tag in ("laplace", "exact"):
        m = pyGPs.GPR()
        m.setPrior(kernel=pyGPs.cov.RBF(np.log(2.0), 0.1))
        m.setNoise(np.log(0.2))
        if tag == "laplace":
            m.useInference("Laplace")
        with Steps() as st:
            nlZ, dnlZ, post = m.getPosterior(x, y)
        out.update({"%s_nlZ" % tag: nlZ, "%s_alpha" % tag: post.alpha, "%s_sW" % tag: post.sW,
                    "%s_L_diag" % tag: np.diag(post.L).copy()})
        out.update({"%s_%s" % (tag, k): v for k, v in dn(dnlZ).items()})
        if tag == "laplace":
            out.update(st.arrays())
    save("G20_laplace_gauss_N300", x=x, y=y, cov_hyp=np.array([np.log(2.0), 0.1]), lik_hyp=np.array([np.log(0.2)]), **out)


def optimize():
    d = 8
    x, y = synth_cls(512, d)
    m = pyGPs.GPC()
    m.useInference("Laplace")
    m.setPrior(kernel=pyGPs.cov.RBF(np.log(np.sqrt(d)), 0.0))
    m.setData(x, y)
    t0 = time.time()
    m.optimize(numIterations=10)
    nlZ, dnlZ, post = m.getPosterior()
    print("   optimize: %.1f s" % (time.time() - t0), flush=True)
    save("G20_laplace_optimize_N512", x=x, y=y, d=d, iters=10, cov_hyp0=np.array([np.log(np.sqrt(d)), 0.0]),
         cov_hyp=np.array(m.covfunc.hyp), opt_nlZ=np.array(m.nlZ, dtype=float), nlZ=nlZ, alpha=post.alpha, **dn(dnlZ))


def warm():
    d = 8
    x, y = synth_cls(512, d)
    m = pyGPs.GPC()
    m.useInference("Laplace")
    m.setPrior(kernel=pyGPs.cov.RBF(np.log(np.sqrt(d)), 0.0))
    m.setData(x, y)
    with Steps() as st1:
        nlZ1, dnlZ1, post1 = m.getPosterior()
    hyp2 = np.array([np.log(np.sqrt(d)) + 0.2, 0.3])
    m.covfunc.hyp = list(hyp2)
    with Steps() as st2:
        nlZ2, dnlZ2, post2 = m.getPosterior()
    save("G20_laplace_warm_N512", x=x, y=y, d=d, cov_hyp1=np.array([np.log(np.sqrt(d)), 0.0]), cov_hyp2=hyp2,
         nlZ1=nlZ1, alpha1=post1.alpha, newton_steps1=len(st1.s),
         nlZ2=nlZ2, alpha2=post2.alpha, sW2=post2.sW, newton_steps2=len(st2.s), step_s2=np.array(st2.s),
         step_psi2=np.array(st2.psi), **{"second_" + k: v for k, v in dn(dnlZ2).items()})


CASES = {
    "lik": lik_modes, "demo": demo, "const_mean": const_mean, "dense": dense, "gauss": gauss, "optimize": optimize,
    "warm": warm, "d32_128": lambda: d32(128), "d32_512": lambda: d32(512), "d32_2048": lambda: d32(2048),
    "d32_4096": lambda: d32(4096), "d32_8192": lambda: d32(8192),
}

if __name__ == "__main__":
    ids = sys.argv[1:] or ["lik", "demo", "const_mean", "dense", "gauss", "optimize", "warm", "d32_128", "d32_512",
                           "d32_2048", "d32_4096"]
    for i in ids:
        t = time.time()
        CASES[i]()
        print("  %s done in %.1fs" % (i, time.time() - t), flush=True)
