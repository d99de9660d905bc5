#!/usr/bin/env python3
"""Generate the G27 golden vectors (the dot-product kernels cov.Linear, cov.Poly, cov.LINard) under tests/golden/ by importing
the REFERENCE (marionmari/pyGPs, read-only at /root/reference) in the build container.

Run by hand, here only:

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dot.py [kernels|fits|optimize|clustering|ep|laplace ...]

Same set-up as make_golden_laplace.py: the `past` shim in tests/golden/_shim, pyGPs imported unmodified, `cmp` in the reference's
tools module rebound for the Laplace line search, plain arrays stored.  No reference source is copied.

Reference call sites exercised: Core/cov.py:623-679 (Poly), 986-1024 (Linear), 1028-1074 (LINard, at hyp = 0 only: there the
reference and pygps_amd's definition coincide in every mode), 230-328 (Sum / Product / Scale), Core/inf.py:345-384 (Exact),
459-564 (Laplace), 731-806 (EP), Core/gp.py:349-437 (predict), Demo/Clustering/pyGP_extension.py:27-75.

Layout.  The kernel matrices are large against the 1 MiB cap on a committed file, so they are split: G27_dot_kernels_inputs.npz
holds x3 / z3 / x17 / z17 (n = 130, m = 70; d = 17 crosses one 16-coordinate stage) and <case>_hyp for every case;
G27_dot_k_<case>_d<d>_p<j>.npz hold up to SETS_PER_FILE matrix sets each, a set being K (key "K") or one derivative ("dK<i>") in
the three modes: "<key>_cross", "<key>_self" in full and "<key>_train_ut", the upper triangle of the symmetric 'train' matrix
(row-major, np.triu_indices(n)).  The script asserts that the reference's 'train' matrices are symmetric to 1e-15 of their largest
entry before it drops the lower triangle.

Every recorded fit asserts cond(K / sn2 + I) <= 1e7 (sn2 = 1 for the classifiers): with that cap the reference's own fp64 noise
(about cond * 1e-16) stays two orders below the bars the tests use.  Inputs are scaled down (halved) where Poly would exceed it.
The largest condition number is printed and written into every fit fixture's `meta`.
"""
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
            reference="marionmari/pyGPs v1.3.5 @ /root/reference", note="Core.tools.cmp rebound (numpy bools)")
COND_CAP = 1e7
WORST = dict(cond=0.0, where="")
SETS_PER_FILE = 5
cov = pyGPs.cov


def save(name, **arrs):
    meta = dict(META)
    meta["largest_cond"] = WORST["cond"]
    meta["largest_cond_fit"] = WORST["where"]
    arrs["meta"] = np.array(repr(meta))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrs)
    print("wrote", name, flush=True)


def ells(d):
    return [0.3 + 0.05 * k for k in range(d)]


# name -> kernel of the reference for input dimension d (tests/dot_ref_ld.py builds the same trees from pygps_amd classes)
CASES = {
    "linear": lambda d: cov.Linear(0.3),
    "poly1": lambda d: cov.Poly(-2.0, 1, -0.2),
    "poly2": lambda d: cov.Poly(-2.0, 2, -0.2),
    "poly3": lambda d: cov.Poly(-2.0, 3, -0.2),
    "poly5": lambda d: cov.Poly(-2.0, 5, -0.2),
    "linard": lambda d: cov.LINard(D=d),
    "lin_plus_rbf": lambda d: cov.Linear(0.3) + cov.RBF(0.4, 0.1),
    "lin_times_rbf": lambda d: cov.Linear(-0.2) * cov.RBF(0.7, 0.2),
    "half_lin_plus_rbf": lambda d: 0.5 * cov.Linear(0.1) + cov.RBF(0.3, -0.1),
    "poly_plus_rbfard": lambda d: cov.Poly(-1.0, 2, -0.3) + cov.RBFard(log_ell_list=ells(d), log_sigma=0.2),
    "lin_times_poly_plus_rbfard": lambda d: cov.Linear(0.2) * cov.Poly(-0.5, 3, -0.6) + cov.RBFard(log_ell_list=ells(d), log_sigma=0.2),
}


def n_der(name, k):
    return 3 if name.startswith("poly") and "_" not in name else len(k.hyp)     # plain Poly: der 2 ("the degree") gives zeros


def kernels():
    rng = np.random.RandomState(27)
    inputs = {}
    for d in (3, 17):
        x = rng.randn(130, d)
        z = rng.randn(70, d)
        inputs["x%d" % d], inputs["z%d" % d] = x, z
        iu = np.triu_indices(130)
        for name, make in CASES.items():
            k = make(d)
            inputs["%s_d%d_hyp" % (name, d)] = np.array(k.hyp, dtype=float)
            sets = [("K", None)] + [("dK%d" % i, i) for i in range(n_der(name, k))]
            for j in range(0, len(sets), SETS_PER_FILE):
                out = {}
                for key, der in sets[j:j + SETS_PER_FILE]:
                    for mode, kw in (("train", dict(x=x)), ("cross", dict(x=x, z=z)), ("self", dict(z=z))):
                        m = "self_test" if mode == "self" else mode
                        A = k.getCovMatrix(mode=m, **kw) if der is None else k.getDerMatrix(mode=m, der=der, **kw)
                        A = np.asarray(A, dtype=float)
                        if mode == "train":
                            assert np.max(np.abs(A - A.T)) <= 1e-15 * max(1.0, np.max(np.abs(A))), (name, key)
                            out[key + "_train_ut"] = A[iu].copy()
                        else:
                            out[key + "_" + mode] = A
                save("G27_dot_k_%s_d%d_p%d" % (name, d, j // SETS_PER_FILE), **out)
            if name in ("poly1", "poly2", "poly3", "poly5"):     # c is small enough that c + p < 0 occurs
                assert np.any(np.exp(k.hyp[0]) + x @ z.T < 0) and np.any(np.exp(k.hyp[0]) + x @ x.T < 0), (name, d)
    save("G27_dot_kernels_inputs", **inputs)


def dn(d):
    return dict(dnlZ_mean=np.array(d.mean, dtype=float), dnlZ_cov=np.array(d.cov, dtype=float),
                dnlZ_lik=np.array(d.lik, dtype=float))


def cond_ok(name, k, x, sn2):
    K = np.asarray(k.getCovMatrix(x=x, mode="train"), dtype=float)
    c = float(np.linalg.cond(K / sn2 + np.eye(x.shape[0])))
    return c


def reg_data(N, d, seed):
    rng = np.random.RandomState(seed)
    x = rng.randn(N, d)                                   # unit scale
    w = rng.randn(d, 1)
    y = np.sin(x @ w / np.sqrt(d)) + 0.3 * (x @ w) / np.sqrt(d) + 0.1 * rng.randn(N, 1)
    xs = rng.randn(130, d)
    xs[100:] *= 10.0                                      # ten times farther out: k(z, z) spans two orders of magnitude
    return x, y, xs


FITS = {
    # name: (kernel factory, d, mean)
    "lin_plus_rbf_d1": (lambda d: cov.Linear(0.2) + cov.RBF(0.5, 0.1), 1, None),
    "lin_plus_rbf_d3": (lambda d: cov.Linear(0.2) + cov.RBF(0.5, 0.1), 3, None),
    "lin_times_rbf": (lambda d: cov.Linear(-0.2) * cov.RBF(0.7, 0.2), 3, None),
    "half_lin_plus_rbf": (lambda d: 0.5 * cov.Linear(0.1) + cov.RBF(0.3, -0.1), 3, None),
    "linear": (lambda d: cov.Linear(0.3), 3, None),
    "poly3": (lambda d: cov.Poly(0.0, 3, -0.5), 3, None),
    "poly_plus_rbfard": (lambda d: cov.Poly(-1.0, 2, -0.3) + cov.RBFard(log_ell_list=ells(d), log_sigma=0.2), 3, None),
    "linard": (lambda d: cov.LINard(D=d), 3, None),
    "const_mean": (lambda d: cov.Linear(0.2) + cov.RBF(0.5, 0.1), 3, 0.4),
}
SN = 0.2


def fit(name):
    make, d, mean_c = FITS[name]
    x, y, xs = reg_data(300, d, seed=270 + sorted(FITS).index(name))
    scale = 1.0
    while True:
        c = cond_ok(name, make(d), x * scale, SN * SN)
        if c <= COND_CAP:
            break
        scale *= 0.5                                      # Poly: the inputs are scaled down until the cap holds
    x, xs = x * scale, xs * scale
    if c > WORST["cond"]:
        WORST["cond"], WORST["where"] = c, name
    print("   %s: cond(K / sn2 + I) = %.3g, input scale %g" % (name, c, scale), flush=True)
    m = pyGPs.GPR()
    if mean_c is None:
        m.setPrior(kernel=make(d))
    else:
        m.setPrior(mean=pyGPs.mean.Const(mean_c), kernel=make(d))
    m.setNoise(np.log(SN))
    m.setData(x, y)
    nlZ, dnlZ, post = m.getPosterior()
    ym, ys2, fm, fs2, lp = m.predict(xs)
    kss = np.asarray(m.covfunc.getCovMatrix(z=xs, mode="self_test"), dtype=float)
    assert kss.max() / kss.min() >= 100.0, name         # k(z, z) spans two orders of magnitude
    save("G27_dot_fit_" + name, x=x, y=y, pred_xs=xs, cond=np.array(c), input_scale=np.array(scale),
         cov_hyp=np.array(m.covfunc.hyp, dtype=float), lik_hyp=np.array(m.likfunc.hyp, dtype=float),
         mean_hyp=np.array(m.meanfunc.hyp, dtype=float), nlZ=np.array(nlZ, dtype=float), alpha=post.alpha,
         L_diag=np.diag(post.L).copy(), pred_ym=ym, pred_ys2=ys2, pred_fm=fm, pred_fs2=fs2, kss=kss, **dn(dnlZ))


def fits():
    for name in FITS:
        fit(name)
    print("largest cond(K / sn2 + I): %.4g (%s)" % (WORST["cond"], WORST["where"]), flush=True)


def optimize():
    x, y, xs = reg_data(100, 3, seed=290)
    k = cov.Linear(0.2) + cov.RBF(0.5, 0.1)
    c = cond_ok("optimize", k, x, SN * SN)
    assert c <= COND_CAP
    if c > WORST["cond"]:
        WORST["cond"], WORST["where"] = c, "optimize"
    m = pyGPs.GPR()
    m.setPrior(kernel=k)
    m.setNoise(np.log(SN))
    m.setData(x, y)
    hyp0 = np.array(m.covfunc.hyp, dtype=float)
    m.optimize(x, y, numIterations=15)
    ym = m.predict(xs)[0]
    c2 = cond_ok("optimize", m.covfunc, x, float(np.exp(2 * m.likfunc.hyp[0])))
    assert c2 <= COND_CAP
    save("G27_dot_optimize_N100", x=x, y=y, pred_xs=xs, iters=15, cov_hyp0=hyp0, lik_hyp0=np.array([np.log(SN)]), cond=np.array(max(c, c2)),
         cov_hyp=np.array(m.covfunc.hyp, dtype=float), lik_hyp=np.array(m.likfunc.hyp, dtype=float),
         opt_nlZ=np.array(m.nlZ, dtype=float), opt_ym=ym)


def clustering():
    """Demo/Clustering: the accumulated likelihood of one model over several series that share the hypers."""
    import pyGPs.Demo.Clustering.pyGP_extension as ext
    rng = np.random.RandomState(275)
    xs, ys = [], []
    for s in range(3):
        x = np.sort(rng.uniform(0.0, 5.0, (80, 1)), axis=0)
        y = 0.4 * x + np.sin(2.0 * x + 0.3 * s) + 0.1 * rng.randn(80, 1)
        xs.append(x); ys.append(y)
    hyp = np.array([0.2, 0.5, 0.1])
    m = pyGPs.GPR()
    m.setPrior(kernel=cov.Linear() + cov.RBF())
    m.setNoise(np.log(SN))
    worst = 0.0
    for x in xs:
        k = cov.Linear(hyp[0]) + cov.RBF(hyp[1], hyp[2])
        worst = max(worst, cond_ok("clustering", k, x, SN * SN))
    assert worst <= COND_CAP
    if worst > WORST["cond"]:
        WORST["cond"], WORST["where"] = worst, "clustering"
    v0 = ext.gp_likelihood_independent(hyp, m, xs, ys, der=False)
    v1 = ext.gp_likelihood_independent(hyp, m, xs, ys, der=True)
    # the pieces of the sums, series by series, through the same calls
    nl, dc, dl, dm = [], [], [], []
    for x, y in zip(xs, ys):
        m.setData(x, y)
        a, b, _ = m.getPosterior(der=True)
        nl.append(float(a)); dc.append(np.array(b.cov, dtype=float)); dl.append(np.array(b.lik, dtype=float))
        dm.append(np.array(b.mean, dtype=float))
    save("G27_dot_clustering", hyp=hyp, lik_hyp=np.array([np.log(SN)]), cond=np.array(worst),
         **{"x%d" % i: x for i, x in enumerate(xs)}, **{"y%d" % i: y for i, y in enumerate(ys)},
         value=np.array(v0, dtype=float), value_der=np.array(v1, dtype=float), series_nlZ=np.array(nl),
         sum_dnlZ_cov=np.sum(dc, axis=0), sum_dnlZ_lik=np.sum(dl, axis=0), sum_dnlZ_mean=np.sum(dm, axis=0))


def cls_data(N, d, seed):
    rng = np.random.RandomState(seed)
    x = rng.randn(N, d)
    w = rng.randn(d, 1)
    y = np.sign(x @ w / np.sqrt(d) + 0.3 * rng.randn(N, 1))
    y[y == 0] = 1
    xs = rng.randn(130, d)
    xs[100:] *= 10.0
    return x, y, xs


def ep():
    x, y, xs = cls_data(200, 3, seed=276)
    k = cov.Linear(0.0) * cov.RBF(0.5, 0.0) + cov.Poly(-1.0, 2, -0.5)
    c = cond_ok("ep", k, x, 1.0)
    assert c <= COND_CAP
    if c > WORST["cond"]:
        WORST["cond"], WORST["where"] = c, "ep"
    m = pyGPs.GPC()
    m.setPrior(kernel=k)
    calls = []
    orig = type(m.inffunc)._epComputeParams

    def spy(self, *a, **kw):
        out = orig(self, *a, **kw)
        calls.append(float(out[2]))
        return out
    type(m.inffunc)._epComputeParams = spy
    try:
        nlZ, dnlZ, post = m.getPosterior(x, y)
    finally:
        type(m.inffunc)._epComputeParams = orig
    ym, ys2, fm, fs2, lp = m.predict(xs, ys=np.ones((130, 1)))
    save("G27_dot_ep_N200", x=x, y=y, pred_xs=xs, cond=np.array(c), cov_hyp=np.array(m.covfunc.hyp, dtype=float),
         nlZ=np.array(nlZ, dtype=float), alpha=post.alpha, sW=post.sW, L_diag=np.diag(post.L).copy(), n_sweeps=len(calls),
         pred_ym=ym, pred_ys2=ys2, pred_fm=fm, pred_fs2=fs2, pred_lp=lp, **dn(dnlZ))


def laplace():
    import pyGPs.Core.inf as ref_inf
    x, y, xs = cls_data(200, 3, seed=277)
    k = cov.Linear(0.1) + cov.RBF(0.4, 0.2)
    c = cond_ok("laplace", k, x, 1.0)
    assert c <= COND_CAP
    if c > WORST["cond"]:
        WORST["cond"], WORST["where"] = c, "laplace"
    m = pyGPs.GPC()
    m.useInference("Laplace")
    m.setPrior(kernel=k)
    steps = []
    orig = ref_inf.brentmin

    def spy(*a, **kw):
        out = orig(*a, **kw)
        steps.append(float(np.asarray(out[0]).ravel()[0]))
        return out
    ref_inf.brentmin = spy
    try:
        nlZ, dnlZ, post = m.getPosterior(x, y)
    finally:
        ref_inf.brentmin = orig
    ym, ys2, fm, fs2, lp = m.predict(xs, ys=np.ones((130, 1)))
    save("G27_dot_laplace_N200", x=x, y=y, pred_xs=xs, cond=np.array(c), cov_hyp=np.array(m.covfunc.hyp, dtype=float),
         nlZ=np.array(nlZ, dtype=float), alpha=post.alpha, sW=post.sW, L_diag=np.diag(post.L).copy(), newton_steps=len(steps),
         pred_ym=ym, pred_ys2=ys2, pred_fm=fm, pred_fs2=fs2, pred_lp=lp, **dn(dnlZ))


ALL = dict(kernels=kernels, fits=fits, optimize=optimize, clustering=clustering, ep=ep, laplace=laplace)

if __name__ == "__main__":
    for what in (sys.argv[1:] or ["fits", "optimize", "clustering", "ep", "laplace", "kernels"]):
        ALL[what]()
    print("largest condition number of a recorded fit: %.4g (%s)" % (WORST["cond"], WORST["where"]))
