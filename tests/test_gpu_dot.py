"""GPU: the dot-product kernels cov.Linear, cov.Poly and cov.LINard -- the dot-product accumulator of the tile kernels
(csrc/assemble.hip cov_tile_kernel KIND 8 / 9, csrc/sqdist_tile.h dot_value), the fused gradient pass (csrc/grad.hip
hadamard_prog_kernel<., false, true>, lin_dim_reduce) and the per-point prior variance (cov_self_vec_kernel<true> behind pgp_cov's
'self_test', pgp_predict's blocked solve, EP's K_ii) -- against the reference's recordings (tests/golden/G27_dot_*), against the
long-double restatement tests/dot_ref_ld.py at its derived bar, and against the dense route, which shares none of that code.

Conventions the finite-difference tests expect (the reference's, Core/cov.py:1021, 324): the derivative w.r.t. Linear's hyper and
w.r.t. a Scale hyper is TWICE the derivative of the value; every other derivative is the derivative of the value."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden, relerr
import dot_ref_ld as DR

pytestmark = pytest.mark.gpu
MODES = (("train", "train"), ("cross", "cross"), ("self", "self_test"))


def _close(a, b, tol=2e-12):
    scale = max(1.0, float(np.max(np.abs(b))))
    np.testing.assert_allclose(a, b, rtol=tol, atol=tol * scale)


def _kw(mode, x, z):
    return dict(x=x) if mode == "train" else (dict(x=x, z=z) if mode == "cross" else dict(z=z))


@pytest.mark.parametrize("d", [3, 17])
@pytest.mark.parametrize("name", sorted(DR.CASES))
def test_G27_kernel_matrices_all_modes(name, d):
    from pygps_amd import cov
    g = golden("G27_dot_kernels_inputs")
    x, z, hyp = g["x%d" % d], g["z%d" % d], g["%s_d%d_hyp" % (name, d)]
    tree = DR.CASES[name]
    k = DR.build(tree, hyp, cov, d)
    assert list(np.asarray(k.hyp, float)) == list(hyp)
    assert k._on_device()                                   # a device program (plain LINard: a one-leaf program on scaled coordinates)
    rec = DR.golden_sets(golden, name, d)
    nd = DR.n_der(name, tree, hyp)
    for mode, m in MODES:
        K = k.getCovMatrix(mode=m, **_kw(mode, x, z))
        assert K.shape == rec["K"][mode].shape
        _close(K, rec["K"][mode])
        for i in range(nd):
            _close(k.getDerMatrix(mode=m, der=i, **_kw(mode, x, z)), rec["dK%d" % i][mode], 1e-11)
    with pytest.raises(Exception):
        k.getDerMatrix(x=x, mode="train", der=nd)


def _inputs(d, kind, rng, n=70, m=40):
    """Ragged against the 64 tile, more than one tile row; `kind`: unit-scale points, a common offset of 1e4, or a zero row."""
    x, z = rng.randn(n, d), rng.randn(m, d)
    if kind == "offset":
        x, z = x + 1e4, z + 1e4
    if kind == "zero_row":
        x[5] = 0.0
        z[3] = 0.0
    return x, z


def _against_helper(tree, hyp, x, z):
    from pygps_amd import cov
    d = x.shape[1]
    k = DR.build(tree, hyp, cov, d)
    nd = DR.n_der("", tree, hyp)
    # every derivative, or -- for the many length-scales of an ARD leaf at large d -- those around the 16-coordinate stages, the
    # first and last coordinates and the hypers behind them
    ders = list(range(nd)) if nd <= 24 else sorted(set(range(4)) | {14, 15, 16, 17, 31, 32, 47, 48, 63, 64} & set(range(nd))
                                                   | set(range(nd - 4, nd)))
    worst = 0.0
    for mode, m in MODES:
        for der in [None] + ders:
            kw = _kw(mode, x, z)
            got = k.getCovMatrix(mode=m, **kw) if der is None else k.getDerMatrix(mode=m, der=der, **kw)
            K, bar = DR.tree_matrix(tree, hyp, mode=m, der=der, **kw)
            err = np.abs(got.astype(np.longdouble) - K).astype(np.float64)
            worst = max(worst, float(np.max(err / np.maximum(bar, 1e-300))))
            assert np.all(err <= bar), (mode, der, float(np.max(err / np.maximum(bar, 1e-300))))
    return worst


def _hyp_for(tree, d, rng):
    h = 0.3 * rng.randn(DR.n_hyp(tree, d))
    return h


@pytest.mark.parametrize("kind", ["unit", "offset", "zero_row"])
@pytest.mark.parametrize("d", [1, 16, 17, 64, 65])
def test_against_the_long_double_helper_at_its_bar(d, kind):
    rng = np.random.RandomState(100 + d)
    x, z = _inputs(d, kind, rng)
    for name in ("linear", "poly3", "poly2", "linard", "lin_plus_rbf", "lin_times_poly_plus_rbfard"):
        tree = DR.CASES[name]
        w = _against_helper(tree, _hyp_for(tree, d, rng), x, z)
        print("%-28s d=%-3d %-8s worst err / bar %.3g" % (name, d, kind, w))


def test_large_dimensions_d300_and_linard_d70():
    rng = np.random.RandomState(7)
    x, z = _inputs(300, "unit", rng)
    for name in ("linear", "poly3", "lin_plus_rbf"):
        tree = DR.CASES[name]
        _against_helper(tree, _hyp_for(tree, 300, rng), x, z)
    x, z = _inputs(70, "unit", rng)
    _against_helper(DR.CASES["linard"], 0.3 * rng.randn(70), x, z)


def _gpr(tree, g, mean_c=None):
    import pygps_amd as pyGPs
    d = g["x"].shape[1]
    m = pyGPs.GPR()
    k = DR.build(tree, g["cov_hyp"], pyGPs.cov, d)
    if mean_c is None:
        m.setPrior(kernel=k)
    else:
        m.setPrior(mean=pyGPs.mean.Const(mean_c), kernel=k)
    m.setNoise(float(g["lik_hyp"][0]))
    m.setData(g["x"], g["y"])
    return m


@pytest.mark.parametrize("name", sorted(DR.FITS))
def test_G27_fits_and_predictions(name):
    g = golden("G27_dot_fit_" + name)
    m = _gpr(DR.FITS[name], g, float(g["mean_hyp"][0]) if g["mean_hyp"].size else None)
    nlZ, dnlZ, post = m.getPosterior()
    print("%s: nlZ %.3g alpha %.3g Ldiag %.3g dcov %.3g dlik %.3g" % (
        name, relerr(nlZ, g["nlZ"]), relerr(post.alpha, g["alpha"]), relerr(np.diag(post.L), g["L_diag"]),
        relerr(dnlZ.cov, g["dnlZ_cov"]), relerr(dnlZ.lik, g["dnlZ_lik"])))
    assert relerr(nlZ, g["nlZ"]) < 1e-9
    assert relerr(post.alpha, g["alpha"]) < 1e-6
    assert relerr(np.diag(post.L), g["L_diag"]) < 1e-8
    assert relerr(dnlZ.cov, g["dnlZ_cov"]) < 1e-7 and relerr(dnlZ.lik, g["dnlZ_lik"]) < 1e-7
    if g["dnlZ_mean"].size:
        assert relerr(dnlZ.mean, g["dnlZ_mean"]) < 1e-7
    ym, ys2, fm, fs2, lp = m.predict(g["pred_xs"])
    print("   ym %.3g fs2 %.3g ys2 %.3g" % (relerr(ym, g["pred_ym"]), relerr(fs2, g["pred_fs2"]), relerr(ys2, g["pred_ys2"])))
    assert relerr(ym, g["pred_ym"]) < 1e-8 and relerr(fs2, g["pred_fs2"]) < 1e-6 and relerr(ys2, g["pred_ys2"]) < 1e-6
    kss = m.covfunc.getCovMatrix(z=g["pred_xs"], mode="self_test")
    _close(kss, g["kss"])
    assert kss.max() / kss.min() >= 100.0                   # the per-point prior variance is exercised over two orders


def test_G27_optimize():
    import pygps_amd as pyGPs
    g = golden("G27_dot_optimize_N100")
    m = pyGPs.GPR()
    m.setPrior(kernel=DR.build(DR.CASES["lin_plus_rbf"], g["cov_hyp0"], pyGPs.cov, 3))
    m.setNoise(float(g["lik_hyp0"][0]))
    m.setData(g["x"], g["y"])
    m.optimize(g["x"], g["y"], numIterations=int(g["iters"]))
    assert abs(m.nlZ - g["opt_nlZ"]) < 1e-4 * abs(g["opt_nlZ"])           # optimiser path amplifies rounding
    assert relerr(m.predict(g["pred_xs"])[0], g["opt_ym"]) < 1e-3


def test_G27_clustering_flow():
    """Demo/Clustering: one model, shared hypers, the likelihood and its gradient accumulated over several series
    (setData, getPosterior(der=...), dnlZStruct.accumulateDnlZ)."""
    import pygps_amd as pyGPs
    g = golden("G27_dot_clustering")
    m = pyGPs.GPR()
    m.setPrior(kernel=pyGPs.cov.Linear() + pyGPs.cov.RBF())
    m.setNoise(float(g["lik_hyp"][0]))
    m.covfunc.hyp = g["hyp"].tolist()
    for der in (False, True):
        total = 0.0
        acc = pyGPs.inf.dnlZStruct(m.meanfunc, m.covfunc, m.likfunc)
        series = []
        for i in range(3):
            m.setData(g["x%d" % i], g["y%d" % i])
            if der:
                nlZ, dnlZ, post = m.getPosterior(der=True)
                acc = acc.accumulateDnlZ(dnlZ)
            else:
                nlZ, post = m.getPosterior(der=False)
            total += nlZ
            series.append(nlZ)
        assert relerr(series, g["series_nlZ"]) < 1e-9
        if der:
            assert relerr(acc.cov, g["sum_dnlZ_cov"]) < 1e-7 and relerr(acc.lik, g["sum_dnlZ_lik"]) < 1e-7
            assert relerr(total + np.sum(acc.cov) + np.sum(acc.mean), g["value_der"]) < 1e-7
        else:
            assert relerr(total, g["value"]) < 1e-9


def test_G27_ep():
    import pygps_amd as pyGPs
    g = golden("G27_dot_ep_N200")
    m = pyGPs.GPC()
    m.setPrior(kernel=DR.build(DR.EP_TREE, g["cov_hyp"], pyGPs.cov, 3))
    assert m.covfunc._on_device()
    nlZ, dnlZ, post = m.getPosterior(g["x"], g["y"])
    assert m.inffunc.sweeps == int(g["n_sweeps"])
    assert relerr(nlZ, g["nlZ"]) < 1e-8 and relerr(post.alpha, g["alpha"]) < 1e-6 and relerr(post.sW, g["sW"]) < 1e-6
    assert relerr(dnlZ.cov, g["dnlZ_cov"]) < 1e-6
    ym, ys2, fm, fs2, lp = m.predict(g["pred_xs"], ys=np.ones((130, 1)))
    assert relerr(ym, g["pred_ym"]) < 1e-7 and relerr(lp, g["pred_lp"]) < 1e-7


def test_G27_laplace():
    import pygps_amd as pyGPs
    g = golden("G27_dot_laplace_N200")
    m = pyGPs.GPC()
    m.useInference("Laplace")
    m.setPrior(kernel=DR.build(DR.LAPLACE_TREE, g["cov_hyp"], pyGPs.cov, 3))
    nlZ, dnlZ, post = m.getPosterior(g["x"], g["y"])
    assert m.inffunc.newton_steps == int(g["newton_steps"])
    assert relerr(nlZ, g["nlZ"]) < 1e-8 and relerr(post.alpha, g["alpha"]) < 1e-6 and relerr(post.sW, g["sW"]) < 1e-6
    assert relerr(dnlZ.cov, g["dnlZ_cov"]) < 1e-6
    ym, ys2, fm, fs2, lp = m.predict(g["pred_xs"], ys=np.ones((130, 1)))
    assert relerr(ym, g["pred_ym"]) < 1e-7 and relerr(lp, g["pred_lp"]) < 1e-7


# ---- program route against dense route (no dot-product device code on that side) ----------------------------------------------
TREE = DR.CASES["lin_times_poly_plus_rbfard"]


def _n300():
    rng = np.random.RandomState(11)
    d = 3
    x = rng.randn(300, d)
    y = np.sin(x @ rng.randn(d, 1)) + 0.1 * rng.randn(300, 1)
    hyp = np.array([0.2, -0.5, -0.6, 0.3, 0.35, 0.4, 0.2])
    return x, y, hyp


def _f64(t):
    from pygps_amd import _lib
    return _lib.f64(t[0].astype(np.float64))


def test_exact_program_route_against_dense_route():
    import pygps_amd as pyGPs
    from pygps_amd import _lib
    x, y, hyp = _n300()
    n = x.shape[0]
    m = pyGPs.GPR()
    m.setPrior(kernel=DR.build(TREE, hyp, pyGPs.cov, 3))
    assert m.covfunc._on_device()
    m.setNoise(np.log(0.2))
    m.setData(x, y)
    nlZ, dnlZ, post = m.getPosterior()
    lib, ctx = _lib.load(), _lib.ctx()
    log_sn = float(m.likfunc.hyp[0])
    K = _f64(DR.tree_matrix(TREE, hyp, x=x, mode="train"))
    r = _lib.f64((y - m.meanfunc.getMean(x)).reshape(n))
    alpha, nlz, glik = np.empty(n), np.zeros(1), np.zeros(1)
    fh = C.c_void_p()
    _lib.check(lib.pgp_exact_fit_dense(ctx, _lib.ptr(K), n, _lib.ptr(r), log_sn, 3, _lib.ptr(alpha), _lib.ptr(nlz), _lib.ptr(glik),
                                       C.byref(fh)), "pgp_exact_fit_dense")
    gcov, g = [], np.zeros(1)
    for h in range(len(hyp)):
        dK = _f64(DR.tree_matrix(TREE, hyp, x=x, mode="train", der=h))
        _lib.check(lib.pgp_dense_grad_term(ctx, _lib.ptr(dK), n, log_sn, _lib.ptr(g)), "pgp_dense_grad_term")
        gcov.append(g[0])
    lib.pgp_factor_free(ctx, fh)
    print("program vs dense: nlZ %.3g dnlZ.cov %.3g" % (relerr(nlZ, nlz[0]), relerr(dnlZ.cov, gcov)))
    assert relerr(nlZ, nlz[0]) < 1e-10 and relerr(dnlZ.cov, gcov) < 1e-8 and relerr(dnlZ.lik, glik) < 1e-8


def test_ep_program_route_against_dense_route():
    import pygps_amd as pyGPs
    from pygps_amd import _lib, inf
    x, y, hyp = _n300()
    y = np.sign(y - np.median(y))
    y[y == 0] = 1
    n = x.shape[0]
    m = pyGPs.GPC()
    m.setPrior(kernel=DR.build(TREE, hyp, pyGPs.cov, 3))
    nlZ, dnlZ, post = m.getPosterior(x, y)
    lib, dev = _lib.load(), _lib.default_device()
    ctx = _lib.ctx(dev)
    K = _f64(DR.tree_matrix(TREE, hyp, x=x, mode="train"))
    ttau, tnu, alpha, sW, nlz, gm = np.zeros(n), np.zeros(n), np.empty(n), np.empty(n), np.zeros(1), np.zeros(1)
    sweeps, fh = C.c_int(), C.c_void_p()
    inf._Resident.ensure(_lib.f64(x), _lib.f64(y).reshape(n), dev)
    _lib.check(lib.pgp_ep_fit_dense(ctx, _lib.ptr(K), _lib.ptr(np.zeros(n)), None, 0, 3, 0, _lib.ptr(ttau), _lib.ptr(tnu),
                                    _lib.ptr(alpha), _lib.ptr(sW), _lib.ptr(nlz), _lib.ptr(gm), C.byref(sweeps), C.byref(fh)),
               "pgp_ep_fit_dense")
    keep = inf.DeviceFactor(fh, n, dev, _lib.current_slot())
    gcov, g = [], np.zeros(1)
    for h in range(len(hyp)):
        dK = _f64(DR.tree_matrix(TREE, hyp, x=x, mode="train", der=h))
        _lib.check(lib.pgp_dense_grad_term(ctx, _lib.ptr(dK), n, 0.0, _lib.ptr(g)), "pgp_dense_grad_term")
        gcov.append(g[0])
    del keep
    assert sweeps.value == m.inffunc.sweeps
    print("EP program vs dense: nlZ %.3g alpha %.3g dnlZ.cov %.3g" % (relerr(nlZ, nlz[0]), relerr(post.alpha.ravel(), alpha),
                                                                     relerr(dnlZ.cov, gcov)))
    assert relerr(nlZ, nlz[0]) < 1e-10 and relerr(dnlZ.cov, gcov) < 1e-8


def test_predict_against_predict_dense_N1100_in_one_and_three_batches():
    """np >= 1024 and 1100 test points: the product form would be chosen if the guard for per-point k(z, z) were missing."""
    import pygps_amd as pyGPs
    from pygps_amd import _lib
    rng = np.random.RandomState(12)
    d, n, ns = 3, 1100, 1100
    x = rng.randn(n, d)
    y = np.sin(x @ rng.randn(d, 1)) + 0.1 * rng.randn(n, 1)
    xs = rng.randn(ns, d)
    xs[900:] *= 10.0
    hyp = np.array([0.2, -0.5, -0.6, 0.3, 0.35, 0.4, 0.2])
    m = pyGPs.GPR()
    m.setPrior(kernel=DR.build(TREE, hyp, pyGPs.cov, d))
    m.setNoise(np.log(0.2))
    m.setData(x, y)
    nlZ, post = m.getPosterior(der=False)
    ym, ys2, fm, fs2, lp = m.predict(xs)
    lib, ctx = _lib.load(), _lib.ctx()
    _lib.check(lib.pgp_set_option(ctx, b"predict_batch", 512))
    try:
        fm3, fs23 = m.predict(xs)[2:4]
    finally:
        lib.pgp_set_option(ctx, b"predict_batch", 65536)
    assert np.array_equal(fm3, fm) and np.array_equal(fs23, fs2)             # 512 + 512 + 76
    Ks = _f64(DR.tree_matrix(TREE, hyp, x=x, z=xs, mode="cross"))
    kss = _f64(DR.tree_matrix(TREE, hyp, z=xs, mode="self_test")).reshape(ns)
    ms = _lib.f64(m.meanfunc.getMean(xs)).reshape(ns)
    fmd, fs2d = np.empty(ns), np.empty(ns)
    _lib.check(lib.pgp_predict_dense(post.L.ctx, post.L.handle, _lib.ptr(Ks), ns, _lib.ptr(kss), _lib.ptr(ms), _lib.ptr(fmd),
                                     _lib.ptr(fs2d)), "pgp_predict_dense")
    print("predict vs dense: fm %.3g fs2 %.3g" % (relerr(fm.ravel(), fmd), relerr(fs2.ravel(), fs2d)))
    assert relerr(fm.ravel(), fmd) < 1e-8 and relerr(fs2.ravel(), fs2d) < 1e-6
    assert fs2.max() / fs2.min() > 100.0


# ---- LINard away from ell = 1, finite differences -----------------------------------------------------------------------------
def _fd(m, h=1e-5):
    f = m.covfunc
    out = []
    for k in range(len(f.hyp)):
        v = []
        for sgn in (1, -1):
            hh = list(f.hyp)
            hh[k] += sgn * h
            f.hyp = hh
            v.append(m.getPosterior(der=False)[0])
            hh[k] -= sgn * h
            f.hyp = hh
        out.append((v[0] - v[1]) / (2 * h))
    return np.array(out)


@pytest.mark.parametrize("d,n", [(3, 200), (70, 200)])
def test_linard_fit_and_gradients_away_from_unit_length_scales(d, n):
    import pygps_amd as pyGPs
    rng = np.random.RandomState(20 + d)
    x = rng.randn(n, d) / np.sqrt(d)
    y = x @ rng.randn(d, 1) + 0.1 * rng.randn(n, 1)
    hyp = 0.4 * rng.randn(d)
    m = pyGPs.GPR()
    m.setPrior(kernel=pyGPs.cov.LINard(log_ell_list=list(hyp)))
    m.setNoise(np.log(0.2))
    m.setData(x, y)
    nlZ, dnlZ, post = m.getPosterior()
    tree = DR.CASES["linard"]
    K = DR.tree_matrix(tree, hyp, x=x, mode="train")[0].astype(np.float64)
    dKs = [DR.tree_matrix(tree, hyp, x=x, mode="train", der=i)[0].astype(np.float64) for i in range(d)]
    rn, ra, rl, rc, rk = DR.exact_gp(K, dKs, y, m.meanfunc.getMean(x), 0.04)
    print("LINard d=%d: nlZ %.3g alpha %.3g dcov %.3g" % (d, relerr(nlZ, rn), relerr(post.alpha, ra), relerr(dnlZ.cov, rc)))
    assert relerr(nlZ, rn) < 1e-9 and relerr(post.alpha, ra) < 1e-6 and relerr(np.diag(post.L), rl) < 1e-8
    assert relerr(dnlZ.cov, rc) < 1e-7 and relerr(dnlZ.lik, [rk]) < 1e-7
    xs = rng.randn(9, d)
    fm, fs2 = m.predict(xs)[2:4]                            # (before the finite differences: they leave a perturbed posterior behind)
    Ks = DR.tree_matrix(tree, hyp, x=x, z=xs, mode="cross")[0].astype(np.float64)
    assert relerr(fm, Ks.T @ ra + m.meanfunc.getMean(xs)) < 1e-8
    fd = _fd(m)
    assert np.max(np.abs(np.array(dnlZ.cov) - fd)) <= 1e-6 * np.max(np.abs(fd))


@pytest.mark.parametrize("name,factor", [("lin_plus_rbf", [2, 1, 1]), ("poly3", [1, 1]), ("half_lin_plus_rbf", [2, 2, 1, 1])])
def test_central_differences_expect_the_factor_2_in_linear_and_scale_hypers_only(name, factor):
    g = golden("G27_dot_fit_" + (name if name != "lin_plus_rbf" else "lin_plus_rbf_d3"))
    m = _gpr(DR.FITS[name if name != "lin_plus_rbf" else "lin_plus_rbf_d3"], g)
    nlZ, dnlZ, post = m.getPosterior()
    fd = _fd(m) * np.array(factor, dtype=float)
    assert np.max(np.abs(np.array(dnlZ.cov) - fd)) <= 1e-6 * np.max(np.abs(fd)), (dnlZ.cov, fd)


def test_two_models_alternating_on_one_context_bit_for_bit():
    import pygps_amd as pyGPs
    g = golden("G27_dot_fit_lin_plus_rbf_d3")

    def dot_model():
        return _gpr(DR.FITS["lin_plus_rbf_d3"], g)

    def rbf_model():
        m = pyGPs.GPR()
        m.setPrior(kernel=pyGPs.cov.RBF(0.4, 0.1))
        m.setNoise(float(g["lik_hyp"][0]))
        m.setData(g["x"], g["y"])
        return m

    def run(m):
        nlZ, dnlZ, post = m.getPosterior()
        return [np.float64(nlZ), np.array(dnlZ.cov), np.array(dnlZ.lik), post.alpha.copy(), m.predict(g["pred_xs"])[3].copy()]
    alone_dot, alone_rbf = run(dot_model()), run(rbf_model())
    a, b, c = dot_model(), rbf_model(), dot_model()
    for got, want in ((run(a), alone_dot), (run(b), alone_rbf), (run(c), alone_dot)):
        for u, v in zip(got, want):
            assert np.array_equal(u, v)


def test_refusals_with_nothing_allocated():
    import pygps_amd as pyGPs
    from pygps_amd import cov, inf
    g = golden("G27_dot_fit_lin_plus_rbf_d3")
    x, y = g["x"], g["y"]
    import gc
    _gpr(DR.FITS["lin_plus_rbf_d3"], g).getPosterior(der=False)              # the device is up
    gc.collect()                                            # factors of models that are already garbage go now, not in between
    live = inf.DeviceFactor.live_bytes
    with pytest.raises(NotImplementedError, match="dot-product kernels"):
        m = pyGPs.GPR()
        m.setPrior(kernel=cov.Linear() + cov.RBF())
        m.inffunc = inf.Exact(sharded=True)
        m.getPosterior(x, y)
    with pytest.raises(NotImplementedError, match="dot-product kernels"):
        m = pyGPs.GPR_FITC()
        m.setPrior(kernel=cov.Linear() + cov.RBF(), inducing_points=x[:20])
        m.getPosterior(x, y)
    k = cov.RBF().fitc(x[:20])
    k.covfunc = cov.Poly() + cov.RBF()                      # swapped in behind the constructor's check
    for infcls in (inf.FITC_Exact, inf.FITC_EP):
        with pytest.raises(NotImplementedError, match="dot-product kernels"):
            lik = pyGPs.lik.Gauss() if infcls is inf.FITC_Exact else pyGPs.lik.Erf()
            infcls().evaluate(pyGPs.mean.Zero(), k, lik, x, np.sign(y) if infcls is inf.FITC_EP else y, 1)
    gc.collect()
    assert inf.DeviceFactor.live_bytes == live


def test_status_codes_of_the_c_abi():
    """-12: Poly's degree below 1; -4: a derivative index that does not exist; -13: over the limits (LINard beyond 255 length-scales,
    two ARD leaves beside a dot-product leaf); -2: LINard as a leaf of a program."""
    from pygps_amd import _lib
    lib, ctx = _lib.load(), _lib.ctx()
    x = _lib.f64(np.random.RandomState(0).randn(8, 2))
    out = np.empty((8, 8))

    def cov_rc(kind, hyp, para=0, der=-1, xx=x, o=out):
        h = _lib.f64(np.asarray(hyp, dtype=float))
        return lib.pgp_cov(ctx, kind, _lib.MODE_TRAIN, der, _lib.ptr(xx), xx.shape[0], None, 0, xx.shape[1], _lib.ptr(h), len(h),
                           para, 0, _lib.ptr(o))
    assert cov_rc(_lib.COV_POLY, [0., 0.], para=2) == 0
    assert cov_rc(_lib.COV_POLY, [0., 0.], para=0) == -12
    assert cov_rc(_lib.COV_POLY, [0., 0.], para=2, der=2) == 0 and cov_rc(_lib.COV_POLY, [0., 0.], para=2, der=3) == -4
    assert cov_rc(_lib.COV_LINEAR, [0.], der=0) == 0 and cov_rc(_lib.COV_LINEAR, [0.], der=1) == -4
    assert cov_rc(_lib.COV_LINARD, [0., 0.], der=1) == 0 and cov_rc(_lib.COV_LINARD, [0., 0.], der=2) == -4
    assert cov_rc(_lib.COV_LINARD, [0., 0., 0.]) == -11
    x300 = _lib.f64(np.zeros((8, 300)))
    assert cov_rc(_lib.COV_LINARD, np.zeros(300), xx=x300) == -13
    L, S = _lib.PROG_LEAF, _lib.PROG_SUM

    def prog_rc(tok, nh):
        arr = (C.c_int32 * len(tok))(*tok)
        _lib.check(lib.pgp_set_composite(ctx, arr, len(tok)), "pgp_set_composite")
        return cov_rc(_lib.COV_COMPOSITE, np.zeros(nh))
    assert prog_rc([L, 13, 0, 0, 0, L, _lib.COV_RBFARD, 0, 0, 1, S], 4) == 0
    assert prog_rc([L, 13, 0, 0, 0, L, _lib.COV_RBFARD, 0, 0, 1, S, L, _lib.COV_RQARD, 0, 0, 4, S], 8) == -13
    assert prog_rc([L, 15, 0, 0, 0, L, _lib.COV_RBF, 0, 0, 2, S], 4) == -2
    assert prog_rc([L, 14, 0, 0, 0, L, _lib.COV_RBF, 0, 0, 2, S], 4) == -12


def test_gpmc_takes_the_pairs_route_and_equals_a_loop_over_gpc():
    """GPMC with a dot-product prior: choose_route answers "pairs"; the votes are those of one GPC per pair of classes."""
    import pygps_amd as pyGPs
    rng = np.random.RandomState(31)
    n, d, nc = 90, 3, 3
    centres = 2.0 * rng.randn(nc, d)
    lab = np.repeat(np.arange(nc), n // nc)
    x = centres[lab] + rng.randn(n, d)
    xs = centres[np.arange(12) % nc] + rng.randn(12, d)
    m = pyGPs.GPMC(nc)
    m.setPrior(kernel=pyGPs.cov.Linear(-1.0) + pyGPs.cov.RBF(0.5, 0.0))
    m.setData(x, lab.reshape(-1, 1))
    votes = m.fitAndPredict(xs)
    assert m.last_route == "pairs"
    want = np.zeros((12, nc))
    for i in range(nc):
        for j in range(i + 1, nc):
            sel = (lab == i) | (lab == j)
            g = pyGPs.GPC()
            g.setPrior(kernel=pyGPs.cov.Linear(-1.0) + pyGPs.cov.RBF(0.5, 0.0))
            g.getPosterior(x[sel], np.where(lab[sel] == i, 1.0, -1.0).reshape(-1, 1))
            ym = g.predict(xs)[0].ravel()
            want[:, i] += ym + 1
            want[:, j] += 2 - (ym + 1)
    want /= want.sum(axis=1)[:, np.newaxis]
    assert relerr(votes, want) < 1e-10
    assert np.mean(np.argmax(votes, axis=1) == np.arange(12) % nc) > 0.6
