"""GPU: sparse GP classification -- GPC_FITC (Core/gp.py:1117-1202) with FITC_EP inference (Core/inf.py:810-944) through
pgp_fitc_ep_fit, against the G21 recordings of the reference, the CPU restatement in tests/fitc_ep_cpu.py, central
differences of the device's own nlZ and device dense EP on the explicit Kt = V'V + diag(d0)."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden, relerr, synth_cls
from fitc_ep_cpu import fitc_ep_fit
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu


def _kernel(nm, h):
    from pygps_amd import cov
    h = [float(v) for v in h]
    if nm == "rbf":
        return cov.RBF(h[0], h[1])
    if nm == "rbfard":
        return cov.RBFard(log_ell_list=h[:-1], log_sigma=h[-1])
    if nm == "matern5":
        return cov.Matern(h[0], 5, h[1])
    return cov.RBF(h[0], h[1]) + cov.Matern(h[2], 3, h[3])


def _model(kernel, u, mean=None):
    import pygps_amd as pyGPs
    m = pyGPs.GPC_FITC()
    m.setPrior(mean=mean if mean is not None else pyGPs.mean.Zero(), kernel=kernel, inducing_points=u)
    return m


def _triple(h, x, u):
    return (O.cov_matrix(O.RBF, h, 0, z=x, mode="self_test"), O.cov_matrix(O.RBF, h, 0, x=u, mode="train"),
            O.cov_matrix(O.RBF, h, 0, x=u, z=x, mode="cross"))


def test_G21_demo_gpc_fitc():
    import pygps_amd as pyGPs
    g = golden("G21_fitc_ep_demo")
    x, y, xs = g["x"], g["y"], g["xstar"]
    m = pyGPs.GPC_FITC()
    m.setData(x, y)
    assert np.array_equal(m.u, g["u"])
    nlZ, dnlZ, post = m.getPosterior()
    assert m.inffunc.sweeps == g["sweeps"]
    assert type(nlZ) is np.float64 and relerr(nlZ, g["nlZ"]) < 1e-8
    assert relerr(m.inffunc.last_ttau, g["ttau"]) < 1e-6 and relerr(m.inffunc.last_tnu, g["tnu"]) < 1e-6
    assert relerr(post.alpha, g["alpha"]) < 1e-6 and relerr(post.L, g["L"]) < 1e-6 and relerr(post.sW, g["sW"]) < 1e-6
    assert relerr(dnlZ.cov, g["dnlZ_cov"]) < 1e-7 and relerr(dnlZ.mean, g["dnlZ_mean"]) < 1e-7 and dnlZ.lik == []
    ym, ys2, fm, fs2, lp = m.predict(xs, ys=np.ones((xs.shape[0], 1)))
    assert relerr(fm, g["pred_fm"]) < 1e-7 and relerr(fs2, g["pred_fs2"]) < 1e-6
    assert relerr(lp, g["pred_lp"]) < 1e-6 and relerr(ym, g["pred_ym"]) < 1e-7
    m2 = pyGPs.GPC_FITC()
    m2.setData(x, y)
    m2.optimize()
    assert abs(m2.nlZ - g["opt_nlZ"]) < 1e-5 * abs(g["opt_nlZ"])
    assert relerr(m2.covfunc.hyp, g["opt_cov_hyp"]) < 1e-3
    assert relerr(m2.predict(g["opt_xs"], ys=np.ones((g["opt_xs"].shape[0], 1)))[4], g["opt_lp"]) < 1e-4


@pytest.mark.parametrize("nm", ["rbf_N128_nu25", "rbf_N1500_nu160", "rbfard_N1500_nu160", "matern5_N1500_nu160",
                                "sum_N1500_nu160", "rbf_N4096_nu256"])
def test_G21_synth(nm):
    g = golden("G21_fitc_ep_" + nm)
    kind = nm.split("_")[0]
    x, y = synth_cls(int(g["N"]), int(g["d"]))
    m = _model(_kernel(kind, g["cov_hyp"]), g["u"])
    if kind == "matern5":
        m.covfunc.covfunc.reference_compat = True            # the fixture's gradients hold the reference's Matern quirk (Q4)
    if kind == "sum":
        m.covfunc.covfunc.cov2.reference_compat = True
    assert list(np.asarray(m.covfunc.hyp, float)) == list(g["cov_hyp"])
    nlZ, dnlZ, post = m.getPosterior(x, y)
    assert m.inffunc.sweeps == g["sweeps"]
    assert relerr(nlZ, g["nlZ"]) < 1e-8
    assert relerr(m.inffunc.last_ttau, g["ttau"]) < 1e-6 and relerr(m.inffunc.last_tnu, g["tnu"]) < 1e-6
    assert relerr(post.alpha, g["alpha"]) < 1e-3 and relerr(np.diag(post.L), g["L_diag"]) < 1e-3
    if "L_sample" in g:
        assert relerr(np.asarray(post.L).ravel()[::int(g["L_stride"])], g["L_sample"]) < 1e-3
    scale = max(1.0, np.max(np.abs(g["dnlZ_cov"])))
    assert np.max(np.abs(np.array(dnlZ.cov) - g["dnlZ_cov"])) < 1e-6 * scale
    ym, ys2, fm, fs2, lp = m.predict(g["pred_xs"], ys=np.ones((g["pred_xs"].shape[0], 1)))
    assert relerr(fm, g["pred_fm"]) < 1e-7 and relerr(fs2, g["pred_fs2"]) < 1e-5 and relerr(lp, g["pred_lp"]) < 1e-5


def test_G21_const_mean_and_warm_start_pair():
    import pygps_amd as pyGPs
    g = golden("G21_fitc_ep_const_mean_N300_nu30")
    m = _model(pyGPs.cov.RBF(*g["cov_hyp"]), g["u"], pyGPs.mean.Const(float(g["mean_hyp"][0])))
    nlZ, dnlZ, post = m.getPosterior(g["x"], g["y"])
    assert m.inffunc.sweeps == g["sweeps"] and relerr(nlZ, g["nlZ"]) < 1e-8
    assert relerr(m.inffunc.last_ttau, g["ttau"]) < 1e-6 and relerr(m.inffunc.last_tnu, g["tnu"]) < 1e-6
    assert relerr(post.alpha, g["alpha"]) < 1e-6 and relerr(post.L, g["L"]) < 1e-6
    assert relerr(dnlZ.mean, g["dnlZ_mean"]) < 1e-7 and relerr(dnlZ.cov, g["dnlZ_cov"]) < 1e-7
    assert relerr(m.predict(g["pred_xs"], ys=np.ones((32, 1)))[4], g["pred_lp"]) < 1e-6
    w = golden("G21_fitc_ep_warm_N512_nu64")
    m = _model(pyGPs.cov.RBF(*w["hyps"][0]), w["u"])
    for k in range(3):
        m.covfunc.hyp = [float(v) for v in w["hyps"][k]]
        nlZ, dnlZ, post = m.getPosterior(w["x"], -w["y"] if w["flip"][k] else w["y"])
        assert m.inffunc.sweeps == w["sweeps%d" % k], k
        assert relerr(nlZ, w["nlZ%d" % k]) < 1e-8 and relerr(m.inffunc.last_ttau, w["ttau%d" % k]) < 1e-6
        assert relerr(dnlZ.cov, w["dnlZ_cov%d" % k]) < 1e-7


def test_central_differences_every_hyper():
    """EP stops at |delta nlZ| < 1e-4 (inf.py:873), and the gradient formula holds at the fixed point only.  The base fit is
    therefore run twice (the second call starts from the first one's sites and sweeps at least twice more), and every
    displaced fit starts from the base's sites too."""
    import pygps_amd as pyGPs
    x, y = synth_cls(700, 3, seed=7)
    u = np.random.RandomState(8).randn(40, 3)
    kern = pyGPs.cov.RBFard(log_ell_list=[0.3, 0.5, 0.1], log_sigma=0.2) + pyGPs.cov.Matern(0.4, 5, -0.3)
    m = _model(kern, u, pyGPs.mean.Const(0.2))
    m.getPosterior(x, y)
    nlZ, dnlZ, _ = m.getPosterior(x, y)
    base = (m.inffunc.last_ttau.copy(), m.inffunc.last_tnu.copy())
    g = np.array(dnlZ.mean + dnlZ.cov)
    h0 = [float(v) for v in m.covfunc.hyp]
    e = 1e-5
    for k in range(len(g)):
        vals = []
        for sgn in (1, -1):
            f = pyGPs.inf.FITC_EP()
            f.last_ttau, f.last_tnu = base[0].copy(), base[1].copy()
            m.inffunc = f
            hh = list(h0)
            if k == 0:
                m.meanfunc.hyp = [0.2 + sgn * e]
            else:
                m.meanfunc.hyp = [0.2]
                hh[k - 1] += sgn * e
            m.covfunc.hyp = hh
            vals.append(m.getPosterior(x, y, der=False)[0])
        fd = (vals[0] - vals[1]) / (2 * e)
        assert abs(fd - g[k]) < 1e-3 * max(1.0, abs(g[k])), (k, fd, g[k])


@pytest.mark.parametrize("n,nu", [(2048, 256), (8192, 256)])
def test_equals_device_dense_ep_on_Kt(n, nu):
    import pygps_amd as pyGPs
    from pygps_amd import _lib, inf
    x, y = synth_cls(n, 8, seed=9)
    u = np.random.RandomState(10).randn(nu, 8)
    h = [np.log(np.sqrt(8.0)), 0.1]
    m = _model(pyGPs.cov.RBF(*h), u)
    nlZ, _, post = m.getPosterior(x, y)
    diagK, Kuu, Ku = _triple(h, x, u)
    Luu = np.linalg.cholesky(Kuu + 1e-6 * np.eye(nu))
    V = np.linalg.solve(Luu, Ku)
    Kt = V.T @ V
    Kt[np.diag_indices(n)] += diagK.ravel() - (V * V).sum(0)
    ep = inf.EP()
    Kt = np.ascontiguousarray(Kt)
    dev = _lib.default_device()
    ttau, tnu, alpha, sW, nlz, gm = np.zeros(n), np.zeros(n), np.empty(n), np.empty(n), np.zeros(1), np.zeros(1)
    sweeps, fh = C.c_int(), C.c_void_p()
    inf._Resident.ensure(_lib.f64(x), _lib.f64(y).reshape(n), dev)
    _lib.check(_lib.load().pgp_ep_fit_dense(_lib.ctx(dev), _lib.ptr(Kt), _lib.ptr(np.zeros(n)), None, 0, 2, 0, _lib.ptr(ttau),
                                            _lib.ptr(tnu), _lib.ptr(alpha), _lib.ptr(sW), _lib.ptr(nlz), _lib.ptr(gm),
                                            C.byref(sweeps), C.byref(fh)), "pgp_ep_fit_dense")
    inf.DeviceFactor(fh, n, dev, _lib.current_slot())
    del ep
    assert sweeps.value == m.inffunc.sweeps
    assert relerr(nlZ, nlz[0]) < 1e-9
    assert relerr(m.inffunc.last_ttau.ravel(), ttau) < 1e-6 and relerr(m.inffunc.last_tnu.ravel(), tnu) < 1e-6
    # predictive means at the training inputs: Kt alpha_long (dense) == Q alpha_long + d0 o alpha_long == Ku' post.alpha + d0 ...
    fm = m.predict(x[:256])[2].ravel()
    fm_dense = Kt[:256] @ alpha - (diagK.ravel()[:256] - (V[:, :256] ** 2).sum(0)) * alpha[:256]
    assert relerr(fm, fm_dense) < 1e-6


@pytest.mark.parametrize("n,nu", [(1, 1), (5, 12), (127, 1), (129, 130), (300, 128), (257, 129)])
def test_ragged_shapes_against_restatement(n, nu):
    import pygps_amd as pyGPs
    x, y = synth_cls(n, 2, seed=11)
    if n > 1:
        y[0] = -y[1]
    u = np.random.RandomState(12).randn(nu, 2)
    h = [0.2, 0.1]
    m = _model(pyGPs.cov.RBF(*h), u)
    nlZ, dnlZ, post = m.getPosterior(x, y)
    ders = [(O.der_matrix(O.RBF, h, 0, z=x, mode="self_test", der=k), O.der_matrix(O.RBF, h, 0, x=u, mode="train", der=k),
             O.der_matrix(O.RBF, h, 0, x=u, z=x, mode="cross", der=k)) for k in range(2)]
    r = fitc_ep_fit(*_triple(h, x, u), y, np.zeros(n), ders=ders)
    assert m.inffunc.sweeps == r["sweeps"]
    assert relerr(nlZ, r["nlZ"]) < 1e-8
    assert relerr(m.inffunc.last_ttau, r["ttau"]) < 1e-6 and relerr(m.inffunc.last_tnu, r["tnu"]) < 1e-6
    assert relerr(post.alpha, r["alpha"]) < 1e-5
    assert np.max(np.abs(np.array(dnlZ.cov) - r["dnlZ_cov"])) < 1e-6 * max(1.0, np.max(np.abs(r["dnlZ_cov"])))


def test_warm_start_across_optimize_and_repeat_is_bit_identical():
    import pygps_amd as pyGPs
    x, y = synth_cls(1000, 3, seed=13)
    u = np.random.RandomState(14).randn(50, 3)
    m = _model(pyGPs.cov.RBF(0.3, 0.0), u)
    m.optimizer.searchConfig = None
    m.optimize(x, y, numIterations=15)
    assert m.inffunc.last_ttau is not None and m.inffunc.sweeps < 10
    h = [float(v) for v in m.covfunc.hyp]
    r = fitc_ep_fit(*_triple(h, x, u), y, np.zeros(1000))
    assert relerr(m.nlZ, r["nlZ"]) < 1e-6                  # warm-started fits end where a cold one does (tol 1e-4 on nlZ)

    def fit():
        f = _model(pyGPs.cov.RBF(0.3, 0.0), u)
        nlZ, dnlZ, post = f.getPosterior(x, y)
        return nlZ, np.array(post.alpha), np.array(post.L), np.array(dnlZ.cov)
    first = fit()
    for nn in (129, 3000):
        xo, yo = synth_cls(nn, 3, seed=15)
        _model(pyGPs.cov.RBF(0.3, 0.0), u).getPosterior(xo, yo)
    again = fit()
    assert first[0] == again[0] and all(np.array_equal(a, b) for a, b in zip(first[1:], again[1:]))


def test_large_fit_n65536_nu1024_finite_and_block_restatement():
    import pygps_amd as pyGPs
    n, nu, d = 65536, 1024, 8
    x, y = synth_cls(n, d, seed=16)
    u = x[np.random.RandomState(17).choice(n, nu, replace=False)] + 0.01
    h = [np.log(np.sqrt(d)), 0.0]
    m = _model(pyGPs.cov.RBF(*h), u)
    nlZ, dnlZ, post = m.getPosterior(x, y)
    assert np.isfinite(nlZ) and np.all(np.isfinite(post.alpha)) and np.all(np.isfinite(dnlZ.cov))
    r = fitc_ep_fit(*_triple(h, x, u), y, np.zeros(n), block=128)
    assert m.inffunc.sweeps == r["sweeps"]
    assert relerr(nlZ, r["nlZ"]) < 1e-8
    assert relerr(m.inffunc.last_ttau, r["ttau"]) < 1e-6 and relerr(post.alpha, r["alpha"]) < 1e-5
