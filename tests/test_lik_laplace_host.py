"""lik.Laplace, host side (no GPU): the EP-mode moments of pygps_amd.lik.Laplace and the CPU restatement of dense EP
(tests/lik_laplace_cpu.py) against the G22 recordings of the reference, the gradients' evaluation point against central
differences, and the routing of GPR.useLikelihood / inf.EP without a device."""
import numpy as np
import pytest

from conftest import golden, relerr
from lik_laplace_cpu import ep_laplace_fit
from oracle import gp_oracle as O


def _ep():
    from pygps_amd import inf
    return inf.EP()


def test_G22_moments_interior():
    from pygps_amd import lik
    z = golden("G22_lik_laplace_moments")
    for i in range(len(z["y"])):
        L = lik.Laplace(np.log(z["sn"][i]))
        lZ, dlZ, d2lZ = L.evaluate(z["y"][i], z["mu"][i], z["s2"][i], _ep(), None, 3)
        assert lZ == pytest.approx(z["lZ"][i], rel=1e-12, abs=1e-12)
        assert dlZ == pytest.approx(z["dlZ"][i], rel=1e-12, abs=1e-12)
        # d2lZ = E[b] - dlZ^2 cancels where |mu - y| >> sqrt(s2): compare on the scale of its terms
        assert abs(d2lZ - z["d2lZ"][i]) <= 1e-12 * max(1.0, dlZ * dlZ)
        dh = L.evaluate(z["y"][i], z["mu"][i], z["s2"][i], _ep(), 0)
        # (dap + dam) / (ep + em) - 1 cancels on the scale of tvar
        assert abs(dh - z["dlZhyp"][i]) <= 1e-12 * max(1.0, z["s2"][i] / z["sn"][i] ** 2, abs(z["mu"][i] - z["y"][i]) / z["sn"][i])


def test_G22_moments_vectorised_and_idlik():
    from pygps_amd import lik
    z = golden("G22_lik_laplace_moments")
    L = lik.Laplace(np.log(float(z["idlik_sn"])))
    assert np.array_equal(L.evaluate(z["idlik_y"], z["idlik_mu"], z["idlik_s2"], _ep(), 0), z["idlik_dlZhyp"])
    # elementwise value mode on a vector equals the scalar calls (the reference broadcasts the first dlZ, see lik.Laplace)
    sel = slice(0, 60)
    y, mu, s2 = z["y"][sel], z["mu"][sel], z["s2"][sel]
    L = lik.Laplace(np.log(0.3))
    lZ, dlZ, d2lZ = L.evaluate(y, mu, s2, _ep(), None, 3)
    for i in range(len(y)):
        assert np.array_equal(np.array(L.evaluate(y[i], mu[i], s2[i], _ep(), None, 3)), np.array([lZ[i], dlZ[i], d2lZ[i]]))


def test_limits_of_the_three_regimes():
    """idlik: log N(y | mu, s2 + sn^2); idgau: the Laplace density at mu; both continuous with the interior at the switch."""
    from pygps_amd import lik
    sn = 0.2
    L = lik.Laplace(np.log(sn))
    y, mu = 0.3, 0.1
    s2 = (1.01e3 * sn) ** 2
    lZ, dlZ, d2lZ = L.evaluate(y, mu, s2, _ep(), None, 3)
    v = s2 + sn * sn
    assert lZ == pytest.approx(-(y - mu) ** 2 / v / 2 - np.log(2 * np.pi * v) / 2, rel=1e-15)
    assert (dlZ, d2lZ) == pytest.approx(((y - mu) / v, -1 / v), rel=1e-15)
    assert L.evaluate(y, mu, s2, _ep(), 0) == 0.0
    b = sn / np.sqrt(2)
    s2 = (sn / 1.01e3) ** 2
    lZ, dlZ, d2lZ = L.evaluate(y, mu, s2, _ep(), None, 3)
    assert (lZ, dlZ, d2lZ) == pytest.approx((-abs(y - mu) / b - np.log(2 * b), 1 / b, 0.0), rel=1e-15)
    assert L.evaluate(y, mu, s2, _ep(), 0) == pytest.approx(abs(y - mu) / b - 1, rel=1e-15)
    # the interior next to both switches
    for s2i, s2o in (((0.99e3 * sn) ** 2, (1.01e3 * sn) ** 2), ((sn / 0.99e3) ** 2, (sn / 1.01e3) ** 2)):
        a = np.array(L.evaluate(y, mu, s2i, _ep(), None, 2))
        c = np.array(L.evaluate(y, mu, s2o, _ep(), None, 2))
        assert np.all(np.abs(a - c) <= 0.05 * np.maximum(1.0, np.abs(c)))


def test_prediction_and_other_modes():
    from pygps_amd import inf, lik
    L = lik.Laplace(np.log(0.5))
    b = 0.5 / np.sqrt(2)
    mu = np.array([[0.2], [1.0]])
    lp, ym, ys2 = L.evaluate(np.array([[0.0], [0.5]]), mu, np.zeros((2, 1)), None, None, 3)
    assert np.allclose(lp, -np.abs(np.array([[0.0], [0.5]]) - mu) / b - np.log(2 * b), rtol=1e-15)
    assert np.array_equal(ym, mu) and np.allclose(ys2, 0.25)
    s2 = np.array([[0.1], [0.3]])
    lp, ym, ys2 = L.evaluate(None, mu, s2, None, None, 3)
    assert np.array_equal(lp, L.evaluate(np.zeros_like(mu), mu, s2, inf.EP()))
    assert np.allclose(ys2, s2 + 0.25, rtol=1e-15)
    lp = L.evaluate(np.array([0.3]), np.array([0.1]), None, inf.Laplace(), None, 1)
    assert lp == pytest.approx(-0.2 / b - np.log(2 * b))       # a log-density (the reference's sign is flipped)
    with pytest.raises(NotImplementedError):
        inf.Laplace()._lik_args(L)                              # "ONLY works with EP"
    with pytest.raises(Exception, match="Incorrect inference in lik.Laplace"):
        L.evaluate(np.array([0.3]), np.array([0.1]), np.array([0.1]), inf.Exact())


def test_routing_without_a_device():
    import pygps_amd as pyGPs
    from pygps_amd import inf, lik
    m = pyGPs.GPR()
    m.useLikelihood("Laplace")
    assert isinstance(m.likfunc, lik.Laplace) and isinstance(m.inffunc, inf.EP)
    assert m.likfunc.hyp == [np.log(0.1)]
    assert m.inffunc.reference_compat is False
    with pytest.raises(Exception, match='Possible lik values are "Laplace".'):
        pyGPs.GPR().useLikelihood("Gauss")
    mf = pyGPs.GPR_FITC()
    mf.useLikelihood("Laplace")
    assert isinstance(mf.likfunc, lik.Laplace) and isinstance(mf.inffunc, inf.FITC_EP)
    assert mf.inffunc.reference_compat is False
    with pytest.raises(Exception, match='Possible lik values are "Laplace".'):
        pyGPs.GPR_FITC().useLikelihood("Erf")
    with pytest.raises(NotImplementedError, match="lik.Erf and lik.Laplace only"):
        inf.FITC_EP().evaluate(pyGPs.mean.Zero(), pyGPs.cov.RBF().fitc(np.zeros((2, 1))), lik.Gauss(), np.zeros((3, 1)),
                               np.zeros((3, 1)), 3)
    # the other likelihoods keep their error paths
    with pytest.raises(NotImplementedError, match="lik.Erf and lik.Laplace only"):
        inf.EP().evaluate(pyGPs.mean.Zero(), pyGPs.cov.RBF(), lik.Gauss(), np.zeros((3, 1)), np.zeros((3, 1)), 3)
    # opt.Minimize trains the likelihood hyper-parameter like any other
    from pygps_amd import opt
    o = opt.Minimize(m)
    o._apply_in_objects(np.array([0.1, 0.2, np.log(0.3)]))
    assert m.likfunc.hyp == [pytest.approx(np.log(0.3))]


def _problem(name, n=None):
    z = golden(name)
    x, y = z["x"], z["y"]
    if n is not None:
        x, y = x[:n], y[:n]
    hyp = z["cov_hyp"]
    K = O.cov_matrix(O.RBF, hyp, 0, x=x, mode="train")
    dK = [O.der_matrix(O.RBF, hyp, 0, x=x, mode="train", der=h) for h in range(len(hyp))]
    mh = z["mean_hyp"]
    m = (mh[0] if len(mh) else 0.0) * np.ones(len(y))
    dm = [np.ones(len(y))] if len(mh) else []
    return z, K, dK, y.ravel(), m, dm


@pytest.mark.parametrize("name", ["G22_lik_laplace_const_N200", "G22_lik_laplace_zero_N200", "G22_lik_laplace_demo"])
def test_G22_restatement(name):
    z, K, dK, y, m, dm = _problem(name)
    r = ep_laplace_fit(K, y, m, z["lik_hyp"][0], dm=dm, dK=dK, point="reference")
    assert r["sweeps"] == int(z["sweeps"])
    assert abs(r["nlZ"] - float(z["nlZ"])) <= 1e-9 * max(1.0, abs(float(z["nlZ"])))
    assert relerr(r["ttau"], z["ttau"].ravel()) <= 1e-6 and relerr(r["tnu"], z["tnu"].ravel()) <= 1e-6
    assert relerr(r["alpha"], z["alpha"].ravel()) <= 1e-8
    assert relerr(r["dnlZ_cov"], z["dnlZ_cov"]) <= 1e-8
    assert relerr(r["dnlZ_lik"], z["dnlZ_lik"]) <= 1e-8


def test_G22_restatement_warm_pair():
    z = golden("G22_lik_laplace_warm_N200")
    x, y = z["x"], z["y"].ravel()
    prev = (None, None)
    for tag in "abc":
        hyp = z[tag + "_cov_hyp"]
        K = O.cov_matrix(O.RBF, hyp, 0, x=x, mode="train")
        m = z[tag + "_mean_hyp"][0] * np.ones(len(y))
        r = ep_laplace_fit(K, y, m, z[tag + "_lik_hyp"][0], last_ttau=prev[0], last_tnu=prev[1], point="reference")
        assert r["sweeps"] == int(z[tag + "_sweeps"]), tag
        assert abs(r["nlZ"] - float(z[tag + "_nlZ"])) <= 1e-9 * max(1.0, abs(float(z[tag + "_nlZ"]))), tag
        assert relerr(r["alpha"], z[tag + "_alpha"].ravel()) <= 1e-7, tag
        prev = (r["ttau"], r["tnu"])


def test_gradient_point_by_central_differences():
    """The reference evaluates dlZhyp at nu_n / tau_n (inf.py:796-798), without the prior mean: with a Const mean its
    dnlZ.lik is wrong, and its mean gradient takes the first site's dlZ for every site.  The cavity of f is right."""
    z, K, dK, y, m, dm = _problem("G22_lik_laplace_const_N200", n=60)
    K = K[:60, :60]
    ls = float(z["lik_hyp"][0])
    kw = dict(tol=1e-13, max_sweep=400)
    r = ep_laplace_fit(K, y, m, ls, dm=dm, dK=[d[:60, :60] for d in dK], **kw)
    h = 1e-5
    fd_lik = (ep_laplace_fit(K, y, m, ls + h, **kw)["nlZ"] - ep_laplace_fit(K, y, m, ls - h, **kw)["nlZ"]) / (2 * h)
    fd_mean = (ep_laplace_fit(K, y, m + h, ls, **kw)["nlZ"] - ep_laplace_fit(K, y, m - h, ls, **kw)["nlZ"]) / (2 * h)
    assert abs(r["dnlZ_lik"][0] - fd_lik) <= 1e-5 * max(1.0, abs(fd_lik))
    assert abs(r["dnlZ_mean"][0] - fd_mean) <= 1e-4 * max(1.0, abs(fd_mean))
    rr = ep_laplace_fit(K, y, m, ls, dm=dm, **dict(kw, point="reference"))
    assert abs(rr["dnlZ_lik"][0] - fd_lik) > 1e-2 * abs(fd_lik)
