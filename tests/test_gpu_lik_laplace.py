"""GPU: lik.Laplace with EP (GPR.useLikelihood("Laplace"), Core/gp.py:624-635; Core/inf.py:723-806; Core/lik.py:370-512)
through pgp_ep_fit_lik / pgp_ep_fit_dense_lik: the device moments against the host's, the fits against the G22 recordings
of the reference and the CPU restatement, gradients against central differences of the device's own nlZ."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden, relerr
from lik_laplace_cpu import ep_laplace_fit
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu


def _model(x, y, cov_hyp=None, lik_hyp=None, zero_mean=False, compat=False):
    import pygps_amd as pyGPs
    m = pyGPs.GPR()
    m.useLikelihood("Laplace")
    if zero_mean:
        m.setPrior(mean=pyGPs.mean.Zero())
    m.setData(x, y)
    if cov_hyp is not None:
        m.covfunc.hyp = [float(v) for v in cov_hyp]
    if lik_hyp is not None:
        m.likfunc.hyp = [float(v) for v in lik_hyp]
    m.inffunc.reference_compat = compat
    return m


def test_device_moments_all_regimes():
    import pygps_amd as pyGPs
    from pygps_amd import _lib
    rng = np.random.RandomState(7)
    k = 6000
    sn = np.exp(rng.uniform(np.log(1e-3), np.log(10.0), k))
    s2 = sn ** 2 * np.exp(rng.uniform(np.log(1e-9), np.log(1e9), k))     # idgau, interior and idlik
    y = rng.randn(k)
    mu = y + rng.uniform(-40, 40, k) * np.sqrt(s2)
    out = np.zeros(4 * k)
    _lib.check(_lib.load().pgp_test_laplace_ep_lik(_lib.ctx(), _lib.ptr(y), _lib.ptr(mu), _lib.ptr(s2), _lib.ptr(sn), k,
                                                   _lib.ptr(out)), "pgp_test_laplace_ep_lik")
    out = out.reshape(4, k)
    assert np.all(np.isfinite(out))
    idlik = 1e3 * sn < np.sqrt(s2)
    idgau = 1e3 * np.sqrt(s2) < sn
    assert idlik.sum() > 100 and idgau.sum() > 100 and (~idlik & ~idgau).sum() > 1000
    # the reference's formulas are evaluated as written (log space, no subtraction of two exps); the library functions of device
    # and host differ by an ulp, which the formulas amplify by tvar = s2 / sn^2, 1 / tvar or |mu - y| / sn where their terms cancel
    for i in range(k):
        L = pyGPs.lik.Laplace(np.log(sn[i]))
        lZ, dlZ, d2lZ = L.evaluate(y[i], mu[i], s2[i], pyGPs.inf.EP(), None, 3)
        dh = L.evaluate(y[i], mu[i], s2[i], pyGPs.inf.EP(), 0)
        tvar = s2[i] / sn[i] ** 2
        tv = max(1.0, tvar, 1.0 / tvar, abs(mu[i] - y[i]) / sn[i])
        assert abs(out[0, i] - lZ) <= 1e-13 * tv * max(1.0, abs(lZ)), i      # logsum2exp(ap, am) + tvar - ...: terms of size tvar
        assert abs(out[1, i] - dlZ) <= 1e-13 * tv * max(abs(dlZ), 1.0 / sn[i]), i
        assert abs(out[2, i] - d2lZ) <= 1e-13 * tv * max(abs(d2lZ), dlZ * dlZ, 1.0 / sn[i] ** 2), i
        # dlZhyp: (dap + dam) / (ep + em) - 1 cancels terms of size tvar whose exponents exp(-zp^2 - lezp) carry an error of
        # size tvar eps (host build of the same header against numpy: at most 1.3e-11 tv; the device: 1.6e-10 tv)
        assert abs(out[3, i] - dh) <= 1e-9 * tv * max(1.0, abs(dh)), i


@pytest.mark.parametrize("name", ["G22_lik_laplace_const_N200", "G22_lik_laplace_zero_N200", "G22_lik_laplace_const_N1000",
                                  "G22_lik_laplace_demo"])
def test_G22_fit(name):
    z = golden(name)
    m = _model(z["x"], z["y"], z["cov_hyp"], z["lik_hyp"], zero_mean=len(z["mean_hyp"]) == 0, compat=True)
    nlZ, dnlZ, post = m.getPosterior()
    assert m.inffunc.sweeps == int(z["sweeps"])
    assert abs(nlZ - float(z["nlZ"])) <= 1e-8 * max(1.0, abs(float(z["nlZ"])))
    assert relerr(m.inffunc.last_ttau, z["ttau"]) <= 1e-6 and relerr(m.inffunc.last_tnu, z["tnu"]) <= 1e-6
    assert relerr(post.alpha, z["alpha"]) <= 1e-6 and relerr(post.sW, z["sW"]) <= 1e-6
    assert relerr(dnlZ.cov, z["dnlZ_cov"]) <= 1e-6
    assert relerr(dnlZ.lik, z["dnlZ_lik"]) <= 1e-6          # reference_compat: the reference's evaluation point
    xs = z["xstar"] if "xstar" in z.files else z["pred_xs"]
    ys = np.sin(xs[:, :1])
    ym, ys2, fm, fs2, lp = m.predict(xs, ys=ys)
    for got, key in ((ym, "pred_ym"), (ys2, "pred_ys2"), (fm, "pred_fm"), (fs2, "pred_fs2")):
        assert relerr(got, z[key]) <= 1e-6, key
    assert relerr(lp, z["pred_lp"]) <= 5e-6


def test_G22_warm_pair():
    z = golden("G22_lik_laplace_warm_N200")
    m = _model(z["x"], z["y"], compat=True)
    for tag in "abc":
        m.covfunc.hyp = [float(v) for v in z[tag + "_cov_hyp"]]
        m.likfunc.hyp = [float(v) for v in z[tag + "_lik_hyp"]]
        nlZ, dnlZ, post = m.getPosterior()
        assert m.inffunc.sweeps == int(z[tag + "_sweeps"]), tag
        # (outlier sites sit where the reference's d2lZ = E[b] - dlZ^2 cancels: the site parameters carry that rounding)
        assert abs(nlZ - float(z[tag + "_nlZ"])) <= 1e-7 * max(1.0, abs(float(z[tag + "_nlZ"]))), tag
        assert relerr(post.alpha, z[tag + "_alpha"]) <= 1e-6, tag


def test_default_gradients_match_restatement_and_central_differences():
    z = golden("G22_lik_laplace_const_N200")
    x, y = z["x"], z["y"]
    m = _model(x, y, z["cov_hyp"], z["lik_hyp"])
    m.inffunc._tol_exp = 12
    nlZ, dnlZ, post = m.getPosterior()
    g = np.array(dnlZ.mean + dnlZ.cov + dnlZ.lik)
    hyp = z["cov_hyp"]
    K = O.cov_matrix(O.RBF, hyp, 0, x=x, mode="train")
    dK = [O.der_matrix(O.RBF, hyp, 0, x=x, mode="train", der=h) for h in range(2)]
    n = len(y)
    r = ep_laplace_fit(K, y, m.meanfunc.hyp[0] * np.ones(n), z["lik_hyp"][0], dm=[np.ones(n)], dK=dK, tol=1e-12, max_sweep=1000)
    assert relerr(g, np.concatenate([r["dnlZ_mean"], r["dnlZ_cov"], r["dnlZ_lik"]])) <= 1e-6
    h = 1e-3                       # nlZ from the carried sweep state is good to ~1e-9: a step that rounding does not swamp

    def f(dmean=0.0, dcov=(0.0, 0.0), dlik=0.0):
        mm = _model(x, y, np.array(z["cov_hyp"]) + np.array(dcov), np.array(z["lik_hyp"]) + dlik)
        mm.meanfunc.hyp = [m.meanfunc.hyp[0] + dmean]
        mm.inffunc._tol_exp = 12
        return mm.getPosterior(der=False)[0]
    fd = [(f(dmean=h) - f(dmean=-h)) / (2 * h),
          (f(dcov=(h, 0)) - f(dcov=(-h, 0))) / (2 * h), (f(dcov=(0, h)) - f(dcov=(0, -h))) / (2 * h),
          (f(dlik=h) - f(dlik=-h)) / (2 * h)]
    assert np.max(np.abs(g - fd) / np.maximum(1.0, np.abs(fd))) <= 1e-4, (g, fd)


def _dense_vs_program(n, d=3, seed=0):
    """pgp_ep_fit_dense_lik on the host-built K against pgp_ep_fit_lik on the device program, same data."""
    from pygps_amd import _lib, inf
    rng = np.random.RandomState(seed)
    x = rng.randn(n, d)
    y = np.sin(x.sum(1, keepdims=True)) + 0.1 * rng.standard_t(3, size=(n, 1))
    m = _model(x, y, [np.log(1.1), np.log(0.8)], [np.log(0.2)])
    nlZ, dnlZ, post = m.getPosterior()
    K = O.cov_matrix(O.RBF, np.array(m.covfunc.hyp), 0, x=x, mode="train")
    lib = _lib.load()
    inf._Resident.ensure(x, y.ravel(), _lib.default_device())
    mv = m.meanfunc.hyp[0] * np.ones(n)
    dm = np.ones(n)
    lh = np.array(m.likfunc.hyp, dtype=float)
    ttau, tnu, alpha, sW, nz, g = np.zeros(n), np.zeros(n), np.empty(n), np.empty(n), np.zeros(1), np.zeros(2)
    sweeps, fh = C.c_int(), C.c_void_p()
    _lib.check(lib.pgp_ep_fit_dense_lik(_lib.ctx(), _lib.ptr(K), _lib.LIK_LAPLACE, _lib.ptr(lh), 1, 0, _lib.ptr(mv), _lib.ptr(dm), 1,
                                        3, 0, _lib.ptr(ttau), _lib.ptr(tnu), _lib.ptr(alpha), _lib.ptr(sW), _lib.ptr(nz),
                                        _lib.ptr(g), C.byref(sweeps), C.byref(fh)), "pgp_ep_fit_dense_lik")
    lib.pgp_factor_free(_lib.ctx(), fh)
    assert sweeps.value == m.inffunc.sweeps
    assert abs(nz[0] - nlZ) <= 1e-9 * max(1.0, abs(nlZ))
    assert relerr(alpha, post.alpha.ravel()) <= 1e-7
    assert relerr(g, [dnlZ.mean[0], dnlZ.lik[0]]) <= 1e-7
    return m, x, y, nlZ, dnlZ, post


@pytest.mark.parametrize("n", [1, 127, 129])
def test_ragged_against_restatement(n):
    m, x, y, nlZ, dnlZ, post = _dense_vs_program(n, seed=n)
    K = O.cov_matrix(O.RBF, np.array(m.covfunc.hyp), 0, x=x, mode="train")
    dK = [O.der_matrix(O.RBF, np.array(m.covfunc.hyp), 0, x=x, mode="train", der=h) for h in range(2)]
    r = ep_laplace_fit(K, y, m.meanfunc.hyp[0] * np.ones(n), m.likfunc.hyp[0], dm=[np.ones(n)], dK=dK)
    assert m.inffunc.sweeps == r["sweeps"]
    assert abs(nlZ - r["nlZ"]) <= 1e-8 * max(1.0, abs(r["nlZ"]))
    assert relerr(post.alpha.ravel(), r["alpha"]) <= 1e-6
    assert relerr(np.array(dnlZ.mean + dnlZ.cov + dnlZ.lik), np.concatenate([r["dnlZ_mean"], r["dnlZ_cov"], r["dnlZ_lik"]])) <= 1e-6


def test_large_ragged_dense_equals_program():
    m, x, y, nlZ, dnlZ, post = _dense_vs_program(4500, seed=3)
    assert np.all(np.isfinite(post.alpha)) and np.all(np.isfinite(dnlZ.cov))


def test_erf_through_the_lik_entry_point_is_bitwise_pgp_ep_fit():
    from pygps_amd import _lib, inf
    rng = np.random.RandomState(4)
    n = 300
    x = rng.randn(n, 3)
    y = np.sign(x[:, 0] + 0.3 * rng.randn(n))
    y[y == 0] = 1
    inf._Resident.ensure(x, y, _lib.default_device())
    lib = _lib.load()
    hyp = np.array([0.2, 0.1])
    res = []
    for which in (0, 1):
        ttau, tnu, alpha, sW, nz, g = np.zeros(n), np.zeros(n), np.empty(n), np.empty(n), np.zeros(1), np.zeros(3)
        sweeps, fh = C.c_int(), C.c_void_p()
        mv, dm = np.zeros(n), np.zeros(n)
        if which == 0:
            rc = lib.pgp_ep_fit(_lib.ctx(), _lib.COV_RBF, _lib.ptr(hyp), 2, 0, 0, _lib.ptr(mv), _lib.ptr(dm), 0, 3, 0, _lib.ptr(ttau),
                                _lib.ptr(tnu), _lib.ptr(alpha), _lib.ptr(sW), _lib.ptr(nz), _lib.ptr(g), C.byref(sweeps), C.byref(fh))
        else:
            rc = lib.pgp_ep_fit_lik(_lib.ctx(), _lib.COV_RBF, _lib.ptr(hyp), 2, 0, 0, _lib.LIK_ERF, None, 0, 0, _lib.ptr(mv),
                                    _lib.ptr(dm), 0, 3, 0, _lib.ptr(ttau), _lib.ptr(tnu), _lib.ptr(alpha), _lib.ptr(sW), _lib.ptr(nz),
                                    _lib.ptr(g), C.byref(sweeps), C.byref(fh))
        _lib.check(rc, "ep fit")
        lib.pgp_factor_free(_lib.ctx(), fh)
        res.append(np.concatenate([ttau, tnu, alpha, nz, g, [sweeps.value]]))
    assert np.array_equal(res[0], res[1])
    bad = lib.pgp_ep_fit_lik(_lib.ctx(), _lib.COV_RBF, _lib.ptr(hyp), 2, 0, 0, _lib.LIK_GAUSS, _lib.ptr(hyp), 1, 0, None, None, 0, 3,
                             0, _lib.ptr(ttau), _lib.ptr(tnu), None, None, None, None, None, None)
    assert bad == -15


def test_optimize_trains_log_sigma():
    """optimize() trains log_sigma.  The reference's optimum (G22 demo, reached with its gradients) is a point at which the device's
    nlZ must equal the recorded one; optimising with the correct gradients ends no higher."""
    z = golden("G22_lik_laplace_demo")
    ref = _model(z["x"], z["y"], z["opt_cov_hyp"], z["opt_lik_hyp"])
    ref.meanfunc.hyp = [float(v) for v in z["opt_mean_hyp"]]
    nlZ_ref = ref.getPosterior(der=False)[0]
    assert abs(nlZ_ref - float(z["opt_nlZ"])) <= 1e-8 * max(1.0, abs(float(z["opt_nlZ"])))
    ym, ys2, fm, fs2, lp = ref.predict(z["xstar"], ys=np.sin(z["xstar"]))
    assert relerr(ym, z["opt_ym"]) <= 1e-6 and relerr(fs2, z["opt_fs2"]) <= 1e-6
    m = _model(z["x"], z["y"])
    nlZ0 = m.getPosterior(der=False)[0]
    h0 = m.likfunc.hyp[0]
    m.optimize()
    assert m.likfunc.hyp[0] != h0
    assert m.nlZ < nlZ0 and m.nlZ <= nlZ_ref + 1e-6 * abs(nlZ_ref)
    nlZ, dnlZ, _ = m.getPosterior()
    assert abs(nlZ - m.nlZ) <= 1e-8 * max(1.0, abs(nlZ))


# ---- FITC_EP + lik.Laplace (GPR_FITC.useLikelihood("Laplace"), Core/gp.py:1104-1114; Core/inf.py:810-944) ----------------
def _fitc_model(x, y, u, cov_hyp, lik_hyp, mean_hyp, compat=False):
    import pygps_amd as pyGPs
    m = pyGPs.GPR_FITC()
    m.useLikelihood("Laplace")
    m.setPrior(mean=pyGPs.mean.Const(float(mean_hyp[0])) if len(mean_hyp) else pyGPs.mean.Zero(),
               kernel=pyGPs.cov.RBF(float(cov_hyp[0]), float(cov_hyp[1])), inducing_points=u)
    m.setData(x, y)
    m.likfunc.hyp = [float(v) for v in lik_hyp]
    m.inffunc.reference_compat = compat
    return m


def _fitc_kt(x, u, cov_hyp, lik_hyp):
    """The explicit FITC covariance Kt = Q + diag(K - Q), Q = Ku' inv(Kuu + snu2 I) Ku, snu2 = 1e-6 sn2 (inf.py:837-848)."""
    snu2 = 1e-6 * np.exp(2 * lik_hyp[0])
    Kuu = O.cov_matrix(O.RBF, cov_hyp, 0, x=u, mode="train")
    Ku = O.cov_matrix(O.RBF, cov_hyp, 0, x=u, z=x, mode="cross")
    Q = Ku.T @ np.linalg.solve(Kuu + snu2 * np.eye(len(u)), Ku)
    kss = np.exp(2 * cov_hyp[1])
    return Q + np.diag(kss - np.diag(Q))


def test_G22_fitc_fit_against_restatement_on_kt():
    """The reference's FITC_EP with lik.Laplace ends with nlZ = NaN on this problem (recorded as such: NaN fails its convergence
    test, so it stops after min_sweep = 2), which leaves nothing to compare with.  The device is held to the CPU restatement of
    dense EP on the explicit Kt instead (same snu2 = 1e-6 sn2), and to the reference's predictive machinery through it."""
    z = golden("G22_fitc_lik_laplace_const_N1500_nu100")
    assert np.isnan(float(z["nlZ"])) and int(z["sweeps"]) == 2
    m = _fitc_model(z["x"], z["y"], z["u"], z["cov_hyp"], z["lik_hyp"], z["mean_hyp"])
    nlZ, dnlZ, post = m.getPosterior()
    n = len(z["y"])
    r = ep_laplace_fit(_fitc_kt(z["x"], z["u"], z["cov_hyp"], z["lik_hyp"]), z["y"], z["mean_hyp"][0] * np.ones(n), z["lik_hyp"][0],
                       dm=[np.ones(n)])
    assert m.inffunc.sweeps == r["sweeps"]
    assert abs(nlZ - r["nlZ"]) <= 1e-8 * max(1.0, abs(r["nlZ"]))
    # (site parameters converged to the sweep tolerance 1e-4 in nlZ, reached by two different arithmetic paths)
    assert relerr(m.inffunc.last_ttau.ravel(), r["ttau"]) <= 1e-5 and relerr(m.inffunc.last_tnu.ravel(), r["tnu"]) <= 1e-5
    assert relerr(dnlZ.mean, r["dnlZ_mean"]) <= 1e-5


def test_fitc_against_dense_ep_on_kt():
    import pygps_amd as pyGPs
    z = golden("G22_fitc_lik_laplace_const_N1500_nu100")
    x, y, u = z["x"][:700], z["y"][:700], z["u"][:60]
    m = _fitc_model(x, y, u, z["cov_hyp"], z["lik_hyp"], z["mean_hyp"])
    nlZ, dnlZ, post = m.getPosterior()
    Kt = _fitc_kt(x, u, z["cov_hyp"], z["lik_hyp"])
    from pygps_amd import _lib, inf
    n = len(y)
    inf._Resident.ensure(x, y.ravel(), _lib.default_device())
    lh = np.array(z["lik_hyp"], dtype=float)
    mv, dm = m.meanfunc.hyp[0] * np.ones(n), np.ones(n)
    ttau, tnu, alpha, sW, nz, g = np.zeros(n), np.zeros(n), np.empty(n), np.empty(n), np.zeros(1), np.zeros(2)
    sweeps, fh = C.c_int(), C.c_void_p()
    lib = _lib.load()
    _lib.check(lib.pgp_ep_fit_dense_lik(_lib.ctx(), _lib.ptr(Kt), _lib.LIK_LAPLACE, _lib.ptr(lh), 1, 0, _lib.ptr(mv), _lib.ptr(dm),
                                        1, 3, 0, _lib.ptr(ttau), _lib.ptr(tnu), _lib.ptr(alpha), _lib.ptr(sW), _lib.ptr(nz),
                                        _lib.ptr(g), C.byref(sweeps), C.byref(fh)), "pgp_ep_fit_dense_lik")
    lib.pgp_factor_free(_lib.ctx(), fh)
    assert sweeps.value == m.inffunc.sweeps
    assert abs(nz[0] - nlZ) <= 1e-8 * max(1.0, abs(nlZ))
    assert relerr(m.inffunc.last_ttau.ravel(), ttau) <= 1e-6 and relerr(m.inffunc.last_tnu.ravel(), tnu) <= 1e-6
    assert abs(g[0] - dnlZ.mean[0]) <= 1e-6 * max(1.0, abs(g[0]))      # the mean gradient: same cavities, same point


def test_fitc_gradients_by_central_differences():
    """Every entry, dnlZ.lik with its snu2 term included, against central differences of the device's own nlZ; with a Const
    mean the reference's dlZhyp point nu_n / tau_n + m is off (reference_compat), the default is not."""
    z = golden("G22_fitc_lik_laplace_const_N1500_nu100")
    x, y, u = z["x"][:500], z["y"][:500], z["u"][:40]

    def fit(dmean=0.0, dcov=(0.0, 0.0), dlik=0.0, der=False, compat=False):
        m = _fitc_model(x, y, u, np.array(z["cov_hyp"]) + np.array(dcov), np.array(z["lik_hyp"]) + dlik,
                        np.array(z["mean_hyp"]) + dmean, compat=compat)
        m.inffunc._tol_exp = 12
        return m.getPosterior() if der else m.getPosterior(der=False)[0]
    nlZ, dnlZ, _ = fit(der=True)
    g = np.array(dnlZ.mean + dnlZ.cov + dnlZ.lik)
    h = 1e-3
    fd = np.array([(fit(dmean=h) - fit(dmean=-h)) / (2 * h), (fit(dcov=(h, 0)) - fit(dcov=(-h, 0))) / (2 * h),
                   (fit(dcov=(0, h)) - fit(dcov=(0, -h))) / (2 * h), (fit(dlik=h) - fit(dlik=-h)) / (2 * h)])
    # (as tests/test_gpu_fitc_ep.py for lik.Erf: the FITC sweeps' nlZ is good to ~1e-3 relative in its differences; the mean
    # gradient alone is pinned to dense EP on Kt to 1e-6 above)
    assert np.max(np.abs(g - fd) / np.maximum(1.0, np.abs(fd))) <= 5e-3, (g, fd)
    gc = fit(der=True, compat=True)[1].lik[0]
    assert abs(g[3] - fd[3]) < 0.5 * abs(gc - fd[3])          # the reference's point is the further one


def test_fitc_large():
    """n = 65536, nu = 512: finite, and the ragged last block (n not a multiple of 128) on the way."""
    rng = np.random.RandomState(12)
    n, d, nu = 65536, 4, 512
    x = rng.randn(n, d)
    y = np.sin(x[:, :1]) + 0.1 * rng.standard_t(3, size=(n, 1))
    u = x[rng.choice(n, nu, replace=False)]
    m = _fitc_model(x, y, u, [np.log(1.4), 0.0], [np.log(0.15)], [float(np.mean(y))])
    nlZ, dnlZ, post = m.getPosterior()
    assert np.isfinite(nlZ) and 2 <= m.inffunc.sweeps <= 10
    assert np.all(np.isfinite(post.alpha)) and np.all(np.isfinite(dnlZ.mean + dnlZ.cov + dnlZ.lik))
    m2 = _fitc_model(x[:4500], y[:4500], u[:128], [np.log(1.4), 0.0], [np.log(0.15)], [float(np.mean(y))])
    nlZ2, dnlZ2, post2 = m2.getPosterior()
    assert np.isfinite(nlZ2) and np.all(np.isfinite(post2.alpha))
