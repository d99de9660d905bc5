"""GPU: learned FITC inducing inputs -- d nlZ / d xu of GPR_FITC, GPR_FITC + lik.Laplace and GPC_FITC (csrc/fitc_xu.hip through
pgp_fitc_fit_xu / pgp_fitc_ep_fit_lik_xu), the contraction kernel alone (pgp_test_fitc_xu_contract) and optimize() with
GP_FITC.learnInducing, against the long-double reference tests/fitc_xu_ref_ld.py under its tolerance rule (bar + summation bound +
4 ulps of the absolute terms + 8 x the measured float64 error, capped at 1e-5 max |gradient|) and against central differences of the
device's own nlZ.

Worst |device - reference| / tolerance measured on the MI355X (2026-10-21; every test prints its own):
    contraction alone      RBF 0.088, RBFunit 0.084, RBFard 0.093, RQ 0.088, RQard 0.126, Matern3 0.089, Matern5 0.108, Matern7 0.165
                           (the ARD kinds with D = 65 at every n)
    GPR_FITC               demo grid 0.265, (300, 25, 2) Matern3 0.040, (700, 77, 3) RBF 0.023 and RQard 0.022, u a subset of x 0.029,
                           Const mean 0.093, (1500, 160, 4) RBF 0.016, Matern5 0.014, RBFard 0.008
    GPC_FITC               0.036        GPR_FITC + lik.Laplace   0.033
The GPC_FITC case takes the data, inducing points and mean of test_gpu_fitc_ep.test_central_differences_every_hyper with the RBFard
leaf of that test's kernel: its Sum is a device program, for which the gradient w.r.t. xu is not built.

End to end: minimize.run over the float64 restatement of tests/fitc_xu_ref_ld.py (hyper-gradients by central differences) from the
start of the test reaches nlZ = -60.3 with the eight inducing points fixed in the left half and -145.1 with them learned (E2E_SEED
= 2), so the reference itself shows the gap the test asserts."""
import ctypes as C

import numpy as np
import pytest

import fitc_xu_ref_ld as R
from conftest import golden, synth_cls, synth_reg

pytestmark = pytest.mark.gpu


def _kind(name):
    from pygps_amd import _lib
    return {"RBF": (_lib.COV_RBF, 0), "RBFunit": (_lib.COV_RBFUNIT, 0), "RBFard": (_lib.COV_RBFARD, 0), "RQ": (_lib.COV_RQ, 0),
            "RQard": (_lib.COV_RQARD, 0), "Matern3": (_lib.COV_MATERN, 3), "Matern5": (_lib.COV_MATERN, 5),
            "Matern7": (_lib.COV_MATERN, 7)}[name]


def _hyp(name, D, rng):
    """Length scales of the order of the spread of D standard-normal coordinates: scaled distances of order one."""
    ell = 0.5 * np.log(D) + 0.3
    if name in ("RBFard", "RQard"):
        h = list(ell + 0.2 * rng.randn(D)) + [0.1]
        return h + [0.4] if name == "RQard" else h
    return {"RBF": [ell, 0.1], "RBFunit": [ell], "RQ": [ell, 0.1, 0.4]}.get(name, [ell, 0.1])


def _device_contract(name, hyp, rows, cols, A):
    from pygps_amd import _lib
    kind, para = _kind(name)
    rows, A = _lib.f64(rows), _lib.f64(A)
    cols = None if cols is None else _lib.f64(cols)
    h = _lib.f64(np.asarray(hyp, dtype=float))
    out = np.full(rows.shape, np.nan)
    rc = _lib.load().pgp_test_fitc_xu_contract(_lib.ctx(), kind, _lib.ptr(h), len(h), para, 0, rows.shape[1], _lib.ptr(rows),
                                               rows.shape[0], _lib.ptr(cols), 0 if cols is None else cols.shape[0], _lib.ptr(A),
                                               _lib.ptr(out))
    assert rc == 0, rc
    return out


def _check_contract(name, hyp, rows, cols, A, worst):
    got = _device_contract(name, hyp, rows, cols, A)
    again = _device_contract(name, hyp, rows, cols, A)
    assert np.array_equal(got, again)                                   # fixed-order sums: repeatable bit for bit
    cc = rows if cols is None else cols
    ref = R.contract(name, hyp, rows, cc, A)
    e64 = float(np.abs(R.contract(name, hyp, rows, cc, A, np.float64).astype(R.LD) - ref).max())
    bar, T = R.contract_bars(name, hyp, rows, cc, A)
    tol = R.tolerance(bar, T, cc.shape[0], e64)
    ref = ref.astype(np.float64)
    assert np.all(np.isfinite(got))
    assert tol.max() <= R.CAP * np.abs(ref).max(), (name, rows.shape, cc.shape, tol.max(), np.abs(ref).max())
    ratio = float((np.abs(got - ref) / tol).max())
    worst[0] = max(worst[0], ratio)
    assert ratio <= 1.0, (name, rows.shape, cc.shape, ratio)
    return got


@pytest.mark.parametrize("name", R.KINDS)
def test_contraction_alone_against_long_double(name):
    """Every (nu, n, D) of the tile edges, rows that coincide with columns, a column so far away that exp underflows, and the
    inducing-against-inducing call; each run twice and compared bit for bit."""
    worst = [0.0]
    dims = (1, 3, 17) + ((65,) if name in ("RBFard", "RQard") else ())
    for D in dims:
        for nu in (1, 63, 64, 65, 129):
            rng = np.random.RandomState(1000 * D + nu)
            hyp = _hyp(name, D, rng)
            rows = rng.randn(nu, D)
            for n in (1, 64, 65, 1000):
                cols = rng.randn(n, D)
                nco = min(nu, n - 1, 3)
                cols[:nco] = rows[:nco]                                 # coincident points: k' is finite there, the difference zero
                A = rng.randn(nu, n)
                far = n >= 8
                if far:
                    cols[-1] = rows[0] + 1e3 * np.exp(max(hyp[:D] if name in ("RBFard", "RQard") else hyp[:1]))
                got = _check_contract(name, hyp, rows, cols, A, worst)
                if far and not name.startswith("RQ"):                   # exp underflows: the far column contributes an exact zero
                    A0 = A.copy()
                    A0[:, -1] = 0.0
                    assert np.array_equal(got, _device_contract(name, hyp, rows, cols, A0))
            if nu > 1:                                                  # inducing against inducing (one point alone gives an exact 0)
                _check_contract(name, hyp, rows, None, rng.randn(nu, nu), worst)
    print("worst ratio, contraction, %s: %.3f" % (name, worst[0]))


# ---- GPR_FITC: the full gradient ----------------------------------------------------------------------------------------------
def _cov(name, hyp):
    from pygps_amd import cov
    h = [float(v) for v in hyp]
    if name == "RBF":
        return cov.RBF(h[0], h[1])
    if name == "RBFunit":
        return cov.RBFunit(h[0])
    if name == "RBFard":
        return cov.RBFard(log_ell_list=h[:-1], log_sigma=h[-1])
    if name == "RQ":
        return cov.RQ(h[0], h[1], h[2])
    if name == "RQard":
        return cov.RQard(log_ell_list=h[:-2], log_sigma=h[-2], log_alpha=h[-1])
    return cov.Matern(h[0], int(name[-1]), h[1])


def _exact_cases():
    cases = {}
    rng = np.random.RandomState(11)
    x = np.linspace(-4, 4, 20)[:, None] + 0.05 * rng.randn(20, 1)
    y = np.sin(x) + 0.1 * rng.randn(20, 1)
    cases["demo_grid"] = ("RBF", [0.0, 0.0], np.log(0.1), x, y, np.linspace(x.min(), x.max(), 5)[:, None], None)
    x, y = synth_reg(300, 2, seed=3)
    cases["n300_matern3"] = ("Matern3", [0.6, 0.1], np.log(0.2), x, y, np.random.RandomState(4).randn(25, 2), None)
    rng = np.random.RandomState(5)
    x = rng.randn(700, 3)
    y = np.sin(x.sum(1, keepdims=True)) + 0.1 * rng.randn(700, 1)
    u = x[rng.choice(700, 77, replace=False)] + 0.05 * rng.randn(77, 3)
    cases["ragged_rbf"] = ("RBF", [0.4, 0.2], np.log(0.2), x, y, u, None)
    cases["ragged_rqard"] = ("RQard", [0.5, 0.3, 0.6, 0.1, 0.5], np.log(0.2), x, y, u, None)
    cases["subset_matern7"] = ("Matern7", [0.7, 0.0], np.log(0.3), x[:300], y[:300], x[:300][::12].copy(), None)
    cases["const_mean_rq"] = ("RQ", [0.5, 0.1, 0.3], np.log(0.2), x[:300], y[:300] + 0.7, x[:300][5::15] + 0.1, 0.7)
    x, y = synth_reg(1500, 4)
    for nm, name in (("rbf", "RBF"), ("matern5", "Matern5"), ("rbfard", "RBFard")):
        g = golden("G12_fitc_%s_N1500_nu160" % nm)
        cases["G12_" + nm] = (name, [float(v) for v in g["cov_hyp"]], float(g["lik_hyp"][0]), x, y, np.array(g["u"]), None)
    return cases


EXACT = None


def _exact(key):
    global EXACT
    if EXACT is None:
        EXACT = _exact_cases()
    return EXACT[key]


def _gpr(name, hyp, log_sn, x, y, u, cmean, learn):
    import pygps_amd as pyGPs
    m = pyGPs.GPR_FITC()
    m.setPrior(mean=pyGPs.mean.Zero() if cmean is None else pyGPs.mean.Const(cmean), kernel=_cov(name, hyp), inducing_points=u.copy())
    m.setNoise(log_sn)
    m.learnInducing(learn)
    return m


@pytest.mark.parametrize("key", ["demo_grid", "n300_matern3", "ragged_rbf", "ragged_rqard", "subset_matern7", "const_mean_rq",
                                 "G12_rbf", "G12_matern5", "G12_rbfard"])
def test_gpr_fitc_gradient_against_long_double_and_flag_changes_nothing_else(key):
    name, hyp, log_sn, x, y, u, cmean = _exact(key)
    xs = x[:7] + 0.05
    out = []
    for learn in (False, True):
        m = _gpr(name, hyp, log_sn, x, y, u, cmean, learn)
        nlZ, dnlZ, post = m.getPosterior(x, y)
        pred = m.predict(xs)
        out.append((nlZ, dnlZ, post, pred))
    (n0, d0, p0, q0), (n1, d1, p1, q1) = out
    assert d0.xu is None and d1.xu.shape == u.shape
    assert n0 == n1 and d0.mean == d1.mean and d0.cov == d1.cov and d0.lik == d1.lik           # bit for bit
    assert np.array_equal(p0.alpha, p1.alpha) and np.array_equal(p0.L, p1.L)
    for a, b in zip(q0, q1):
        assert np.array_equal(a, b)
    mvec = np.zeros(x.shape[0]) if cmean is None else np.full(x.shape[0], cmean)
    ref, tol, e64 = R.exact_case(name, hyp, log_sn, x, y, mvec, u)
    assert tol.max() <= R.CAP * np.abs(ref).max(), (key, tol.max(), np.abs(ref).max())
    ratio = float((np.abs(d1.xu - ref) / tol).max())
    print("worst ratio, GPR_FITC %s: %.3f (e64 %.2e, max |g| %.3g)" % (key, ratio, e64, np.abs(ref).max()))
    assert ratio <= 1.0, (key, ratio)


def test_gpr_fitc_directional_central_difference():
    """The device's own nlZ along dnlZ.xu at (700, 77, 3), e = 1e-5, as test_fitc_against_oracle_ragged_sizes_and_gradient_fd does for
    the hyper-parameters."""
    name, hyp, log_sn, x, y, u, cmean = _exact("ragged_rbf")
    m = _gpr(name, hyp, log_sn, x, y, u, cmean, True)
    g = m.getPosterior(x, y)[1].xu
    nrm = np.linalg.norm(g)
    e = 1e-5
    vals = []
    for sgn in (1, -1):
        m.covfunc.inducingInput = u + sgn * e * g / nrm
        vals.append(m.getPosterior(x, y, der=False)[0])
    assert abs((vals[0] - vals[1]) / (2 * e) - nrm) < 1e-4 * nrm, ((vals[0] - vals[1]) / (2 * e), nrm)


# ---- FITC_EP: GPC_FITC and GPR_FITC + lik.Laplace -------------------------------------------------------------------------------
def _gpc():
    """Data, inducing points and mean of test_gpu_fitc_ep.test_central_differences_every_hyper with the RBFard leaf of its kernel (its
    Sum is a device program: out of scope for the gradient w.r.t. xu)."""
    import pygps_amd as pyGPs
    x, y = synth_cls(700, 3, seed=7)
    u = np.random.RandomState(8).randn(40, 3)
    hyp = [0.3, 0.5, 0.1, 0.2]
    m = pyGPs.GPC_FITC()
    m.setPrior(mean=pyGPs.mean.Const(0.2), kernel=_cov("RBFard", hyp), inducing_points=u.copy())
    m.learnInducing()
    return m, x, y, u, hyp


def test_gpc_fitc_gradient_at_the_final_sites_and_central_difference():
    import pygps_amd as pyGPs
    m, x, y, u, hyp = _gpc()
    m.getPosterior(x, y)
    nlZ, dnlZ, _ = m.getPosterior(x, y)
    base = (m.inffunc.last_ttau.copy(), m.inffunc.last_tnu.copy())
    ref, tol, e64 = R.sites_case("RBFard", hyp, 1e-6, x, u, base[0], base[1])
    assert tol.max() <= R.CAP * np.abs(ref).max()
    ratio = float((np.abs(dnlZ.xu - ref) / tol).max())
    print("worst ratio, GPC_FITC: %.3f (e64 %.2e)" % (ratio, e64))
    assert ratio <= 1.0, ratio
    g = dnlZ.xu
    nrm = np.linalg.norm(g)
    e = 1e-5
    vals = []
    for sgn in (1, -1):
        f = pyGPs.inf.FITC_EP()
        f.last_ttau, f.last_tnu = base[0].copy(), base[1].copy()
        m.inffunc = f
        m.covfunc.inducingInput = u + sgn * e * g / nrm
        vals.append(m.getPosterior(x, y, der=False)[0])
    fd = (vals[0] - vals[1]) / (2 * e)
    assert abs(fd - nrm) < 1e-3 * max(1.0, nrm), (fd, nrm)


def test_gpr_fitc_laplace_likelihood_gradient_at_the_final_sites():
    import pygps_amd as pyGPs
    x, y = synth_reg(300, 2, seed=13)
    u = np.random.RandomState(14).randn(30, 2)
    hyp = [0.5, 0.1]
    m = pyGPs.GPR_FITC()
    m.setPrior(mean=pyGPs.mean.Zero(), kernel=_cov("Matern5", hyp), inducing_points=u.copy())
    m.useLikelihood("Laplace")
    m.likfunc.hyp = [np.log(0.2)]
    m.learnInducing()
    nlZ, dnlZ, _ = m.getPosterior(x, y)
    ref, tol, e64 = R.sites_case("Matern5", hyp, 1e-6 * np.exp(2 * np.log(0.2)), x, u, m.inffunc.last_ttau, m.inffunc.last_tnu)
    assert tol.max() <= R.CAP * np.abs(ref).max()
    ratio = float((np.abs(dnlZ.xu - ref) / tol).max())
    print("worst ratio, GPR_FITC + lik.Laplace: %.3f (e64 %.2e)" % (ratio, e64))
    assert ratio <= 1.0, ratio


# ---- end to end ---------------------------------------------------------------------------------------------------------------
E2E_SEED = 2


def _e2e_data():
    rng = np.random.RandomState(E2E_SEED)
    x = np.sort(rng.uniform(-3, 3, (200, 1)), axis=0)
    y = np.sin(2 * x) + 0.1 * rng.randn(200, 1)
    u = np.linspace(-3, -0.5, 8)[:, None]                      # every inducing point in the left half
    return x, y, u


def _e2e_model(learn, u):
    import pygps_amd as pyGPs
    m = pyGPs.GPR_FITC()
    m.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(0.0, 0.0), inducing_points=u.copy())
    m.setNoise(np.log(0.3))
    m.learnInducing(learn)
    return m


def test_optimize_moves_the_inducing_inputs_and_beats_the_fixed_ones():
    import pygps_amd as pyGPs
    x, y, u = _e2e_data()
    fixed = _e2e_model(False, u)
    fixed.optimize(x, y, numIterations=20)
    m = _e2e_model(True, u)
    m.optimize(x, y, numIterations=20)
    assert m.nlZ < fixed.nlZ - 1.0, (m.nlZ, fixed.nlZ)
    assert np.array_equal(fixed.u, u) and np.abs(m.u - u).max() > 0.1
    assert m.u is m.covfunc.inducingInput or np.array_equal(m.u, m.covfunc.inducingInput)
    xs = np.linspace(-3, 3, 50)[:, None]
    pred = m.predict(xs)
    fresh = pyGPs.GPR_FITC()
    fresh.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(*[float(v) for v in m.covfunc.hyp]), inducing_points=m.u.copy())
    fresh.setNoise(float(m.likfunc.hyp[0]))
    fresh.getPosterior(x, y)
    for a, b in zip(pred, fresh.predict(xs)):
        assert np.array_equal(a, b)


def test_random_restarts_with_learned_inducing_inputs_finish():
    x, y, u = _e2e_data()
    m = _e2e_model(True, u)
    m.setOptimizer("Minimize", num_restarts=2, covRange=[(-1.0, 1.0), (-1.0, 1.0)], likRange=[(-3.0, 0.0)])
    np.random.seed(3)
    m.optimize(x, y, numIterations=10)
    assert np.isfinite(m.nlZ) and m.u.shape == u.shape and np.array_equal(m.u, m.covfunc.inducingInput)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_return_before_device_work_and_leave_the_context_usable():
    import pygps_amd as pyGPs
    from pygps_amd import _lib
    name, hyp, log_sn, x, y, u, cmean = _exact("n300_matern3")
    before = _gpr(name, hyp, log_sn, x, y, u, cmean, False).getPosterior(x, y)
    lib, ctx = _lib.load(), _lib.ctx()
    xu, h = _lib.f64(u), _lib.f64(np.array([0.1, 0.2]))
    out = np.zeros(u.shape)
    scratch = [np.zeros(u.shape[0]), np.zeros((u.shape[0],) * 2), np.zeros(1), np.zeros(3)]
    for kind, para, hh in ((_lib.COV_MATERN, 1, h), (_lib.COV_PIECEPOLY, 2, h), (_lib.COV_GABOR, 0, h), (_lib.COV_COMPOSITE, 0, h),
                           (_lib.COV_PERIODIC, 0, np.append(h, 0.3)),
                           (_lib.COV_CONST, 0, h[:1]), (_lib.COV_NOISE, 0, h[:1]), (_lib.COV_SM, 1, h)):
        fh = C.c_void_p()
        rc = lib.pgp_fitc_fit_xu(ctx, kind, _lib.ptr(hh), len(hh), para, 0, log_sn, _lib.ptr(xu), u.shape[0], None, None, 0, 3,
                                 _lib.ptr(scratch[0]), _lib.ptr(scratch[1]), _lib.ptr(scratch[2]), _lib.ptr(scratch[3]), C.byref(fh),
                                 _lib.ptr(out))
        assert rc == _lib.ERR_XU_UNSUPPORTED and not fh.value, (kind, rc)
        assert "inducing" in _lib.strerror(rc)
    m = _gpr("Matern3", hyp, log_sn, x, y, u, cmean, False)
    m.setPrior(kernel=pyGPs.cov.Matern(0.1, 1, 0.2), inducing_points=u.copy())
    m.learnInducing()
    with pytest.raises(NotImplementedError, match="Matern"):
        m.getPosterior(x, y)
    after = _gpr(name, hyp, log_sn, x, y, u, cmean, False).getPosterior(x, y)
    assert before[0] == after[0] and before[1].cov == after[1].cov and np.array_equal(before[2].alpha, after[2].alpha)
