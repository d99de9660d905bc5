"""CPU: pin the Laplace oracle (oracle/gp_oracle.py laplace_fit, brent_min and the Laplace-mode likelihoods) to the G20
recordings of the reference, and check it where no recording reaches -- ARD, Matern, RQard, a Linear + Const mean, the Gauss
likelihood's hyper-parameter -- by the mode's fixed-point equation, central differences of nlZ and, for the Gauss
likelihood, the exact fit.  tests/test_gpu_laplace_oracle.py compares the device with this oracle."""
import numpy as np
import pytest

from conftest import golden, relerr, synth_cls, synth_reg
from oracle import gp_oracle as O

# With the reference's own LU solves (faithful=True) the oracle takes the reference's Newton and line-search path bit for bit:
# every measured difference below is 0 or a few ulps (nlZ <= 5e-16, alpha / sW / L 0, gradients <= 3e-15).
TOL_NLZ = 1e-14
TOL = 1e-13


def check_steps(out, g, prefix=""):
    """Newton count equal; Psi on every step; s on every step that lowers Psi by more than 1e-3 (the rule of
    tests/test_gpu_laplace.py) -- measured: both exact."""
    n_ref = int(g[prefix + "newton_steps"]) if prefix + "newton_steps" in g.files else len(g[prefix + "step_s"])
    assert out["newton_steps"] == n_ref
    s_ref, psi_ref = g[prefix + "step_s"], g[prefix + "step_psi"]
    st = out["steps"]
    assert st.shape == (n_ref, 3)
    if prefix + "step_nfun" in g.files:
        assert np.array_equal(st[:, 2], g[prefix + "step_nfun"])
    prev = np.inf
    for k in range(n_ref):
        if prev - psi_ref[k] > 1e-3:
            assert abs(st[k, 0] - s_ref[k]) <= 1e-12, (k, st[k, 0], s_ref[k])
        assert abs(st[k, 1] - psi_ref[k]) <= 1e-14 * abs(psi_ref[k]), (k, st[k, 1], psi_ref[k])
        prev = psi_ref[k]


def check_fit(out, g, prefix="", L_full=False):
    keys = g.files
    assert abs(out["nlZ"] - float(g[prefix + "nlZ"])) <= TOL_NLZ * abs(float(g[prefix + "nlZ"]))
    assert relerr(out["alpha"], g[prefix + "alpha"]) <= TOL
    assert relerr(out["sW"], g[prefix + "sW"]) <= TOL
    assert np.all(np.tril(out["L"], -1) == 0)
    if L_full:
        assert relerr(out["L"], g[prefix + "L"]) <= TOL
    else:
        assert relerr(np.diag(out["L"]), g[prefix + "L_diag"]) <= TOL
    if prefix + "L_sample" in keys:
        assert relerr(out["L"].ravel()[::int(g[prefix + "L_stride"])], g[prefix + "L_sample"]) <= TOL
    for k in ("mean", "cov", "lik"):
        want = g[prefix + "dnlZ_" + k]
        assert out["dnlZ_" + k].shape == want.shape, k
        if want.size:
            assert relerr(out["dnlZ_" + k], want) <= 1e-13, k       # measured <= 3e-15


def test_laplace_likelihood_modes_match_reference():
    g = golden("G20_lik_laplace_modes")
    f = g["f"]
    for tag, yv in (("pos", 1.0), ("neg", -1.0)):
        got = O.erf_laplace_derivs(yv * np.ones_like(f), f)
        for a, k in zip(got, ("lp", "dlp", "d2lp", "d3lp")):
            assert np.array_equal(a, g["erf_%s_%s" % (tag, k)]), (tag, k)                # measured: bit for bit
    ls = float(g["gauss_log_sn"])
    got = O.gauss_laplace_derivs(g["gauss_y"], f, ls) + O._gauss_lik_dhyp(g["gauss_y"], f, ls)
    for a, k in zip(got, ("lp", "dlp", "d2lp", "d3lp", "lp_dhyp", "dlp_dhyp", "d2lp_dhyp")):
        assert np.array_equal(a, g["gauss_" + k]), k


def test_laplace_demo_matches_reference():
    g = golden("G20_laplace_demo")
    n = g["x"].shape[0]
    out = O.laplace_fit(O.RBF, g["cov_hyp"], 0, g["x"], g["y"], np.zeros((n, 1)))
    check_steps(out, g)
    check_fit(out, g, L_full=True)
    ym, ys2, fm, fs2 = O.predict(O.RBF, g["cov_hyp"], 0, None, g["x"], out["alpha"], out["L"], out["sW"], g["xstar5"],
                                 np.zeros((5, 1)), gauss=False)
    for got, k in ((ym, "pred_ym"), (ys2, "pred_ys2"), (fm, "pred_fm"), (fs2, "pred_fs2")):
        assert np.max(np.abs(got - g[k])) <= 1e-15, k


@pytest.mark.parametrize("N", [128, 512, 2048])
def test_laplace_d32_matches_reference(N):
    g = golden("G20_laplace_d32_N%d" % N)
    x, y = synth_cls(N, int(g["d"]))
    out = O.laplace_fit(O.RBF, g["cov_hyp"], 0, x, y, np.zeros((N, 1)))
    check_steps(out, g)
    check_fit(out, g)


def test_laplace_const_mean_and_composite_match_reference():
    g = golden("G20_laplace_const_mean_N200")
    n = g["x"].shape[0]
    tree = ("sum", ("prod", ("leaf", O.RBF, 0), ("leaf", O.RQ, 0)), ("leaf", O.CONST, 0))
    out = O.laplace_fit(tree, g["cov_hyp"], 0, g["x"], g["y"], g["mean_hyp"][0] * np.ones((n, 1)), np.ones((n, 1)))
    check_steps(out, g)
    check_fit(out, g)


def test_laplace_dense_tree_matches_reference():
    g = golden("G20_laplace_dense_N200")
    n = g["x"].shape[0]
    ard = ("leaf", O.RBFARD, 0)
    out = O.laplace_fit(("sum", ("prod", ard, ard), ard), g["cov_hyp"], 0, g["x"], g["y"], np.zeros((n, 1)))
    check_steps(out, g)
    check_fit(out, g)


def test_laplace_gauss_matches_reference_and_exact():
    g = golden("G20_laplace_gauss_N300")
    n = g["x"].shape[0]
    out = O.laplace_fit(O.RBF, g["cov_hyp"], 0, g["x"], g["y"], np.zeros((n, 1)), lik="gauss", lik_hyp=g["lik_hyp"])
    check_steps(out, g)
    check_fit(out, g, prefix="laplace_")


def test_laplace_warm_start_matches_reference():
    """G20_laplace_warm_N512: setData gives the model Const(mean(y)); the second call starts from the first call's alpha and
    the reference's Psi_def rule decides whether it is kept."""
    g = golden("G20_laplace_warm_N512")
    x, y = g["x"], g["y"]
    n = x.shape[0]
    m, dm = y.mean() * np.ones((n, 1)), np.ones((n, 1))
    o1 = O.laplace_fit(O.RBF, g["cov_hyp1"], 0, x, y, m, dm)
    assert o1["newton_steps"] == int(g["newton_steps1"])
    assert abs(o1["nlZ"] - float(g["nlZ1"])) <= TOL_NLZ * abs(float(g["nlZ1"])) and relerr(o1["alpha"], g["alpha1"]) <= TOL
    o2 = O.laplace_fit(O.RBF, g["cov_hyp2"], 0, x, y, m, dm, last_alpha=o1["alpha"])
    assert o2["newton_steps"] == int(g["newton_steps2"])
    assert np.all(np.abs(o2["steps"][:, 1] - g["step_psi2"]) <= 1e-14 * np.abs(g["step_psi2"]))
    assert abs(o2["nlZ"] - float(g["nlZ2"])) <= TOL_NLZ * abs(float(g["nlZ2"]))
    assert relerr(o2["alpha"], g["alpha2"]) <= TOL and relerr(o2["sW"], g["sW2"]) <= TOL
    for k in ("mean", "cov"):
        assert relerr(o2["dnlZ_" + k], g["second_dnlZ_" + k]) <= 1e-13, k


# ---- where no recording reaches: the mode equation, central differences, the exact fit ------------------------------------
def _lik(lik, lh):
    if lik == "erf":
        return lambda y, f: O.erf_laplace_derivs(y, f)
    return lambda y, f: O.gauss_laplace_derivs(y, f, lh[0])


def _nlz(kind, hyp, para, x, y, m, dm, lik="erf", lik_hyp=(), compat=False, nargout=3):
    """laplace_fit at tol = 1e-12, then three full Newton steps: the line search finds s only to its fractional precision,
    which leaves the mode ~1e-8 off (test_laplace_mode_solves_its_fixed_point_equation); nlZ's log-determinant moves
    with it to first order, too much for central differences.  The polished mode is handed back (keep_warm, maxit=0) for
    nlZ and the gradients at it."""
    out = O.laplace_fit(kind, hyp, para, x, y, m, dm, lik=lik, lik_hyp=lik_hyp, tol=1e-12, faithful=False, nargout=2)
    K = O.cov_matrix(kind, hyp, para, x=x, mode="train")
    derivs = _lik(lik, lik_hyp)
    alpha = out["alpha"]
    for _ in range(3):
        f = K @ alpha + m
        _, dlp, d2lp, _ = derivs(y, f)
        W = -d2lp
        sW = np.sqrt(W)
        L = O.jitchol(np.eye(len(y)) + (sW @ sW.T) * K).T
        b = W * (f - m) + dlp
        alpha = b - sW * O.solve_chol(L, sW * (K @ b), faithful=False)
    return O.laplace_fit(kind, hyp, para, x, y, m, dm, lik=lik, lik_hyp=lik_hyp, last_alpha=alpha, keep_warm=True, maxit=0,
                         matern_reference_compat=compat, nargout=nargout)


def _linear_const(x, c, w):
    """SumOfMean(Const(c), Linear(w)): m = c + x w, dm = [1, x]."""
    n = x.shape[0]
    return c + x @ np.asarray(w).reshape(-1, 1), np.hstack([np.ones((n, 1)), x])


_RQARD3 = [0.2, -0.1, 0.4, 0.3, 0.5]
CASES = {                               # kind, cov hyp, para, mean, lik
    "rbfard": (O.RBFARD, [0.3, -0.2, 0.5, 0.1, 0.4], 0, "zero", "erf"),
    "matern1": (O.MATERN, [0.3, 0.4], 1, "zero", "erf"),
    "matern3": (O.MATERN, [0.3, 0.4], 3, "zero", "erf"),
    "matern5": (O.MATERN, [0.3, 0.4], 5, "zero", "erf"),
    "matern7": (O.MATERN, [0.3, 0.4], 7, "zero", "erf"),
    "rqard": (O.RQARD, _RQARD3 + [0.0], 0, "zero", "erf"),
    "linear_const_mean": (O.RBF, [0.4, 0.6], 0, "linear_const", "erf"),
    "gauss": (O.RBFARD, [0.3, -0.2, 0.5, 0.1, 0.2], 0, "linear_const", "gauss"),
}


def _case(name, N=80):
    kind, hyp, para, mean, lik = CASES[name]
    D = 4
    if name == "rqard":
        hyp = [0.2, -0.1, 0.4, 0.3, 0.5, 0.0]
    x, y = (synth_reg(N, D, seed=4) if lik == "gauss" else synth_cls(N, D, seed=4))
    if mean == "zero":
        m, dm = np.zeros((N, 1)), None
    else:
        m, dm = _linear_const(x, 0.2, [0.3, -0.4, 0.1, 0.2])
    return kind, np.array(hyp, dtype=float), para, x, y, m, dm, lik, ([np.log(0.3)] if lik == "gauss" else [])


@pytest.mark.parametrize("name", list(CASES))
def test_laplace_mode_solves_its_fixed_point_equation(name):
    """At tol = 1e-12 the converged mode satisfies alpha = dlp(f), f = K alpha + m.  What is left is set by the line search's
    fractional precision (thr = 1e-4 puts s within ~1e-4 of the Newton step), not by the Newton tolerance.  Measured:
    <= 3.2e-8 relative (Gauss, 2 steps), 1.8e-8 (RBFard), <= 1.5e-8 elsewhere."""
    kind, hyp, para, x, y, m, dm, lik, lh = _case(name)
    out = O.laplace_fit(kind, hyp, para, x, y, m, dm, lik=lik, lik_hyp=lh, tol=1e-12, matern_reference_compat=False)
    K = O.cov_matrix(kind, hyp, para, x=x, mode="train")
    f = K @ out["alpha"] + m
    assert relerr(out["alpha"], _lik(lik, lh)(y, f)[1]) <= 1e-7
    if kind in (O.MATERN, O.RQARD):     # the reference's derivative convention changes the gradient, never the mode or nlZ
        ref = O.laplace_fit(kind, hyp, para, x, y, m, dm, lik=lik, lik_hyp=lh, tol=1e-12, matern_reference_compat=True)
        assert ref["nlZ"] == out["nlZ"] and np.array_equal(ref["alpha"], out["alpha"])
        assert not np.allclose(ref["dnlZ_cov"], out["dnlZ_cov"], rtol=1e-3)


@pytest.mark.parametrize("name", list(CASES))
def test_laplace_gradient_by_central_differences(name):
    """Every dnlZ entry (mean, cov, lik) against central differences of nlZ, step 1e-5, the mode converged to 1e-12.  With
    the mathematically correct derivatives (matern_reference_compat=False).  Measured: <= 8e-11 relative to the largest."""
    kind, hyp, para, x, y, m0, dm, lik, lh = _case(name)
    out = _nlz(kind, hyp, para, x, y, m0, dm, lik, lh)
    got = np.concatenate([out["dnlZ_mean"], out["dnlZ_cov"], out["dnlZ_lik"]])
    h = 1e-5
    nm = 0 if dm is None else dm.shape[1]
    mhyp = np.array([0.2, 0.3, -0.4, 0.1, 0.2])
    fd = []
    for part, k in [("mean", i) for i in range(nm)] + [("cov", i) for i in range(len(hyp))] + [("lik", i) for i in range(len(lh))]:
        v = []
        for sg in (1, -1):
            hc, hm, hl = hyp.copy(), mhyp.copy(), np.array(lh, dtype=float)
            {"cov": hc, "mean": hm, "lik": hl}[part][k] += sg * h
            m = m0 if dm is None else _linear_const(x, hm[0], hm[1:])[0]
            v.append(_nlz(kind, hc, para, x, y, m, dm, lik, hl, nargout=2)["nlZ"])
        fd.append((v[0] - v[1]) / (2 * h))
    fd = np.array(fd)
    assert relerr(got, fd) <= 1e-9, (got, fd)


@pytest.mark.parametrize("log_sn", [-3.0, np.log(0.3), 1.5])
def test_laplace_gauss_equals_the_exact_fit(log_sn):
    """With the Gauss likelihood the Laplace approximation is exact: at tol = 1e-12 nlZ, alpha and every gradient equal
    O.exact_fit's.  Measured: nlZ <= 1.3e-15, alpha <= 3e-11, sW 0, gradients <= 3e-10 (log_sn = -3: B = I + K / sn2 is
    the worst conditioned)."""
    kind, hyp, para, x, y, m, dm, lik, _ = _case("gauss", N=97)
    out = _nlz(kind, hyp, para, x, y, m, dm, "gauss", [log_sn])
    ex = O.exact_fit(kind, hyp, para, log_sn, x, y, m, dm, faithful=False)
    assert abs(out["nlZ"] - ex["nlZ"]) <= 1e-14 * abs(ex["nlZ"])
    assert relerr(out["alpha"], ex["alpha"]) <= 3e-10
    assert relerr(out["sW"], ex["sW"]) <= 1e-15
    for k in ("mean", "cov", "lik"):
        assert relerr(out["dnlZ_" + k], ex["dnlZ_" + k]) <= 3e-9, k


@pytest.mark.parametrize("md", [1, 3, 5, 7])
def test_matern_correct_derivative_matches_fd_every_order(md):
    """matern_reference_compat=False is the derivative of K in both hyper-parameters for every d.  d = 7 caught the
    reference's f_7 - f_7' (t / 15 where 3 t / 15 belongs, Core/cov.py:1114), which the oracle and the device had taken
    over.  Measured: <= 3e-10 absolute."""
    g = golden("G4_kernels_seed0")
    x = g["x"]
    hyp = np.array(g["matern%d_hyp" % md])
    for der in (0, 1):
        good = O.der_matrix(O.MATERN, hyp, md, x=x, mode="train", der=der, matern_reference_compat=False)
        h = 1e-6
        hp, hm = hyp.copy(), hyp.copy()
        hp[der] += h
        hm[der] -= h
        fd = (O.cov_matrix(O.MATERN, hp, md, x=x, mode="train") - O.cov_matrix(O.MATERN, hm, md, x=x, mode="train")) / (2 * h)
        assert np.max(np.abs(good - fd)) < 1e-8, (md, der)
