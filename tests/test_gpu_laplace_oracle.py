"""GPU: Laplace inference on the device (csrc/laplace.hip, inf.Laplace) against the CPU oracle (oracle/gp_oracle.py
laplace_fit, pinned to the reference's G20 recordings by tests/test_laplace_oracle.py) where no recording reaches: ragged
sizes and partial 1024-wide panels, every kernel family, means with several hyper-parameters, the Gauss likelihood, saturated
modes, the Newton cap, warm starts, prediction in both forms, pool reuse, K-fold validation and restarts."""
import numpy as np
import pytest

from conftest import synth_cls, synth_reg
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

# The converged posterior, nlZ and gradients are held to the tolerances tests/test_gpu_laplace.py holds the device to against
# the reference: nlZ 1e-8, everything else 1e-6.  The oracle agrees with the reference bit for bit with its LU solves; above
# N = 1024 it takes triangular solves (the same mathematics, faster).
#
# The line-search trace needs a looser rule than the reference comparison's, because the two sides are independent runs of
# Brent's method, not one run seen twice.  Brent stops once the bracket [a, b] around its point is at most 2 tol2 wide, tol2 =
# 2 (sqrt(eps) s + thr / 3) = 6.7e-5 for s <= 2, and a round-off difference of Psi near the flat minimum changes which
# points it visits; so each side's s lies within 1.3e-4 of the minimiser and the two within 2.7e-4 (measured: 1.3e-4).  S_TOL
# applies to steps that lower Psi by more than S_FROM, as in check_steps of tests/test_gpu_laplace.py.  Step k + 1 then starts
# from a state moved by that difference of s along step k's direction, so its Psi may differ by up to S_TOL times step k's
# decrease (measured: 1.1e-4 absolute where that bound is >= 0.1); the first step starts from the same state on both sides,
# its Psi is held to 1e-7, and s is compared only on steps that both sides start with Psi equal to 1e-7.
S_FROM, S_TOL, PSI_TOL = 1e-3, 3e-4, 1e-7
NLZ_TOL, TOL = 1e-8, 1e-6


def rel(got, want):
    want = np.asarray(want, dtype=float).ravel()
    return float(np.max(np.abs(np.asarray(got, dtype=float).ravel() - want)) / max(float(np.max(np.abs(want))), 1e-300))


def build(tree, hyp, D, compat=True):
    """pygps_amd kernel for an oracle `kind` tree with flattened hypers."""
    from pygps_amd import cov
    hyp = [float(h) for h in hyp]
    if tree[0] == "leaf":
        kind, para = tree[1], tree[2]
        k = {O.RBF: lambda: cov.RBF(), O.RQ: lambda: cov.RQ(), O.CONST: lambda: cov.Const(), O.NOISE: lambda: cov.Noise(),
             O.RBFARD: lambda: cov.RBFard(D=D), O.RQARD: lambda: cov.RQard(D=D), O.MATERN: lambda: cov.Matern(d=para)}[kind]()
        k.reference_compat = compat
        assert len(k.hyp) == len(hyp)
        k.hyp = hyp
        return k
    if tree[0] == "scale":
        return build(tree[1], hyp[1:], D, compat) * hyp[0]
    n1 = O.n_cov_hyp(tree[1] if tree[1][0] != "leaf" else tree[1][1], D)
    a, b = build(tree[1], hyp[:n1], D, compat), build(tree[2], hyp[n1:], D, compat)
    return a + b if tree[0] == "sum" else a * b


def leaf(kind, para=0):
    return ("leaf", kind, para)


def means(name, x):
    """(pygps_amd mean, m, dm) -- m and dm written out here, not taken from the mean objects."""
    import pygps_amd as pyGPs
    n, D = x.shape
    w = np.linspace(-0.4, 0.3, D)
    if name == "zero":
        return pyGPs.mean.Zero(), np.zeros((n, 1)), None
    if name == "const":
        return pyGPs.mean.Const(0.2), 0.2 * np.ones((n, 1)), np.ones((n, 1))
    xw = x @ w.reshape(D, 1)
    if name == "linear":
        return pyGPs.mean.Linear(alpha_list=list(w)), xw, x.copy()
    if name == "const+linear":
        return (pyGPs.mean.SumOfMean(pyGPs.mean.Const(-0.3), pyGPs.mean.Linear(alpha_list=list(w))), xw - 0.3,
                np.hstack([np.ones((n, 1)), x]))
    if name == "scale*linear":
        return pyGPs.mean.ScaleOfMean(pyGPs.mean.Linear(alpha_list=list(w)), 0.7), 0.7 * xw, np.hstack([xw, 0.7 * x])
    raise ValueError(name)


def gpc(kernel, mean):
    import pygps_amd as pyGPs
    m = pyGPs.GPC()
    m.useInference("Laplace")
    m.setPrior(mean=mean, kernel=kernel)
    return m


def oracle(tree, hyp, x, y, m, dm, lik="erf", lik_hyp=(), last_alpha=None, compat=True, **kw):
    kind, para = (tree[1], tree[2]) if tree[0] == "leaf" else (tree, 0)
    return O.laplace_fit(kind, np.asarray(hyp, dtype=float), para, x, y, m, dm, lik=lik, lik_hyp=lik_hyp,
                         last_alpha=last_alpha, matern_reference_compat=compat, faithful=x.shape[0] <= 1024, **kw)


def check_steps(inffunc, ref):
    assert inffunc.newton_steps == ref["newton_steps"]
    st, rs = inffunc.last_steps, ref["steps"]
    assert st.shape == rs.shape
    print("steps %d  s %.1e  Psi %.1e" % (rs.shape[0], np.max(np.abs(st[:, 0] - rs[:, 0]), initial=0.0),
                                         np.max(np.abs(st[:, 1] - rs[:, 1]) / np.maximum(np.abs(rs[:, 1]), 1.0), initial=0.0)))
    psi = np.concatenate([[ref["psi0"]], rs[:, 1]])            # psi[k]: Psi before step k
    for k in range(rs.shape[0]):
        same_start = k == 0 or abs(st[k - 1, 1] - rs[k - 1, 1]) <= PSI_TOL * max(abs(rs[k - 1, 1]), 1.0)
        if psi[k] - psi[k + 1] > S_FROM and same_start:
            assert abs(st[k, 0] - rs[k, 0]) <= S_TOL, (k, st[k], rs[k])
        carried = S_TOL * (psi[k - 1] - psi[k]) if k > 0 else 0.0
        assert abs(st[k, 1] - rs[k, 1]) <= PSI_TOL * max(abs(rs[k, 1]), 1.0) + carried, (k, st[k], rs[k])


def check_fit(nlZ, dnlZ, post, ref, nlz_tol=NLZ_TOL, tol=TOL):
    print("nlZ %.1e  alpha %.1e  sW %.1e  diagL %.1e  dnlZ %s" % (
        abs(nlZ - ref["nlZ"]) / max(abs(ref["nlZ"]), 1.0), rel(post.alpha, ref["alpha"]), rel(post.sW, ref["sW"]),
        rel(np.diag(np.asarray(post.L)), np.diag(ref["L"])),
        " ".join("%s %.1e" % (k, rel(getattr(dnlZ, k), ref["dnlZ_" + k])) for k in ("mean", "cov", "lik") if ref["dnlZ_" + k].size)))
    assert abs(nlZ - ref["nlZ"]) <= nlz_tol * max(abs(ref["nlZ"]), 1.0), (nlZ, ref["nlZ"])
    assert rel(post.alpha, ref["alpha"]) <= tol
    assert rel(post.sW, ref["sW"]) <= tol
    assert rel(np.diag(np.asarray(post.L)), np.diag(ref["L"])) <= tol
    scale = max(float(np.max(np.abs(ref["dnlZ_" + k]), initial=0.0)) for k in ("mean", "cov", "lik"))
    for k in ("mean", "cov", "lik"):            # an entry near 0 (a mean already at its optimum) is held to 1 % of the largest
        want = ref["dnlZ_" + k]
        assert len(getattr(dnlZ, k)) == want.size, k
        if want.size:
            err = np.max(np.abs(np.asarray(getattr(dnlZ, k), dtype=float) - want))
            assert err <= tol * max(float(np.max(np.abs(want))), 1e-2 * scale), (k, np.asarray(getattr(dnlZ, k)), want)


def fit_and_check(tree, hyp, x, y, mean="zero", compat=True, nlz_tol=NLZ_TOL, tol=TOL, tol_exp=None):
    D = x.shape[1]
    mo, m, dm = means(mean, x)
    model = gpc(build(tree, hyp, D, compat), mo)
    model.inffunc._tol_exp = tol_exp
    nlZ, dnlZ, post = model.getPosterior(x, y)
    ref = oracle(tree, hyp, x, y, m, dm, compat=compat, tol=10.0 ** -(6 if tol_exp is None else tol_exp))
    check_steps(model.inffunc, ref)
    check_fit(nlZ, dnlZ, post, ref, nlz_tol, tol)
    return model, ref


# ---- a. ragged sizes: N = 1, 2, a 128 boundary either side, partial and whole last 1024-wide panels ----------------------------
@pytest.mark.parametrize("mean", ["zero", "const"])
@pytest.mark.parametrize("N", [1, 2, 7, 127, 129, 1000, 2049, 3000, 4500])
def test_a_ragged_sizes(lib, N, mean):
    x, y = synth_cls(N, 8, seed=1)
    fit_and_check(leaf(O.RBF), [np.log(np.sqrt(8.0)), 0.3], x, y, mean)


# ---- b. kernel families ---------------------------------------------------------------------------------------------------------
def _ard_hyp(d, seed, tail):
    rng = np.random.RandomState(seed)
    return list(np.log(np.sqrt(d)) + 0.3 * rng.randn(d)) + list(tail)


KERNELS = {                                  # tree, hyp, N, d
    "rbfard_d5": (leaf(O.RBFARD), _ard_hyp(5, 1, [0.2]), 900, 5),
    "rbfard_d40_gram": (leaf(O.RBFARD), _ard_hyp(40, 2, [0.1]), 1100, 40),
    "rbfard_d70_gram": (leaf(O.RBFARD), _ard_hyp(70, 3, [0.3]), 800, 70),
    "rq": (leaf(O.RQ), [np.log(2.0), 0.2, -0.3], 1000, 5),
    "rqard": (leaf(O.RQARD), _ard_hyp(5, 4, [0.1, 0.4]), 900, 5),
    "ard_plus_rqard": (("sum", leaf(O.RBFARD), leaf(O.RQARD)), _ard_hyp(4, 5, [0.1]) + _ard_hyp(4, 6, [-0.2, 0.3]), 1000, 4),
    "ard_scaled_prod": (("sum", ("prod", ("scale", leaf(O.RBFARD)), leaf(O.RQ)), leaf(O.CONST)),
                        [0.3] + _ard_hyp(4, 7, [0.0]) + [0.5, 0.1, -0.2, -1.0], 1200, 4),
}


@pytest.mark.parametrize("name", list(KERNELS))
def test_b_kernel_families(lib, name):
    tree, hyp, N, d = KERNELS[name]
    x, y = synth_cls(N, d, seed=2)
    model, _ = fit_and_check(tree, hyp, x, y, "zero", compat=False)
    if tree[0] != "leaf":
        assert model.covfunc._on_device()


@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("md", [1, 3, 5, 7])
def test_b_matern(lib, md, compat):
    x, y = synth_cls(1000, 6, seed=3)
    fit_and_check(leaf(O.MATERN, md), [np.log(2.0), 0.2], x, y, "zero", compat=compat)


def test_b_tree_that_is_no_device_program_through_the_panels(lib):
    """Three ARD leaves: K and the derivative matrices come from the host, the Newton loop runs on the dense path at N > 1024."""
    ard = leaf(O.RBFARD)
    tree = ("sum", ("prod", ard, ard), ard)
    hyp = _ard_hyp(3, 8, [0.3]) + _ard_hyp(3, 9, [0.0]) + _ard_hyp(3, 10, [-0.4])
    x, y = synth_cls(1300, 3, seed=4)
    model, _ = fit_and_check(tree, hyp, x, y, "zero")
    assert model.covfunc._on_device() is False


# ---- c. means with several hyper-parameters (the dm[i * n + j] loop) ---------------------------------------------------------------
@pytest.mark.parametrize("mean", ["linear", "const+linear", "scale*linear"])
def test_c_means(lib, mean):
    x, y = synth_cls(1000, 5, seed=5)
    fit_and_check(leaf(O.RBF), [np.log(2.0), 0.4], x, y, mean)


# ---- d. Gauss likelihood: GPR + Laplace against the oracle, against the device's exact fit, prediction on both posteriors ---------
@pytest.mark.parametrize("log_sn", [-3.0, 0.0, 1.5])
def test_d_gauss(lib, log_sn):
    import pygps_amd as pyGPs
    N, d = 1029, 5
    x, y = synth_reg(N, d, seed=6)
    hyp = [np.log(2.0), 0.1]

    def model(laplace):
        m = pyGPs.GPR()
        m.setPrior(mean=pyGPs.mean.Const(0.1), kernel=pyGPs.cov.RBF(*hyp))
        m.setNoise(log_sn)
        if laplace:
            m.useInference("Laplace")
        return m
    mL = model(True)
    nlZ, dnlZ, post = mL.getPosterior(x, y)
    ref = oracle(leaf(O.RBF), hyp, x, y, 0.1 * np.ones((N, 1)), np.ones((N, 1)), lik="gauss", lik_hyp=[log_sn])
    check_steps(mL.inffunc, ref)
    check_fit(nlZ, dnlZ, post, ref)
    mL.inffunc._tol_exp = 12
    nlZ, dnlZ, post = mL.getPosterior(x, y)
    mE = model(False)
    nE, dE, pE = mE.getPosterior(x, y)
    assert abs(nlZ - nE) <= 1e-10 * abs(nE)
    assert rel(post.alpha, pE.alpha) <= 1e-6 and rel(post.sW, pE.sW) <= 1e-12
    for k in ("mean", "cov", "lik"):
        assert rel(getattr(dnlZ, k), getattr(dE, k)) <= 1e-6, k
    xs = np.random.RandomState(7).randn(300, d)
    a, b = mL.predict(xs), mE.predict(xs)
    for u, v in zip(a[:4], b[:4]):
        assert np.max(np.abs(u - v)) <= 1e-6 * max(1.0, float(np.max(np.abs(v))))


# ---- e. saturated modes: |f| >> 6, where the log Phi / ratio blends and the d3lp cancellation matter ------------------------------
@pytest.mark.parametrize("labels,log_sigma,tol_exp", [("flipped", 3.0, None), ("one_class", 4.0, 10)])
def test_e_saturation(lib, labels, log_sigma, tol_exp):
    """10 % of the labels flipped at log_sigma = 3 (measured max |f| 8.9); one class, where the mode stays near 6 unless the
    prior is wide, at log_sigma = 4 (6.6).  There Psi is nearly flat (0.02), so both sides converge to 1e-10: at the
    reference's 1e-6 the oracle's own two solve flavours end 2e-8 apart in nlZ.  The line search fixes the mode only to its
    fractional precision along a nearly flat Psi, so the one-class case is held to nlZ 1e-7 (measured 1.2e-8) and 1e-5."""
    N, d = 600, 4
    x, y = synth_cls(N, d, seed=8)
    if labels == "flipped":
        y[np.random.RandomState(9).permutation(N)[:N // 10]] *= -1
    else:
        y = np.ones_like(y)
    loose = dict(nlz_tol=1e-7, tol=1e-5) if labels == "one_class" else {}
    model, ref = fit_and_check(leaf(O.RBF), [np.log(2.0), log_sigma], x, y, "zero", tol_exp=tol_exp, **loose)
    assert np.max(np.abs(ref["f"])) > 6.0
    assert np.all(np.asarray(model.posterior.sW) > 0)          # no W < 0 (the device raises on it)


# ---- f. the Newton cap -----------------------------------------------------------------------------------------------------------
def test_f_newton_cap(lib):
    """log_sigma = 10 with mixed labels: Psi still falls by ~0.2 per step at the 20th, so both sides stop at LAP_MAXIT.  The
    trajectory there is ill-conditioned (the oracle's LU and triangular solves end 1e-3 apart), so beyond the first step the
    device's own end point is checked: the oracle evaluates the posterior, nlZ and the gradients at the device's alpha."""
    N = 300
    x, y = synth_cls(N, 3, seed=3)
    hyp = [np.log(2.0), 10.0]
    ref = oracle(leaf(O.RBF), hyp, x, y, np.zeros((N, 1)), None, nargout=2)
    assert ref["newton_steps"] == 20 and ref["steps"][-1, 1] < ref["steps"][-2, 1] - 1e-3
    model = gpc(build(leaf(O.RBF), hyp, 3), means("zero", x)[0])
    nlZ, dnlZ, post = model.getPosterior(x, y)
    assert model.inffunc.newton_steps == 20 and model.inffunc.last_steps.shape == (20, 3)
    st = model.inffunc.last_steps
    # sf2 = e^20: f = K alpha carries terms of ~5e8, so Psi itself is evaluated to ~1e-5 relative at best (measured 1.0e-5)
    assert abs(st[0, 0] - ref["steps"][0, 0]) <= S_TOL and abs(st[0, 1] - ref["steps"][0, 1]) <= 1e-4 * abs(ref["steps"][0, 1])
    assert np.all(np.diff(st[:, 1]) < 0)
    # nlZ, sW and L at the device's alpha.  The gradients are not compared here: with K ~ 5e8 their explicit and implicit parts
    # cancel to ~1e-2 relative in either arrangement (the oracle and the device's R = Z - u dlp' - dlp u' disagree by 1.6e-2)
    at = oracle(leaf(O.RBF), hyp, x, y, np.zeros((N, 1)), None, last_alpha=np.asarray(post.alpha), keep_warm=True, maxit=0)
    assert abs(nlZ - at["nlZ"]) <= 1e-6 * abs(at["nlZ"])                     # measured 1.3e-8
    assert rel(post.sW, at["sW"]) <= 1e-5                                    # 6.8e-7
    assert rel(np.diag(np.asarray(post.L)), np.diag(at["L"])) <= 1e-5        # 1.6e-7
    assert np.all(np.isfinite(dnlZ.cov))


# ---- g. warm starts at N = 2049 -----------------------------------------------------------------------------------------------
def test_g_warm_start_sent_cold_by_psi_def(lib):
    """GPC, Zero mean: Psi_def = -log Phi(0) = log 2 is below any Psi of a last alpha, so the second call starts cold -- and equals
    a fresh model's fit bit for bit."""
    N, d = 2049, 6
    x, y = synth_cls(N, d, seed=10)
    h1, h2 = [np.log(np.sqrt(d)), 0.0], [np.log(np.sqrt(d)) + 0.2, 0.3]
    model = gpc(build(leaf(O.RBF), h1, d), means("zero", x)[0])
    model.getPosterior(x, y)
    a1 = np.asarray(model.inffunc.last_alpha).copy()
    model.covfunc.hyp = list(h2)
    nlZ, dnlZ, post = model.getPosterior(x, y)
    ref = oracle(leaf(O.RBF), h2, x, y, np.zeros((N, 1)), None, last_alpha=a1)
    check_steps(model.inffunc, ref)
    check_fit(nlZ, dnlZ, post, ref)
    fresh = gpc(build(leaf(O.RBF), h2, d), means("zero", x)[0])
    nF, dF, pF = fresh.getPosterior(x, y)
    assert nF == nlZ and np.array_equal(np.asarray(pF.alpha), np.asarray(post.alpha))


def test_g_warm_start_kept(lib):
    """GPR + Laplace at log_sn = -3: Psi_def = y_1^2 / (2 sn2) + log(2 pi sn2) / 2 lies far above the Psi of the last alpha, so the
    warm start is kept; refitting at the same hyper-parameters then takes one Newton step where a cold start takes two."""
    import pygps_amd as pyGPs
    N, d = 2049, 6
    x, y = synth_reg(N, d, seed=11)
    y = y + 1.0
    hyp, log_sn = [np.log(np.sqrt(d)), 0.0], -3.0
    m = pyGPs.GPR()
    m.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(*hyp))
    m.setNoise(log_sn)
    m.useInference("Laplace")
    m.getPosterior(x, y)
    a1 = np.asarray(m.inffunc.last_alpha).copy()
    nlZ, dnlZ, post = m.getPosterior(x, y)
    z = np.zeros((N, 1))
    ref = oracle(leaf(O.RBF), hyp, x, y, z, None, lik="gauss", lik_hyp=[log_sn], last_alpha=a1)
    cold = oracle(leaf(O.RBF), hyp, x, y, z, None, lik="gauss", lik_hyp=[log_sn], nargout=2)
    assert ref["newton_steps"] < cold["newton_steps"]
    check_steps(m.inffunc, ref)
    check_fit(nlZ, dnlZ, post, ref)


# ---- h. prediction on a Laplace posterior: blocked solve, product form, blocked again ------------------------------------------
def test_h_predict(lib):
    from pygps_amd import _lib
    N, d = 1100, 5
    x, y = synth_cls(N, d, seed=12)
    hyp = [np.log(2.0), 0.5]
    model, ref = fit_and_check(leaf(O.RBF), hyp, x, y, "const")
    rng = np.random.RandomState(13)
    xs_all = rng.randn(2500, d)
    xs_all[:200] = x[rng.randint(0, N, 200)] + 1e-3 * rng.randn(200, d)
    ys_all = np.sign(rng.randn(2500, 1))
    got = {}
    for ns in (1, 127, 1023, 2500, 127):
        xs, ys = xs_all[:ns], ys_all[:ns]
        ym, ys2, fm, fs2, lp = model.predict(xs, ys=ys)
        rym, rys2, rfm, rfs2 = O.predict(O.RBF, np.array(hyp), 0, None, x, ref["alpha"], ref["L"], ref["sW"], xs,
                                         0.2 * np.ones((ns, 1)), gauss=False, faithful=False)
        rlp = O.erf_ep_moments(ys, rfm, rfs2, 1)[0]
        p = np.exp(rlp)                  # with ys, ym and ys2 are the moments of the label ys (Core/lik.py Erf, prediction mode)
        rym, rys2 = 2 * p - 1, 4 * p * (1 - p)
        for u, v, k in ((fm, rfm, "fm"), (fs2, rfs2, "fs2"), (ym, rym, "ym"), (ys2, rys2, "ys2"), (lp, rlp, "lp")):
            assert np.max(np.abs(u - v)) <= 1e-6 * max(1.0, float(np.max(np.abs(v)))), (ns, k)
        got[ns] = [np.array(v) for v in (ym, ys2, fm, fs2)]
    ctx = _lib.ctx()
    try:
        _lib.check(lib.pgp_set_option(ctx, b"predict_inverse", 0))          # the blocked solve for all 2500 points
        blocked = [np.array(v) for v in model.predict(xs_all, ys=ys_all)[:4]]
    finally:
        lib.pgp_set_option(ctx, b"predict_inverse", 1)
    for u, v, tol in zip(blocked, got[2500], (1e-11, 1e-9, 1e-11, 1e-9)):   # test_predict_product_form_equals_the_blocked_solve
        assert np.max(np.abs(u - v)) <= tol * max(1.0, float(np.max(np.abs(u))))


# ---- i. pool reuse: Laplace, exact and EP fits of other sizes in one process ---------------------------------------------------
def test_i_pool_reuse_is_bit_identical(lib):
    import pygps_amd as pyGPs

    def lap(N):
        x, y = synth_cls(N, 8, seed=14)
        model = gpc(build(leaf(O.RBF), [np.log(np.sqrt(8.0)), 0.3], 8), pyGPs.mean.Const(0.1))
        nlZ, dnlZ, post = model.getPosterior(x, y)
        return nlZ, np.array(post.alpha), np.array(post.sW), np.array(dnlZ.mean + dnlZ.cov), np.diag(np.asarray(post.L)).copy()
    first = lap(2049)
    lap(129)
    lap(4500)
    xr, yr = synth_reg(700, 5, seed=15)
    e = pyGPs.GPR()
    e.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(0.5, 0.0))
    e.setNoise(np.log(0.1))
    e.getPosterior(xr, yr)
    xc, yc = synth_cls(1500, 5, seed=16)
    ep = pyGPs.GPC()
    ep.setPrior(mean=pyGPs.mean.Zero(), kernel=pyGPs.cov.RBF(0.5, 0.0))
    ep.getPosterior(xc, yc)
    again = lap(2049)
    assert first[0] == again[0]
    for u, v in zip(first[1:], again[1:]):
        assert np.array_equal(u, v)


# ---- j. K-fold validation and restarts on a Laplace model --------------------------------------------------------------------
def test_j_kfold_equals_fresh_fits(lib):
    import pygps_amd as pyGPs
    from pygps_amd import valid
    N, d, K = 600, 4, 4
    x, y = synth_cls(N, d, seed=17)

    def make():
        return gpc(pyGPs.cov.RBF(np.log(2.0), 0.3), pyGPs.mean.Zero())
    res = valid.sharded_k_fold(make, x, y, K=K, metrics=("ACC",))
    idx = np.arange(N)
    for k in range(K):
        te = idx % K == k
        m = make()
        m.setData(x[~te], y[~te])
        nlZ = m.getPosterior()[0]
        ym = m.predict(x[te], ys=y[te])[0]
        assert abs(res["nlZ"][k] - nlZ) <= 1e-12 * abs(nlZ)
        assert res["ACC"][k] == valid.ACC(np.sign(ym), y[te])


def test_j_restarts_equal_cold_single_fits(lib):
    import pygps_amd as pyGPs
    N, d = 400, 4
    x, y = synth_cls(N, d, seed=18)

    def make():
        m = gpc(pyGPs.cov.RBF(np.log(2.0), 0.3), pyGPs.mean.Zero())
        m.setData(x, y)
        return m
    m = make()
    m.setOptimizer("ShardedMinimize", num_restarts=3)
    np.random.seed(19)
    m.optimize(x, y, numIterations=3)
    o = m.optimizer
    assert len(o.runs) >= 2
    for t, run in enumerate(o.runs):
        single = make()
        single.setOptimizer("Minimize")
        r = single.optimizer._one(o.init_table[t].copy(), 3)
        assert run.ok == r.ok
        if r.ok:
            assert abs(run.f - r.f) <= 1e-10 * abs(r.f) and rel(run.hyp, r.hyp) <= 1e-10
