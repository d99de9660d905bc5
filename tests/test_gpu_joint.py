"""GPU: GP.predict_joint, GP.sample_posterior and GP.sample_prior (csrc/joint.hip) against the long-double reference of
tests/joint_ref_ld.py, at the shapes where the code takes another path: ns across the 128 edges (1, 127, 129, 300, 1153: ns < n,
ns > n, two slab widths), np = 256 / 384 (the blocked solve) and np = 1152 (the product form), both GEMM tile sizes.

The reference predicts from the posterior the device itself reports (post.alpha, post.sW, post.L), as test_gpu_predict_ld.py does.
Every fcov assertion is `worst <= 1`, worst = max_ij |device - reference|_ij / tol_ij with the tolerance of joint_ref_ld (kernel bar
to first order + 8 x the measured error of two fp64 CPU evaluations + 4 ulps of sqrt(kss_i kss_j)); tests/test_joint_host.py shows
on the CPU that it rejects every single-slip mutant by >= 10 x.  The factor is held to 8 x the componentwise backward error of
numpy's own Cholesky of the same matrix, the draws to the order-independent dot-product bound gamma_(ns+1) |Lc| |z| + 2 u |ref|.

Measured on the MI355X on 2026-10-20: worst ratio per case (1 = the tolerance; "blocked / product" = predict_inverse 0 / 2).

    1  fcov against long double                                   fmu                  fcov
       GPR + RBF n = 130   ns = 1 / 127 / 129 / 300               0.0004 ... 0.0051    0.00004 ... 0.0043
       GPR + RBF n = 300   ns = 1 / 127 / 129 / 300               0.0008 ... 0.0053    0.0010 ... 0.0030
       GPR + RBF n = 1100  ns = 1 / 127 / 129 / 300, blocked      0.0005 ... 0.0025    0.0005 ... 0.0009
                                                     product      0.0023 ... 0.0032    0.0019 ... 0.0036
       GPR + RBF n = 1100  ns = 1153            blocked / product 0.0026 / 0.0035      0.0021 / 0.0038
       GPR + RBFard d = 17, n = 300, ns = 129                     0.0017               0.0039
       RBF + Periodic * RBF, 1-d, n = 300, ns = 129               0.0027               0.0016
       Linear + RBF n = 1100, ns = 300 (blocked solve)            0.0042               0.0050
       GPC + EP, Matern 3, n = 300 (sites with sW = 0)            0.064                0.064
       GPC + Laplace, RBFard d = 17, n = 300                      0.0013               0.0028
       GPR + lik.Laplace + EP, n = 300                            0.0036               0.0042
       three RBFard (the dense route), n = 300                    0.0027               0.0027
       RBF + Noise, n = 300                                       0.0036               0.0027
       n = 1100, ns = 300 with 128-tiles / 64-tiles               the same figures as above in both forms
    3  Cholesky, r = max |Lc Lc' - A| / (|Lc| |Lc|'):             device      numpy       device / numpy  (bound: 8)
       noise = True   ns = 129                                    1.2e-15     3.9e-16     3.2
       noise = True   ns = 300                                    2.4e-15     7.7e-16     3.1
       noise = True   ns = 1153                                   6.1e-15     1.2e-15     5.0
       latent, default jitter, ns = 300 (64- and 128-tiles)       1.93e-15    1.77e-15    1.09
       prior RBF / Linear + RBF   ns = 129                        1.3e-15     1.2e-15     1.04 / 1.04
       prior RBF / Linear + RBF   ns = 300                        2.0e-15 / 1.6e-15       0.91 / 0.64
    4  draws, share of the dot-product bound: 0.17 (129, 1), 0.14 (300, 5), 0.27 (1153, 130); priors 0.15 ... 0.30

The factor is the Cholesky sweep's after one Newton step (joint.hip joint_refine).  Without it (option joint_refine 0) the latent
case at ns = 300 has r = 2.05e-14, 11.6 x numpy's and above the bound: the sweep's panel solves multiply by explicit inverses of
16 x 16 pivot blocks, and the same arithmetic in numpy on the same matrix gives 16 x.  At ns = 1920 (rbf1100, latent, measured
once, not a test: its long-double residual takes a minute): 3.1e-13 without the step, 4.1e-15 with it, numpy 4.5e-15.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import joint_ref_ld as J
import predict_ref_ld as P
from pool_state import pool_state as _pool_state

pytestmark = pytest.mark.gpu

DEFAULTS = dict(predict_inverse=1, keep_inverse=1, small_tile_below=200)
_FIT = {}


class _options(object):
    def __init__(self, lib, **kw):
        self.lib, self.kw = lib, kw

    def __enter__(self):
        from pygps_amd import _lib
        for k, v in self.kw.items():
            _lib.check(self.lib.pgp_set_option(_lib.ctx(), k.encode(), int(v)))

    def __exit__(self, *exc):
        from pygps_amd import _lib
        for k in self.kw:
            self.lib.pgp_set_option(_lib.ctx(), k.encode(), DEFAULTS[k])
        return False


def _model(name):
    """The fitted model of joint_ref_ld.MODELS[name] (one fit per name), its spec and its pool of test points."""
    if name not in _FIT:
        _FIT[name] = _build(name)
    return _FIT[name]


def _build(name):
    """A fresh fit of joint_ref_ld.MODELS[name]: (model, spec, pool of test points, prior mean there)."""
    import pygps_amd as pyGPs
    cov = pyGPs.cov
    kind, spec, hyp, d, n, nmax, seed = J.MODELS[name]
    x, y, xs, ms, _ = J.model_data(name)
    m = {"gpr": pyGPs.GPR, "gpr_liklaplace": pyGPs.GPR, "gpc_ep": pyGPs.GPC, "gpc_laplace": pyGPs.GPC}[kind]()
    if kind == "gpc_laplace":
        m.useInference("Laplace")
    if kind == "gpr_liklaplace":
        m.useLikelihood("Laplace")
    if name in ("rbf130", "rbf300", "rbf1100"):
        k = cov.RBF(hyp[0], hyp[1])
    elif name in ("rbfard17", "lap300"):
        k = cov.RBFard(log_ell_list=list(hyp[:17]), log_sigma=hyp[17])
    elif name == "sum_per":
        k = cov.RBF(hyp[0], hyp[1]) + cov.Periodic(hyp[2], hyp[3], hyp[4]) * cov.RBF(hyp[5], hyp[6])
    elif name == "lin_rbf1100":
        k = cov.Linear(hyp[0]) + cov.RBF(hyp[1], hyp[2])
    elif name == "ep300":
        k = cov.Matern(hyp[0], 3, hyp[1])
    elif name == "liklap300":
        k = cov.RBF(hyp[0], hyp[1])
    elif name == "rbf_noise300":
        k = cov.RBF(hyp[0], hyp[1]) + cov.Noise(hyp[2])
    else:
        assert name == "dense300"
        h = hyp
        k = (cov.RBFard(log_ell_list=h[0:3], log_sigma=h[3]) + cov.RBFard(log_ell_list=h[4:7], log_sigma=h[7])) \
            + cov.RBFard(log_ell_list=h[8:11], log_sigma=h[11])
    mean = pyGPs.mean.Const(P.MEAN_C)
    if kind == "gpc_ep":
        mean = mean + pyGPs.mean.Linear(alpha_list=list(P.MEAN_W_ISLAND))
    m.setPrior(mean=mean, kernel=k)
    if kind == "gpr":
        m.setNoise(float(np.log(P.SN)))
    if kind == "gpr_liklaplace":
        m.likfunc.hyp = [J.LIK_LAPLACE_LOG_SN]
    m.setData(x, y)
    m.getPosterior()
    assert np.allclose(np.asarray(m.meanfunc.getMean(xs)).ravel(), ms)
    assert [float(v) for v in m.covfunc.hyp] == [float(v) for v in hyp], name
    return m, spec, xs, ms


def _ref(name):
    m, spec, xs, ms = _model(name)
    post = m.posterior
    return J.cached(spec, np.array(m.covfunc.hyp, dtype=float), m.x, xs, ms, post.alpha, post.sW, np.asarray(post.L))


def _case(name, ns):
    m, spec, xs, ms = _model(name)
    idx = P.select(J.MODELS[name][5], ns)
    return m, xs[idx], idx


def _check_fcov(tag, fmu, fcov, ref):
    r = J.ratios(fmu, fcov, ref)
    worst, where = J.check_joint(fmu, fcov, ref)
    print("joint %-44s worst %.3g at %s   fmu %.3g  fcov %.3g" % (tag, worst, where, r["fmu"][0], r["fcov"][0]))
    assert worst <= 1.0, (tag, worst, where)
    assert np.array_equal(fcov, fcov.T), tag
    return worst


def _vpad(lib, m, xs):
    """Through the test hook: which form V took, and that its padding rows and columns are exact zeros."""
    L = m.posterior.L
    form, nz = C.c_int(), (C.c_int64 * 3)()
    xs = np.ascontiguousarray(xs, dtype=np.float64)
    rc = lib.pgp_test_joint_vpad(L.ctx, L.handle, xs.ctypes.data_as(C.POINTER(C.c_double)), xs.shape[0], C.byref(form), nz)
    assert rc == 0, rc
    assert nz[0] == 0 and nz[1] == 0 and nz[2] > 0, list(nz)
    return form.value


# ---- 1: fcov against long double ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ns", J.FCOV_CASES)
def test_fcov_against_long_double(lib, name, ns):
    m, xs, idx = _case(name, ns)
    ref = _ref(name).take(idx)
    n = m.x.shape[0]
    dense = bool(getattr(m.posterior.L, "dense", False))
    assert dense == (name == "dense300")
    modes = (0, 2) if n == 1100 and name != "lin_rbf1100" else (1,)
    for mode in modes:
        with _options(lib, predict_inverse=mode):
            fmu, fcov = m.predict_joint(xs)
            if not dense:
                form = _vpad(lib, m, xs)
                assert form == (1 if mode == 2 else 0), (name, mode, form)     # np < 1024 and dot leaves: the blocked solve
        _check_fcov("%s ns=%d mode=%d" % (name, ns, mode), fmu.ravel(), fcov, ref)


@pytest.mark.parametrize("tile_below", [1, 1000000], ids=["tile128", "tile64"])
def test_fcov_with_both_tile_sizes(lib, tile_below):
    m, xs, idx = _case("rbf1100", 300)
    ref = _ref("rbf1100").take(idx)
    for mode in (0, 2):
        with _options(lib, predict_inverse=mode, small_tile_below=tile_below):
            fmu, fcov = m.predict_joint(xs)
        _check_fcov("rbf1100 ns=300 mode=%d small_tile_below=%d" % (mode, tile_below), fmu.ravel(), fcov, ref)


# ---- 2: consistency with predict ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ns", [("rbf130", 1), ("rbf130", 129), ("rbf300", 300), ("ep300", 129), ("lap300", 129),
                                     ("liklap300", 129), ("sum_per", 129), ("dense300", 129)])
def test_mean_and_diagonal_are_predicts_bits_below_1024(lib, name, ns):
    m, xs, idx = _case(name, ns)
    fmu, fcov = m.predict_joint(xs)
    out = m.predict(xs)
    assert np.array_equal(fmu, np.asarray(out[2])), name
    assert np.array_equal(fcov.diagonal(), np.asarray(out[3]).ravel()), name
    assert np.array_equal(fcov, fcov.T)


@pytest.mark.parametrize("name", ["rbf1100", "lin_rbf1100"])
def test_mean_and_diagonal_agree_with_predict_at_1100(lib, name):
    m, xs, idx = _case(name, 300)
    ref = _ref(name).take(idx)
    fmu, fcov = m.predict_joint(xs)
    out = m.predict(xs)
    t_mu, t_s2 = ref.pref.tol()
    assert np.all(np.abs(fmu.ravel() - np.asarray(out[2]).ravel()) <= 2 * t_mu)
    assert np.all(np.abs(fcov.diagonal() - np.asarray(out[3]).ravel()) <= t_s2 + ref.tol().diagonal())
    assert np.array_equal(fcov, fcov.T)


def test_noise_adds_sn2_on_the_diagonal_only(lib):
    m, xs, idx = _case("rbf300", 300)
    f0, c0 = m.predict_joint(xs)
    f1, c1 = m.predict_joint(xs, noise=True)
    sn2 = float(np.exp(2.0 * m.likfunc.hyp[0]))
    assert np.array_equal(f0, f1)
    off = ~np.eye(300, dtype=bool)
    assert np.array_equal(c0[off], c1[off])
    d = c1.diagonal() - c0.diagonal()
    assert np.all(np.abs(d - sn2) <= np.spacing(c1.diagonal())), float(np.max(np.abs(d - sn2)))


# ---- 3, 4: the factor and the draws ------------------------------------------------------------------------------------------------
def _chol_check(tag, Lc, A):
    assert np.array_equal(Lc, np.tril(Lc)), tag                          # exact zeros above the diagonal
    r_dev = J.chol_residual(Lc, A)
    r_cpu = J.chol_residual(np.linalg.cholesky(A), A)
    print("joint %-44s chol residual: device %.3g  numpy %.3g  (ratio %.3g)" % (tag, r_dev, r_cpu, r_dev / r_cpu))
    assert r_dev <= J.SOLVE_FACTOR * r_cpu, (tag, r_dev, r_cpu)


@pytest.mark.parametrize("name,ns,noise", J.CHOL_CASES)
def test_cholesky_against_numpys(lib, name, ns, noise):
    """r_dev <= 8 r_cpu.  Measured on the MI355X, 2026-10-20: r_dev / r_cpu = 3.2 (ns = 129), 3.1 (300), 5.0 (1153) with noise,
    1.09 on the latent case with the default jitter at ns = 300 (11.6 before the factor's Newton step was added)."""
    m, xs = _model(name)[0], J.chol_points(name, ns)
    fmu, fcov = m.predict_joint(xs)
    z = np.random.default_rng(ns).standard_normal((ns, 1))
    F, Lc, fmu2, jitter = m.sample_posterior(xs, z=z, noise=noise, return_chol=True)
    assert np.array_equal(fmu, fmu2)
    add = (float(np.exp(2.0 * m.likfunc.hyp[0])) if noise else 0.0) + jitter
    assert (jitter == 0.0) == noise
    A = fcov.copy()
    A[np.diag_indices(ns)] += add
    _chol_check("%s ns=%d noise=%s" % (name, ns, noise), Lc, A)


@pytest.mark.parametrize("tile_below", [1, 1000000], ids=["tile128", "tile64"])
def test_cholesky_with_both_tile_sizes_and_without_the_refinement(lib, tile_below):
    """The factor's Newton step (joint.hip joint_refine) on 128- and on 64-tiles, latent with the default jitter at ns = 300; with
    joint_refine = 0 the sweep's own factor comes back: a valid factor (the draws' bound holds), without the 8 x bound."""
    from pygps_amd import _lib
    m, xs = _model("rbf300")[0], J.chol_points("rbf300", 300)
    fmu, fcov = m.predict_joint(xs)
    z = np.random.default_rng(1).standard_normal((300, 2))
    with _options(lib, small_tile_below=tile_below):
        F, Lc, _, jitter = m.sample_posterior(xs, z=z, return_chol=True)
        try:
            _lib.check(lib.pgp_set_option(_lib.ctx(), b"joint_refine", 0))
            F0, L0, _, _ = m.sample_posterior(xs, z=z, return_chol=True)
        finally:
            lib.pgp_set_option(_lib.ctx(), b"joint_refine", 1)
    A = fcov.copy()
    A[np.diag_indices(300)] += jitter
    _chol_check("rbf300 ns=300 latent small_tile_below=%d" % tile_below, Lc, A)
    r0 = J.chol_residual(L0, A)
    print("joint without the refinement: chol residual %.3g" % r0)
    assert np.array_equal(L0, np.tril(L0)) and np.all(np.isfinite(L0))
    assert J.draws_excess(F, fmu.ravel(), Lc, z) <= 1.0 and J.draws_excess(F0, fmu.ravel(), L0, z) <= 1.0


@pytest.mark.parametrize("name,ns,nsamp", J.DRAW_CASES)
def test_draws_against_long_double(lib, name, ns, nsamp):
    m, xs = _model(name)[0], J.chol_points(name, ns)
    z = np.random.default_rng(5).standard_normal((ns, nsamp))
    F, Lc, fmu, jitter = m.sample_posterior(xs, z=z, noise=True, return_chol=True)
    assert F.shape == (ns, nsamp)
    ex = J.draws_excess(F, fmu.ravel(), Lc, z)
    print("joint draws %s ns=%d nsamp=%d: %.3g of the bound" % (name, ns, nsamp, ex))
    assert ex <= 1.0, ex
    assert np.array_equal(m.sample_posterior(xs, z=z, noise=True), F)                                   # the same z: the same bits
    assert np.array_equal(m.sample_posterior(xs, nsamples=nsamp, rng=np.random.default_rng(5), noise=True), F)
    assert np.array_equal(m.sample_posterior(xs, nsamples=nsamp, rng=5, noise=True), F)


# ---- 5: sample_prior -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["rbf", "lin_rbf"])
@pytest.mark.parametrize("ns", [129, 300])
def test_sample_prior(lib, kernel, ns):
    import pygps_amd as pyGPs
    cov = pyGPs.cov
    m = pyGPs.GPR()
    k = cov.RBF(J.LOG_ELL3, 0.0) if kernel == "rbf" else cov.Linear(J.LIN_RBF_HYP[0]) + cov.RBF(J.LIN_RBF_HYP[1], J.LIN_RBF_HYP[2])
    m.setPrior(mean=pyGPs.mean.Const(P.MEAN_C), kernel=k)
    xs = np.random.RandomState(ns).randn(ns, 3)
    z = np.random.default_rng(7).standard_normal((ns, 5))
    F, Lc, mu, jitter = m.sample_prior(xs, z=z, return_chol=True)
    K = np.asarray(m.covfunc.getCovMatrix(x=xs, mode="train"), dtype=float)
    assert jitter == 1e-8 * float(np.mean(K.diagonal())) and np.all(mu == P.MEAN_C)
    _chol_check("prior %s ns=%d" % (kernel, ns), Lc, K + jitter * np.eye(ns))
    ex = J.draws_excess(F, mu.ravel(), Lc, z)
    print("joint prior draws %s ns=%d: %.3g of the bound" % (kernel, ns, ex))
    assert ex <= 1.0, ex
    assert np.array_equal(m.sample_prior(xs, z=z), F)


# ---- 6: refusals and statuses ----------------------------------------------------------------------------------------------------
def test_refusals(lib):
    import pygps_amd as pyGPs
    m, xs, idx = _case("rbf300", 129)
    # a sharded posterior stand-in (world 1): what GP.predict recognises by its type name
    post = copy.copy(m.posterior)
    post.L = type("DistributedFactor", (), {})()
    m2 = copy.copy(m)
    m2.posterior = post
    with pytest.raises(NotImplementedError, match="sharded"):
        m2.predict_joint(xs)
    with pytest.raises(NotImplementedError, match="sharded"):
        m2.sample_posterior(xs)
    # FITC
    x, y = P.reg_data(200, 3, 5)
    f = pyGPs.GPR_FITC()
    f.setData(x, y)
    f.setPrior(kernel=pyGPs.cov.RBF(J.LOG_ELL3, 0.0), inducing_points=x[:32].copy())
    f.getPosterior()
    with pytest.raises(NotImplementedError, match="FITC"):
        f.predict_joint(xs)
    # cov.Pre
    K2 = np.exp(-0.5 * ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)) + 1e-6 * np.eye(200)
    K1 = np.vstack([K2[:, :5], np.ones((1, 5))])
    p = pyGPs.GPR()
    p.setPrior(kernel=pyGPs.cov.Pre(K1, K2))
    p.setData(x, y)
    p.getPosterior()
    with pytest.raises(NotImplementedError, match="Pre"):
        p.predict_joint(np.arange(5.0).reshape(5, 1))
    # noise on a classifier
    c, cxs, _ = _case("ep300", 129)
    with pytest.raises(Exception, match="lik.Gauss"):
        c.predict_joint(cxs, noise=True)
    with pytest.raises(Exception, match="lik.Gauss"):
        c.sample_posterior(cxs, noise=True)
    # too many points: refused before anything is allocated
    before = _pool_state(lib)
    with pytest.raises(Exception, match="16384"):
        m.predict_joint(np.zeros((16385, 3)))
    assert _pool_state(lib) == before
    from pygps_amd import _lib
    L = m.posterior.L
    big = np.zeros((16385, 3))
    fmu = np.zeros(16385)
    assert lib.pgp_predict_joint(L.ctx, L.handle, _lib.ptr(big), 16385, None, 0.0, 0.0, None, 0, _lib.ptr(fmu), None, None, None,
                                 None) == -4
    assert lib.pgp_predict_joint(L.ctx, L.handle, _lib.ptr(big), 5, None, 0.0, 0.0, None, 0, _lib.ptr(fmu), None, None, _lib.ptr(fmu),
                                 None) == -8
    assert _pool_state(lib) == before


def test_rank_deficient_covariance_names_its_pivot_and_the_context_goes_on(lib):
    """300 points on a line under an RBF with a long length scale: the latent covariance has a handful of eigenvalues above
    rounding, so with jitter = 0 some pivot of the factorisation is not positive -- a numerical condition, reported as a status."""
    import pygps_amd as pyGPs
    x, y = P.reg_data(130, 3, 9)
    m = pyGPs.GPR()
    m.setPrior(mean=pyGPs.mean.Const(P.MEAN_C), kernel=pyGPs.cov.RBF(3.0, 0.0))
    m.setNoise(float(np.log(P.SN)))
    m.setData(x, y)
    m.getPosterior()
    t = np.linspace(-1.0, 1.0, 300).reshape(300, 1)
    xs = t * np.array([[1.0, 0.5, -0.25]])
    with pytest.raises(np.linalg.LinAlgError) as e:
        m.sample_posterior(xs, nsamples=2, rng=1, jitter=0.0)
    pivot = int(str(e.value).split("pivot")[1].split(";")[0])
    assert 1 <= pivot <= 300, str(e.value)
    F = m.sample_posterior(xs, nsamples=2, rng=1, noise=True)            # the next call on the same context succeeds
    assert F.shape == (300, 2) and np.all(np.isfinite(F))
    fmu, fcov = m.predict_joint(xs)
    assert np.array_equal(np.asarray(m.predict(xs)[3]).ravel(), fcov.diagonal())


# ---- 7: handle hygiene --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2])
def test_predict_is_unchanged_by_a_joint_call_and_the_scratch_goes_back(lib, mode):
    m, xs, idx = _case("rbf1100", 300)
    ref = _ref("rbf1100").take(idx)
    h = m.posterior.L.handle
    with _options(lib, predict_inverse=mode):
        before = m.predict(xs)                                            # fixes the handle's form: Wd (mode 0) or Linv (mode 2)
        s0 = _pool_state(lib, h)
        z = np.random.default_rng(3).standard_normal((300, 4))
        m.predict_joint(xs)
        m.sample_posterior(xs, z=z, noise=True)
        s1 = _pool_state(lib, h)
        m.predict_joint(xs)
        m.sample_posterior(xs, z=z, noise=True)
        s2 = _pool_state(lib, h)
        after = m.predict(xs)
    assert s0[8] > 0                                                      # (the handle's own buffers are out: the counter counts)
    assert s1[7:] == s0[7:] and s2[7:] == s0[7:], (s0, s1, s2)          # outstanding scratch is back to its value before the calls
    assert s1[4:7] == s0[4:7] and s2[4:7] == s0[4:7], (s0, s1, s2)      # nothing new on the handle
    assert s1[0] == s0[0] and s2[0] == s0[0]                              # the factor pool is untouched
    assert s2[:4] == s1[:4], (s1, s2)                                     # ... and the idle pool does not grow from call to call
    assert np.array_equal(np.asarray(before[2]), np.asarray(after[2])) and np.array_equal(np.asarray(before[3]), np.asarray(after[3]))
    worst, where = P.check(np.asarray(after[2]).ravel(), np.asarray(after[3]).ravel(), ref.pref)
    assert worst <= 1.0, (worst, where)


def test_a_joint_call_that_fixes_the_handles_form_keeps_predict_within_tolerance(lib):
    """A fresh n = 1100 handle without the fit's inverse rows, default predict_inverse: predict at 300 points takes the blocked solve,
    the joint call at 1153 points takes the product form and leaves W = L^-1 on the handle, and the same predict then takes the
    product form.  Before and after are two evaluations of the same prediction: each inside the long-double bar, and apart by at
    most the two tolerances added."""
    with _options(lib, keep_inverse=0):
        m, spec, pool, ms = _build("rbf1100")
    idx = P.select(J.MODELS["rbf1100"][5], 300)
    xs = pool[idx]
    h = m.posterior.L.handle
    post = m.posterior
    ref = P.cached(spec, np.array(m.covfunc.hyp, dtype=float), m.x, xs, ms[idx], post.alpha, post.sW, np.asarray(post.L))
    s0 = _pool_state(lib, h)
    assert s0[5] == 0 and s0[6] == 0                                      # neither W nor the inverse rows
    before = m.predict(xs)
    s1 = _pool_state(lib, h)
    assert s1[4] == 1 and s1[5] == 0                                      # the blocked solve: Wd
    fmu, fcov = m.predict_joint(J.chol_points("rbf1100", 1153))
    s2 = _pool_state(lib, h)
    assert s2[5] == 1                                                     # the joint call took the product form: W is on the handle
    assert s2[7:] == s1[7:], (s1, s2)                                     # (W comes from the factor pool; the scratch is back)
    after = m.predict(xs)
    b = [np.asarray(before[k]).ravel() for k in (2, 3)]
    a = [np.asarray(after[k]).ravel() for k in (2, 3)]
    for got in (b, a):
        worst, where = P.check(got[0], got[1], ref)
        print("joint hygiene, form fixed by the joint call: %.3g of the tolerance at %s" % (worst, where))
        assert worst <= 1.0, (worst, where)
    t_mu, t_s2 = ref.tol()
    assert np.all(np.abs(a[0] - b[0]) <= 2 * t_mu) and np.all(np.abs(a[1] - b[1]) <= 2 * t_s2)
    assert not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))  # the form did change
