"""CPU: the mathematics and the host API of learned FITC inducing inputs (no device).

  * the long-double analytic gradient d nlZ / d xu of tests/fitc_xu_ref_ld.py against long-double central differences of the
    long-double nlZ, every supported kind, D = 1 and 3, inducing inputs off and on training points;
  * every single-slip mutant of the float64 restatement lies outside the tolerance rule the device comparisons use;
  * GP_FITC.learnInducing, the optimiser's vector mean | cov | lik | xu.ravel(), restarts, and the refusals.

Measured here: central differences at e = 3e-5 and 6e-5, extrapolated to remove their e^2 term, agree with the analytic gradient to
5.4e-10 max |gradient| at worst (RQard in one dimension; plain central differences at any one step stay above 2e-8, between their
truncation and the rounding of nlZ through Kuu + 1e-6 sn2 I); FD_BOUND is 8 times that.  The weakest mutant rejection is 'no_cw' at
3.2e11 times the tolerance (test_every_single_slip_mutant_exceeds_the_tolerance prints every factor)."""
import numpy as np
import pytest

import fitc_xu_ref_ld as R

FD_BOUND = 8 * 5.4e-10


def _case(kind, D, on_points, n=40, nu=6, seed=3):
    rng = np.random.RandomState(seed + 10 * D)
    x = rng.randn(n, D)
    y = np.sin(x.sum(1)) + 0.1 * rng.randn(n)
    xu = rng.randn(nu, D)
    if on_points:
        xu[:3] = x[:3]
    hyp = list(0.3 * rng.randn(R.nhyp(kind, D)))
    if kind in ("RBFard", "RQard"):
        hyp[:D] = list(np.log(0.8 + 0.4 * rng.rand(D)))
    return hyp, x, y, np.zeros(n), xu


@pytest.mark.parametrize("on_points", [False, True])
@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("kind", R.KINDS)
def test_analytic_gradient_equals_central_differences_in_long_double(kind, D, on_points):
    hyp, x, y, m, xu = _case(kind, D, on_points)
    g = R.grad_exact(kind, hyp, -1.0, x, y, m, xu)
    f = lambda u: R.nlz_exact(kind, hyp, -1.0, x, y, m, u)
    fd = (4 * R.central_difference(f, xu, 3e-5) - R.central_difference(f, xu, 6e-5)) / 3
    err = float(np.abs(g - fd).max() / np.abs(g).max())
    print("central differences, %s D=%d on=%d: %.3g" % (kind, D, on_points, err))
    assert err <= FD_BOUND, err


def test_sites_adjoint_reduces_to_the_exact_one():
    """With ttau = 1 / sn2 and tnu = (y - m) / sn2 the EP quantities are FITC_Exact's: s = 1 / g, t o b = (y - m) / g."""
    hyp, x, y, m, xu = _case("Matern5", 3, True)
    sn2 = np.exp(2 * R.LD(-1.0))
    a = R.grad_exact("Matern5", hyp, -1.0, x, y, m, xu)
    b = R.grad_sites("Matern5", hyp, R.LD(1e-6) * sn2, x, xu, np.full(40, 1 / sn2), (R._as(y, R.LD) - m) / sn2)
    assert float(np.abs(a - b).max()) < 1e-15 * float(np.abs(a).max())


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_single_slip_mutant_exceeds_the_tolerance(mutant):
    kind = "Matern5" if mutant == "rbf_kprime" else "RBFard"
    hyp, x, y, m, xu = _case(kind, 3, True, n=200, nu=12)
    ref, tol, e64 = R.exact_case(kind, hyp, -1.0, x, y, m, xu)
    assert tol.max() <= R.CAP * np.abs(ref).max()
    good = R.grad_exact(kind, hyp, -1.0, x, y, m, xu, np.float64)
    assert float((np.abs(good - ref) / tol).max()) <= 1.0                 # the restatement itself passes
    bad = R.grad_exact(kind, hyp, -1.0, x, y, m, xu, np.float64, mutant)
    factor = float((np.abs(bad - ref) / tol).max())
    print("mutant %s: %.3g times the tolerance" % (mutant, factor))
    assert factor > 1.0, (mutant, factor)


# ---- host API ---------------------------------------------------------------------------------------------------------------------
def _model(kernel=None, nu=4, D=2):
    import pygps_amd as pyGPs
    m = pyGPs.GPR_FITC()
    u = np.arange(nu * D, dtype=float).reshape(nu, D) / 10
    m.setPrior(mean=pyGPs.mean.Const(0.5), kernel=kernel if kernel is not None else pyGPs.cov.RBF(0.1, 0.2), inducing_points=u)
    m.setNoise(-1.0)
    return m, u


def test_learn_inducing_sets_the_flag():
    import pygps_amd as pyGPs
    m, u = _model()
    assert m.covfunc.learn_inducing is False and pyGPs.cov.FITCOfKernel.learn_inducing is False
    m.learnInducing()
    assert m.covfunc.learn_inducing is True
    m.learnInducing(False)
    assert m.covfunc.learn_inducing is False
    with pytest.raises(Exception, match="setData"):
        pyGPs.GPR_FITC().learnInducing()
    assert pyGPs.inf.dnlZStruct(m.meanfunc, m.covfunc, m.likfunc).xu is None


def test_optimiser_vector_packs_and_unpacks_the_inducing_inputs():
    m, u = _model()
    off = m.optimizer._convert_to_array()
    assert off.tolist() == [0.5, 0.1, 0.2, -1.0]                          # what it was: mean | cov | lik
    m.optimizer._apply_in_objects(off + 1.0)
    assert m.covfunc.hyp == [1.1, 1.2] and np.array_equal(m.covfunc.inducingInput, u) and m.u is u
    m.optimizer._apply_in_objects(off)
    m.learnInducing()
    v = m.optimizer._convert_to_array()
    assert v.tolist() == [0.5, 0.1, 0.2, -1.0] + u.ravel().tolist()
    w = v + np.arange(v.size)
    m.optimizer._apply_in_objects(w)
    assert m.meanfunc.hyp == [0.5] and m.covfunc.hyp == [1.1, 2.2] and m.likfunc.hyp == [2.0]
    assert np.array_equal(m.u, (u.ravel() + np.arange(4, 12)).reshape(u.shape))
    assert np.array_equal(m.u, m.covfunc.inducingInput) and m.u.shape == u.shape
    assert np.array_equal(m.optimizer._convert_to_array(), w)


def test_a_restart_redraws_the_hyper_parameters_only(monkeypatch):
    from pygps_amd import opt
    m, u = _model()
    m.learnInducing()
    m.setOptimizer("Minimize", num_restarts=3, meanRange=[(2, 3)], covRange=[(4, 5), (6, 7)], likRange=[(8, 9)])
    seen = []

    def one(self, hyp0, numIters):
        seen.append(np.array(hyp0, copy=True))
        hyp0[4:] += 1.0                                                  # a minimiser that moved the inducing inputs in place
        return opt._Run(True, float(len(seen)), np.array(hyp0, copy=True), 1)
    monkeypatch.setattr(opt.Minimize, "_one", one)
    m.optimizer.findMin(m.x, m.y, 5)
    assert len(seen) == 3
    assert seen[0].tolist() == [0.5, 0.1, 0.2, -1.0] + u.ravel().tolist()
    for s in seen[1:]:
        assert np.array_equal(s[4:], u.ravel())                           # the inducing inputs findMin began with
        assert 2 <= s[0] <= 3 and 4 <= s[1] <= 5 and 6 <= s[2] <= 7 and 8 <= s[3] <= 9


def test_sharded_minimize_refuses_learned_inducing_inputs():
    m, u = _model()
    m.learnInducing()
    m.setOptimizer("ShardedMinimize", num_restarts=2)
    with pytest.raises(NotImplementedError, match="ShardedMinimize"):
        m.optimizer.findMin(m.x, m.y, 5)


def _unsupported():
    from pygps_amd import cov
    return [cov.Matern(0.1, 1, 0.2), cov.PiecePoly(0.1, 2, 0.2), cov.Periodic(0.1, 0.2, 0.3), cov.Gabor(0.1, 0.2), cov.Const(0.1),
            cov.Noise(0.1), cov.SM(1, [0.1, 0.2, 0.3, 0.2, 0.3], D=2), cov.RBF() + cov.RBF(), cov.RBF() * cov.Matern(0.1, 3, 0.2),
            cov.RBF() * 2.0]


@pytest.mark.parametrize("idx", range(10))
def test_unsupported_kernels_refuse_before_device_work(idx):
    import pygps_amd as pyGPs
    k = _unsupported()[idx]
    D = 1 if isinstance(k, pyGPs.cov.Periodic) else 2
    x = np.random.RandomState(0).randn(12, D)
    y = np.sign(x[:, :1])
    fk = k.fitc(x[:3].copy())
    fk.learn_inducing = True
    with pytest.raises(NotImplementedError, match=type(k).__name__):
        pyGPs.inf.FITC_Exact().evaluate(pyGPs.mean.Zero(), fk, pyGPs.lik.Gauss(), x, y, 3)
    with pytest.raises(NotImplementedError, match=type(k).__name__):
        pyGPs.inf.FITC_EP().evaluate(pyGPs.mean.Zero(), fk, pyGPs.lik.Erf(), x, y, 3)
