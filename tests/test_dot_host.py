"""CPU: the host-side surface of the dot-product kernels cov.Linear, cov.Poly and cov.LINard that needs no device
(constructors, hyper layout, the reference's exceptions, program tokens and the accumulator budget, refusals, route selection)
and the long-double reference tests/dot_ref_ld.py -- against every matrix the reference recorded (tests/golden/G27_dot_k_*)
within twice its derived bar, which also pins the LINard definition at ell = 1, and through a numpy exact GP against the
recorded fits."""
import numpy as np
import pytest

from conftest import golden, relerr
import dot_ref_ld as DR


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    from pygps_amd import _lib

    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(_lib, "ctx", touched)


def test_constructors_defaults_and_kinds():
    from pygps_amd import cov, _lib
    assert cov.Linear().hyp == [0.] and cov.Linear().para == []
    assert cov.Linear(0.3).hyp == [0.3]
    assert cov.Poly().hyp == [0., 0.] and cov.Poly().para == [2]
    k = cov.Poly(0.1, 3, 0.2)                              # positional order: log_c, d, log_sigma
    assert k.hyp == [0.1, 0.2] and k.para == [3]
    assert cov.LINard(D=3).hyp == [0., 0., 0.]
    assert cov.LINard(log_ell_list=[0.1, 0.2]).hyp == [0.1, 0.2]
    assert (cov.Linear._kind, cov.Poly._kind, cov.LINard._kind) == (13, 14, 15)
    assert (_lib.COV_LINEAR, _lib.COV_POLY, _lib.COV_LINARD) == (13, 14, 15)
    assert cov.Linear(0.3)._device_params() == (13, 0, 0)
    assert cov.Poly(0., 3 + 1e-10, 0.)._device_params() == (14, 3, 0)          # the rounding rule of Core/cov.py:640-643
    assert cov.Poly(0., 2.7, 0.)._device_params() == (14, 2, 0)                # int() after the assert, as the reference


def test_exceptions_with_the_reference_text():
    from pygps_amd import cov
    x = np.zeros((4, 3))
    for k in (cov.Linear(), cov.Poly(), cov.LINard(D=3)):
        with pytest.raises(Exception, match="Specify the mode"):
            k.getCovMatrix(x=x)
        with pytest.raises(Exception, match="Specify at least one"):
            k.getCovMatrix(mode="train")
        with pytest.raises(Exception, match="Specify both"):
            k.getCovMatrix(x=x, mode="cross")
        with pytest.raises(Exception, match="Specify the index"):
            k.getDerMatrix(x=x, mode="train")
    with pytest.raises(Exception, match="Wrong derivative index in covLinear"):
        cov.Linear().getDerMatrix(x=x, mode="train", der=1)
    with pytest.raises(Exception, match="Wrong derivative entry in Poly"):
        cov.Poly().getDerMatrix(x=x, mode="train", der=3)
    with pytest.raises(Exception, match="Wrong derivative index in covLINard"):
        cov.LINard(D=3).getDerMatrix(x=x, mode="train", der=3)
    with pytest.raises(Exception, match="Wrong derivative index in covLINard"):
        cov.LINard(D=3).getDerMatrix(z=x, mode="self_test", der=5)
    for bad in (0, -1, 0.5):
        with pytest.raises(AssertionError):                # Core/cov.py:642
            cov.Poly(d=bad).getCovMatrix(x=x, mode="train")
        with pytest.raises(AssertionError):
            cov.Poly(d=bad).getDerMatrix(x=x, mode="train", der=0)


def test_program_tokens_and_the_accumulator_budget():
    from pygps_amd import cov, _lib
    LEAF, SUM, PROD, SCALE = _lib.PROG_LEAF, _lib.PROG_SUM, _lib.PROG_PRODUCT, _lib.PROG_SCALE
    k = cov.Linear() + cov.RBF()
    assert k._on_device()
    assert k._tokens() == [LEAF, 13, 0, 0, 0, LEAF, _lib.COV_RBF, 0, 0, 1, SUM]
    k = cov.Linear() * cov.Poly(d=3) + cov.RBFard(D=4)      # one ARD leaf + the dot product: two extra accumulators
    assert k._on_device()
    assert k._tokens() == [LEAF, 13, 0, 0, 0, LEAF, 14, 3, 0, 1, PROD, LEAF, _lib.COV_RBFARD, 0, 0, 3, SUM]
    k = 0.5 * cov.Linear() + cov.RBF()
    assert k._tokens() == [LEAF, 13, 0, 0, 1, SCALE, 0, LEAF, _lib.COV_RBF, 0, 0, 2, SUM]
    assert not (cov.Linear() + cov.RBFard(D=2) + cov.RQard(D=2))._on_device()           # three accumulators
    assert (cov.RBFard(D=2) + cov.RQard(D=2))._on_device()
    assert (cov.Linear() + cov.Poly() * cov.Poly(d=3) + cov.Linear() * cov.RBFard(D=2))._on_device()   # the dot leaves share one
    assert not (cov.LINard(D=2) + cov.RBF())._on_device() and cov.LINard(D=2)._program(0) is None
    assert (cov.Linear() + cov.RBFard(D=300))._tokens() is None                          # an ARD leaf of a program: D <= 64
    assert cov.Linear()._program(7)[0] == [LEAF, 13, 0, 0, 7]
    pre = cov.Pre(np.zeros((4, 2)), np.eye(3))
    assert (pre + cov.RBF())._on_device() and not (pre + cov.Linear())._on_device()
    with pytest.raises(AssertionError):                    # Poly's degree is checked when the tokens are made
        (cov.Poly(d=0) + cov.RBF())._tokens()


def test_flatten_order_of_hyp():
    from pygps_amd import cov
    k = cov.Linear(0.1) * cov.Poly(0.2, 3, 0.3) + cov.RBFard(log_ell_list=[0.4, 0.5], log_sigma=0.6)
    assert k.hyp == [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]
    k.hyp = [1., 2., 3., 4., 5., 6.]
    assert k.cov1.cov1.hyp == [1.] and k.cov1.cov2.hyp == [2., 3.] and k.cov2.hyp == [4., 5., 6.]
    s = 0.5 * cov.Linear(0.1) + cov.RBF(0.3, -0.1)
    assert s.hyp == [0.5, 0.1, 0.3, -0.1]
    s2 = cov.Linear(0.1) * 0.5
    assert s2.hyp == [0.5, 0.1]
    for name, tree in DR.CASES.items():                    # the recorded flatten order
        for d in (3, 17):
            h = golden("G27_dot_kernels_inputs")["%s_d%d_hyp" % (name, d)]
            assert list(DR.build(tree, h, cov, d).hyp) == list(h)


def test_refusals_and_route_selection():
    import pygps_amd as pyGPs
    from pygps_amd import cov, inf
    u = np.zeros((5, 2))
    for k in (cov.Linear(), cov.Poly(), cov.LINard(D=2), cov.Linear() + cov.RBF(), 0.5 * cov.Poly() * cov.RBF()):
        assert k._dot_leaves()
        with pytest.raises(NotImplementedError, match="dot-product kernels"):
            k.fitc(u)
        with pytest.raises(NotImplementedError, match="dot-product kernels"):
            inf.Exact(sharded=True).evaluate(pyGPs.mean.Zero(), k, pyGPs.lik.Gauss(), np.zeros((8, 2)), np.zeros((8, 1)), 1)
        m = pyGPs.GPMC(3)
        m.setPrior(kernel=k)
        assert m.choose_route(100, device_bytes=288 * 2.0 ** 30) == "pairs"
    assert not (cov.RBF() + cov.Const())._dot_leaves()
    m = pyGPs.GPMC(3)
    m.setPrior(kernel=cov.RBF())
    m.x_all, m.y_all = np.zeros((30, 2)), np.repeat(np.arange(3), 10).reshape(-1, 1)
    assert m.choose_route(100, device_bytes=288 * 2.0 ** 30) == "shared"


@pytest.mark.parametrize("d", [3, 17])
@pytest.mark.parametrize("name", sorted(DR.CASES))
def test_helper_reproduces_every_recorded_matrix(name, d):
    """Within twice the helper's bar: once for the helper's fp64 model, once for the reference's own fp64 evaluation."""
    g = golden("G27_dot_kernels_inputs")
    x, z, hyp = g["x%d" % d], g["z%d" % d], g["%s_d%d_hyp" % (name, d)]
    tree = DR.CASES[name]
    rec = DR.golden_sets(golden, name, d)
    nd = DR.n_der(name, tree, hyp)
    assert sorted(rec) == sorted(["K"] + ["dK%d" % i for i in range(nd)])
    for key, mats in rec.items():
        der = None if key == "K" else int(key[2:])
        for mode, kw in (("train", dict(x=x)), ("cross", dict(x=x, z=z)), ("self", dict(z=z))):
            K, bar = DR.tree_matrix(tree, hyp, mode="self_test" if mode == "self" else mode, der=der, **kw)
            assert K.shape == mats[mode].shape
            err = np.abs(K - mats[mode].astype(np.longdouble)).astype(np.float64)
            assert np.all(err <= 2.0 * bar), (name, d, key, mode, float(np.max(err / np.maximum(bar, 1e-300))))


@pytest.mark.parametrize("name", sorted(DR.FITS))
def test_numpy_exact_gp_on_the_helper_matrices_reproduces_the_recorded_fits(name):
    g = golden("G27_dot_fit_" + name)
    x, y, hyp = g["x"], g["y"], g["cov_hyp"]
    tree = DR.FITS[name]
    f64 = lambda t: t[0].astype(np.float64)
    K = f64(DR.tree_matrix(tree, hyp, x=x, mode="train"))
    dKs = [f64(DR.tree_matrix(tree, hyp, x=x, mode="train", der=i)) for i in range(len(hyp))]
    m = (g["mean_hyp"][0] if g["mean_hyp"].size else 0.0) * np.ones_like(y)
    sn2 = float(np.exp(2 * g["lik_hyp"][0]))
    nlZ, alpha, Ld, dcov, dlik = DR.exact_gp(K, dKs, y, m, sn2)
    assert relerr(nlZ, g["nlZ"]) < 1e-9 and relerr(alpha, g["alpha"]) < 1e-6 and relerr(Ld, g["L_diag"]) < 1e-8
    assert relerr(dcov, g["dnlZ_cov"]) < 1e-7 and relerr(dlik, g["dnlZ_lik"]) < 1e-7
    assert float(g["cond"]) <= 1e7
