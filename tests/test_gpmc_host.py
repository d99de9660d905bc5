"""CPU: pygps_amd.GPMC's surface (Core/gp.py:738-932) -- defaults, exception texts, createBinaryClass, pair order, the
empty-class check, the host vote arithmetic and the choice of route -- without a device.  Fixtures: G24
(tests/golden/make_golden_gpmc.py), data from tests/gpmc_data.py."""
import numpy as np
import pytest

import gpmc_cpu
import gpmc_data
from conftest import golden


def _model(name, **kw):
    import pygps_amd as pyGPs
    shape = gpmc_data.SHAPES[name]
    x, y, xs = gpmc_data.blobs(**shape)
    m = pyGPs.GPMC(len(shape["counts"]), **kw)
    mean, kernel = gpmc_data.prior(name, pyGPs.cov, pyGPs.mean)
    if mean is not None or kernel is not None:
        m.setPrior(mean=mean, kernel=kernel)
    m.setData(x, y)
    return m, xs


def test_defaults_and_setters():
    import pygps_amd as pyGPs
    m = pyGPs.GPMC(7)
    assert m.n_class == 7 and m.x_all is None and m.y_all is None
    assert type(m.meanfunc) is pyGPs.mean.Zero and type(m.covfunc) is pyGPs.cov.RBF
    assert list(m.covfunc.hyp) == list(pyGPs.cov.RBF().hyp)
    assert m.newPrior is False and m.newInf is None and m.newLik is None
    assert m.shared_kernel is True and m.last_route is None
    assert m.pair_nlZ == {} and m.pair_iters == {} and m.pair_hyp == {}
    k, mu = pyGPs.cov.RBF(0.3, 0.1), pyGPs.mean.Const(0.5)
    m.setPrior(kernel=k)
    assert m.covfunc is k and m.newPrior is True and type(m.meanfunc) is pyGPs.mean.Zero
    m.setPrior(mean=mu)
    assert m.meanfunc is mu and m.covfunc is k
    m2 = pyGPs.GPMC(3)
    m2.setPrior()                                       # the reference sets newPrior whatever the arguments (gp.py:772)
    assert m2.newPrior is True
    with pytest.raises(AssertionError, match="mean function is not an instance of"):
        m.setPrior(mean=pyGPs.cov.RBF())
    with pytest.raises(AssertionError, match="cov function is not an instance of"):
        m.setPrior(kernel=pyGPs.mean.Zero())
    assert pyGPs.GPMC(3, shared_kernel=False).shared_kernel is False


def test_exception_texts():
    import pygps_amd as pyGPs
    m = pyGPs.GPMC(3)
    with pytest.raises(Exception) as e:
        m.useInference("EP")
    assert str(e.value) == 'Possible inf values are "Laplace".'
    with pytest.raises(Exception) as e:
        m.useLikelihood("Logistic")
    assert str(e.value) == "Logistic likelihood is currently not implemented."
    with pytest.raises(Exception) as e:
        m.useLikelihood("Erf")
    assert str(e.value) == 'Possible lik values are "Logistic".'
    with pytest.raises(AssertionError, match="number of inputs and labels does not match"):
        m.setData(np.zeros((4, 2)), np.zeros((3, 1)))


def test_setData_reshapes_1d():
    import pygps_amd as pyGPs
    m = pyGPs.GPMC(2)
    m.setData(np.arange(6.0), np.array([0, 1, 0, 1, 1, 0.0]))
    assert m.x_all.shape == (6, 1) and m.y_all.shape == (6, 1)
    x, y = m.createBinaryClass(0, 1)
    assert x.reshape(-1).tolist() == [0, 2, 5, 1, 3, 4] and y.reshape(-1).tolist() == [1, 1, 1, -1, -1, -1]
    assert y.shape == (6, 1)


@pytest.mark.parametrize("name", ["fit_default", "fit_c5_uneven", "fit_c10_d64"])
def test_createBinaryClass_matches_the_recorded_index_order(name):
    import pygps_amd as pyGPs
    g = golden("G24_" + name)
    shape = gpmc_data.SHAPES[name]
    x, y, _ = gpmc_data.blobs(**shape)
    i, j = (int(v) for v in g["binary_pair"])
    m = pyGPs.GPMC(int(g["n_class"]))
    m.setData(np.arange(x.shape[0], dtype=float), y)    # the "inputs" are the row numbers, as the recipe recorded them
    bx, by = m.createBinaryClass(i, j)
    assert np.array_equal(bx.reshape(-1).astype(np.int64), g["binary_index"])
    assert np.array_equal(by.reshape(-1), g["binary_y"]) and by.shape == (len(g["binary_index"]), 1)
    m.setData(x, y)
    bx2, _ = m.createBinaryClass(i, j)
    assert np.array_equal(bx2, x[g["binary_index"]])
    # two ascending runs, not globally sorted (the data are permuted)
    n1 = int(np.sum(g["binary_y"] > 0))
    idx = g["binary_index"]
    assert np.all(np.diff(idx[:n1]) > 0) and np.all(np.diff(idx[n1:]) > 0) and idx[n1] < idx[n1 - 1]
    assert np.array_equal(gpmc_cpu.binary_class(x, y, i, j)[2], idx)


def test_pair_order():
    import pygps_amd as pyGPs
    assert pyGPs.GPMC(4).pairs() == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert pyGPs.GPMC(10).pairs() == gpmc_cpu.pairs(10) and len(pyGPs.GPMC(10).pairs()) == 45


def test_empty_class_raises_before_any_device_work(monkeypatch):
    import pygps_amd as pyGPs
    from pygps_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(_lib, "ctx", no_device)
    x, y, xs = gpmc_data.blobs(seed=1, counts=[5, 6, 7], d=2, ns=4)
    for fn in ("fitAndPredict", "optimizeAndPredict"):
        m = pyGPs.GPMC(4)                               # class 3 has no training point
        m.setData(x, y)
        with pytest.raises(Exception) as e:
            getattr(m, fn)(xs)
        assert type(e.value) is Exception and "class 3" in str(e.value)
    m = pyGPs.GPMC(3)
    m.setData(x, np.where(y == 1, 2.0, y))              # ... nor has class 1 here
    with pytest.raises(Exception) as e:
        m.fitAndPredict(xs)
    assert type(e.value) is Exception and "class 1" in str(e.value)


@pytest.mark.parametrize("name", ["fit_default", "fit_laplace"])
def test_host_vote_arithmetic_reproduces_the_recorded_votes(name):
    """Per-pair ym from the CPU restatement (pinned to the same fixture by test_gpmc_oracle.py) through GPMC.add_votes."""
    import pygps_amd as pyGPs
    g = golden("G24_" + name)
    shape = gpmc_data.SHAPES[name]
    x, y, xs = gpmc_data.blobs(**shape)
    kind, hyp, para, c = gpmc_data.oracle_prior(name)
    C = int(g["n_class"])
    _, _, _, yms = gpmc_cpu.fit_and_predict(kind, hyp, para, x, y, C, xs, laplace=name == "fit_laplace")
    votes = np.zeros((xs.shape[0], C))
    for i, j in pyGPs.GPMC(C).pairs():
        pyGPs.GPMC.add_votes(votes, yms[(i, j)], i, j)
    votes /= votes.sum(axis=1)[:, np.newaxis]
    assert np.max(np.abs(votes - g["votes"]) / g["votes"]) < 1e-12
    assert np.max(np.abs(votes.sum(axis=1) - 1)) < 1e-14


class _FakeGPC(object):
    """Stands in for GPC in the "pairs" route: records what GPMC does with each pair's model."""
    log = []

    def __init__(self):
        from pygps_amd import inf
        self.inffunc = inf.EP()
        self.covfunc = None
        self.nlZ = None
        self.calls = []
        _FakeGPC.log.append(self)

    def setPrior(self, mean=None, kernel=None):
        self.calls.append(("setPrior", mean, kernel))
        self.covfunc = kernel

    def useInference(self, name):
        from pygps_amd import inf
        self.calls.append(("useInference", name))
        self.inffunc = inf.Laplace()

    def _fit(self, what, x, y):
        self.calls.append((what, x.shape[0], int(np.sum(y > 0))))
        self.nlZ = float(x.shape[0])
        self.inffunc.sweeps = 3
        self.inffunc.newton_steps = 5
        if self.covfunc is None:
            import pygps_amd as pyGPs
            self.covfunc = pyGPs.cov.RBF()

    def getPosterior(self, x, y):
        self._fit("getPosterior", x, y)

    def optimize(self, x, y):
        self._fit("optimize", x, y)
        self.covfunc.hyp = [h + 0.25 for h in self.covfunc.hyp]       # "optimised": visible to the next pair through a shared kernel

    def predict(self, xs):
        k = len(_FakeGPC.log)
        return (np.tanh(0.1 * k + 0.01 * np.arange(xs.shape[0], dtype=float)).reshape(-1, 1),)


@pytest.mark.parametrize("laplace", [False, True])
def test_pairs_route_order_votes_and_inference_on_the_host(monkeypatch, laplace):
    import pygps_amd as pyGPs
    from pygps_amd import gp, inf
    monkeypatch.setattr(gp, "GPC", _FakeGPC)
    _FakeGPC.log = []
    counts = [5, 6, 7, 4]
    x, y, xs = gpmc_data.blobs(seed=3, counts=counts, d=2, ns=9)
    m = pyGPs.GPMC(4, shared_kernel=False)
    m.setData(x, y)
    if laplace:
        m.useInference("Laplace")
        assert m.newInf == "Laplace" and isinstance(m.inffunc, inf.Laplace)
    votes = m.fitAndPredict(xs)
    assert m.last_route == "pairs" and len(_FakeGPC.log) == 6
    want = np.zeros((9, 4))
    for k, (i, j) in enumerate(gpmc_cpu.pairs(4)):
        fake = _FakeGPC.log[k]
        fits = [c for c in fake.calls if c[0] == "getPosterior"]
        assert fits == [("getPosterior", counts[i] + counts[j], counts[i])]          # the pairs in the reference's order
        # useInference("Laplace") takes effect for every pair (the reference ignores it: class docstring)
        assert [c for c in fake.calls if c[0] == "useInference"] == ([("useInference", "Laplace")] if laplace else [])
        assert not [c for c in fake.calls if c[0] == "setPrior"]                      # no user prior: a default GPC per pair
        gpmc_cpu.add_votes(want, np.tanh(0.1 * (k + 1) + 0.01 * np.arange(9.0)), i, j)
        assert m.pair_nlZ[(i, j)] == counts[i] + counts[j]
        assert m.pair_iters[(i, j)] == (5 if laplace else 3)
    assert np.array_equal(votes, gpmc_cpu.normalise(want))
    assert np.max(np.abs(votes.sum(axis=1) - 1)) < 1e-14


def test_real_pair_models_use_the_chosen_inference():
    import pygps_amd as pyGPs
    from pygps_amd import inf
    m = pyGPs.GPMC(3)
    assert isinstance(m._new_pair_model().inffunc, inf.EP)
    m.useInference("Laplace")
    pm = m._new_pair_model()
    assert isinstance(pm, pyGPs.GPC) and isinstance(pm.inffunc, inf.Laplace) and isinstance(pm.likfunc, pyGPs.lik.Erf)


def test_optimize_chains_the_starts_through_a_user_prior_only(monkeypatch):
    import pygps_amd as pyGPs
    from pygps_amd import gp
    monkeypatch.setattr(gp, "GPC", _FakeGPC)
    x, y, xs = gpmc_data.blobs(seed=3, counts=[5, 6, 7], d=2, ns=4)
    _FakeGPC.log = []
    m = pyGPs.GPMC(3)
    k = pyGPs.cov.RBF(0.0, 0.0)
    m.setPrior(kernel=k)
    m.setData(x, y)
    m.optimizeAndPredict(xs)
    assert m.last_route == "pairs"
    assert all(f.covfunc is k for f in _FakeGPC.log)                                  # the same kernel object for every pair
    assert [m.pair_hyp[p] for p in m.pairs()] == [[0.25, 0.25], [0.5, 0.5], [0.75, 0.75]]
    _FakeGPC.log = []
    m = pyGPs.GPMC(3)
    m.setData(x, y)
    m.optimizeAndPredict(xs)
    assert [m.pair_hyp[p] for p in m.pairs()] == [[0.25, 0.25]] * 3                   # a fresh default GPC per pair


def test_route_selection_without_a_device(monkeypatch):
    import pygps_amd as pyGPs
    from pygps_amd import _lib
    cov = pyGPs.cov

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(_lib, "ctx", no_device)
    HBM = 288 * 2.0 ** 30
    m, xs = _model("fit_program")
    assert m.covfunc._on_device()
    assert m.choose_route(xs.shape[0], device_bytes=HBM) == "shared"                  # a device program
    m, xs = _model("fit_default")
    assert m.choose_route(xs.shape[0], device_bytes=HBM) == "shared"                  # no setPrior: GPC's default RBF
    m, xs = _model("fit_ard_const")
    assert m.choose_route(xs.shape[0], device_bytes=HBM) == "shared"                  # one ARD leaf, Const mean
    d = gpmc_data.SHAPES["fit_ard_const"]["d"]
    tree = cov.RBFard(D=d) + cov.RBFard(D=d) * cov.RBFard(D=d)                        # three ARD leaves: not a device program
    assert not tree._on_device()
    m.setPrior(kernel=tree)
    assert m.choose_route(xs.shape[0], device_bytes=HBM) == "pairs"
    m, xs = _model("fit_program", shared_kernel=False)
    assert m.choose_route(xs.shape[0], device_bytes=HBM) == "pairs"
    # the memory guard: K_all plus one batch of Ks_all (and the pairs' blocks) must fit
    m, xs = _model("fit_c5_uneven")
    need = m.shared_bytes(xs.shape[0])
    n_p = (m.x_all.shape[0] + 127) // 128 * 128
    assert need > 8 * (n_p * n_p + n_p * 384)
    assert m.choose_route(xs.shape[0], device_bytes=HBM) == "shared"
    assert m.choose_route(xs.shape[0], device_bytes=4 * need - 8) == "pairs"          # a quarter of the device, as DeviceFactor.reserve
    m.shared_memory_limit = need
    assert m.choose_route(xs.shape[0]) == "shared"
    m.shared_memory_limit = need - 1
    assert m.choose_route(xs.shape[0]) == "pairs"
