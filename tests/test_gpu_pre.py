"""GPU: cov.Pre as a resident leaf of the device program -- fits and predictions against fixtures recorded from the reference
(tests/golden/make_golden_graph.py: G25), the program route against the dense route (Pre.device_leaf = False: K and every
derivative matrix built on the host; the two share no assembly code), more test points than the reference can take, and
the residency rules.  Inputs are rebuilt from seeds by tests/graph_cpu.py, itself pinned to the fixtures on the CPU.

Tolerances are those the suite already holds the same quantities to: Exact nlZ 1e-9, alpha 1e-7, dnlZ 1e-7 (G6); EP identical
sweep count, nlZ 1e-8, alpha / sW / dnlZ 1e-6 (G8); Laplace nlZ 1e-8, alpha / sW / L / dnlZ 1e-6, predictions 1e-7 absolute
(G20); the optimiser run nlZ 1e-5, hypers 1e-4 (G1b)."""
import numpy as np
import pytest

import graph_cpu
from conftest import golden, relerr

pytestmark = pytest.mark.gpu

_problems = {}


def problem(n, ns, d=8, seed=0):
    key = (n, ns, d, seed)
    if key not in _problems:
        _problems[key] = graph_cpu.graph_problem(n, ns, d, seed)
    return _problems[key]


def fixture_problem():
    g = golden("G25_pre_fits_N300")
    n, ns, d, seed = (int(v) for v in g["ntds"])
    p = problem(n, ns, d, seed)
    assert np.max(np.abs(p["M1"] - g["M1"])) <= 1e-12 and np.max(np.abs(np.diag(p["M2"]) - g["M2_diag"])) <= 1e-12
    return g, p


def pre_of(p):
    import pygps_amd as pyGPs
    return pyGPs.cov.Pre(p["M1"], p["M2"])


def check_pred(pred, g, tag, tol):
    ym, ys2, fm, fs2, lp = pred
    for got, k in ((ym, "pred_ym"), (ys2, "pred_ys2"), (fm, "pred_fm"), (fs2, "pred_fs2")):
        assert got.shape == g[tag + "_" + k].shape
        assert relerr(got, g[tag + "_" + k]) < tol, (tag, k)


# ---- against the reference --------------------------------------------------------------------------------------
def test_gpc_pre_alone_ep_matches_reference(lib):
    """demo_NodeKernel's second model: GPC on the diffusion kernel of a 3-NN graph, dummy inputs."""
    import pygps_amd as pyGPs
    g, p = fixture_problem()
    n, ns = p["M2"].shape[0], p["M1"].shape[1]
    m = pyGPs.GPC()
    m.setPrior(kernel=pre_of(p))
    m.setData(np.zeros((n, 1)), p["y"])
    assert m.covfunc._on_device()
    nlZ, dnlZ, post = m.getPosterior()
    assert not post.L.dense
    assert m.inffunc.sweeps == int(g["pre_ep_n_sweeps"])
    assert relerr(nlZ, g["pre_ep_nlZ"]) < 1e-8
    assert relerr(post.alpha, g["pre_ep_alpha"]) < 1e-6 and relerr(post.sW, g["pre_ep_sW"]) < 1e-6
    assert relerr(np.diag(np.asarray(post.L)), g["pre_ep_L_diag"]) < 1e-6
    assert isinstance(m.meanfunc, pyGPs.mean.Zero)              # Pre alone keeps the zero mean (Core/gp.py:221-222)
    assert dnlZ.cov == [] and dnlZ.mean == [] and dnlZ.lik == [] and g["pre_ep_dnlZ_mean"].size == 0
    check_pred(m.predict(np.zeros((ns, 1))), g, "pre_ep", 1e-6)
    check_pred(m.predict_with_posterior(post, np.zeros((ns, 1))), g, "pre_ep", 1e-6)


@pytest.mark.parametrize("engine", ["ep", "laplace"])
def test_gpc_pre_plus_rbfunit_matches_reference(lib, engine):
    """demo_NodeKernel's third model, EP and Laplace: nlZ, the RBFunit gradient, predictions."""
    import pygps_amd as pyGPs
    g, p = fixture_problem()
    tag = "sum_" + engine
    m = pyGPs.GPC()
    if engine == "laplace":
        m.useInference("Laplace")
    m.setPrior(kernel=pre_of(p) + pyGPs.cov.RBFunit(np.log(2.5)))
    m.setData(p["x"], p["y"])
    assert m.covfunc._on_device()
    nlZ, dnlZ, post = m.getPosterior()
    assert not post.L.dense
    if engine == "ep":
        assert m.inffunc.sweeps == int(g[tag + "_n_sweeps"])
    assert relerr(nlZ, g[tag + "_nlZ"]) < 1e-8
    assert relerr(post.alpha, g[tag + "_alpha"]) < 1e-6 and relerr(post.sW, g[tag + "_sW"]) < 1e-6
    assert relerr(np.diag(np.asarray(post.L)), g[tag + "_L_diag"]) < 1e-6
    assert relerr(dnlZ.cov, g[tag + "_dnlZ_cov"]) < 1e-6 and relerr(dnlZ.mean, g[tag + "_dnlZ_mean"]) < 1e-6
    ym, ys2, fm, fs2, lp = m.predict(p["xs"])
    if engine == "laplace":
        for got, k in ((ym, "pred_ym"), (ys2, "pred_ys2"), (fm, "pred_fm"), (fs2, "pred_fs2")):
            assert np.max(np.abs(got - g[tag + "_" + k])) <= 1e-7, k
    else:
        check_pred((ym, ys2, fm, fs2, lp), g, tag, 1e-6)


@pytest.mark.parametrize("tag", ["scale_sum", "prod"])
def test_gpr_pre_trees_exact_match_reference(lib, tag):
    """Pre * s + RBF (the Scale node's gradient is 2 exp(h) M2 through the Hadamard sum) and Pre * RBF (the RBF
    derivatives are weighted by M2)."""
    import pygps_amd as pyGPs
    cov = pyGPs.cov
    g, p = fixture_problem()
    k = pre_of(p) * 0.4 + cov.RBF(np.log(2.0), -0.3) if tag == "scale_sum" else pre_of(p) * cov.RBF(np.log(3.0), 0.2)
    assert relerr(k.hyp, g[tag + "_cov_hyp"]) < 1e-15
    m = pyGPs.GPR()
    m.setPrior(mean=pyGPs.mean.Zero(), kernel=k)
    m.setNoise(np.log(0.2))
    m.setData(p["x"], g["yr"])
    assert m.covfunc._on_device()
    nlZ, dnlZ, post = m.getPosterior()
    assert not post.L.dense
    assert relerr(nlZ, g[tag + "_nlZ"]) < 1e-9
    assert relerr(post.alpha, g[tag + "_alpha"]) < 1e-7
    assert relerr(np.diag(np.asarray(post.L)), g[tag + "_L_diag"]) < 1e-9
    assert relerr(dnlZ.cov, g[tag + "_dnlZ_cov"]) < 1e-7 and relerr(dnlZ.lik, g[tag + "_dnlZ_lik"]) < 1e-7
    ym, ys2, fm, fs2, lp = m.predict(p["xs"])
    assert relerr(ym, g[tag + "_pred_ym"]) < 1e-8 and np.max(np.abs(fs2 - g[tag + "_pred_fs2"])) <= 1e-7
    assert np.max(np.abs(ys2 - g[tag + "_pred_ys2"])) <= 1e-7


def test_optimize_pre_plus_rbfunit_matches_reference(lib):
    import pygps_amd as pyGPs
    g = golden("G25_pre_optimize_N300")
    n, ns, d, seed = (int(v) for v in g["ntds"])
    p = problem(n, ns, d, seed)
    m = pyGPs.GPC()
    m.setPrior(kernel=pre_of(p) + pyGPs.cov.RBFunit(float(g["cov_hyp0"][0])))
    m.setData(p["x"], p["y"])
    m.optimize(numIterations=int(g["iters"]))
    assert abs(float(m.nlZ) - float(g["opt_nlZ"])) < 1e-5 * abs(float(g["opt_nlZ"]))
    assert relerr(m.covfunc.hyp, g["cov_hyp"]) < 1e-4
    ym, ys2, fm, fs2, lp = m.predict(p["xs"])
    assert relerr(ym, g["pred_ym"]) < 1e-5 and relerr(fs2, g["pred_fs2"]) < 1e-4


# ---- the program route against the dense route -------------------------------------------------------------------
def _fit_predict(make_model, p, xs, device_leaf, batch=None):
    import pygps_amd as pyGPs
    from pygps_amd import _lib
    Pre = pyGPs.cov.Pre
    ctx = _lib.ctx()
    Pre.device_leaf = device_leaf
    try:
        m = make_model()
        assert m.covfunc._on_device() is device_leaf
        nlZ, dnlZ, post = m.getPosterior()
        assert bool(post.L.dense) is (not device_leaf)
        if batch:
            _lib.check(_lib.load().pgp_set_option(ctx, b"predict_batch", batch))
        try:
            pred = m.predict(xs)
        finally:
            if batch:
                _lib.load().pgp_set_option(ctx, b"predict_batch", 65536)
    finally:
        Pre.device_leaf = True
    grads = np.array(list(dnlZ.mean) + list(dnlZ.cov) + list(dnlZ.lik), dtype=float)
    return nlZ, grads, post, pred


CASES = ["exact_scale_sum", "exact_prod", "exact_alone", "exact_ard_tree", "ep_sum", "ep_alone", "laplace_sum"]


@pytest.mark.parametrize("case", CASES)
def test_program_route_equals_dense_route(lib, case):
    """n = 333 is not a multiple of the 64 tile (nor of the 128 padding); 700 test points in batches of 256 span three
    predict batches, the last one partial."""
    import pygps_amd as pyGPs
    cov = pyGPs.cov
    n, ns, d = 333, 700, 5
    p = problem(n, ns, d, seed=4)
    yr = np.sin(p["x"] @ np.ones((d, 1)) / np.sqrt(d)) + 0.1 * np.random.RandomState(6).randn(n, 1)
    xs = p["xs"]

    def make_model():
        pre = pre_of(p)
        if case.startswith("exact"):
            m = pyGPs.GPR()
            k = {"exact_scale_sum": lambda: pre * 0.4 + cov.RBF(np.log(2.0), -0.3),
                 "exact_prod": lambda: pre * cov.RBF(np.log(3.0), 0.2),
                 "exact_alone": lambda: pre,
                 "exact_ard_tree": lambda: (pre * cov.RBFard(log_ell_list=[0.9, 1.1, 1.0, 0.8, 1.2], log_sigma=0.1)) * -0.2
                 + cov.Matern(np.log(2.0), 3, -0.5)}[case]()
            m.setPrior(mean=pyGPs.mean.Const(0.1), kernel=k)
            m.setNoise(np.log(0.2))
            m.setData(np.zeros((n, 1)) if case == "exact_alone" else p["x"], yr)
        else:
            m = pyGPs.GPC()
            if case.startswith("laplace"):
                m.useInference("Laplace")
            m.setPrior(kernel=pre if case == "ep_alone" else pre + cov.RBFunit(np.log(2.5)))
            m.setData(np.zeros((n, 1)) if case == "ep_alone" else p["x"], p["y"])
        return m

    if case.endswith("alone"):
        xs = np.zeros((ns, 1))
    a = _fit_predict(make_model, p, xs, True, batch=256)
    b = _fit_predict(make_model, p, xs, False)
    exact = case.startswith("exact")
    assert relerr(a[0], b[0]) < (1e-9 if exact else 1e-8)
    assert relerr(a[2].alpha, b[2].alpha) < (1e-7 if exact else 1e-6)
    assert relerr(a[2].sW, b[2].sW) < 1e-6
    assert relerr(np.diag(np.asarray(a[2].L)), np.diag(np.asarray(b[2].L))) < (1e-9 if exact else 1e-6)
    assert a[1].shape == b[1].shape
    if b[1].size:                                           # (GPC on a Pre alone with its zero mean has no hyper at all)
        assert np.max(np.abs(a[1] - b[1])) <= (1e-7 if exact else 1e-6) * np.max(np.abs(b[1])), (a[1], b[1])
    for u, v in zip(a[3][:4], b[3][:4]):
        assert u.shape == (ns, 1)
        assert np.max(np.abs(u - v)) <= 1e-7 * max(1.0, float(np.max(np.abs(v))))


def test_predict_with_more_than_1000_test_points(lib):
    """The reference batches xs by 1000 while its Pre returns all of M1 (Core/gp.py:395-406): it cannot do this."""
    import pygps_amd as pyGPs
    cov = pyGPs.cov
    n, ns, d = 320, 1500, 5
    p = problem(n, ns, d, seed=7)
    yr = np.sin(p["x"] @ np.ones((d, 1)) / np.sqrt(d)) + 0.1 * np.random.RandomState(8).randn(n, 1)

    def make_model():
        m = pyGPs.GPR()
        m.setPrior(mean=pyGPs.mean.Zero(), kernel=pre_of(p) * 0.2 + cov.RBF(np.log(2.0), -0.3))
        m.setNoise(np.log(0.2))
        m.setData(p["x"], yr)
        return m
    a = _fit_predict(make_model, p, p["xs"], True, batch=1024)
    b = _fit_predict(make_model, p, p["xs"], False)
    for u, v in zip(a[3][:4], b[3][:4]):
        assert u.shape == (ns, 1)
        assert np.max(np.abs(u - v)) <= 1e-7 * max(1.0, float(np.max(np.abs(v))))
    assert np.all(a[3][3] >= 0) and np.std(a[3][0]) > 0.05


# ---- residency ---------------------------------------------------------------------------------------------------
def test_a_second_model_on_the_same_context(lib):
    """Model B (another Pre, other sizes) fits and predicts on the context that holds A's matrices; A's posterior then
    predicts exactly what it predicted before, and refits to the same numbers."""
    import pygps_amd as pyGPs
    cov = pyGPs.cov
    pa, pb = problem(300, 20, 8, 0), problem(333, 700, 5, 4)

    def model(p):
        m = pyGPs.GPC()
        m.setPrior(kernel=pre_of(p) + cov.RBFunit(np.log(2.5)))
        m.setData(p["x"], p["y"])
        return m
    A, B = model(pa), model(pb)
    nlZ_a, _, post_a = A.getPosterior()
    first = A.predict(pa["xs"])
    nlZ_b, _, post_b = B.getPosterior()
    first_b = B.predict(pb["xs"])
    again = A.predict(pa["xs"])
    again_wp = A.predict_with_posterior(post_a, pa["xs"])
    for u, v, w in zip(first[:4], again[:4], again_wp[:4]):
        assert np.array_equal(u, v) and np.array_equal(u, w)
    again_b = B.predict(pb["xs"])
    for u, v in zip(first_b[:4], again_b[:4]):
        assert np.array_equal(u, v)
    A2 = model(pa)
    assert A2.getPosterior()[0] == nlZ_a
    # a wrong number of test points is an error, not a read of whatever M1 is resident
    with pytest.raises(Exception, match="test inputs"):
        A.predict(pb["xs"])


def test_rebinding_and_touch_reach_the_device(lib):
    import pygps_amd as pyGPs
    cov = pyGPs.cov
    p = problem(300, 20, 8, 0)
    yr = np.sin(p["x"] @ np.ones((8, 1)) / np.sqrt(8.0))
    pre = pyGPs.cov.Pre(p["M1"].copy(), p["M2"].copy())
    m = pyGPs.GPR()
    m.setPrior(mean=pyGPs.mean.Zero(), kernel=pre + cov.RBF(np.log(2.0), -0.3))
    m.setNoise(np.log(0.2))
    m.setData(p["x"], yr)
    nlZ0 = m.getPosterior()[0]
    ym0 = m.predict(p["xs"])[0]
    pre.M2[np.diag_indices(300)] += 0.5                 # in place: the resident copy is still the old one ...
    assert m.getPosterior()[0] == nlZ0
    pre.touch()                                         # ... until told
    nlZ1 = m.getPosterior()[0]
    assert abs(nlZ1 - nlZ0) > 1e-3
    pre.M2 = p["M2"]                                    # rebinding needs no touch()
    assert m.getPosterior()[0] == nlZ0
    pre.M1 = 2.0 * p["M1"]
    ym1 = m.predict(p["xs"])[0]
    assert np.max(np.abs(ym1 - ym0)) > 1e-3
    pre.M1 = p["M1"]
    assert np.array_equal(m.predict(p["xs"])[0], ym0)


def test_demo_node_kernel_flow(lib):
    """Demo/USPS/demo_NodeKernel.py end to end on a synthetic graph: its three models (RBF, Pre, Pre + RBFunit) through
    optimize and predict.  The class is sign(ym) of predict(xs) WITHOUT ys, as in the demo: with ys given, lik.Erf's ym is
    2 p(y = ys) - 1, whose sign says whether the prediction is right, not which class it is (Core/lik.py:251-269).

    The bound: labels are sign(x.w / sqrt(d) + 0.3 e) with x.w / sqrt(d) of standard deviation |w| / sqrt(d) ~ 1, so the
    best possible accuracy is 1 - atan(0.3) / pi ~ 0.91; over 20 test points its standard deviation is ~0.07, and 0.7 lies
    three of those below.  The graph kernel alone knows the inputs only through their 3-NN graph and gets no bound."""
    import pygps_amd as pyGPs
    cov = pyGPs.cov
    p = problem(300, 20, 8, 0)
    n, ns = 300, 20
    acc = {}
    for tag in ("rbf", "pre", "sum"):
        m = pyGPs.GPC()
        if tag == "rbf":
            m.setPrior(kernel=cov.RBF(np.log(2.5), 0.0))
        elif tag == "pre":
            m.setPrior(kernel=pre_of(p))
        else:
            m.setPrior(kernel=pre_of(p) + cov.RBFunit(np.log(2.5)))
        x, xs = (np.zeros((n, 1)), np.zeros((ns, 1))) if tag == "pre" else (p["x"], p["xs"])
        m.setData(x, p["y"])
        m.optimize(numIterations=5)
        ym, ys2, fm, fs2, lp = m.predict(xs)
        assert ym.shape == (ns, 1) and np.all(np.isfinite(ym)) and np.all(fs2 >= 0) and lp is None
        acc[tag] = float(np.mean(np.sign(ym) == p["ys"]))
        lp = m.predict(xs, ys=p["ys"])[4]
        assert lp.shape == (ns, 1) and np.all(np.isfinite(lp)) and np.all(lp <= 0)
    assert acc["rbf"] >= 0.7 and acc["sum"] >= 0.7, acc
