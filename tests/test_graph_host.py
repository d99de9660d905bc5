"""CPU: the cov.Pre contract, its place in device programs, the refusals, the host half of pygps_amd.GraphExtensions and the
numpy restatement tests/graph_cpu.py -- the latter two against fixtures recorded from the reference
(tests/golden/make_golden_graph.py).  No device call is made here."""
import numpy as np
import pytest

import graph_cpu
from conftest import golden


def _adj(n, edges):
    A = np.zeros((n, n))
    A[edges[0], edges[1]] = 1.0
    return A


def _pre(n=6, ns=3, seed=0):
    import pygps_amd as pyGPs
    rng = np.random.RandomState(seed)
    B = rng.randn(n, n)
    return pyGPs.cov.Pre(rng.randn(n + 1, ns), B @ B.T), n, ns


# ---- cov.Pre -------------------------------------------------------------------------------------------------
def test_pre_contract_modes_and_derivative_error():
    k, n, ns = _pre()
    x, z = np.zeros((n, 1)), np.zeros((ns, 1))
    assert k.hyp == [] and k.para == []
    assert k.getCovMatrix(x=x, mode='train') is k.M2
    assert np.array_equal(k.getCovMatrix(x=x, z=z, mode='cross'), k.M1[:-1, :])
    st = k.getCovMatrix(z=z, mode='self_test')
    assert st.shape == (ns, 1) and np.array_equal(st[:, 0], k.M1[-1, :])
    assert k.getDerMatrix(x=x, mode='train') == 0                      # Core/cov.py:1452-1455
    with pytest.raises(Exception) as e:
        k.getDerMatrix(x=x, mode='train', der=0)
    assert str(e.value) == "Error: NO optimization in precomputed kernel matrix"


def test_pre_shape_checks():
    import pygps_amd as pyGPs
    rng = np.random.RandomState(1)
    with pytest.raises(Exception, match="square"):
        pyGPs.cov.Pre(rng.randn(7, 3), rng.randn(6, 5))
    with pytest.raises(Exception, match="one row more"):
        pyGPs.cov.Pre(rng.randn(6, 3), np.eye(6))
    k, n, ns = _pre()
    with pytest.raises(Exception, match="training inputs"):
        k.getCovMatrix(x=np.zeros((n + 1, 1)), mode='train')
    with pytest.raises(Exception, match="test inputs"):
        k.getCovMatrix(x=np.zeros((n, 1)), z=np.zeros((ns + 2, 1)), mode='cross')
    with pytest.raises(Exception, match="test inputs"):
        k.getCovMatrix(z=np.zeros((ns + 2, 1)), mode='self_test')
    with pytest.raises(Exception, match="one row more"):
        k.M1 = rng.randn(n, ns)
    # a fit checks M2 against the training inputs before anything reaches the device
    m = pyGPs.GPR()
    m.setPrior(kernel=k + pyGPs.cov.RBF())
    with pytest.raises(Exception, match="training inputs"):
        m.getPosterior(np.zeros((n + 2, 1)), np.zeros((n + 2, 1)))


def test_pre_alone_keeps_the_zero_mean():
    """Core/gp.py:221-222: setPrior with a Pre (not a tree that holds one) switches the label-mean default off."""
    import pygps_amd as pyGPs
    k, n, ns = _pre()
    y = np.ones((n, 1))
    m = pyGPs.GPC()
    m.setPrior(kernel=k)
    m.setData(np.zeros((n, 1)), y)
    assert isinstance(m.meanfunc, pyGPs.mean.Zero)
    m = pyGPs.GPC()
    m.setPrior(kernel=k + pyGPs.cov.RBFunit())
    m.setData(np.zeros((n, 1)), y)
    assert isinstance(m.meanfunc, pyGPs.mean.Const)


def test_pre_tokens_follow_rebinding_and_touch():
    k, n, ns = _pre()
    t1, t2 = k._tok1, k._tok2
    k.M1 = k.M1.copy()
    assert k._tok1 != t1 and k._tok2 == t2
    k.M2 = k.M2.copy()
    assert k._tok2 != t2
    t1, t2 = k._tok1, k._tok2
    k.M2[0, 0] += 1.0                       # in place: nothing notices ...
    assert (k._tok1, k._tok2) == (t1, t2)
    k.touch()                               # ... until told
    assert k._tok1 != t1 and k._tok2 != t2
    other, _, _ = _pre(seed=2)
    assert len({k._tok1, k._tok2, other._tok1, other._tok2}) == 4


def test_pre_token_streams():
    import pygps_amd as pyGPs
    from pygps_amd import _lib
    cov = pyGPs.cov
    k, n, ns = _pre()
    L, PRE = _lib.PROG_LEAF, _lib.COV_PRE
    assert PRE == 12
    assert (k + cov.RBFunit())._tokens() == [L, PRE, 0, 0, 0, L, _lib.COV_RBFUNIT, 0, 0, 0, _lib.PROG_SUM]
    assert (k * 0.5)._tokens() == [L, PRE, 0, 0, 1, _lib.PROG_SCALE, 0]
    assert (k * cov.RBF())._tokens() == [L, PRE, 0, 0, 0, L, _lib.COV_RBF, 0, 0, 0, _lib.PROG_PRODUCT]
    assert (cov.RBF() + k * 0.5)._tokens() == [L, _lib.COV_RBF, 0, 0, 0, L, PRE, 0, 0, 3, _lib.PROG_SCALE, 2, _lib.PROG_SUM]
    assert (k + cov.RBFunit()).hyp == [0.] and (k * 0.5).hyp == [0.5]
    for tree in (k + cov.RBFunit(), k * 0.5, k * cov.RBF()):
        assert tree._on_device() and len(tree._program(0)) == 4
    assert k._on_device() and k._program(0)[0] == [L, PRE, 0, 0, 0]


def test_two_pre_leaves_and_the_switch_take_the_dense_route():
    import pygps_amd as pyGPs
    from pygps_amd import inf
    cov = pyGPs.cov
    k, n, ns = _pre()
    k2, _, _ = _pre(seed=3)
    assert (k + k2)._on_device() is False
    assert (k * k2 + cov.RBF())._on_device() is False
    assert inf._dense_route(k + k2) and not inf._dense_route(k + cov.RBF())
    tree = k * 0.3 + cov.RBF()
    assert tree._on_device()
    k.device_leaf = False                                   # the A/B switch, per object here
    try:
        assert tree._on_device() is False and k._on_device() is False
        assert inf._dense_route(tree) and inf._dense_route(k)
    finally:
        del k.device_leaf
    assert tree._on_device() and pyGPs.cov.Pre.device_leaf is True


def test_trees_with_pre_combine_their_matrices_on_the_host():
    """getCovMatrix / getDerMatrix of a tree that holds a Pre: the Pre slices its arrays, the other child is stubbed here
    (its own matrices are device-built and covered on the GPU)."""
    import pygps_amd as pyGPs
    cov = pyGPs.cov
    k, n, ns = _pre()
    x = np.zeros((n, 1))
    sc = k * 0.5
    assert np.allclose(sc.getCovMatrix(x=x, mode='train'), np.exp(0.5) * k.M2, rtol=1e-15)
    assert np.allclose(sc.getDerMatrix(x=x, mode='train', der=0), 2 * np.exp(0.5) * k.M2, rtol=1e-15)
    assert np.array_equal((k + k).getCovMatrix(z=np.zeros((ns, 1)), mode='self_test')[:, 0], 2 * k.M1[-1])

    class Stub(cov.Kernel):
        def __init__(self):
            self.hyp, self.para = [0.1], []

        def getCovMatrix(self, x=None, z=None, mode=None):
            return np.full((n, n), 2.0)

        def getDerMatrix(self, x=None, z=None, mode=None, der=None):
            return np.full((n, n), 3.0)
    pr = k * Stub()
    assert pr._on_device() is False
    assert np.array_equal(pr.getCovMatrix(x=x, mode='train'), 2.0 * k.M2)
    assert np.array_equal(pr.getDerMatrix(x=x, mode='train', der=0), 3.0 * k.M2)        # the RBF-side derivative weighted by M2


def test_refusals_name_cov_pre():
    import pygps_amd as pyGPs
    cov, inf = pyGPs.cov, pyGPs.inf
    k, n, ns = _pre()
    x, y = np.zeros((n, 1)), np.ones((n, 1))
    u = np.zeros((2, 1))
    for tree in (k, k + cov.RBF()):
        with pytest.raises(NotImplementedError, match="cov.Pre"):
            tree.fitc(u)
        with pytest.raises(NotImplementedError, match="cov.Pre"):
            inf.Exact(sharded=True).evaluate(pyGPs.mean.Zero(), tree, pyGPs.lik.Gauss(), x, y, 3)
        mc = pyGPs.GPMC(2)
        mc.setPrior(kernel=tree)
        mc.setData(x, np.array([0, 1] * (n // 2)).reshape(n, 1))
        with pytest.raises(NotImplementedError, match="cov.Pre"):
            mc.fitAndPredict(np.zeros((ns, 1)))
        with pytest.raises(NotImplementedError, match="cov.Pre"):
            mc.optimizeAndPredict(np.zeros((ns, 1)))
    fk = cov.RBF().fitc(u)
    fk.covfunc = k                                          # smuggled in behind the constructor's check
    for eng, lik in ((inf.FITC_Exact(), pyGPs.lik.Gauss()), (inf.FITC_EP(), pyGPs.lik.Erf())):
        with pytest.raises(NotImplementedError, match="cov.Pre"):
            eng.evaluate(pyGPs.mean.Zero(), fk, lik, x, y, 3)


# ---- GraphExtensions, host half ------------------------------------------------------------------------------
def test_graph_extensions_import_and_argument_rules():
    """The module layout, and the argument rules that are decided before any device work (nodeKernels.py:114-119)."""
    import pygps_amd
    from pygps_amd.GraphExtensions import graphUtil, nodeKernels
    assert pygps_amd.GraphExtensions.graphUtil is graphUtil and pygps_amd.GraphExtensions.nodeKernels is nodeKernels
    A = _adj(4, np.array([[0, 1, 1, 2, 2, 3], [1, 0, 2, 1, 3, 2]]))
    with pytest.raises(Exception, match="Step parameter p needs to be larger than 0"):
        nodeKernels.rwKernel(A, p=0.9)
    with pytest.raises(ValueError, match="square"):
        nodeKernels.diffKernel(np.zeros((3, 4)))
    with pytest.raises(ValueError, match="1 <= k < n"):
        graphUtil.formKnnGraph(np.zeros((4, 2)), 4)


def test_form_kernel_matrix_and_normalize_kernel_bit_for_bit():
    from pygps_amd.GraphExtensions import graphUtil
    g, a = golden("G25_kernel_matrix_helpers"), golden("G25_node_kernels_a")
    K = a["diff"]
    for fn in (graphUtil.formKernelMatrix, graph_cpu.form_kernel_matrix):
        M1, M2 = fn(K, g["train"], g["test"])
        assert np.array_equal(M1, g["M1"]) and np.array_equal(M2, g["M2"])
        M1, M2 = fn(K, list(g["train"]), list(g["test"]))                   # index lists, as the demo passes them
        assert np.array_equal(M1, g["M1"]) and np.array_equal(M2, g["M2"])
    assert np.array_equal(graphUtil.normalizeKernel(K), g["normalized"])
    assert np.array_equal(graph_cpu.normalize_kernel(K), g["normalized"])


def test_host_node_kernels_against_the_reference():
    """normLap and cosKernel are elementwise: bit for bit.  psInvLapKernel is the same LAPACK call on the same matrix."""
    from pygps_amd.GraphExtensions import nodeKernels
    a, b = golden("G25_node_kernels_a"), golden("G25_node_kernels_b")
    A = _adj(int(a["ndks"][0]), a["edges"])
    assert np.array_equal(nodeKernels.normLap(A), a["normLap"])
    assert np.array_equal(nodeKernels.cosKernel(A), b["cos"])
    P = nodeKernels.psInvLapKernel(A)
    assert np.max(np.abs(P - b["psInv"])) <= 1e-12 * np.max(np.abs(b["psInv"]))


def test_graph_cpu_against_the_reference():
    """The restatement the GPU tests build their inputs with.  Elementwise results bit for bit; the inverses, the power
    and the eigendecomposition route are the same LAPACK / BLAS calls on bit-identical inputs, held to 1e-12 of max|K|
    (inputs of condition <= 3 for the two inverses: spectrum of I + L in [1, 3], of I - S / 2 in [1/2, 3/2])."""
    a, b = golden("G25_node_kernels_a"), golden("G25_node_kernels_b")
    n, d, k, seed = (int(v) for v in a["ndks"])
    pts = np.random.RandomState(seed).randn(n, d)
    A = graph_cpu.form_knn_graph(pts, k)
    assert np.array_equal(A, _adj(n, a["edges"]))
    assert np.array_equal(graph_cpu.norm_lap(A), a["normLap"])
    assert np.array_equal(graph_cpu.cos_kernel(A), b["cos"])
    for got, want in ((graph_cpu.reg_lap_kernel(A, 1), a["regLap"]), (graph_cpu.reg_lap_kernel(A, 0.7), a["regLap_s07"]),
                      (graph_cpu.diff_kernel(A, 0.5), a["diff"]), (graph_cpu.ps_inv_lap_kernel(A), b["psInv"]),
                      (graph_cpu.vnd_kernel(A, 0.5), b["VND"]), (graph_cpu.rw_kernel(A, 3, 2), b["rw_p3_a2"]),
                      (graph_cpu.rw_kernel(A, 2.7, 0.5), b["rw_p2_a1"])):
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
    with pytest.raises(Exception, match="larger than 0"):
        graph_cpu.rw_kernel(A, 0.5)


def test_graph_cpu_knn_graph_equals_the_reference_on_tie_free_data():
    g = golden("G25_knn_graphs")
    for tag in ("a", "usps"):
        n, d, k, seed = (int(v) for v in g[tag + "_ndks"])
        pts = np.random.RandomState(seed).randn(n, d)
        if tag == "usps":
            pts = np.tanh(pts)
        A = graph_cpu.form_knn_graph(pts, k)
        assert np.array_equal(A, _adj(n, g[tag + "_edges"])) and np.array_equal(A.sum(axis=0), g[tag + "_degree"])
        assert np.array_equal(A, A.T) and not np.any(np.diag(A))


def test_graph_problem_rebuilds_the_recorded_pre_matrices():
    g = golden("G25_pre_fits_N300")
    n, ns, d, seed = (int(v) for v in g["ntds"])
    p = graph_cpu.graph_problem(n, ns, d, seed)
    assert p["M2"].shape == (n, n) and p["M1"].shape == (n + 1, ns)
    assert np.max(np.abs(p["M1"] - g["M1"])) <= 1e-12 and np.max(np.abs(np.diag(p["M2"]) - g["M2_diag"])) <= 1e-12
    assert np.max(np.abs(p["M2"][0] - g["M2_row0"])) <= 1e-12
    assert float(g["eig_min"]) > 1e-3                       # the conditioning the fits rest on


def test_graph_cpu_against_the_reference_at_the_device_test_sizes():
    """n = 200 (full matrices) and n = 1500 (diagonal, K v, sampled entries): the inputs and expected values of
    tests/test_gpu_graph.py, same 1e-12 of max|K| as above."""
    for name, fn in (("regLap", lambda A: graph_cpu.reg_lap_kernel(A, 0.7)), ("VND", lambda A: graph_cpu.vnd_kernel(A, 0.5)),
                     ("rw", lambda A: graph_cpu.rw_kernel(A, 3, 2)), ("diff", lambda A: graph_cpu.diff_kernel(A, 0.5))):
        g = golden("G25_node_n200_" + name)
        n, d, k, seed = (int(v) for v in g["ndks"])
        A = graph_cpu.form_knn_graph(np.random.RandomState(seed).randn(n, d), k)
        assert np.array_equal(A, _adj(n, g["edges"]))
        assert np.max(np.abs(fn(A) - g["K"])) <= 1e-12 * np.max(np.abs(g["K"]))
    g = golden("G25_node_kernels_n1500")
    n, d, k, seed = (int(v) for v in g["ndks"])
    A = graph_cpu.form_knn_graph(np.random.RandomState(seed).randn(n, d), k)
    assert np.array_equal(A, _adj(n, g["edges"]))
    K = graph_cpu.diff_kernel(A, 0.5)
    m = float(g["diff_absmax"])
    assert np.max(np.abs(np.diag(K) - g["diff_diag"])) <= 1e-12 * m and np.max(np.abs(K[g["ii"], g["jj"]] - g["diff_entries"])) <= 1e-12 * m


def test_pre_asymmetric_m2_is_refused_before_it_reaches_the_device():
    """The device program mirrors one triangle, the dense route uses the whole matrix: an asymmetric M2 is an error at bind
    time (rounding-level asymmetry, as a product B B' has, passes)."""
    k, n, ns = _pre()
    k._check_symmetric()
    M = np.array(k.M2)
    M[1, 0] += 1e-3
    k.M2 = M
    with pytest.raises(Exception, match="M2 must be symmetric"):
        k._check_symmetric()
