"""GPU: the device half of pygps_amd.GraphExtensions -- the four O(n^3) node kernels (pgp_node_kernel) and the k-NN graph
(pgp_knn_graph) -- against the numpy restatement tests/graph_cpu.py and against fixtures recorded from the reference
(tests/golden/make_golden_graph.py: G25).

The tolerance is measured, not chosen.  tests/graph_ld.py computes each kernel in np.longdouble (Gauss-Jordan for the two
inverses, repeated multiplication for the power, the scaled Taylor series for the exponential) and reports how far the
float64 routes of tests/graph_cpu.py (LAPACK inverse, matrix_power, eigh) are from it, relative to max|K|:

            n = 200      n = 1500
    regLap  6.5e-16      1.2e-15
    VND     6.7e-16      6.7e-16
    rw      3.9e-16      2.8e-16
    diff    1.8e-15      2.5e-15

The device is allowed 8 times that with a floor of 1e-13 (its inverse and its exponential take different but equally stable
routes), relative to max|K|: TOL below -- the floor everywhere.  Measured on an MI355X against the fixtures: regLap 1.6e-15 /
4.4e-15 (n = 200 / 1500), VND 1.8e-15 / 5.0e-15, rw 1.1e-16 / 4.2e-16, diff 2.4e-14 / 7.9e-14 (four squarings double the error of the
scaled exponential four times).  Against the float64 restatement and the float64 fixtures the allowance covers both
sides' errors, so the same figure is used for both comparisons."""
import numpy as np
import pytest

import graph_cpu
from conftest import golden

pytestmark = pytest.mark.gpu

F64_ERR = {200: dict(regLap=6.5e-16, VND=6.7e-16, rw=3.9e-16, diff=1.8e-15),
           1500: dict(regLap=1.2e-15, VND=6.7e-16, rw=2.8e-16, diff=2.5e-15)}
TOL = {n: {k: max(8.0 * e, 1e-13) for k, e in d.items()} for n, d in F64_ERR.items()}

_graphs = {}


def graph(n):
    if n not in _graphs:
        _graphs[n] = graph_cpu.form_knn_graph(np.random.RandomState(5).randn(n, 8), 3)
    return _graphs[n]


def device_kernel(name, A):
    from pygps_amd.GraphExtensions import nodeKernels
    return {"regLap": lambda: nodeKernels.regLapKernel(A, 0.7), "VND": lambda: nodeKernels.VNDKernel(A, 0.5),
            "rw": lambda: nodeKernels.rwKernel(A, 3, 2), "diff": lambda: nodeKernels.diffKernel(A, 0.5)}[name]()


def cpu_kernel(name, A):
    return {"regLap": lambda: graph_cpu.reg_lap_kernel(A, 0.7), "VND": lambda: graph_cpu.vnd_kernel(A, 0.5),
            "rw": lambda: graph_cpu.rw_kernel(A, 3, 2), "diff": lambda: graph_cpu.diff_kernel(A, 0.5)}[name]()


@pytest.mark.parametrize("name", ["regLap", "VND", "rw", "diff"])
def test_node_kernel_n200_full_matrix(lib, name):
    """n = 200 is no multiple of the 128 padding and spans two blocks of the Cholesky."""
    g = golden("G25_node_n200_" + name)
    A = graph(200)
    assert np.array_equal(np.stack(np.nonzero(A)), g["edges"])
    K = device_kernel(name, A)
    ref = cpu_kernel(name, A)
    m = float(np.max(np.abs(g["K"])))
    err_cpu, err_fix = float(np.max(np.abs(K - ref))) / m, float(np.max(np.abs(K - g["K"]))) / m
    print("n=200 %s: device vs graph_cpu %.3e, vs fixture %.3e (allowed %.3e)" % (name, err_cpu, err_fix, TOL[200][name]))
    assert K.shape == (200, 200) and np.max(np.abs(K - K.T)) <= 1e-15 * m
    assert err_cpu <= TOL[200][name] and err_fix <= TOL[200][name]


@pytest.mark.parametrize("name", ["regLap", "VND", "rw", "diff"])
def test_node_kernel_n1500_sampled(lib, name):
    """n = 1500: twelve blocks, 128-tiles in the GEMM; the fixture holds the diagonal, K v and 3000 sampled entries.  K v sums
    1500 products per entry, so it is compared relative to max|K| |v|_1."""
    g = golden("G25_node_kernels_n1500")
    A = graph(1500)
    assert np.array_equal(np.stack(np.nonzero(A)), g["edges"])
    K = device_kernel(name, A)
    ref = cpu_kernel(name, A)
    m, tol = float(g[name + "_absmax"]), TOL[1500][name]
    errs = dict(cpu=float(np.max(np.abs(K - ref))) / m,
                diag=float(np.max(np.abs(np.diag(K) - g[name + "_diag"]))) / m,
                entries=float(np.max(np.abs(K[g["ii"], g["jj"]] - g[name + "_entries"]))) / m,
                Kv=float(np.max(np.abs(K @ g["v"] - g[name + "_Kv"]))) / (m * float(np.sum(np.abs(g["v"])))))
    print("n=1500 %s: %s (allowed %.3e)" % (name, errs, tol))
    assert all(e <= tol for e in errs.values()), errs


def test_rw_kernel_argument_rules_on_the_device(lib):
    """int(p), a <= 1 becomes 1.0001 (nodeKernels.py:114-119): the reference's own rw_p2_a1 was recorded with p = 2.7, a = 0.5;
    p = 1 takes no product at all."""
    from pygps_amd.GraphExtensions import nodeKernels
    a, b = golden("G25_node_kernels_a"), golden("G25_node_kernels_b")
    n = int(a["ndks"][0])
    A = np.zeros((n, n))
    A[a["edges"][0], a["edges"][1]] = 1.0
    want = b["rw_p2_a1"]
    assert np.max(np.abs(nodeKernels.rwKernel(A, 2.7, 0.5) - want)) <= 1e-13 * np.max(np.abs(want))
    one = graph_cpu.rw_kernel(A, 1, 2)
    assert np.max(np.abs(nodeKernels.rwKernel(A, 1, 2) - one)) <= 1e-13 * np.max(np.abs(one))
    for got, want in ((nodeKernels.regLapKernel(A), a["regLap"]), (nodeKernels.diffKernel(A), a["diff"]),
                      (nodeKernels.VNDKernel(A), b["VND"])):                    # the default arguments
        assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))


def test_vnd_kernel_alpha_above_one_is_a_linalg_error(lib):
    """I - alpha S has a negative eigenvalue for alpha > 1 (S has the eigenvalue 1): an ordinary non-PD return code."""
    from pygps_amd.GraphExtensions import nodeKernels
    with pytest.raises(np.linalg.LinAlgError):
        nodeKernels.VNDKernel(graph(200), 1.5)
    K = nodeKernels.VNDKernel(graph(200), 0.5)                                  # the context is fine afterwards
    assert np.all(np.isfinite(K))


@pytest.mark.parametrize("tag", ["a", "usps"])
def test_form_knn_graph_equals_the_reference(lib, tag):
    """(n, d, k) = (400, 8, 3), and a USPS-shaped case at d = 256 (grey values in [-1, 1]); tie-free random data."""
    from pygps_amd.GraphExtensions import graphUtil
    g = golden("G25_knn_graphs")
    n, d, k, seed = (int(v) for v in g[tag + "_ndks"])
    pts = np.random.RandomState(seed).randn(n, d)
    if tag == "usps":
        pts = np.tanh(pts)
    A = graphUtil.formKnnGraph(pts, k)
    want = np.zeros((n, n))
    want[g[tag + "_edges"][0], g[tag + "_edges"][1]] = 1.0
    assert A.dtype == np.float64 and np.array_equal(A, want) and np.array_equal(A.sum(axis=0), g[tag + "_degree"])


def test_form_knn_graph_many_coordinates_and_lower_index_wins_a_tie(lib):
    """d = 700 takes two coordinate chunks of the distance kernel; on a regular 1-d grid every inner point has two nearest
    neighbours at the same distance and k = 1 picks the lower index."""
    from pygps_amd.GraphExtensions import graphUtil
    pts = np.random.RandomState(3).randn(150, 700)
    assert np.array_equal(graphUtil.formKnnGraph(pts, 4), graph_cpu.form_knn_graph(pts, 4))
    grid = np.arange(10.0).reshape(10, 1)
    A = graphUtil.formKnnGraph(grid, 1)
    want = np.zeros((10, 10))
    for i in range(10):
        j = 1 if i == 0 else i - 1
        want[i, j] = want[j, i] = 1.0
    assert np.array_equal(A, want)


def test_semi_supervised_flow_end_to_end_with_the_package_alone(lib):
    """Points -> formKnnGraph -> diffKernel -> formKernelMatrix -> cov.Pre -> GPC: the demo's flow with no helper from the
    test tree; equal to the flow through tests/graph_cpu.py."""
    import pygps_amd as pyGPs
    from pygps_amd.GraphExtensions import graphUtil, nodeKernels
    p = graph_cpu.graph_problem(300, 20, 8, 0)
    A = graphUtil.formKnnGraph(p["pts"], 3)
    assert np.array_equal(A, p["A"])
    M1, M2 = graphUtil.formKernelMatrix(nodeKernels.diffKernel(A, 0.5), p["train"], p["test"])
    assert np.max(np.abs(M2 - p["M2"])) <= 1e-13 and np.max(np.abs(M1 - p["M1"])) <= 1e-13
    m = pyGPs.GPC()
    m.setPrior(kernel=pyGPs.cov.Pre(M1, M2) + pyGPs.cov.RBFunit(np.log(2.5)))
    m.setData(p["x"], p["y"])
    ym = m.predict(p["xs"])[0]
    g = golden("G25_pre_fits_N300")
    assert np.max(np.abs(ym - g["sum_ep_pred_ym"])) <= 1e-6 * np.max(np.abs(g["sum_ep_pred_ym"]))
