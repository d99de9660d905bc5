"""GPU: pygps_amd.GraphExtensions.graphKernels.propagationKernel (pgp_propagation_kernel, csrc/propagate.hip) against the G26
fixtures recorded from the reference and against the numpy restatement tests/propagation_cpu.py.

Kernel matrices are compared with np.array_equal: every entry is an integer count and every floating-point step of the device
code has a defined order (the restatement's), so there is nothing to tolerate.  The label distributions after the last iteration
are compared bit for bit as well, p = 'hellinger' included: the bound foreseen for it was 1e-14 relative (one ulp per square root,
h_max + 1 <= 7 of them carried through convex combinations), but the device's square root (__dsqrt_rn) is correctly rounded --
the largest difference measured on an MI355X over every Hellinger case here was 0 -- so the check is equality."""
import numpy as np
import pytest
import scipy.sparse as spsp

import propagation_cpu as P
from conftest import golden
from test_propagation_host import W, case_labels, case_list, check_summary, mutag_inputs

pytestmark = pytest.mark.gpu


def both(A, l, gr, h_max, w, p, ktype, SUM=True, seed=0):
    """(K of the package, its final label distributions, the restatement's dict) from the same seed."""
    from pygps_amd.GraphExtensions import graphKernels
    np.random.seed(seed)
    K, lab, _ = graphKernels._propagation(A, l, gr, h_max, w, p, ktype, SUM, want_lab=True)
    np.random.seed(seed)
    r = P.propagation_cpu(A, l, gr, h_max, w, p, ktype, SUM)
    return K, lab, r


def check_against_restatement(K, lab, r, p):
    assert K.dtype == np.float64 and K.flags["C_CONTIGUOUS"] and K.shape == r["K"].shape
    assert np.array_equal(K, r["K"])
    if p == "hellinger":
        err = np.max(np.abs(lab - r["lab"]) / np.maximum(np.abs(r["lab"]), 1e-300))
        print("hellinger: max relative difference of the final label distributions %.3g" % err)
    assert np.array_equal(lab, r["lab"])


# ----------------------------------------------------------------------------------------------------- fixtures
def test_demo_configuration_equals_the_reference():
    A, l, gr, _ = mutag_inputs()
    g = golden("G26_demo_K")
    K, lab, r = both(A, l, gr, 10, W, "tv", "label_diffusion", seed=int(g["seed"]))
    assert np.array_equal(P.lower(K), g["tri"])
    check_against_restatement(K, lab, r, "tv")


@pytest.mark.parametrize("tag,form,h_max,p,ktype", case_list())
def test_case_fixtures_equal_the_reference(tag, form, h_max, p, ktype):
    A, _, gr, _ = mutag_inputs()
    K, lab, r = both(A, case_labels(form), gr, h_max, W, p, ktype, seed=int(golden("G26_cases")[tag + "_seed"]))
    check_summary(K, tag)
    check_against_restatement(K, lab, r, p)


def test_label_spreading_equals_the_restatement():
    A, l, gr, _ = mutag_inputs()
    K, lab, r = both(A, case_labels("partial"), gr, 3, W, "tv", "label_spreading", seed=5)
    check_against_restatement(K, lab, r, "tv")
    assert K[:, :, 3].sum() > K[:, :, 0].sum()


# ----------------------------------------------------------------------------------------------------- shapes
def sizes_for(N, seed):
    return np.random.RandomState(seed).randint(1, 10, N)


SHAPES = {
    # name: (sizes, k, synthetic kwargs, h_max, w, p, ktype, SUM)
    "one_graph": ([7], 3, {}, 3, 1e-3, "tv", "label_diffusion", True),
    "N17": (sizes_for(17, 1), 3, {}, 3, 1e-3, "tv", "label_propagation", True),
    "N129": (sizes_for(129, 2), 4, dict(unlabelled=0.3), 3, 1e-3, "L2", "label_propagation", True),
    "single_nodes": ([1] * 21, 3, {}, 2, 1e-3, "L1", "label_diffusion", True),
    "interleaved": (sizes_for(40, 3), 3, dict(interleave=True, unlabelled=0.2), 3, 1e-3, "hellinger", "label_propagation", True),
    "k2": (sizes_for(33, 4), 2, {}, 3, 1e-3, "tv", "label_diffusion", True),
    "k256": ([40] * 12, 256, {}, 2, 1e-3, "L2", "label_diffusion", True),
    "h0": (sizes_for(20, 5), 3, {}, 0, 1e-3, "tv", "label_diffusion", True),
    "no_sum": (sizes_for(20, 6), 3, {}, 4, 1e-3, "tv", "label_diffusion", False),
    "no_update": (sizes_for(20, 7), 3, dict(unlabelled=0.5), 2, 1e-3, "L2", None, True),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_small_shapes_equal_the_restatement(name):
    sizes, k, kw, h_max, w, p, ktype, SUM = SHAPES[name]
    A, l, gr = P.synthetic(sizes, k, 11, **kw)
    K, lab, r = both(A, l, gr, h_max, w, p, ktype, SUM, seed=3)
    assert K.shape == (len(sizes), len(sizes), h_max + 1)
    check_against_restatement(K, lab, r, p)


def test_a_graph_beyond_the_on_chip_limits_beside_short_ones():
    """One graph with more nodes than the LDS sort takes and more distinct keys than a Gram tile holds, between short graphs:
    the global-memory sort and the global-memory merge, and the tiles that mix both."""
    from pygps_amd.GraphExtensions import graphKernels
    long_graph = 2 * max(graphKernels.SORT_LDS_MAX, graphKernels.GRAM_LDS_MAX)
    sizes = [5] * 20 + [long_graph] + [6] * 19 + [graphKernels.SORT_LDS_MAX, graphKernels.SORT_LDS_MAX + 1]
    A, l, gr = P.synthetic(sizes, 4, 12, extra=2)
    K, lab, r = both(A, l, gr, 4, 1e-6, "tv", "label_diffusion", seed=3)
    assert max(r["distinct"]) > graphKernels.GRAM_LDS_MAX and min(r["distinct"]) <= 4
    check_against_restatement(K, lab, r, "tv")


def test_dense_and_unsorted_adjacency():
    A, l, gr = P.synthetic(sizes_for(25, 8), 3, 13, extra=2)
    K, lab, r = both(A, l, gr, 3, 1e-3, "tv", "label_diffusion", seed=3)
    Kd, labd, _ = both(A.toarray(), l, gr, 3, 1e-3, "tv", "label_diffusion", seed=3)
    assert np.array_equal(K, Kd) and np.array_equal(lab, labd)
    # the same matrix with every row's entries stored in descending column order: the sums run in THAT order
    indptr, indices, data = A.indptr, A.indices.copy(), A.data.copy()
    for i in range(A.shape[0]):
        indices[indptr[i]:indptr[i + 1]] = indices[indptr[i]:indptr[i + 1]][::-1]
    U = spsp.csr_matrix((data, indices, indptr), shape=A.shape)
    assert not U.has_sorted_indices
    Ku, labu, ru = both(U, l, gr, 3, 1e-3, "tv", "label_diffusion", seed=3)
    check_against_restatement(Ku, labu, ru, "tv")
    assert not U.has_sorted_indices


# ----------------------------------------------------------------------------------------------------- state
def small_fit():
    import pygps_amd as pyGPs
    rng = np.random.RandomState(0)
    x = rng.randn(200, 3)
    y = np.sin(x.sum(axis=1, keepdims=True)) + 0.1 * rng.randn(200, 1)
    m = pyGPs.GPR()
    m.setPrior(kernel=pyGPs.cov.RBF(np.log(2.0), 0.1))
    m.setData(x, y)
    return m


def test_calls_repeat_and_leave_a_resident_fit_alone():
    """Same seed, same bytes; and a model whose data is resident on the context gives the same nlZ after the calls as before them,
    as does a model set up afresh."""
    from pygps_amd.GraphExtensions import graphKernels
    A, l, gr = P.synthetic(sizes_for(30, 9), 3, 14)
    m = small_fit()
    before = m.getPosterior()[0]
    out = []
    for _ in range(2):
        np.random.seed(8)
        out.append(graphKernels.propagationKernel(A, l, gr, 3, 1e-3, "tv", "label_diffusion"))
    assert out[0].tobytes() == out[1].tobytes()
    assert m.getPosterior()[0] == before and small_fit().getPosterior()[0] == before


def test_non_finite_key_is_a_value_error_and_the_context_survives(monkeypatch):
    from pygps_amd.GraphExtensions import graphKernels
    A, l, gr = P.synthetic(sizes_for(30, 9), 3, 14)
    real = np.random.normal

    def poisoned(*a, **kw):
        v = real(*a, **kw)
        v.flat[0] = np.inf
        return v
    np.random.seed(8)
    monkeypatch.setattr(np.random, "normal", poisoned)
    with pytest.raises(ValueError, match="not finite"):
        graphKernels.propagationKernel(A, l, gr, 2, 1e-3, "L2", "label_diffusion")
    monkeypatch.setattr(np.random, "normal", real)
    K, lab, r = both(A, l, gr, 2, 1e-3, "L2", "label_diffusion", seed=8)
    check_against_restatement(K, lab, r, "L2")


# ----------------------------------------------------------------------------------------------------- the demo's flow
def test_demo_flow_one_fold_with_the_package_alone():
    """demo_GraphKernel.py on MUTAG with the package alone: propagationKernel -> formKernelMatrix -> cov.Pre -> GPC (EP) -> predict,
    one fold (test graphs 0, 10, 20, ...) on slice 10, against the reference's run of the same fold."""
    import pygps_amd as pyGPs
    from pygps_amd.GraphExtensions import graphUtil, graphKernels
    A, l, gr, graph_label = mutag_inputs()
    np.random.seed(1)
    K = graphKernels.propagationKernel(A, l, gr, 10, W, "tv", "label_diffusion", SUM=True, VIS=False, showEachStep=False)
    assert np.array_equal(P.lower(K), golden("G26_demo_K")["tri"])
    g = golden("G26_demo_fold")
    y = np.where(graph_label == 0, -1, graph_label).astype(np.int8)
    M1, M2 = graphUtil.formKernelMatrix(K[:, :, 10], g["train"], g["test"])
    model = pyGPs.GPC()
    model.setPrior(kernel=pyGPs.cov.Pre(M1, M2))
    nlZ = model.getPosterior(np.zeros((len(g["train"]), 1)), y[g["train"], :])[0]
    ym = model.predict(np.zeros((len(g["test"]), 1)))[0]
    assert abs(nlZ - float(g["nlZ"])) <= 1e-6 * abs(float(g["nlZ"]))
    assert np.max(np.abs(ym - g["ym"])) <= 1e-6 * np.max(np.abs(g["ym"]))
    assert np.mean(np.sign(ym) == y[g["test"], :]) == float(g["accuracy"])


def test_inconsistent_index_arrays_are_refused_by_the_library():
    """What a kernel would index with is checked on the host side of the C call: a column index past n, row pointers that
    decrease, a grouping that is no permutation or whose segments do not cover it all answer an argument error."""
    from pygps_amd import _lib
    from pygps_amd.GraphExtensions import graphKernels
    A, l, gr = P.synthetic(sizes_for(12, 2), 3, 15)
    A = P.to_csr(A)
    n = A.shape[0]
    lab, orig, push_back = graphKernels._labels(l, n)
    N, perm, seg = graphKernels._graphs(gr, n)
    vals = graphKernels._operator(A, "label_diffusion")
    V, b = P.draws(3, 1, 1e-3, "L2")

    def call(A=A, perm=perm, seg=seg):
        return graphKernels._device(n, 3, N, A, vals, lab, None, None, perm, seg, 1, V, b, 1e-3, _lib.PROP_T, 0.0, False, True)
    good = call()[0]
    bad_cols = A.copy()
    bad_cols.indices[3] = n
    bad_rows = A.copy()
    bad_rows.indptr[2] = bad_rows.indptr[3] + 1
    twice = perm.copy()
    twice[1] = twice[0]
    short = seg.copy()
    short[-1] = n - 1
    for kw in (dict(A=bad_cols), dict(A=bad_rows), dict(perm=twice), dict(seg=short)):
        with pytest.raises(ValueError, match="inconsistent"):
            call(**kw)
    assert np.array_equal(call()[0], good)
