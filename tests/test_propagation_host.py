"""CPU: the numpy restatement of the propagation kernel (tests/propagation_cpu.py) reproduces every G26 fixture recorded from
the reference exactly, and the host side of pygps_amd.GraphExtensions.graphKernels -- argument rules, grouping, the order of
the random draws -- behaves as documented without touching the device."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as spsp

from conftest import ROOT, golden
import propagation_cpu as P

W = 1e-4


def mutag_inputs():
    d = golden("G26_mutag")
    A = spsp.csc_matrix((d["adj_data"], d["adj_indice"], d["adj_indptr"]), shape=d["adj_shape"])
    return A, d["responses"], d["graph_ind"], d["labels"]


def label_matrix(l):
    k = int(l.max())
    M = np.zeros((l.shape[0], k))
    on = np.nonzero(l[:, 0] > 0)[0]
    M[on, l[on, 0] - 1] = 1
    return M


def case_list():
    """(tag, labels form, h_max, p, ktype) of the cases (b), (c), (d) in G26_cases."""
    out = []
    for ktype in ("label_diffusion", "label_propagation"):
        for p in ("tv", "hellinger", "L2"):
            out.append(("b_%s_%s" % (ktype, p), "full", 4, p, ktype))
        out.append(("c_%s" % ktype, "partial", 6, "tv", ktype))
        out.append(("d_%s" % ktype, "matrix", 6, "tv", ktype))
    return out


def case_labels(form):
    A, l, gr, _ = mutag_inputs()
    if form == "full":
        return l
    lp = golden("G26_cases")["c_labels"]
    return lp if form == "partial" else label_matrix(lp)


def check_summary(K, tag):
    """K (N, N, h_max + 1) against the stored last slice and the per-slice sum, trace and K_h u: exact."""
    g = golden("G26_cases")
    u = g["u"].astype(float)
    assert K.shape[2] == int(g[tag + "_h_max"]) + 1
    assert np.array_equal(P.lower(K[:, :, -1:])[0], g[tag + "_last"])
    assert np.array_equal(K.sum(axis=(0, 1)), g[tag + "_sums"])
    assert np.array_equal(np.trace(K, axis1=0, axis2=1), g[tag + "_traces"])
    assert np.array_equal(np.einsum("ijh,j->hi", K, u), g[tag + "_Ku"])
    assert np.array_equal(K, np.transpose(K, (1, 0, 2)))


def test_restatement_reproduces_the_demo_fixture():
    A, l, gr, _ = mutag_inputs()
    g = golden("G26_demo_K")
    np.random.seed(int(g["seed"]))
    r = P.propagation_cpu(A, l, gr, int(g["h_max"]), float(g["w"]), "tv", "label_diffusion")
    assert np.array_equal(P.lower(r["K"]), g["tri"])
    assert np.array_equal(r["V"], g["V"]) and np.array_equal(r["b"], g["b"])
    assert r["edge"] == float(g["edge"]) and r["edge"] >= 100 * P.rounding_bound(A, 7, 10, r["V"], W)


@pytest.mark.parametrize("tag,form,h_max,p,ktype", case_list())
def test_restatement_reproduces_the_case_fixtures(tag, form, h_max, p, ktype):
    A, _, gr, _ = mutag_inputs()
    g = golden("G26_cases")
    np.random.seed(int(g[tag + "_seed"]))
    r = P.propagation_cpu(A, case_labels(form), gr, h_max, W, p, ktype)
    check_summary(r["K"], tag)
    assert r["edge"] == float(g[tag + "_edge"]) and r["edge"] >= 100 * float(g[tag + "_bound"])


def test_restatement_counts_node_pairs():
    """K_h against its definition, pair by pair, on a case small enough for the double loop."""
    A, l, gr = P.synthetic([3, 1, 5, 2], 3, 0)
    np.random.seed(4)
    r = P.propagation_cpu(A, l, gr, 1, 0.05, "L2", "label_diffusion", SUM=False)
    lab = P.label_setup(l, A.shape[0])[0]
    D = A.toarray()
    lab1 = (D / D.sum(axis=1, keepdims=True)) @ lab
    assert r["edge"] > 1e-9                             # (so the order of the dense product here cannot move a key)
    for h, X in enumerate((lab, lab1)):
        keys = np.floor((X @ r["V"][h] + r["b"][h]) / 0.05)
        want = np.zeros((4, 4))
        for i in range(len(keys)):
            for j in range(len(keys)):
                want[gr[i, 0] - 1, gr[j, 0] - 1] += keys[i] == keys[j]
        assert np.array_equal(r["K"][:, :, h], want)


# ----------------------------------------------------------------------------------------------------- host rules of the package
def small():
    return P.synthetic([4, 3, 5], 3, 1)


def test_module_is_exported_and_limits_match_the_header():
    from pygps_amd.GraphExtensions import graphKernels
    from pygps_amd import GraphExtensions, _lib
    assert GraphExtensions.graphKernels is graphKernels
    src = open(os.path.join(ROOT, "include", "pygps_amd.h")).read()
    for name, value in (("PGP_PROP_MAX_LABELS", graphKernels.MAX_LABELS), ("PGP_PROP_SORT_LDS", graphKernels.SORT_LDS_MAX),
                        ("PGP_PROP_GRAM_LDS", graphKernels.GRAM_LDS_MAX), ("PGP_PROP_NONE", _lib.PROP_NONE),
                        ("PGP_PROP_T", _lib.PROP_T), ("PGP_PROP_SPREAD", _lib.PROP_SPREAD)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, src).group(1)) == value, name
    assert int(re.search(r"#define PGP_ERR_PROP_NONFINITE\s+\((-\d+)\)", src).group(1)) == _lib.ERR_PROP_NONFINITE
    assert graphKernels.MAX_LABELS == 256


@pytest.fixture
def stubbed(monkeypatch):
    """graphKernels with the device call replaced by a recorder: everything up to the call runs, nothing touches the device."""
    from pygps_amd.GraphExtensions import graphKernels
    calls = []

    def fake(n, k, N, A, vals, lab, orig, push_back, perm, seg, h_max, V, b, w, update, orig_weight, take_sqrt, SUM,
             want_lab=False, want_stages=False):
        calls.append(dict(n=n, k=k, N=N, A=A, vals=vals, lab=lab, orig=orig, push_back=push_back, perm=perm, seg=seg, h_max=h_max,
                          V=V, b=b, w=w, update=update, orig_weight=orig_weight, take_sqrt=take_sqrt, SUM=SUM))
        return np.zeros((N, N, h_max + 1)), None, None
    monkeypatch.setattr(graphKernels, "_device", fake)
    graphKernels.calls = calls
    return graphKernels


def test_isolated_node_is_refused(stubbed):
    A, l, gr = small()
    A = A.tolil()
    A[2, :] = 0
    A[:, 2] = 0
    with pytest.raises(ValueError, match="isolated node"):
        stubbed.propagationKernel(A.tocsr(), l, gr, 2, W, "tv", "label_diffusion")
    assert not stubbed.calls


def test_label_count_limits(stubbed):
    A, l, gr = small()
    with pytest.raises(ValueError, match="2 <= number of labels <= 256"):
        stubbed.propagationKernel(A, np.ones_like(l), gr, 1, W, "tv", "label_diffusion")
    with pytest.raises(ValueError, match="2 <= number of labels <= 256"):
        stubbed.propagationKernel(A, np.ones((A.shape[0], 257)) / 257, gr, 1, W, "tv", "label_diffusion")
    big = l.copy()
    big[0, 0] = 257
    with pytest.raises(ValueError, match="2 <= number of labels <= 256"):
        stubbed.propagationKernel(A, big, gr, 1, W, "tv", "label_diffusion")
    big[0, 0] = 256
    stubbed.propagationKernel(A, big, gr, 1, W, "tv", "label_diffusion")
    assert stubbed.calls[-1]["k"] == 256


@pytest.mark.parametrize("bad", ["zero", "negative", "fraction", "short", "too_many"])
def test_bad_graph_ids_are_refused(stubbed, bad):
    A, l, gr = small()
    gr = gr.astype(float)
    if bad == "zero":
        gr[0, 0] = 0
    elif bad == "negative":
        gr[1, 0] = -2
    elif bad == "fraction":
        gr[1, 0] = 1.5
    elif bad == "short":
        gr = gr[:-1]
    else:
        gr[0, 0] = A.shape[0] + 1
    with pytest.raises(ValueError):
        stubbed.propagationKernel(A, l, gr, 1, W, "tv", "label_diffusion")
    assert not stubbed.calls


def test_unknown_ktype_is_refused(stubbed):
    A, l, gr = small()
    for ktype in ("belief_propagation", "diffusion", ""):
        with pytest.raises(ValueError, match="unknown ktype"):
            stubbed.propagationKernel(A, l, gr, 1, W, "tv", ktype)
    assert not stubbed.calls


def test_float_graph_ids_and_any_matrix_form_are_accepted(stubbed):
    A, l, gr = small()
    stubbed.propagationKernel(A, l, gr, 1, W, "tv", "label_diffusion")
    stubbed.propagationKernel(A.tocsc(), l.astype(np.uint8), gr.astype(float), 1, W, "tv", "label_diffusion")
    stubbed.propagationKernel(A.toarray(), l, gr, 1, W, "tv", "label_diffusion")
    a, b, c = stubbed.calls
    for other in (b, c):
        for key in ("vals", "lab", "perm", "seg"):
            assert np.array_equal(a[key], other[key]), key
        assert np.array_equal(a["A"].indices, other["A"].indices) and other["N"] == 3 and other["k"] == 3


def test_grouping_is_stable_and_handles_interleaved_graphs(stubbed):
    A, l, gr = P.synthetic([4, 3, 5], 3, 1, interleave=True)
    stubbed.propagationKernel(A, l, gr, 0, W, "L2", None)
    c = stubbed.calls[0]
    g = gr[:, 0]
    assert sorted(c["perm"].tolist()) == list(range(12)) and c["seg"].tolist() == [0, 4, 7, 12]
    for q in range(3):
        mine = c["perm"][c["seg"][q]:c["seg"][q + 1]]
        assert np.all(g[mine] == q + 1) and np.all(np.diff(mine) > 0)
    assert c["update"] == 0 and c["vals"] is None and c["orig"] is None and c["push_back"] is None


def test_host_values_are_the_restatements(stubbed):
    """T.data, the entries of 0.8 S, the 1 / k rows, lab_orig and the pushed-back rows: bit for bit those of the restatement."""
    A, l, gr = P.synthetic([6, 5, 7], 4, 2, unlabelled=0.4)
    lab, orig, labelled = P.label_setup(l, A.shape[0])
    for ktype, update in (("label_diffusion", 1), ("label_propagation", 1), ("label_spreading", 2)):
        stubbed.propagationKernel(A, l, gr, 2, W, "hellinger", ktype)
        c = stubbed.calls[-1]
        assert np.array_equal(c["vals"], P.operator_entries(P.to_csr(A), ktype)) and c["update"] == update and c["take_sqrt"]
        assert np.array_equal(c["lab"], lab) and np.any(lab == 0.25)
        if ktype == "label_diffusion":
            assert c["orig"] is None and c["push_back"] is None
        else:
            assert np.array_equal(c["orig"], orig) and np.any(orig.sum(axis=1) == 0)
        if ktype == "label_propagation":
            assert np.array_equal(c["push_back"].astype(bool), labelled)
        if ktype == "label_spreading":
            assert c["push_back"] is None and c["orig_weight"] == 1 - 0.8


@pytest.mark.parametrize("p", ["tv", "L1", "hellinger", "L2"])
def test_random_draws_follow_the_reference_order(stubbed, p):
    A, l, gr = small()
    h_max, k = 3, 3
    np.random.seed(11)
    stubbed.propagationKernel(A, l, gr, h_max, W, p, "label_diffusion")
    after = np.random.get_state()
    np.random.seed(11)
    V, b = np.empty((h_max + 1, k)), np.empty(h_max + 1)
    for h in range(h_max + 1):
        v = np.random.normal(size=(k, 1))
        if p in ("tv", "L1"):
            v /= np.random.normal(size=(k, 1))
        V[h], b[h] = v[:, 0], W * np.random.rand()
    by_hand = np.random.get_state()
    assert after[0] == by_hand[0] and np.array_equal(after[1], by_hand[1]) and after[2:] == by_hand[2:]
    c = stubbed.calls[0]
    assert np.array_equal(c["V"], V) and np.array_equal(c["b"], b)
