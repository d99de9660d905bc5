"""numpy restatement of the propagation kernel (reference: pyGPs/GraphExtensions/graphKernels.py:27-184) with a DEFINED order of
arithmetic, the one csrc/propagate.hip follows:

  * the sparse product sums a row's terms in the stored CSR order, multiply then add, from 0.0: a loop over the position within
    the row, vectorised over the rows;
  * the hash dot product sums over j = 0 .. k - 1 in order, multiply then add, from 0.0; then (dot + b) / w, then floor;
  * the counts are integers (scipy.sparse), so K is exact whatever the order.

Draws come from numpy's global stream in the reference's order unless (V, b) are given.  Nothing here imports the package."""
import numpy as np
import scipy.sparse as spsp

SPREAD_ALPHA = 0.8


def to_csr(A):
    if not spsp.issparse(A):
        A = spsp.csr_matrix(np.asarray(A))
    elif not spsp.isspmatrix_csr(A):
        A = A.tocsr()
    return A.astype(float)


def label_setup(l, n):
    """(lab_prob, lab_orig, pushed-back rows) as graphKernels.py:74-91."""
    if spsp.issparse(l):
        l = np.asarray(l.todense())
    l = np.asarray(l)
    if l.shape[1] == 1:
        col = l[:, 0].astype(np.int64)
        k = int(col.max())
        lab = np.zeros((n, k))
        for i in range(n):
            if col[i] > 0:
                lab[i, col[i] - 1] = 1
    else:
        lab = np.array(l, dtype=np.float64)
    orig = lab.copy()
    labelled = np.max(lab, axis=1) == 1
    lab[np.sum(lab, axis=1) == 0, :] = 1. / lab.shape[1]
    return lab, orig, labelled


def operator_entries(A, ktype):
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    row_sums = np.array(A.sum(axis=1))[:, 0]
    if ktype == 'label_spreading':
        d = row_sums ** (-1. / 2)
        return SPREAD_ALPHA * ((d[rows] * A.data) * d[A.indices])
    return A.data / row_sums[rows]


def csr_times_dense(indptr, indices, vals, X):
    """sum_e vals[e] X[indices[e]] per row, terms in stored order, multiply then add."""
    n = len(indptr) - 1
    deg = np.diff(indptr)
    out = np.zeros((n, X.shape[1]))
    for q in range(int(deg.max()) if n else 0):
        rows = np.nonzero(deg > q)[0]
        e = indptr[rows] + q
        out[rows] = out[rows] + vals[e][:, None] * X[indices[e]]
    return out


def draws(k, h_max, w, p):
    V, b = np.empty((h_max + 1, k)), np.empty(h_max + 1)
    for h in range(h_max + 1):
        v = np.random.normal(size=(k, 1))
        if p == 'L1' or p == 'tv':
            v /= np.random.normal(size=(k, 1))
        V[h] = v[:, 0]
        b[h] = w * np.random.rand()
    return V, b


def propagation_cpu(A, l, gr_id, h_max, w, p, ktype=None, SUM=True, V=None, b=None):
    """dict with K (N, N, h_max + 1), lab (the label distributions after the last iteration), V, b, and the two figures that say
    how far the case is from being decided by rounding: edge = the smallest distance, in bins, of any (lab . v + b) / w to an
    integer, max_key = max |key|; distinct = per iteration the largest number of distinct keys within one graph."""
    A = to_csr(A)
    n = A.shape[0]
    g = np.asarray(gr_id).reshape(-1).astype(np.int64)
    N = int(g.max())
    lab, orig, labelled = label_setup(l, n)
    k = lab.shape[1]
    if V is None:
        V, b = draws(k, h_max, w, p)
    vals = operator_entries(A, ktype) if ktype is not None else None
    K = np.empty((N, N, h_max + 1))
    edge, max_key, distinct = np.inf, 0.0, []
    for h in range(h_max + 1):
        if h > 0 and ktype is not None:
            src = lab
            if ktype == 'label_propagation':
                src = lab.copy()
                src[labelled] = orig[labelled]
            lab = csr_times_dense(A.indptr, A.indices, vals, src)
            if ktype == 'label_spreading':
                lab = lab + (1 - SPREAD_ALPHA) * orig
        if p == 'hellinger':
            lab = np.sqrt(lab)
        dot = np.zeros(n)
        for j in range(k):
            dot = dot + lab[:, j] * V[h, j]
        t = (dot + b[h]) / w
        keys = np.floor(t)
        frac = t - keys
        edge = min(edge, float(np.min(np.minimum(frac, 1.0 - frac))))
        max_key = max(max_key, float(np.max(np.abs(keys))))
        uniq, inv = np.unique(keys, return_inverse=True)
        counts = spsp.csr_matrix((np.ones(n, dtype=np.int64), (g - 1, inv.reshape(-1))), shape=(N, len(uniq)))
        distinct.append(int(np.diff(counts.indptr).max()))
        K_h = np.asarray((counts @ counts.T).todense(), dtype=np.float64)
        K[:, :, h] = K_h + K[:, :, h - 1] if (SUM and h > 0) else K_h
    return dict(K=K, lab=lab, V=V, b=b, edge=edge, max_key=max_key, distinct=distinct)


def rounding_bound(A, k, h_max, V, w):
    """The issue's bound on what an unknown summation order can move (dot + b) / w by, in bins:
    eps (k + h_max (maxdeg + 2)) max_h sum_j |v_hj| / w."""
    maxdeg = int(np.diff(to_csr(A).indptr).max())
    return np.finfo(float).eps * (k + h_max * (maxdeg + 2)) * float(np.max(np.sum(np.abs(V), axis=1))) / w


def lower(K):
    """int32 lower triangles of the slices of K, (h_max + 1, N (N + 1) / 2)."""
    i, j = np.tril_indices(K.shape[0])
    out = K[i, j, :].T
    assert np.array_equal(out, np.round(out)) and np.max(np.abs(out)) < 2 ** 31
    return np.ascontiguousarray(out.astype(np.int32))


def from_lower(tri, N):
    i, j = np.tril_indices(N)
    K = np.zeros((N, N, tri.shape[0]))
    K[i, j, :] = tri.T
    K[j, i, :] = tri.T
    return K


def synthetic(sizes, k, seed, extra=1, interleave=False, unlabelled=0.0):
    """Graphs of the given sizes: a ring (a single edge for two nodes, a self-loop for one) plus `extra` random in-graph edges per
    node, symmetric 0 / 1 adjacency; labels 1 .. k drawn uniformly (label k is always present), a fraction set to -1.
    Returns (A csr, l (n, 1) int64, gr_id (n, 1) int64); with `interleave` the nodes are shuffled across graphs."""
    rng = np.random.RandomState(seed)
    sizes = np.asarray(sizes)
    n = int(sizes.sum())
    start = np.concatenate([[0], np.cumsum(sizes)])
    ii, jj = [], []
    for gi, m in enumerate(sizes):
        s = start[gi]
        a = np.arange(m)
        ii.append(s + a)
        jj.append(s + (a + 1) % m)
        if m > 2 and extra:
            ii.append(s + np.repeat(a, extra))
            jj.append(s + rng.randint(0, m, m * extra))
    ii, jj = np.concatenate(ii), np.concatenate(jj)
    A = spsp.coo_matrix((np.ones(len(ii)), (ii, jj)), shape=(n, n)).tocsr()
    A = ((A + A.T) > 0).astype(float).tocsr()
    l = rng.randint(1, k + 1, (n, 1)).astype(np.int64)
    l[rng.randint(0, n), 0] = k
    if unlabelled:
        mask = rng.rand(n) < unlabelled
        keep = np.argmax(l[:, 0] == k)
        mask[keep] = False
        l[mask, 0] = -1
    gr = np.repeat(np.arange(1, len(sizes) + 1), sizes).reshape(-1, 1).astype(np.int64)
    if interleave:
        order = rng.permutation(n)
        A = A[order][:, order].tocsr()
        l, gr = l[order], gr[order]
    return A, l, gr
