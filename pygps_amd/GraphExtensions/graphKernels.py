"""Kernels between whole graphs (reference: pyGPs/GraphExtensions/graphKernels.py): the propagation kernel of Neumann,
Patricia, Garnett, Kersting, "Efficient Graph Kernels by Randomization", ECML/PKDD 2012.

Index work and O(nnz) arithmetic (the CSR form of the adjacency matrix, its row normalisation, the grouping of the nodes by
graph, all random draws) run on the host in numpy; the iterations -- sparse times dense, hashing, per-graph sorting, the Gram
product of the count vectors -- run on the device in one call (``pgp_propagation_kernel``, csrc/propagate.hip).  There is no
CPU fallback."""
import ctypes as C
import logging

import numpy as np
import scipy.sparse as spsp

from .. import _lib

MAX_LABELS = _lib.PROP_MAX_LABELS     # label classes the device call takes
SORT_LDS_MAX = _lib.PROP_SORT_LDS     # nodes of one graph whose keys are sorted on chip; longer graphs sort in global memory
GRAM_LDS_MAX = _lib.PROP_GRAM_LDS     # (key, count) pairs of a tile of 32 graphs held on chip; larger tiles read global memory
KTYPES = ('label_diffusion', 'label_propagation', 'label_spreading', None)
SPREAD_ALPHA = 0.8

_ARG_MESSAGES = {
    -2: "pygps_amd: propagationKernel needs at least one node (and fewer than 2^31)",
    -3: "pygps_amd: propagationKernel needs 2 <= number of labels <= %d" % MAX_LABELS,
    -4: "pygps_amd: propagationKernel: the number of graphs must lie in 1 .. number of nodes",
    -6: "pygps_amd: propagationKernel: inconsistent CSR arrays",
    -9: "pygps_amd: propagationKernel: the grouping of the nodes by graph is inconsistent",
    -12: "pygps_amd: propagationKernel: the bin width w must be positive and finite",
}


def _csr(A):
    """A as CSR float64, stored entries in the order they have (no sorting, no merging of duplicates)."""
    if not spsp.issparse(A):
        A = spsp.csr_matrix(np.asarray(A))
    elif not spsp.isspmatrix_csr(A):
        A = A.tocsr()
    A = A.astype(float)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("pygps_amd: the adjacency matrix must be square, got shape %s" % (A.shape,))
    return A


def _labels(l, n):
    """(lab_prob, lab_orig, push_back): graphKernels.py:74-91.  lab_orig is taken BEFORE the all-zero rows become 1 / k, so those
    rows of lab_orig stay zero; push_back marks the rows whose original maximum is 1."""
    if spsp.issparse(l):
        l = np.asarray(l.todense())
    l = np.asarray(l)
    if l.ndim == 1:
        l = l.reshape(-1, 1)
    if l.ndim != 2 or l.shape[0] != n:
        raise ValueError("pygps_amd: the labels must have one row per node (%d), got shape %s" % (n, l.shape))
    if l.shape[1] == 1:
        col = l[:, 0]
        if not np.all(np.isfinite(col)) or np.any(col != np.floor(col)):
            raise ValueError("pygps_amd: node labels must be integers (1 .. k, <= 0 for unlabelled nodes)")
        col = col.astype(np.int64)
        k = int(col.max()) if n else 0
        if k < 2 or k > MAX_LABELS:
            raise ValueError("pygps_amd: propagationKernel needs 2 <= number of labels <= %d, got %d" % (MAX_LABELS, k))
        lab = np.zeros((n, k), dtype=np.float64)
        on = np.nonzero(col > 0)[0]
        lab[on, col[on] - 1] = 1
    else:
        k = l.shape[1]
        if k > MAX_LABELS:
            raise ValueError("pygps_amd: propagationKernel needs 2 <= number of labels <= %d, got %d" % (MAX_LABELS, k))
        lab = np.array(l, dtype=np.float64)
    orig = lab.copy()
    push_back = (np.max(lab, axis=1) == 1).astype(np.uint8)
    unif = np.nonzero(np.sum(lab, axis=1) == 0)[0]
    if unif.shape[0] != 0:
        lab[unif, :] = 1. / k
    return lab, orig, push_back


def _graphs(gr_id, n):
    """(N, perm, seg): ids 1 .. N (integer-valued floats accepted); perm lists the nodes grouped by graph, each graph's nodes in
    their input order (a stable sort), graph g owning perm[seg[g] : seg[g + 1]]."""
    g = np.asarray(gr_id).reshape(-1)
    if g.shape[0] != n:
        raise ValueError("pygps_amd: gr_id must have one entry per node (%d), got %d" % (n, g.shape[0]))
    if not np.all(np.isfinite(g)) or np.any(g != np.floor(g)):
        raise ValueError("pygps_amd: graph ids must be integers")
    g = g.astype(np.int64)
    if n == 0 or g.min() < 1:
        raise ValueError("pygps_amd: graph ids must lie in 1 .. N")
    N = int(g.max())
    if N > n:
        raise ValueError("pygps_amd: graph ids must lie in 1 .. N with N <= number of nodes, got %d" % N)
    perm = np.argsort(g, kind='stable').astype(np.int32)
    seg = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(g - 1, minlength=N), out=seg[1:])
    return N, perm, seg


def _operator(A, ktype):
    """Entries (in A's stored order) of the matrix the update applies: T = A with each row divided by its sum
    (graphKernels.py:93-96), or SPREAD_ALPHA * D^-1/2 A D^-1/2 for 'label_spreading' (graphKernels.py:118-125)."""
    n = A.shape[0]
    counts = np.diff(A.indptr)
    if np.any(counts == 0):
        raise ValueError("pygps_amd: isolated node (row %d of the adjacency matrix has no entries)" % int(np.argmin(counts != 0)))
    rows = np.repeat(np.arange(n), counts)
    row_sums = np.array(A.sum(axis=1))[:, 0]
    if ktype == 'label_spreading':
        d = row_sums ** (-1. / 2)
        return SPREAD_ALPHA * ((d[rows] * A.data) * d[A.indices])
    return A.data / row_sums[rows]


def _draws(k, h_max, w, p):
    """The reference's draws from numpy's global stream, in its order (graphKernels.py:136-141): per iteration normal(k), for
    'L1' / 'tv' a second normal(k) that divides the first, then rand() for the offset."""
    V = np.empty((h_max + 1, k))
    b = np.empty(h_max + 1)
    for h in range(h_max + 1):
        v = np.random.normal(size=(k, 1))
        if p == 'L1' or p == 'tv':
            v /= np.random.normal(size=(k, 1))
        V[h] = v[:, 0]
        b[h] = w * np.random.rand()
    return V, b


def _device(n, k, N, A, vals, lab, orig, push_back, perm, seg, h_max, V, b, w, update, orig_weight, take_sqrt, SUM,
            want_lab=False, want_stages=False):
    """One call of pgp_propagation_kernel.  Returns (K, lab after the last iteration or None, stage times or None)."""
    K = np.empty((N, N, h_max + 1))
    lab_out = np.empty((n, k)) if want_lab else None
    stages = np.zeros(len(_lib.PROP_STAGES)) if want_stages else None
    i64p, i32p, u8p = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    if update != _lib.PROP_NONE:
        indptr = np.ascontiguousarray(A.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(A.indices, dtype=np.int32)
        vals = _lib.f64(vals)
        csr = (indptr.ctypes.data_as(i64p), indices.ctypes.data_as(i32p), _lib.ptr(vals))
    else:
        csr = (None, None, None)
    lab, V, b = _lib.f64(lab), _lib.f64(V), _lib.f64(b)
    orig = None if orig is None else _lib.f64(orig)
    push_back = None if push_back is None else np.ascontiguousarray(push_back, dtype=np.uint8)
    perm = np.ascontiguousarray(perm, dtype=np.int32)
    seg = np.ascontiguousarray(seg, dtype=np.int64)
    rc = _lib.load().pgp_propagation_kernel(
        _lib.ctx(), n, k, N, csr[0], csr[1], csr[2], _lib.ptr(lab), _lib.ptr(orig),
        None if push_back is None else push_back.ctypes.data_as(u8p), perm.ctypes.data_as(i32p), seg.ctypes.data_as(i64p),
        int(h_max), _lib.ptr(V), _lib.ptr(b), float(w), int(update), float(orig_weight), int(bool(take_sqrt)), int(bool(SUM)),
        _lib.ptr(K), _lib.ptr(lab_out), _lib.ptr(stages))
    if rc == _lib.ERR_PROP_NONFINITE:
        raise ValueError("pygps_amd: propagationKernel: a hash key is not finite (a projection entry overflowed, or a Cauchy draw "
                         "was divided by zero); use a larger bin width w or another seed")
    if rc in _ARG_MESSAGES:
        raise ValueError(_ARG_MESSAGES[rc])
    _lib.check(rc, "pgp_propagation_kernel")
    return K, lab_out, stages


def _propagation(A, l, gr_id, h_max, w, p, ktype, SUM, want_lab=False, want_stages=False):
    if ktype not in KTYPES:
        raise ValueError("pygps_amd: unknown ktype %r (known: 'label_diffusion', 'label_propagation', 'label_spreading', None)"
                         % (ktype,))
    h_max = int(h_max)
    if h_max < 0:
        raise ValueError("pygps_amd: h_max must be >= 0")
    if not (w > 0 and np.isfinite(w)):
        raise ValueError(_ARG_MESSAGES[-12])
    A = _csr(A)
    n = A.shape[0]
    lab, orig, push_back = _labels(l, n)
    k = lab.shape[1]
    if k < 2:
        raise ValueError("pygps_amd: propagationKernel needs 2 <= number of labels <= %d, got %d" % (MAX_LABELS, k))
    N, perm, seg = _graphs(gr_id, n)
    vals, update, orig_weight = None, _lib.PROP_NONE, 0.0
    if ktype is not None:
        vals = _operator(A, ktype)
        update = _lib.PROP_SPREAD if ktype == 'label_spreading' else _lib.PROP_T
        if ktype == 'label_spreading':
            orig_weight = 1 - SPREAD_ALPHA
    if ktype != 'label_propagation':
        push_back = None
    if ktype not in ('label_propagation', 'label_spreading'):
        orig = None
    V, b = _draws(k, h_max, w, p)
    return _device(n, k, N, A, vals, lab, orig, push_back, perm, seg, h_max, V, b, w, update, orig_weight, p == 'hellinger', SUM,
                   want_lab, want_stages)


def propagationKernel(A, l, gr_id, h_max, w, p, ktype=None, SUM=True, VIS=False, showEachStep=False):
    '''
    Propagation kernel for graphs as described in:
    Neumann, M., Patricia, N., Garnett, R., Kersting, K.: Efficient Graph Kernels by
    Randomization. In: P.A. Flach, T.D. Bie, N. Cristianini (eds.) ECML/PKDD, Notes in
    Computer Science, vol. 7523, pp. 378-393. Springer (2012).

    :param A: adjacency matrix (num_nodes x num_nodes), dense or any scipy.sparse matrix; no row without entries
    :param l: label array (num_nodes x 1); values [1,...,k], values <= 0 for unlabeled nodes
              OR label array (num_nodes x num_labels); values [0,1], unlabeled nodes have only 0 entries.  2 <= k <= 256
    :param gr_id: graph indicator array (num_nodes x 1); values [1,..,N] (integer-valued floats accepted); the nodes of a
                  graph need not be contiguous
    :param h_max: number of iterations
    :param w: bin widths parameter
    :param p: distance ('tv', 'hellinger', 'L1', 'L2')
    :param ktype: type of propagation kernel ['label_diffusion', 'label_propagation', 'label_spreading', None]

    :return: kernel matrix (N x N x (h_max + 1)), float64 with integer entries; slice h is the sum of the contributions
             of iterations 0..h with SUM, else the contribution of iteration h alone

    Every random draw comes from numpy's global stream in the reference's order, so after ``np.random.seed(s)`` the
    projections are the reference's.  With p == 'hellinger' the square root is taken of the label distributions in place
    in every iteration and therefore carries into the next update, exactly as in the reference (graphKernels.py:133-134).
    Departures from the reference: an isolated node, an unknown ktype and a hash key that is not finite raise ValueError
    (the reference yields NaNs, silently propagates nothing, or fails in numpy); 'label_spreading' works.
    '''
    log = logging.getLogger(__name__)
    K, _, _ = _propagation(A, l, gr_id, h_max, w, p, ktype, SUM)
    if showEachStep:
        for h in range(K.shape[2]):
            log.info('ITERATION: ' + str(h))
            log.info(str(K[:, :, h]))
    if VIS:
        import matplotlib.pyplot as plt
        for h in range(K.shape[2]):
            plt.figure()
            plt.title('height:' + str(h))
            imgplot = plt.imshow(K[:, :, h])
            imgplot.set_interpolation('nearest')
            plt.colorbar()
        plt.show()
    return K
