"""Graph utilities (reference: pyGPs/GraphExtensions/graphUtil.py)."""
import numpy as np

from .. import _lib


def formKnnGraph(pc, k):
    """Symmetrised k-nearest-neighbour graph of the rows of ``pc`` as a dense 0 / 1 float array (graphUtil.py:29-46): every
    point's k nearest other points, an edge if either end chose the other.  Device (``pgp_knn_graph``, csrc/graph.hip):
    brute-force squared distances and a per-row selection.  The reference asks a KD-tree for k + 1 neighbours and drops the
    first as the point itself; with duplicate points or exact ties among the distances the tree's order is unspecified, so
    equality with the reference is promised for tie-free data only (here the lower index wins a tie)."""
    pc = _lib.f64(np.asarray(pc))
    if pc.ndim != 2:
        raise ValueError("pygps_amd: formKnnGraph takes an (n, d) array of points, got shape %s" % (pc.shape,))
    n, d = pc.shape
    k = int(k)
    if not 1 <= k < n:
        raise ValueError("pygps_amd: formKnnGraph needs 1 <= k < n, got k = %d, n = %d" % (k, n))
    A = np.empty((n, n))
    _lib.check(_lib.load().pgp_knn_graph(_lib.ctx(), _lib.ptr(pc), n, d, k, _lib.ptr(A)), "pgp_knn_graph")
    return A


def formKernelMatrix(M, indice_train, indice_test):
    """Split a precomputed n x n kernel matrix over all nodes into the two matrices ``cov.Pre(M1, M2)`` takes
    (graphUtil.py:49-67): M1 is (train + 1) x test, the train-test block with the diagonal of the test-test block as its
    last row; M2 is the train x train block.  Host index work."""
    tr = np.asarray(indice_train)
    te = np.asarray(indice_test)
    M = np.asarray(M)
    M1 = np.concatenate((M[np.ix_(tr, te)], np.diag(M)[te].reshape(1, te.shape[0])))
    M2 = M[np.ix_(tr, tr)]
    return M1, M2


def normalizeKernel(K):
    """Correlation matrix of a kernel matrix: entry (i, j) divided by sqrt(K_ii K_jj)  (graphUtil.py:70-82).  Host, O(n^2)."""
    Kdiag = np.atleast_2d(np.diag(K))
    return K / np.sqrt(Kdiag * Kdiag.T)
