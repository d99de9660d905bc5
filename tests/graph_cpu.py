"""CPU restatement (numpy, float64) of the reference's graph helpers, written from their formulas
(pyGPs/GraphExtensions/nodeKernels.py, graphUtil.py), for building test inputs where the reference is not available: the
GPU tests make their adjacency matrices, node kernels and the (M1, M2) pair of cov.Pre from seeds with these functions.
tests/test_graph_host.py pins every one of them to fixtures recorded from the reference (tests/golden/make_golden_graph.py).

A: dense symmetric 0/1 adjacency matrix without self loops and without isolated nodes.
"""
import numpy as np


def norm_lap(A):
    """Normalised Laplacian L = I - D^-1/2 A D^-1/2, D = diag(degrees)  (nodeKernels.py:28-39)."""
    A = np.asarray(A, dtype=float)
    s = np.sqrt(1.0 / A.sum(axis=0))
    return np.identity(A.shape[0]) - (s[:, None] * A) * s[None, :]


def reg_lap_kernel(A, sigma=1):
    """Regularised Laplacian kernel inv(I + sigma^2 L)  (nodeKernels.py:42-52)."""
    return np.linalg.inv(np.identity(A.shape[0]) + (sigma ** 2) * norm_lap(A))


def ps_inv_lap_kernel(A):
    """Pseudo-inverse of the normalised Laplacian  (nodeKernels.py:55-63)."""
    return np.linalg.pinv(norm_lap(A))


def diff_kernel(A, beta=0.5):
    """Diffusion kernel exp(beta H), H = A - D, through the symmetric eigendecomposition  (nodeKernels.py:66-80)."""
    A = np.array(A, dtype=float)
    w, Q = np.linalg.eigh(A - np.diag(A.sum(axis=1)))
    return np.dot(np.dot(Q, np.diag(np.exp(beta * w))), Q.T)


def vnd_kernel(A, alpha=0.5):
    """Von Neumann diffusion kernel inv(I - alpha S), S = D^-1/2 A D^-1/2  (nodeKernels.py:83-98)."""
    A = np.asarray(A, dtype=float)
    s = np.sqrt(1.0 / A.sum(axis=0))
    return np.linalg.inv(np.identity(A.shape[0]) - alpha * ((s[:, None] * A) * s[None, :]))


def rw_kernel(A, p=1, a=2):
    """p-step random walk kernel (a I - L)^p; int(p), p < 1 raises, a <= 1 becomes 1.0001  (nodeKernels.py:101-119)."""
    p = int(p)
    if p < 1:
        raise Exception('Step parameter p needs to be larger than 0.')
    if a <= 1:
        a = 1.0001
    return np.linalg.matrix_power(a * np.identity(A.shape[0]) - norm_lap(A), p)


def cos_kernel(A):
    """Elementwise cos(L pi / 4)  (nodeKernels.py:122-131); not positive semi-definite in general."""
    return np.cos(norm_lap(A) * np.pi / 4)


def form_knn_graph(pc, k):
    """Symmetrised k-nearest-neighbour graph by brute force: every point's k nearest other points, edge if either end chose
    the other (graphUtil.py:29-46, which asks a KD-tree for k + 1 neighbours and drops the first, the point itself).
    Equal to the reference on data without duplicate points and without ties among the distances."""
    pc = np.asarray(pc, dtype=float)
    n = pc.shape[0]
    A = np.zeros((n, n))
    for i in range(n):
        d2 = np.sum((pc - pc[i]) ** 2, axis=1)
        d2[i] = -1.0                                  # the point itself comes first
        nn = np.argsort(d2, kind="stable")[1:k + 1]
        A[i, nn] = 1.0
    return np.maximum(A, A.T)


def form_kernel_matrix(M, indice_train, indice_test):
    """(M1, M2) of cov.Pre from a kernel matrix over all nodes: M1 = [K(train, test); diag K(test, test)], M2 = K(train, train)
    (graphUtil.py:49-67)."""
    tr, te = np.asarray(indice_train), np.asarray(indice_test)
    M1 = np.concatenate((M[np.ix_(tr, te)], np.diag(M)[te][None, :]))
    return M1, M[np.ix_(tr, tr)]


def normalize_kernel(K):
    """K_ij / sqrt(K_ii K_jj)  (graphUtil.py:70-82)."""
    d = np.atleast_2d(np.diag(K))
    return K / np.sqrt(d * d.T)


def graph_problem(n, ns, d, seed, k=3, beta=0.5):
    """A semi-supervised problem shaped like Demo/USPS/demo_NodeKernel.py: n + ns random points in d dimensions with labels
    from a noisy linear rule, their k-NN graph, the diffusion kernel over all nodes, and the split into n training and ns
    test nodes (a fixed permutation).  Returns dict(x, y, xs, ys, M1, M2, A, K, train, test)."""
    rng = np.random.RandomState(seed)
    N = n + ns
    pts = rng.randn(N, d)
    w = rng.randn(d, 1)
    lab = np.sign(pts @ w / np.sqrt(d) + 0.3 * rng.randn(N, 1))
    lab[lab == 0] = 1
    perm = rng.permutation(N)
    train, test = np.sort(perm[:n]), np.sort(perm[n:])
    A = form_knn_graph(pts, k)
    K = diff_kernel(A, beta)
    M1, M2 = form_kernel_matrix(K, train, test)
    return dict(x=pts[train], y=lab[train], xs=pts[test], ys=lab[test], M1=M1, M2=M2, A=A, K=K, train=train, test=test,
                pts=pts, lab=lab)
