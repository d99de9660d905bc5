"""Kernels on the nodes of a graph given by its adjacency matrix A (reference: pyGPs/GraphExtensions/nodeKernels.py).

A is a dense symmetric matrix without isolated nodes.  The O(n^2) kernels and the pseudo-inverse run on the host; the
O(n^3) ones -- two inverses, a matrix power, a matrix exponential -- run on the device (``pgp_node_kernel``,
csrc/graph.hip) on the Cholesky factorisation and the fp64 GEMM of the fits.  There is no CPU fallback."""
import numpy as np

from .. import _lib

REGLAP, VND, RW, DIFF = 0, 1, 2, 3


def _device(kind, A, p0, p1=0.0):
    A = _lib.f64(np.asarray(A))
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("pygps_amd: the adjacency matrix must be square, got shape %s" % (A.shape,))
    n = A.shape[0]
    K = np.empty((n, n))
    _lib.check(_lib.load().pgp_node_kernel(_lib.ctx(), kind, _lib.ptr(A), n, float(p0), float(p1), _lib.ptr(K)),
               "pgp_node_kernel")
    return K


def normLap(A):
    """Normalised Laplacian L = I - D^-1/2 A D^-1/2 with D the diagonal matrix of the degrees (nodeKernels.py:28-39).
    Host, O(n^2): the two diagonal scalings are applied elementwise."""
    A = np.asarray(A)
    s = np.sqrt(1. / A.sum(axis=0))
    return np.identity(A.shape[0]) - (s[:, None] * A) * s[None, :]


def regLapKernel(A, sigma=1):
    """Regularised Laplacian kernel inv(I + sigma^2 L)  (nodeKernels.py:42-52).  Device: the matrix is symmetric positive
    definite (spectrum in [1, 1 + 2 sigma^2]), so the inverse is a Cholesky factorisation with its inverse."""
    return _device(REGLAP, A, sigma)


def psInvLapKernel(A):
    """Pseudo-inverse of the normalised Laplacian (nodeKernels.py:55-63).  An SVD with a rank decision (L has one zero
    eigenvalue per connected component): stays ``np.linalg.pinv`` on the host."""
    return np.linalg.pinv(normLap(A))


def diffKernel(A, beta=0.5):
    """Diffusion kernel exp(beta H), H = A - D  (nodeKernels.py:66-80).  Device, without an eigendecomposition: beta H is
    scaled by 2^-s (s from the 1-norm bound 2 |beta| max degree, scaled norm <= 1/2), the Taylor series is taken to degree
    18 and the result squared s times."""
    return _device(DIFF, A, beta)


def VNDKernel(A, alpha=0.5):
    """Von Neumann diffusion kernel inv(I - alpha D^-1/2 A D^-1/2)  (nodeKernels.py:83-98).  Device, Cholesky: positive
    definite for alpha < 1; alpha >= 1 raises ``numpy.linalg.LinAlgError`` like a kernel matrix that is not."""
    return _device(VND, A, alpha)


def rwKernel(A, p=1, a=2):
    """p-step random walk kernel (a I - L)^p  (nodeKernels.py:101-119): p is truncated to an integer, p < 1 raises, a <= 1
    becomes 1.0001, as in the reference.  Device: repeated squaring on the GEMM."""
    if type(p) != int:
        p = int(p)
    if p < 1:
        raise Exception('Step parameter p needs to be larger than 0.')
    if a <= 1:
        a = 1.0001
    return _device(RW, A, a, p)


def cosKernel(A):
    """Cosine kernel cos(L pi / 4), ELEMENTWISE as in the reference (nodeKernels.py:122-131) -- not a matrix function and not
    positive semi-definite in general; mirrored as it is.  Host, O(n^2)."""
    return np.cos(normLap(A) * np.pi / 4)
