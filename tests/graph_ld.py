"""np.longdouble restatement of the four O(n^3) node kernels (64-bit significand on x86: about 1.1e-19 per operation), for
measuring how far the float64 CPU restatement tests/graph_cpu.py is from the exact matrices.  tests/test_gpu_graph.py allows
the device 8 times that error (floor 1e-13); the measured figures are in its docstring.  Run by hand:

    python tests/graph_ld.py            # prints, per (n, kernel), max |K_float64 - K_longdouble| / max |K_longdouble|

The inverses are Gauss-Jordan eliminations without pivoting (the matrices are symmetric positive definite), the power is
repeated multiplication, the exponential the scaled Taylor series (degree 30 after scaling the 1-norm bound below 1/2,
then repeated squaring)."""
import sys

import numpy as np

import graph_cpu

LD = np.longdouble


def norm_lap(A):
    A = np.asarray(A, dtype=LD)
    s = np.sqrt(LD(1) / A.sum(axis=0))
    return np.identity(A.shape[0], dtype=LD) - (s[:, None] * A) * s[None, :]


def inv_spd(M):
    n = M.shape[0]
    W = np.concatenate((np.array(M, dtype=LD), np.identity(n, dtype=LD)), axis=1)
    for k in range(n):
        W[k] /= W[k, k]
        f = W[:, k].copy()
        f[k] = 0
        W -= f[:, None] * W[k][None, :]
    return W[:, n:]


def reg_lap_kernel(A, sigma=1):
    return inv_spd(np.identity(A.shape[0], dtype=LD) + (LD(sigma) ** 2) * norm_lap(A))


def vnd_kernel(A, alpha=0.5):
    return inv_spd(np.identity(A.shape[0], dtype=LD) - LD(alpha) * (np.identity(A.shape[0], dtype=LD) - norm_lap(A)))


def rw_kernel(A, p=1, a=2):
    p = int(p)
    if a <= 1:
        a = 1.0001
    M = LD(a) * np.identity(A.shape[0], dtype=LD) - norm_lap(A)
    K = M
    for _ in range(p - 1):
        K = K @ M
    return K


def diff_kernel(A, beta=0.5):
    A = np.asarray(A, dtype=LD)
    H = LD(beta) * (A - np.diag(A.sum(axis=1)))
    s = 0
    while float(np.abs(H).sum(axis=0).max()) / 2.0 ** s > 0.5:
        s += 1
    H = H / LD(2) ** s
    X = np.identity(A.shape[0], dtype=LD) + H / LD(30)
    for k in range(29, 0, -1):
        X = np.identity(A.shape[0], dtype=LD) + (H @ X) / LD(k)
    for _ in range(s):
        X = X @ X
    return X


CASES = (("regLap", lambda A: graph_cpu.reg_lap_kernel(A, 0.7), lambda A: reg_lap_kernel(A, 0.7)),
         ("VND", lambda A: graph_cpu.vnd_kernel(A, 0.5), lambda A: vnd_kernel(A, 0.5)),
         ("rw", lambda A: graph_cpu.rw_kernel(A, 3, 2), lambda A: rw_kernel(A, 3, 2)),
         ("diff", lambda A: graph_cpu.diff_kernel(A, 0.5), lambda A: diff_kernel(A, 0.5)))


def graph(n, d=8, k=3, seed=5):
    return graph_cpu.form_knn_graph(np.random.RandomState(seed).randn(n, d), k)


if __name__ == "__main__":
    for n in [int(a) for a in sys.argv[1:]] or [200, 1500]:
        A = graph(n)
        for name, f64, ld in CASES:
            K = ld(A)
            print("n=%d %-6s float64 error %.3e" % (n, name, float(np.max(np.abs(f64(A) - K)) / np.max(np.abs(K)))), flush=True)
