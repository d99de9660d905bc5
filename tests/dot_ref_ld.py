"""Long-double restatement of the dot-product kernels cov.Linear, cov.Poly and cov.LINard and of the trees the G27 fixtures use,
with a per-entry forward error bar (test infrastructure, CPU only).

    dot_matrix(name, hyp, para, x=None, z=None, mode=..., der=None) -> (K, bar)      name in "linear" | "poly" | "linard"
    tree_matrix(tree, hyp, x=None, z=None, mode=..., der=None) -> (K, bar)
    build(tree, hyp, cov) -> the pygps_amd kernel object of a tree;  CASES / case_tree(name, d): the G27 cases

x / z are the exact fp64 arrays handed to the device; everything after them runs in np.longdouble (x86 80-bit).  Definitions
(p = sum_k x_k z_k, J = 1e-10 on the training diagonal, 0 elsewhere; 'self_test': p = |z|^2 per point, J = 0):

    linear   sf2 (p + J), sf2 = exp(h0)                         der 0: 2 sf2 p
    poly     sf2 (c + p + J)^d, c = exp(h0), sf2 = exp(2 h1)     der 0: c d sf2 (c + p)^(d-1); der 1: 2 sf2 (c + p)^d; der 2: 0
    linard   sum_k x_k z_k / ell_k^2 + J, ell = exp(h)          der k: -2 x_k z_k / ell_k^2

The bar (EPS = 2^-53, the unit roundoff of fp64; d = input dimension) bounds the rounding of an fp64 evaluation that sums p by an
fma chain in coordinate order:

  * the chain over d terms:  |dp| <= gamma_d sum_k |x_k z_k| <= EPS (d + 1) sum_k |x_k z_k|  (one rounding per fma; Higham 3.1);
  * linard works on coordinates a_k = x_k * (1 / ell_k): 1 / ell_k = 1 / exp(h_k) carries the rounding of exp (at most one ulp
    = 2 EPS) and of the division (EPS), each a_k one more, twice over for the two factors: 8 EPS per term, so
    |dp| <= EPS (d + 9) sum_k |a_k b_k|;
  * poly's base b = c + p + J: c = exp(h0) within 2 EPS c, the two additions within EPS |b| each:  |db| <= |dp| + 2 EPS (c + |b|);
  * the error of the argument goes through |dk/dp| (first order, evaluated in long double);
  * the map itself: integer powers by squaring take at most 2 floor(log2 d) + 1 <= d_poly + 1 multiplications, one more by sf2:
    EPS (d_poly + 2) |k|  (d_poly = 1 for linear and linard); the derivatives' prefactors (2, c d) two more: EPS (d_poly + 4) |k|;
  * sf2 = exp(.) within one ulp: 2 EPS |k|.

Nothing is tuned: the device and the recorded reference matrices (which sum p in BLAS order, bounded by the same gamma_d) are held
to these bars as they stand.  Trees combine the bars of their leaves to first order (sum: added; product: |a| bar_b + |b| bar_a
+ EPS |a b|; scale: exp(h) within 2 EPS, one multiplication); the RBF / RBFard leaves come from tests/kernel_ref_ld.py with
their own bars.
"""
import numpy as np

import kernel_ref_ld as R
from oracle import gp_oracle as O

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble must be the x86 80-bit extended format"
EPS = 2.0 ** -53
JITTER = LD(1e-10)


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def _dots(x, z, mode, sc, extra):
    """p (long double), |dp| bound, same-point mask; sc: per-coordinate factor applied to both sides (long double)."""
    if mode == "self_test":
        a = _ld(z) * sc[None, :]
        p = (a * a).sum(axis=1)[:, None]
        ab = p.copy()
        same = np.zeros(p.shape, dtype=bool)
    else:
        zz = x if mode == "train" else z
        a, b = _ld(x) * sc[None, :], _ld(zz) * sc[None, :]
        p = a @ b.T
        ab = np.abs(a) @ np.abs(b).T
        same = np.eye(x.shape[0], dtype=bool) if mode == "train" else np.zeros(p.shape, dtype=bool)
    d = (z if mode == "self_test" else x).shape[1]
    return p, EPS * (d + 1 + extra) * ab, same


def _ipow(b, n):
    r = np.ones_like(b)
    for _ in range(int(n)):
        r = r * b
    return r


def dot_matrix(name, hyp, para, x=None, z=None, mode="train", der=None):
    hyp = _ld(hyp)
    ref = z if mode == "self_test" else x
    D = ref.shape[1]
    if name == "linard":
        assert len(hyp) == D
        sc = 1.0 / np.exp(hyp)
        p, dp, same = _dots(x, z, mode, sc, 8)
        if der is None:
            k = p + np.where(same, JITTER, LD(0))
            return k, (dp + EPS * 3 * np.abs(k)).astype(np.float64)
        if der >= D:
            raise Exception("Wrong derivative index in covLINard")
        one = np.zeros(D, dtype=LD)
        one[der] = sc[der]
        pk, dpk, _ = _dots(x, z, mode, one, 8)
        k = -2.0 * pk
        return k, (2.0 * dpk + EPS * 5 * np.abs(k)).astype(np.float64)
    p, dp, same = _dots(x, z, mode, np.ones(D, dtype=LD), 0)
    J = np.where(same, JITTER, LD(0))
    if name == "linear":
        sf2 = np.exp(hyp[0])
        if der is None:
            k = sf2 * (p + J)
            return k, (sf2 * dp + EPS * (3 + 2) * np.abs(k)).astype(np.float64)
        if der >= 1:
            raise Exception("Wrong derivative index in covLinear")
        k = 2.0 * sf2 * p
        return k, (2.0 * sf2 * dp + EPS * (5 + 2) * np.abs(k)).astype(np.float64)
    assert name == "poly"
    dg = int(para)
    assert dg >= 1
    c, sf2 = np.exp(hyp[0]), np.exp(2.0 * hyp[1])
    if der is None:
        b = c + p + J
        k = sf2 * _ipow(b, dg)
        dk = sf2 * dg * np.abs(_ipow(b, dg - 1))
        nmul = dg + 2
    elif der == 0:
        b = c + p
        k = c * dg * sf2 * _ipow(b, dg - 1)
        dk = c * dg * sf2 * (dg - 1) * np.abs(_ipow(b, dg - 2)) if dg >= 2 else np.zeros_like(b)
        nmul = dg + 4
    elif der == 1:
        b = c + p
        k = 2.0 * sf2 * _ipow(b, dg)
        dk = 2.0 * sf2 * dg * np.abs(_ipow(b, dg - 1))
        nmul = dg + 4
    elif der == 2:
        return np.zeros(p.shape, dtype=LD), np.zeros(p.shape)
    else:
        raise Exception("Wrong derivative entry in Poly")
    db = dp + 2.0 * EPS * (c + np.abs(b))
    return k, (dk * db + EPS * (nmul + 2) * np.abs(k)).astype(np.float64)


# ---- trees: ("leaf", name, para) | ("sum", a, b) | ("prod", a, b) | ("scale", a); leaf names: the three above, "rbf", "rbfard" ----
def n_hyp(tree, D):
    if tree[0] == "leaf":
        return {"linear": 1, "poly": 2, "linard": D, "rbf": 2, "rbfard": D + 1}[tree[1]]
    if tree[0] == "scale":
        return 1 + n_hyp(tree[1], D)
    return n_hyp(tree[1], D) + n_hyp(tree[2], D)


def tree_matrix(tree, hyp, x=None, z=None, mode="train", der=None):
    hyp = np.asarray(hyp, dtype=np.float64)
    D = (z if mode == "self_test" else x).shape[1]
    kw = dict(x=x, z=z, mode=mode)
    if tree[0] == "leaf":
        if tree[1] in ("linear", "poly", "linard"):
            return dot_matrix(tree[1], hyp, tree[2], der=der, **kw)
        K, bar = R.ref_matrix(O.RBF if tree[1] == "rbf" else O.RBFARD, hyp, 0, der=der, **kw)
        return K, np.asarray(bar, dtype=np.float64)
    if tree[0] == "scale":
        s = np.exp(_ld(hyp[0]))
        if der == 0:
            K, bar = tree_matrix(tree[1], hyp[1:], **kw)
            return 2.0 * s * K, (2.0 * s * bar + 4 * EPS * np.abs(2.0 * s * K)).astype(np.float64)
        K, bar = tree_matrix(tree[1], hyp[1:], der=None if der is None else der - 1, **kw)
        return s * K, (s * bar + 3 * EPS * np.abs(s * K)).astype(np.float64)
    n1 = n_hyp(tree[1], D)
    h1, h2 = hyp[:n1], hyp[n1:]
    if tree[0] == "sum":
        if der is None:
            (A, ba), (B, bb) = tree_matrix(tree[1], h1, **kw), tree_matrix(tree[2], h2, **kw)
            return A + B, (ba + bb + EPS * np.abs(A + B)).astype(np.float64)
        return tree_matrix(tree[1], h1, der=der, **kw) if der < n1 else tree_matrix(tree[2], h2, der=der - n1, **kw)
    assert tree[0] == "prod"
    if der is None:
        (A, ba), (B, bb) = tree_matrix(tree[1], h1, **kw), tree_matrix(tree[2], h2, **kw)
    elif der < n1:
        (A, ba), (B, bb) = tree_matrix(tree[1], h1, der=der, **kw), tree_matrix(tree[2], h2, **kw)
    else:
        (A, ba), (B, bb) = tree_matrix(tree[1], h1, **kw), tree_matrix(tree[2], h2, der=der - n1, **kw)
    return A * B, (np.abs(A) * bb + np.abs(B) * ba + EPS * np.abs(A * B)).astype(np.float64)


def build(tree, hyp, cov, D):
    """The pygps_amd kernel object of `tree` with the flat hypers `hyp`."""
    hyp = [float(h) for h in hyp]
    if tree[0] == "leaf":
        k = {"linear": lambda: cov.Linear(), "poly": lambda: cov.Poly(d=tree[2]), "linard": lambda: cov.LINard(D=D),
             "rbf": lambda: cov.RBF(), "rbfard": lambda: cov.RBFard(D=D)}[tree[1]]()
        assert len(k.hyp) == len(hyp)
        k.hyp = hyp
        return k
    if tree[0] == "scale":
        return hyp[0] * build(tree[1], hyp[1:], cov, D)
    n1 = n_hyp(tree[1], D)
    a, b = build(tree[1], hyp[:n1], cov, D), build(tree[2], hyp[n1:], cov, D)
    return a + b if tree[0] == "sum" else a * b


L = lambda name, para=0: ("leaf", name, para)
# the kernel-matrix cases of tests/golden/make_golden_dot.py (CASES there), the fits (FITS there) and the classifiers
CASES = {
    "linear": L("linear"), "poly1": L("poly", 1), "poly2": L("poly", 2), "poly3": L("poly", 3), "poly5": L("poly", 5),
    "linard": L("linard"),
    "lin_plus_rbf": ("sum", L("linear"), L("rbf")),
    "lin_times_rbf": ("prod", L("linear"), L("rbf")),
    "half_lin_plus_rbf": ("sum", ("scale", L("linear")), L("rbf")),
    "poly_plus_rbfard": ("sum", L("poly", 2), L("rbfard")),
    "lin_times_poly_plus_rbfard": ("sum", ("prod", L("linear"), L("poly", 3)), L("rbfard")),
}
FITS = {
    "lin_plus_rbf_d1": CASES["lin_plus_rbf"], "lin_plus_rbf_d3": CASES["lin_plus_rbf"], "lin_times_rbf": CASES["lin_times_rbf"],
    "half_lin_plus_rbf": CASES["half_lin_plus_rbf"], "linear": CASES["linear"], "poly3": CASES["poly3"],
    "poly_plus_rbfard": CASES["poly_plus_rbfard"], "linard": CASES["linard"], "const_mean": CASES["lin_plus_rbf"],
}
EP_TREE = ("sum", ("prod", L("linear"), L("rbf")), L("poly", 2))
LAPLACE_TREE = CASES["lin_plus_rbf"]


def n_der(name, tree, hyp):
    return 3 if tree[0] == "leaf" and tree[1] == "poly" else len(hyp)       # plain Poly: der 2 ("the degree") gives zeros


def golden_sets(golden, name, d, n=130):
    """The recorded matrices of one G27 kernel case: {key: {"train" | "cross" | "self": array}}, key "K" or "dK<i>"; the
    'train' matrices are rebuilt from their stored upper triangle."""
    import glob
    import os
    import conftest
    out = {}
    iu = np.triu_indices(n)
    files = sorted(glob.glob(os.path.join(conftest.GOLDEN, "G27_dot_k_%s_d%d_p*.npz" % (name, d))))
    assert files
    for f in files:
        g = np.load(f, allow_pickle=False)
        for key in g.files:
            if key == "meta":
                continue
            what, mode = key.split("_", 1)
            if mode == "train_ut":
                A = np.zeros((n, n))
                A[iu] = g[key]
                A = A + np.triu(A, 1).T
                out.setdefault(what, {})["train"] = A
            else:
                out.setdefault(what, {})[mode] = g[key]
    return out


def exact_gp(K, dKs, y, m, sn2):
    """nlZ, alpha, diag L and dnlZ of an exact GP from fp64 matrices (Core/inf.py:353-384), in numpy."""
    n = K.shape[0]
    Lc = np.linalg.cholesky(K / sn2 + np.eye(n))
    r = y - m
    alpha = np.linalg.solve(Lc.T, np.linalg.solve(Lc, r)) / sn2
    nlZ = float((r.T @ alpha).item() / 2 + np.log(np.diag(Lc)).sum() + n * np.log(2 * np.pi * sn2) / 2)
    Q = np.linalg.solve(Lc.T, np.linalg.solve(Lc, np.eye(n))) / sn2 - alpha @ alpha.T
    return nlZ, alpha, np.diag(Lc.T).copy(), [float((Q * dK).sum() / 2) for dK in dKs], float(sn2 * np.trace(Q))
