"""Long-double reference of GP.predict (Core/gp.py:395-417) and of tools.solve_chol (Core/tools.py:81-97), with a per-point
tolerance that is computed from the reference side only (test infrastructure, CPU only).

    reference(spec, hyp, x, xs, ms, alpha, sW, R) -> Ref        spec: ("oracle", kind, para) | ("dot", tree)
    check(fmu, fs2, ref) -> (worst ratio, (field, index))       the unit the tests assert <= 1 in; ratios(): per field
    solve_chol_ld(R, B), solve_tolerance(R, B, X_ld)

The reference predicts from a GIVEN posterior (alpha, sW and the upper factor R, L = R'): the fits are pinned elsewhere, so a
failure here points at the prediction alone.  x, xs and ms are the exact fp64 arrays handed to the device; everything after them
runs in np.longdouble (x86 80-bit):

    Ks, barK = the cross block and its fp64 rounding bar (kernel_ref_ld.ref_matrix / dot_ref_ld.tree_matrix), kss from 'self_test'
    fmu = ms + Ks' alpha
    V   = L^-1 (sW o Ks)             row-by-row forward substitution
    fs2 = max(kss - colsum(V o V), 0)

Tolerance of test point j:  tol_j = T_j + SOLVE_FACTOR E_cpu + floor_j

  * T_j, the kernel bar propagated to first order:  T_fmu[j] = sum_i barK[i,j] |alpha_i|,
    T_fs2[j] = 2 sum_i |V[i,j]| (|L^-1| (sW o barK))[i,j]   (|L^-1| in fp64: a bar need not be extended precision);
  * E_cpu, the solve term, MEASURED on the CPU: the prediction is evaluated twice in fp64 from the same L, sW, alpha and the
    oracle's fp64 Ks -- by scipy's solve_triangular and by inv(L) @ (sW o Ks) -- and E_cpu is the larger of their max-abs errors
    against the long-double values over the case's test points.  The device gets SOLVE_FACTOR = 8 times that: it does the same O(n)
    dot products per entry in another order (MFMA k-chunks, explicit 128 x 128 diagonal inverses instead of substitution, W from
    a recursive trtri or from the fit's inverse rows), each of which obeys the same componentwise bound within a small constant;
  * floor_j = 4 * 2^-53 * scale_j,  scale_j = kss_j for fs2 and |ms_j| + sum_i |Ks_ij alpha_i| for fmu: the last roundings.

Columns (test points) are independent: a Ref is computed once per model at all its test points and `take(idx)` selects the points
of one case; E_cpu is then taken over the selected points.  `cached` keeps one Ref per distinct set of inputs.
"""
import hashlib

import numpy as np
from scipy.linalg import solve_triangular

import kernel_ref_ld as KR
import dot_ref_ld as DR
from oracle import gp_oracle as O

LD = np.longdouble
EPS = 2.0 ** -53
SOLVE_FACTOR = 8.0            # the device's share of the measured CPU solve error (module docstring)
FLOOR = 4.0                   # roundings of the last operations, in units of EPS * scale_j
BATCH = 128                   # predict_batch of the multi-batch cases


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


# ---- fp64 covariances of the dot-product trees (the oracle has no dot-product kinds) ---------------------------------------------
def dot_cov64(tree, hyp, x=None, z=None, mode="cross"):
    """fp64 value matrix of a dot_ref_ld tree: plain numpy, the reference's formulas (dot_ref_ld's docstring)."""
    hyp = np.asarray(hyp, dtype=np.float64)
    D = (z if mode == "self_test" else x).shape[1]
    if tree[0] == "leaf":
        name = tree[1]
        if name in ("rbf", "rbfard"):
            return O.cov_matrix(O.RBF if name == "rbf" else O.RBFARD, hyp, 0, x=x, z=z, mode=mode)
        sc = 1.0 / np.exp(hyp) if name == "linard" else np.ones(D)
        if mode == "self_test":
            p = ((z * sc) ** 2).sum(axis=1)[:, None]
        else:
            zz = x if mode == "train" else z
            p = (x * sc) @ (zz * sc).T
            if mode == "train":
                p = p + 1e-10 * np.eye(x.shape[0])
        if name == "linard":
            return p
        if name == "linear":
            return np.exp(hyp[0]) * p
        return np.exp(2.0 * hyp[1]) * (np.exp(hyp[0]) + p) ** int(tree[2])
    if tree[0] == "scale":
        return np.exp(hyp[0]) * dot_cov64(tree[1], hyp[1:], x, z, mode)
    n1 = DR.n_hyp(tree[1], D)
    a, b = dot_cov64(tree[1], hyp[:n1], x, z, mode), dot_cov64(tree[2], hyp[n1:], x, z, mode)
    return a + b if tree[0] == "sum" else a * b


def _cov_ld(spec, hyp, x, z, mode):
    if spec[0] == "dot":
        K, bar = DR.tree_matrix(spec[1], hyp, x=x, z=z, mode=mode)
    else:
        K, bar = KR.ref_matrix(spec[1], hyp, spec[2], x=x, z=z, mode=mode)
    return K, np.asarray(bar, dtype=np.float64)


def _cov64(spec, hyp, x, z, mode):
    if spec[0] == "dot":
        return dot_cov64(spec[1], hyp, x, z, mode)
    return O.cov_matrix(spec[1], hyp, spec[2], x=x, z=z, mode=mode)


# ---- long-double triangular solves ---------------------------------------------------------------------------------------------
def forward_ld(L, B):
    """V with L V = B (L lower triangular), long double, row by row."""
    L, B = np.asarray(L, dtype=LD), np.asarray(B, dtype=LD)
    n = L.shape[0]
    V = np.empty_like(B)
    for i in range(n):
        V[i] = (B[i] - L[i, :i] @ V[:i]) / L[i, i] if i else B[0] / L[0, 0]
    return V


def backward_ld(U, B):
    """X with U X = B (U upper triangular), long double, row by row from the last."""
    U, B = np.asarray(U, dtype=LD), np.asarray(B, dtype=LD)
    n = U.shape[0]
    X = np.empty_like(B)
    for i in range(n - 1, -1, -1):
        X[i] = (B[i] - U[i, i + 1:] @ X[i + 1:]) / U[i, i] if i < n - 1 else B[i] / U[i, i]
    return X


def solve_chol_ld(R, B):
    """X = (R'R)^-1 B for the upper factor R: the two substitutions of tools.solve_chol in long double."""
    R = _ld(R)
    B = _ld(B).reshape(R.shape[0], -1)
    return backward_ld(R, forward_ld(R.T, B))


def solve_tolerance(R, B, X):
    """Per column j of tools.solve_chol: SOLVE_FACTOR x the error of the oracle's two fp64 triangular solves against the
    long-double X, plus the floor FLOOR EPS max_i |X_ij| (the solution's own last roundings).  Returns (tol (nrhs), cpu error)."""
    R = np.asarray(R, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64).reshape(R.shape[0], -1)
    cpu = O.solve_chol(R, B, faithful=False)
    e = np.max(np.abs(cpu.astype(LD) - X), axis=0).astype(np.float64)
    scale = np.max(np.abs(X), axis=0).astype(np.float64)
    return SOLVE_FACTOR * e + FLOOR * EPS * scale, e


def check_solve(Xdev, X, tol):
    """(worst ratio, column) of max_i |Xdev_ij - X_ij| / tol_j."""
    Xdev = np.asarray(Xdev, dtype=np.float64).reshape(X.shape)
    err = np.max(np.abs(Xdev.astype(LD) - X), axis=0).astype(np.float64)
    err = np.where(np.all(np.isfinite(Xdev), axis=0), err, np.inf)
    r = err / tol
    j = int(np.argmax(r))
    return float(r[j]), j


# ---- the fp64 CPU prediction (the two forms of the solve term; the host test's mutants start from it) -----------------------------
def cpu_predict(L, sW, alpha, Ks, kss, ms, form="solve"):
    """fmu, fs2, V in fp64 from fp64 inputs: form "solve" = scipy's triangular solve, "inverse" = inv(L) @ (sW o Ks)."""
    L = np.asarray(L, dtype=np.float64)
    B = np.asarray(sW, dtype=np.float64).reshape(-1, 1) * Ks
    if form == "solve":
        V = solve_triangular(L, B, lower=True)
    else:
        V = np.tril(np.linalg.inv(L)) @ B
    fmu = np.asarray(ms, dtype=np.float64).ravel() + Ks.T @ np.asarray(alpha, dtype=np.float64).ravel()
    fs2 = np.maximum(np.asarray(kss, dtype=np.float64).ravel() - (V * V).sum(axis=0), 0.0)
    return fmu, fs2, V


class Ref(object):
    """Long-double prediction at a set of test points and what the tolerance is made of (per point unless noted)."""
    FIELDS = ("fmu", "fs2", "kss", "ms", "T_fmu", "T_fs2", "scale_fmu", "cpu_fmu", "sumsq", "absdot")

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def ns(self):
        return self.fmu.shape[0]

    def take(self, idx):
        """The Ref of the test points idx (columns are independent)."""
        idx = np.asarray(idx)
        kw = dict(self.__dict__)
        for k in self.FIELDS:
            kw[k] = getattr(self, k)[idx]
        for k in ("Ks", "V", "Ks64", "barK"):
            kw[k] = getattr(self, k)[:, idx]
        kw["cpu_fs2"] = self.cpu_fs2[:, idx]
        kw["kss64"] = self.kss64[idx]
        return Ref(**kw)

    # ---- the tolerance --------------------------------------------------------------------------------------------
    def e_cpu(self):
        """(E_cpu of fmu, E_cpu of fs2): the larger max-abs error of the two fp64 CPU forms over these test points."""
        return float(np.max(self.cpu_fmu)), float(np.max(self.cpu_fs2))

    def tol(self):
        e_mu, e_s2 = self.e_cpu()
        return (self.T_fmu + SOLVE_FACTOR * e_mu + FLOOR * EPS * self.scale_fmu,
                self.T_fs2 + SOLVE_FACTOR * e_s2 + FLOOR * EPS * self.kss.astype(np.float64))

    def exact(self):
        """Points whose cross-covariances have underflowed against the prior: |Ks' alpha| and colsum(V o V) are below a quarter
        ulp of ms and kss in ANY summation order, so an fp64 prediction gives fmu == ms and fs2 == kss exactly."""
        return ((self.absdot < 0.25 * EPS * np.abs(self.ms).astype(np.float64))
                & (self.sumsq < 0.25 * EPS * self.kss.astype(np.float64)))


def reference(spec, hyp, x, xs, ms, alpha, sW, R):
    x, xs = np.asarray(x, dtype=np.float64), np.asarray(xs, dtype=np.float64)
    n, ns = x.shape[0], xs.shape[0]
    ms = np.asarray(ms, dtype=np.float64).reshape(ns)
    alpha = np.asarray(alpha, dtype=np.float64).reshape(n)
    sW = np.asarray(sW, dtype=np.float64).reshape(n)
    R = np.asarray(R, dtype=np.float64)
    assert R.shape == (n, n)
    L64 = np.ascontiguousarray(R.T)
    Ks, barK = _cov_ld(spec, hyp, x, xs, "cross")
    kss = _cov_ld(spec, hyp, None, xs, "self_test")[0].reshape(ns)
    al, sw = _ld(alpha), _ld(sW)
    prod = Ks * al[:, None]
    fmu = _ld(ms) + prod.sum(axis=0)
    absdot = np.abs(prod).sum(axis=0).astype(np.float64)
    V = forward_ld(_ld(L64), sw[:, None] * Ks)
    sumsq = (V * V).sum(axis=0)
    fs2 = np.maximum(kss - sumsq, LD(0))
    # the kernel bar, to first order
    T_fmu = (barK * np.abs(alpha)[:, None]).sum(axis=0)
    absLinv = np.abs(np.tril(solve_triangular(L64, np.eye(n), lower=True)))
    T_fs2 = 2.0 * (np.abs(V).astype(np.float64) * (absLinv @ (sW[:, None] * barK))).sum(axis=0)
    # the solve term: two fp64 CPU evaluations from the oracle's fp64 cross block
    Ks64 = np.asarray(_cov64(spec, hyp, x, xs, "cross"), dtype=np.float64)
    kss64 = np.asarray(_cov64(spec, hyp, None, xs, "self_test"), dtype=np.float64).reshape(ns)
    cpu_fs2 = np.empty((2, ns))
    for k, form in enumerate(("solve", "inverse")):
        f1, f2, _ = cpu_predict(L64, sW, alpha, Ks64, kss64, ms, form)
        cpu_fs2[k] = np.abs(f2.astype(LD) - fs2).astype(np.float64)
        cpu_fmu = np.abs(f1.astype(LD) - fmu).astype(np.float64)
    return Ref(fmu=fmu, fs2=fs2, kss=kss, ms=ms, T_fmu=T_fmu, T_fs2=T_fs2, scale_fmu=np.abs(ms) + absdot, cpu_fmu=cpu_fmu,
               cpu_fs2=cpu_fs2, sumsq=sumsq.astype(np.float64), absdot=absdot, Ks=Ks, V=V, barK=barK, Ks64=Ks64, kss64=kss64,
               L=L64, alpha=alpha, sW=sW)


_CACHE = {}


def cached(spec, hyp, x, xs, ms, alpha, sW, R):
    """reference(...) once per distinct set of inputs (fits that give the same posterior bit for bit share one Ref)."""
    h = hashlib.blake2b(repr(spec).encode(), digest_size=16)
    for a in (hyp, x, xs, ms, alpha, sW, R):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
        h.update(repr(a.shape).encode())
        h.update(memoryview(a).cast("B"))
    key = h.digest()
    if key not in _CACHE:
        _CACHE[key] = reference(spec, hyp, x, xs, ms, alpha, sW, R)
    return _CACHE[key]


def ratios(fmu, fs2, ref):
    """{"fmu": (worst, j), "fs2": (worst, j)}: per field the largest |value - reference| / tol_j over these test points and
    where it sits.  A value that is not finite counts as infinitely wrong."""
    t_mu, t_s2 = ref.tol()
    out = {}
    for name, got, want, tol in (("fmu", fmu, ref.fmu, t_mu), ("fs2", fs2, ref.fs2, t_s2)):
        got = np.asarray(got, dtype=np.float64).reshape(-1)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert np.all(tol > 0) and np.all(np.isfinite(tol))
        r = np.abs(got.astype(LD) - want).astype(np.float64) / tol
        r = np.where(np.isfinite(got), r, np.inf)
        j = int(np.argmax(r))
        out[name] = (float(r[j]), j)
    return out


def check(fmu, fs2, ref):
    """(worst, (field, j)): the largest |value - reference| / tol_j over fmu and fs2 of these test points, and where it sits."""
    r = ratios(fmu, fs2, ref)
    name = max(r, key=lambda k: r[k][0])
    return r[name][0], (name, r[name][1])


# ---- the test points of every case -------------------------------------------------------------------------------------------
def make_points(x, nmax, seed, far=50.0):
    """The pool of nmax test points of a model, in four blocks: [training points + 1e-3 randn | one exact copy of a training
    point | randn | three points at |x| = far].  `select(nmax, ns)` picks the points of a case with ns of them."""
    rng = np.random.RandomState(seed)
    n, d = x.shape
    near = max(nmax // 3, 0)
    xs = rng.randn(nmax, d)
    if near:
        xs[:near] = x[rng.randint(0, n, near)] + 1e-3 * rng.randn(near, d)
    xs[near] = x[rng.randint(0, n)]
    if nmax >= 5:
        u = rng.randn(3, d)
        xs[nmax - 3:] = far * u / np.sqrt((u * u).sum(axis=1, keepdims=True))
    return xs


def select(nmax, ns):
    """Indices into make_points(x, nmax, ...) of a case with ns points: the first third near training points, the exact copy,
    random points, the three far points last (from ns = 5; below that the copy first, then random points)."""
    assert 1 <= ns <= nmax
    near = nmax // 3
    if ns < 5 or nmax < 5:
        return np.array([near] + list(range(near + 1, near + ns)), dtype=int)
    k = ns // 3
    rest = ns - k - 1 - 3
    assert near + 1 + rest <= nmax - 3
    return np.array(list(range(k)) + [near] + list(range(near + 1, near + 1 + rest)) + [nmax - 3, nmax - 2, nmax - 1], dtype=int)


# ---- input recipes shared by the host test and the GPU test ---------------------------------------------------------------------
MEAN_C = 0.5                                   # mean.Const(0.5): a nonzero ms
MEAN_W = (0.3, -0.2, 0.1)                      # + mean.Linear(MEAN_W) in the multi-batch cases (d = 3): ms differs per test point
MEAN_W_ISLAND = (5.0, 5.0)                     # the EP case (d = 2): a prior mean of ~60 on the island, whose sites end with ttau = 0
SN = 0.05                                      # noise of the regression cases
# RBF + Matern 5 (d = 3), both at ell = sqrt(d): RBF with sf = 1, Matern 5 with sf = exp(-1.5).  Chosen on the CPU so that the
# weakest mutant of tests/test_predict_ref_host.py (one entry of L) exceeds the tolerance > 100 x (at sf = exp(-0.5): ~5 x)
SUM_HYP = np.array([np.log(np.sqrt(3.0)), 0.0, np.log(np.sqrt(3.0)), -1.5])


def reg_data(n, d, seed):
    """x ~ N(0, I), y = sin(x w / sqrt(d)) + 0.1 noise (the suite's synthetic regression recipe)."""
    rng = np.random.RandomState(seed)
    x = rng.randn(n, d)
    w = rng.randn(d, 1)
    return x, np.sin(x @ w / np.sqrt(d)) + 0.1 * rng.randn(n, 1)


def cls_data(n, d, seed, island=0.0):
    """Labels sign(x w / sqrt(d) + 0.3 noise); with island > 0 the first third of the points forms a tight, well-separated
    group around (island, ..., island), all labelled +1."""
    rng = np.random.RandomState(seed)
    x = rng.randn(n, d)
    w = rng.randn(d, 1)
    y = np.sign(x @ w / np.sqrt(d) + 0.3 * rng.randn(n, 1))
    y[y == 0] = 1
    if island:
        k = n // 3
        x[:k] = island + 0.05 * rng.randn(k, d)
        y[:k] = 1
    return x, y


def mean_values(x, linear=False):
    """mean.Const(MEAN_C) (+ mean.Linear(w), w = MEAN_W for linear=True or the given weights) at x, as a column."""
    m = MEAN_C * np.ones((x.shape[0], 1))
    if linear is not False:
        w = MEAN_W if linear is True else linear
        m = m + np.dot(x, np.reshape(np.array(w, dtype=float), (x.shape[1], 1)))
    return m
