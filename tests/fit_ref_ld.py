"""Long-double reference of the exact fit (Core/inf.py:353-384 on the device: the Cholesky sweep of csrc/sweep.hip with its fused
inverse rows, B^-1 = E E', alpha, nlZ, tr Q) with a per-entry tolerance that is computed from the reference side only (test
infrastructure, CPU only).

    reference(B, r, sn2, barB=None) -> FitRef      B (n, n): the matrix the device factorises (K / sn2 + I), fp64 or long double
    cached(...)                                    the same, once per distinct set of inputs
    FitRef.ratios(got) -> {field: (worst, index)}  the unit the tests assert <= 1 in; got: dict of L / Binv / alpha / nlZ / trQ
    FitRef.grad_term(dK), dnlz_reference(...)      1/2 sum Q o dK and the gradient sums with their tolerances
    blocked_fit64(B, r, sn2, leaf, panel, mutant)  the device's form restated in numpy fp64 (and its single-slip mutants)
    large_reference / large_ratios                 n > FULL_MAX: O(n^2) functionals on the device's downloaded outputs

The reference works from B itself, so a failure points at the fit and not at the kernel matrix.  In long double (x86 80-bit):

    L      column Cholesky (left-looking in 64-column panels: every entry is the same dot product, then one sqrt or division)
    E      = L^-T      (predict_ref_ld.forward_ld on column blocks of the identity)
    Binv   = E E'
    z      = L^-1 r,   alpha = E z / sn2
    nlZ    = z'z / (2 sn2) + sum log L_ii + n / 2 log(2 pi sn2)
    trQ    = sn2 tr(Binv / sn2 - alpha alpha')

Tolerance of entry ij of a field X:   tol_ij = bar_ij + (SOLVE_FACTOR E_cpu + FLOOR 2^-53) scale_ij     (predict_ref_ld's construction)

  * scale_ij (fp64: a bar need not be extended precision)
        L       S = |L| Phi(|L^-1| (|L| |L'|) |L^-T|), the first-order sensitivity of the factor to a backward error of |L| |L'|
                (Phi: the lower triangle with a halved diagonal)
        Binv    (|E| |E'|)_ij
        alpha   max |alpha|    (as predict_ref_ld.solve_tolerance)
        nlZ     z'z / (2 sn2) + sum |log L_ii| + |n / 2 log(2 pi sn2)|,      trQ:  tr |Binv| + sn2 sum alpha_i^2
  * E_cpu is MEASURED: the largest max_ij |X_cpu - X_ld| / scale_ij over three fp64 CPU evaluations of the same B -- LAPACK
    (numpy.linalg.cholesky + solve_triangular), and blocked_fit64 with panel = 512 and with panel = 128.  The device gets
    SOLVE_FACTOR = 8 times that: it does the same dot products in another order (MFMA k-chunks, lazy C, 64- or 128-tiles,
    explicit inverses of the diagonal blocks).
  * bar_ij: what a rounding bar barB on the entries of B does to first order
        bar_L = |L| Phi(|L^-1| barB |L^-T|),  bar_Binv = |Binv| barB |Binv|,  bar_alpha = |Binv| barB |alpha|,
        bar_nlZ = 1/2 sum |Q_ij| barK_ij  (Q = Binv / sn2 - alpha alpha', barK = sn2 barB),
        bar_trQ = tr(bar_Binv) + 2 sn2 sum |alpha_i| bar_alpha_i
    barB is None where the device forms B bit for bit as the host does (the dense route at log_sn = 0: fma(K, 1, delta));
    dense_bar(K, sn2) = 3 2^-53 |K| / sn2 for another log_sn (exp, the reciprocal and the fma); the program route adds the kernel
    bar of kernel_ref_ld.ref_matrix divided by sn2.

The CPU evaluations start from B rounded to fp64 -- for the program route, where B is long double, that adds one rounding of B and
no kernel error of the oracle, so E_cpu is not widened by it.

Large n (n > FULL_MAX = 1600, where a full long-double factor is too slow): five functionals of the device's own outputs, each
O(n^2) per probe in long double, each relative to its own componentwise scale:

    residual column j      |B[:, j] - L L[j, :]'|          /  (|L| |L[j, :]|')
    left-inverse row i     |(Binv B)[i, :] - e_i'|         /  (|Binv[i, :]| |B|)
    inverse on a vector    |Binv (B v) - v|, v = +-1       /  (|Binv| |B| |v|)       one probe that crosses every tile of B^-1
    solve residual         |B (sn2 alpha) - r|             /  (|B| |sn2 alpha|)
    nlZ                    |nlZ - nlZ_ld(L, L^-1 r)|       /  its sum of absolute terms

with the same rule: the functional is evaluated on the three fp64 CPU fits, and the device may reach SOLVE_FACTOR times the worst of
them plus FLOOR 2^-53 (plus the first-order bar: barB[:, j], |Binv[i, :]| barB, |Binv| barB |v|, barB |sn2 alpha|, bar_nlZ from the device's Q).
"""
import hashlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from scipy.linalg import solve_triangular

import predict_ref_ld as P

LD = np.longdouble
EPS = P.EPS
SOLVE_FACTOR = P.SOLVE_FACTOR
FLOOR = P.FLOOR
LEAF, PANEL = 128, 512            # the sweep's leaf and panel widths (csrc/sweep.hip sweep_plan)
FULL_MAX = 1600                   # beyond this n the large-n functionals replace the full reference
FIELDS = ("L", "Binv", "alpha", "nlZ", "trQ")
MUTANTS = ("tu_fp32", "solve_fp32", "eet_last_tile", "eet_first_tile", "e_unsolved", "alpha_last_block", "logdet_short",
           "binv_ragged")
# the field every mutant damages (tests/test_fit_ref_host.py)
MUTANT_FIELD = dict(tu_fp32="L", solve_fp32="L", eet_last_tile="Binv", eet_first_tile="Binv", e_unsolved="Binv",
                    alpha_last_block="alpha", logdet_short="nlZ", binv_ragged="Binv")


def _ld(a):
    a = np.asarray(a)
    return a if a.dtype == LD else a.astype(np.float64).astype(LD)


def _f64(a):
    return np.asarray(a).astype(np.float64)


def _threads():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    for v in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS"):
        if os.environ.get(v, "").isdigit():
            n = min(n, int(os.environ[v]))
    return max(1, min(16, n))


def _pmap(fn, items):
    """map on a thread pool: numpy's long-double loops run without the interpreter lock."""
    items = list(items)
    if len(items) < 2 or _threads() < 2:
        return [fn(i) for i in items]
    with ThreadPoolExecutor(_threads()) as ex:
        return list(ex.map(fn, items))


def _round_up(n, m):
    return (n + m - 1) // m * m


# ---- long-double factorisation, inverse, Gram product ------------------------------------------------------------------------------
def chol_ld(B, nb=64):
    """Lower Cholesky factor in long double: left-looking over nb-column panels (the updates of a panel are one product, split
    by rows over the pool), column by column inside a panel."""
    B = _ld(B)
    n = B.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j0 in range(0, n, nb):
        j1 = min(n, j0 + nb)
        if j0:
            Lt = np.ascontiguousarray(L[j0:j1, :j0].T)
            rows = [(r0, min(n, r0 + 256)) for r0 in range(j0, n, 256)]
            Pn = np.vstack(_pmap(lambda rr: B[rr[0]:rr[1], j0:j1] - np.dot(np.ascontiguousarray(L[rr[0]:rr[1], :j0]), Lt), rows))
        else:
            Pn = B[:, :j1].copy()
        for k in range(j1 - j0):
            v = Pn[k:, k] - Pn[k:, :k] @ Pn[k, :k] if k else Pn[:, 0].copy()
            if not v[0] > 0:
                raise np.linalg.LinAlgError("chol_ld: pivot %d is not positive" % (j0 + k + 1))
            d = np.sqrt(v[0])
            Pn[k, k] = d
            Pn[k + 1:, k] = v[1:] / d
        L[j0:, j0:j1] = Pn
    return np.tril(L)


def inv_lower_ld(L, w=128):
    """V = L^-1 (lower triangular): predict_ref_ld.forward_ld on w-column blocks of the identity, each from its own diagonal down."""
    L = _ld(L)
    n = L.shape[0]
    V = np.zeros((n, n), dtype=LD)

    def blk(c0):
        c1 = min(n, c0 + w)
        rhs = np.zeros((n - c0, c1 - c0), dtype=LD)
        rhs[np.arange(c1 - c0), np.arange(c1 - c0)] = 1
        return c0, c1, P.forward_ld(L[c0:, c0:], rhs)
    for c0, c1, X in _pmap(blk, range(0, n, w)):
        V[c0:, c0:c1] = X
    return V


def gram_lower_ld(V, w=128):
    """V'V for a lower-triangular V (= E E' with E = V'), long double, block by block on the lower triangle, then mirrored."""
    n = V.shape[0]
    G = np.empty((n, n), dtype=LD)
    tasks = [(i0, j0) for i0 in range(0, n, w) for j0 in range(0, i0 + 1, w)]

    def task(ij):
        i0, j0 = ij
        return i0, j0, np.dot(np.ascontiguousarray(V[i0:, i0:i0 + w].T), np.ascontiguousarray(V[i0:, j0:j0 + w]))
    for i0, j0, X in _pmap(task, tasks):
        G[i0:i0 + w, j0:j0 + w] = X
        G[j0:j0 + w, i0:i0 + w] = X.T
    return G


def _phi(X):
    return np.tril(X, -1) + np.diag(0.5 * np.diag(X))


# ---- the fp64 CPU evaluations ------------------------------------------------------------------------------------------------------
def _scalars64(L, z, alpha, Binv, sn2):
    n = L.shape[0]
    nlZ = float(z @ z) / (2.0 * sn2) + float(np.sum(np.log(np.diag(L)))) + 0.5 * n * np.log(2.0 * np.pi * sn2)
    return nlZ, float(np.trace(Binv)) - sn2 * float(alpha @ alpha)


def lapack_fit64(B, r, sn2):
    """The fit by LAPACK: numpy.linalg.cholesky, solve_triangular; alpha by the two substitutions."""
    B, r = _f64(B), _f64(r).ravel()
    n = B.shape[0]
    L = np.linalg.cholesky(B)
    E = np.triu(solve_triangular(L, np.eye(n), lower=True).T)
    Binv = E @ E.T
    z = solve_triangular(L, r, lower=True)
    alpha = solve_triangular(L.T, z, lower=False) / sn2
    nlZ, trQ = _scalars64(L, z, alpha, Binv, sn2)
    return dict(L=L, E=E, Binv=Binv, z=z, alpha=alpha, nlZ=nlZ, trQ=trQ)


def blocked_fit64(B, r, sn2, leaf=LEAF, panel=PANEL, mutant=None):
    """The device's form in numpy fp64: B padded with the identity to a multiple of `leaf`; below it one row r' and the rows of an
    identity ride along and end as z' and E = L^-T.  Right-looking over `panel`-column panels: inside a panel, leaf by leaf, the
    diagonal block is factorised, EXPLICITLY inverted, everything below it multiplied by that inverse and the panel's remaining
    columns updated; behind the panel one trailing update of depth `panel`, and the panel's share E_p E_p' goes into B^-1.
    alpha = E z / sn2 over 128-blocks of z.  mutant: one of MUTANTS, a single slip of that arithmetic (module docstring of
    tests/test_fit_ref_host.py)."""
    assert mutant is None or mutant in MUTANTS
    B, r = _f64(B), _f64(r).ravel()
    n = B.shape[0]
    m = _round_up(n, leaf)
    A = np.zeros((2 * m + 1, m))
    A[:m, :m] = np.eye(m)
    A[:n, :n] = B
    A[m, :n] = r
    A[m + 1:, :] = np.eye(m)
    Binv = np.zeros((m, m))
    starts = list(range(0, m, panel))
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    for p, c0 in enumerate(starts):
        c1 = min(m, c0 + panel)
        for l0 in range(c0, c1, leaf):
            l1 = l0 + leaf
            D = np.linalg.cholesky(A[l0:l1, l0:l1])
            A[l0:l1, l0:l1] = D
            Dinv = np.tril(solve_triangular(D, np.eye(leaf), lower=True))
            below = A[l1:, l0:l1].copy()
            new = below @ Dinv.T
            if mutant == "solve_fp32" and l0 == 0 and m > leaf:                  # the tile below the first leaf, its last k-chunk
                new[:leaf] += f32(below[:leaf, -16:]) @ f32(Dinv[:, -16:]).T - below[:leaf, -16:] @ Dinv[:, -16:].T
            if mutant == "e_unsolved" and l0 == 0:                               # the E rows of leaf 0 keep what they held
                new[m + 1 - l1:m + 1 - l1 + leaf] = below[m + 1 - l1:m + 1 - l1 + leaf]
            A[l1:, l0:l1] = new
            if l1 < c1:
                A[l1:, l1:c1] -= new @ new[:c1 - l1].T
        if c1 < m:
            Y = A[c1:, c0:c1]
            A[c1:, c1:] -= Y @ Y[:m - c1].T
            if mutant == "tu_fp32" and p == 0:                                   # the first trailing tile, the panel's last k-chunk
                Yt = Y[:leaf, -16:]
                A[c1:c1 + leaf, c1:c1 + leaf] -= f32(Yt) @ f32(Yt).T - Yt @ Yt.T
        Ep = A[m + 1:, c0:c1]
        share = Ep @ Ep.T
        if mutant == "eet_last_tile" and c1 == m:                                # the 64-tile in front of the last, ragged one
            t0 = ((n - 1) // 64 - 1) * 64
            share[t0:t0 + 64, t0:t0 + 64] = 0.0
        if mutant == "eet_first_tile" and p == 0 and len(starts) > 1:
            share[0:64, 0:64] = 0.0
        Binv += share
    L = np.tril(A[:n, :n])
    z = A[m, :n].copy()
    E = np.triu(A[m + 1:m + 1 + n, :n])
    zp = A[m, :]
    Ef = A[m + 1:, :]
    nblk, w = m // leaf, leaf
    alpha = np.zeros(m)
    for b in range(nblk - (1 if mutant == "alpha_last_block" else 0)):
        alpha += Ef[:, b * w:(b + 1) * w] @ zp[b * w:(b + 1) * w]
    alpha = alpha[:n] / sn2
    Binv = Binv[:n, :n].copy()
    if mutant == "binv_ragged":                                                  # the last live row read one row further down
        Binv[n - 1, :] = 0.0
        Binv[:, n - 1] = 0.0
        Binv[n - 1, n - 1] = 1.0
    d = np.diag(L)
    if mutant == "logdet_short":
        d = d[:-1]
    nlZ = float(z @ z) / (2.0 * sn2) + float(np.sum(np.log(d))) + 0.5 * n * np.log(2.0 * np.pi * sn2)
    trQ = float(np.trace(Binv)) - sn2 * float(alpha @ alpha)
    return dict(L=L, E=E, Binv=Binv, z=z, alpha=alpha, nlZ=nlZ, trQ=trQ)


CPU_FORMS = ("lapack", "blocked-512", "blocked-128")


def cpu_fits(B, r, sn2):
    """The three fp64 CPU evaluations E_cpu is measured on, in the order of CPU_FORMS."""
    return [lapack_fit64(B, r, sn2), blocked_fit64(B, r, sn2, LEAF, PANEL), blocked_fit64(B, r, sn2, LEAF, LEAF)]


def dense_bar(K, sn2):
    """The rounding bar on B = K / sn2 + I of the dense route at log_sn != 0: exp, the reciprocal and the fma, 3 2^-53 |K| / sn2."""
    return 3.0 * EPS * np.abs(_f64(K)) / float(sn2)


# ---- the full reference -----------------------------------------------------------------------------------------------------------
class FitRef(object):
    """Long-double fit of one (B, r, sn2) and what its tolerance is made of."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def tol(self, field):
        s = self.scale[field]
        return self.bar[field] + (SOLVE_FACTOR * self.e_cpu[field] + FLOOR * EPS) * s

    def errors(self, got, field):
        """|got - reference| / scale (no bar, no factor): the unit of E_cpu."""
        g = np.asarray(got[field], dtype=np.float64)
        want = getattr(self, field)
        err = np.abs(g.astype(LD) - want).astype(np.float64)
        if field == "L":
            err, s = err[self.low], self.scale["L"][self.low]
        else:
            s = self.scale[field]
        return err / s

    def ratios(self, got, fields=None):
        """{field: (worst |got - reference| / tol, index)} over the fields present in got.  A value that is not finite counts
        as infinitely wrong; L is compared on its lower triangle (the caller checks the exact zeros above it)."""
        out = {}
        for f in fields or [f for f in FIELDS if f in got]:
            g = np.asarray(got[f], dtype=np.float64)
            want = getattr(self, f)
            g = g.reshape(np.shape(want))
            tol = self.tol(f)
            err = np.abs(g.astype(LD) - want).astype(np.float64)
            if f == "L":
                err, tol, g = err[self.low], tol[self.low], g[self.low]
            assert np.all(np.asarray(tol) > 0) and np.all(np.isfinite(tol)), f
            rr = np.where(np.isfinite(g), err / tol, np.inf)
            k = int(np.argmax(rr))
            out[f] = (float(np.ravel(rr)[k]), k)
        return out

    # ---- gradient sums ----------------------------------------------------------------------------------------------
    def q_ld(self):
        return self.Binv / LD(self.sn2) - self.alpha[:, None] * self.alpha[None, :]

    def q_tol(self):
        """Per-entry tolerance of Q = Binv / sn2 - alpha alpha' from the tolerances of Binv and alpha."""
        ta = np.broadcast_to(self.tol("alpha"), (self.n,))
        a = np.abs(_f64(self.alpha))
        return self.tol("Binv") / self.sn2 + np.outer(ta, a) + np.outer(a, ta)

    def grad_term(self, dK):
        """(1/2 sum Q o dK in long double, tolerance): the tolerance of Q summed against |dK| plus FLOOR roundings of the terms
        |Binv_ij / sn2| + |alpha_i alpha_j| and of a 256-lane strided sum and its tree (2 + n / 256 + log2(256 n) additions)."""
        dK = _f64(dK)
        n = dK.shape[0]
        val = np.sum(self.q_ld() * _ld(dK)) / 2
        a = np.abs(_f64(self.alpha))
        terms = (np.abs(_f64(self.Binv)) / self.sn2 + np.outer(a, a)) * np.abs(dK)
        depth = 2.0 + n / 256.0 + np.log2(256.0 * n)
        tol = 0.5 * float(np.sum(self.q_tol() * np.abs(dK))) + 0.5 * (FLOOR + depth) * EPS * float(np.sum(terms))
        return val, tol


def ld_fit(B, r, sn2):
    """The long-double quantities alone: dict of L, V = L^-1, E, Binv, z, alpha, nlZ, trQ, logd, const."""
    Bl = _ld(B)
    n = Bl.shape[0]
    L = chol_ld(Bl)
    V = inv_lower_ld(L)
    E = np.ascontiguousarray(V.T)
    Binv = gram_lower_ld(V)
    z = P.forward_ld(L, _ld(r).reshape(n, 1))[:, 0]
    alpha = (E @ z) / LD(sn2)
    logd = np.log(np.diag(L))
    const = LD(n) / 2 * np.log(2 * LD(np.pi) * LD(sn2))
    nlZ = (z @ z) / (2 * LD(sn2)) + np.sum(logd) + const
    trQ = np.trace(Binv) - LD(sn2) * (alpha @ alpha)
    return dict(L=L, V=V, E=E, Binv=Binv, z=z, alpha=alpha, nlZ=nlZ, trQ=trQ, logd=logd, const=const)


def reference(B, r, sn2, barB=None):
    Bl = _ld(B)
    n = Bl.shape[0]
    assert Bl.shape == (n, n)
    r64 = _f64(r).ravel()
    sn2 = float(sn2)
    q = ld_fit(Bl, r64, sn2)
    L, V, E, Binv, z, alpha, nlZ, trQ, logd, const = (q[k] for k in ("L", "V", "E", "Binv", "z", "alpha", "nlZ", "trQ", "logd", "const"))
    # scales (fp64)
    aL, aV = np.abs(_f64(L)), np.abs(_f64(V))
    low = np.tril_indices(n)
    scale = dict(L=aL @ _phi(aV @ (aL @ aL.T) @ aV.T), Binv=aV.T @ aV, alpha=float(np.max(np.abs(_f64(alpha)))),
                 nlZ=float((z @ z) / (2 * LD(sn2)) + np.sum(np.abs(logd)) + np.abs(const)),
                 trQ=float(np.trace(np.abs(Binv)) + LD(sn2) * (alpha @ alpha)))
    aB, aa = np.abs(_f64(Binv)), np.abs(_f64(alpha))
    if barB is None:
        bar = dict(L=0.0, Binv=0.0, alpha=0.0, nlZ=0.0, trQ=0.0)
    else:
        bb = _f64(barB)
        assert bb.shape == (n, n) and np.all(bb >= 0)
        Q = np.abs(_f64(Binv / LD(sn2) - alpha[:, None] * alpha[None, :]))
        b_inv, b_al = aB @ bb @ aB, aB @ (bb @ aa)
        bar = dict(L=aL @ _phi(aV @ bb @ aV.T), Binv=b_inv, alpha=b_al, nlZ=0.5 * float(np.sum(Q * bb)) * sn2,
                   trQ=float(np.trace(b_inv)) + 2.0 * sn2 * float(aa @ b_al))
    ref = FitRef(n=n, sn2=sn2, r=r64, B=Bl, L=L, E=E, Binv=Binv, z=z, alpha=alpha, nlZ=nlZ, trQ=trQ, scale=scale, bar=bar, low=low,
                 barB=None if barB is None else _f64(barB), e_cpu=dict.fromkeys(FIELDS, 0.0), e_cpu_form={})
    # E_cpu: the three fp64 CPU evaluations of the same B
    B64 = _f64(Bl)
    for name, fit in zip(CPU_FORMS, cpu_fits(B64, r64, sn2)):
        ref.e_cpu_form[name] = {f: float(np.max(ref.errors(fit, f))) for f in FIELDS}
    ref.e_cpu = {f: max(v[f] for v in ref.e_cpu_form.values()) for f in FIELDS}
    return ref


_CACHE = {}


def _key(tag, arrays, scalars):
    h = hashlib.blake2b(repr((tag, scalars)).encode(), digest_size=16)
    for a in arrays:
        if a is None:
            h.update(b"none")
            continue
        a = np.ascontiguousarray(a)
        h.update(repr((a.shape, str(a.dtype))).encode())
        h.update(memoryview(a).cast("B"))
    return h.digest()


def cached(B, r, sn2, barB=None):
    """reference(...) once per distinct set of inputs: option variants of one matrix share a reference."""
    key = _key("full", (B, r, barB), float(sn2))
    if key not in _CACHE:
        _CACHE[key] = reference(B, r, sn2, barB)
    return _CACHE[key]


def program_b(kind, hyp, para, x, sn2):
    """(B, barB) of the program route: B = K / sn2 + I in long double from kernel_ref_ld.ref_matrix, barB = its fp64 bar divided by
    sn2 plus dense_bar (the scaling and the fma)."""
    import kernel_ref_ld as KR
    K, barK = KR.ref_matrix(kind, hyp, para, x=np.asarray(x, dtype=np.float64), mode="train")
    B = K / LD(sn2)
    B[np.diag_indices_from(B)] += 1
    return B, np.asarray(barK, dtype=np.float64) / float(sn2) + dense_bar(K, sn2)


def dnlz_reference(ref, kind, hyp, para, x, **kw):
    """(values, tolerances) of [dnlZ.cov ..., dnlZ.lik] of an exact fit: kernel_ref_ld.hadamard_ref on the reference B^-1 and alpha
    (sums / 2 for the covariance hypers, sn2 tr Q last), its own bar plus sum_ij tol_Binv,ij |dK_h,ij| (the last hyper's
    dK = sn2 I: sn2 tr tol_Binv).  kw: hadamard_ref's compat / gram / centred."""
    import kernel_ref_ld as KR
    x = np.asarray(x, dtype=np.float64)
    sums, bars, dks = KR.hadamard_ref(kind, hyp, para, x, ref.Binv, ref.alpha, sn2=ref.sn2, return_dks=True, **kw)
    tb = ref.tol("Binv")
    nh = len(sums) - 1
    tol = np.array(bars, dtype=np.float64)
    for h in range(nh):
        tol[h] += float(np.sum(tb * np.abs(dks[h]).astype(np.float64)))
    tol[nh] += ref.sn2 * float(np.trace(tb))
    vals = np.array(sums, dtype=LD)
    vals[:nh] /= 2
    tol[:nh] /= 2
    return vals, tol


# ---- large n: functionals of the downloaded outputs ---------------------------------------------------------------------------
def default_probes(n, seed=0):
    """Columns / rows probed: 0, 127, 128, 511, 512, 513, the first and the last row of the last panel, n - 1 and two random."""
    last0 = (_round_up(n, LEAF) - 1) // PANEL * PANEL
    rng = np.random.RandomState(seed + n)
    p = [0, 127, 128, 511, 512, 513, last0, n - 1] + list(rng.randint(0, n, 2))
    return sorted(set(int(i) for i in p if 0 <= i < n))


def nlz_ld(L, r, sn2):
    """(nlZ, its sum of absolute terms) in long double from a factor L: z = L^-1 r by forward substitution."""
    Ll = _ld(L)
    n = Ll.shape[0]
    z = P.forward_ld(Ll, _ld(r).reshape(n, 1))[:, 0]
    logd = np.log(np.diag(Ll))
    const = LD(n) / 2 * np.log(2 * LD(np.pi) * LD(sn2))
    q = (z @ z) / (2 * LD(sn2))
    return q + np.sum(logd) + const, float(q + np.sum(np.abs(logd)) + np.abs(const))


def functionals(Bl, aB, r, sn2, fit, probes, barB=None):
    """{name: (residuals, scales, bars)} of one fit (dict with L, Binv, alpha, nlZ; fp64) against the long-double B (aB = |B| in
    fp64); arrays over the probed entries."""
    n = Bl.shape[0]
    L, Binv, alpha = _f64(fit["L"]), _f64(fit["Binv"]), _f64(fit["alpha"]).ravel()
    Ll, aL, aBi = _ld(L), np.abs(L), np.abs(Binv)

    def col(j):
        res = np.abs(Bl[:, j] - Ll[:, :j + 1] @ Ll[j, :j + 1]).astype(np.float64)
        return res, aL[:, :j + 1] @ aL[j, :j + 1], (barB[:, j] if barB is not None else np.zeros(n))

    def row(i):
        e = np.zeros(n, dtype=LD)
        e[i] = 1
        res = np.abs(_ld(Binv[i]) @ Bl - e).astype(np.float64)
        return res, aBi[i] @ aB, (aBi[i] @ barB if barB is not None else np.zeros(n))
    out = {}
    for name, fn in (("resid_col", col), ("left_inv_row", row)):
        parts = _pmap(fn, probes)
        out[name] = tuple(np.concatenate([p[k] for p in parts]) for k in range(3))
    x = sn2 * alpha
    out["solve_resid"] = (np.abs(Bl @ _ld(x) - _ld(r)).astype(np.float64), aB @ np.abs(x),
                          barB @ np.abs(x) if barB is not None else np.zeros(n))
    v = np.random.RandomState(n).choice([-1.0, 1.0], size=n)              # every tile of B^-1 at once: |Binv (B v) - v|
    one = np.ones(n)
    out["inv_vec"] = (np.abs(_ld(Binv) @ (Bl @ _ld(v)) - _ld(v)).astype(np.float64), aBi @ (aB @ one),
                      aBi @ (barB @ one) if barB is not None else np.zeros(n))
    ref, sabs = nlz_ld(L, r, sn2)
    bar_nlz = 0.0
    if barB is not None:
        bar_nlz = 0.5 * sn2 * float(np.sum(np.abs(Binv / sn2 - np.outer(alpha, alpha)) * barB))
    out["nlZ"] = (np.array([abs(float(LD(float(fit["nlZ"])) - ref))]), np.array([sabs]), np.array([bar_nlz]))
    return out


LARGE_FIELDS = ("resid_col", "left_inv_row", "inv_vec", "solve_resid", "nlZ")


class LargeRef(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def large_reference(B64, r, sn2, probes=None):
    """E_cpu of the four functionals on the three fp64 CPU fits of B64 (fp64, the matrix itself: the CPU fits see no bar)."""
    B64 = _f64(B64)
    n = B64.shape[0]
    probes = default_probes(n) if probes is None else list(probes)
    Bl, aB = _ld(B64), np.abs(B64)
    forms = {}
    for name, fit in zip(CPU_FORMS, cpu_fits(B64, r, sn2)):
        fv = functionals(Bl, aB, r, sn2, fit, probes)
        forms[name] = {k: float(np.max(v[0] / v[1])) for k, v in fv.items()}
    e_cpu = {k: max(v[k] for v in forms.values()) for k in LARGE_FIELDS}
    return LargeRef(n=n, sn2=float(sn2), r=_f64(r).ravel(), probes=probes, e_cpu=e_cpu, e_cpu_form=forms)


def large_cached(B64, r, sn2, probes=None):
    key = _key("large", (B64, r, None if probes is None else np.asarray(probes)), float(sn2))
    if key not in _CACHE:
        _CACHE[key] = large_reference(B64, r, sn2, probes)
    return _CACHE[key]


def large_ratios(lref, Bl, fit, barB=None, aB=None):
    """{name: worst residual / (bar + (SOLVE_FACTOR E_cpu + FLOOR 2^-53) scale)} of a device fit against the long-double B it
    was meant to factorise (Bl; barB: the rounding bar of the device's own B against it)."""
    Bl = _ld(Bl)
    aB = np.abs(_f64(Bl)) if aB is None else aB
    fv = functionals(Bl, aB, lref.r, lref.sn2, fit, lref.probes, None if barB is None else _f64(barB))
    out = {}
    for k, (res, sc, bar) in fv.items():
        tol = bar + (SOLVE_FACTOR * lref.e_cpu[k] + FLOOR * EPS) * sc
        assert np.all(tol > 0)
        finite = np.isfinite(res)
        out[k] = float(np.max(np.where(finite, res / tol, np.inf)))
    return out


# ---- input recipes shared by the host test and the GPU test ----------------------------------------------------------------------
def rbf_matrix(n, d, seed=None, sf2=np.exp(0.2)):
    """(x, y, K): the suite's synthetic regression data (conftest.synth_reg's recipe) and its RBF matrix at ell = sqrt(d) in plain
    fp64 numpy.  K / 0.01 + I has cond ~ 1e4 (n = 700, d = 5: 4e4)."""
    x, y = P.reg_data(n, d, n if seed is None else seed)
    sq = np.sum(x * x, axis=1)
    D2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * (x @ x.T), 0.0)
    D2 = 0.5 * (D2 + D2.T)
    np.fill_diagonal(D2, 0.0)
    return x, y, sf2 * np.exp(-0.5 * D2 / d)


def sorted_1d_matrix(n, cond=1e6, seed=3):
    """(t, y, K): the RBF matrix (ell = 0.05) of n sorted points of [0, 1], strongly correlated neighbours, scaled so that K + I has
    cond ~ `cond` (lambda_max(K) ~ 0.125 n amp)."""
    rng = np.random.RandomState(seed + n)
    t = np.sort(rng.rand(n))
    amp = cond / (0.125 * n)
    K = amp * np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2 / 0.05 ** 2)
    y = np.sin(6.0 * t) + 0.1 * rng.randn(n)
    return t, y, 0.5 * (K + K.T)
