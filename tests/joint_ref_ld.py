"""Long-double reference of the joint posterior covariance GP.predict_joint forms (csrc/joint.hip), with a per-entry tolerance
computed from the reference side only, and the checks of its Cholesky factor and of the draws (test infrastructure, CPU only).

    reference(spec, hyp, x, xs, ms, alpha, sW, R) -> JointRef        built on predict_ref_ld.reference (its Ref holds V, Ks, barK, L, sW)
    check_joint(fmu, fcov, ref) -> (worst ratio, (field, index))     the unit the tests assert <= 1 in
    chol_residual(Lc, A), draws_excess(F, fmu, Lc, z)                 the factor and the draws, each against its own bound

    Kss  = k(xs, xs) in 'train' mode, its diagonal from 'self_test'   (kernel_ref_ld / dot_ref_ld through predict_ref_ld._cov_ld)
    fcov = Kss - V'V,  diagonal clipped at 0                          V = L^-1 (sW o Ks) from the Ref

Tolerance of entry (i, j), the recipe of predict_ref_ld's fs2:  tol_ij = T_ij + SOLVE_FACTOR E_cpu + floor_ij

  * T_ij = barKss_ij + sum_k |V_ki| G_kj + sum_k |V_kj| G_ki,  G = |L^-1| (sW o barK): the kernel bars to first order;
  * E_cpu: the larger max-abs error, over the case's entries, of two fp64 CPU evaluations against long double --
    solve_triangular + V.T @ V and inv(L) @ B + V.T @ V -- of which the device gets SOLVE_FACTOR = 8 times;
  * floor_ij = 4 * 2^-53 * sqrt(kss_i kss_j).

Rows and columns (test points) are independent: `take(idx)` selects the points of one case, E_cpu is then taken over them.
"""
import hashlib

import numpy as np

import predict_ref_ld as P

LD = P.LD
EPS = P.EPS
SOLVE_FACTOR = P.SOLVE_FACTOR
FLOOR = P.FLOOR


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def gram_ld(V, W=None, block=256):
    """V' W in long double (W = V: symmetric, the lower blocks computed and mirrored)."""
    V = np.asarray(V, dtype=LD)
    sym = W is None
    W = V if sym else np.asarray(W, dtype=LD)
    m, p = V.shape[1], W.shape[1]
    out = np.zeros((m, p), dtype=LD)
    Vt = np.ascontiguousarray(V.T)
    for a in range(0, m, block):
        hi = min(a + block, m) if sym else p
        out[a:a + block, :hi] = Vt[a:a + block] @ W[:, :hi]
    if sym:
        il = np.tril_indices(m, -1)
        out.T[il] = out[il]
    return out


def cpu_joint(L, sW, Ks, Kss, kss, form="solve", scale=None):
    """fcov in fp64 from fp64 inputs: Kss (its diagonal replaced by kss) - V'V, diagonal clipped; returns (fcov, V)."""
    L = np.asarray(L, dtype=np.float64)
    B = (np.asarray(sW, dtype=np.float64).reshape(-1, 1) if scale is None else 1.0) * Ks
    if form == "solve":
        V = P.solve_triangular(L, B, lower=True)
    else:
        V = np.tril(np.linalg.inv(L)) @ B
    return finish64(Kss, kss, V.T @ V * (1.0 if scale is None else scale)), V


def finish64(Kss, kss, VtV):
    C = np.array(Kss, dtype=np.float64)
    ns = C.shape[0]
    C[np.diag_indices(ns)] = kss
    C = C - VtV
    C[np.diag_indices(ns)] = np.maximum(C.diagonal(), 0.0)
    return C


class JointRef(object):
    MATS = ("Kss", "barKss", "fcov", "T", "Kss64")

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def ns(self):
        return self.fcov.shape[0]

    def take(self, idx):
        idx = np.asarray(idx)
        kw = dict(self.__dict__)
        kw["pref"] = self.pref.take(idx)
        for k in self.MATS:
            kw[k] = getattr(self, k)[np.ix_(idx, idx)]
        kw["cpu"] = self.cpu[:, idx][:, :, idx]
        return JointRef(**kw)

    def e_cpu(self):
        return float(np.max(self.cpu))

    def tol(self):
        kss = self.pref.kss.astype(np.float64)
        return self.T + SOLVE_FACTOR * self.e_cpu() + FLOOR * EPS * np.sqrt(np.outer(kss, kss))


def reference(spec, hyp, x, xs, ms, alpha, sW, R):
    pref = P.cached(spec, hyp, x, xs, ms, alpha, sW, R)
    xs = np.asarray(xs, dtype=np.float64)
    ns = xs.shape[0]
    sW = np.asarray(sW, dtype=np.float64).reshape(-1)
    Kss, barKss = P._cov_ld(spec, hyp, xs, None, "train")
    Kss = np.array(Kss, dtype=LD)
    barKss = np.array(barKss, dtype=np.float64)
    dg = np.diag_indices(ns)
    Kss[dg] = pref.kss
    barKss[dg] = np.asarray(P._cov_ld(spec, hyp, None, xs, "self_test")[1], dtype=np.float64).reshape(ns)
    fcov = Kss - gram_ld(pref.V)
    fcov[dg] = np.maximum(fcov[dg], LD(0))
    n = pref.L.shape[0]
    absLinv = np.abs(np.tril(P.solve_triangular(pref.L, np.eye(n), lower=True)))
    G = absLinv @ (sW[:, None] * pref.barK)
    H = np.abs(pref.V).astype(np.float64).T @ G
    T = barKss + H + H.T
    Kss64 = np.array(P._cov64(spec, hyp, xs, None, "train"), dtype=np.float64)
    cpu = np.empty((2, ns, ns))
    for k, form in enumerate(("solve", "inverse")):
        C, _ = cpu_joint(pref.L, sW, pref.Ks64, Kss64, pref.kss64, form)
        cpu[k] = np.abs(C.astype(LD) - fcov).astype(np.float64)
    return JointRef(pref=pref, Kss=Kss, barKss=barKss, fcov=fcov, T=T, Kss64=Kss64, cpu=cpu)


_CACHE = {}


def cached(spec, hyp, x, xs, ms, alpha, sW, R):
    h = hashlib.blake2b(repr(spec).encode(), digest_size=16)
    for a in (hyp, x, xs, ms, alpha, sW, R):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
        h.update(repr(a.shape).encode())
        h.update(memoryview(a).cast("B"))
    key = h.digest()
    if key not in _CACHE:
        _CACHE[key] = reference(spec, hyp, x, xs, ms, alpha, sW, R)
    return _CACHE[key]


def ratios(fmu, fcov, ref):
    """{"fmu": (worst, j), "fcov": (worst, (i, j))}: per field the largest |value - reference| / tol and where it sits."""
    fmu = np.asarray(fmu, dtype=np.float64).reshape(-1)
    fcov = np.asarray(fcov, dtype=np.float64)
    assert fmu.shape == (ref.ns,) and fcov.shape == (ref.ns, ref.ns), (fmu.shape, fcov.shape)
    t_mu = ref.pref.tol()[0]
    tol = ref.tol()
    assert np.all(tol > 0) and np.all(np.isfinite(tol)) and np.all(t_mu > 0)
    r1 = np.abs(fmu.astype(LD) - ref.pref.fmu).astype(np.float64) / t_mu
    r1 = np.where(np.isfinite(fmu), r1, np.inf)
    r2 = np.abs(fcov.astype(LD) - ref.fcov).astype(np.float64) / tol
    r2 = np.where(np.isfinite(fcov), r2, np.inf)
    j = int(np.argmax(r1))
    ij = tuple(int(v) for v in np.unravel_index(int(np.argmax(r2)), r2.shape))
    return {"fmu": (float(r1[j]), j), "fcov": (float(r2[ij]), ij)}


def check_joint(fmu, fcov, ref):
    r = ratios(fmu, fcov, ref)
    name = max(r, key=lambda k: r[k][0])
    return r[name][0], (name, r[name][1])


# ---- the Cholesky factor and the draws --------------------------------------------------------------------------------------------
def chol_residual(Lc, A):
    """r = max_ij |Lc Lc' - A|_ij / (|Lc| |Lc|')_ij in long double (the componentwise backward error of a Cholesky factor)."""
    Lc = np.asarray(Lc, dtype=np.float64)
    Ll = Lc.astype(LD)
    LLt = gram_ld(np.ascontiguousarray(Ll.T))
    den = np.abs(Lc) @ np.abs(Lc).T
    return float(np.max(np.abs(LLt - np.asarray(A, dtype=np.float64).astype(LD)).astype(np.float64) / den))


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


def draws_excess(F, fmu, Lc, z):
    """max_ij |F - ref|_ij / bound_ij with ref = fmu 1' + Lc z in long double and the order-independent dot-product bound
    bound_ij = gamma_(ns+1) (|Lc| |z|)_ij + 2 * 2^-53 |ref_ij|."""
    Lc, z = np.asarray(Lc, dtype=np.float64), np.asarray(z, dtype=np.float64)
    ns = Lc.shape[0]
    ref = _ld(fmu).reshape(ns, 1) + gram_ld(np.ascontiguousarray(Lc.astype(LD).T), z.astype(LD))
    bound = gamma(ns + 1) * (np.abs(Lc) @ np.abs(z)) + 2.0 * EPS * np.abs(ref).astype(np.float64)
    F = np.asarray(F, dtype=np.float64)
    assert F.shape == ref.shape
    err = np.abs(F.astype(LD) - ref).astype(np.float64)
    err = np.where(np.isfinite(F), err, np.inf)
    return float(np.max(err / np.where(bound > 0, bound, 1.0) * np.where((bound > 0) | (err == 0), 1.0, np.inf)))


# ---- input recipes shared by the host test and the GPU test ---------------------------------------------------------------------
from oracle import gp_oracle as O  # noqa: E402

LOG_ELL3 = float(np.log(np.sqrt(3.0)))
LOG_ELL17 = float(np.log(np.sqrt(17.0)))
ARD3 = ("sum", ("sum", ("leaf", O.RBFARD, 0), ("leaf", O.RBFARD, 0)), ("leaf", O.RBFARD, 0))
ARD3_HYP = [0.5, 0.6, 0.4, -0.5, 0.7, 0.5, 0.6, -0.5, 0.4, 0.7, 0.5, -0.5]
SUM_PER = ("sum", ("leaf", O.RBF, 0), ("prod", ("leaf", O.PERIODIC, 0), ("leaf", O.RBF, 0)))
SUM_PER_HYP = [0.0, 0.0, 0.0, 0.5, -0.5, 0.7, 0.0]       # RBF(ell, sf) + Periodic(ell, p, sf) * RBF(ell, sf), 1-d inputs
LIN_RBF = ("sum", ("leaf", "linear", 0), ("leaf", "rbf", 0))
RBF_NOISE = ("sum", ("leaf", O.RBF, 0), ("leaf", O.NOISE, 0))       # Noise: sf2 I on 'train', 0 on 'self_test'
LIN_RBF_HYP = [-1.0, LOG_ELL3, 0.0]

# name -> (kind of model, spec, hyp, d, n, size of the pool of test points, data seed)
MODELS = {
    "rbf130": ("gpr", ("oracle", O.RBF, 0), [LOG_ELL3, 0.0], 3, 130, 300, 141),
    "rbf300": ("gpr", ("oracle", O.RBF, 0), [LOG_ELL3, 0.0], 3, 300, 300, 311),
    "rbf1100": ("gpr", ("oracle", O.RBF, 0), [LOG_ELL3, 0.0], 3, 1100, 1153, 1111),
    "rbfard17": ("gpr", ("oracle", O.RBFARD, 0), [LOG_ELL17] * 17 + [0.5], 17, 300, 129, 17),
    "sum_per": ("gpr", ("oracle", SUM_PER, 0), SUM_PER_HYP, 1, 300, 129, 18),
    "lin_rbf1100": ("gpr", ("dot", LIN_RBF), LIN_RBF_HYP, 3, 1100, 300, 13),
    "ep300": ("gpc_ep", ("oracle", O.MATERN, 3), [0.0, 0.0], 2, 300, 129, 3),
    "lap300": ("gpc_laplace", ("oracle", O.RBFARD, 0), [LOG_ELL17] * 17 + [0.5], 17, 300, 129, 4),
    "liklap300": ("gpr_liklaplace", ("oracle", O.RBF, 0), [LOG_ELL3, 0.0], 3, 300, 129, 15),
    "dense300": ("gpr", ("oracle", ARD3, 0), ARD3_HYP, 3, 300, 129, 14),
    "rbf_noise300": ("gpr", ("oracle", RBF_NOISE, 0), [LOG_ELL3, 0.0, -1.0], 3, 300, 129, 19),
}
# (model, ns): the fcov cases of the GPU module; the host module runs the fp64 CPU evaluation on every one of them
FCOV_CASES = ([("rbf%d" % n, ns) for n in (130, 300, 1100) for ns in (1, 127, 129, 300)] + [("rbf1100", 1153)] +
              [("rbfard17", 129), ("sum_per", 129), ("lin_rbf1100", 300), ("ep300", 129), ("lap300", 129), ("liklap300", 129),
               ("dense300", 129), ("rbf_noise300", 129)])
LIK_LAPLACE_LOG_SN = float(np.log(0.1))


def model_data(name):
    """x, y, xs (the pool), ms (prior mean at the pool, flat), m (prior mean at x, column) of a model."""
    kind, spec, hyp, d, n, nmax, seed = MODELS[name]
    if kind.startswith("gpc"):
        x, y = P.cls_data(n, d, seed, island=6.0 if kind == "gpc_ep" else 0.0)
    else:
        x, y = P.reg_data(n, d, seed)
    xs = P.make_points(x, nmax, seed=100 + n)
    lin = P.MEAN_W_ISLAND if kind == "gpc_ep" else False
    return x, y, xs, P.mean_values(xs, lin).ravel(), P.mean_values(x, lin)


# (model, ns, noise): the Cholesky cases; (model, ns, nsamp): the draw cases.  Their test points are a pool of their own without
# the points at |x| = 50: covariances that have underflowed into the subnormal range (1e-320) carry a few bits, and a componentwise
# residual relative to |Lc| |Lc|' measures that instead of the factorisation.
CHOL_CASES = [("rbf300", 129, True), ("rbf300", 300, True), ("rbf1100", 1153, True), ("rbf300", 300, False)]
DRAW_CASES = [("rbf300", 129, 1), ("rbf300", 300, 5), ("rbf1100", 1153, 130)]


def chol_points(name, ns):
    """ns test points for the factor and the draws of a model: a third near training points, one exact copy, the rest randn; the
    three outliers at |x| = 3."""
    return P.make_points(model_data(name)[0], ns, seed=200 + ns, far=3.0)
