"""Leave-one-out inference on the device (csrc/loo.hip, pgp_loo_fit / pgp_loo_fit_dense, inf.LOO, GPR.predict_loo,
valid.loo_validation) against the long-double reference of tests/loo_ref_ld.py, in units of its tolerance (<= 1 asserted).

Inputs are well conditioned: sf = 1, sn = 0.2 (0.1 ... 0.3 in the kernel cases), x standard normal.  The reference starts from
the fp64 matrix the device factorises: on the dense route the K handed in (bar: fit_ref_ld.dense_bar, the scaling by 1 / sn2 and
the fma), on the program route the long-double kernel matrix with the bar of an fp64 evaluation (kernel_ref_ld / dot_ref_ld).
cov.SM and cov.Pre have no long-double kernel reference in this suite: their reference matrix is the package's own fp64
getCovMatrix with the relative bar kernel_ref_ld gives any fp64 kernel entry (its safety factor C = 16 roundings) on top of
dense_bar -- the fit's tile assembly and getCovMatrix evaluate the same functor, entry by entry, in fp64.

The gradient is pinned in two stages: S = sn2 Q_loo entry by entry (pgp_test_read_binv reads c->Binv, which holds S after a LOO
fit with gradients; its padding rows must be exact zeros), and the sums given S -- fit_ref_ld.dnlz_reference on the reference's S
for the kernels kernel_ref_ld covers, else 1/2 sum(S o dK_h) / sn2 in long double with the same bar (grad_sums below).

want = 2 and want = 3 read diag(B^-1) off the same row sums of squares of the fused inverse rows: their values are compared BIT
FOR BIT (with fused_inverse 0 both take the triangular inverse + W'W and read its diagonal: bit for bit again).  The posterior of a
LOO fit is the exact fit's bit for bit where both take the same route to alpha -- always at want = 3, and at want = 2 with the
fused inverse; a want = 2 LOO call WITHOUT it takes want = 3's route (alpha = W'z), an Exact want = 2 call the blocked
back-substitution, and the two alphas then agree to rounding only (test_value_only_posterior_without_the_fused_inverse).

Worst |device - reference| / tolerance, from the MI355X run of this module on 2026-10-20 (-s prints every case):

    A  dense route, n = 1 ... 641    alpha 0.10 (n = 1)  mu 0.13 (n = 1)  s2 0.092 (n = 641, 64-tiles)  lp 0.069 (n = 2)  nlZ 0.036
                                     u 0.068  S 0.075  tr S 0.075  grad terms 0.038 -- all at n = 1, where E_cpu is a fraction of an
                                     ulp; from n = 63 every field is <= 0.061 (n = 641: alpha 0.033 mu 0.031 s2 0.061 lp 0.031
                                     nlZ 0.0034 u 0.014 S 0.012 tr S 0.00024 grad 7.8e-5); n = 129: both tile sizes the same bits;
                                     n = 641, 64-tiles / 128-tiles: S 0.013 / 0.012, s2 0.092 / 0.061
    A' program route, n = 1 ... 641  alpha 0.012  mu 0.0070  s2 0.026 (n = 641, 64-tiles)  lp 0.021  nlZ 0.024  S 0.011  tr S 0.011
                                     dcov 0.026  dlik sum 0.049  dmean 0.0036 -- all but s2 at n = 1 or 2; n = 641: alpha 0.0030 mu 0.0028
                                     s2 0.016 lp 0.0030 nlZ 0.00016 S 0.00094 dcov 3.1e-9 dlik sum 0.00021; n = 129: both tile sizes the
                                     same bits; n = 641, 64-tiles / 128-tiles: S 0.00096 / 0.00094
    B  kernels, n = 129 and 385      S <= 0.0013, dcov <= 1.8e-6 (matern3_d3, n = 129), dlik sum <= 0.0010, dmean <= 1.6e-5 (three_ard);
                                     rbfard_d5 form 2: alpha 0.00089 mu 0.00085 s2 0.0036 lp 0.00092 nlZ 0.00035 S 0.00027 (n = 129)
    C  means                         dmean_h <= 3.3e-6 (mean.Linear)
    E  padding, n = 129              S 0.0013 and tr S 5.2e-5 on both routes; the padding rows of S are exact zeros in every case
    E  want = 2, fused_inverse 0     alpha of LOO (= Exact's want = 3 alpha, bit for bit) 0.0013, of Exact's back-substitution 0.0013
    want = 2 against want = 3: the same bits on both routes, with the fused inverse and without it.

The program route sits three orders of magnitude below its tolerance because the bar of an fp64 kernel evaluation, carried through
two inverses, is a worst case the errors do not approach; the dense route, where B is exact, sits at 0.01 ... 0.1.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import dot_ref_ld as D
import kernel_ref_ld as KR
import loo_ref_ld as R
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu
F = R.F
LD = R.LD
DEFAULTS = dict(small_tile_below=200, fused_inverse=1, fused_value_max_np=12288, ard_grad_form=0)
SN = 0.2
LOG_SN = float(np.log(SN))
SN2 = float(np.exp(2.0 * LOG_SN))
WORST = {}


@contextlib.contextmanager
def _options(lib, **kw):
    from pygps_amd import _lib
    ctx = _lib.ctx()
    try:
        for k, v in kw.items():
            _lib.check(lib.pgp_set_option(ctx, k.encode(), int(v)))
        yield
    finally:
        for k in kw:
            lib.pgp_set_option(ctx, k.encode(), DEFAULTS[k])


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    for f in sorted(set(f for _, f in WORST)):
        print("loo worst %-12s %.3g  (%s)" % ((f,) + max((r, c) for (c, ff), r in WORST.items() if ff == f)))


def _record(case, rr):
    for f, v in rr.items():
        WORST[(case, f)] = max(WORST.get((case, f), 0.0), v)
    print("loo %-44s %s" % (case, "  ".join("%s %.3g" % (f, v) for f, v in rr.items())))
    bad = {f: v for f, v in rr.items() if not v <= 1.0}
    assert not bad, (case, bad)


def _data(n, d, seed=0):
    rng = np.random.RandomState(1000 * d + n + seed)
    x = rng.randn(n, d)
    y = np.sin(x.sum(axis=1)) + SN * rng.randn(n) + 0.7
    return x, y


def _read_s(lib, n):
    """(S on the live rows, mirrored; the padding rows of the workspace): pgp_test_read_binv at n, and at np for the padding."""
    from pygps_amd import _lib
    out = np.full((n, n), np.nan)
    _lib.check(lib.pgp_test_read_binv(_lib.ctx(), n, _lib.ptr(out)), "pgp_test_read_binv")
    m = (n + 127) // 128 * 128
    full = np.full((m, m), np.nan)
    _lib.check(lib.pgp_test_read_binv(_lib.ctx(), m, _lib.ptr(full)), "pgp_test_read_binv")
    return out, full[n:, :].copy()


def _dense_loo(lib, K, r, log_sn, want, read_s=True):
    from pygps_amd import _lib
    ctx = _lib.ctx()
    n = K.shape[0]
    K, r = np.ascontiguousarray(K), np.ascontiguousarray(r)
    alpha, mu, s2, lp, u = (np.full(n, np.nan) for _ in range(5))
    nlz, glik = np.zeros(2), np.zeros(1)
    fh = C.c_void_p()
    _lib.check(lib.pgp_loo_fit_dense(ctx, _lib.ptr(K), n, _lib.ptr(r), float(log_sn), want, _lib.ptr(alpha), _lib.ptr(mu),
                                     _lib.ptr(s2), _lib.ptr(lp), _lib.ptr(nlz), _lib.ptr(glik), _lib.ptr(u), C.byref(fh)),
               "pgp_loo_fit_dense")
    lib.pgp_factor_free(ctx, fh)
    got = dict(alpha=alpha, mu=mu, s2=s2, lp=lp, nlZ=float(nlz[0]), marginal=float(nlz[1]))
    if want >= 3:
        got.update(u=u, dlik=float(glik[0]))
        if read_s:
            got["S"], got["Spad"] = _read_s(lib, n)
    return got


def grad_sums(ref, dks):
    """[(1/2 sum(S o dK_h) / sn2 in long double, tolerance)] for (dK_h, bar_h) pairs: the tolerance of S summed against |dK_h|, the
    bar of dK_h summed against |S|, and kernel_ref_ld.hadamard_ref's C EPS L sum |S o dK_h| for the device's reduction tree."""
    S, tS = ref.val["S"], ref.tol("S")
    aS = np.abs(F._f64(S))
    L = 2.0 + np.log2(float(ref.n) ** 2)
    out = []
    for dK, bK in dks:
        a = np.abs(F._f64(dK))
        tol = (float(np.sum(tS * a)) + float(np.sum(aS * bK)) + KR.C * KR.EPS * L * float(np.sum(aS * a))) / (2 * ref.sn2) + KR.TINY
        out.append((np.sum(S * F._ld(dK)) / (2 * LD(ref.sn2)), tol))
    return out


def _sum_ratios(got, want):
    return max(abs(float(LD(float(g)) - v)) / t if np.isfinite(g) else np.inf for g, (v, t) in zip(got, want))


# ---- A: sizes across the edges (dense route: B from the K handed in) -----------------------------------------------------------
_DENSE = {}


def _dense_case(n):
    if n not in _DENSE:
        x, y = _data(n, 3)
        sq = np.sum(x * x, axis=1)
        K = np.exp(-0.5 * np.maximum(sq[:, None] + sq[None, :] - 2.0 * (x @ x.T), 0.0) / 3.0)
        K = 0.5 * (K + K.T)
        np.fill_diagonal(K, 1.0)
        r = y - 0.7
        B = F._ld(K) / LD(SN2)
        B[np.diag_indices(n)] += 1
        _DENSE[n] = (K, r, R.cached(B, r, SN2, None, F.dense_bar(K, SN2)))
    return _DENSE[n]


def _dense_dks(n):
    rng = np.random.RandomState(n)
    G = rng.randn(n, n)
    edge = np.zeros((n, n))
    i, j = (64, 63) if n > 64 else (n - 1, 0)
    edge[i, j] = edge[j, i] = -0.75
    return [np.ascontiguousarray(G + G.T), edge]


SIZES = [(n, None) for n in (1, 2, 63, 64, 65, 127, 128, 129, 257, 385, 641)] + [(129, 1), (129, 10 ** 6), (641, 1), (641, 10 ** 6)]


@pytest.mark.parametrize("n,small", SIZES)
def test_sizes_across_the_edges(lib, n, small):
    from pygps_amd import _lib
    K, r, ref = _dense_case(n)
    case = "A dense n=%d%s" % (n, "" if small is None else " small_tile_below=%d" % small)
    print("loo %-44s E_cpu / 2^-53: %s" % (case, "  ".join("%s %.3g" % (f, v / R.EPS) for f, v in ref.e_cpu.items())))
    with _options(lib, **({} if small is None else dict(small_tile_below=small))):
        got = _dense_loo(lib, K, r, LOG_SN, 3)
        g, sums = np.zeros(1), []
        dks = _dense_dks(n)
        for dK in dks:
            _lib.check(lib.pgp_dense_grad_term(_lib.ctx(), _lib.ptr(dK), n, LOG_SN, _lib.ptr(g)), "pgp_dense_grad_term")
            sums.append(float(g[0]))
    rr = ref.ratios(got)
    rr["grad"] = _sum_ratios(sums, grad_sums(ref, [(dK, 0.0) for dK in dks]))
    _record(case, rr)


# ---- B: kernels (program route through inf.LOO; the three-ARD tree takes the dense route) ---------------------------------------
def _leaf(kind, para=0):
    return ("leaf", kind, para)


def _kernel_case(name, n):
    """(covfunc, x, y, (B, barB), kr) -- kr: (kind, hyp, para) for kernel_ref_ld, or None; dks: callable h -> (dK_h, bar_h)."""
    from pygps_amd import cov
    if name == "rbf_d1":
        x, y = _data(n, 1)
        hyp = np.array([0.1, 0.0])
        k = cov.RBF(hyp[0], hyp[1])
        kr = (O.RBF, hyp, 0)
    elif name == "rbfard_d5":
        x, y = _data(n, 5)
        hyp = np.array([0.75, 0.85, 0.8, 0.9, 0.7, 0.0])
        k = cov.RBFard(log_ell_list=list(hyp[:5]), log_sigma=0.0)
        kr = (O.RBFARD, hyp, 0)
    elif name == "matern3_d3":
        x, y = _data(n, 3)
        hyp = np.array([0.5, 0.0])
        k = cov.Matern(log_ell=hyp[0], d=3, log_sigma=hyp[1])
        kr = (O.MATERN, hyp, 3)
    elif name == "rbf_plus_periodic_times_rbf":
        x, y = _data(n, 1)
        hyp = np.array([0.1, -0.2, 0.2, 0.4, -0.2, 0.6, 0.0])
        k = cov.RBF(hyp[0], hyp[1]) + cov.Periodic(hyp[2], hyp[3], hyp[4]) * cov.RBF(hyp[5], hyp[6])
        kr = (("sum", _leaf(O.RBF), ("prod", _leaf(O.PERIODIC), _leaf(O.RBF))), hyp, 0)
    elif name == "linear_plus_rbf":
        x, y = _data(n, 2)
        hyp = np.array([-0.5, 0.3, -0.1])
        tree = ("sum", D.L("linear"), D.L("rbf"))
        k = D.build(tree, hyp, cov, 2)
        K, barK = D.tree_matrix(tree, hyp, x=x)
        return k, x, y, _b_of(K, barK), None, lambda h: D.tree_matrix(tree, hyp, x=x, der=h)
    elif name in ("sm_q2", "pre_scaled_plus_rbf", "three_ard"):
        if name == "sm_q2":
            x, y = _data(n, 1)
            k = cov.SM(2, [np.log(0.6), np.log(0.4), np.log(0.2), np.log(0.5), np.log(0.3), np.log(0.4)])
        elif name == "pre_scaled_plus_rbf":
            x, y = _data(n, 2)
            A = np.random.RandomState(n).randn(n, 6) / np.sqrt(6.0)
            k = 0.5 * cov.Pre(np.zeros((n + 1, 1)), A @ A.T) + cov.RBF(0.3, -0.2)
        else:
            x, y = _data(n, 3)
            k = (cov.RBFard(log_ell_list=[0.5, 0.7, 0.6], log_sigma=-0.5)
                 + cov.RBFard(log_ell_list=[1.0, 0.9, 1.1], log_sigma=-0.7) * cov.RBFard(log_ell_list=[0.2, 0.4, 0.3], log_sigma=0.0))
        K = np.ascontiguousarray(np.asarray(k.getCovMatrix(x=x, mode="train"), dtype=float))
        barK = 0.0 if name == "three_ard" else KR.C * KR.EPS * np.abs(K)        # (the dense route is handed this very K)

        def dkf(h):
            dK = np.asarray(k.getDerMatrix(x=x, mode="train", der=h), dtype=float)
            return dK, (0.0 if name == "three_ard" else KR.C * KR.EPS * np.abs(dK))
        return k, x, y, _b_of(F._ld(K), barK, K64=K), None, dkf
    K, barK = KR.ref_matrix(kr[0], kr[1], kr[2], x=x, mode="train")
    return k, x, y, _b_of(K, barK), kr, lambda h: KR.ref_matrix(kr[0], kr[1], kr[2], x=x, mode="train", der=h)


def _b_of(K, barK, K64=None):
    B = F._ld(K) / LD(SN2)
    B[np.diag_indices_from(B)] += 1
    return B, np.asarray(barK, dtype=np.float64) / SN2 + F.dense_bar(F._f64(K) if K64 is None else K64, SN2)


KERNEL_NAMES = ["rbf_d1", "rbfard_d5", "matern3_d3", "rbf_plus_periodic_times_rbf", "linear_plus_rbf", "sm_q2", "pre_scaled_plus_rbf",
                "three_ard"]


def _evaluate(k, meanf, x, y, nargout=3, cls=None):
    from pygps_amd import inf, lik
    i = (cls or inf.LOO)()
    res = i.evaluate(meanf, k, lik.Gauss(LOG_SN), x, y.reshape(-1, 1), nargout)
    return i, res


@pytest.mark.parametrize("n", [129, 385])
@pytest.mark.parametrize("name", KERNEL_NAMES)
def test_kernels(lib, name, n):
    from pygps_amd import mean, inf
    k, x, y, (B, barB), kr, dkf = _kernel_case(name, n)
    c = 0.7
    ref = R.cached(B, y - c, SN2, y, barB)
    case = "B %s n=%d" % (name, n)
    forms = [(1, dict(gram=True, centred=True)), (2, {})] if name == "rbfard_d5" else [(0, {})]
    for form, kw in forms:
        with _options(lib, ard_grad_form=form):
            i, (post, nlZ, dnlZ) = _evaluate(k, mean.Const(c), x, y)
            S, Spad = _read_s(lib, n)
        assert (name == "three_ard") == bool(getattr(post.L, "dense", False))         # the route the case is about
        mu, s2, lp = i.last_loo
        rr = ref.ratios(dict(alpha=post.alpha, mu=mu, s2=s2, lp=lp, nlZ=float(nlZ), S=S, Spad=Spad, dlik=float(dnlZ.lik[0])))
        tu = ref.tol("u")
        rr["dmean"] = abs(float(LD(float(dnlZ.mean[0])) + np.sum(ref.val["u"]))) / float(np.sum(tu))
        if kr is not None:
            vals, tol = R.dnlz_reference(ref.grad_shim(), kr[0], kr[1], kr[2], x, **kw)
            e = np.abs(np.array(dnlZ.cov + dnlZ.lik, dtype=np.float64).astype(LD) - vals).astype(np.float64) / tol
            rr["dcov"], rr["dlik_sum"] = float(np.max(e[:-1])), float(e[-1])
        else:
            rr["dcov"] = _sum_ratios(dnlZ.cov, grad_sums(ref, [dkf(h) for h in range(len(dnlZ.cov))]))
        _record(case + ("" if not form else " ard_grad_form=%d" % form), rr)


# ---- C: means ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname", ["zero", "const", "linear"])
def test_means(lib, mname):
    from pygps_amd import mean, cov
    n = 129
    k, x, y, (B, barB), kr, dkf = _kernel_case("matern3_d3", n)
    meanf = dict(zero=mean.Zero(), const=mean.Const(0.7), linear=mean.Linear(alpha_list=[0.3, -0.2, 0.1]))[mname]
    m = np.asarray(meanf.getMean(x), dtype=float).ravel()
    ref = R.cached(B, y - m, SN2, y, barB)
    i, (post, nlZ, dnlZ) = _evaluate(k, meanf, x, y)
    mu, s2, lp = i.last_loo
    rr = ref.ratios(dict(alpha=post.alpha, mu=mu, s2=s2, lp=lp, nlZ=float(nlZ)))                # mu includes m: the reference's y is y
    nm = len(meanf.hyp) if meanf.hyp else 0
    assert len(dnlZ.mean) == nm
    tu, au = ref.tol("u"), np.abs(F._f64(ref.val["u"]))
    for h in range(nm):
        dm = np.asarray(meanf.getDerMatrix(x, h), dtype=float).ravel()
        want = -np.sum(ref.val["u"] * F._ld(dm))
        tol = float(np.sum(tu * np.abs(dm))) + n * R.EPS * float(np.sum(au * np.abs(dm)))
        rr["dmean%d" % h] = abs(float(LD(float(dnlZ.mean[h])) - want)) / tol
    _record("C mean %s" % mname, rr)


# ---- D: the value-only path -------------------------------------------------------------------------------------------------------
def _program_loo(lib, x, y, c, want, hyp=(0.1, 0.0)):
    from pygps_amd import _lib, inf
    ctx = _lib.ctx()
    n, d = x.shape
    x, yv = _lib.f64(x), _lib.f64(y).ravel()
    _lib.check(lib.pgp_set_data(ctx, _lib.ptr(x), n, d, _lib.ptr(yv)))
    inf._Resident.key.pop((_lib.default_device(), _lib.current_slot()), None)
    hyp = _lib.f64(np.array(hyp))
    m, dm = np.full(n, float(c)), np.ones((1, n))
    alpha, mu, s2, lp = (np.full(n, np.nan) for _ in range(4))
    nlz, dn = np.zeros(2), np.zeros(1 + len(hyp) + 1)
    fh = C.c_void_p()
    _lib.check(lib.pgp_loo_fit(ctx, _lib.COV_RBF, _lib.ptr(hyp), len(hyp), 0, 0, LOG_SN, _lib.ptr(m), _lib.ptr(dm), 1, want,
                               _lib.ptr(alpha), _lib.ptr(mu), _lib.ptr(s2), _lib.ptr(lp), _lib.ptr(nlz), _lib.ptr(dn), C.byref(fh)),
               "pgp_loo_fit")
    lib.pgp_factor_free(ctx, fh)
    return dict(alpha=alpha, mu=mu, s2=s2, lp=lp, nlZ=float(nlz[0]), marginal=float(nlz[1]), dn=dn)


CLASS = "gemm_f64(lauum W^T W)"          # the product S = G G' is profiled in lauum's class, beside B^-1 = E E' (or W'W)


def _launches(lib, fn):
    from pygps_amd import _lib
    _lib.check(lib.pgp_profile_reset(_lib.ctx()))
    out = fn()
    return out, _lib.profile()[CLASS]["launches"]


def _exact_pair(lib, x, y, K, r):
    """An exact fit with gradients on either route (what B^-1 alone costs in launches of the class)."""
    from pygps_amd import _lib, inf
    ctx = _lib.ctx()
    n, d = x.shape
    x, yv = _lib.f64(x), _lib.f64(y).ravel()
    _lib.check(lib.pgp_set_data(ctx, _lib.ptr(x), n, d, _lib.ptr(yv)))
    inf._Resident.key.pop((_lib.default_device(), _lib.current_slot()), None)
    hyp = _lib.f64(np.array([0.1, 0.0]))
    m, dm = np.full(n, 0.7), np.ones((1, n))
    alpha, nlz, dn, gl = np.zeros(n), np.zeros(1), np.zeros(4), np.zeros(1)
    _lib.check(lib.pgp_exact_fit(ctx, _lib.COV_RBF, _lib.ptr(hyp), 2, 0, 0, LOG_SN, _lib.ptr(m), _lib.ptr(dm), 1, 3, _lib.ptr(alpha),
                                 _lib.ptr(nlz), _lib.ptr(dn), None), "pgp_exact_fit")
    _lib.check(lib.pgp_exact_fit_dense(ctx, _lib.ptr(K), n, _lib.ptr(r), LOG_SN, 3, _lib.ptr(alpha), _lib.ptr(nlz), _lib.ptr(gl), None),
               "pgp_exact_fit_dense")


@pytest.mark.parametrize("fused", [1, 0])
def test_value_only_path(lib, fused):
    """want = 2 against want = 3, bit for bit, on both routes.  With profiling on, the class the product is profiled in records
    for the two want = 2 calls (program route, dense route) nothing at all with the fused inverse -- neither the product nor
    E E' -- and with fused_inverse 0 only the program route's documented fall-back to want = 3's route to B^-1, one W'W launch
    (the dense route always runs the fused inverse); the two want = 3 calls record what two exact fits with gradients record,
    plus one product each."""
    from pygps_amd import _lib
    n = 257
    x, y = _data(n, 2)
    K, r, ref = _dense_case(n)
    K, r = np.ascontiguousarray(K), np.ascontiguousarray(r)
    ctx = _lib.ctx()
    with _options(lib, fused_inverse=fused):
        _lib.check(lib.pgp_set_profiling(ctx, 1))
        try:
            _, base = _launches(lib, lambda: _exact_pair(lib, x, y, K, r))
            (v2, d2), l2 = _launches(lib, lambda: (_program_loo(lib, x, y, 0.7, 2), _dense_loo(lib, K, r, LOG_SN, 2)))
            (v3, d3), l3 = _launches(lib, lambda: (_program_loo(lib, x, y, 0.7, 3), _dense_loo(lib, K, r, LOG_SN, 3, read_s=False)))
        finally:
            lib.pgp_set_profiling(ctx, 0)
    print("loo D launches of %s: two exact fits %d, two want = 2 calls %d, two want = 3 calls %d" % (CLASS, base, l2, l3))
    assert base >= 2 and l2 == (0 if fused else 1) and l3 == base + 2
    for a, b in ((v2, v3), (d2, d3)):
        for f in ("alpha", "mu", "s2", "lp", "nlZ", "marginal"):
            assert np.array_equal(np.asarray(a[f]), np.asarray(b[f])), (fused, f)
    _record("D value-only dense n=%d fused_inverse=%d" % (n, fused), ref.ratios({f: d2[f] for f in ("alpha", "mu", "s2", "lp", "nlZ")}))


# ---- A': the same sizes on the program route (pgp_loo_fit: exact_fit_run's LOO tail and the 64-row Hadamard tiles on S) ---------
_PROG = {}
PROG_HYP = np.array([np.log(np.sqrt(3.0)), 0.0])


def _prog_case(n):
    if n not in _PROG:
        x, y = _data(n, 3, seed=11)
        B, barB = R.program_b(O.RBF, PROG_HYP, 0, x, SN2)
        _PROG[n] = (x, y, R.cached(B, y - 0.7, SN2, y, barB))
    return _PROG[n]


@pytest.mark.parametrize("n,small", SIZES)
def test_sizes_across_the_edges_program_route(lib, n, small):
    """RBF d = 3, mean.Const, through pgp_loo_fit with gradients: every value, S entry by entry (padding rows exact zeros), and the
    gradient sums of hadamard_reduce_launch on S and the zero vector -- cov and lik through fit_ref_ld.dnlz_reference given S,
    the mean's -u' 1 through the tolerance of u."""
    x, y, ref = _prog_case(n)
    case = "A' program n=%d%s" % (n, "" if small is None else " small_tile_below=%d" % small)
    with _options(lib, **({} if small is None else dict(small_tile_below=small))):
        got = _program_loo(lib, x, y, 0.7, 3, hyp=PROG_HYP)
        S, Spad = _read_s(lib, n)
    dn = got["dn"]
    rr = ref.ratios(dict(alpha=got["alpha"], mu=got["mu"], s2=got["s2"], lp=got["lp"], nlZ=got["nlZ"], S=S, Spad=Spad, dlik=float(dn[-1])))
    rr["dmean"] = abs(float(LD(float(dn[0])) + np.sum(ref.val["u"]))) / float(np.sum(ref.tol("u")))
    vals, tol = R.dnlz_reference(ref.grad_shim(), O.RBF, PROG_HYP, 0, x)
    assert np.all(np.isfinite(dn))
    e = np.abs(dn[1:].astype(LD) - vals).astype(np.float64) / tol
    rr["dcov"], rr["dlik_sum"] = float(np.max(e[:-1])), float(e[-1])
    _record(case, rr)


# ---- E: padding, posterior, hand-over ---------------------------------------------------------------------------------------------
def test_padding_contributes_nothing(lib):
    """n = 129, np = 256: the program route's noise gradient and S against the dense route's at the same K -- the two differ only
    in how B is formed (both within the reference's tolerance), and the padding rows of S are exact zeros on both."""
    from pygps_amd import cov, mean
    n = 129
    k, x, y, (B, barB), kr, dkf = _kernel_case("rbf_d1", n)
    ref = R.cached(B, y - 0.7, SN2, y, barB)
    i, (post, nlZ, dnlZ) = _evaluate(k, mean.Const(0.7), x, y)
    S, Spad = _read_s(lib, n)
    assert np.all(Spad == 0)
    K = np.ascontiguousarray(np.asarray(k.getCovMatrix(x=x, mode="train"), dtype=float))
    d = _dense_loo(lib, K, y - 0.7, LOG_SN, 3)
    assert np.all(d["Spad"] == 0)
    rr = ref.ratios(dict(dlik=float(dnlZ.lik[0]), S=S))
    rd = ref.ratios(dict(dlik=d["dlik"], S=d["S"]))
    _record("E padding n=129", dict(dlik_program=rr["dlik"], dlik_dense=rd["dlik"], S_program=rr["S"], S_dense=rd["S"]))
    assert d["dlik"] == float(np.trace(d["S"])) or abs(d["dlik"] - np.trace(d["S"])) <= 4 * n * R.EPS * np.trace(np.abs(d["S"]))


def test_posterior_is_the_exact_fits(lib):
    from pygps_amd import inf, mean, cov
    import pygps_amd as pyGPs
    n = 300
    x, y = _data(n, 2)
    xs = np.random.RandomState(5).randn(40, 2)
    res = {}
    for name in ("Exact", "LOO"):
        m = pyGPs.GPR()
        m.setPrior(mean=mean.Const(0.7), kernel=cov.RBF(0.1, 0.0))
        m.setNoise(LOG_SN)
        m.setData(x, y.reshape(-1, 1))
        if name == "LOO":
            m.useInference("LOO")
        nlZ, dnlZ, post = m.getPosterior()
        L = np.zeros((n, n))
        from pygps_amd import _lib
        _lib.check(lib.pgp_factor_to_host(post.L.ctx, post.L.handle, _lib.ptr(L)))
        res[name] = (post.alpha.copy(), L, m.predict(xs)[:4], nlZ, m)
    assert np.array_equal(res["Exact"][0], res["LOO"][0]) and np.array_equal(res["Exact"][1], res["LOO"][1])
    for a, b in zip(res["Exact"][2], res["LOO"][2]):
        assert np.array_equal(a, b)
    assert res["LOO"][4].inffunc.last_nlZ_marginal == res["Exact"][3]


def test_value_only_posterior_without_the_fused_inverse(lib):
    """fused_inverse 0, want = 2: LOO's alpha (want = 3's route) against Exact's (back-substitution), both within the reference's
    tolerance of alpha; LOO's equals Exact's want = 3 alpha bit for bit."""
    from pygps_amd import inf, mean
    n = 257
    x, y, ref = _prog_case(n)
    from pygps_amd import cov
    k = cov.RBF(PROG_HYP[0], PROG_HYP[1])
    with _options(lib, fused_inverse=0):
        _, (pl, _) = _evaluate(k, mean.Const(0.7), x, y, nargout=2, cls=inf.LOO)
        _, (pe2, _) = _evaluate(k, mean.Const(0.7), x, y, nargout=2, cls=inf.Exact)
        _, (pe3, _, _) = _evaluate(k, mean.Const(0.7), x, y, nargout=3, cls=inf.Exact)
    assert np.array_equal(pl.alpha, pe3.alpha)
    _record("E want=2 fused_inverse=0 alpha", dict(alpha_loo=ref.ratios(dict(alpha=pl.alpha))["alpha"],
                                                  alpha_exact=ref.ratios(dict(alpha=pe2.alpha))["alpha"]))


@pytest.mark.parametrize("fused", [1, 0])
def test_a_fit_between_two_others(lib, fused):
    """Exact, LOO, Exact on one context, program route and dense route: the two Exact results are the same bits (the LOO fit
    leaves S in c->Binv and, on the dense route, a zeroed alpha in the workspace).  With fused_inverse 0 the LOO tail takes
    c->W for G and overwrites all of it, the tiles above the diagonal included: the Exact fit behind it (triangular inverse into
    c->W, W'W) must not see that."""
    from pygps_amd import inf, mean, cov
    n = 257
    for name in ("rbf_d1", "three_ard"):
        k, x, y, _, _, _ = _kernel_case(name, n)
        out = []
        for cls in (inf.Exact, inf.LOO, inf.Exact):
            with _options(lib, fused_inverse=fused):
                i, (post, nlZ, dnlZ) = _evaluate(k, mean.Const(0.7), x, y, cls=cls)
            out.append((post.alpha.copy(), float(nlZ), [float(v) for v in dnlZ.mean + dnlZ.cov + dnlZ.lik]))
        assert np.array_equal(out[0][0], out[2][0]) and out[0][1] == out[2][1] and out[0][2] == out[2][2], name
        assert np.array_equal(out[0][0], out[1][0]), name
        assert out[1][1] != out[0][1]


# ---- F: API -------------------------------------------------------------------------------------------------------------------------
def _model(n=200, d=2):
    import pygps_amd as pyGPs
    x, y = _data(n, d, seed=3)
    m = pyGPs.GPR()
    m.setPrior(kernel=pyGPs.cov.RBF(0.5, 0.3))
    m.setNoise(np.log(0.3))
    m.setData(x, y.reshape(-1, 1))
    return m, x, y


def test_optimize_lowers_the_loo_objective(lib):
    m, x, y = _model()
    m.useInference("LOO")
    before = float(m.getPosterior()[0])
    m.optimize(numIterations=5)
    after = float(m.getPosterior()[0])
    print("loo optimize: nlZ_loo %.6f -> %.6f" % (before, after))
    assert after < before and float(m.nlZ) == after


def test_predict_loo_and_validation(lib):
    from pygps_amd import valid
    for use in (None, "LOO"):
        m, x, y = _model()
        if use:
            m.useInference(use)
        n = x.shape[0]
        ymu, ys2, fmu, fs2, lp = m.predict_loo()
        sn2 = float(np.exp(2 * m.likfunc.hyp[0]))
        for a in (ymu, ys2, fmu, fs2, lp):
            assert a.shape == (n, 1) and np.all(np.isfinite(a))
        assert np.array_equal(fmu, ymu) and np.array_equal(fs2, ys2 - sn2) and np.all(fs2 > 0)
        rec = valid.loo_validation(m)
        assert set(rec) == {"RMSE", "NLPD"} and all(np.isfinite(v) for v in rec.values())
        assert rec["NLPD"] == pytest.approx(-float(np.mean(lp)), rel=1e-12)


def test_refusals(lib):
    import pygps_amd as pyGPs
    from pygps_amd import inf, lik, mean, cov
    x, y = _data(50, 1)
    with pytest.raises(Exception, match="LOO inference only possible with Gaussian likelihood"):
        inf.LOO().evaluate(mean.Zero(), cov.RBF(), lik.Erf(), x, np.sign(y).reshape(-1, 1), 2)
    with pytest.raises(NotImplementedError):
        inf.LOO(sharded=True).evaluate(mean.Zero(), cov.RBF(), lik.Gauss(LOG_SN), x, y.reshape(-1, 1), 2)
    with pytest.raises(Exception):
        pyGPs.GPR_FITC().useInference("LOO")
    for cls in (pyGPs.GPC, pyGPs.GPMC):
        with pytest.raises(Exception):
            (cls(3) if cls is pyGPs.GPMC else cls()).useInference("LOO")
    m = pyGPs.GPR()
    m.useLikelihood("Laplace")
    m.setData(x, y.reshape(-1, 1))
    with pytest.raises(Exception, match="predict_loo needs Exact or LOO inference"):
        m.predict_loo()
