"""GPU: the exact fit -- the Cholesky sweep of csrc/sweep.hip with its fused inverse rows E = L^-T, B^-1 = E E', alpha, nlZ, tr Q and
the gradient sums -- entry by entry against the long-double reference of tests/fit_ref_ld.py, at the sizes and options where
sweep_plan() queues something else.

Every assertion is `worst <= 1`, worst = max_ij |device - reference| / tol_ij with tol_ij = bar_ij + (8 E_cpu + 4 2^-53) scale_ij
from fit_ref_ld (the input bar propagated to first order; 8 x the measured error of three fp64 CPU evaluations -- LAPACK and the
device's blocked form restated in numpy at panel 512 and 128 -- in units of the field's first-order sensitivity; four ulps of that
scale).  Nothing in a tolerance comes from the device.  tests/test_fit_ref_host.py shows on the CPU that this tolerance rejects every
single-slip mutant of the blocked arithmetic, the weakest by 95 x, and that the weakest one passes the suite's max-norm thresholds.

  A  dense route (pgp_exact_fit_dense, log_sn = 0: B = K + I bit for bit, no bar), n in {1, 127, 128, 129, 513, 1025, 1153, 1537}:
     the "rbf" matrix (d = 5 RBF at ell = sqrt(d), K / 0.01, cond ~ 1e4 ... 9e4) and at 513 / 1153 the "line" matrix (sorted 1-d
     inputs, cond ~ 1e6); want = 3: L, alpha, nlZ, tr Q, B^-1 through pgp_test_read_binv, three pgp_dense_grad_term sums (a random
     symmetric dK, one entry in the last ragged row, one entry across the first 128-tile edge); want = 2 / 1: the back-substitution's
     alpha; log_sn = log(0.1) at n = 1153 with the bar 3 2^-53 |K| / sn2
  B  the same B through pgp_potrf (the plain sweep, no inverse rows), n in {129, 1025, 1153, 1537}
  C  options at n = 1153 and 1537, want = 3: small_tile_below 1 / 1000000, eet_first 0 / 1, eet_overlap 0 / 2, pair_launch 0,
     eet_tile 64, lookahead 0, leaf_pivot 0 / 1, s_tile 128, fused_inverse 0, tile_ring 0, and nb_outer 8 at 1537
  D  program route (pgp_exact_fit: RBF d = 3 and RBFard d = 5, sn = 0.1, mean.Const), n in {129, 1025, 1153}: every field carries
     the kernel bar of kernel_ref_ld.ref_matrix; dnlZ against kernel_ref_ld.hadamard_ref on the reference B^-1 and alpha (its own
     bar plus sum_ij tol_Binv,ij |dK_h,ij|); RBFard runs the default form of the gradient pass and both forced ones
     (ard_grad_form 1 / 2, each against hadamard_ref's bar for that form; the default's sums are those of one of them, bit for
     bit, and every other field is); want = 2 with fused_value_max_np -1 and 1024
  E  default plans at N = 2561 (pf = 1, sched 0) and N = 4097 (sched 2, s_pan, tur_tile 1264, a one-leaf last panel, 127 padding
     rows) and sched 0 / 1 at 4097, both routes: fit_ref_ld's large-n functionals at columns / rows 0, 127,
     128, 511, 512, 513, the first row of the last panel, n - 1 and two random, and one +-1 vector through B^-1 B, which crosses
     every tile of B^-1.  The N = 4097 case takes ~14 s once per session: ~5 s the long-double kernel matrix, ~6 s the three fp64
     CPU fits (blocked_fit64 works on a (2 m + 1) x m array), ~3 s all probes of the four fits together -- cutting probes would
     not bring it under 10 s, so they stay
  F  stale buffers: n = 1537, then 700, then 1537 on one context, both routes: the small fit within tolerance, the repeated fit
     bit-equal to the first (and pgp_test_read_binv answers -3 for an n the workspace is not sized for)

Measured on the MI355X, 2026-10-20 (`pytest -s` prints every figure): E_cpu per case in units of 2^-53 x scale, then the device's
worst ratio per field (1 = the tolerance).

    case                         E_cpu / 2^-53:  L     Binv     alpha    nlZ    trQ  |  device:  L      Binv    alpha   nlZ     trQ
    A  dense rbf   n = 1                        0.14   0.16     1.5     0.012  0.045 |         0.028   0.031   0.094   0.0030  0.010
    A  dense rbf   n = 127                      0.68   3.1e5    1.4e3   1.9    17    |         0.035   0.014   0.021   0.013   0.013
    A  dense rbf   n = 128                      0.75   6.2e5    1.5e3   0.58   3.5   |         0.062   0.039   0.019   0.067   0.11
    A  dense rbf   n = 129                      1.1    2.1e6    1.3e3   1.7    2.3   |         0.039   0.0048  0.025   0.097   0.16
    A  dense rbf   n = 513                      1.3    1.2e7    6.3e3   6.3    21    |         0.13    0.15    0.047   0.012   0.0072
    A  dense rbf   n = 1025                     1.8    1.4e8    1.2e4   4.5    17    |         0.062   0.32    0.087   0.28    0.27
    A  dense rbf   n = 1153                     1.8    4.4e8    1.8e4   0.98   17    |         0.062   0.011   0.069   0.16    0.012
    A  dense rbf   n = 1537                     1.8    1.6e8    2.1e4   8.6    33    |         0.076   0.029   0.073   0.033   0.025
    A  dense line  n = 513                      4.0    7.7e7    3.3e5   292    844   |         0.057   0.16    0.15    0.24    0.28
    A  dense line  n = 1153                     4.0    6.4e9    2.4e5   603    1.3e3 |         0.29    0.087   0.22    0.027   0.024
    A  dense rbf   n = 1153, log_sn = log 0.1   1.6    1.2e8    1.8e4   89     464   |         0.069   0.051   0.024   0.00064 0.00016
    D  program rbf     n = 129                  1.1    6.1e5    1.6e3   21     137   |         0.011   0.0039  0.0016  0.00022 6.7e-5
    D  program rbf     n = 1025                 2.9    6.7e7    1.4e4   96     454   |         0.031   0.016   0.0019  0.00021 5.7e-5
    D  program rbf     n = 1153                 2.7    2.3e8    1.8e4   102    445   |         0.026   0.0082  0.0021  8.4e-5  2.2e-5
    D  program rbfard  n = 129                  0.68   7.7e5    992     4.9    67    |         0.0087  0.0011  0.00069 3.8e-5  1.3e-5
    D  program rbfard  n = 1025                 2.1    4.3e7    1.6e4   74     355   |         0.013   0.0059  0.0014  0.00016 3.4e-5
    D  program rbfard  n = 1153                 1.6    1.0e8    1.4e4   59     298   |         0.023   0.0038  0.0014  0.00015 3.1e-5
    F  the n = 700 fit between two n = 1537 fits: dense 0.086 / 0.097 / 0.063 / 0.044 / 0.017, program 0.024 / 0.0027 / 0.0026 /
       0.00016 / 4.1e-5; the repeated n = 1537 fit bit-equal to the first on both routes

    A  want = 2 / 1: L and nlZ bit for bit as want = 3, alpha within 1 % of its want = 3 ratio (the back-substitution)
    A  pgp_dense_grad_term: random dK <= 0.026 (n = 1; <= 7e-6 from n = 127), last ragged row <= 0.024, 128-tile edge <= 0.0023
    B  pgp_potrf: the dense route's L ratio at every size (0.039, 0.062, 0.062, 0.076)
    C  n = 1153: small_tile_below 1: 0.085 / 0.065 / 0.11 / 0.083 / 0.090; leaf_pivot 0: 0.071 / 0.024 / 0.053 / 0.52 / 0.11;
       leaf_pivot 1: 0.067 / 0.014 / 0.080 / 0.037 / 0.035; every other option the default's figures (0.062 / 0.011 / 0.069 / 0.16 / 0.012)
    C  n = 1537: small_tile_below 1: 0.078 / 0.043 / 0.097 / 0.0027 / 0.013; leaf_pivot 0: 0.076 / 0.046 / 0.060 / 0.12 / 0.10;
       leaf_pivot 1: 0.072 / 0.052 / 0.10 / 0.033 / 0.025; nb_outer 8: 0.074 / 0.068 / 0.092 / 0.012 / 0.029; every other option
       the default's figures (0.076 / 0.029 / 0.073 / 0.033 / 0.025)
    D  dnlZ: cov <= 6.1e-6 (RBF), <= 3.7e-6 / 1.2e-5 (RBFard, form 1 / 2), lik <= 0.0028, mean <= 6.7e-7: the sum of the per-entry
       tolerances of B^-1 over |dK| is a worst case that the errors, which cancel, do not approach; the default RBFard form's sums
       are those of one of the two forced forms, bit for bit; want = 2 with fused_value_max_np -1 and 1024: the want = 3 figures of L, alpha, nlZ

    E  large-n functionals    E_cpu / 2^-53: resid_col  left_inv_row  inv_vec  solve_resid  nlZ   |  device (same order): program route / dense route
    E  n = 2561                               30         19            0.28     1.5          0.24  |  0.26  0.076 0.0042 0.0052 7e-8  /  0.37 0.19 0.035 0.15  1e-6
    E  n = 4097 (default = sched 2; sched 1)  49         37            0.19     1.1          0.57  |  0.30  0.077 0.0024 0.0075 1e-7  /  0.30 0.22 0.031 0.088 7e-6
    E  n = 4097 sched 0                                                                            |  0.30  0.075 0.0023 0.0051 2e-8  /  0.30 0.21 0.038 0.086 2e-6

The fit sits at 0.3 of its tolerance at the worst (L on the cond 1e6 matrix, B^-1 at n = 1025; nlZ 0.52 with the lane-per-row
leaf), i.e. at ~2.5 x the error of the worst fp64 CPU form: no case exceeded 1 and csrc/sweep.hip is unchanged.  E_cpu of B^-1 is
large in ulps because (|E| |E'|)_ij is a local scale and the error of an inverse at cond 1e4 ... 1e6 is not: the mutants of
tests/test_fit_ref_host.py that damage B^-1 are still rejected by > 1e7.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import fit_ref_ld as F
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

# the defaults of csrc/ctx.h, restored after every case
DEFAULTS = dict(small_tile_below=200, eet_first=-1, eet_overlap=3, pair_launch=1, eet_tile=128, lookahead=1, leaf_pivot=2, s_tile=0,
                fused_inverse=1, tile_ring=1, nb_outer=0, fused_value_max_np=12288, sched=-1, ard_grad_form=0)
LOG_SN = float(np.log(0.1))
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
    """After the module's last test: the worst ratio per field over the cases that ran (shown with -s)."""
    yield
    for f in sorted(set(f for _, f in WORST)):
        print("fit_ld worst %-18s %.3g  (%s)" % ((f,) + max((r, c) for (c, ff), r in WORST.items() if ff == f)))


def _record(case, rr):
    """rr: {field: ratio}.  Prints, keeps the worst per (case, field), asserts <= 1."""
    for f, v in rr.items():
        WORST[(case, f)] = max(WORST.get((case, f), 0.0), v)
    print("fit_ld %-46s %s" % (case, "  ".join("%s %.3g" % (f, v) for f, v in rr.items())))
    bad = {f: v for f, v in rr.items() if not v <= 1.0}
    assert not bad, (case, bad)


def _ecpu(case, ref):
    print("fit_ld %-46s E_cpu / 2^-53: %s" % (case, "  ".join("%s %.3g" % (f, v / F.EPS) for f, v in ref.e_cpu.items())))


# ---- matrices ------------------------------------------------------------------------------------------------------------------
_MAT = {}


def _matrix(kind, n):
    """(K, r) of the dense route: "rbf" = the d = 5 RBF matrix over sn2 = 0.01 (cond(K + I) ~ 1e4 ... 9e4), "line" = sorted 1-d
    inputs (cond ~ 1e6), "rbf_sn" = the unscaled d = 5 RBF matrix (fitted with log_sn = log 0.1)."""
    if (kind, n) not in _MAT:
        if kind == "line":
            _, y, K = F.sorted_1d_matrix(n)
            r = y
        else:
            _, y, K = F.rbf_matrix(n, 5)
            r = y.ravel() - 0.1                               # (a constant prior mean; n = 1 keeps a nonzero residual)
            if kind == "rbf":
                K = K * 100.0
        _MAT[(kind, n)] = (np.ascontiguousarray(K), np.ascontiguousarray(r))
    return _MAT[(kind, n)]


def _dense_ref(kind, n):
    K, r = _matrix(kind, n)
    if kind == "rbf_sn":
        B = F._ld(K) / F.LD(SN2)
        B[np.diag_indices(n)] += 1
        return F.cached(B, r, SN2, F.dense_bar(K, SN2))
    return F.cached(K + np.eye(n), r, 1.0)


# ---- device calls -----------------------------------------------------------------------------------------------------------------
def _factor(lib, fh, n):
    from pygps_amd import _lib
    R = np.zeros((n, n))
    try:
        _lib.check(lib.pgp_factor_to_host(_lib.ctx(), fh, _lib.ptr(R)))
    finally:
        lib.pgp_factor_free(_lib.ctx(), fh)
    assert np.all(np.tril(R, -1) == 0)
    return np.ascontiguousarray(R.T)


def _binv(lib, n):
    from pygps_amd import _lib
    out = np.full((n, n), np.nan)
    _lib.check(lib.pgp_test_read_binv(_lib.ctx(), n, _lib.ptr(out)), "pgp_test_read_binv")
    return out


def _dense_fit(lib, K, r, log_sn, want):
    from pygps_amd import _lib
    ctx = _lib.ctx()
    n = K.shape[0]
    alpha, nlz, glik = np.zeros(n), np.zeros(1), np.zeros(1)
    fh = C.c_void_p()
    _lib.check(lib.pgp_exact_fit_dense(ctx, _lib.ptr(K), n, _lib.ptr(r), float(log_sn), want, _lib.ptr(alpha), _lib.ptr(nlz),
                                       _lib.ptr(glik), C.byref(fh)), "pgp_exact_fit_dense")
    got = dict(alpha=alpha, L=_factor(lib, fh, n))
    if want >= 2:
        got["nlZ"] = float(nlz[0])
    if want >= 3:
        got["trQ"] = float(glik[0])
        got["Binv"] = _binv(lib, n)
    return got


def _program_fit(lib, kind, hyp, x, y, c, want):
    from pygps_amd import _lib, inf
    ctx = _lib.ctx()
    n, d = x.shape
    x, yv = _lib.f64(x), _lib.f64(y).ravel()
    _lib.check(lib.pgp_set_data(ctx, _lib.ptr(x), n, d, _lib.ptr(yv)))
    inf._Resident.key.pop((_lib.default_device(), _lib.current_slot()), None)     # the package's record of what this context holds
    hyp = _lib.f64(hyp)
    m, dm = np.full(n, float(c)), np.ones((1, n))
    alpha, nlz, dn = np.zeros(n), np.zeros(1), np.zeros(1 + len(hyp) + 1)
    fh = C.c_void_p()
    _lib.check(lib.pgp_exact_fit(ctx, kind, _lib.ptr(hyp), len(hyp), 0, 0, LOG_SN, _lib.ptr(m), _lib.ptr(dm), 1, want,
                                 _lib.ptr(alpha), _lib.ptr(nlz), _lib.ptr(dn), C.byref(fh)), "pgp_exact_fit")
    got = dict(alpha=alpha, L=_factor(lib, fh, n))
    if want >= 2:
        got["nlZ"] = float(nlz[0])
    if want >= 3:
        got["trQ"] = float(dn[-1])
        got["dnlZ"] = dn
        got["Binv"] = _binv(lib, n)
    return got


def _ratios(ref, got):
    assert np.all(np.triu(got["L"], 1) == 0)
    return {f: v[0] for f, v in ref.ratios(got).items()}


# ---- A: dense route -----------------------------------------------------------------------------------------------------------------
def _grad_matrices(n, seed):
    rng = np.random.RandomState(seed)
    G = rng.randn(n, n)
    last = np.zeros((n, n))
    j = n // 2
    last[n - 1, j] = last[j, n - 1] = 1.5
    edge = np.zeros((n, n))
    i, j = (128, 127) if n > 128 else (n - 1, 0)
    edge[i, j] = edge[j, i] = -0.75
    return (("random", G + G.T), ("last_row", last), ("tile_edge", edge))


DENSE = [("rbf", n) for n in (1, 127, 128, 129, 513, 1025, 1153, 1537)] + [("line", 513), ("line", 1153)]


@pytest.mark.parametrize("kind,n", DENSE)
def test_dense_route_every_field(lib, kind, n):
    from pygps_amd import _lib
    K, r = _matrix(kind, n)
    ref = _dense_ref(kind, n)
    case = "A dense %s n=%d" % (kind, n)
    _ecpu(case, ref)
    got = _dense_fit(lib, K, r, 0.0, 3)
    rr = _ratios(ref, got)
    g = np.zeros(1)
    for name, dK in _grad_matrices(n, n):
        dK = np.ascontiguousarray(dK)
        _lib.check(lib.pgp_dense_grad_term(_lib.ctx(), _lib.ptr(dK), n, 0.0, _lib.ptr(g)), "pgp_dense_grad_term")
        val, tol = ref.grad_term(dK)
        rr["grad_" + name] = abs(float(F.LD(float(g[0])) - val)) / tol if np.isfinite(g[0]) else np.inf
    _record(case, rr)
    for want in (2, 1):
        _record(case + " want=%d" % want, _ratios(ref, _dense_fit(lib, K, r, 0.0, want)))


def test_dense_route_with_a_noise_scale(lib):
    n = 1153
    K, r = _matrix("rbf_sn", n)
    ref = _dense_ref("rbf_sn", n)
    case = "A dense rbf n=1153 log_sn=log(0.1)"
    _ecpu(case, ref)
    _record(case, _ratios(ref, _dense_fit(lib, K, r, LOG_SN, 3)))


# ---- B: the plain sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 1025, 1153, 1537])
def test_potrf_of_the_same_matrix(lib, n):
    from pygps_amd import _lib
    K, r = _matrix("rbf", n)
    ref = _dense_ref("rbf", n)
    A = np.ascontiguousarray(K + np.eye(n))
    L = np.full((n, n), np.nan)
    assert lib.pgp_potrf(_lib.ctx(), _lib.ptr(A), n, _lib.ptr(L)) == 0
    _record("B potrf rbf n=%d" % n, _ratios(ref, dict(L=L)))


# ---- C: options ------------------------------------------------------------------------------------------------------------------
OPTIONS = [dict(small_tile_below=1), dict(small_tile_below=1000000), dict(eet_first=0), dict(eet_first=1), dict(eet_overlap=0),
           dict(eet_overlap=2), dict(pair_launch=0), dict(eet_tile=64), dict(lookahead=0), dict(leaf_pivot=0), dict(leaf_pivot=1),
           dict(s_tile=128), dict(fused_inverse=0), dict(tile_ring=0)]


@pytest.mark.parametrize("n,opts", [(n, o) for n in (1153, 1537) for o in OPTIONS] + [(1537, dict(nb_outer=8))],
                         ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else str(v))
def test_dense_route_options(lib, n, opts):
    K, r = _matrix("rbf", n)
    ref = _dense_ref("rbf", n)
    with _options(lib, **opts):
        got = _dense_fit(lib, K, r, 0.0, 3)
    _record("C dense rbf n=%d %s" % (n, " ".join("%s=%s" % kv for kv in opts.items())), _ratios(ref, got))


# ---- D: program route ------------------------------------------------------------------------------------------------------------
PROGRAMS = dict(rbf=(O.RBF, 3, np.array([np.log(np.sqrt(3.0)), 0.1])),
                rbfard=(O.RBFARD, 5, np.array([0.75, 0.85, 0.8, 0.9, 0.7, 0.1])))
_PROG = {}


def _program_case(name, n):
    if (name, n) not in _PROG:
        kind, d, hyp = PROGRAMS[name]
        x, y = F.P.reg_data(n, d, 100 + n)
        c = float(y.mean())
        r = y.ravel() - c                                     # what aug_rhs forms on the device, bit for bit
        B, barB = F.program_b(kind, hyp, 0, x, SN2)
        _PROG[(name, n)] = (kind, hyp, x, y, c, F.cached(B, r, SN2, barB))
    return _PROG[(name, n)]


@pytest.mark.parametrize("n", [129, 1025, 1153])
@pytest.mark.parametrize("name", ["rbf", "rbfard"])
def test_program_route_every_field(lib, name, n):
    kind, hyp, x, y, c, ref = _program_case(name, n)
    case = "D program %s n=%d" % (name, n)
    _ecpu(case, ref)
    got = _program_fit(lib, kind, hyp, x, y, c, 3)                # the default form of the gradient pass (ard_grad_form 0)
    rr = _ratios(ref, got)
    ta = np.broadcast_to(ref.tol("alpha"), (n,))
    a = F._f64(ref.alpha)
    rr["dnlZ_mean"] = abs(float(F.LD(float(got["dnlZ"][0])) + np.sum(ref.alpha))) / (float(np.sum(ta)) + n * F.EPS * float(np.sum(np.abs(a))))

    def dnlz_ratios(dn, **kw):
        vals, tol = F.dnlz_reference(ref, kind, hyp, 0, x, **kw)
        assert np.all(np.isfinite(dn))
        e = np.abs(dn[1:].astype(F.LD) - vals).astype(np.float64) / tol
        return float(np.max(e[:-1])), float(e[-1])
    if name == "rbf":
        rr["dnlZ_cov"], rr["dnlZ_lik"] = dnlz_ratios(got["dnlZ"])
    else:
        # RBFard: the pass sums the length-scale derivatives in the Gram form on centred coordinates (form 1) or in the difference
        # form (2); 0 picks one of them by the norm bound.  Both run, each against hadamard_ref's bar for it (as in
        # tests/test_gpu_kernel_matrices.py), and the default's sums are those of one of the two, bit for bit
        forced = {}
        for form, kw in ((1, dict(gram=True, centred=True)), (2, {})):
            with _options(lib, ard_grad_form=form):
                forced[form] = _program_fit(lib, kind, hyp, x, y, c, 3)
            rr["dnlZ_cov_form%d" % form], rr["dnlZ_lik_form%d" % form] = dnlz_ratios(forced[form]["dnlZ"], **kw)
            for f in ("L", "alpha", "nlZ", "Binv"):
                assert np.array_equal(forced[form][f], got[f]), (form, f)
        assert any(np.array_equal(forced[form]["dnlZ"], got["dnlZ"]) for form in (1, 2))
    _record(case, rr)
    for fv in (-1, 1024):
        with _options(lib, fused_value_max_np=fv):
            _record(case + " want=2 fused_value_max_np=%d" % fv, _ratios(ref, _program_fit(lib, kind, hyp, x, y, c, 2)))


# ---- E: default plans at size -------------------------------------------------------------------------------------------------
_LARGE = {}


def _large_case(n):
    if n not in _LARGE:
        kind, d, hyp = PROGRAMS["rbf"]
        x, y = F.P.reg_data(n, d, 100 + n)
        c = float(y.mean())
        r = y.ravel() - c
        Bp, barBp = F.program_b(kind, hyp, 0, x, SN2)
        B64 = F._f64(Bp)
        K64 = np.ascontiguousarray(F._f64((Bp - F._ld(np.eye(n))) * F.LD(SN2)))        # the dense route's input: K rounded to fp64
        _LARGE[n] = (kind, hyp, x, y, c, r, Bp, barBp, K64, F.large_cached(B64, r, SN2), np.abs(B64))
    return _LARGE[n]


@pytest.mark.parametrize("n,sched", [(2561, -1), (4097, -1), (4097, 0), (4097, 1)])
def test_default_plans_at_size(lib, n, sched):
    kind, hyp, x, y, c, r, Bp, barBp, K64, lref, aB = _large_case(n)
    case = "E n=%d%s" % (n, "" if sched < 0 else " sched=%d" % sched)
    print("fit_ld %-46s E_cpu / 2^-53: %s" % (case, "  ".join("%s %.3g" % (f, v / F.EPS) for f, v in lref.e_cpu.items())))
    with _options(lib, **({} if sched < 0 else dict(sched=sched))):
        got = _program_fit(lib, kind, hyp, x, y, c, 3)
        gotd = _dense_fit(lib, K64, r, LOG_SN, 3)
    assert np.all(np.triu(got["L"], 1) == 0) and np.all(np.triu(gotd["L"], 1) == 0)
    _record(case + " program", F.large_ratios(lref, Bp, got, barBp, aB))
    Bd = F._ld(K64) / F.LD(SN2)
    Bd[np.diag_indices(n)] += 1
    _record(case + " dense", F.large_ratios(lref, Bd, gotd, F.dense_bar(K64, SN2), aB))


# ---- F: stale buffers ------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_stale_buffers_dense_route(lib):
    K, r = _matrix("rbf", 1537)
    Ks, rs = _matrix("rbf", 700)
    first = _dense_fit(lib, K, r, 0.0, 3)
    small = _dense_fit(lib, Ks, rs, 0.0, 3)
    from pygps_amd import _lib
    assert lib.pgp_test_read_binv(_lib.ctx(), 1537, _lib.ptr(np.zeros((1537, 1537)))) == -3      # the workspace is the n = 700 one
    again = _dense_fit(lib, K, r, 0.0, 3)
    _record("F dense 1537 -> 700 -> 1537: the 700", _ratios(_dense_ref("rbf", 700), small))
    _same_bits(first, again)


def test_stale_buffers_program_route(lib):
    kind, d, hyp = PROGRAMS["rbf"]
    x, y = F.P.reg_data(1537, d, 100 + 1537)
    kind, hyp, xs, ys, cs, ref = _program_case("rbf", 700)
    first = _program_fit(lib, kind, hyp, x, y, float(y.mean()), 3)
    small = _program_fit(lib, kind, hyp, xs, ys, cs, 3)
    again = _program_fit(lib, kind, hyp, x, y, float(y.mean()), 3)
    _record("F program 1537 -> 700 -> 1537: the 700", _ratios(ref, small))
    _same_bits(first, again)
