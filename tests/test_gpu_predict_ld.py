"""GPU: GP.predict (csrc/predict.hip; Core/gp.py:395-417) and tools.solve_chol (pgp_potrs; Core/tools.py:81-97) against the
long-double reference of tests/predict_ref_ld.py, per test point, at the shapes and options where predict.hip takes another path.

The reference predicts from the posterior the device itself reports (post.alpha, post.sW, post.L): the fits are pinned by other
modules, a failure here points at the prediction.  Every assertion is `worst <= 1`, worst = max_j |device - reference| / tol_j with
tol_j = T_j + 8 E_cpu + floor_j from predict_ref_ld (kernel bar propagated to first order, 8 x the measured error of two fp64 CPU
evaluations, 4 ulps of the result's scale); no tolerance is taken from the device's output.  tests/test_predict_ref_host.py shows
on the CPU that this tolerance rejects every single-slip mutant of the arithmetic by >= 10 x.

Test points of every case (predict_ref_ld.make_points / select): the first third are training points + 1e-3 randn (fs2 ~ 1e-4),
one is an exact copy of a training point, the last three sit at |x| = 50 where the cross-covariances have underflowed against the
prior (fmu == ms and fs2 == kss exactly), the rest are randn.  The prior mean is mean.Const(0.5); the cases that run more than one
device batch (and the n = 1300 model they share) add mean.Linear so that ms differs per test point, the EP case uses the linear
mean that makes its island's sites end with ttau = 0.

  A  shapes: GPR, RBF d = 3, (n, ns) across the 128-leaf edges and the product form's gate np >= 1024, predict_inverse 0 / 2,
     keep_inverse 1 / 0; the slab widths of the product form at n = 1025 (ns = 1024, 1025, 1100, 1536) and its default gate
  B  options on the n = 1300 model (11 leaves, two outer panels): solve_outer, small_tile_below, trtri_small_tile_below,
     fused_inverse, predict_batch
  C  per-point sW: GPC + EP (Matern 3, n = 1025, sites with sW = 0), GPC + Laplace (RBFard d = 17), GPR + lik.Laplace + EP
  D  an RBF + Matern 5 program; Linear + RBF (per-point kss, batch offset of the coordinates); a tree that is not a device
     program (pgp_predict_dense)
  E  tools.solve_chol at n in {1, 129, 1025, 1300} x nrhs in {1, 5, 129}
  F  a posterior handle whose inverse rows went back to the pool predicts the same bits after another fit reused the memory

Measured on the MI355X: worst ratio per case (1 = the tolerance).

    case                                                             blocked solve      product form
                                                                     fmu      fs2       fmu      fs2
    A  n = 1     ns = 1     (keep_inverse 1 and 0)                   0        0.0072    (np < 1024: the blocked solve, bit for bit)
    A  n = 127   ns = 129                                            0.0054   0.0040    (same)
    A  n = 128   ns = 128                                            0.0056   0.0047    (same)
    A  n = 129   ns = 1                                              0.0011   0.0001    (same)
    A  n = 1023  ns = 130                                            0.0019   0.0009    0.0025   0.0026
    A  n = 1024  ns = 127                                            0.0026   0.0009    0.0026   0.0023
    A  n = 1025  ns = 300                                            0.0028   0.0012    0.0045   0.0044
    A  n = 1300  ns = 257                                            0.0027   0.0007    0.0035   0.0022
    A  n = 1025  ns = 1024 / 1025 / 1100 / 1536 (default = product)  0.0030   0.0014    0.0044   0.0040
    A  n = 1025  ns = 1023 (default = blocked)                       0.0030   0.0014
    B  solve_outer 1 / 3 / 8                                         0.0027   0.0007
    B  small_tile_below 1 / 1000000                                  0.0027   0.0007    0.0035   0.0022
    B  keep_inverse 0, trtri_small_tile_below 1 / 2049                                  0.0035   0.0022
    B  fused_inverse 0                                               0.0025   0.0007    0.0038   0.0022
    B  predict_batch 128, ns = 300 (bit-equal to one batch)          0.0027   0.0007    0.0035   0.0022
    C  GPC + EP, Matern 3, n = 1025 (island sites with sW = 0)       0.037    0.0095    0.037    0.0091
    C  GPC + Laplace, RBFard d = 17, n = 257                         0.0014   0.0033
    C  GPR + lik.Laplace + EP, n = 300                               0.0036   0.0020
    D  RBF + Matern 5, n = 1153                                      0.0020   0.0009    0.0031   0.0043
    D  Linear + RBF, n = 1153, predict_batch 128 (= one batch)       0.0078   0.0024
    D  three RBFard (dense route), n = 257, predict_batch 128        0.0033   0.0025
    E  solve_chol  n = 1: 0.10   n = 129: 0.23   n = 1025: 0.61   n = 1300: 0.52   (worst over nrhs = 1, 5, 129)
    F  bit-equal: yes (modes 2 and 0, and through predict_with_posterior on a deepcopy); 0.0041 / 0.0024 of the tolerance

The prediction sits at 1e-3 ... 4e-2 of its tolerance -- the kernel bar (16 ulps per covariance entry, summed to first order)
dominates it, as on the CPU, where the two fp64 forms sit at 2e-3 ... 5e-2 -- so the factor 8 on the solve term stays as it is.
solve_chol has no kernel term: the device uses up to 0.61 of 8 x the CPU's error, i.e. its error is up to ~5 x that of LAPACK's two
substitutions (explicit 128 x 128 leaf inverses, twice).  No case exceeded 1; predict.hip is unchanged.
"""
import contextlib
import copy
import gc

import numpy as np
import pytest

import predict_ref_ld as P
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

# the defaults of csrc/ctx.h, restored after every case
DEFAULTS = dict(predict_inverse=1, keep_inverse=1, solve_outer=8, small_tile_below=200, trtri_small_tile_below=2049,
                fused_inverse=1, predict_batch=65536)
LOG_ELL3 = float(np.log(np.sqrt(3.0)))
ARD3 = ("sum", ("sum", ("leaf", O.RBFARD, 0), ("leaf", O.RBFARD, 0)), ("leaf", O.RBFARD, 0))
ARD3_HYP = [0.5, 0.6, 0.4, -0.5, 0.7, 0.5, 0.6, -0.5, 0.4, 0.7, 0.5, -0.5]
SUM = ("sum", ("leaf", O.RBF, 0), ("leaf", O.MATERN, 5))
LIN_RBF = ("sum", ("leaf", "linear", 0), ("leaf", "rbf", 0))
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


def _record(case, worst, where, detail=""):
    WORST[case] = max(WORST.get(case, 0.0), worst)
    print("predict_ld %-50s worst %.3g at %s%s" % (case, worst, where, detail))


# ---- models ----------------------------------------------------------------------------------------------------------------
def _mean(kind):
    import pygps_amd as pyGPs
    if kind == "const":
        return pyGPs.mean.Const(P.MEAN_C)
    w = P.MEAN_W if kind == "linear" else P.MEAN_W_ISLAND
    return pyGPs.mean.Const(P.MEAN_C) + pyGPs.mean.Linear(alpha_list=list(w))


def _model(name, n):
    """(model with its data set, not yet fitted; reference spec): the cases' models by name."""
    import pygps_amd as pyGPs
    cov = pyGPs.cov
    if name == "rbf":                                     # A, B, F: GPR, RBF d = 3; the n = 1300 model carries the linear mean
        x, y = P.reg_data(n, 3, 11 + n)
        m = pyGPs.GPR()
        m.setPrior(mean=_mean("linear" if n == 1300 else "const"), kernel=cov.RBF(LOG_ELL3, 0.0))
        spec = ("oracle", O.RBF, 0)
    elif name == "rbf_other":                             # F: the model that reuses the memory
        x, y = P.reg_data(n, 3, 977)
        m = pyGPs.GPR()
        m.setPrior(mean=_mean("const"), kernel=cov.RBF(LOG_ELL3 + 0.3, 0.2))
        spec = ("oracle", O.RBF, 0)
    elif name == "sum":
        x, y = P.reg_data(n, 3, 12)
        m = pyGPs.GPR()
        m.setPrior(mean=_mean("const"), kernel=cov.RBF(P.SUM_HYP[0], P.SUM_HYP[1]) + cov.Matern(P.SUM_HYP[2], 5, P.SUM_HYP[3]))
        spec = ("oracle", SUM, 0)
    elif name == "lin_plus_rbf":
        x, y = P.reg_data(n, 3, 13)
        m = pyGPs.GPR()
        m.setPrior(mean=_mean("linear"), kernel=cov.Linear(-1.0) + cov.RBF(LOG_ELL3, 0.0))
        spec = ("dot", LIN_RBF)
    elif name == "dense_ard3":
        x, y = P.reg_data(n, 3, 14)
        m = pyGPs.GPR()
        h = ARD3_HYP
        m.setPrior(mean=_mean("linear"), kernel=(cov.RBFard(log_ell_list=h[0:3], log_sigma=h[3])
                                                 + cov.RBFard(log_ell_list=h[4:7], log_sigma=h[7]))
                   + cov.RBFard(log_ell_list=h[8:11], log_sigma=h[11]))
        spec = ("oracle", ARD3, 0)
    elif name == "ep_matern3":
        x, y = P.cls_data(n, 2, 3, island=6.0)
        m = pyGPs.GPC()
        m.setPrior(mean=_mean("island"), kernel=cov.Matern(0.0, 3, 0.0))
        spec = ("oracle", O.MATERN, 3)
    elif name == "laplace_rbfard":
        x, y = P.cls_data(n, 17, 4)
        m = pyGPs.GPC()
        m.useInference("Laplace")
        m.setPrior(mean=_mean("const"), kernel=cov.RBFard(log_ell_list=[float(np.log(np.sqrt(17.0)))] * 17, log_sigma=0.5))
        spec = ("oracle", O.RBFARD, 0)
    else:
        assert name == "liklaplace_ep"
        x, y = P.reg_data(n, 3, 15)
        m = pyGPs.GPR()
        m.useLikelihood("Laplace")
        m.setPrior(mean=_mean("const"), kernel=cov.RBF(LOG_ELL3, 0.0))
        m.likfunc.hyp = [float(np.log(0.1))]
        spec = ("oracle", O.RBF, 0)
    if isinstance(m, pyGPs.GPR) and name != "liklaplace_ep":
        m.setNoise(float(np.log(P.SN)))
    m.setData(x, y)
    return m, spec


_POOLS = {}


def _pool(m, name, nmax):
    """The model's pool of test points and its prior mean there (one pool per model name, size and data)."""
    key = (name, m.x.shape[0], nmax)
    if key not in _POOLS:
        xs = P.make_points(m.x, nmax, seed=100 + m.x.shape[0])
        _POOLS[key] = (xs, np.asarray(m.meanfunc.getMean(xs), dtype=float).ravel())
    return _POOLS[key]


def _ref(m, spec, name, nmax):
    """The long-double reference of the model's CURRENT posterior at its whole pool (cached by the posterior's bits)."""
    xs, ms = _pool(m, name, nmax)
    post = m.posterior
    return P.cached(spec, np.array(m.covfunc.hyp, dtype=float), m.x, xs, ms, post.alpha, post.sW, np.asarray(post.L))


def _predict(m, xs, post=None):
    out = m.predict(xs) if post is None else m.predict_with_posterior(post, xs)
    return np.array(out[2]).ravel(), np.array(out[3]).ravel()


def _check(case, got, ref, dot=False):
    """The device's (fmu, fs2) against the Ref of the same test points: inside the bar, exact where the reference says so."""
    fmu, fs2 = got
    worst, where = P.check(fmu, fs2, ref)
    _record(case, worst, where, "   fmu %.3g  fs2 %.3g" % tuple(P.ratios(fmu, fs2, ref)[k][0] for k in ("fmu", "fs2")))
    assert worst <= 1.0, (case, worst, where)
    ex = ref.exact()
    if not dot and ref.ns >= 5:
        assert np.all(ex[-3:]), case                     # the three points at |x| = 50
    assert np.array_equal(fmu[ex], ref.ms[ex]) and np.array_equal(fs2[ex], ref.kss[ex].astype(np.float64)), case
    return worst


# ---- A: shapes ---------------------------------------------------------------------------------------------------------------
NMAX = {1: 1, 127: 129, 128: 128, 129: 1, 1023: 130, 1024: 127, 1025: 1536, 1300: 300}


@pytest.mark.parametrize("n,ns", [(1, 1), (127, 129), (128, 128), (129, 1), (1023, 130), (1024, 127), (1025, 300), (1300, 257)])
def test_shapes_both_forms_with_and_without_the_fits_inverse_rows(lib, n, ns):
    m, spec = _model("rbf", n)
    idx = P.select(NMAX[n], ns)
    for keep in (1, 0):
        with _options(lib, keep_inverse=keep):
            m.getPosterior()
        ref = _ref(m, spec, "rbf", NMAX[n]).take(idx)
        xs = _pool(m, "rbf", NMAX[n])[0][idx]
        out = {}
        for mode in (0, 2):
            with _options(lib, predict_inverse=mode):
                out[mode] = _predict(m, xs)
            _check("A n=%d ns=%d keep=%d mode=%d" % (n, ns, keep, mode), out[mode], ref)
        if (n + 127) // 128 * 128 < 1024:                 # below the gate mode 2 IS the blocked solve
            assert np.array_equal(out[0][0], out[2][0]) and np.array_equal(out[0][1], out[2][1])


@pytest.mark.parametrize("ns", [1024, 1025, 1100, 1536])
def test_product_form_slab_widths_and_the_default_gate(lib, ns):
    """n = 1025 (np = 1152).  nrhs = 1024: one slab of 1024; 1152: slabs of 128, the last one holding one point (ns = 1025) or 76
    (ns = 1100); 1536: slabs of 512.  A handle without inverse rows and without W takes the product form by default from 1024
    points: bit-equal to predict_inverse 2; the blocked solve is held to the same bar."""
    n = 1025
    m, spec = _model("rbf", n)
    idx = P.select(NMAX[n], ns)
    with _options(lib, keep_inverse=0):
        m.getPosterior()
    ref = _ref(m, spec, "rbf", NMAX[n]).take(idx)
    xs = _pool(m, "rbf", NMAX[n])[0][idx]
    default = _predict(m, xs)                             # first: no W on the handle yet, the count alone opens the gate
    _check("A n=1025 ns=%d default" % ns, default, ref)
    out = {}
    for mode in (2, 0):
        with _options(lib, predict_inverse=mode):
            out[mode] = _predict(m, xs)
        _check("A n=1025 ns=%d mode=%d" % (ns, mode), out[mode], ref)
    assert np.array_equal(default[0], out[2][0]) and np.array_equal(default[1], out[2][1])


def test_default_gate_stays_shut_below_1024_points(lib):
    """The same handle state (no inverse rows, no W) at 1023 points: the default is the blocked solve, bit for bit."""
    n, ns = 1025, 1023
    m, spec = _model("rbf", n)
    idx = P.select(NMAX[n], ns)
    with _options(lib, keep_inverse=0):
        m.getPosterior()
    xs = _pool(m, "rbf", NMAX[n])[0][idx]
    default = _predict(m, xs)
    with _options(lib, predict_inverse=0):
        blocked = _predict(m, xs)
    _check("A n=1025 ns=1023 default", default, _ref(m, spec, "rbf", NMAX[n]).take(idx))
    assert np.array_equal(default[0], blocked[0]) and np.array_equal(default[1], blocked[1])


# ---- B: options on the n = 1300 model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit_opts,opts,modes", [
    ({}, dict(solve_outer=1), (0,)), ({}, dict(solve_outer=3), (0,)), ({}, dict(solve_outer=8), (0,)),
    ({}, dict(small_tile_below=1), (0, 2)), ({}, dict(small_tile_below=1000000), (0, 2)),
    (dict(keep_inverse=0), dict(trtri_small_tile_below=1), (2,)), (dict(keep_inverse=0), dict(trtri_small_tile_below=2049), (2,)),
    (dict(fused_inverse=0), {}, (2, 0)),
], ids=["solve_outer1", "solve_outer3", "solve_outer8", "tile128", "tile64", "trtri_tile128", "trtri_default", "no_fused_inverse"])
def test_options_of_the_solve_and_of_the_inverse(lib, fit_opts, opts, modes):
    n, ns = 1300, 257
    m, spec = _model("rbf", n)
    idx = P.select(NMAX[n], ns)
    with _options(lib, **fit_opts):
        m.getPosterior()
    ref = _ref(m, spec, "rbf", NMAX[n]).take(idx)
    xs = _pool(m, "rbf", NMAX[n])[0][idx]
    tag = " ".join("%s=%s" % kv for kv in sorted(list(fit_opts.items()) + list(opts.items())))
    for mode in modes:
        with _options(lib, predict_inverse=mode, **opts):
            got = _predict(m, xs)
        _check("B %s mode=%d" % (tag, mode), got, ref)


def test_three_batches_equal_one_batch_in_both_forms(lib):
    """predict_batch = 128 at ns = 300 (128 + 128 + 44): the offsets of ms, of the coordinates and of the outputs move with the batch."""
    n, ns = 1300, 300
    m, spec = _model("rbf", n)
    m.getPosterior()
    ref = _ref(m, spec, "rbf", NMAX[n])
    xs = _pool(m, "rbf", NMAX[n])[0]
    for mode in (0, 2):
        with _options(lib, predict_inverse=mode):
            one = _predict(m, xs)
        with _options(lib, predict_inverse=mode, predict_batch=P.BATCH):
            three = _predict(m, xs)
        _check("B predict_batch=128 ns=300 mode=%d" % mode, three, ref)
        _check("B one batch ns=300 mode=%d" % mode, one, ref)
        assert np.array_equal(one[0], three[0]) and np.array_equal(one[1], three[1]), mode


# ---- C: per-point sW ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,ns", [("ep_matern3", 1025, 130), ("laplace_rbfard", 257, 130), ("liklaplace_ep", 300, 130)])
def test_per_point_sW(lib, name, n, ns):
    m, spec = _model(name, n)
    m.getPosterior()
    sW = np.asarray(m.posterior.sW).ravel()
    assert np.ptp(sW) > 0
    if name == "ep_matern3":                              # the island's sites: ttau clipped to 0, rows of sW o Ks that are zero
        assert np.any(sW == 0) and np.any(sW > 0)
    ref = _ref(m, spec, name, ns)
    xs = _pool(m, name, ns)[0]
    for mode in (0, 2) if n >= 1024 else (0,):
        with _options(lib, predict_inverse=mode):
            got = _predict(m, xs)
        _check("C %s n=%d mode=%d" % (name, n, mode), got, ref)


# ---- D: kernels and paths ---------------------------------------------------------------------------------------------------
def test_sum_program_both_forms(lib):
    n, ns = 1153, 257
    m, spec = _model("sum", n)
    m.getPosterior()
    assert not getattr(m.posterior.L, "dense", False)
    ref = _ref(m, spec, "sum", ns)
    xs = _pool(m, "sum", ns)[0]
    for mode in (0, 2):
        with _options(lib, predict_inverse=mode):
            got = _predict(m, xs)
        _check("D rbf+matern5 n=1153 mode=%d" % mode, got, ref)


@pytest.mark.parametrize("name,n", [("lin_plus_rbf", 1153), ("dense_ard3", 257)])
def test_batched_paths_of_dot_leaves_and_of_the_dense_route(lib, name, n):
    """Linear + RBF: the blocked solve with k(z, z) per test point from the batch's coordinates.  Three ARD leaves: not a device
    program, the cross block comes from the host (pgp_predict_dense: its own transpose, batch loop and clamp).  ns = 300 in batches
    of 128, and in one batch: the same bits."""
    ns = 300
    m, spec = _model(name, n)
    m.getPosterior()
    assert bool(getattr(m.posterior.L, "dense", False)) == (name == "dense_ard3")
    ref = _ref(m, spec, name, ns)
    xs = _pool(m, name, ns)[0]
    one = _predict(m, xs)
    with _options(lib, predict_batch=P.BATCH):
        three = _predict(m, xs)
    _check("D %s n=%d predict_batch=128" % (name, n), three, ref, dot=name == "lin_plus_rbf")
    _check("D %s n=%d one batch" % (name, n), one, ref, dot=name == "lin_plus_rbf")
    assert np.array_equal(one[0], three[0]) and np.array_equal(one[1], three[1])


# ---- E: tools.solve_chol ------------------------------------------------------------------------------------------------------
_SOLVE = {}


def _solve_case(n):
    """R = chol(K + sn^2 I) (upper, fp64, from the oracle), B (n x 129) and the long-double solution, once per n."""
    if n not in _SOLVE:
        x, _ = P.reg_data(n, 3, 21 + n)
        A = O.cov_matrix(O.RBF, np.array([LOG_ELL3, 0.0]), 0, x=x, mode="train") + P.SN ** 2 * np.eye(n)
        R = np.ascontiguousarray(O.jitchol(A).T)
        B = np.random.RandomState(n).randn(n, 129)
        _SOLVE[n] = (R, B, P.solve_chol_ld(R, B))
    return _SOLVE[n]


@pytest.mark.parametrize("n", [1, 129, 1025, 1300])
@pytest.mark.parametrize("nrhs", [1, 5, 129])
def test_solve_chol_against_long_double(lib, n, nrhs):
    from pygps_amd import tools
    R, B, X = _solve_case(n)
    B, X = np.ascontiguousarray(B[:, :nrhs]), X[:, :nrhs]
    tol, _ = P.solve_tolerance(R, B, X)
    got = tools.solve_chol(R, B)
    worst, j = P.check_solve(got, X, tol)
    _record("E n=%d nrhs=%d" % (n, nrhs), worst, ("column", j))
    assert worst <= 1.0, (n, nrhs, worst, j)


# ---- F: handle lifetime ---------------------------------------------------------------------------------------------------------
def test_handle_predicts_the_same_bits_after_its_inverse_rows_were_reused(lib):
    n, ns = 1025, 130
    a, spec = _model("rbf", n)
    a.getPosterior()                                      # keep_inverse = 1: the handle holds the fit's inverse rows
    xs = _pool(a, "rbf", NMAX[n])[0][P.select(NMAX[n], ns)]
    first = {}
    for mode in (2, 0):                                   # mode 2 first: the rows are transposed into W and go back to the pool
        with _options(lib, predict_inverse=mode):
            first[mode] = _predict(a, xs)
    b, _ = _model("rbf_other", n)
    b.getPosterior()
    with _options(lib, predict_inverse=2):
        _predict(b, xs)
    del b
    gc.collect()
    post = copy.deepcopy(a.posterior)
    for mode in (2, 0):
        with _options(lib, predict_inverse=mode):
            again = _predict(a, xs)
            through = _predict(a, xs, post)
        for got in (again, through):
            assert np.array_equal(got[0], first[mode][0]) and np.array_equal(got[1], first[mode][1]), mode
    ref = _ref(a, spec, "rbf", NMAX[n]).take(P.select(NMAX[n], ns))
    _check("F n=1025 after reuse mode=2", first[2], ref)
    print("predict_ld F bit-equal: yes")
