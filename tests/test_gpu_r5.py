"""GPU: round 5.

* K-fold validation on the device against the reference's own loop (G19: Validation/valid.py:20-66 driven as
  Demo/JHUI/demo_Validation.py:70-90 does, G6 N = 2048 data, K = 10; GPC + EP, K = 5) -- in process and sharded over ranks with NO
  torch in the processes (world 1: the library's RCCL transport; world 2: its host transport served by pygps_amd.hostgroup, two
  ranks sharing the GPU).
* cfg 4 (Core/opt.py:301-327 sharded) without torch at world 1 (RCCL) and world 2 against G9; at the stated size N = 8192 against
  the bounded fixture recorded from the reference (8 restarts x 3 line searches).
* the multi-dataset objective of Demo/Clustering/pyGP_extension.py:27-76.
* plain RBF with d = 300 (the Gram-form prep buffer's mean region), the ARD gradient forms just under the bound.
"""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden, relerr, synth_cls, synth_reg
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def _flat(d):
    return np.array(list(d.mean) + list(d.cov) + list(d.lik), dtype=float)


def _make_reg(d):
    import pygps_amd as pyGPs

    def make():
        m = pyGPs.GPR()
        m.setPrior(kernel=pyGPs.cov.RBF(np.log(np.sqrt(d)), 0.0))
        m.setNoise(np.log(0.1))
        return m
    return make


def test_G19_k_fold_regression_in_process(lib):
    from pygps_amd import valid
    g = golden("G19_kfold")
    N, d, K = int(g["N"]), int(g["d"]), int(g["K"])
    x, y = synth_reg(N, d)
    res = valid.sharded_k_fold(_make_reg(d), x, y, K=K, metrics=("RMSE", "NLPD"))
    assert relerr(res["nlZ"], g["nlZ"]) < 1e-9
    assert np.max(np.abs(res["RMSE"] - g["rmse"]) / g["rmse"]) < 1e-8
    assert np.max(np.abs(res["NLPD"] - g["nlpd"]) / np.abs(g["nlpd"])) < 1e-7
    # one fold by hand through the reference-style generator: first prediction of fold 0
    import pygps_amd as pyGPs
    xtr, xte, ytr, yte = next(valid.k_fold_validation(x, y, K))
    m = _make_reg(d)()
    m.setData(xtr, ytr)
    m.getPosterior()
    ym, ys2, fm, fs2, lp = m.predict(xte, ys=yte)
    assert abs(ym[0, 0] - g["ym0"][0]) < 1e-8 * abs(g["ym0"][0]) and abs(ys2[0, 0] - g["ys20"][0]) < 1e-7 * g["ys20"][0]
    # with the demo's optimize() per fold (5 line searches): the optimiser path amplifies rounding, loose tolerances
    # (the fixture's flow per fold: setData -> optimize, i.e. the default mean is Const(mean(y_train)): set_data=True, the default)
    res = valid.sharded_k_fold(_make_reg(d), x, y, K=K, metrics=("RMSE", "NLPD"), numIterations=int(g["optimize_iters"]))
    assert np.max(np.abs(res["nlZ"] - g["opt_nlZ"]) / np.abs(g["opt_nlZ"])) < 1e-5
    assert np.max(np.abs(res["RMSE"] - g["opt_rmse"]) / g["opt_rmse"]) < 1e-4
    assert np.max(np.abs(res["NLPD"] - g["opt_nlpd"]) / np.abs(g["opt_nlpd"])) < 1e-3


def test_G19_k_fold_classification_ep(lib):
    import pygps_amd as pyGPs
    from pygps_amd import valid
    g = golden("G19_kfold")
    N, d, K = int(g["cls_N"]), int(g["cls_d"]), int(g["cls_K"])
    x, y = synth_cls(N, d)

    def make():
        m = pyGPs.GPC()
        m.setPrior(kernel=pyGPs.cov.RBF(np.log(np.sqrt(d)), 0.0))
        return m
    res = valid.sharded_k_fold(make, x, y, K=K, metrics=("ACC", "Prec", "Recall", "RMSE_class"))
    assert relerr(res["nlZ"], g["cls_nlZ"]) < 1e-8
    assert np.array_equal(res["ACC"], g["cls_acc"]) and np.array_equal(res["Prec"], g["cls_prec"])
    assert np.array_equal(res["Recall"], g["cls_rec"]) and np.allclose(res["RMSE_class"], g["cls_rmse"], rtol=1e-14)


@pytest.mark.parametrize("world", [1, 2])
def test_G19_k_fold_sharded_without_torch(tmp_path, world):
    from test_hostgroup import launch
    g = golden("G19_kfold")
    rs = launch(world, "kfold_gpu", tmp_path, timeout=900)
    for z in rs:
        assert relerr(z["nlZ"], g["nlZ"]) < 1e-9 and np.max(np.abs(z["RMSE"] - g["rmse"]) / g["rmse"]) < 1e-8
        assert np.max(np.abs(z["NLPD"] - g["nlpd"]) / np.abs(g["nlpd"])) < 1e-7
        assert np.array_equal(z["nlZ"], rs[0]["nlZ"]) and np.array_equal(z["owner"], rs[0]["owner"])
    assert set(rs[0]["owner"].tolist()) == set(range(world))                      # every rank ran folds


@pytest.mark.parametrize("world,streams,stub", [(1, 2, False), (2, 1, False), (2, 1, True), (4, 2, True)])
def test_cfg4_restart_search_without_torch(tmp_path, world, streams, stub):
    """BASELINE configs[3] with nothing but libpygps_amd.so + sockets for the 128-byte id: world 1 over the library's RCCL
    transport (system librccl), world 2 over its host transport -- and (round 6) world 2 / 4 over the library's RCCL BRANCH
    (ncclBroadcast of the start table and the data, ncclAllGather of the records, staged through device buffers) bound to the
    shared-memory stand-in of tests/stub_rccl; per-restart objectives against the reference's run (G9, N = 512)."""
    from test_hostgroup import launch
    from conftest import build_stub_rccl
    g = golden("G9_restarts_N512")
    env = dict(PYGPS_AMD_TRANSPORT="rccl", PYGPS_AMD_RCCL_PATH=build_stub_rccl()) if stub else None
    rs = launch(world, "g9_search", tmp_path, 512, streams, timeout=900, extra_env=env)
    want_transport = "rccl" if world == 1 or stub else "host"
    for z in rs:
        assert str(z["transport"]) == want_transport
        assert relerr(z["X0"], g["run_X0"]) < 1e-14
        assert np.array_equal(z["f"], rs[0]["f"]) and np.array_equal(z["hyp"], rs[0]["hyp"])
    f = rs[0]["f"]
    ok = np.isfinite(g["run_f"])
    assert np.array_equal(np.isfinite(f), ok)
    assert np.max(np.abs(f[ok] - g["run_f"][ok]) / np.abs(g["run_f"][ok])) < 1e-5, (f, g["run_f"])
    assert abs(float(rs[0]["nlZ"]) - float(g["best_nlZ"])) < 1e-6 * abs(float(g["best_nlZ"]))


def test_cfg4_at_its_stated_size_N8192_bounded_fixture(lib):
    """BASELINE configs[3] says N = 8192; G9_restarts_N8192_3ls is the reference's own run at that size with the search bounded to
    3 line searches per restart (8 restarts, np.random.seed(123): 3.4 h of reference fits; the complete run).  Start table bit for bit,
    which restarts fail, per-restart objective <= 1e-5, line-search counts, the optimum the reference settled on."""
    path = os.path.join(GOLDEN, "G9_restarts_N8192_3ls.npz")
    assert os.path.exists(path), "tests/golden/G9_restarts_N8192_3ls.npz is missing: record it (make_golden.py g9_8192_3ls), cfg 4 is not pinned at its size without it"
    import pygps_amd as pyGPs
    g = golden("G9_restarts_N8192_3ls")
    N, d = int(g["N"]), int(g["d"])
    x, y = synth_reg(N, d)
    m = pyGPs.GPR()
    m.setPrior(kernel=pyGPs.cov.RBF(np.log(np.sqrt(d)), 0.0))
    m.setNoise(np.log(0.1))
    m.setData(x, y)
    m.setOptimizer("ShardedMinimize", num_restarts=int(g["num_restarts"]))
    np.random.seed(int(g["np_seed"]))
    m.optimize(x, y, numIterations=int(g["numIterations"]))
    o = m.optimizer
    k = int(g["n_runs"])                               # 8: the complete run (a fixture of a stopped run would hold its first n_runs restarts: make_golden.g9_from_partial)
    assert k >= 3 and relerr(o.init_table[:k], g["run_X0"]) < 1e-14
    f = np.array([r.f for r in o.runs])[:k]
    okr = np.array([r.ok for r in o.runs])[:k]
    assert np.array_equal(okr, g["run_ok"])
    ok = g["run_ok"]
    assert np.max(np.abs(f[ok] - g["run_f"][ok]) / np.abs(g["run_f"][ok])) < 1e-5, (f, g["run_f"])
    assert np.array_equal(np.array([r.nls for r in o.runs])[:k][ok], g["run_nls"][ok])
    if "best_nlZ" in g.files:                          # the complete run: the optimum the reference settled on
        assert abs(m.nlZ - float(g["best_nlZ"])) < 1e-6 * abs(float(g["best_nlZ"]))
        assert relerr(o._convert_to_array(), g["best_hyp"]) < 1e-4


def test_multi_dataset_objective_sums_like_the_clustering_demo(lib):
    """Demo/Clustering/pyGP_extension.py:27-76: one model, several independent data sets, nlZ and dnlZ accumulated."""
    import pygps_amd as pyGPs
    from pygps_amd import opt
    rng = np.random.RandomState(5)
    xs = [rng.randn(n, 3) for n in (150, 200, 97)]
    ys = [np.sin(x.sum(axis=1, keepdims=True)) + 0.1 * rng.randn(x.shape[0], 1) for x in xs]
    hyp = np.array([0.3, -0.2])
    m = pyGPs.GPR()
    m.setPrior(kernel=pyGPs.cov.RBF(0.0, 0.0))
    m.setNoise(np.log(0.2))
    tot, dn, each = opt.multi_dataset_objective(hyp, m, xs, ys, der=True)
    want, wg = 0.0, np.zeros(4)
    for i, (x, y) in enumerate(zip(xs, ys)):
        ref = O.exact_fit(O.RBF, hyp, 0, np.log(0.2), x, y, float(np.mean(y)) * np.ones_like(y), np.ones_like(y), faithful=False)
        want += ref["nlZ"]
        wg += np.concatenate([ref["dnlZ_mean"], ref["dnlZ_cov"], ref["dnlZ_lik"]])
        assert abs(each[i] - ref["nlZ"]) < 1e-9 * abs(ref["nlZ"])
    assert abs(tot - want) < 1e-9 * abs(want) and np.max(np.abs(_flat(dn) - wg)) < 1e-7 * np.max(np.abs(wg))
    assert type(dn.cov[0]) is np.float64
    tot2, dn2, _ = opt.multi_dataset_objective(hyp, m, xs, ys, der=False)
    assert dn2 is None and abs(tot2 - want) < 1e-9 * abs(want)


def test_rbf_with_300_dimensions_gram_vs_difference_form(lib):
    """plain RBF has no cap on d; the Gram-form assembly's prep buffer holds 272 coordinate means in front of the
    norms.  d = 300 pixel-like data in [0, 1] with ell ~ sqrt(d) passes the host's norm bound: the fit must not depend on the
    gram_assembly option (beyond 272 coordinates the Gram form is not offered) and must match the oracle."""
    import pygps_amd as pyGPs
    from test_gpu_parity_r4 import _fit_with
    rng = np.random.RandomState(11)
    n, d = 900, 300
    x = rng.rand(n, d)
    y = np.sin(x[:, :5].sum(axis=1, keepdims=True)) + 0.05 * rng.randn(n, 1)
    kern = lambda: pyGPs.cov.RBF(np.log(np.sqrt(d)) - 0.5, 0.1)
    r0, r1, r2 = (_fit_with(lib, o, x, y, kern, np.log(0.1)) for o in (0, 1, 2))
    c = float(np.mean(y))
    ref = O.exact_fit(O.RBF, np.array([np.log(np.sqrt(d)) - 0.5, 0.1]), 0, np.log(0.1), x, y, c * np.ones_like(y), np.ones_like(y),
                      faithful=False)
    gref = np.concatenate([ref["dnlZ_mean"], ref["dnlZ_cov"], ref["dnlZ_lik"]])
    for r in (r0, r1, r2):
        assert relerr(r[0], ref["nlZ"]) < 1e-9 and relerr(r[2], ref["alpha"]) < 1e-7
        assert np.max(np.abs(r[1] - gref)) < 1e-7 * np.max(np.abs(gref))
    # d = 256 (16 chunks of 16: the largest dpad the Gram form takes) still runs it, forced vs forbidden agree
    x2 = x[:, :256].copy()
    k2 = lambda: pyGPs.cov.RBF(np.log(16.0) - 0.5, 0.1)
    a0, a2 = (_fit_with(lib, o, x2, y, k2, np.log(0.1)) for o in (0, 2))
    assert a0[0] != a2[0] or not np.array_equal(a0[2], a2[2])                     # two different code paths ...
    assert relerr(a2[0], a0[0]) < 1e-12 and relerr(a2[2], a0[2]) < 1e-10 and relerr(a2[1], a0[1]) < 1e-9


def test_ard_gradient_forms_just_under_the_bound(lib):
    """the matrix-core form of the ARD gradient weights is used up to |x|^2 = 1e6 of the scaled, centred points (was
    1e8).  Data just under the bound (a spread of ~800 length scales along one coordinate): default = matrix-core form, and it
    agrees with the difference form and the oracle's per-length-scale getDerMatrix loop within the gradient tolerance."""
    from test_gpu_parity_r4 import _ard_fit_with
    rng = np.random.RandomState(2)
    n, d = 600, 6
    x = rng.randn(n, d)
    x[:, 0] *= 220.0                                   # |x0|^2 up to ~ (4.1 * 220)^2 ~ 8e5 < 1e6 at ell = 1
    assert np.sum(np.max(np.abs(x - x.mean(axis=0)), axis=0) ** 2) < 0.95e6
    x[1::2] = x[::2] + 0.3 * rng.randn(n // 2, d) * np.array([0.5, 1, 1, 1, 1, 1])    # near pairs: non-trivial K entries
    y = np.sin(x[:, 1:].sum(axis=1, keepdims=True)) + 0.1 * rng.randn(n, 1)
    log_ell = np.zeros(d)
    r0, r1, r2 = (_ard_fit_with(lib, f, x, y, log_ell) for f in (0, 1, 2))
    assert np.array_equal(r0[1], r1[1])                                            # the default is the matrix-core form here
    c = float(np.mean(y))
    ref = O.exact_fit(O.RBFARD, np.concatenate([log_ell, [0.1]]), 0, np.log(0.12), x, y, c * np.ones_like(y), np.ones_like(y),
                      faithful=False)
    gref = np.concatenate([ref["dnlZ_mean"], ref["dnlZ_cov"], ref["dnlZ_lik"]])
    for r in (r1, r2):
        assert np.max(np.abs(r[1] - gref)) < 1e-7 * np.max(np.abs(gref))


def test_two_ep_fits_at_once_on_two_fit_streams(lib):
    """Two EP fits on two fit streams of one GPU (what a restart / fold search over a GPC model does): a block sweep is a resident
    kernel that meets bulk launches through device counters, and two of them at once could starve each other on shared hardware
    queues until their bounded waits gave up (seen once in the K-fold test).  Sweeps are now serialised per device; 2 x 8 fits must
    all succeed and reproduce the single-stream numbers bit for bit."""
    import threading
    import pygps_amd as pyGPs
    from pygps_amd import _lib
    x, y = synth_cls(1024, 8)

    def fit():
        m = pyGPs.GPC()
        m.setPrior(kernel=pyGPs.cov.RBF(np.log(np.sqrt(8.0)), 0.0))
        nlZ, dnlZ, post = m.getPosterior(x, y)
        return nlZ, np.array(post.alpha)
    ref = fit()
    out, errs = {}, []

    def work(k):
        try:
            with _lib.fit_stream(k):
                out[k] = [fit() for _ in range(8)]
        except Exception as e:           # pragma: no cover
            errs.append(e)
    ths = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errs, errs
    for k in range(2):
        for nlZ, a in out[k]:
            assert nlZ == ref[0] and np.array_equal(a, ref[1])


def test_getCovMatrix_train_at_cfg3_size_in_the_gram_form(lib):
    """getCovMatrix('train') of RBFard at d = 64, n >= 4096 runs the Gram form on the matrix cores when the host's norm bound
    allows it (round 5; Core/cov.py:887-904 is the difference form).  Kernel-matrix parity stays <= 1e-13: against the same call
    with the Gram form forbidden, against the oracle's cdist form on a sample of rows; ragged n (general kernel) and n % 64 == 0
    (restructured kernel); data beyond the bound keeps the difference form bit for bit."""
    import pygps_amd as pyGPs
    from pygps_amd import _lib
    ctx = _lib.ctx()
    d = 64
    for n in (4096, 4133):
        x, _ = synth_reg(n, d)
        k = pyGPs.cov.RBFard(log_ell_list=[float(np.log(np.sqrt(d)) + 0.01 * (i % 5)) for i in range(d)], log_sigma=0.2)
        try:
            _lib.check(lib.pgp_set_option(ctx, b"gram_assembly", 0))
            K0 = k.getCovMatrix(x=x, mode="train")
            _lib.check(lib.pgp_set_option(ctx, b"gram_assembly", 1))
            K1 = k.getCovMatrix(x=x, mode="train")
            _lib.check(lib.pgp_set_option(ctx, b"gram_assembly", 2))
            K2 = k.getCovMatrix(x=x, mode="train")
        finally:
            lib.pgp_set_option(ctx, b"gram_assembly", 1)
        assert np.array_equal(K1, K2) and not np.array_equal(K1, K0)              # the bound let the Gram form through
        assert np.max(np.abs(K1 - K0) / K0) < 1e-13 and np.array_equal(K1, K1.T) and np.all(np.diag(K1) == np.exp(0.4))
        rows = np.arange(0, n, 397)
        ref = O.cov_matrix(O.RBFARD, np.array(k.hyp), 0, x=x[rows], z=x, mode="cross")
        assert np.max(np.abs(K1[rows] - ref) / ref) < 1e-13
        xb = x.copy()
        xb[::2, 0] += 5.0e3                                                        # a second cluster far beyond the bound
        K3 = k.getCovMatrix(x=xb, mode="train")
        try:
            _lib.check(lib.pgp_set_option(ctx, b"gram_assembly", 0))
            K4 = k.getCovMatrix(x=xb, mode="train")
        finally:
            lib.pgp_set_option(ctx, b"gram_assembly", 1)
        assert np.array_equal(K3, K4)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [4096, 4608, 5120, 8064, 9088])
def test_s_pan_schedule_is_bit_identical_to_the_main_stream_solve(lib, N):
    """End of round 5: under sched=2 the panel solve S(p) runs on the panel stream behind D(p)'s leaf chain, TU_d waits for the paired
    launch by its own event and D's stage-out runs on the main stream from a double-buffered scratch (csrc/sweep.hip run_sched02,
    options s_pan / s_pan_direct / s_pan_out).  Same kernels, same per-tile order: every output of Exact.evaluate
    (Core/inf.py:353-384) -- nlZ, alpha, dnlZ, the factor -- must equal the s_pan=0 schedule's BIT FOR BIT, at even and odd panel
    counts (N = 4608: 9 panels, 5120: 10) and with a partial last panel (N = 8064 = 15.75 panels, 9088 = 17.75)."""
    import ctypes as C
    from pygps_amd import _lib
    d = 16
    x, y = synth_reg(N, d, seed=N)
    x = _lib.f64(x); y = _lib.f64(y).ravel()
    hyp = _lib.f64(np.array([np.log(np.sqrt(d)), 0.2])); m = np.full(N, float(y.mean())); dm = np.ones((1, N))
    ctx = _lib.ctx()
    _lib.check(lib.pgp_set_data(ctx, _lib.ptr(x), N, d, _lib.ptr(y)))
    res = {}
    sets = {"off": dict(sched=2, s_pan=0), "on": dict(sched=2, s_pan=1), "marked": dict(sched=2, s_pan=2),
            "no_direct": dict(sched=2, s_pan=1, s_pan_direct=0), "no_out": dict(sched=2, s_pan=1, s_pan_out=0)}
    try:
        for name, opts in sets.items():
            for k, v in dict(s_pan=-1, s_pan_direct=1, s_pan_out=1).items():
                _lib.check(lib.pgp_set_option(ctx, k.encode(), v))
            for k, v in opts.items():
                _lib.check(lib.pgp_set_option(ctx, k.encode(), v))
            for rep in range(2):
                alpha = np.zeros(N); nlZ = np.zeros(1); g = np.zeros(4); fh = C.c_void_p()
                _lib.check(lib.pgp_exact_fit(ctx, 0, _lib.ptr(hyp), 2, 0, 0, float(np.log(0.1)), _lib.ptr(m), _lib.ptr(dm), 1, 3,
                                             _lib.ptr(alpha), _lib.ptr(nlZ), _lib.ptr(g), C.byref(fh)))
                L = np.zeros((N, N))
                _lib.check(lib.pgp_factor_to_host(ctx, fh, _lib.ptr(L)))
                lib.pgp_factor_free(ctx, fh)
                res[name, rep] = (nlZ.copy(), alpha.copy(), g.copy(), np.tril(L))
    finally:
        for k, v in dict(sched=-1, s_pan=-1, s_pan_direct=1, s_pan_out=1).items():
            lib.pgp_set_option(ctx, k.encode(), v)
    ref = res["off", 0]
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    for key, got in res.items():
        for a, b in zip(ref, got):
            assert np.array_equal(a, b), key
