"""GPU: pygps_amd.GPMC (Core/gp.py:738-932) -- the shared-kernel engine (pgp_gpmc_fit_predict, csrc/gpmc.hip) and the
per-pair route against the reference's recordings (G24, tests/golden/make_golden_gpmc.py; data from tests/gpmc_data.py),
the gather and vote kernels through their test hooks, the fall-backs to the per-pair route and stale state.

Bars: votes relative 1e-7 (the project's bar for EP's ym, test_gpu_composite.py), per-pair nlZ 1e-8 and equal sweep /
Newton-step counts (the G8 / G20 bars), rows summing to 1 within 1e-14; the two routes within 2e-7 of each other (the sum
of their bars).  Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

import gpmc_cpu
import gpmc_data
from conftest import golden, relerr

pytestmark = pytest.mark.gpu

FIT = ["fit_default", "fit_laplace", "fit_ard_const", "fit_program", "fit_c5_uneven", "fit_c10_d64"]


def _model(name, **kw):
    import pygps_amd as pyGPs
    shape = gpmc_data.SHAPES[name]
    x, y, xs = gpmc_data.blobs(**shape)
    m = pyGPs.GPMC(len(shape["counts"]), **kw)
    mean, kernel = gpmc_data.prior(name, pyGPs.cov, pyGPs.mean)
    if mean is not None or kernel is not None:
        m.setPrior(mean=mean, kernel=kernel)
    if name == "fit_laplace":
        m.useInference("Laplace")
    m.setData(x, y)
    return m, xs


def _vote_err(v, ref):
    return float(np.max(np.abs(v - ref) / ref))


def _check_against_reference(tag, m, votes, g):
    P = m.pairs()
    nlz_err = max(abs(m.pair_nlZ[p] - g["pair_nlZ"][k]) / abs(g["pair_nlZ"][k]) for k, p in enumerate(P))
    rows = float(np.max(np.abs(votes.sum(axis=1) - 1)))
    print("%s: route %s, votes rel %.3e, pair nlZ rel %.3e, iterations %s, rows-1 %.1e"
          % (tag, m.last_route, _vote_err(votes, g["votes"]), nlz_err, sorted(set(m.pair_iters.values())), rows))
    assert votes.shape == g["votes"].shape
    assert _vote_err(votes, g["votes"]) < 1e-7
    assert nlz_err < 1e-8
    assert [m.pair_iters[p] for p in P] == [int(v) for v in g["pair_iters"]]
    assert rows <= 1e-14


@pytest.mark.parametrize("name", FIT)
def test_fit_fixture_through_the_default_route(name, lib):
    g = golden("G24_" + name)
    m, xs = _model(name)
    votes = m.fitAndPredict(xs)
    assert m.last_route == "shared"
    _check_against_reference(name + " shared", m, votes, g)


@pytest.mark.parametrize("name", FIT)
def test_fit_fixture_through_the_pairs_route_and_both_routes_agree(name, lib):
    g = golden("G24_" + name)
    m, xs = _model(name, shared_kernel=False)
    votes = m.fitAndPredict(xs)
    assert m.last_route == "pairs"
    _check_against_reference(name + " pairs", m, votes, g)
    ms, _ = _model(name)
    vs = ms.fitAndPredict(xs)
    assert ms.last_route == "shared"
    d = float(np.max(np.abs(vs - votes) / votes))
    dn = max(abs(ms.pair_nlZ[p] - m.pair_nlZ[p]) / abs(m.pair_nlZ[p]) for p in m.pairs())
    print("%s: shared vs pairs: votes rel %.3e, pair nlZ rel %.3e" % (name, d, dn))
    assert d < 2e-7
    assert ms.pair_iters == m.pair_iters


def test_a_tree_that_is_not_a_device_program_falls_back_to_pairs(lib):
    """Three ARD leaves: getCovMatrix only, so every pair takes GPC's dense path; compared with the CPU restatement."""
    import pygps_amd as pyGPs
    from oracle import gp_oracle as O
    cov = pyGPs.cov
    d, counts = 4, [30, 25, 35]
    x, y, xs = gpmc_data.blobs(seed=77, counts=counts, d=d, ns=40, sep=0.8)
    ells = [list(np.log(2.0) + 0.1 * k + np.linspace(-0.2, 0.2, d)) for k in range(3)]
    tree = cov.RBFard(log_ell_list=ells[0], log_sigma=0.0) + cov.RBFard(log_ell_list=ells[1], log_sigma=-0.3) * cov.RBFard(
        log_ell_list=ells[2], log_sigma=0.1)
    assert not tree._on_device()
    m = pyGPs.GPMC(3)
    m.setPrior(kernel=tree)
    m.setData(x, y)
    votes = m.fitAndPredict(xs)
    assert m.last_route == "pairs"
    L = ("leaf", O.RBFARD, 0)
    hyp = np.array(ells[0] + [0.0] + ells[1] + [-0.3] + ells[2] + [0.1])
    assert [float(h) for h in tree.hyp] == [float(h) for h in hyp]
    want, nlZ, iters, _ = gpmc_cpu.fit_and_predict(("sum", L, ("prod", L, L)), hyp, 0, x, y, 3, xs)
    err = _vote_err(votes, want)
    nerr = max(abs(m.pair_nlZ[p] - nlZ[p]) / abs(nlZ[p]) for p in m.pairs())
    print("non-program tree: votes rel %.3e, pair nlZ rel %.3e" % (err, nerr))
    assert err < 1e-7 and nerr < 1e-8 and m.pair_iters == iters


@pytest.mark.parametrize("name", ["opt_default", "opt_prior"])
def test_optimize_and_predict_matches_the_reference(name, lib):
    """Bars: three times the deviation measured on the first MI355X run (OPT_BARS below, as test_gpu_laplace.py sets its
    optimise bar), never looser than what the project accepts for optimised results (test_gpu_fitc_ep.py: hypers 1e-3,
    nlZ 1e-5, predictions 1e-4)."""
    g = golden("G24_" + name)
    m, xs = _model(name)
    votes = m.optimizeAndPredict(xs)
    assert m.last_route == "pairs"
    P = m.pairs()
    herr = max(relerr(m.pair_hyp[p], g["pair_hyp"][k]) for k, p in enumerate(P))
    nerr = max(abs(m.pair_nlZ[p] - g["pair_nlZ"][k]) / abs(g["pair_nlZ"][k]) for k, p in enumerate(P))
    verr = _vote_err(votes, g["votes"])
    print("%s: hypers rel %.3e, pair nlZ rel %.3e, votes rel %.3e" % (name, herr, nerr, verr))
    bars = OPT_BARS[name]
    assert bars[0] <= 1e-3 and bars[1] <= 1e-5 and bars[2] <= 1e-4
    assert herr < bars[0] and nerr < bars[1] and verr < bars[2]
    assert np.max(np.abs(votes.sum(axis=1) - 1)) <= 1e-14
    if name == "opt_prior":                               # chained starts: the user's kernel object ends at the last pair's optimum
        assert relerr(m.covfunc.hyp, g["final_cov_hyp"]) < bars[0]
    else:
        assert list(m.covfunc.hyp) == list(g["final_cov_hyp"])        # untouched defaults


# (hypers, pair nlZ, votes): 3 x the deviation from the reference measured on the first MI355X run (the same figures, digit for
# digit, in a second run), capped at the project's bars.  Measured:
#   opt_default: hypers 1.148e-07, pair nlZ 9.853e-15, votes 1.566e-07
#   opt_prior:   hypers 4.822e-07, pair nlZ 1.565e-14, votes 6.252e-07
OPT_BARS = {"opt_default": (3.5e-7, 3.0e-14, 4.7e-7), "opt_prior": (1.5e-6, 4.7e-14, 1.9e-6)}


def _gather(lib, K, idx, n_pos, m_all):
    from pygps_amd import _lib
    n, k = K.shape[0], len(idx)
    np_ = (k + 127) // 128 * 128
    out, y, mg = np.full((np_, np_), np.nan), np.full(np_, np.nan), np.full(np_, np.nan)
    idx32 = np.ascontiguousarray(idx, dtype=np.int32)
    _lib.check(lib.pgp_test_gather_sym(_lib.ctx(), _lib.ptr(K), n, idx32.ctypes.data_as(C.POINTER(C.c_int32)), k, n_pos, _lib.ptr(m_all),
                                       _lib.ptr(out), _lib.ptr(y), _lib.ptr(mg)), "pgp_test_gather_sym")
    return out, y, mg


@pytest.mark.parametrize("n", [300, 1000])
@pytest.mark.parametrize("runs", [(1, 1), (127, 2), (129, 200)])
def test_gather_sym_bit_for_bit(lib, n, runs):
    rng = np.random.RandomState(n + runs[0])
    K = np.ascontiguousarray(rng.randn(n, n))                      # not symmetric: a transposed gather would show
    m_all = rng.randn(n)
    a, b = runs
    patterns = {
        # scattered rows; the second run starts BELOW the end of the first, so idx[r] < idx[c] for some r > c
        "scattered": np.concatenate([np.sort(rng.choice(np.arange(n // 3, n), a, replace=False)),
                                     np.sort(rng.choice(np.arange(0, n - n // 6), b, replace=False))]),
        # consecutive rows (the 16-byte loads), odd and even starts
        "consecutive": np.concatenate([np.arange(n // 2 + 1, n // 2 + 1 + a) if n // 2 + 1 + a <= n else np.arange(n - a, n),
                                       np.arange(6, 6 + b)]),
    }
    for tag, idx in patterns.items():
        assert len(idx) == a + b and idx.max() < n and idx[a] < idx[a - 1]
        assert np.all(np.diff(idx[:a]) > 0) and np.all(np.diff(idx[a:]) > 0)
        out, y, mg = _gather(lib, K, idx, a, m_all)
        k = a + b
        assert np.array_equal(out[:k, :k], K[np.ix_(idx, idx)]), tag
        assert np.all(out[k:, :] == 0) and np.all(out[:, k:] == 0), tag          # the padding the dense drivers expect: zeros
        assert np.array_equal(y[:k], np.concatenate([np.ones(a), -np.ones(b)])) and np.all(y[k:] == 0), tag
        assert np.array_equal(mg[:k], m_all[idx]) and np.all(mg[k:] == 0), tag


def test_vote_kernel_against_lik_erf(lib):
    import pygps_amd as pyGPs
    from pygps_amd import _lib
    rng = np.random.RandomState(5)
    ns, ncls, ci, cj = 700, 5, 1, 3
    fmu = np.concatenate([np.linspace(-30, 30, 241), 4 * rng.randn(ns - 241)])
    fs2_mixed = np.concatenate([np.zeros(100), np.abs(3 * rng.randn(ns - 100)) ** 2])
    worst = 0.0
    for fs2 in (np.zeros(ns), fs2_mixed):
        votes, norm = np.empty((ns, ncls)), np.empty((ns, ncls))
        _lib.check(lib.pgp_test_vote(_lib.ctx(), _lib.ptr(fmu), _lib.ptr(fs2), ns, ncls, ci, cj, _lib.ptr(votes), _lib.ptr(norm)),
                   "pgp_test_vote")
        ym = pyGPs.lik.Erf().evaluate(None, fmu.reshape(-1, 1), fs2.reshape(-1, 1), None, None, 3)[1]
        want = pyGPs.GPMC.add_votes(np.zeros((ns, ncls)), ym, ci, cj)
        worst = max(worst, float(np.max(np.abs(votes - want))))
        assert np.max(np.abs(votes - want)) < 1e-7
        assert np.all(votes[:, [0, 2, 4]] == 0)
        assert np.max(np.abs(votes[:, ci] + votes[:, cj] - 2)) < 1e-15
        assert np.max(np.abs(norm - want / want.sum(axis=1)[:, None])) < 1e-7
        assert np.max(np.abs(norm.sum(axis=1) - 1)) <= 1e-14
    print("vote kernel vs lik.Erf + host arithmetic: max abs deviation %.3e" % worst)


def test_shared_matrices_over_the_memory_guard_fall_back_to_pairs(lib):
    g = golden("G24_fit_c5_uneven")
    m, xs = _model("fit_c5_uneven")
    need = m.shared_bytes(xs.shape[0])
    m.shared_memory_limit = need - 1                      # the guard's own parameter: nothing is allocated to get here
    votes = m.fitAndPredict(xs)
    assert m.last_route == "pairs"
    _check_against_reference("memory fall-back", m, votes, g)
    m.shared_memory_limit = need
    votes = m.fitAndPredict(xs)
    assert m.last_route == "shared"
    _check_against_reference("at the guard", m, votes, g)


def test_nothing_stale_between_two_calls(lib):
    import pygps_amd as pyGPs
    shape = gpmc_data.SHAPES["fit_default"]
    x, y, xs = gpmc_data.blobs(**shape)

    def fresh(h, xx, yy):
        f = pyGPs.GPMC(4)
        f.setPrior(kernel=pyGPs.cov.RBF(*h))
        f.setData(xx, yy)
        return f
    h1, h2 = [0.0, 0.0], [0.7, 0.4]
    m = fresh(h1, x, y)
    v1 = m.fitAndPredict(xs)
    n1 = dict(m.pair_nlZ)
    m.covfunc.hyp = list(h2)                              # changed hyper-parameters, same object, same data
    v2 = m.fitAndPredict(xs)
    assert m.last_route == "shared"
    f2 = fresh(h2, x, y)
    v2f = f2.fitAndPredict(xs)
    assert np.array_equal(v2, v2f) and m.pair_nlZ == f2.pair_nlZ
    assert np.max(np.abs(v2 - v1)) > 1e-3 and m.pair_nlZ != n1
    x3, y3, _ = gpmc_data.blobs(**dict(shape, seed=991))   # changed data of the same shape (the resident-data key)
    m.setData(x3, y3)
    v3 = m.fitAndPredict(xs)
    assert np.array_equal(v3, fresh(h2, x3, y3).fitAndPredict(xs))
    assert np.max(np.abs(v3 - v2)) > 1e-3
    m.setData(x, y)
    m.covfunc.hyp = list(h1)
    assert np.array_equal(m.fitAndPredict(xs), v1)         # and back: the first result again, bit for bit
