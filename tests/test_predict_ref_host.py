"""CPU: the long-double prediction reference of tests/predict_ref_ld.py and its tolerance are tight (no GPU).

Posteriors come from the CPU oracle with the input recipes of tests/test_gpu_predict_ld.py (EP at n <= 300, where the oracle's
per-site loop is slow).  Three things are shown per case:

  * the reference itself: the long-double forward substitution leaves a residual |L V - B| of a few long-double ulps of |L| |V|;
  * both fp64 CPU evaluations (triangular solve; explicit inverse) pass `check`: the reference alone stays inside the bar;
  * every mutant of the numpy arithmetic -- the slips a prediction kernel can make: a training row or a block of columns left
    out, one wrong entry of L, one sW off by 1e-6, a scalar sW, ms or kss of the wrong test point, V in fp32 -- fails `check` by
    at least MUTANT_FACTOR = 10.  The mutants are arrays on the CPU; no project code is altered for them.
"""
import numpy as np
import pytest

import predict_ref_ld as P
from oracle import gp_oracle as O

LD = P.LD
MUTANT_FACTOR = 10.0
ARD3 = ("sum", ("sum", ("leaf", O.RBFARD, 0), ("leaf", O.RBFARD, 0)), ("leaf", O.RBFARD, 0))
SUM = ("sum", ("leaf", O.RBF, 0), ("leaf", O.MATERN, 5))
LIN_RBF = ("sum", ("leaf", "linear", 0), ("leaf", "rbf", 0))


def _exact(spec, hyp, x, y, m):
    """alpha, sW, upper R of an exact fit from the fp64 training matrix (Core/inf.py:353-384)."""
    n = x.shape[0]
    K = P._cov64(spec, hyp, x, None, "train")
    sn2 = P.SN ** 2
    R = O.jitchol(K / sn2 + np.eye(n)).T
    alpha = O.solve_chol(R, y - m, faithful=False) / sn2
    return alpha, np.ones((n, 1)) / P.SN, R


def _case(name):
    """(spec, hyp, x, xs, ms, alpha, sW, R, flags) of one case; flags: which mutants apply beside the common ones."""
    if name == "gpr_rbf_n1300":                          # the model of the shape / option cases; Const + Linear mean, two batches
        d, n, ns = 3, 1300, 140
        spec, hyp = ("oracle", O.RBF, 0), np.array([np.log(np.sqrt(d)), 0.0])
        x, y = P.reg_data(n, d, 11)
        alpha, sW, R = _exact(spec, hyp, x, y, P.mean_values(x, True))
        flags = {"ms_batch"}
    elif name == "gpr_sum_n1153":
        d, n, ns = 3, 1153, 60
        spec, hyp = ("oracle", SUM, 0), P.SUM_HYP
        x, y = P.reg_data(n, d, 12)
        alpha, sW, R = _exact(spec, hyp, x, y, P.mean_values(x))
        flags = set()
    elif name == "gpr_lin_plus_rbf_n1153":               # dot-product leaf: per-point kss; Const + Linear mean, two batches
        d, n, ns = 3, 1153, 140
        spec, hyp = ("dot", LIN_RBF), np.array([-1.0, np.log(np.sqrt(d)), 0.0])
        x, y = P.reg_data(n, d, 13)
        alpha, sW, R = _exact(spec, hyp, x, y, P.mean_values(x, True))
        flags = {"ms_batch", "kss_const"}
    elif name == "gpr_dense_ard3_n257":                  # three ARD leaves: not a device program
        d, n, ns = 3, 257, 140
        spec = ("oracle", ARD3, 0)
        hyp = np.array([0.5, 0.6, 0.4, -0.5, 0.7, 0.5, 0.6, -0.5, 0.4, 0.7, 0.5, -0.5])
        x, y = P.reg_data(n, d, 14)
        alpha, sW, R = _exact(spec, hyp, x, y, P.mean_values(x, True))
        flags = {"ms_batch"}
    elif name == "gpc_ep_matern3_n300":                  # sites of the island end with ttau = 0
        d, n, ns = 2, 300, 60
        spec, hyp = ("oracle", O.MATERN, 3), np.array([0.0, 0.0])
        x, y = P.cls_data(n, d, 3, island=6.0)
        r = O.ep_fit(O.MATERN, hyp, 3, x, y, P.mean_values(x, P.MEAN_W_ISLAND), nargout=2)
        assert np.any(r["sW"] == 0) and np.any(r["sW"] > 0)
        alpha, sW, R = r["alpha"], r["sW"], r["L"]
        flags = {"sw_scalar"}
    elif name == "gpc_laplace_rbfard_n257":
        d, n, ns = 17, 257, 60
        spec, hyp = ("oracle", O.RBFARD, 0), np.array([np.log(np.sqrt(d))] * d + [0.5])
        x, y = P.cls_data(n, d, 4)
        r = O.laplace_fit(O.RBFARD, hyp, 0, x, y, P.mean_values(x), nargout=2, faithful=False)
        alpha, sW, R = r["alpha"], r["sW"], r["L"]
        flags = {"sw_scalar"}
    else:
        assert name == "gpr_liklaplace_ep_n300"
        from lik_laplace_cpu import ep_laplace_fit
        d, n, ns = 3, 300, 60
        spec, hyp = ("oracle", O.RBF, 0), np.array([np.log(np.sqrt(d)), 0.0])
        x, y = P.reg_data(n, d, 15)
        r = ep_laplace_fit(O.cov_matrix(O.RBF, hyp, 0, x=x, mode="train"), y, P.mean_values(x), np.log(0.1))
        alpha, sW, R = r["alpha"].reshape(n, 1), r["sW"].reshape(n, 1), r["L"]
        flags = {"sw_scalar"}
    xs = P.make_points(x, ns, seed=100 + n)
    ms = P.mean_values(xs, P.MEAN_W_ISLAND if name.startswith("gpc_ep") else "ms_batch" in flags)
    return spec, hyp, x, xs, ms.ravel(), np.asarray(alpha).ravel(), np.asarray(sW).ravel(), np.asarray(R), flags


CASES = ["gpr_rbf_n1300", "gpr_sum_n1153", "gpr_lin_plus_rbf_n1153", "gpr_dense_ard3_n257", "gpc_ep_matern3_n300",
         "gpc_laplace_rbfard_n257", "gpr_liklaplace_ep_n300"]
_BUILT = {}


def _built(name):
    if name not in _BUILT:
        c = _case(name)
        _BUILT[name] = (c, P.cached(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]))
    return _BUILT[name]


@pytest.mark.parametrize("name", CASES)
def test_forward_substitution_residual_is_a_few_long_double_ulps(name):
    (spec, hyp, x, xs, ms, alpha, sW, R, flags), ref = _built(name)
    L = ref.L.astype(LD)
    B = sW.astype(LD)[:, None] * ref.Ks
    res = np.abs(L @ ref.V - B)
    bound = np.abs(L) @ np.abs(ref.V) + np.abs(B)
    u = float(np.finfo(LD).eps) / 2                     # 2^-64, the unit roundoff of the 80-bit format
    worst = float(np.max(res / np.where(bound > 0, bound, LD(1))))
    print("%s: residual %.3g long-double unit roundoffs of |L||V| + |B|" % (name, worst / u))
    # Higham, Accuracy and Stability, theorem 8.5: substitution leaves |B - L V| <= gamma_n |L| |V|; measured: a few units
    assert np.all(res <= (x.shape[0] + 1) * u * bound) and worst <= 16 * u, worst / u
    # ... and the reference's fs2 is kss - sum V^2 from that V, fmu the plain sum
    assert np.array_equal(ref.fs2, np.maximum(ref.kss - (ref.V * ref.V).sum(axis=0), LD(0)))


def test_solve_chol_ld_residual():
    rng = np.random.RandomState(0)
    x = rng.randn(300, 3)
    A = O.cov_matrix(O.RBF, np.array([np.log(np.sqrt(3.0)), 0.0]), 0, x=x, mode="train") + P.SN ** 2 * np.eye(300)
    R = O.jitchol(A).T
    B = rng.randn(300, 5)
    X = P.solve_chol_ld(R, B)
    Rl = R.astype(LD)
    Y = Rl @ X                                          # R X = R'^-1 B  =>  R' (R X) = B
    res = np.abs(Rl.T @ Y - B.astype(LD))
    bound = np.abs(Rl.T) @ (np.abs(Rl) @ np.abs(X)) + np.abs(B)
    assert np.all(res <= 8 * float(np.finfo(LD).eps) * bound)
    tol, e = P.solve_tolerance(R, B, X)
    r, j = P.check_solve(O.solve_chol(R, B, faithful=False), X, tol)
    assert r <= 1.0 / P.SOLVE_FACTOR + 1e-12
    assert P.check_solve(X.astype(np.float64) * (1 + 1e-9), X, tol)[0] > MUTANT_FACTOR      # a relative 1e-9 is seen


@pytest.mark.parametrize("name", CASES)
def test_both_fp64_cpu_forms_are_inside_the_bar(name):
    (spec, hyp, x, xs, ms, alpha, sW, R, flags), ref = _built(name)
    far = np.arange(ref.ns - 3, ref.ns)
    if spec[0] != "dot":                                # the points at |x| = 50: the cross-covariances have underflowed
        assert np.all(ref.exact()[far]), name
    for form in ("solve", "inverse"):
        fmu, fs2, _ = P.cpu_predict(ref.L, sW, alpha, ref.Ks64, ref.kss64, ms, form)
        worst, where = P.check(fmu, fs2, ref)
        print("%s %s: %.3g of the tolerance at %s" % (name, form, worst, where))
        assert worst <= 1.0, (form, worst, where)
        ex = ref.exact()
        assert np.array_equal(fmu[ex], ms[ex]) and np.array_equal(fs2[ex], ref.kss64[ex])
    # a prefix / selection of the points is a Ref of its own, with its own E_cpu
    sub = ref.take(P.select(ref.ns, 7))
    fmu, fs2, _ = P.cpu_predict(ref.L, sW, alpha, sub.Ks64, sub.kss64, sub.ms, "solve")
    assert sub.ns == 7 and P.check(fmu, fs2, sub)[0] <= 1.0
    # the kernel term dominates: the two CPU forms use a small part of the tolerance they contribute to
    t_mu, t_s2 = ref.tol()
    assert np.all(t_s2 >= P.FLOOR * P.EPS * ref.kss.astype(float)) and np.all(t_mu > 0)


def _mutants(c, ref):
    """name -> (fmu, fs2) of every mutant that applies to this case, computed in fp64 from the unmutated CPU form."""
    spec, hyp, x, xs, ms, alpha, sW, R, flags = c
    n, ns = x.shape[0], xs.shape[0]
    L, Ks, kss = ref.L, ref.Ks64, ref.kss64
    fmu0, fs20, V0 = P.cpu_predict(L, sW, alpha, Ks, kss, ms, "solve")
    out = {}
    out["fmu_last_row_left_out"] = (ms + Ks[:n - 1].T @ alpha[:n - 1], fs20)
    out["fs2_last_row_left_out"] = (fmu0, np.maximum(kss - (V0[:n - 1] ** 2).sum(axis=0), 0.0))
    if n > 128:
        ii, jj = np.tril_indices(128, -1)                # one sub-diagonal entry of the last 128-leaf: the one of median magnitude
        mag = np.abs(L[n - 128:, n - 128:][ii, jj])      # among its nonzero entries (rows of sites with sW = 0 are rows of I)
        nz = np.flatnonzero(mag > 0)
        k = nz[np.argsort(mag[nz])[len(nz) // 2]]
        Lm = L.copy()
        Lm[n - 128 + ii[k], n - 128 + jj[k]] = 0.0
        out["one_entry_of_L_zeroed"] = P.cpu_predict(Lm, sW, alpha, Ks, kss, ms, "solve")[:2]
        W = np.tril(np.linalg.inv(L))
        Wm = W.copy()
        Wm[:, n - 128:] = 0.0                            # the last 128 training columns skipped in the product V = W (sW o Ks)
        Vm = Wm @ (sW[:, None] * Ks)
        out["last_128_columns_skipped"] = (fmu0, np.maximum(kss - (Vm * Vm).sum(axis=0), 0.0))
    i = int(np.flatnonzero(sW > 0)[len(np.flatnonzero(sW > 0)) // 2])
    swm = sW.copy()
    swm[i] *= 1.0 + 1e-6
    out["one_sW_off_by_1e-6"] = P.cpu_predict(L, swm, alpha, Ks, kss, ms, "solve")[:2]
    if "sw_scalar" in flags:
        out["scalar_mean_sW"] = P.cpu_predict(L, np.full(n, sW.mean()), alpha, Ks, kss, ms, "solve")[:2]
    if "ms_batch" in flags:
        assert ns > P.BATCH
        msm = ms.copy()
        msm[P.BATCH:] = ms[:ns - P.BATCH]                # the second batch reads batch 0's prior mean
        out["ms_of_batch_0"] = P.cpu_predict(L, sW, alpha, Ks, kss, msm, "solve")[:2]
    if "kss_const" in flags:
        out["constant_kss"] = P.cpu_predict(L, sW, alpha, Ks, np.full(ns, kss[0]), ms, "solve")[:2]
    V32 = V0.astype(np.float32).astype(np.float64)
    out["V_in_fp32"] = (fmu0, np.maximum(kss - (V32 * V32).sum(axis=0), 0.0))
    return out


@pytest.mark.parametrize("name", CASES)
def test_every_mutant_fails_by_a_factor_of_ten(name):
    c, ref = _built(name)
    seen = {}
    for mname, (fmu, fs2) in _mutants(c, ref).items():
        seen[mname] = P.check(fmu, fs2, ref)
    print(name, {k: "%.3g" % v[0] for k, v in seen.items()})
    for mname, (worst, where) in seen.items():
        assert worst >= MUTANT_FACTOR, (mname, worst, where)


def test_select_keeps_the_layout_of_the_test_points():
    x = np.random.RandomState(1).randn(50, 3)
    xs = P.make_points(x, 300, seed=2)
    assert np.all(np.abs(np.sqrt((xs[-3:] ** 2).sum(axis=1)) - 50.0) < 1e-12)
    assert np.any(np.all(xs[100] == x, axis=1))                                   # the exact copy
    for ns in (1, 5, 127, 129, 257, 300):
        idx = P.select(300, ns)
        assert len(idx) == ns == len(set(idx)) and 100 in idx
        if ns >= 5:
            assert list(idx[-3:]) == [297, 298, 299] and list(idx[:ns // 3]) == list(range(ns // 3))
    assert list(P.select(300, 300)) == list(range(300))
