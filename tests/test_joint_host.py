"""CPU: the long-double reference of the joint posterior covariance (tests/joint_ref_ld.py) and its tolerance are tight, the
Cholesky and draw checks of tests/test_gpu_joint.py pass on numpy's own factor, and the package exposes the interface (no GPU).

Posteriors come from the CPU oracle with the input recipes of joint_ref_ld.MODELS, the ones the GPU module fits on the device.

  1  the fp64 CPU evaluation of fcov (both forms of V) passes check_joint on every (model, ns) of the GPU module;
  2  every single-slip mutant of that evaluation is rejected by at least MUTANT_FACTOR = 10 (the smallest factor is printed);
  3  numpy.linalg.cholesky of A = fcov + (noise + jitter) I succeeds on the GPU module's Cholesky cases, its residual and the
     draws F = fmu + Lc z computed in fp64 pass the GPU module's own bounds;
  4  GP.predict_joint / sample_posterior / sample_prior exist and _lib declares the three entry points.
"""
import numpy as np
import pytest

import joint_ref_ld as J
import predict_ref_ld as P
from oracle import gp_oracle as O

LD = P.LD
MUTANT_FACTOR = 10.0
_POST = {}
_REF = {}


def _posterior(name):
    """(x, xs, ms, alpha, sW, R) of a model from the CPU oracle (fp64)."""
    if name in _POST:
        return _POST[name]
    kind, spec, hyp, d, n, nmax, seed = J.MODELS[name]
    hyp = np.array(hyp, dtype=float)
    x, y, xs, ms, m = J.model_data(name)
    if kind == "gpr":
        K = P._cov64(spec, hyp, x, None, "train")
        sn2 = P.SN ** 2
        R = O.jitchol(K / sn2 + np.eye(n)).T
        alpha, sW = O.solve_chol(R, y - m, faithful=False) / sn2, np.ones(n) / P.SN
    elif kind == "gpc_ep":
        r = O.ep_fit(spec[1], hyp, spec[2], x, y, m, nargout=2)
        assert np.any(r["sW"] == 0) and np.any(r["sW"] > 0)
        alpha, sW, R = r["alpha"], r["sW"], r["L"]
    elif kind == "gpc_laplace":
        r = O.laplace_fit(spec[1], hyp, spec[2], x, y, m, nargout=2, faithful=False)
        alpha, sW, R = r["alpha"], r["sW"], r["L"]
    else:
        from lik_laplace_cpu import ep_laplace_fit
        r = ep_laplace_fit(O.cov_matrix(spec[1], hyp, spec[2], x=x, mode="train"), y, m, J.LIK_LAPLACE_LOG_SN)
        alpha, sW, R = r["alpha"], r["sW"], r["L"]
    _POST[name] = (x, xs, ms, np.asarray(alpha, dtype=float).ravel(), np.asarray(sW, dtype=float).ravel(), np.asarray(R, dtype=float))
    return _POST[name]


def _ref(name):
    if name not in _REF:
        kind, spec, hyp = J.MODELS[name][:3]
        x, xs, ms, alpha, sW, R = _posterior(name)
        _REF[name] = J.cached(spec, np.array(hyp, dtype=float), x, xs, ms, alpha, sW, R)
    return _REF[name]


def _cpu(name, ref, form="solve"):
    x, xs, ms, alpha, sW, R = _posterior(name)
    p = ref.pref
    fmu = p.ms + p.Ks64.T @ alpha
    return fmu, J.cpu_joint(p.L, sW, p.Ks64, ref.Kss64, p.kss64, form)[0]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ns", J.FCOV_CASES)
def test_fp64_cpu_evaluation_is_inside_the_bar(name, ns):
    nmax = J.MODELS[name][5]
    ref = _ref(name).take(P.select(nmax, ns))
    for form in ("solve", "inverse"):
        fmu, fcov = _cpu(name, ref, form)
        worst, where = J.check_joint(fmu, fcov, ref)
        print("%s ns=%d %s: %.3g of the tolerance at %s" % (name, ns, form, worst, where))
        assert worst <= 1.0, (form, worst, where)
        assert np.all(fcov.diagonal() >= 0)
    # the diagonal of the reference is predict's fs2, entry by entry
    assert np.array_equal(ref.fcov.diagonal(), ref.pref.fs2)
    assert np.all(ref.tol() >= P.FLOOR * P.EPS * np.sqrt(np.outer(ref.pref.kss, ref.pref.kss)).astype(float))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def _mutants(name, ref):
    x, xs, ms, alpha, sW, R = _posterior(name)
    kind, spec, hyp = J.MODELS[name][:3]
    hyp = np.array(hyp, dtype=float)
    p = ref.pref
    n, ns = x.shape[0], ref.ns
    L, Ks, Kss, kss = p.L, p.Ks64, ref.Kss64, p.kss64
    fcov0, V0 = J.cpu_joint(L, sW, Ks, Kss, kss)
    out = {}
    Vm = V0.copy()
    Vm[n - 1] = 0.0
    out["training_row_left_out_of_V"] = J.finish64(Kss, kss, Vm.T @ Vm)
    if ns > 128:
        Vm = V0.copy()
        Vm[:, :128] = 0.0
        out["128_columns_of_V_left_out"] = J.finish64(Kss, kss, Vm.T @ Vm)
    if kind == "gpr":
        out["sw2_scale_missing"] = J.cpu_joint(L, sW, Ks, Kss, kss, scale=1.0)[0]
    else:
        out["scalar_mean_sW"] = J.cpu_joint(L, np.full(n, sW.mean()), Ks, Kss, kss)[0]
    if name == "rbf_noise300":
        # cov.Noise is sf2 on the 'train' diagonal and 0 on 'self_test': the diagonal has to be the cross block's kind (the dot-product
        # kernels' J = 1e-10 is the same slip, but lies below their kernel bar)
        out["train_diagonal_of_Kss"] = J.finish64(Kss, Kss.diagonal(), V0.T @ V0)
    Km = Kss.copy()
    Km[:, :-1] = Kss[:, 1:]
    Km[np.diag_indices(ns)] = kss
    out["Kss_of_the_next_point"] = J.finish64(Km, kss, V0.T @ V0)
    V32 = V0.astype(np.float32).astype(np.float64)
    out["V_in_fp32"] = J.finish64(Kss, kss, V32.T @ V32)
    C = fcov0.copy()
    iu = np.triu_indices(ns, 1)
    C[iu] = Kss[iu]                                        # the product ran on the lower tiles and the mirror was forgotten
    out["not_mirrored"] = C
    return out


MUTANT_CASES = [("rbf300", 300), ("rbf1100", 300), ("lin_rbf1100", 300), ("ep300", 129), ("lap300", 129), ("liklap300", 129),
                ("dense300", 129), ("rbf_noise300", 129)]
_SMALLEST = {}


@pytest.mark.parametrize("name,ns", MUTANT_CASES)
def test_every_mutant_fails_by_a_factor_of_ten(name, ns):
    nmax = J.MODELS[name][5]
    idx = P.select(nmax, ns)
    ref = _ref(name).take(idx)
    fmu = _cpu(name, ref)[0]
    seen = {m: J.check_joint(fmu, C, ref) for m, C in _mutants(name, ref).items()}
    print(name, {k: "%.3g" % v[0] for k, v in seen.items()})
    for m, (worst, where) in seen.items():
        _SMALLEST[m] = min(_SMALLEST.get(m, np.inf), worst)
        assert worst >= MUTANT_FACTOR, (m, worst, where)
    print("smallest factor so far: %.3g (%s)" % min((v, k) for k, v in _SMALLEST.items()))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ns,noise", J.CHOL_CASES)
def test_cholesky_and_draw_checks_pass_on_numpys_factor(name, ns, noise):
    kind, spec, hyp = J.MODELS[name][:3]
    hyp = np.array(hyp, dtype=float)
    x, _, _, alpha, sW, R = _posterior(name)
    xs = J.chol_points(name, ns)
    Ks, Kss = P._cov64(spec, hyp, x, xs, "cross"), P._cov64(spec, hyp, xs, None, "train")
    kss = np.asarray(P._cov64(spec, hyp, None, xs, "self_test"), dtype=float).reshape(ns)
    fmu = P.MEAN_C + Ks.T @ alpha
    fcov = J.cpu_joint(np.ascontiguousarray(R.T), sW, Ks, Kss, kss)[0]
    fcov = np.tril(fcov) + np.tril(fcov, -1).T           # one triangle, mirrored: what the device hands out
    add = P.SN ** 2 if noise else 1e-8 * float(np.mean(kss))
    A = fcov.copy()
    A[np.diag_indices(ns)] += add
    Lc = np.linalg.cholesky(A)                            # must succeed: the GPU module's cases are chosen here
    r = J.chol_residual(Lc, A)
    print("%s ns=%d noise=%s: chol residual %.3g (in units of 2^-53: %.3g)" % (name, ns, noise, r, r / P.EPS))
    assert r <= (ns + 1) * P.EPS                          # Higham, theorem 10.3: |A - L L'| <= gamma_(n+1) |L| |L|'
    for nsamp in (1, 5):
        z = np.random.default_rng(5).standard_normal((ns, nsamp))
        F = fmu[:, None] + Lc @ z
        ex = J.draws_excess(F, fmu, Lc, z)
        assert ex <= 1.0, ex
        assert J.draws_excess(F * (1 + 1e-9), fmu, Lc, z) > MUTANT_FACTOR


def test_prior_cases_factor_on_the_cpu():
    for spec, hyp in ((("oracle", O.RBF, 0), [J.LOG_ELL3, 0.0]), (("dot", J.LIN_RBF), J.LIN_RBF_HYP)):
        for ns in (129, 300):
            xs = np.random.RandomState(ns).randn(ns, 3)
            K = np.array(P._cov64(spec, np.array(hyp), xs, None, "train"))
            A = K + 1e-8 * float(np.mean(K.diagonal())) * np.eye(ns)
            assert J.chol_residual(np.linalg.cholesky(A), A) <= (ns + 1) * P.EPS


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_package_exposes_the_joint_interface():
    import pygps_amd as pyGPs
    from pygps_amd import _lib
    for name in ("predict_joint", "sample_posterior", "sample_prior"):
        assert callable(getattr(pyGPs.GP, name, None)), name
    for name in ("pgp_predict_joint", "pgp_predict_joint_dense", "pgp_sample_mvn"):
        assert name in _lib.SIGNATURES, name
    assert _lib.JOINT_MAX_POINTS == 16384


def test_draws_come_from_z_or_from_the_generator():
    import pygps_amd as pyGPs
    z = pyGPs.GP._draws(7, 3, 5, None)
    assert np.array_equal(z, np.random.default_rng(5).standard_normal((7, 3)))
    assert np.array_equal(pyGPs.GP._draws(7, 3, np.random.default_rng(5), None), z)
    assert np.array_equal(pyGPs.GP._draws(7, 1, None, z[:, 0]), z[:, :1])
    with pytest.raises(Exception):
        pyGPs.GP._draws(7, 3, None, np.zeros((6, 3)))
    with pytest.raises(Exception):
        pyGPs.GPC()._noise_var(True)
    m = pyGPs.GPR()
    m.setNoise(np.log(0.05))
    assert m._noise_var(True) == float(np.exp(2.0 * np.log(0.05))) and m._noise_var(False) == 0.0
