"""Seeded multi-class data for the GPMC fixtures (G24) and tests: Gaussian blobs, one per class, in permuted order.

The recipe (tests/golden/make_golden_gpmc.py) and the tests both import this module, so the fixtures store seeds and
results, not inputs.  Everything is drawn from ONE numpy RandomState in a fixed order: the class centres, the training
points class by class, the permutation, the classes of the test points, the test points."""
import numpy as np


def blobs(seed, counts, d, ns, sep=1.0):
    """x (n, d), y (n, 1) integer-valued class labels 0 .. len(counts)-1 in permuted order, xs (ns, d).

    counts: training points per class.  Class k is N(c_k, I) with centres c_k = sep * N(0, I): unit-variance blobs whose
    centres are about sep * sqrt(2 d) apart, so sep sets how much the classes overlap."""
    rng = np.random.RandomState(seed)
    C = len(counts)
    centres = sep * rng.randn(C, d)
    x = np.concatenate([centres[k] + rng.randn(counts[k], d) for k in range(C)])
    y = np.concatenate([np.full(counts[k], k, dtype=float) for k in range(C)])
    perm = rng.permutation(x.shape[0])
    x, y = x[perm], y[perm].reshape(-1, 1)
    ks = rng.randint(0, C, size=ns)
    xs = centres[ks] + rng.randn(ns, d)
    return x, y, xs


# name -> arguments of blobs(); the kernels and means of the fixtures are built from these names by the recipe
# (reference objects) and by the tests (pygps_amd objects or the oracle's kinds): see SHAPES' users
SHAPES = {
    "fit_c10_d64": dict(seed=2401, counts=[200] * 10, d=64, ns=1000, sep=0.5),
    "fit_c5_uneven": dict(seed=2402, counts=[150, 90, 200, 37, 129], d=16, ns=300, sep=0.6),
    "fit_default": dict(seed=2403, counts=[40] * 4, d=5, ns=100, sep=0.8),
    "fit_ard_const": dict(seed=2404, counts=[60] * 4, d=16, ns=150, sep=0.6),
    "fit_program": dict(seed=2405, counts=[70] * 3, d=4, ns=120, sep=0.9),
    "fit_laplace": dict(seed=2403, counts=[40] * 4, d=5, ns=100, sep=0.8),
    "opt_default": dict(seed=2406, counts=[40] * 4, d=5, ns=100, sep=0.8),
    "opt_prior": dict(seed=2406, counts=[40] * 4, d=5, ns=100, sep=0.8),
}


def ard_ells(d):
    """log length scales of the fit_ard_const fixture's RBFard."""
    return list(np.log(np.sqrt(d)) + np.linspace(-0.3, 0.3, d))


def prior(name, cov, mean):
    """(mean, kernel) of fixture ``name`` built from the given ``cov`` / ``mean`` modules (the reference's or pygps_amd's), or
    (None, None) where the fixture never calls setPrior."""
    d = SHAPES[name]["d"]
    if name == "fit_c10_d64":
        return None, cov.RBF(np.log(np.sqrt(64.0)), 0.0)
    if name == "fit_c5_uneven":
        return None, cov.RBF(np.log(4.0), 0.0)
    if name == "fit_ard_const":
        return mean.Const(0.2), cov.RBFard(log_ell_list=ard_ells(d), log_sigma=0.1)
    if name == "fit_program":
        return None, cov.RBF(np.log(2.0), 0.0) + cov.Matern(np.log(2.5), d=5, log_sigma=-0.2) * cov.RBFunit(np.log(3.0))
    if name == "opt_prior":
        return None, cov.RBF(np.log(2.0), 0.0)
    return None, None


def oracle_prior(name):
    """(kind, hyp, para, constant mean) of fixture ``name`` in the oracle's terms (oracle/gp_oracle.py)."""
    from oracle import gp_oracle as O
    d = SHAPES[name]["d"]
    if name == "fit_c10_d64":
        return O.RBF, np.array([np.log(np.sqrt(64.0)), 0.0]), 0, 0.0
    if name == "fit_c5_uneven":
        return O.RBF, np.array([np.log(4.0), 0.0]), 0, 0.0
    if name == "fit_ard_const":
        return O.RBFARD, np.array(ard_ells(d) + [0.1]), 0, 0.2
    if name == "fit_program":
        tree = ("sum", ("leaf", O.RBF, 0), ("prod", ("leaf", O.MATERN, 5), ("leaf", O.RBFUNIT, 0)))
        return tree, np.array([np.log(2.0), 0.0, np.log(2.5), -0.2, np.log(3.0)]), 0, 0.0
    if name == "opt_prior":
        return O.RBF, np.array([np.log(2.0), 0.0]), 0, 0.0
    return O.RBF, np.array([0.0, 0.0]), 0, 0.0            # cov.RBF()'s defaults
