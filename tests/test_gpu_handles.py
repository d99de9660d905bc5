"""Pool ownership of the posterior handles, engine by engine through inf.py: a fit with all gradients, its posterior dropped, leaves
the context's pools (idle factor and scratch buffers, buffers that are out) exactly as the same fit and drop left them before -- a
handle that keeps or loses a pool buffer shows up as a difference.  n = 129 (two 128-blocks, one point of padding short of empty),
d = 2, nu = 40."""
import gc

import numpy as np
import pytest

from pool_state import pool_state

pytestmark = pytest.mark.gpu

N, D, NU = 129, 2, 40


def _data():
    rng = np.random.RandomState(11)
    x = rng.randn(N, D)
    f = np.sin(x @ np.array([[1.0], [-0.7]]))
    return x, f + 0.1 * rng.randn(N, 1), np.where(f > 0, 1.0, -1.0)


def _dense_tree(cov):
    k = cov.RBFard(D=D) + cov.RBFard(D=D, log_ell_list=[0.3, -0.2]) + cov.RBFard(D=D, log_ell_list=[-0.4, 0.5], log_sigma=-1.0)
    return k                                        # three ARD leaves: not a device program


MAKERS = {          # name -> (engine, kernel, likelihood, labels instead of targets)
    "exact-program": ("Exact", lambda cov, u: cov.RBF(0.1, 0.2), "Gauss", False),
    "exact-dense": ("Exact", lambda cov, u: _dense_tree(cov), "Gauss", False),
    "ep-program": ("EP", lambda cov, u: cov.RBF(0.1, 0.2), "Erf", True),
    "ep-dense": ("EP", lambda cov, u: _dense_tree(cov), "Erf", True),
    "laplace-program": ("Laplace", lambda cov, u: cov.RBF(0.1, 0.2), "Erf", True),
    "fitc-exact": ("FITC_Exact", lambda cov, u: cov.RBF(0.1, 0.2).fitc(u), "Gauss", False),
    "fitc-ep": ("FITC_EP", lambda cov, u: cov.RBF(0.1, 0.2).fitc(u), "Erf", True),
}


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_fit_and_drop_leaves_the_pools_as_they_were(lib, name):
    import pygps_amd as pyGPs
    from pygps_amd import inf
    engine, kernel, likname, labels = MAKERS[name]
    x, y, lab = _data()
    k = kernel(pyGPs.cov, x[:NU].copy())
    assert inf._dense_route(k) == name.endswith("dense")
    states = []
    for _ in range(2):
        out = getattr(inf, engine)().evaluate(pyGPs.mean.Zero(), k, getattr(pyGPs.lik, likname)(), x, lab if labels else y, 3)
        post, nlZ, dnlZ = out
        assert np.isfinite(nlZ) and np.all(np.isfinite(dnlZ.cov)) and np.all(np.isfinite(post.alpha))
        assert (hasattr(post, "fitc")) == name.startswith("fitc")
        del out, post
        gc.collect()
        states.append(pool_state(lib))
    print("pool state %s: %s" % (name, states[0]))
    assert states[1] == states[0], states
