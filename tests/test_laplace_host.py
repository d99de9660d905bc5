"""Laplace inference, host side (no GPU): the likelihoods' Laplace modes against the reference (G20_lik_laplace_modes,
tests/golden/make_golden_laplace.py) and the routing of useInference."""
import os

import numpy as np
import pytest

import pygps_amd as pyGPs
from pygps_amd import inf, lik

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def _rel(got, want):
    return np.max(np.abs(np.asarray(got) - want)) / max(np.max(np.abs(want)), 1e-300)


def _d3lp_err(got, want, f, y, n_p):
    """d3lp cancels where y f << 0: the error is measured against its largest term, per point."""
    scale = np.maximum.reduce([np.abs(2 * n_p ** 3), np.abs(3 * f * n_p ** 2), np.abs((f ** 2 - 1) * n_p), np.full_like(f, 1e-300)])
    return np.max(np.abs(got - want) / scale)


@pytest.mark.parametrize("tag,yv", [("pos", 1.0), ("neg", -1.0)])
def test_erf_laplace_mode_matches_reference(tag, yv):
    z = _gold("G20_lik_laplace_modes")
    f = z["f"]
    y = yv * np.ones_like(f)
    lp, dlp, d2lp, d3lp = lik.Erf().evaluate(y, f, None, inf.Laplace(), None, 4)
    for got, key in ((lp, "lp"), (dlp, "dlp"), (d2lp, "d2lp")):
        want = z["erf_%s_%s" % (tag, key)]
        assert np.all(np.abs(got - want) <= 1e-13 * np.maximum(np.abs(want), 1e-300)), key
    n_p = np.abs(dlp)
    assert _d3lp_err(d3lp, z["erf_%s_d3lp" % tag], f, y, n_p) <= 1e-13
    # nargout 1 .. 3 are prefixes of the same tuple
    assert np.array_equal(lik.Erf().evaluate(y, f, None, inf.Laplace(), None, 1), lp)
    assert len(lik.Erf().evaluate(y, f, None, inf.Laplace(), None, 3)) == 3


def test_erf_laplace_der_mode_is_empty():
    z = _gold("G20_lik_laplace_modes")
    assert lik.Erf().evaluate(np.ones_like(z["f"]), z["f"], None, inf.Laplace(), 0, 3) == []
    assert int(z["erf_der"]) == 0


def test_gauss_laplace_modes_match_reference():
    z = _gold("G20_lik_laplace_modes")
    g = lik.Gauss(float(z["gauss_log_sn"]))
    f, y = z["f"], z["gauss_y"]
    out = g.evaluate(y, f, None, inf.Laplace(), None, 4)
    for got, key in zip(out, ("lp", "dlp", "d2lp", "d3lp")):
        want = z["gauss_" + key]
        assert np.all(np.abs(got - want) <= 1e-13 * np.maximum(np.abs(want), 1e-300) + (0 if key != "d3lp" else 0.0)), key
    der = g.evaluate(y, f, None, inf.Laplace(), 0, 3)
    for got, key in zip(der, ("lp_dhyp", "dlp_dhyp", "d2lp_dhyp")):
        want = z["gauss_" + key]
        assert np.all(np.abs(got - want) <= 1e-13 * np.maximum(np.abs(want), 1e-300)), key


def test_use_inference_laplace_routes():
    for cls in (pyGPs.GPC, pyGPs.GPR):
        m = cls()
        m.useInference("Laplace")
        assert isinstance(m.inffunc, inf.Laplace)
        assert m.inffunc.last_alpha is None and m.inffunc.newton_steps == 0
        m.useInference("EP")
        assert isinstance(m.inffunc, inf.EP)
        with pytest.raises(Exception):
            m.useInference("VB")
    with pytest.raises(Exception):
        pyGPs.GPR_FITC().useInference("Laplace")


def test_laplace_rejects_other_likelihoods_without_touching_the_device():
    class Other(lik.Likelihood):
        pass
    with pytest.raises(NotImplementedError):
        inf.Laplace()._lik_args(Other())
    assert inf.Laplace()._lik_args(lik.Erf())[0] == 0
    assert inf.Laplace()._lik_args(lik.Gauss(0.1))[2] == 1


def test_warm_start_resets_clear_last_alpha():
    from pygps_amd import opt
    m = pyGPs.GPC()
    m.useInference("Laplace")
    m.inffunc.last_alpha = np.ones((5, 1))
    opt.ShardedMinimize._cold_start(m)
    assert m.inffunc.last_alpha is None
