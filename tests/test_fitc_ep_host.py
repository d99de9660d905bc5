"""CPU: the FITC_EP restatement in tests/fitc_ep_cpu.py against the G21 recordings of the reference (FITC_EP.evaluate,
Core/inf.py:828-944), and the host-side surface of GPC_FITC / inf.FITC_EP that needs no device."""
import numpy as np
import pytest

from conftest import golden, relerr
from fitc_ep_cpu import fitc_ep_fit, fitc_ep_predict
from oracle import gp_oracle as O


def _triple(kind, h, para, x, u):
    return (O.cov_matrix(kind, h, para, z=x, mode="self_test"), O.cov_matrix(kind, h, para, x=u, mode="train"),
            O.cov_matrix(kind, h, para, x=u, z=x, mode="cross"))


def _ders(kind, h, para, x, u):
    return [(O.der_matrix(kind, h, para, z=x, mode="self_test", der=k), O.der_matrix(kind, h, para, x=u, mode="train", der=k),
             O.der_matrix(kind, h, para, x=u, z=x, mode="cross", der=k)) for k in range(len(h))]


@pytest.mark.parametrize("block", [None, 128])
def test_restatement_matches_G21_demo(block):
    g = golden("G21_fitc_ep_demo")
    x, y, u, h = g["x"], g["y"], g["u"], g["cov_hyp"]
    n = x.shape[0]
    m = np.full(n, g["mean_hyp"][0])
    r = fitc_ep_fit(*_triple(O.RBF, h, 0, x, u), y, m, dm=[np.ones(n)], ders=_ders(O.RBF, h, 0, x, u), block=block)
    assert r["sweeps"] == g["sweeps"]
    assert relerr(r["nlZ"], g["nlZ"]) < 1e-12
    assert relerr(r["ttau"], g["ttau"]) < 1e-12 and relerr(r["tnu"], g["tnu"]) < 1e-12
    assert relerr(r["alpha"], g["alpha"]) < 1e-12 and relerr(r["L"], g["L"]) < 1e-12
    assert relerr(r["dnlZ_cov"], g["dnlZ_cov"]) < 1e-12 and relerr(r["dnlZ_mean"], g["dnlZ_mean"]) < 1e-12
    xs = g["xstar"]
    fm, fs2 = fitc_ep_predict(O.cov_matrix(O.RBF, h, 0, x=u, z=xs, mode="cross"), O.cov_matrix(O.RBF, h, 0, z=xs, mode="self_test"),
                              r["alpha"], r["L"], np.full(xs.shape[0], g["mean_hyp"][0]))
    assert relerr(fm, g["pred_fm"].ravel()) < 1e-12 and relerr(fs2, g["pred_fs2"].ravel()) < 1e-12


@pytest.mark.parametrize("nm", ["rbf_N128_nu25", "rbf_N1500_nu160", "rbfard_N1500_nu160"])
def test_restatement_matches_G21_synth(nm):
    g = golden("G21_fitc_ep_" + nm)
    from conftest import synth_cls
    x, y = synth_cls(int(g["N"]), int(g["d"]))
    kind = O.RBFARD if nm.startswith("rbfard") else O.RBF
    h, u = g["cov_hyp"], g["u"]
    r = fitc_ep_fit(*_triple(kind, h, 0, x, u), y, np.zeros(x.shape[0]), ders=_ders(kind, h, 0, x, u), block=128)
    assert r["sweeps"] == g["sweeps"]
    assert relerr(r["nlZ"], g["nlZ"]) < 1e-11
    assert relerr(r["ttau"], g["ttau"]) < 1e-9 and relerr(r["tnu"], g["tnu"]) < 1e-9
    assert relerr(r["alpha"], g["alpha"]) < 1e-8 and relerr(np.diag(r["L"]), g["L_diag"]) < 1e-8
    assert relerr(r["dnlZ_cov"], g["dnlZ_cov"]) < 1e-9


def test_restatement_warm_start_both_branches():
    g = golden("G21_fitc_ep_warm_N512_nu64")
    x, y, u = g["x"], g["y"], g["u"]
    last = (None, None)
    for k in range(3):
        h = g["hyps"][k]
        yk = -y if g["flip"][k] else y
        r = fitc_ep_fit(*_triple(O.RBF, h, 0, x, u), yk, np.zeros(x.shape[0]), last_ttau=last[0], last_tnu=last[1])
        assert r["sweeps"] == g["sweeps%d" % k]
        assert r["warm_kept"] == (None if k == 0 else g["pre_refresh%d" % k] == 1)
        assert relerr(r["nlZ"], g["nlZ%d" % k]) < 1e-12 and relerr(r["ttau"], g["ttau%d" % k]) < 1e-11
        last = (r["ttau"], r["tnu"])
    assert [bool(g["pre_refresh%d" % k] == 1) for k in (1, 2)] == [True, False]      # the fixture covers both branches


def test_gpc_fitc_surface_without_device():
    import pygps_amd as pyGPs
    from pygps_amd import inf, lik
    m = pyGPs.GPC_FITC()
    assert isinstance(m.inffunc, inf.FITC_EP) and isinstance(m.likfunc, lik.Erf)
    assert m.inffunc.last_ttau is None and m.inffunc.last_tnu is None and m.inffunc.sweeps == 0
    with pytest.raises(NotImplementedError, match="FITC_Laplace"):
        m.useInference("Laplace")
    with pytest.raises(Exception, match='Possible inf values are "Laplace"'):
        m.useInference("EP")
    x = np.random.RandomState(0).randn(20, 2)
    m.setData(x, np.where(x[:, :1] > 0, 1.0, 0.0))
    with pytest.raises(Exception, match="labels different from"):
        m.getPosterior()
    with pytest.raises(NotImplementedError):
        inf.FITC_EP().evaluate(pyGPs.mean.Zero(), pyGPs.cov.RBF(), lik.Erf(), x, np.ones((20, 1)), 3)
    with pytest.raises(NotImplementedError):
        inf.FITC_EP().evaluate(pyGPs.mean.Zero(), pyGPs.cov.RBF().fitc(x[:4]), lik.Gauss(), x, np.ones((20, 1)), 3)
