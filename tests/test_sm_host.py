"""CPU: the host-side surface of cov.SM that needs no device (constructor, hyper layout, exceptions, device limits, initSMhypers,
composites take the dense route) and the long-double reference tests/sm_ref_ld.py -- against the D = 1 recordings of the
reference (tests/golden/G23_sm_kernels_*.npz) within its own bar, and its derivatives against central differences of its value
for D = 1, 3, 4."""
import numpy as np
import pytest

from conftest import golden
import sm_ref_ld as S


def _hyp(Q, D, rng):
    return np.concatenate([np.log(rng.uniform(0.2, 0.6, Q)), np.log(rng.uniform(0.1, 0.9, D * Q)),
                           np.log(rng.uniform(0.1, 0.4, D * Q))])


def test_constructor_layout_and_para():
    from pygps_amd import cov, _lib
    k = cov.SM(3, [0.1 * i for i in range(9)])
    assert k.para == [3] and k.hyp == [0.1 * i for i in range(9)]
    assert k._kind == _lib.COV_SM == 11
    assert k._device_params() == (_lib.COV_SM, 3, 0)
    assert k._program(0) is None
    np.random.seed(4)
    r = cov.SM(Q=2, D=3)
    np.random.seed(4)
    assert r.hyp == list(np.random.random(2 * 7)) and r.para == [2]
    assert cov.SM().hyp == [] and cov.SM().para == [0]
    # layout: (j, q) of the means at Q + j Q + q, of the scales at Q + Q D + j Q + q
    Q, D = 2, 3
    assert S.decode_der(1, Q, D) == (0, -1, 1)
    assert S.decode_der(Q + 2 * Q + 1, Q, D) == (1, 2, 1)
    assert S.decode_der(Q + Q * D + 1 * Q + 0, Q, D) == (2, 1, 0)


def test_exceptions_before_the_device_is_touched():
    from pygps_amd import cov
    k = cov.SM(2, [0.0] * 6)
    x = np.zeros((4, 1))
    with pytest.raises(Exception, match="Specify the mode"):
        k.getCovMatrix(x=x)
    with pytest.raises(Exception, match="Specify at least one"):
        k.getCovMatrix(mode="train")
    with pytest.raises(Exception, match="Specify both"):
        k.getCovMatrix(x=x, mode="cross")
    with pytest.raises(Exception, match="Specify the index"):
        k.getDerMatrix(x=x, mode="train")
    with pytest.raises(Exception, match="Wrong derivative entry in SM"):
        k.getDerMatrix(x=x, mode="train", der=6)
    with pytest.raises(AssertionError):                    # Q != len(hyp) / (1 + 2 D)
        k.getCovMatrix(x=np.zeros((4, 2)), mode="train")
    with pytest.raises(AssertionError):                    # a ragged hyp: 7 / 3 != 2 (true division, as the reference)
        cov.SM(2, [0.0] * 7).getCovMatrix(x=x, mode="train")
    with pytest.raises(Exception, match="Wrong derivative entry in SM"):
        k.getDerMatrix(x=x, mode="train", der=-1)


def test_device_limits_raise_and_name_the_limit():
    from pygps_amd import cov
    k = cov.SM(1, [0.0] * (1 + 2 * 17))
    with pytest.raises(Exception, match="D <= 16"):
        k.getCovMatrix(x=np.zeros((3, 17)), mode="train")
    with pytest.raises(Exception, match="D <= 16"):
        k.getDerMatrix(z=np.zeros((3, 17)), mode="self_test", der=0)
    with pytest.raises(Exception, match="D <= 16"):
        k._device_params()                                 # what a fit asks for
    k = cov.SM(86, [0.0] * (86 * 3))                       # 258 hypers
    with pytest.raises(Exception, match=r"Q \(1 \+ 2 D\) <= 255"):
        k.getCovMatrix(x=np.zeros((3, 1)), mode="train")
    with pytest.raises(Exception, match=r"Q \(1 \+ 2 D\) <= 255"):
        k._device_params()
    cov.SM(85, [0.0] * 255)._device_params()               # the largest D = 1 mixture passes
    cov.SM(7, [0.0] * (7 * 33))._device_params()           # and the largest at D = 16 (231 hypers)


def test_initSMhypers_as_documented():
    from pygps_amd import cov
    rng = np.random.RandomState(0)
    n, D, Q = 50, 3, 4
    x = rng.rand(n, D) * np.array([1.0, 5.0, 0.2])
    y = rng.randn(n, 1)
    k = cov.SM(Q, [])
    np.random.seed(11)
    k.initSMhypers(x, y)
    h = np.array(k.hyp)
    assert isinstance(k.hyp, list) and len(k.hyp) == Q * (1 + 2 * D) and np.all(np.isfinite(h))
    assert np.allclose(np.exp(h[:Q]), np.std(y) / Q)
    m = np.exp(h[Q:Q + Q * D]).reshape(D, Q)
    s = np.exp(h[Q + Q * D:]).reshape(D, Q)
    np.random.seed(11)
    for j in range(D):
        sh = np.abs(x[:, j][:, None] - x[:, j][None, :])
        nyq = 0.5 / max(sh[sh > 0].min(), 1e-6)
        assert np.all(m[j] > 0) and np.all(m[j] <= nyq)
        assert np.allclose(m[j], nyq * np.random.ranf(Q))                     # the reference's draw order: means, then scales
        assert np.allclose(s[j], 1.0 / (max(sh.max(), 1e-6) * np.random.ranf(Q)))
    k2 = cov.SM(Q, [])
    np.random.seed(11)
    k2.initSMhypers(x, y)
    assert k2.hyp == k.hyp                                                    # reproducible under np.random.seed
    k1 = cov.SM(2, [])
    k1.initSMhypers(np.array([[0.3]]), np.array([[1.0], [2.0]]))             # n = 1: no shifts, unit defaults
    assert len(k1.hyp) == 6 and np.all(np.isfinite(k1.hyp))


def test_composites_with_SM_are_not_device_programs():
    from pygps_amd import cov
    sm = cov.SM(2, [0.0] * 6)
    for k in (sm + cov.Noise(-1.0), sm * cov.RBF(0.1, 0.2), sm * 0.5, cov.RBF() + sm * cov.Const(0.1)):
        assert k._on_device() is False and k._program(0) is None
    assert (sm + cov.Noise(-1.0)).hyp == [0.0] * 6 + [-1.0]


@pytest.mark.parametrize("nm", ["q1", "q3"])
def test_sm_ref_ld_matches_the_reference_recordings_within_the_bar(nm):
    """The reference's own fp64 evaluation (D = 1; value and every derivative, three modes) obeys the derived bar."""
    g = golden("G23_sm_kernels_" + nm)
    x, z, hyp = g["x"], g["z"], g["hyp"]
    Q = len(hyp) // 3
    worst = 0.0
    for mode, kw in (("train", dict(x=x)), ("cross", dict(x=x, z=z)), ("self_test", dict(z=z))):
        for der in [None] + list(range(len(hyp))):
            ref, bar = S.sm_matrix(hyp, Q, mode=mode, der=der, **kw)
            got = g["K_%s" % mode] if der is None else g["dK%d_%s" % (der, mode)]
            assert got.shape == ref.shape
            e = float(np.max(np.abs(got.astype(S.LD) - ref).astype(np.float64) / bar))
            assert e <= 1.0, (nm, mode, der, e)
            worst = max(worst, e)
    print("\nworst |reference - long double| / bar, %s: %.3g" % (nm, worst))


@pytest.mark.parametrize("D,Q", [(1, 3), (3, 4), (4, 2)])
def test_sm_ref_ld_derivatives_against_central_differences(D, Q):
    """Central differences of the long-double value with h = 1e-6 in log space: truncation h^2 / 6 |d^3 k| (|d^3 k| <= ~1e4 at
    |a| <= 25) and rounding 2^-63 |k| / h, both below 1e-7 of the largest entry."""
    rng = np.random.RandomState(10 * D + Q)
    x, z = rng.rand(30, D) * 4, rng.rand(20, D) * 4
    hyp = _hyp(Q, D, rng)
    h = S.LD(1e-6)
    for der in range(Q * (1 + 2 * D)):
        dK, _ = S.sm_matrix(hyp, Q, x=x, z=z, mode="cross", der=der)
        e = np.zeros(len(hyp), dtype=S.LD)
        e[der] = h
        Kp, _ = S.sm_matrix(hyp.astype(S.LD) + e, Q, x=x, z=z, mode="cross")
        Km, _ = S.sm_matrix(hyp.astype(S.LD) - e, Q, x=x, z=z, mode="cross")
        fd = (Kp - Km) / (2 * h)
        assert float(np.max(np.abs(fd - dK))) <= 1e-7 * max(1.0, float(np.max(np.abs(dK)))), (D, Q, der)
        d64 = S.sm_fp64(hyp, Q, x=x, z=z, mode="cross", der=der)
        _, bar = S.sm_matrix(hyp, Q, x=x, z=z, mode="cross", der=der)
        assert float(np.max(np.abs(d64.astype(S.LD) - dK).astype(np.float64) / bar)) <= 1.0      # a plain fp64 evaluation obeys the bar


def test_self_test_mode_and_hadamard_reference_consistency():
    rng = np.random.RandomState(2)
    D, Q, n = 2, 3, 40
    x = rng.rand(n, D) * 3
    hyp = _hyp(Q, D, rng)
    K, _ = S.sm_matrix(hyp, Q, z=x, mode="self_test")
    assert K.shape == (n, 1) and np.allclose(K.astype(float), np.sum(np.exp(hyp[:Q])))
    for der in range(len(hyp)):
        dK, _ = S.sm_matrix(hyp, Q, z=x, mode="self_test", der=der)
        want = np.exp(hyp[der]) if der < Q else 0.0
        assert np.allclose(dK.astype(float), want)
    A = rng.randn(n, n) / np.sqrt(n)
    B, al, wv = np.eye(n) + 0.3 * (A + A.T) / 2, rng.randn(n), rng.uniform(0.2, 1.5, n)
    (s0, b0), (s1, b1) = S.sm_hadamard_ref(hyp, Q, x, [(B, al, None, 0.3), (B, al, wv, 1.0)], rows=16, threads=2)
    for (s, b), W, sn2 in ((( s0, b0), np.full((n, n), 1 / 0.3), 0.3), ((s1, b1), np.outer(wv, wv), 1.0)):
        Qm = B * W - np.outer(al, al)
        for der in range(len(hyp)):
            dK = S.sm_fp64(hyp, Q, x=x, mode="train", der=der)
            assert abs(float(s[der]) - float(np.sum(Qm * dK))) <= b[der]
        assert abs(float(s[-1]) - sn2 * np.trace(Qm)) <= b[-1]
