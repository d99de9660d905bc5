"""GPU: the structural zeros the exact fit's bulk trailing updates no longer multiply (csrc/gemm_tile.h, csrc/sweep.hip
trailing_skip; option skip_zeros).

* tile level, through pgp_test_gemm_zskip: the k-clip of first-touch rows that are upper-trapezoidal in A (GemmArgs::zf_upper)
  changes NO bit of C, and the clip really does not read what it promises not to read;
* fit level: pgp_exact_fit with the option on against off, bit for bit, over the panel counts, panel widths and schedules the
  trailing-update builders serve.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import relerr, synth_reg

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b):
    """bit-for-bit: tells -0 from +0 and compares NaNs by payload (np.array_equal does neither)"""
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _zskip(lib, tile, A, B, C0, Cin=None, tri=0, mask_diag=0, zero_from=0, zf_upper=0, alpha=-1.0, beta=1.0):
    """C = beta Cin + alpha A B' through the MFMA tile kernel; numpy (row-major) in, the device's column-major views are the transposes"""
    from pygps_amd import _lib
    M, K = A.shape
    N = B.shape[0]
    At, Bt = np.ascontiguousarray(A.T), np.ascontiguousarray(B.T)
    Ct = np.ascontiguousarray(C0.T)
    Cit = None if Cin is None else np.ascontiguousarray(Cin.T)
    _lib.check(lib.pgp_test_gemm_zskip(_lib.ctx(), tile, tri, mask_diag, zero_from, zf_upper, alpha, beta, _lib.ptr(At), M,
                                       _lib.ptr(Bt), N, None if Cit is None else _lib.ptr(Cit), _lib.ptr(Ct), M, M, N, K))
    return np.ascontiguousarray(Ct.T)


@pytest.fixture(scope="module")
def trapezoid():
    """M = 640, N = 256, K = 512, zero_from = 128: A random in rows < 128, upper-trapezoidal with exact zeros (A(i, k) = 0 for
    k < i - 128) in rows 128 ... 639; C rows >= 128 are NaN (first touch: never read); the numpy reference, computed once"""
    rng = np.random.RandomState(11)
    M, N, K, zf = 640, 256, 512, 128
    A = rng.randn(M, K)
    i, k = np.arange(M)[:, None], np.arange(K)[None, :]
    A[(i >= zf) & (k < i - zf)] = 0.0
    B = rng.randn(N, K)
    C0 = rng.randn(M, N)
    C0[zf:] = np.nan
    ref = -(A @ B.T)
    ref[:zf] += C0[:zf]
    # the 128-aligned region the clip promises not to read: k < 128 floor((i - 128) / 128)
    poison = (i >= zf) & (k < 128 * ((i - zf) // 128))
    Ap = A.copy()
    Ap[poison] = np.nan
    for a in (A, B, C0, ref, Ap):
        a.setflags(write=False)
    return dict(M=M, N=N, K=K, zf=zf, A=A, B=B, C0=C0, ref=ref, Ap=Ap, npoison=int(poison.sum()))


@pytest.mark.parametrize("tile", [128, 64])
@pytest.mark.parametrize("inplace", [True, False])
def test_k_clip_of_upper_trapezoidal_first_touch_rows(lib, trapezoid, tile, inplace):
    """Flag on == flag off bit for bit, both match numpy to 1e-12, and with the flag on NaNs in the region the clip promises not to
    read change nothing.  beta = 1 with NaN in C's first-touch rows: those are never read either."""
    t = trapezoid
    assert t["npoison"] == 128 * (128 + 256 + 384)
    if inplace:
        start, cin = t["C0"], None
    else:
        start, cin = np.full((t["M"], t["N"]), 7.0), t["C0"]          # every entry of C is written
    out = {}
    for name, A, zu in (("off", t["A"], 0), ("on", t["A"], 1), ("on_poisoned", t["Ap"], 1)):
        out[name] = _zskip(lib, tile, A, t["B"], start, Cin=cin, zero_from=t["zf"], zf_upper=zu)
    err_off, err_on = relerr(out["off"], t["ref"]), relerr(out["on"], t["ref"])
    print("tile %d inplace %s: relerr off %.3e on %.3e" % (tile, inplace, err_off, err_on))
    assert np.isfinite(out["off"]).all()
    assert err_off < 1e-12 and err_on < 1e-12
    assert _same_bits(out["on"], out["off"])
    assert _same_bits(out["on_poisoned"], out["on"])


def _fit_all(lib, ctx, N, hyp, m, dm):
    from pygps_amd import _lib
    alpha = np.zeros(N); nlZ = np.zeros(1); g = np.zeros(4); fh = C.c_void_p()
    rc = lib.pgp_exact_fit(ctx, 0, _lib.ptr(hyp), 2, 0, 0, float(np.log(0.1)), _lib.ptr(m), _lib.ptr(dm), 1, 3,
                           _lib.ptr(alpha), _lib.ptr(nlZ), _lib.ptr(g), C.byref(fh))
    if rc != 0:
        return rc, None
    L = np.zeros((N, N))
    _lib.check(lib.pgp_factor_to_host(ctx, fh, _lib.ptr(L)))
    lib.pgp_factor_free(ctx, fh)
    return 0, (nlZ, alpha, g, np.tril(L))


SKIPS = {"off": dict(skip_zeros=0), "on": dict(skip_zeros=1)}


@pytest.mark.parametrize("N,opts", [(1024, {}), (1536, {}), (1664, {}), (3072, dict(nb_outer=8)), (4608, dict(sched=2)),
                                    (7168, dict(sched=1)), (7168, dict(sched=0))],
                         ids=["1024", "1536", "1664", "3072-nb_outer8", "4608-sched2", "7168-sched1", "7168-sched0"])
def test_fit_is_bit_identical_with_the_skips(lib, N, opts):
    """pgp_exact_fit, nargout 3: nlZ, alpha, dnlZ and tril(L) with skip_zeros = 1 equal the skip_zeros = 0 fit's BIT FOR BIT.
    N = 1024: two panels, no look-ahead; 1536: three, look-ahead; 1664: a partial last panel; 3072 with nb_outer = 8: 1024-wide
    panels (tile rows r up to 7 in the own inverse rows); 4608 under sched 2 (TU_d / TU_r); 7168 under sched 1 and 0."""
    from pygps_amd import _lib
    d = 16
    x, y = synth_reg(N, d, seed=N)
    x = _lib.f64(x); y = _lib.f64(y).ravel()
    hyp = _lib.f64(np.array([np.log(np.sqrt(d)), 0.2])); m = np.full(N, float(y.mean())); dm = np.ones((1, N))
    ctx = _lib.ctx()
    _lib.check(lib.pgp_set_data(ctx, _lib.ptr(x), N, d, _lib.ptr(y)))
    res = {}
    try:
        for k, v in opts.items():
            _lib.check(lib.pgp_set_option(ctx, k.encode(), v))
        for name, sk in SKIPS.items():
            for k, v in sk.items():
                _lib.check(lib.pgp_set_option(ctx, k.encode(), v))
            rc, res[name] = _fit_all(lib, ctx, N, hyp, m, dm)
            assert rc == 0, (name, rc)
    finally:
        for k, v in dict(sched=-1, nb_outer=0, skip_zeros=1).items():
            lib.pgp_set_option(ctx, k.encode(), v)
    ref = res["off"]
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all() and np.isfinite(ref[3]).all()
    for a, b in zip(ref, res["on"]):
        assert _same_bits(a, b)


def test_non_positive_definite_input_reports_the_same_pivot(lib):
    """N = 1536 (three panels): duplicated points and a tiny noise -- the fit fails with the same `info` (first bad pivot) whether
    the skip is on or off."""
    from pygps_amd import _lib
    N, d = 1536, 3
    rng = np.random.RandomState(4)
    x = rng.randn(N, d)
    x[900:] = x[:636]
    x = _lib.f64(x); y = _lib.f64(rng.randn(N))
    hyp = _lib.f64(np.array([2.0, 3.0])); m = np.zeros(N); dm = np.ones((1, N))
    ctx = _lib.ctx()
    _lib.check(lib.pgp_set_data(ctx, _lib.ptr(x), N, d, _lib.ptr(y)))
    info = {}
    try:
        for name, sk in SKIPS.items():
            for k, v in sk.items():
                _lib.check(lib.pgp_set_option(ctx, k.encode(), v))
            alpha = np.zeros(N); nlZ = np.zeros(1); g = np.zeros(4)
            info[name] = lib.pgp_exact_fit(ctx, 0, _lib.ptr(hyp), 2, 0, 0, -18.0, _lib.ptr(m), _lib.ptr(dm), 1, 3,
                                           _lib.ptr(alpha), _lib.ptr(nlZ), _lib.ptr(g), None)
    finally:
        lib.pgp_set_option(ctx, b"skip_zeros", 1)
    print("info", info)
    assert info["off"] > 0
    assert info["on"] == info["off"]
