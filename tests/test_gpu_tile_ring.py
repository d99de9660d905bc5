"""GPU: the four-slot staging ring of the LDS-DMA GEMM tiles (csrc/gemm_tile.h, RING; GemmArgs::ring, option tile_ring).

The ring changes WHEN a tile's operand pieces and its lazy C chunks are fetched and waited for, never what is multiplied, in which
order, or the k-step at which C is folded in.  So every product here is compared

* ring on against ring off BIT FOR BIT, and
* both against a numpy.longdouble product at the tolerance tests/test_gpu_r6.py uses for the fold kernel (1e-12 of the largest entry),

over the shapes at which a ring can go wrong: fewer stages than the ring is deep, the last K of the pre-loaded-C path and the first
of the lazy-C path ((LZ + 2) BK = 288), loop exits behind each of the four k-step positions, clipped k-ranges that start off the
ring's span, both LDS-DMA tile shapes and all three kernel entry points; and one exact fit per schedule with the option on and off.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import synth_reg

pytestmark = pytest.mark.gpu

TOL = 1e-12          # tests/test_gpu_r6.py, test_gemm_fold_rows_kernel_against_numpy
KMAX = 512
KM_FULL, KM_GE_I, KM_LT_I, KM_LT_J = 0, 1, 3, 4


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def ops():
    """Operands shared by every product of this file (column-major, as the kernel reads them) and their long-double products
    A[:, k0:k1] B[:, k0:k1]' for the k-ranges asked for, each computed once."""
    rng = np.random.RandomState(7)
    A = np.asfortranarray(rng.randn(512, KMAX))
    B = np.asfortranarray(rng.randn(256, KMAX))
    C0 = np.asfortranarray(rng.randn(512, 256))
    for a in (A, B, C0):
        a.setflags(write=False)
    Al, Bl = A.astype(np.longdouble), B.astype(np.longdouble)
    cache = {}

    def prod(r0, r1, c0, c1, k0, k1):
        key = (r0, r1, c0, c1, k0, k1)
        if key not in cache:
            cache[key] = Al[r0:r1, k0:k1] @ Bl[c0:c1, k0:k1].T
        return cache[key]
    return dict(A=A, B=B, C0=C0, prod=prod)


@pytest.fixture()
def ring(lib):
    """set(v): the context's tile_ring option; restored to the default (on) afterwards"""
    from pygps_amd import _lib
    ctx = _lib.ctx()
    yield lambda v: _lib.check(lib.pgp_set_option(ctx, b"tile_ring", v))
    lib.pgp_set_option(ctx, b"tile_ring", 1)


def _gemm(lib, o, M, N, K, tile=128, tri=0, mask_diag=0, kmode=KM_FULL, koff=0, alpha=-1.0, beta=1.0):
    from pygps_amd import _lib
    Cw = np.asfortranarray(o["C0"][:M, :N].copy(order="F"))
    ms = C.c_double()
    rc = lib.pgp_test_gemm(_lib.ctx(), tile, 0, 0, tri, mask_diag, kmode, koff, alpha, beta, _lib.ptr(o["A"]), 512, _lib.ptr(o["B"]), 256,
                           _lib.ptr(Cw), M, M, N, K, 0, C.byref(ms))
    assert rc == 0, _lib.strerror(rc)
    return Cw


def _both(ring, fn):
    """fn() with the ring off and on: {0: ..., 1: ...}"""
    out = {}
    for v in (0, 1):
        ring(v)
        out[v] = fn()
    return out


def _check(out, ref, what):
    ref = np.asarray(ref, dtype=np.longdouble)
    scale = max(1.0, float(np.max(np.abs(ref))))
    for v in (0, 1):
        err = float(np.max(np.abs(out[v].astype(np.longdouble) - ref)))
        print("%s ring %d: max abs err %.3e (scale %.3g)" % (what, v, err, scale))
        assert err <= TOL * scale, (what, v, err)
    assert _same_bits(out[1], out[0]), what


@pytest.mark.parametrize("alpha,beta", [(-1.0, 1.0), (1.0, 1.0), (1.0, 0.0), (-1.0, 0.0)])
@pytest.mark.parametrize("K", [16, 32, 48, 64, 272, 288, 304, 320, 512])
def test_ring_equals_plain_loop_over_K(lib, ops, ring, K, alpha, beta):
    """M = N = 256 (four workgroups).  K = 16 .. 64: one to four stages, fewer slots than the ring holds, and its drain; 272 / 288: the last
    K with C pre-loaded and the first with the lazy-C prologue; 304, 320, 512 with 288: the loop behind the prologue ends after each of
    the four k-step positions.  These launches do not poll the yield table (test_ring_polling_loop_over_K does)."""
    out = _both(ring, lambda: _gemm(lib, ops, 256, 256, K, alpha=alpha, beta=beta))
    ref = beta * ops["C0"][:256, :256].astype(np.longdouble) + alpha * ops["prod"](0, 256, 0, 256, 0, K)
    _check(out, ref, "K=%d alpha=%g beta=%g" % (K, alpha, beta))


@pytest.mark.parametrize("tile,N", [(128, 256), (1264, 128)])
@pytest.mark.parametrize("K", [16, 48, 64, 272, 288, 304, 320, 336, 512])
def test_ring_polling_loop_over_K(lib, ops, ring, monkeypatch, K, tile, N):
    """The same products through the POLLING instantiations (PGP_TEST_GEMM_YIELD: yield role 1 on the device's table, which is clear, so
    no workgroup sleeps): a stage that polls has one more load in flight, and the ring's waits count it (2P + 1 and 2P + 9 at barrier
    A).  K = 288 .. 336 end the polling loop, four k-steps long, behind each of its positions.  Bit for bit the plain loop with and
    without the poll."""
    from pygps_amd import _lib
    tab = np.ones(4096, dtype=np.uint32)       # the table the poll reads exists (the hook refuses to run without it) and is clear
    assert lib.pgp_test_yield_table(_lib.ctx(), tab.ctypes.data_as(C.POINTER(C.c_uint32))) == 0 and not tab.any()
    ring(0)
    plain = _gemm(lib, ops, 256, N, K, tile=tile)
    monkeypatch.setenv("PGP_TEST_GEMM_YIELD", "1")
    out = _both(ring, lambda: _gemm(lib, ops, 256, N, K, tile=tile))
    ref = ops["C0"][:256, :N].astype(np.longdouble) - ops["prod"](0, 256, 0, N, 0, K)
    _check(out, ref, "poll tile=%d K=%d" % (tile, K))
    assert _same_bits(out[1], plain)


@pytest.mark.parametrize("K", [48, 320])
def test_ring_lower_tiles_with_masked_diagonal(lib, ops, ring, K):
    """tri (packed lower tile set) with mask_diag: the diagonal tiles take the masked epilogue, the upper tile is not touched"""
    out = _both(ring, lambda: _gemm(lib, ops, 256, 256, K, tri=2, mask_diag=1))
    C0 = ops["C0"][:256, :256]
    full = C0.astype(np.longdouble) - ops["prod"](0, 256, 0, 256, 0, K)
    low = np.tril(np.ones((256, 256), dtype=bool))
    _check(out, np.where(low, full, C0.astype(np.longdouble)), "tri K=%d" % K)
    assert _same_bits(out[1][~low], np.asfortranarray(C0)[~low])


@pytest.mark.parametrize("kmode,koff", [(KM_GE_I, -16), (KM_GE_I, 16), (KM_LT_J, 176)], ids=["ge_i-16", "ge_i+16", "lt_j+176"])
def test_ring_clipped_k_ranges(lib, ops, ring, kmode, koff):
    """K = 512, M = N = 256.  KM_GE_I: k >= i0 + koff, the ranges start at 0 / 112 and 16 / 144 -- not multiples of the ring's span of 32
    k-rows; KM_LT_J: k < j0 + 128 + koff = 304 / 432 (an odd and an even number of stages)."""
    out = _both(ring, lambda: _gemm(lib, ops, 256, 256, KMAX, kmode=kmode, koff=koff))
    ref = ops["C0"][:256, :256].astype(np.longdouble).copy()
    for i0 in (0, 128):
        for j0 in (0, 128):
            k0, k1 = (max(0, i0 + koff), KMAX) if kmode == KM_GE_I else (0, min(KMAX, j0 + 128 + koff))
            ref[i0:i0 + 128, j0:j0 + 128] -= ops["prod"](i0, i0 + 128, j0, j0 + 128, k0, k1)
    _check(out, ref, "kmode %d koff %d" % (kmode, koff))


def test_ring_first_touch_rows_upper_trapezoidal(lib, ops, ring):
    """zero_from = 256 with zf_upper at M = 512, N = 256, K = 512: rows >= 256 take beta = 0 (NaN in C there is never read) and start
    their k-range at i0 - 256 (NaN in A's rows 384 .. 511, k < 128, is never read): the trick of tests/test_gpu_skip_zeros.py."""
    from pygps_amd import _lib
    M, N, K, zf = 512, 256, 512, 256
    A = np.array(ops["A"], order="F")
    i, k = np.arange(M)[:, None], np.arange(K)[None, :]
    A[(i >= zf) & (k < i - zf)] = 0.0
    Ap = A.copy(order="F")
    Ap[(i >= zf) & (k < 128 * ((i - zf) // 128))] = np.nan
    C0 = np.array(ops["C0"], order="F")
    C0[zf:] = np.nan

    def run(Ause):
        Cw = C0.copy(order="F")
        _lib.check(lib.pgp_test_gemm_zskip(_lib.ctx(), 128, 0, 0, zf, 1, -1.0, 1.0, _lib.ptr(Ause), M, _lib.ptr(ops["B"]), 256, None,
                                           _lib.ptr(Cw), M, M, N, K))
        return Cw
    out = _both(ring, lambda: run(Ap))
    ring(0)
    clean = run(A)
    ref = -(A.astype(np.longdouble) @ ops["B"].astype(np.longdouble).T)
    ref[:zf] += ops["C0"][:zf].astype(np.longdouble)
    _check(out, ref, "zero_from")
    assert _same_bits(out[1], clean)


@pytest.mark.parametrize("K", [32, 288, 304, 512])
def test_ring_128x64_tile(lib, ops, ring, K):
    """tile 1264 at M = 256, N = 128 (four workgroups of 128 x 64): three pieces per wave and slot, the lazy C chunks of a wave in one
    half of the prologue only; and bit for bit what the 128 x 128 tile gives"""
    out = _both(ring, lambda: _gemm(lib, ops, 256, 128, K, tile=1264))
    ref = ops["C0"][:256, :128].astype(np.longdouble) - ops["prod"](0, 256, 0, 128, 0, K)
    _check(out, ref, "1264 K=%d" % K)
    ring(1)
    assert _same_bits(_gemm(lib, ops, 256, 128, K, tile=128), out[1])


@pytest.mark.parametrize("Ka,Kb", [(320, 48), (288, 512)])
def test_ring_pair_kernel_two_depths(lib, ops, ring, Ka, Kb):
    """gemm_f64_pair_kernel: two products of different depth in one launch"""
    from pygps_amd import _lib

    def run():
        Ca = np.array(ops["C0"][:256, :256], order="F")
        Cb = np.array(ops["C0"][256:, :256], order="F")
        _lib.check(lib.pgp_test_gemm_pair(_lib.ctx(), -1.0, 1.0, _lib.ptr(ops["A"]), 512, _lib.ptr(ops["B"]), 256, _lib.ptr(Ca), _lib.ptr(Cb),
                                          256, 256, 256, Ka, Kb))
        return np.concatenate([Ca, Cb])
    out = _both(ring, run)
    ref = np.concatenate([ops["C0"][:256].astype(np.longdouble) - ops["prod"](0, 256, 0, 256, 0, Ka),
                          ops["C0"][256:].astype(np.longdouble) - ops["prod"](0, 256, 0, 256, 0, Kb)])
    _check(out, ref, "pair %d %d" % (Ka, Kb))


def test_ring_fold_kernel_odd_tile_rows(lib, ops, ring, monkeypatch):
    """gemm_f64_fold_kernel at M = 384 (three tile rows: one workgroup runs rows 2 and 0 back to back through the same LDS, the other the
    middle row alone), KM_LT_I: k < i0 + 128"""
    monkeypatch.setenv("PGP_TEST_GEMM_FOLD", "1")
    out = _both(ring, lambda: _gemm(lib, ops, 384, 128, 384, kmode=KM_LT_I))
    ref = ops["C0"][:384, :128].astype(np.longdouble).copy()
    for i0 in (0, 128, 256):
        ref[i0:i0 + 128] -= ops["prod"](i0, i0 + 128, 0, 128, 0, i0 + 128)
    _check(out, ref, "fold")
    monkeypatch.delenv("PGP_TEST_GEMM_FOLD")
    ring(0)
    assert _same_bits(_gemm(lib, ops, 384, 128, 384, kmode=KM_LT_I), out[1])


@pytest.mark.parametrize("N", [1536, 4096])
def test_fit_is_bit_identical_with_the_ring(lib, ring, N):
    """pgp_exact_fit, nargout 3, with tile_ring 0 and 1: nlZ, alpha, dnlZ and the factor are the same bits, and no bulk workgroup is left
    marked in the device's yield table."""
    from pygps_amd import _lib
    d = 16
    x, y = synth_reg(N, d, seed=N)
    x = _lib.f64(x); y = _lib.f64(y).ravel()
    hyp = _lib.f64(np.array([np.log(np.sqrt(d)), 0.2])); m = np.full(N, float(y.mean())); dm = np.ones((1, N))
    ctx = _lib.ctx()
    _lib.check(lib.pgp_set_data(ctx, _lib.ptr(x), N, d, _lib.ptr(y)))
    res = {}
    for v in (0, 1):
        ring(v)
        alpha = np.zeros(N); nlZ = np.zeros(1); g = np.zeros(4); fh = C.c_void_p()
        _lib.check(lib.pgp_exact_fit(ctx, 0, _lib.ptr(hyp), 2, 0, 0, float(np.log(0.1)), _lib.ptr(m), _lib.ptr(dm), 1, 3,
                                     _lib.ptr(alpha), _lib.ptr(nlZ), _lib.ptr(g), C.byref(fh)))
        L = np.zeros((N, N))
        _lib.check(lib.pgp_factor_to_host(ctx, fh, _lib.ptr(L)))
        lib.pgp_factor_free(ctx, fh)
        res[v] = (nlZ, alpha, g, np.tril(L))
        tab = np.ones(4096, dtype=np.uint32)
        assert lib.pgp_test_yield_table(ctx, tab.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
        assert not tab.any(), (v, np.flatnonzero(tab))
    assert np.isfinite(res[0][0]).all() and np.isfinite(res[0][1]).all()
    for name, a, b in zip(("nlZ", "alpha", "dnlZ", "L"), res[1], res[0]):
        assert _same_bits(a, b), name
