"""GPU: the covariance tile kernels (csrc/assemble.hip behind pgp_cov) and the fits' gradient pass (csrc/grad.hip through
pgp_test_hadamard) entry by entry against the long-double reference of tests/kernel_ref_ld.py, at the shapes where tile kernels
break: interior and ragged 64 x 64 tiles, mirrored tiles of the symmetric form, odd n / m (the general store path), the slab
loop past 16 coordinates, ARD derivative indices past 16, the Gram-form kernels.  Every entry is held to its own rounding bar
(no normwise tolerance); in the regions where the reference's formula itself loses digits (kernel_ref_ld.formula_loses_digits)
to 4x the oracle's worst error on that matrix."""
import zlib

import numpy as np
import pytest

from conftest import g11_trees, g14_trees, g15_trees
from oracle import gp_oracle as O
import kernel_ref_ld as R

pytestmark = pytest.mark.gpu


def _cov_obj(kind, para, hyp, D, compat):
    from test_gpu_composite import build
    tree = kind if isinstance(kind, tuple) else ("leaf", kind, para)
    return build(tree, hyp, D, compat)


def _device(k, mode, x, z, der):
    kw = dict(x=x) if mode == "train" else (dict(x=x, z=z) if mode == "cross" else dict(z=z))
    return k.getCovMatrix(mode=mode, **kw) if der is None else k.getDerMatrix(mode=mode, der=der, **kw)


def _oracle(kind, hyp, para, mode, x, z, der, compat):
    kw = dict(x=x) if mode == "train" else (dict(x=x, z=z) if mode == "cross" else dict(z=z))
    if der is None:
        return O.cov_matrix(kind, hyp, para, mode=mode, **kw)
    return O.der_matrix(kind, hyp, para, mode=mode, der=der, matern_reference_compat=compat, **kw)


def _check(kind, para, hyp, x, z, mode, der, compat, k, what):
    """|dev - ref| <= limit entry by entry; returns the worst |dev - ref| / limit."""
    D = (x if x is not None else z).shape[1]
    dev = _device(k, mode, x, z, der)
    kw = dict(x=x) if mode == "train" else (dict(x=x, z=z) if mode == "cross" else dict(z=z))
    ref, bar = R.ref_matrix(kind, hyp, para, mode=mode, der=der, compat=compat, **kw)
    assert dev.shape == ref.shape, what
    assert np.all(np.isfinite(dev)), what
    lim = bar
    if R.formula_loses_digits(kind, hyp, der, D):
        lim = R.limit(kind, hyp, der, D, bar, _oracle(kind, hyp, para, mode, x, z, der, compat), ref)
    assert np.all(lim > 0) and np.all(np.isfinite(ref.astype(np.float64))), what
    err = np.abs(dev.astype(R.LD) - ref).astype(np.float64)
    worst = float(np.max(err / lim))
    if not worst <= 1.0:
        i = np.unravel_index(np.argmax(err / lim), err.shape)
        pytest.fail("%s: entry %s dev %r ref %r bar %r (%.3g x the limit)" % (what, i, dev[i], float(ref[i]), lim[i], worst))
    return worst


def _points(n, d, rng, spread=1.0):
    """Points whose scaled squared distances span ~0 ... 1500 at ell ~ 0.5: per-point radii from 0.02 to ~5 (x spread)."""
    r = np.exp(rng.uniform(np.log(0.02), np.log(5.0), (n, 1))) * spread
    return rng.randn(n, d) / np.sqrt(d) * r * 3.0


def _with_duplicates(x, z):
    """Copies of rows in DIFFERENT 64-tiles (train diagonal detection), z rows equal to x rows and at |x - z|^2 = 3e-9 (the
    'cross' Noise threshold 1e-9 sits between them and 1e-8)."""
    x = x.copy()
    n = x.shape[0]
    if n > 64:
        x[n - 1] = x[0]
        x[64] = x[3]
    if z is not None:
        z = z.copy()
        m = z.shape[0]
        z[m - 1] = x[n // 2]
        if m > 1:
            z[0] = x[0]
            z[0, 0] += np.sqrt(3e-9)
    return x, z


# (kind, para, hyp-maker, compat variants); hyp(D, rng)
def _ard_hyp(D, rng, extra):
    return list(rng.uniform(-1.0, 0.5, D)) + extra


FAMILIES = {
    "rbf": (O.RBF, 0, lambda D, r: [-0.7, 0.2], (False,)),
    "rbfunit": (O.RBFUNIT, 0, lambda D, r: [-0.5], (False,)),
    "rbfard": (O.RBFARD, 0, lambda D, r: _ard_hyp(D, r, [0.1]), (False,)),
    "matern1": (O.MATERN, 1, lambda D, r: [-0.4, 0.1], (False, True)),
    "matern3": (O.MATERN, 3, lambda D, r: [-0.4, 0.1], (False, True)),
    "matern5": (O.MATERN, 5, lambda D, r: [-0.4, 0.1], (False, True)),
    "matern7": (O.MATERN, 7, lambda D, r: [-0.4, 0.1], (False, True)),
    "rq": (O.RQ, 0, lambda D, r: [-0.5, 0.1, -0.4], (False,)),
    "rqard": (O.RQARD, 0, lambda D, r: _ard_hyp(D, r, [0.1, 0.6]), (False, True)),
    "pp0": (O.PIECEPOLY, 0, lambda D, r: [0.8, 0.1], (False,)),
    "pp1": (O.PIECEPOLY, 1, lambda D, r: [0.8, 0.1], (False,)),
    "pp2": (O.PIECEPOLY, 2, lambda D, r: [0.8, 0.1], (False,)),
    "pp3": (O.PIECEPOLY, 3, lambda D, r: [0.8, 0.1], (False,)),
    "gabor": (O.GABOR, 0, lambda D, r: [-0.3, 0.2], (False,)),
    "periodic": (O.PERIODIC, 0, lambda D, r: [0.1, -0.6, 0.2], (False,)),
    "noise": (O.NOISE, 0, lambda D, r: [0.1], (False,)),
    "const": (O.CONST, 0, lambda D, r: [-0.3], (False,)),
}
# (n, m, d): every tile edge, both parities, n != m both ways, m = 1; d across the slab edges (16-coordinate slabs)
SHAPES = [(1, 1, 1), (2, 1, 3), (63, 65, 15), (64, 64, 16), (65, 127, 17), (128, 129, 31), (129, 128, 32), (191, 63, 33),
          (333, 2, 48), (127, 191, 64), (65, 63, 65), (64, 1, 100), (1000, 333, 3)]


def _shapes_for(name):
    """A covering subset: every family meets both parities, a mirrored tile, a ragged tile, the slab loop and m = 1; the
    families rotate through the rest of SHAPES so that each shape is met by several of them."""
    if name == "periodic":
        return [(n, m, 1) for n, m, _ in SHAPES[:11]]
    i = sorted(FAMILIES).index(name)
    pick = [0, 2, 4, 7, 10] + [k for k in range(len(SHAPES)) if k % 4 == i % 4 and k not in (0, 2, 4, 7, 10)]
    return [SHAPES[k] for k in sorted(set(pick))]


def _ders(kind, D):
    nh = O.n_cov_hyp(kind, D)
    if kind in (O.RBFARD, O.RQARD):
        return sorted({k for k in (0, 15, 16, 17, D - 1) if k < D} | set(range(D, nh)))
    return list(range(nh + (1 if kind in (O.MATERN, O.PIECEPOLY) else 0)))


WORST = {}


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_pgp_cov_families_entry_by_entry(name):
    kind, para, hmk, compats = FAMILIES[name]
    rng = np.random.RandomState(sorted(FAMILIES).index(name) + 1)
    worst = 0.0
    for n, m, D in _shapes_for(name):
        x, z = _with_duplicates(_points(n, D, rng), _points(m, D, rng))
        if kind == O.PERIODIC:                                            # |x - z| / p up to ~1e3
            x, z = x * 30.0, z * 30.0
        hyp = np.array(hmk(D, rng), dtype=float)
        for compat in compats:
            k = _cov_obj(kind, para, hyp, D, compat)
            for mode in ("train", "cross", "self_test"):
                for der in [None] + _ders(kind, D):
                    w = _check(kind, para, hyp, x, z, mode, der, compat, k, "%s n=%d m=%d d=%d %s der=%s compat=%s"
                               % (name, n, m, D, mode, der, compat))
                    worst = max(worst, w)
    WORST[name] = worst
    print("\nworst |dev - ref| / bar, %s: %.3g" % (name, worst))


@pytest.mark.parametrize("name,kind,para,hyp,scale", [
    ("rbf_offset_1e4", O.RBF, 0, [0.3, 0.1], None),
    ("rbfard_offset_1e4", O.RBFARD, 0, None, None),
    ("matern5_offset_1e4", O.MATERN, 5, [0.2, 0.1], None),
    ("pp_support_edge_v0", O.PIECEPOLY, 0, [0.0, 0.1], "unit"),
    ("pp_support_edge_v2", O.PIECEPOLY, 2, [0.0, 0.1], "unit"),
    ("gabor_cos_zero", O.GABOR, 0, [0.0, 0.5], "gabor"),
    ("rq_alpha_e-3", O.RQ, 0, [0.0, 0.1, -3.0], None),
    ("rq_alpha_e8", O.RQ, 0, [0.0, 0.1, 8.0], None),
    ("rqard_alpha_e8", O.RQARD, 0, None, None),
])
def test_pgp_cov_value_edges(name, kind, para, hyp, scale):
    """A common coordinate offset of 1e4, PiecePoly at r = 1 +- a few ulps (and v = 0, d = 1: the 0**0 length-scale
    derivative beyond the support), Gabor near cos = 0, RQ with alpha from e^-3 to e^8."""
    rng = np.random.RandomState(17)
    if scale == "unit":
        D = 1 if para == 0 else 2
        u = rng.randn(70, D)
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        x = np.vstack([np.zeros((1, D)), u * (1.0 + rng.randint(-4, 5, (70, 1)) * 2.0 ** -52), 0.5 * u[:10], 2.0 * u[:10]])
        z = np.vstack([u[:40] * (1.0 - 2.0 ** -52), np.zeros((1, D))])
    elif scale == "gabor":
        D = 1
        p = np.exp(2 * hyp[1])
        r = ((np.pi / 2 + np.pi * np.arange(6))[:, None] * p / (2 * np.pi) * (1.0 + rng.uniform(-1e-9, 1e-9, (6, 12)))).reshape(-1, 1)
        x = np.vstack([np.zeros((1, 1)), r, rng.randn(30, 1)])
        z = np.vstack([np.zeros((1, 1)), -r[:40]])
    else:
        D = 17 if kind == O.RBFARD or kind == O.RQARD else 3
        x, z = _points(130, D, rng), _points(67, D, rng)
        if "offset" in name:
            x, z = x + 1e4, z + 1e4
    if hyp is None:
        hyp = list(rng.uniform(-0.5, 0.5, D)) + ([0.1] if kind == O.RBFARD else [0.1, 8.0])
    hyp = np.array(hyp, dtype=float)
    k = _cov_obj(kind, para, hyp, D, False)
    worst = 0.0
    for mode in ("train", "cross"):
        for der in [None] + _ders(kind, D):
            worst = max(worst, _check(kind, para, hyp, x, z, mode, der, False, k, "%s %s der=%s" % (name, mode, der)))
    print("\nworst |dev - ref| / bar, %s: %.3g" % (name, worst))


def _eight_leaf_tree():
    L = lambda kd, p=0: ("leaf", kd, p)                                  # noqa: E731
    return ("sum", ("sum", ("prod", ("sum", L(O.RBFARD), L(O.MATERN, 5)), ("sum", L(O.RQ), ("scale", L(O.PIECEPOLY, 2)))),
                    ("sum", L(O.GABOR), L(O.NOISE))), ("sum", L(O.CONST), L(O.RBFUNIT)))


def _programs():
    out = []
    for nm, t in g11_trees().items():
        if nm not in ("maunaloa", "periodic", "rqard", "gabor", "noise", "const"):
            out.append(("g11_" + nm, t))
    out += [("g14_" + nm, t) for nm, t in g14_trees().items()]
    out += [("g15_" + nm, t) for nm, t in g15_trees().items()]
    out.append(("eight_leaves", _eight_leaf_tree()))
    return out


@pytest.mark.parametrize("name,tree", _programs())
def test_programs_entry_by_entry(name, tree):
    """Device programs (Sum / Product / Scale trees, up to two ARD leaves, the 8-leaf limit) at d = 3, 17, 40, 64, every flat
    hyper, all three modes; ragged tiles and duplicates."""
    rng = np.random.RandomState(zlib.crc32(name.encode()) % 100003)
    worst = 0.0
    for (n, m), D in zip([(65, 63), (130, 1), (63, 129), (97, 64)], (3, 17, 40, 64)):
        x, z = _with_duplicates(_points(n, D, rng), _points(m, D, rng))
        hyp = rng.uniform(-0.6, 0.4, O.n_cov_hyp(tree, D))
        k = _cov_obj(tree, 0, hyp, D, False)
        assert k._on_device()
        ders = list(range(len(hyp)))
        if D > 17:                                                        # every non-ARD hyper, ARD indices at the slab edges
            slots = R.ard_slots(tree, D)
            ders = [h for h in ders if not any(h0 <= h < h0 + D and (h - h0) not in (0, 15, 16, 17, D - 1) for h0 in slots)]
        for mode in ("train", "cross", "self_test"):
            for der in [None] + ders:
                worst = max(worst, _check(tree, 0, hyp, x, z, mode, der, False, k, "%s d=%d %s der=%s" % (name, D, mode, der)))
    print("\nworst |dev - ref| / bar, %s: %.3g" % (name, worst))


def _gram_bound(x, sc):
    a = x * sc[None, :]
    dev = np.max(np.abs(a - a.mean(axis=0)), axis=0)
    return float(np.sum(dev * dev))


@pytest.mark.parametrize("n,d", [(4096, 32), (4097, 33), (4133, 40), (4160, 48), (4096, 64), (4097, 65), (4133, 100), (4160, 250)])
def test_gram_assembly_entry_by_entry(n, d):
    """getCovMatrix('train') of RBF / RBFard at n >= 4096, d >= 32: the Gram-form kernels (cov_gram_fast_kernel at dpad 32 / 48 /
    64 with n % 64 == 0, cov_gram_kernel otherwise, the generic one beyond d = 64) when the norm bound allows, the difference form
    when it does not -- both data sets per shape.  Rows every ~97th, every entry of three diagonal tiles and of the last tile row."""
    rng = np.random.RandomState(n + d)
    x0 = 1000.0 + rng.uniform(-1.0, 1.0, (n, d))                          # offset: the Gram kernels only pass if they centre
    nt = (n + 63) // 64
    last = np.arange((nt - 1) * 64, n)
    blocks = [(np.arange(0, n, 97), np.arange(n))]                          # every 97th row, all columns
    blocks += [(np.arange(t * 64, min(n, t * 64 + 64)),) * 2 for t in (0, nt // 2, nt - 1)]     # three diagonal tiles
    blocks += [(last, np.unique(np.concatenate([np.arange(0, n, 7), last])))]                  # the last tile row
    seen = set()
    worst = 0.0
    for kind in (O.RBF, O.RBFARD):
        for ell in (np.sqrt(d / 32.0), 0.5):                               # bound sum_k (max dev_k / ell)^2 ~ 32, then ~ 4 d
            hyp = np.array([np.log(ell), 0.2]) if kind == O.RBF else np.concatenate([np.log(ell) + rng.uniform(-0.1, 0.1, d), [0.2]])
            sc = np.full(d, 1.0 / ell) if kind == O.RBF else 1.0 / np.exp(hyp[:d])
            gram = _gram_bound(x0, sc) <= 64.0
            seen.add(gram)
            k = _cov_obj(kind, 0, hyp, d, False)
            K = k.getCovMatrix(x=x0, mode="train")
            a = x0 * sc[None, :]
            nrm = np.sum((a - a.mean(axis=0)) ** 2, axis=1)
            for rows, cols in blocks:
                dev = K[np.ix_(rows, cols)]
                assert np.all(np.isfinite(dev))
                ref, bar = R.ref_matrix(kind, hyp, 0, x=x0[rows], z=x0[cols], mode="cross")
                if gram:                                                   # the Gram form's distance error: centred norms
                    sig = R.EPS * (d + 2) * (nrm[rows][:, None] + nrm[cols][None, :])
                    bar = bar + R.C * 0.5 * np.abs(ref.astype(np.float64)) * sig
                err = np.abs(dev.astype(R.LD) - ref).astype(np.float64)
                w = float(np.max(err / bar))
                assert w <= 1.0, (kind, ell, gram, w)
                worst = max(worst, w)
            del K
    assert seen == {True, False}
    print("\nworst |dev - ref| / bar, gram n=%d d=%d: %.3g" % (n, d, worst))


# ---- the gradient pass ----------------------------------------------------------------------------------------------
def _hadamard(kind, para, hyp, x, Binv, alpha, wv, sn2, compat=False):
    import ctypes as C
    from pygps_amd import _lib
    lib = _lib.load()
    ctx = _lib.ctx()
    D = x.shape[1]
    k = _cov_obj(kind, para, hyp, D, compat)
    kd, pa, fl = k._bind(ctx)
    _lib.check(lib.pgp_set_data(ctx, _lib.ptr(_lib.f64(x)), x.shape[0], D, None), "pgp_set_data")
    h = _lib.f64(hyp)
    out = np.zeros(len(hyp) + 1)
    B = _lib.f64(Binv)
    a = _lib.f64(alpha.reshape(-1))
    w = None if wv is None else _lib.f64(wv.reshape(-1))
    _lib.check(lib.pgp_test_hadamard(ctx, kd, _lib.ptr(h), len(hyp), pa, fl, _lib.ptr(B), _lib.ptr(a), _lib.ptr(w), C.c_double(sn2),
                                     _lib.ptr(out)), "pgp_test_hadamard")
    return out


def _ard_form(form):
    from pygps_amd import _lib
    _lib.check(_lib.load().pgp_set_option(_lib.ctx(), b"ard_grad_form", form))


def _spd(n, rng):
    A = rng.randn(n, n) / np.sqrt(n)
    return np.eye(n) + 0.3 * (A + A.T) / 2


HAD_CASES = [  # (name, kind, para, n, d, compat, data)
    ("rbf", O.RBF, 0, 2049, 3, False, "spread"), ("rbf", O.RBF, 0, 64, 17, False, "spread"),
    ("rbfunit", O.RBFUNIT, 0, 65, 3, False, "spread"),
    ("matern1", O.MATERN, 1, 63, 3, False, "spread"), ("matern3", O.MATERN, 3, 63, 33, False, "spread"),
    ("matern5", O.MATERN, 5, 65, 17, False, "spread"), ("matern7", O.MATERN, 7, 1000, 3, False, "spread"),
    ("matern1", O.MATERN, 1, 64, 3, True, "spread"), ("matern3", O.MATERN, 3, 65, 3, True, "spread"),
    ("matern5", O.MATERN, 5, 63, 5, True, "spread"), ("matern7", O.MATERN, 7, 64, 17, True, "spread"),
    ("rq", O.RQ, 0, 200, 5, False, "spread"),
    ("pp0", O.PIECEPOLY, 0, 63, 1, False, "spread"), ("pp1", O.PIECEPOLY, 1, 64, 3, False, "spread"),
    ("pp2", O.PIECEPOLY, 2, 65, 3, False, "spread"), ("pp3", O.PIECEPOLY, 3, 65, 17, False, "spread"),
    ("rbfard", O.RBFARD, 0, 1, 3, False, "spread"), ("rbfard", O.RBFARD, 0, 63, 17, False, "spread"),
    ("rbfard", O.RBFARD, 0, 129, 64, False, "spread"), ("rbfard", O.RBFARD, 0, 65, 254, False, "spread"),
    ("rbfard", O.RBFARD, 0, 200, 33, False, "spread"),
    ("rqard", O.RQARD, 0, 64, 16, False, "spread"), ("rqard", O.RQARD, 0, 65, 65, False, "spread"),
    ("rqard", O.RQARD, 0, 64, 16, True, "spread"),
    ("gabor", O.GABOR, 0, 65, 2, False, "spread"), ("periodic", O.PERIODIC, 0, 200, 1, False, "spread"),
    ("noise", O.NOISE, 0, 63, 3, False, "spread"), ("const", O.CONST, 0, 64, 3, False, "spread"),
    # norm bound <= 64 at d >= 17: the fit's Gram-form assembly applies, and the reduce gets its prep (centred norms, means)
    ("rbf", O.RBF, 0, 200, 40, False, "tight"), ("rbfard", O.RBFARD, 0, 130, 40, False, "tight"),
    ("rbfard", O.RBFARD, 0, 65, 64, False, "tight"),
]
_PROG_SIZES = {"g11_tree": (200, 3), "g11_scaled_sum": (65, 17), "g14_ard_scaled_prod": (63, 40), "g14_rqard_sum": (129, 64),
               "g15_ard_plus_rqard": (64, 17), "g15_scaled_ard_rq_ard": (65, 33), "eight_leaves": (200, 5)}
_PROG_CASES = [("prog_" + nm, t, 0) + _PROG_SIZES.get(nm, [(65, 3), (63, 17), (64, 40), (65, 64), (130, 5)][i % 5]) + (False, "spread")
               for i, (nm, t) in enumerate(_programs())]


def _tight_bound(x, hyp, kind, d):
    sc = np.full(d, np.exp(-hyp[0])) if kind == O.RBF else np.exp(-hyp[:d])
    dev2 = np.max((x - x.mean(axis=0)) ** 2, axis=0)
    return float(np.sum(sc * sc * dev2))


@pytest.mark.parametrize("name,kind,para,n,d,compat,data", HAD_CASES + _PROG_CASES)
def test_gradient_pass_component_by_component(name, kind, para, n, d, compat, data):
    """pgp_test_hadamard (the fits' hadamard_reduce_launch on a NaN-padded B^-1) against sum_ij Q_ij dK_h,ij in long double, every
    hyper on its own, the exact weights and the EP / Laplace per-point weights, both ARD forms, both derivative conventions of
    Matern / RQard, every device program; the sums are finite (no NaN of the padding or the unread lower triangle gets in)."""
    rng = np.random.RandomState(n * 7 + d + (1000 if compat else 0))
    if data == "tight":                                                  # offset data: the prep's centring is seen
        x = 10.0 + rng.uniform(-0.5, 0.5, (n, d))
    else:
        x = _points(n, d, rng)
    if n > 64:
        x[n - 1] = x[0]
    hyp = rng.uniform(-0.6, 0.3, O.n_cov_hyp(kind, d))
    if kind == O.RQ:
        hyp[2] = -0.5
    if kind == O.RQARD or (isinstance(kind, tuple) and "rq" in name):
        hyp = np.minimum(hyp, 0.0)
    if data == "tight":
        assert d >= 17 and _tight_bound(x, hyp, kind, d) <= 64.0         # gram_assembly_applies: the Gram prep is handed in
    Binv, alpha = _spd(n, rng), rng.randn(n)
    ard = bool(R.ard_slots(kind, d))
    forms = (1, 2) if ard else (0,)
    worst = 0.0
    try:
        for form in forms:
            _ard_form(form)
            for wv, sn2 in ((None, np.exp(2 * -0.7)), (rng.uniform(0.2, 1.5, n), 1.0)):
                got = _hadamard(kind, para, hyp, x, Binv, alpha, wv, sn2, compat)
                assert np.all(np.isfinite(got)), (name, form, got)
                plain_ard = kind in (O.RBFARD, O.RQARD)
                ref, bar = R.hadamard_ref(kind, hyp, para, x, Binv, alpha, wv=wv, sn2=sn2, compat=compat,
                                          gram=plain_ard and form == 1, centred=form == 1)
                for hh in range(len(got)):
                    lim = bar[hh]
                    if hh < len(hyp) and R.formula_loses_digits(kind, hyp, hh, d):    # 4x the oracle's excess over the bar
                        dK = O.der_matrix(kind, hyp, para, x=x, mode="train", der=hh, matern_reference_compat=compat)
                        Wm = (np.full((n, n), 1.0 / sn2) if wv is None else np.outer(wv, wv))
                        Q = Binv * Wm - np.outer(alpha, alpha)
                        lim = bar[hh] * max(1.0, 4.0 * abs(float(np.sum(Q * dK)) - float(ref[hh])) / bar[hh])
                    e = abs(float(got[hh]) - float(ref[hh])) / lim
                    assert e <= 1.0, (name, form, wv is None, hh, got[hh], float(ref[hh]), lim)
                    worst = max(worst, e)
    finally:
        _ard_form(0)
    print("\nworst |dev - ref| / bar, gradient %s%s n=%d d=%d: %.3g" % (name, " compat" if compat else "", n, d, worst))


def test_hook_reproduces_the_fit_gradient():
    """One small exact fit: the hook on the oracle's B^-1 and alpha gives the fit's dnlZ.cov (= sums / 2) and dnlZ.lik (the
    sn2 tr(Q) slot) -- the hook makes the production call."""
    import pygps_amd as pyGPs
    rng = np.random.RandomState(5)
    n, d = 150, 3
    x = rng.randn(n, d)
    y = np.sin(x.sum(axis=1, keepdims=True)) + 0.1 * rng.randn(n, 1)
    m = pyGPs.GPR()
    m.setPrior(kernel=pyGPs.cov.RBFard(D=d, log_ell_list=[0.1, -0.2, 0.3], log_sigma=0.2))
    m.setNoise(-1.0)
    m.setData(x, y)
    nlZ, dnlZ, post = m.getPosterior()
    hyp = np.array(m.covfunc.hyp)
    sn2 = np.exp(2 * m.likfunc.hyp[0])
    c = m.meanfunc.hyp[0]
    ref = O.exact_fit(O.RBFARD, hyp, 0, m.likfunc.hyp[0], x, y, c * np.ones((n, 1)), np.ones((n, 1)), faithful=False)
    L = ref["L"]                                                            # upper factor of B = K / sn2 + I
    Li = np.linalg.inv(L)
    Binv = Li @ Li.T
    got = _hadamard(O.RBFARD, 0, hyp, x, Binv, ref["alpha"], None, sn2)
    tol = 1e-8 * np.max(np.abs(dnlZ.cov))
    assert np.max(np.abs(0.5 * got[:-1] - np.array(dnlZ.cov))) <= tol
    assert abs(got[-1] - dnlZ.lik[0]) <= 1e-8 * max(1.0, abs(dnlZ.lik[0]))
