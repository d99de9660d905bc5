"""CPU: pin the long-double kernel reference (tests/kernel_ref_ld.py) to the golden vectors recorded from the reference and to the
oracle, entry by entry, and show where the reference's own fp64 formula misses the rounding bar."""
import numpy as np
import pytest

from conftest import golden, g11_trees, g14_trees, g15_trees, G11_1D
from oracle import gp_oracle as O
import kernel_ref_ld as R

KINDS = {"rbf": (O.RBF, 0), "rbfard": (O.RBFARD, 0), "matern1": (O.MATERN, 1), "matern3": (O.MATERN, 3),
         "matern5": (O.MATERN, 5), "matern7": (O.MATERN, 7), "rbfunit": (O.RBFUNIT, 0), "rq": (O.RQ, 0),
         "pp0": (O.PIECEPOLY, 0), "pp1": (O.PIECEPOLY, 1), "pp2": (O.PIECEPOLY, 2), "pp3": (O.PIECEPOLY, 3)}
MODES = (("train", "train"), ("cross", "cross"), ("self", "self_test"))


def _kw(mode, x, z):
    return dict(x=x) if mode == "train" else (dict(x=x, z=z) if mode == "cross" else dict(z=z))


def _pin(g, key, kind, para, hyp, x, z):
    """Every entry of the golden matrices within max(rtol |ref|, bar) of the long-double reference -- rtol 1e-13 for K, 1e-12 for
    the derivatives, as the oracle is held to them (tests/test_oracle_golden.py) -- or, in the regions of
    R.formula_loses_digits, within 4x the oracle's own error."""
    D = x.shape[1]
    for mode, m in MODES:
        kw = _kw(m, x, z)
        for der in [None] + list(range(len(hyp))):
            ref, bar = R.ref_matrix(kind, hyp, para, mode=m, der=der, compat=True, **kw)
            gk = key + ("_K_%s" % mode if der is None else "_dK%d_%s" % (der, mode))
            gv = g[gk]
            assert gv.shape == ref.shape, gk
            orc = (O.cov_matrix(kind, hyp, para, mode=m, **kw) if der is None else
                   O.der_matrix(kind, hyp, para, mode=m, der=der, matern_reference_compat=True, **kw))
            lim = np.maximum((1e-13 if der is None else 1e-12) * np.abs(ref.astype(np.float64)), R.limit(kind, hyp, der, D, bar, orc, ref))
            err = np.abs(gv.astype(R.LD) - ref).astype(np.float64)
            assert np.all(err <= lim), (gk, float(np.max(err / lim)))


@pytest.mark.parametrize("fix", ["G4_kernels_seed0", "G5_kernels_unit_test_setup", "G10_kernels_rbfunit_rq_piecepoly"])
def test_golden_primitive_kernels_entry_by_entry(fix):
    g = golden(fix)
    names = [nm for nm in KINDS if nm + "_hyp" in g.files]
    assert names
    for nm in names:
        kind, para = KINDS[nm]
        _pin(g, nm, kind, para, g[nm + "_hyp"], g["x"], g["z"])


def test_golden_G11_kernels_and_trees_entry_by_entry():
    g = golden("G11_kernels_rqard_gabor_periodic_noise_const_composites")
    trees = g11_trees()
    for nm in ("rqard", "gabor", "noise", "const", "periodic", "sum", "prod", "scale", "tree", "ardsum", "maunaloa"):
        x, z = (g["x1"], g["z1"]) if nm in G11_1D else (g["x"], g["z"])
        tree = trees[nm]
        kind, para = (tree[1], tree[2]) if tree[0] == "leaf" else (tree, 0)
        _pin(g, nm, kind, para, g[nm + "_hyp"], x, z)


@pytest.mark.parametrize("fix,trees", [("G14", g14_trees), ("G15", g15_trees)])
def test_golden_ard_trees_entry_by_entry(fix, trees):
    tr = trees()
    names = [nm for nm in tr if not nm.startswith("ep_")]
    for nm in names:
        g = golden("%s_fit_%s_N300" % (fix, nm))
        _pin(g, "k", tr[nm], 0, g["cov_hyp"], g["kx"], g["kz"])


def _hyp(kind, D, rng):
    return {O.RBF: [0.3, 0.2], O.RBFUNIT: [0.3], O.RBFARD: list(rng.uniform(-0.5, 1.0, D)) + [0.1], O.MATERN: [0.4, 0.1],
            O.RQ: [0.2, 0.1, 0.5], O.RQARD: list(rng.uniform(-0.5, 1.0, D)) + [0.1, -0.3], O.PIECEPOLY: [1.0, 0.2],
            O.GABOR: [0.5, 0.3], O.PERIODIC: [0.1, 0.4, 0.2], O.NOISE: [0.1], O.CONST: [0.3]}[kind]


FAMILIES = [(O.RBF, 0), (O.RBFUNIT, 0), (O.RBFARD, 0), (O.MATERN, 1), (O.MATERN, 3), (O.MATERN, 5), (O.MATERN, 7), (O.RQ, 0),
            (O.RQARD, 0), (O.PIECEPOLY, 0), (O.PIECEPOLY, 1), (O.PIECEPOLY, 2), (O.PIECEPOLY, 3), (O.GABOR, 0), (O.PERIODIC, 0),
            (O.NOISE, 0), (O.CONST, 0)]


@pytest.mark.parametrize("kind,para", FAMILIES)
def test_oracle_meets_the_bar_at_random_shapes(kind, para):
    """The oracle's fp64 matrices lie within the bar of the long-double reference, every entry, both derivative conventions,
    every mode -- except in the regions listed by R.formula_loses_digits (shown below)."""
    rng = np.random.RandomState(100 + kind * 10 + para)
    for D in ((1,) if kind == O.PERIODIC else (1, 3, 17, 65)):
        n, m = rng.randint(1, 40), rng.randint(1, 30)
        x, z = rng.randn(n, D) * 1.5, rng.randn(m, D) * 1.5
        h = np.array(_hyp(kind, D, rng))
        nder = O.n_cov_hyp(kind, D) + (1 if kind in (O.MATERN, O.PIECEPOLY) else 0)
        for compat in (False, True):
            for _, mode in MODES:
                kw = _kw(mode, x, z)
                for der in [None] + list(range(nder)):
                    ref, bar = R.ref_matrix(kind, h, para, mode=mode, der=der, compat=compat, **kw)
                    orc = (O.cov_matrix(kind, h, para, mode=mode, **kw) if der is None else
                           O.der_matrix(kind, h, para, mode=mode, der=der, matern_reference_compat=compat, **kw))
                    assert orc.shape == ref.shape
                    if R.formula_loses_digits(kind, h, der, D):
                        continue
                    assert R.excess(orc, ref, bar) <= 1.0, (kind, para, D, compat, mode, der, R.excess(orc, ref, bar))


@pytest.mark.parametrize("tree", ["g11_tree", "g11_maunaloa", "g14_ard_scaled_prod", "g15_scaled_ard_rq_ard"])
def test_oracle_meets_the_bar_for_trees(tree):
    src, nm = tree.split("_", 1)
    t = {"g11": g11_trees, "g14": g14_trees, "g15": g15_trees}[src]()[nm]
    rng = np.random.RandomState(7)
    D = 1 if nm == "maunaloa" else 5
    x, z = rng.randn(33, D), rng.randn(21, D)
    h = rng.uniform(-0.5, 0.5, O.n_cov_hyp(t, D))
    for _, mode in MODES:
        kw = _kw(mode, x, z)
        for der in [None] + list(range(len(h))):
            ref, bar = R.ref_matrix(t, h, 0, mode=mode, der=der, compat=True, **kw)
            orc = O.cov_matrix(t, h, 0, mode=mode, **kw) if der is None else O.der_matrix(t, h, 0, mode=mode, der=der, **kw)
            lim = R.limit(t, h, der, D, bar, orc, ref)
            assert np.all(np.abs(orc.astype(R.LD) - ref).astype(np.float64) <= lim), (tree, mode, der)


def test_oracle_meets_the_bar_at_the_value_edges():
    """The edges the GPU tests probe: s up to 1500 (underflow tails), a 1e4 offset, PiecePoly at r = 1 +- ulps, Periodic with
    |x - z| / p up to 1e3, Gabor near cos = 0, RQ with alpha from e^-3 to e^8."""
    rng = np.random.RandomState(3)
    cases = []
    x = rng.randn(40, 3) * 15.0                                          # s up to ~1500 at ell = 1
    cases += [(O.RBF, 0, [0.0, 0.2], x), (O.MATERN, 5, [0.0, 0.2], x), (O.RQ, 0, [0.0, 0.1, 2.0], x)]
    cases += [(O.RBFARD, 0, [0.1, -0.2, 0.3, 0.0], 1e4 + rng.randn(30, 3))]
    u = rng.randn(30, 2)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    cases += [(O.PIECEPOLY, v, [0.0, 0.1], np.vstack([np.zeros((1, 2)), u * (1.0 + k * 2.0 ** -52)]))
              for v in range(4) for k in (-3, 0, 3)]
    cases += [(O.PERIODIC, 0, [0.0, 0.0, 0.1], rng.uniform(-1500.0, 1500.0, (30, 1)))]
    ell, lp = 1.0, 0.5                                                  # Gabor: dp = 2 pi r ell / p crosses pi / 2 + k pi
    p = np.exp(2 * lp)
    r = (np.pi / 2 + np.pi * np.arange(4))[:, None] * p / (2 * np.pi * ell) * (1.0 + rng.uniform(-1e-9, 1e-9, (4, 1)))
    cases += [(O.GABOR, 0, [0.0, lp], np.vstack([np.zeros((1, 1)), r]))]
    cases += [(O.RQ, 0, [0.0, 0.1, la], rng.randn(30, 2) * 2.0) for la in (-3.0, 0.0, 2.0, 4.0, 8.0)]
    for kind, para, h, x in cases:
        h = np.array(h)
        D = x.shape[1]
        for der in [None] + list(range(len(h))):
            ref, bar = R.ref_matrix(kind, h, para, x=x, mode="train", der=der)
            orc = (O.cov_matrix(kind, h, para, x=x, mode="train") if der is None else
                   O.der_matrix(kind, h, para, x=x, mode="train", der=der, matern_reference_compat=False))
            if R.formula_loses_digits(kind, h, der, D):
                continue
            assert R.excess(orc, ref, bar) <= 1.0, (kind, para, list(h), der, R.excess(orc, ref, bar))


def test_listed_regions_do_lose_digits():
    """The RQ log-alpha derivative: the oracle misses the bar by orders of magnitude where s << alpha (so the GPU tests hold the
    device to 4x the oracle's excess there), while the long-double reference and a cancellation-free form agree."""
    rng = np.random.RandomState(11)
    x = rng.randn(30, 1) * 0.3
    for kind, h in ((O.RQ, [0.0, 0.1, 2.0]), (O.RQARD, [0.0, 0.1, 2.0])):
        der = 2
        assert R.formula_loses_digits(kind, h, der, 1)
        ref, bar = R.ref_matrix(kind, np.array(h), 0, x=x, mode="train", der=der)
        orc = O.der_matrix(kind, np.array(h), 0, x=x, mode="train", der=der)
        assert R.excess(orc, ref, bar) > 10.0
        s = R._Geom(x, None, "train", R._leaf_scale(kind, h, 0, 1)).s
        al = np.exp(R.LD(h[2]))
        u = s / (2 * al)
        direct = u / (1 + u) - np.log1p(u)                                # long double, still cancelling: eps_ld / u relative
        assert np.all(np.abs(R._rq_bracket(u) - direct) <= 1e-10 * np.abs(direct) + 1e-300)


@pytest.mark.parametrize("log_alpha", [-3.0, 0.0, 1.0, 2.0, 3.0, 4.0, 8.0])
def test_rq_alpha_region_boundary(log_alpha):
    """RQ / RQard value and non-alpha derivatives: 1 + s / (2 alpha) rounds to eps, K then carries alpha eps.  Up to alpha =
    RQ_ALPHA_LOSES (= C / 2) the oracle meets the bar everywhere and the matrices are held to it; from log alpha = 3 on the
    oracle misses it, and only those alphas fall in the listed region."""
    inside = np.exp(log_alpha) > R.RQ_ALPHA_LOSES
    assert inside == (log_alpha >= 3.0)
    worst = 0.0
    for seed in range(3):
        rng = np.random.RandomState(seed)
        for D in (1, 3, 17):
            x, z = rng.randn(60, D), rng.randn(40, D)
            for kind in (O.RQ, O.RQARD):
                h = np.array([0.0, 0.1, log_alpha]) if kind == O.RQ else np.concatenate([rng.uniform(-0.5, 0.5, D), [0.1, log_alpha]])
                ders = [None] + [k for k in range(len(h)) if k != len(h) - 1]
                for der in ders:
                    assert R.formula_loses_digits(kind, h, der, D) == inside
                    for mode, kw in (("train", dict(x=x)), ("cross", dict(x=x, z=z))):
                        ref, bar = R.ref_matrix(kind, h, 0, mode=mode, der=der, **kw)
                        orc = (O.cov_matrix(kind, h, 0, mode=mode, **kw) if der is None else
                               O.der_matrix(kind, h, 0, mode=mode, der=der, matern_reference_compat=False, **kw))
                        worst = max(worst, R.excess(orc, ref, bar))
    if inside:
        assert worst > 1.0
    else:
        assert worst <= 1.0


def test_tree_region_holds_only_matrices_with_the_factor():
    """In a tree only the matrices that hold an RQ factor fall in the region: through a Sum the other child's derivatives stay
    held to the bar, through a Product they do not."""
    D = 3
    L = lambda kd, p=0: ("leaf", kd, p)                                   # noqa: E731
    h_rq = [0.0, 0.1, 5.0]                                                # alpha = e^5: inside
    s_tree = ("sum", L(O.RBF), L(O.RQ))
    p_tree = ("prod", L(O.RBF), L(O.RQ))
    for t in (s_tree, p_tree):
        h = np.array([0.2, 0.1] + h_rq)
        assert R.formula_loses_digits(t, h, None, D)
        assert R.formula_loses_digits(t, h, 2, D) and R.formula_loses_digits(t, h, 4, D)
        assert R.formula_loses_digits(t, h, 0, D) == (t[0] == "prod")
    h = np.array([0.2, 0.1, 0.0, 0.1, 1.0])                               # alpha = e: only the alpha derivative
    assert not R.formula_loses_digits(p_tree, h, None, D) and not R.formula_loses_digits(p_tree, h, 0, D)
    assert R.formula_loses_digits(p_tree, h, 4, D)


def test_bar_is_tight_enough_to_see_a_wrong_entry():
    """A one-ulp-scale perturbation stays inside the bar, a relative 1e-12 one does not: the bar is not a normwise tolerance."""
    rng = np.random.RandomState(2)
    x = rng.randn(25, 3)
    ref, bar = R.ref_matrix(O.MATERN, [0.2, 0.1], 3, x=x, mode="train", der=0)
    f = ref.astype(np.float64)
    assert R.excess(f, ref, bar) <= 1.0
    g = f.copy()
    g[3, 7] *= 1.0 + 1e-12
    g[7, 3] = g[3, 7]
    assert R.excess(g, ref, bar) > 1.0
