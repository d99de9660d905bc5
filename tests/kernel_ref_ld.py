"""Long-double restatement of every device covariance family, with a per-entry error bar (test infrastructure, CPU only).

    ref_matrix(kind, hyp, para, x=None, z=None, mode=..., der=None, compat=False, gram=False) -> (K, bar)

`kind` is an oracle kind (oracle/gp_oracle.py) or a tree ("leaf", KIND, para) | ("sum", a, b) | ("prod", a, b) | ("scale", a)
with the reference's flat hyper order.  x / z are the exact fp64 arrays handed to the device; everything after them -- the
length-scale scaling included -- runs in np.longdouble (x86 80-bit: 64-bit significand).  `compat` selects the reference's
derivative conventions for Matern and RQard (Core/cov.py:1173-1177, 1412-1418), as `reference_compat` does in pygps_amd.cov.

K is the long-double value (der None) or derivative matrix.  bar bounds the forward rounding error of an fp64 evaluation:

    bar = C (EPS |k| + S) + TINY,   S = max over s' in {s - sigma_s, s + sigma_s} of |k(s') - k(s)|   (= EPS |dk/ds| sigma_s/EPS)

sigma_s bounds the rounding of the scaled squared distance s = sum_k (a_k - b_k)^2, a = x * sc, b = z * sc:
EPS (sum_k 2 |a_k - b_k| (|a_k| + |b_k|) + (d + 2) s) -- the input scaling and differences, then the summation.  For the
Gram form (gram=True) it is EPS (d + 2) (|a~|^2 + |b~|^2) with a~, b~ the centred, scaled points.  Taking the change of k over
the interval instead of the derivative keeps the bar honest at the kernels' kinks: the PiecePoly support edge, the Noise
threshold, sqrt at r = 0.  ARD length-scale derivatives also carry |k| sigma_dk2 for the rounding of the coordinate's own
squared difference.  Three evaluations carry roundings that do not flow through s and get a term of their own: the
trigonometric argument of Gabor / Periodic (2 pi ell / p, pi / p) and RQ's exponent -alpha log(Kp), both changed by a relative
ARG_REL, and PiecePoly's length-scale bracket (j + v) f - (1 - r) f', EPS (v + 3) times the sum of its two terms.  Trees
combine the bars of their leaves to first order.  TINY covers entries below the smallest normal.
"""
import numpy as np
import pytest

from oracle import gp_oracle as O

LD = np.longdouble
if np.finfo(LD).nmant < 63:                                        # x86 80-bit: 63 stored fraction bits
    pytest.skip("np.longdouble has %d fraction bits here (need >= 63, x86 80-bit extended): no long-double reference"
                % np.finfo(LD).nmant, allow_module_level=True)

EPS = 2.0 ** -53                  # unit roundoff of fp64
C = 16.0                          # fixed safety factor of the bar
TINY = C * 2.0 ** -1022           # absolute slack below the smallest normal (gradual underflow of exp)
NOISE_THRESHOLD = LD(1e-9)        # Core/cov.py:1280: |x - z|^2 < 1e-9 on 'cross'
CONST_JITTER = LD(1e-10)          # Core/cov.py:957: the training diagonal
ARG_REL = 4 * EPS                 # relative rounding of Gabor's / Periodic's trigonometric argument and of RQ's exponent

ARD = (O.RBFARD, O.RQARD)


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


class _Geom(object):
    """Scaled squared distances of x against z (or x itself), their error bounds and the per-coordinate terms."""

    def __init__(self, x, z, mode, sc, gram=False):
        self.mode = mode
        if mode == "self_test":
            m = z.shape[0]
            self.s = np.zeros((m, 1), dtype=LD)
            self.sig = np.zeros((m, 1))
            self.same = np.zeros((m, 1), dtype=bool)
            self.shape = (m, 1)
            return
        zz = x if mode == "train" else z
        self.x, self.z, self.sc = x, zz, _ld(sc)
        n, m, d = x.shape[0], zz.shape[0], x.shape[1]
        self.shape = (n, m)
        s = np.zeros((n, m), dtype=LD)
        sig = np.zeros((n, m), dtype=LD)
        for k in range(d):
            a = _ld(x[:, k]) * self.sc[k]
            b = _ld(zz[:, k]) * self.sc[k]
            df = a[:, None] - b[None, :]
            s += df * df
            sig += 2.0 * np.abs(df) * (np.abs(a)[:, None] + np.abs(b)[None, :])
        self.s = s
        if gram:                                              # |a~|^2 + |b~|^2 of the centred, scaled points
            a = _ld(x) * self.sc[None, :]
            mu = a.mean(axis=0)
            na = ((a - mu) ** 2).sum(axis=1)
            nb = ((_ld(zz) * self.sc[None, :] - mu) ** 2).sum(axis=1)
            self.sig = (EPS * (d + 2) * (na[:, None] + nb[None, :] + s)).astype(np.float64)
        else:
            self.sig = (EPS * (sig + (d + 2) * s)).astype(np.float64)
        self.same = np.eye(n, dtype=bool) if mode == "train" else np.zeros((n, m), dtype=bool)

    def coord(self, k, factor=LD(1)):
        """(dk2, sigma): scaled squared difference in coordinate k (times factor^2) and its rounding bound."""
        if self.mode == "self_test":
            return np.zeros(self.shape, dtype=LD), np.zeros(self.shape)
        f = self.sc[k] * factor
        a = _ld(self.x[:, k]) * f
        b = _ld(self.z[:, k]) * f
        df = a[:, None] - b[None, :]
        dk2 = df * df
        sig = EPS * (2.0 * np.abs(df) * (np.abs(a)[:, None] + np.abs(b)[None, :]) + 3.0 * dk2)
        return dk2, sig.astype(np.float64)


_GEOM_CACHE = []          # the last few geometries: a gradient reference asks for every derivative of one x in turn


def _geom(x, z, mode, sc, gram):
    key = (mode, gram, sc.astype(LD).tobytes(), x if x is None else (x.shape, x.tobytes()),
           z if z is None or mode == "train" else (z.shape, z.tobytes()))
    for k, g in _GEOM_CACHE:
        if k == key:
            return g
    g = _Geom(x, z, mode, sc, gram)
    _GEOM_CACHE.insert(0, (key, g))
    del _GEOM_CACHE[4:]
    return g


def _arg_sens(fu, v):
    """max |f(u = 1 +- ARG_REL) - f(1)|: a relative rounding of the trigonometric argument / the RQ exponent."""
    return np.maximum(*[np.abs(fu(LD(1) + q * ARG_REL) - v) for q in (1, -1)]).astype(np.float64)


def _sens(f, s, sig):
    """max |f(s +- sig) - f(s)| (s - sig clamped at 0), long double."""
    f0 = f(s)
    up = f(s + _ld(sig))
    dn = f(np.maximum(s - _ld(sig), LD(0)))
    return np.maximum(np.abs(up - f0), np.abs(dn - f0)).astype(np.float64)


def _bar(val, sens, extra=0.0):
    return C * (EPS * np.abs(val).astype(np.float64) + sens + extra) + TINY


def _kp_pow(u, e):
    """(1 + u)^e without rounding 1 + u (e up to e^8: the rounding would cost e ulps of long double)."""
    return np.exp(e * np.log1p(u))


def _rq_bracket(u):
    """u / (1 + u) - log(1 + u) = (0.5 s / Kp - alpha log Kp) / alpha of the RQ log-alpha derivative, without its cancellation:
    the series -u^2/2 + 2 u^3/3 - 3 u^4/4 ... below u = 1/8."""
    u = np.asarray(u, dtype=LD)
    ser = np.zeros_like(u)
    p = u * u
    for k in range(1, 64):
        ser += (-1) ** k * (LD(k) / (k + 1)) * p
        p = p * np.minimum(u, LD(0.125))
    return np.where(u < 0.125, ser, u / (1 + u) - np.log1p(u))


def _matern_d(para):
    return O._matern_d(para)


def _mpoly(d, t):
    return {1: lambda: LD(1) + 0 * t, 3: lambda: 1 + t, 5: lambda: 1 + t + t * t / 3,
            7: lambda: 1 + t + 2 * t * t / 5 + t * t * t / 15}[d]()


def _mdpoly(d, t, exact):
    if d == 7:
        return (3 * t + 3 * t * t + t * t * t) / 15 if exact else (t + 3 * t * t + t * t * t) / 15
    return {1: lambda: LD(1) + 0 * t, 3: lambda: t, 5: lambda: (t + t * t) / 3}[d]()


def _pp_func(v, r, j):
    if v == 0:
        return LD(1) + 0 * r
    if v == 1:
        return 1 + (j + 1) * r
    if v == 2:
        return 1 + (j + 2) * r + (j * j + 4 * j + 3) / LD(3) * r * r
    return 1 + (j + 3) * r + (6 * j * j + 36 * j + 45) / LD(15) * r * r + (j ** 3 + 9 * j * j + 23 * j + 15) / LD(15) * r ** 3


def _pp_dfunc(v, r, j):
    if v == 0:
        return 0 * r
    if v == 1:
        return (j + 1) + 0 * r
    if v == 2:
        return (j + 2) + 2 * (j * j + 4 * j + 3) / LD(3) * r
    return (j + 3) + 2 * (6 * j * j + 36 * j + 45) / LD(15) * r + (j ** 3 + 9 * j * j + 23 * j + 15) / LD(5) * r * r


def _pp_bracket_terms(h, para, D, s):
    """EPS sf2 (1 - r)^(e - 1) r ((j + v) f + (1 - r) f'): the forward bound of the PiecePoly length-scale derivative's bracket,
    whose two positive terms cancel at small r and large j (Core/cov.py:774)."""
    v = O._pp_v(para)
    j = LD(np.floor(0.5 * D) + v + 1)
    e = int(j) + v
    r = np.sqrt(s)
    pm = np.maximum(1 - r, LD(0))
    t = np.exp(2 * h[1]) * pm ** (e - 1) * r * (e * _pp_func(v, r, j) + pm * _pp_dfunc(v, r, j))
    return (EPS * (v + 3) * np.abs(t)).astype(np.float64)


def _leaf_scale(kind, hyp, para, D):
    """Per-coordinate scale sc_k of the device's scaled coordinates (Core/cov.py's a = x / ell, sqrt(d) x / ell, ...)."""
    h = _ld(hyp)
    if kind in (O.PERIODIC, O.NOISE, O.CONST):
        return np.ones(D, dtype=LD)
    if kind in ARD:
        return 1 / np.exp(h[:D])
    if kind == O.MATERN:
        return np.full(D, np.sqrt(LD(_matern_d(para))) / np.exp(h[0]), dtype=LD)
    return np.full(D, 1 / np.exp(h[0]), dtype=LD)


def _leaf(kind, hyp, para, x, z, mode, der, compat, gram=False):
    ref = x if x is not None else z
    D = ref.shape[1]
    h = _ld(hyp)
    g = _geom(x, z, mode, _leaf_scale(kind, hyp, para, D), gram)
    s, sig, same = g.s, g.sig, g.same
    train = mode == "train"
    if kind == O.CONST:                                                   # cov.py:949-982
        sf2 = np.exp(h[0])
        if der is None:
            v = sf2 + np.where(same, CONST_JITTER, LD(0)) + 0 * s
        elif der == 0:
            v = 2 * sf2 + 0 * s
        else:
            raise Exception("Wrong derivative entry in covConst")
        return v, _bar(v, 0.0)
    if kind == O.NOISE:                                                   # cov.py:1265-1300
        s2 = np.exp(2 * h[0])
        if der not in (None, 0):
            raise Exception("Wrong derivative index in covNoise")
        c = s2 if der is None else 2 * s2
        if mode == "self_test":
            v = 0 * s
            return v, _bar(v, 0.0)
        if train:
            v = np.where(same, c, LD(0))
            return v, _bar(v, 0.0)
        f = lambda ss: np.where(ss < NOISE_THRESHOLD, c, LD(0))
        v = f(s)
        return v, _bar(v, _sens(f, s, sig))
    if kind in ARD:
        sf2 = np.exp(2 * h[D])
        al = np.exp(h[D + 1]) if kind == O.RQARD else None
        if kind == O.RBFARD:
            base = lambda ss, u=LD(1): sf2 * np.exp(-ss / 2)
            fd = lambda ss, u=LD(1): sf2 * np.exp(-ss / 2)
        else:
            base = lambda ss, u=LD(1): sf2 * _kp_pow(ss / (2 * al), -al * u)
            fd = lambda ss, u=LD(1): sf2 * _kp_pow(ss / (2 * al), (-al - 1) * u)
        if der is None:
            v = base(s)
            return v, _bar(v, _sens(base, s, sig), _arg_sens(lambda u: base(s, u), v) if kind == O.RQARD else 0.0)
        if der < D:
            if mode == "self_test" or (kind == O.RQARD and compat and train):
                v = 0 * s
                return v, _bar(v, 0.0)
            fac = np.exp(2 * h[der]) if (kind == O.RQARD and compat) else LD(1)     # cov.py:1418: x * ell_k, not x / ell_k
            dk2, sdk = g.coord(der, fac)
            a = fd(s)
            v = a * dk2
            extra = np.abs(a).astype(np.float64) * sdk
            if kind == O.RQARD:
                extra = extra + _arg_sens(lambda u: fd(s, u) * dk2, v)
            return v, _bar(v, _sens(fd, s, sig) * dk2.astype(np.float64), extra)
        if der == D:
            f = lambda ss, u=LD(1): 2 * base(ss, u)
        elif kind == O.RQARD and der == D + 1:
            f = lambda ss, u=LD(1): base(ss, u) * al * _rq_bracket(ss / (2 * al))
        else:
            raise Exception("Wrong derivative index")
        v = f(s)
        return v, _bar(v, _sens(f, s, sig), _arg_sens(lambda u: f(s, u), v) if kind == O.RQARD else 0.0)
    f = _scalar_map(kind, h, para, D, der, compat)
    v = f(s)
    extra = 0.0
    if kind in (O.GABOR, O.PERIODIC, O.RQ):     # the trigonometric argument / RQ's exponent -alpha log Kp carry roundings of their own
        extra = _arg_sens(lambda u: _scalar_map(kind, h, para, D, der, compat, u)(s), v)
    elif kind == O.PIECEPOLY and der == 0:      # the bracket (j + v) f - (1 - r) f' of two positive terms: its own rounding
        extra = _pp_bracket_terms(h, para, D, s)
    return v, _bar(v, _sens(f, s, sig), extra)


def _scalar_map(kind, h, para, D, der, compat, u=LD(1)):
    """k(s) or dk/dh(s) of the isotropic families as a function of the scaled squared distance s (u: a relative change of the
    trigonometric argument of Gabor / Periodic)."""
    if kind in (O.RBF, O.RBFUNIT):
        sf2 = np.exp(2 * h[1]) if kind == O.RBF else LD(1)
        if der is None:
            return lambda s: sf2 * np.exp(-s / 2)
        if der == 0:
            return lambda s: sf2 * np.exp(-s / 2) * s
        if der == 1 and kind == O.RBF:
            return lambda s: 2 * sf2 * np.exp(-s / 2)
    elif kind == O.MATERN:
        d = _matern_d(para)
        sf2 = np.exp(2 * h[1])
        K = lambda s: sf2 * _mpoly(d, np.sqrt(s)) * np.exp(-np.sqrt(s))
        if der is None:
            return K
        if der == 2:
            return lambda s: 0 * s
        if compat:                                                       # cov.py:1173-1177: dfunc / func applied to K
            if der == 0:
                return lambda s: sf2 * _mdpoly(d, K(s), False) * K(s) * np.exp(-K(s))
            if der == 1:
                return lambda s: 2 * sf2 * _mpoly(d, K(s)) * np.exp(-K(s))
        else:
            if der == 0:
                return lambda s: sf2 * _mdpoly(d, np.sqrt(s), True) * np.sqrt(s) * np.exp(-np.sqrt(s))
            if der == 1:
                return lambda s: 2 * K(s)
    elif kind == O.RQ:
        sf2, al = np.exp(2 * h[1]), np.exp(h[2])
        if der is None:
            return lambda s: sf2 * _kp_pow(s / (2 * al), -al * u)
        if der == 0:
            return lambda s: sf2 * _kp_pow(s / (2 * al), (-al - 1) * u) * s
        if der == 1:
            return lambda s: 2 * sf2 * _kp_pow(s / (2 * al), -al * u)
        if der == 2:
            return lambda s: sf2 * _kp_pow(s / (2 * al), -al * u) * al * _rq_bracket(s / (2 * al))
    elif kind == O.PIECEPOLY:
        v = O._pp_v(para)
        j = LD(np.floor(0.5 * D) + v + 1)
        e = int(j) + v
        sf2 = np.exp(2 * h[1])
        pm = lambda s: np.maximum(1 - np.sqrt(s), LD(0))
        if der is None:
            return lambda s: sf2 * _pp_func(v, np.sqrt(s), j) * pm(s) ** e
        if der == 0:                                                     # pm ** 0 = 1 beyond the support at e = 1 (cov.py:774)
            return lambda s: sf2 * pm(s) ** (e - 1) * np.sqrt(s) * (e * _pp_func(v, np.sqrt(s), j) - pm(s) * _pp_dfunc(v, np.sqrt(s), j))
        if der == 1:
            return lambda s: 2 * sf2 * _pp_func(v, np.sqrt(s), j) * pm(s) ** e
        if der == 2:
            return lambda s: 0 * s
    elif kind == O.GABOR:
        ell, p = np.exp(h[0]), np.exp(2 * h[1])
        dp = lambda s: 2 * LD(np.pi) * np.sqrt(s) * ell / p * u
        K = lambda s: np.exp(-s / 2) * np.cos(dp(s))
        if der is None:
            return K
        if der == 0:
            return lambda s: dp(s) * K(s)
        if der == 1:
            return lambda s: np.tan(dp(s)) * dp(s) * K(s)
    elif kind == O.PERIODIC:
        ell, p, sf2 = np.exp(h[0]), np.exp(h[1]), np.exp(2 * h[2])
        Ap = lambda s: LD(np.pi) * np.sqrt(s) / p * u
        R = lambda s: np.sin(Ap(s)) / ell
        if der is None:
            return lambda s: sf2 * np.exp(-2 * R(s) ** 2)
        if der == 0:
            return lambda s: 4 * sf2 * np.exp(-2 * R(s) ** 2) * R(s) ** 2
        if der == 1:
            return lambda s: 4 * sf2 / ell * np.exp(-2 * R(s) ** 2) * R(s) * np.cos(Ap(s)) * Ap(s)
        if der == 2:
            return lambda s: 2 * sf2 * np.exp(-2 * R(s) ** 2)
    raise Exception("Wrong derivative index %r for kind %r" % (der, kind))


# ---- trees ---------------------------------------------------------------------------------------------------------
def _nhyp(tree, D):
    return O.n_cov_hyp(tree[1] if tree[0] == "leaf" else tree, D)


def _tree(tree, hyp, x, z, mode, der, compat, gram):
    D = (x if x is not None else z).shape[1]
    if tree[0] == "leaf":
        return _leaf(tree[1], hyp, tree[2], x, z, mode, der, compat, gram)
    if tree[0] == "scale":                                               # cov.py:313-328
        c = np.exp(_ld(hyp[0]))
        if der == 0:
            v, b = _tree(tree[1], hyp[1:], x, z, mode, None, compat, gram)
            c = 2 * c
        else:
            v, b = _tree(tree[1], hyp[1:], x, z, mode, None if der is None else der - 1, compat, gram)
        out = c * v
        return out, float(c) * b + C * EPS * np.abs(out).astype(np.float64) + TINY
    n1 = _nhyp(tree[1], D)
    h1, h2 = hyp[:n1], hyp[n1:]
    if tree[0] == "sum":                                                 # cov.py:283-293
        if der is None:
            (a, ba), (b, bb) = _tree(tree[1], h1, x, z, mode, None, compat, gram), _tree(tree[2], h2, x, z, mode, None, compat, gram)
            out = a + b
            return out, ba + bb + C * EPS * np.abs(out).astype(np.float64) + TINY
        if der < n1:
            return _tree(tree[1], h1, x, z, mode, der, compat, gram)
        return _tree(tree[2], h2, x, z, mode, der - n1, compat, gram)
    # product, cov.py:246-258
    if der is None:
        (a, ba), (b, bb) = _tree(tree[1], h1, x, z, mode, None, compat, gram), _tree(tree[2], h2, x, z, mode, None, compat, gram)
    elif der < n1:
        (a, ba), (b, bb) = _tree(tree[1], h1, x, z, mode, der, compat, gram), _tree(tree[2], h2, x, z, mode, None, compat, gram)
    else:
        (a, ba), (b, bb) = _tree(tree[2], h2, x, z, mode, der - n1, compat, gram), _tree(tree[1], h1, x, z, mode, None, compat, gram)
    out = a * b
    return out, (np.abs(a).astype(np.float64) * bb + np.abs(b).astype(np.float64) * ba + C * EPS * np.abs(out).astype(np.float64)
                 + TINY)


def ref_matrix(kind, hyp, para=0, x=None, z=None, mode=None, der=None, compat=False, gram=False):
    """(K, bar): long-double value / derivative matrix of `kind` and the error bar of an fp64 evaluation (module docstring).
    Shapes as getCovMatrix: 'train' (n, n), 'cross' (n, m), 'self_test' (m, 1)."""
    x = None if x is None else np.asarray(x, dtype=np.float64)
    z = None if z is None else np.asarray(z, dtype=np.float64)
    hyp = np.asarray(hyp, dtype=np.float64)
    if isinstance(kind, tuple):
        return _tree(kind, hyp, x, z, mode, der, compat, gram)
    return _leaf(kind, hyp, para, x, z, mode, der, compat, gram)


def excess(dev, ref, bar):
    """max |dev - ref| / bar over the entries (the unit the tests assert <= 1 in); dev must be finite where ref is."""
    dev = np.asarray(dev, dtype=np.float64)
    err = np.abs(dev.astype(LD) - ref).astype(np.float64)
    err = np.where(np.isnan(dev) & ~np.isnan(ref.astype(np.float64)), np.inf, err)
    assert np.all(bar > 0) and np.all(np.isfinite(ref.astype(np.float64)))
    return float(np.max(err / bar)) if err.size else 0.0


def oracle_error(dev, ref):
    """max |dev - ref| over the entries (long double difference)."""
    return float(np.max(np.abs(np.asarray(dev, dtype=np.float64).astype(LD) - ref))) if np.size(dev) else 0.0


# ---- the gradient pass --------------------------------------------------------------------------------------------
def ard_slots(kind, D, h0=0):
    """Flat index of the first hyper of every ARD leaf (its D length scales, then its magnitude at + D)."""
    if not isinstance(kind, tuple):
        return [h0] if kind in ARD else []
    if kind[0] == "leaf":
        return ard_slots(kind[1], D, h0)
    if kind[0] == "scale":
        return ard_slots(kind[1], D, h0 + 1)
    return ard_slots(kind[1], D, h0) + ard_slots(kind[2], D, h0 + _nhyp(kind[1], D))


def hadamard_ref(kind, hyp, para, x, Binv, alpha, wv=None, sn2=1.0, compat=False, gram=False, centred=False, return_dks=False):
    """Reference of the fits' gradient pass: for every hyper h, sum_ij Q_ij dK_h,ij with Q = Binv o (w w') - alpha alpha'
    (w = wv; without wv 1/sn2 on the rows, 1 on the columns as in the exact fit), in long double, then sn2 tr(Q).  Per
    component the bar C EPS L sum_ij (|Binv w w'| + |alpha alpha'|)_ij |dK_h,ij| + sum_ij |Q_ij| bar(dK_h)_ij, L = 2 + log2(n^2)
    for the depth of the device's reduction tree.  gram: K weights the sums in the Gram form (dK bars with the centred norms);
    centred: the per-coordinate ARD sums run in the product form on centred coordinates (grad.hip ard_dim_reduce), adding
    C EPS L sum_ij |Q_ij| |w_ij| 2 (x~_ik^2 + x~_jk^2) with |w| <= |dK / d log sf| / 2 of the leaf.
    return_dks: also the dict {h: dK_h} of the long-double derivative matrices the sums were taken against."""
    n, D = x.shape
    nh = O.n_cov_hyp(kind, D)
    B = _ld(Binv)
    a = _ld(alpha).reshape(-1)
    if wv is None:
        W = np.full((n, n), 1 / LD(sn2), dtype=LD)
    else:
        w = _ld(wv).reshape(-1)
        W = w[:, None] * w[None, :]
    aa = a[:, None] * a[None, :]
    Q = B * W - aa
    aQ = np.abs(Q).astype(np.float64)
    rQ = (np.abs(B * W) + np.abs(aa)).astype(np.float64)
    L = 2.0 + np.log2(float(n) * n)
    sums, bars = np.zeros(nh + 1, dtype=LD), np.zeros(nh + 1)
    dks = {}
    for hh in range(nh):
        dK, bK = ref_matrix(kind, hyp, para, x=x, mode="train", der=hh, compat=compat, gram=gram)
        dks[hh] = dK
        sums[hh] = np.sum(Q * dK)
        bars[hh] = C * EPS * L * float(np.sum(rQ * np.abs(dK).astype(np.float64))) + float(np.sum(aQ * bK)) + TINY
    if centred:
        for h0 in ard_slots(kind, D):
            sc = 1 / np.exp(_ld(hyp[h0:h0 + D]))
            xs = _ld(x) * sc[None, :]
            xt2 = ((xs - xs.mean(axis=0)) ** 2).astype(np.float64)
            wgt = aQ * np.abs(dks[h0 + D]).astype(np.float64) / 2
            for k in range(D):
                bars[h0 + k] += C * EPS * L * 2 * float(np.sum(wgt * (xt2[:, k][:, None] + xt2[:, k][None, :])))
    sums[nh] = LD(sn2) * np.trace(Q)
    bars[nh] = C * EPS * L * float(sn2) * float(np.sum(np.diag(rQ))) + TINY
    if return_dks:
        return sums, bars, dks
    return sums, bars


# ---- where the reference's own fp64 formula misses the bar ----------------------------------------------------------
RQ_ALPHA_LOSES = C / 2           # RQ / RQard: beyond this alpha the rounding of 1 + s / (2 alpha) takes more than half the bar


def formula_loses_digits(kind, hyp, der, D):
    """True for the matrices whose REFERENCE formula (Core/cov.py) itself loses digits, so that no fp64 evaluation of it meets
    the bar; tests bound the device by 4x the oracle's worst excess there instead (tests/test_kernel_ref_ld.py shows each region
    and its boundary):
      * RQ / RQard, derivative w.r.t. log alpha: K (0.5 s / Kp - alpha log Kp) with Kp = 1 + s / (2 alpha) -- the two terms
        agree to first order in s / alpha and cancel to -s^2 / (8 alpha) (Core/cov.py:1345, 1425);
      * RQ / RQard at alpha > RQ_ALPHA_LOSES, value and every derivative: Kp^-alpha = exp(-alpha log(1 + s / (2 alpha))) --
        1 + s / (2 alpha) rounds to eps, which alpha turns into alpha eps relative in K, against a bar of C eps (Core/cov.py:1323,
        1394).
    Trees: only the matrices that hold such a leaf's factor -- a value holds every leaf, a derivative the leaf it is taken in
    and, through a Product, the values of the other factor (Core/cov.py:246-328)."""
    hyp = np.asarray(hyp, dtype=np.float64)
    if isinstance(kind, tuple):
        if kind[0] == "leaf":
            return formula_loses_digits(kind[1], hyp, der, D)
        if kind[0] == "scale":
            return formula_loses_digits(kind[1], hyp[1:], None if der in (None, 0) else der - 1, D)
        n1 = _nhyp(kind[1], D)
        a = lambda d: formula_loses_digits(kind[1], hyp[:n1], d, D)            # noqa: E731
        b = lambda d: formula_loses_digits(kind[2], hyp[n1:], d, D)            # noqa: E731
        if der is None:
            return a(None) or b(None)
        if kind[0] == "sum":
            return a(der) if der < n1 else b(der - n1)
        return (a(der) or b(None)) if der < n1 else (b(der - n1) or a(None))
    if kind == O.RQ:
        return der == 2 or np.exp(hyp[2]) > RQ_ALPHA_LOSES
    if kind == O.RQARD:
        return der == D + 1 or np.exp(hyp[D + 1]) > RQ_ALPHA_LOSES
    return False


def limit(kind, hyp, der, D, bar, oracle, ref):
    """Per-entry limit of |dev - ref|: the bar; where formula_loses_digits(), the bar scaled by 4x the oracle's worst excess over
    it on that matrix (max |oracle - ref| / bar) -- so each entry keeps its own scale."""
    if formula_loses_digits(kind, hyp, der, D):
        return bar * max(1.0, 4.0 * excess(oracle, ref, bar))
    return bar
