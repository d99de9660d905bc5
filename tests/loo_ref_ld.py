"""Long-double reference of leave-one-out inference (csrc/loo.hip; inf.LOO) with a per-quantity tolerance computed from the
reference side only (test infrastructure, CPU only; built on fit_ref_ld).

    reference(B, r, sn2, y=None, barB=None) -> LooRef    B (n, n): the matrix the device factorises (K / sn2 + I); r = y - m
    cached(...)                                          the same, once per distinct set of inputs
    LooRef.ratios(got) -> {field: worst |got - reference| / tol}     got: dict of mu / s2 / lp / nlZ / u / S / alpha / dlik (= tr S)
                                                         / Spad (the padding rows of S: exact zeros, anything else counts as inf)
    LooRef.grad_shim()                                   what fit_ref_ld.dnlz_reference needs to sum S against the dK_h
    device_form64(Binv, alpha, y, sn2, mutant=None)      the device's arithmetic restated in numpy fp64 (and its single slips)

With Kinv = B^-1 / sn2, alpha = Kinv r, c = diag(Kinv), in long double (B^-1 = E E' as fit_ref_ld.ld_fit forms it):

    mu = y - alpha / c     s2 = 1 / c     lp = -1/2 log(2 pi) + 1/2 log c - alpha^2 / (2 c)     nlZ = -sum lp
    w = (1 + alpha^2 / c) / (2 c)         u = Kinv (alpha / c)
    S = sn2 Q_loo = (2 / sn2) B^-1 diag(w) B^-1 - sn2 (u alpha' + alpha u')

Tolerance of a quantity X, entry by entry:   tol = bar + (SOLVE_FACTOR E_cpu + FLOOR 2^-53) scale     (SOLVE_FACTOR 8, FLOOR 4)

  * scale: the sum of the absolute values of the terms X is a sum of
        s2  s2             mu  |y| + |alpha / c|         lp  1/2 log(2 pi) + 1/2 |log c| + alpha^2 / (2 c)       nlZ  sum of lp's
        u   |Kinv| |alpha / c|          alpha  max |alpha| (fit_ref_ld)
        S   (2 / sn2) |B^-1| diag(w) |B^-1| + sn2 (|u| |alpha|' + |alpha| |u|')
  * E_cpu is MEASURED: the largest |X_cpu - X_ld| / scale over two fp64 CPU evaluations of the same formulas from the same B --
    LAPACK inv(B), and fit_ref_ld.blocked_fit64 at panel 128 -- both followed by device_form64.
  * bar: a rounding bar barB on the entries of B, to first order, all products of non-negative matrices in long double:
        bar_Binv = |B^-1| barB |B^-1|     bar_c = diag(bar_Binv) / sn2     bar_alpha = |B^-1| barB |alpha|
        bar_s2 = bar_c / c^2              bar_q = bar_alpha / c + |alpha| bar_c / c^2  (q = alpha / c)       bar_mu = bar_q
        bar_lp = bar_c / (2 c) + |alpha| bar_alpha / c + alpha^2 bar_c / (2 c^2)
        bar_u  = (bar_Binv / sn2) |q| + |Kinv| bar_q
        bar_w  = bar_c / (2 c^2) + |alpha| bar_alpha / c^2 + alpha^2 bar_c / c^3
        bar_S  = (2 / sn2) (bar_Binv W |B^-1| + |B^-1| W bar_Binv + |B^-1| bar_W |B^-1|)
                 + sn2 (bar_u |alpha|' + |u| bar_alpha' + bar_alpha |u|' + |alpha| bar_u')
        bar_nlZ = 1/2 sum |S| o barB      (d nlZ_loo = 1/2 sum Q_loo o dK and dK = sn2 dB)
"""
import numpy as np

import fit_ref_ld as F
from fit_ref_ld import chol_ld, inv_lower_ld, gram_lower_ld, program_b, dnlz_reference  # noqa: F401  (the tests take them from here)

LD = F.LD
EPS, SOLVE_FACTOR, FLOOR = F.EPS, F.SOLVE_FACTOR, F.FLOOR
FIELDS = ("alpha", "mu", "s2", "lp", "nlZ", "u", "S")
MUTANTS = ("w_neighbour_c", "mirror_tile", "u_lower_only", "g_padding", "rank2_sign_tile", "gg_fp32_chunk", "trace_np", "s2_unscaled")
# the field every mutant damages
MUTANT_FIELD = dict(w_neighbour_c="S", mirror_tile="S", u_lower_only="u", g_padding="Spad", rank2_sign_tile="S", gg_fp32_chunk="S",
                    trace_np="dlik", s2_unscaled="s2")
LOG2PI = np.log(2 * LD(np.pi))


def _ld(a):
    return F._ld(a)


def _f64(a):
    return F._f64(a)


def loo_formulas(Binv, alpha, y, sn2, xp_ld=True):
    """The formulas of the module docstring on a given B^-1 and alpha, in the precision of the inputs."""
    T = LD if xp_ld else np.float64
    sn2 = T(sn2)
    c = np.diag(Binv) / sn2
    q = alpha / c
    mu = y - q
    s2 = 1 / c
    lp = -T(0.5) * T(LOG2PI) + T(0.5) * np.log(c) - alpha * q / 2
    w = (1 + alpha * q) / (2 * c)
    u = (Binv @ q) / sn2
    S = (2 / sn2) * ((Binv * w[None, :]) @ Binv) - sn2 * (u[:, None] * alpha[None, :] + alpha[:, None] * u[None, :])
    return dict(c=c, q=q, mu=mu, s2=s2, lp=lp, nlZ=-np.sum(lp), w=w, u=u, S=S, alpha=alpha)


def device_form64(Binv, alpha, y, sn2, mutant=None, pad=128):
    """The device's arithmetic in numpy fp64 from an fp64 B^-1 and alpha: B^-1 padded with an identity to a multiple of `pad`,
    the statistics, u from the lower-triangle storage (each stored entry serving both halves), G = sym(B^-1) diag(g) with
    g = sqrt(2 w / sn2) and 0 on the padding, S = G G' on the lower triangle minus the rank-2 term, and the noise gradient
    sn2 tr(Q_loo) = tr(S) over the n live rows.  mutant: one of MUTANTS, a single slip of that arithmetic."""
    assert mutant is None or mutant in MUTANTS
    Binv, alpha, y = _f64(Binv), _f64(alpha).ravel(), _f64(y).ravel()
    n = Binv.shape[0]
    m = (n + pad - 1) // pad * pad
    Bp = np.eye(m)
    Bp[:n, :n] = Binv
    a = np.zeros(m)
    a[:n] = alpha
    cB = np.diag(Bp)[:n]
    c = cB / sn2
    q = a[:n] / c
    mu = y - q
    s2 = 1.0 / (cB if mutant == "s2_unscaled" else c)
    lp = -0.5 * np.log(2 * np.pi) + 0.5 * np.log(c) - 0.5 * a[:n] * q
    cw = c.copy()
    if mutant == "w_neighbour_c" and n > 1:
        k = n // 2
        cw[k] = c[k - 1]
    w = (1.0 + a[:n] * q) / (2.0 * cw)
    g = np.zeros(m) if mutant != "g_padding" else np.ones(m)
    g[:n] = np.sqrt(2.0 * w / sn2)
    qp = np.zeros(m)
    qp[:n] = q
    low = np.tril(Bp)
    if mutant == "u_lower_only":
        u = (low @ qp) / sn2
    else:
        u = (low @ qp + np.tril(Bp, -1).T @ qp) / sn2
    sym = low + np.tril(Bp, -1).T
    if mutant == "mirror_tile" and n > 64:                                  # the upper tile (0, 1) is never written: stays zero
        sym[0:64, 64:128] = 0.0
    G = sym * g[None, :]
    S = G @ G.T
    if mutant == "gg_fp32_chunk":                                           # the first 16-deep k-chunk of the first tile
        f32 = lambda v: v.astype(np.float32).astype(np.float64)
        t = min(64, m)
        S[:t, :t] += f32(G[:t, :16]) @ f32(G[:t, :16]).T - G[:t, :16] @ G[:t, :16].T
    R = sn2 * (np.outer(u, a) + np.outer(a, u))
    if mutant == "rank2_sign_tile":
        t = min(64, n)
        R[:t, :t] = -R[:t, :t]
    S = S - R
    dlik = float(np.trace(S[:n, :n]))
    if mutant == "trace_np":                 # over np, the padding still holding B^-1's identity (S itself is exactly 0 there)
        dlik += float(m - n)
    return dict(alpha=alpha, mu=mu, s2=s2, lp=lp, nlZ=float(-np.sum(lp)), u=u[:n], S=np.tril(S[:n, :n]) + np.tril(S[:n, :n], -1).T,
                dlik=dlik, Spad=S[n:, :].copy())


def cpu_forms(B, r, y, sn2):
    """The two fp64 CPU evaluations E_cpu is measured on: LAPACK inv(B), and blocked_fit64 at panel 128."""
    B64, r64 = _f64(B), _f64(r).ravel()
    Bi = np.linalg.inv(B64)
    Bi = 0.5 * (Bi + Bi.T)
    blk = F.blocked_fit64(B64, r64, sn2, F.LEAF, F.LEAF)
    return [device_form64(Bi, (Bi @ r64) / sn2, y, sn2), device_form64(blk["Binv"], blk["alpha"], y, sn2)]


class LooRef(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def tol(self, field):
        return self.bar[field] + (SOLVE_FACTOR * self.e_cpu[field] + FLOOR * EPS) * self.scale[field]

    def errors(self, got, field):
        g = np.asarray(got[field], dtype=np.float64).reshape(np.shape(self.val[field]))
        return np.abs(g.astype(LD) - self.val[field]).astype(np.float64) / self.scale[field]

    def ratios(self, got, fields=None):
        """{field: worst |got - reference| / tol}; a value that is not finite counts as infinitely wrong."""
        out = {}
        for f in fields or [f for f in FIELDS + ("dlik", "Spad") if f in got]:
            if f == "Spad":                  # the padding rows of S (g = 0 there): exact zeros, no tolerance
                out[f] = 0.0 if np.all(np.asarray(got[f]) == 0) else np.inf
                continue
            g = np.asarray(got[f], dtype=np.float64).reshape(np.shape(self.val[f]))
            tol = self.tol(f)
            assert np.all(np.asarray(tol) > 0) and np.all(np.isfinite(tol)), f
            err = np.abs(g.astype(LD) - self.val[f]).astype(np.float64)
            out[f] = float(np.max(np.where(np.isfinite(g), err / tol, np.inf)))
        return out

    def grad_shim(self):
        """An object fit_ref_ld.dnlz_reference accepts in the place of a FitRef: S where it expects B^-1, a zero alpha, the
        tolerance of S -- the sums it returns are the LOO gradients [cov ..., lik] given S, with their own bars."""
        ref = self

        class Shim(object):
            Binv, alpha, sn2, n = ref.val["S"], np.zeros(ref.n, dtype=LD), ref.sn2, ref.n

            @staticmethod
            def tol(field):
                assert field == "Binv"
                return ref.tol("S")
        return Shim


def reference(B, r, sn2, y=None, barB=None):
    Bl = _ld(B)
    n = Bl.shape[0]
    r64 = _f64(r).ravel()
    y64 = r64 if y is None else _f64(y).ravel()
    sn2 = float(sn2)
    q = F.ld_fit(Bl, r64, sn2)
    Binv, alpha = q["Binv"], q["alpha"]
    v = loo_formulas(Binv, alpha, _ld(y64), sn2)
    aB, aa = np.abs(Binv), np.abs(alpha)
    c, w, u, qq = v["c"], v["w"], v["u"], v["q"]
    au, aq = np.abs(u), np.abs(qq)
    s_lp = LOG2PI / 2 + np.abs(np.log(c)) / 2 + alpha * alpha / (2 * c)
    scale = dict(alpha=float(np.max(aa)), mu=_f64(np.abs(_ld(y64)) + aq), s2=_f64(v["s2"]), lp=_f64(s_lp), nlZ=float(np.sum(s_lp)),
                 u=_f64((aB @ aq) / LD(sn2)),
                 S=_f64((2 / LD(sn2)) * ((aB * w[None, :]) @ aB) + LD(sn2) * (au[:, None] * aa[None, :] + aa[:, None] * au[None, :])))
    scale["dlik"] = float(np.trace(scale["S"]))
    val = dict(alpha=alpha, mu=v["mu"], s2=v["s2"], lp=v["lp"], nlZ=v["nlZ"], u=u, S=v["S"], dlik=np.trace(v["S"]))
    if barB is None:
        bar = dict.fromkeys(FIELDS + ("dlik",), 0.0)
    else:
        bb = _ld(_f64(barB))
        assert bb.shape == (n, n) and np.all(bb >= 0)
        s = LD(sn2)
        bBi = aB @ bb @ aB
        b_c = np.diag(bBi) / s
        b_a = aB @ (bb @ aa)
        b_q = b_a / c + aa * b_c / c ** 2
        b_lp = b_c / (2 * c) + aa * b_a / c + alpha ** 2 * b_c / (2 * c ** 2)
        b_u = (bBi @ aq) / s + (aB @ b_q) / s
        b_w = b_c / (2 * c ** 2) + aa * b_a / c ** 2 + alpha ** 2 * b_c / c ** 3
        X = (bBi * w[None, :]) @ aB
        b_S = (2 / s) * (X + X.T + (aB * b_w[None, :]) @ aB) + s * (b_u[:, None] * aa[None, :] + au[:, None] * b_a[None, :]
                                                                    + b_a[:, None] * au[None, :] + aa[:, None] * b_u[None, :])
        bar = dict(alpha=_f64(b_a), mu=_f64(b_q), s2=_f64(b_c / c ** 2), lp=_f64(b_lp), nlZ=float(np.sum(np.abs(v["S"]) * bb) / 2),
                   u=_f64(b_u), S=_f64(b_S))
        bar["dlik"] = float(np.trace(bar["S"]))
    ref = LooRef(n=n, sn2=sn2, r=r64, y=y64, B=Bl, val=val, scale=scale, bar=bar, w=w, c=c, Binv=Binv,
                 e_cpu=dict.fromkeys(FIELDS + ("dlik",), 0.0), e_cpu_form={})
    for name, fit in zip(("lapack", "blocked-128"), cpu_forms(_f64(Bl), r64, y64, sn2)):
        ref.e_cpu_form[name] = {f: float(np.max(ref.errors(fit, f))) for f in FIELDS + ("dlik",)}
    ref.e_cpu = {f: max(e[f] for e in ref.e_cpu_form.values()) for f in FIELDS + ("dlik",)}
    return ref


_CACHE = {}


def cached(B, r, sn2, y=None, barB=None):
    key = F._key("loo", (B, r, y, barB), float(sn2))
    if key not in _CACHE:
        _CACHE[key] = reference(B, r, sn2, y, barB)
    return _CACHE[key]


def brute_force(K, y, m, sn2):
    """(mu, s2, lp) by n refits in long double: point i predicted from the other n - 1 (K: the long-double covariance matrix)."""
    K, y, m = _ld(K), _ld(y).ravel(), _ld(m).ravel()
    n = K.shape[0]
    mu, s2, lp = (np.zeros(n, dtype=LD) for _ in range(3))
    for i in range(n):
        o = np.arange(n) != i
        if n == 1:
            f, v = m[i], K[i, i]
        else:
            A = K[np.ix_(o, o)] + LD(sn2) * np.eye(n - 1, dtype=LD)
            L = chol_ld(A)
            z = F.P.forward_ld(L, np.column_stack([(y[o] - m[o]), K[o, i]]))
            f, v = m[i] + z[:, 1] @ z[:, 0], K[i, i] - z[:, 1] @ z[:, 1]
        mu[i], s2[i] = f, v + LD(sn2)
        lp[i] = -LOG2PI / 2 - np.log(s2[i]) / 2 - (y[i] - mu[i]) ** 2 / (2 * s2[i])
    return mu, s2, lp
