"""CPU restatement of FITC_EP.evaluate (Core/inf.py:828-944) with lik.Erf, for the FITC_EP tests.  Not a test module.

Written on (V, d0, M = inv(I + V diag(s) V'), h = M V (t o b)) instead of the reference's (d, P, R, nn, gg), with the same
sites in the same order and the same scalar update, so it agrees with the reference up to rounding.  ``block`` = 128 runs the
sweep in blocks of consecutive sites through the matrix inversion lemma as the device does (for sizes at which the per-site
loop is too slow in numpy); both forms are exact identities of the same iteration.  Covariance inputs are the FITCOfKernel
triple (diagK, Kuu, Ku) and, for gradients, one (ddiagK, dKuu, dKu) triple per hyper-parameter."""
import numpy as np

from oracle.gp_oracle import erf_ep_moments


def _site(sii, mui, w, b, m, y):
    tau_ni = 1.0 / sii - w
    nu_ni = mui / sii + m * tau_ni - b
    _, dlZ, d2lZ = [float(np.ravel(v)[0]) for v in erf_ep_moments(y, nu_ni / tau_ni, 1.0 / tau_ni, 3)]
    w_new = max(-d2lZ / (1.0 + d2lZ / tau_ni), 0.0)
    b_new = (dlZ + (m - nu_ni / tau_ni) * d2lZ) / (1.0 + d2lZ / tau_ni)
    return w_new, b_new


class _State(object):
    def __init__(self, V, d0, w, b):
        nu = V.shape[0]
        self.t = 1.0 / (1.0 + d0 * w)
        s = w * self.t
        A = np.eye(nu) + (V * s) @ V.T
        self.Lu = np.linalg.cholesky(A)
        self.M = np.linalg.inv(A)
        self.h = self.M @ (V @ (self.t * b))


def _nlZ(V, d0, w, b, y, m, st):
    t = st.t
    U = np.linalg.solve(st.Lu, V)                       # U'U = V'MV
    ds = d0 * t + t * t * (U * U).sum(0)
    mu = d0 * t * b + t * (V.T @ st.h)
    tau_n = 1.0 / ds - w
    nu_n = mu / ds - b + m * tau_n
    lZ = erf_ep_moments(y, nu_n / tau_n, 1.0 / tau_n, 1)[0]
    ld = 2.0 * np.log(np.diag(st.Lu)).sum() + np.log1p(d0 * w).sum()
    ub = U @ (t * b)
    tst = (d0 * t * b * b).sum() + ub @ ub
    e = nu_n - m * tau_n
    nlZ = (ld / 2.0 - lZ.sum() - tst / 2.0 - (e * ((w / tau_n * e - 2.0 * b) / (w + tau_n))).sum() / 2.0
           + (b * b / (tau_n + w)).sum() / 2.0 - np.log1p(w / tau_n).sum() / 2.0)
    return nlZ, nu_n, tau_n


def fitc_ep_fit(diagK, Kuu, Ku, y, m, dm=(), ders=(), last_ttau=None, last_tnu=None, block=None):
    """Returns dict(nlZ, sweeps, ttau, tnu, alpha (nu,1), L (nu,nu), sW, dnlZ_mean, dnlZ_cov, warm_kept)."""
    n = Ku.shape[1]
    nu = Kuu.shape[0]
    y = np.asarray(y, float).reshape(n)
    m = np.asarray(m, float).reshape(n)
    diagK = np.asarray(diagK, float).reshape(n)
    snu2 = 1e-6                                          # inf.py:837-841
    Luu = np.linalg.cholesky(Kuu + snu2 * np.eye(nu))
    V = np.linalg.solve(Luu, Ku)
    d0 = diagK - (V * V).sum(0)
    nlZ0 = -erf_ep_moments(y, m, diagK, 1)[0].sum()
    warm_kept = None
    w = np.zeros(n)
    b = np.zeros(n)
    nlZ = nlZ0
    if last_ttau is not None:
        w = np.asarray(last_ttau, float).reshape(n).copy()
        b = np.asarray(last_tnu, float).reshape(n).copy()
        nlZ = _nlZ(V, d0, w, b, y, m, _State(V, d0, w, b))[0]
        warm_kept = not nlZ > nlZ0
        if not warm_kept:
            w[:] = 0.0
            b[:] = 0.0
            nlZ = nlZ0
    st = _State(V, d0, w, b)
    nlZ_old, sweep = np.inf, 0
    while (abs(nlZ - nlZ_old) > 1e-4 and sweep < 10) or sweep < 2:
        nlZ_old = nlZ
        sweep += 1
        M, h, t = st.M, st.h, st.t.copy()
        if block is None:
            for i in range(n):
                v = V[:, i]
                Mv = M @ v
                vMv = v @ Mv
                sii = d0[i] * t[i] + t[i] * t[i] * vMv
                mui = d0[i] * t[i] * b[i] + t[i] * (v @ h)
                wi, bi = _site(sii, mui, w[i], b[i], m[i], y[i])
                ti = 1.0 / (1.0 + d0[i] * wi)
                ds = wi * ti - w[i] * t[i]
                dtb = ti * bi - t[i] * b[i]
                # M <- (M^-1 + ds v v')^-1 ; h = M V (t o b) with (t o b)_i changed by dtb
                c = ds / (1.0 + ds * vMv)
                h = h - c * Mv * (v @ h) + (Mv - c * Mv * vMv) * dtb
                M = M - c * np.outer(Mv, Mv)
                w[i], b[i], t[i] = wi, bi, ti
        else:
            for i0 in range(0, n, block):
                B = slice(i0, min(n, i0 + block))
                VB = V[:, B]
                X = M @ VB
                G = VB.T @ X
                vh = VB.T @ h
                tB, dB = t[B], d0[B]
                S = np.diag(dB * tB) + tB[:, None] * G * tB[None, :]
                mu = dB * tB * b[B] + tB * vh
                wB, bB = w[B].copy(), b[B].copy()
                for k in range(S.shape[0]):
                    wk, bk = _site(S[k, k], mu[k], wB[k], bB[k], m[B][k], y[B][k])
                    ds2, dn = wk - wB[k], bk - bB[k]
                    sk = S[:, k].copy()
                    c = ds2 / (1.0 + ds2 * sk[k])
                    mu = mu + sk * (dn * (1.0 - c * sk[k]) - c * mu[k])
                    S = S - c * np.outer(sk, sk)
                    wB[k], bB[k] = wk, bk
                tn = 1.0 / (1.0 + dB * wB)
                D = wB * tn - w[B] * tB
                delta = tn * bB - tB * b[B]
                Gn = (S - np.diag(dB * tn)) / np.outer(tn, tn)
                Y = np.diag(D) - D[:, None] * Gn * D[None, :]
                r = delta - Y @ (vh + G @ delta)
                M = M - X @ Y @ X.T
                h = h + X @ r
                w[B], b[B], t[B] = wB, bB, tn
        st = _State(V, d0, w, b)                          # refresh (inf.py:895)
        nlZ, nu_n, tau_n = _nlZ(V, d0, w, b, y, m, st)
    # posterior (inf.py:902-908): dd = s, tnu / ttau dd = t o b
    t = st.t
    s = w * t
    Bm = np.linalg.solve(Luu.T, V)                       # R0'V = inv(Kuu + snu2 I) Ku
    al = t * b - s * (V.T @ st.h)                        # the long alpha
    alpha = Bm @ al
    Wm = np.linalg.solve(st.Lu, V * s)                  # RVdd up to an orthogonal factor
    BW = Bm @ Wm.T
    L = BW @ BW.T - (Bm * s) @ Bm.T
    out = dict(nlZ=nlZ, sweeps=sweep, ttau=w.reshape(n, 1), tnu=b.reshape(n, 1), alpha=alpha.reshape(nu, 1), L=L,
               sW=np.sqrt(w).reshape(n, 1), warm_kept=warm_kept, nu_n=nu_n, tau_n=tau_n)
    cw = (Wm * Wm).sum(0)
    dcov = []
    for ddiagK, dKuu, dKu in ders:                       # inf.py:910-923
        R = 2.0 * dKu - dKuu @ Bm                        # dA'
        wd = (R * Bm).sum(0)
        v = np.asarray(ddiagK, float).reshape(n) - wd
        z = s @ (v + wd) - cw @ v - ((R @ Wm.T) * BW).sum()
        dcov.append((z - al @ (al * v) - (R @ al) @ (Bm @ al)) / 2.0)
    dlZ = erf_ep_moments(y, nu_n / tau_n, 1.0 / tau_n, 2)[1]
    out["dnlZ_cov"] = np.array(dcov)
    out["dnlZ_mean"] = np.array([-(dlZ @ np.asarray(d, float).reshape(n)) for d in dm])
    return out


def fitc_ep_predict(Ks, kss, alpha, L, ms):
    """GP.predict's dense-L branch (Core/gp.py:404-417): Ks = k(xu, xs) (nu, ns)."""
    fm = ms.reshape(-1) + Ks.T @ alpha.reshape(-1)
    fs2 = np.maximum(kss.reshape(-1) + (Ks * (L @ Ks)).sum(0), 0.0)
    return fm, fs2
