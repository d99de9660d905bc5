"""Long-double restatement of the spectral mixture kernel cov.SM for any D, with a per-entry error bar (test infrastructure,
CPU only; the companion of tests/kernel_ref_ld.py, whose EPS, C, TINY and ARG_REL it reuses).

    sm_matrix(hyp, Q, x=None, z=None, mode=..., der=None) -> (K, bar)
    sm_hadamard_ref(hyp, Q, x, weightings) -> [(sums, bars), ...]

The documented formula (Core/cov.py:454-479, GPML covSM), hyp = [log w (Q) | log m (D x Q) | log sqrt(v) (D x Q)], (j, q) at j Q + q:

    k = sum_q T_q,   T_q = w_q E_q prod_j c_jq,   E_q = exp(-X_q),  X_q = sum_j u_jq,  u_jq = 2 pi^2 v_jq t_j^2,
    c_jq = cos a_jq,  a_jq = 2 pi m_jq t_j,  t_j = x_j - z_j

    d / d log w_q       = T_q
    d / d log m_jq      = w_q E_q (prod_{j' != j} c_j'q) (-a_jq sin a_jq)
    d / d log sqrt(v_jq) = T_q (-2 u_jq)                                   (-(2 pi)^2 v_jq t_j^2)

x / z are the exact fp64 arrays handed to the device; everything after them runs in np.longdouble.

The bar is derived, not measured.  An fp64 evaluation may be off by
  * the rounding of each t_j = x_j - z_j:                       dt_j = EPS (|x_j| + |z_j|);
  * a relative ARG_REL on each trigonometric argument:           dA_j = ARG_REL |a_j| + 2 pi m_j dt_j   (with t_j's share);
  * the exponent's own rounding, EPS (D + 2) relative, and t's:  dX = EPS (D + 2) X + sum_j 4 pi^2 v_j |t_j| dt_j;
  * C EPS of the term itself (the products, exp, cos, the sum over the components).
These are pushed through the term with the product rule for bounds, |prod (f_k + d_k) - prod f_k| <= prod (|f_k| + |d_k|) -
prod |f_k| (all orders, no division by a cosine that may vanish):
    dc_j = |sin a_j| dA_j + dA_j^2 / 2,   d(a sin a)_j = (|sin a_j| + |a_j cos a_j|) dA_j + (1 + |a_j| / 2) dA_j^2,
    dE = E expm1(dX),   du_j = 4 pi^2 v_j |t_j| dt_j,
and bar = sum over the components of C (EPS |term| + d term) + TINY.  The reference's own fp64 evaluation obeys the same bar.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from kernel_ref_ld import ARG_REL, C, EPS, LD, TINY

PI = LD("3.14159265358979323846264338327950288")


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def split_hyp(hyp, Q, D):
    """(w (Q), m (D, Q), v (D, Q)) in long double from the log-space hyp."""
    h = np.asarray(hyp)
    h = (h if h.dtype == LD else _ld(h)).reshape(-1)          # long-double hypers pass through (finite differences)
    assert h.size == Q * (1 + 2 * D), "SM: len(hyp) must be Q (1 + 2 D)"
    return np.exp(h[:Q]), np.exp(h[Q:Q + Q * D]).reshape(D, Q), np.exp(2 * h[Q + Q * D:]).reshape(D, Q)


def decode_der(der, Q, D):
    """(type, j, q): type 0 log w_q, 1 log m_jq, 2 log sqrt(v_jq)."""
    if der < 0 or der >= Q * (1 + 2 * D):
        raise Exception("Wrong derivative entry in SM")
    if der < Q:
        return 0, -1, der
    r = (der - Q) % (Q * D)
    return (1 if der < Q + Q * D else 2), r // Q, r % Q


def _loo(f):
    """Leave-one-out products of the list f: out[j] = prod_{k != j} f[k] (prefix / suffix, no division)."""
    n = len(f)
    pre = [None] * n
    acc = None
    for j in range(n):
        pre[j] = acc
        acc = f[j] if acc is None else acc * f[j]
    out = [None] * n
    suf = None
    for j in range(n - 1, -1, -1):
        a, b = pre[j], suf
        out[j] = (a * b if b is not None else a) if a is not None else (b if b is not None else LD(1) + 0 * f[j])
        suf = f[j] if suf is None else suf * f[j]
    return out, acc


class _Component(object):
    """Everything component q contributes at the differences t (list of D arrays) with roundings dt: the value term and all
    1 + 2 D derivative terms, each with its d term (module docstring)."""

    def __init__(self, wq, mq, vq, t, dt):
        D = len(t)
        a = [2 * PI * mq[j] * t[j] for j in range(D)]
        c = [np.cos(a[j]) for j in range(D)]
        s = [np.sin(a[j]) for j in range(D)]
        u = [2 * PI * PI * vq[j] * t[j] * t[j] for j in range(D)]
        du = [4 * PI * PI * vq[j] * np.abs(t[j]) * dt[j] for j in range(D)]
        X = sum(u[1:], u[0])
        dX = EPS * (D + 2) * X + sum(du[1:], du[0])
        dA = [ARG_REL * np.abs(a[j]) + 2 * PI * mq[j] * dt[j] for j in range(D)]
        dc = [np.abs(s[j]) * dA[j] + dA[j] * dA[j] / 2 for j in range(D)]
        E = np.exp(-X)
        Eb = E * np.exp(dX)                                  # E + dE
        L, P = _loo(c)
        ac = [np.abs(c[j]) for j in range(D)]
        La, Pa = _loo(ac)
        Lb, Pb = _loo([ac[j] + dc[j] for j in range(D)])
        self.D = D
        self.T = wq * E * P
        self.dT = wq * (Eb * Pb - E * Pa)
        self.Tm, self.dTm, self.Tv, self.dTv = [], [], [], []
        aT = np.abs(self.T)
        for j in range(D):
            f = -a[j] * s[j]
            fa = np.abs(f)
            fb = fa + (np.abs(s[j]) + np.abs(a[j] * c[j])) * dA[j] + (1 + np.abs(a[j]) / 2) * dA[j] * dA[j]
            self.Tm.append(wq * E * L[j] * f)
            self.dTm.append(wq * (Eb * Lb[j] * fb - E * La[j] * fa))
            self.Tv.append(self.T * (-2 * u[j]))
            self.dTv.append(2 * ((aT + self.dT) * (u[j] + du[j]) - aT * u[j]))


def _diffs(x, z):
    """t_j (long double) and dt_j = EPS (|x_j| + |z_j|) for every coordinate."""
    t, dt = [], []
    for j in range(x.shape[1]):
        a, b = _ld(x[:, j]), _ld(z[:, j])
        t.append(a[:, None] - b[None, :])
        dt.append(EPS * (np.abs(a)[:, None] + np.abs(b)[None, :]))
    return t, dt


def _bar(val, dval):
    return C * (EPS * np.abs(val).astype(np.float64) + np.asarray(dval, dtype=np.float64))


def sm_matrix(hyp, Q, x=None, z=None, mode=None, der=None):
    """(K, bar): value (der None) or derivative matrix in long double and the bar of an fp64 evaluation.
    Shapes as getCovMatrix: 'train' (n, n), 'cross' (n, m), 'self_test' (m, 1)."""
    ref = np.asarray(z if mode == "self_test" else x, dtype=np.float64)
    D = ref.shape[1]
    w, m, v = split_hyp(hyp, Q, D)
    if mode == "self_test":
        xx, zz = np.zeros((ref.shape[0], D)), np.zeros((1, D))
    else:
        xx = ref
        zz = ref if mode == "train" else np.asarray(z, dtype=np.float64)
    t, dt = _diffs(xx, zz)
    if der is None:
        K = np.zeros(t[0].shape, dtype=LD)
        bar = np.zeros(t[0].shape)
        for q in range(Q):
            comp = _Component(w[q], m[:, q], v[:, q], t, dt)
            K += comp.T
            bar += _bar(comp.T, comp.dT)
        return K, bar + C * EPS * np.abs(K).astype(np.float64) + TINY          # the sum over the components
    typ, j, q = decode_der(der, Q, D)
    comp = _Component(w[q], m[:, q], v[:, q], t, dt)
    if typ == 0:
        val, dval = comp.T, comp.dT
    elif typ == 1:
        val, dval = comp.Tm[j], comp.dTm[j]
    else:
        val, dval = comp.Tv[j], comp.dTv[j]
    return val, _bar(val, dval) + TINY


def sm_fp64(hyp, Q, x=None, z=None, mode=None, der=None):
    """The same formulas in plain numpy fp64 (what a host evaluation would give): feeds the dense route in tests."""
    ref = np.asarray(z if mode == "self_test" else x, dtype=np.float64)
    D = ref.shape[1]
    h = np.asarray(hyp, dtype=np.float64)
    w, m, v = np.exp(h[:Q]), np.exp(h[Q:Q + Q * D]).reshape(D, Q), np.exp(2 * h[Q + Q * D:]).reshape(D, Q)
    if mode == "self_test":
        xx, zz = np.zeros((ref.shape[0], D)), np.zeros((1, D))
    else:
        xx = ref
        zz = ref if mode == "train" else np.asarray(z, dtype=np.float64)
    t = [xx[:, j][:, None] - zz[:, j][None, :] for j in range(D)]
    typ, dj, dq = (-1, -1, -1) if der is None else decode_der(der, Q, D)
    K = np.zeros(t[0].shape)
    for q in (range(Q) if der is None else [dq]):
        T = w[q] * np.exp(-2 * np.pi ** 2 * sum(v[j, q] * t[j] ** 2 for j in range(D)))
        for j in range(D):
            a = 2 * np.pi * m[j, q] * t[j]
            T = T * (-a * np.sin(a) if (typ == 1 and j == dj) else np.cos(a))
        if typ == 2:
            T = T * (-(2 * np.pi) ** 2 * v[dj, q] * t[dj] ** 2)
        K = K + T
    return K


# ---- the gradient pass --------------------------------------------------------------------------------------------
def sm_hadamard_ref(hyp, Q, x, weightings, rows=None, threads=8):
    """Reference of the fits' gradient pass for SM: for every weighting (Binv, alpha, wv, sn2) the sums sum_ij Q_ij dK_h,ij over
    all Q (1 + 2 D) hypers (Qm = Binv o (w w') - alpha alpha'; without wv the weights are 1 / sn2) in long double, then
    sn2 tr(Qm), and their bars, built like kernel_ref_ld.hadamard_ref: C EPS L sum_ij (|Binv w w'| + |alpha alpha'|)_ij |dK_h,ij| +
    sum_ij |Qm_ij| bar(dK_h)_ij, L = 2 + log2(n^2).  One pass over the geometry serves all weightings and all hypers (the
    per-component quantities are shared); row blocks run on a few threads (numpy releases the GIL in its inner loops)."""
    x = np.asarray(x, dtype=np.float64)
    n, D = x.shape
    nh = Q * (1 + 2 * D)
    w, m, v = split_hyp(hyp, Q, D)
    Lr = 2.0 + np.log2(float(n) * n)
    if rows is None:                                          # ~60 long-double arrays of rows x n per coordinate and thread
        rows = int(max(8, min(128, 2e6 // (n * D))))
    mats = []
    for Binv, alpha, wv, sn2 in weightings:
        B = _ld(Binv)
        a = _ld(alpha).reshape(-1)
        W = np.full((n, n), 1 / LD(sn2), dtype=LD) if wv is None else _ld(wv).reshape(-1)[:, None] * _ld(wv).reshape(-1)[None, :]
        aa = a[:, None] * a[None, :]
        Qm = B * W - aa
        mats.append((Qm, np.abs(Qm).astype(np.float64), (np.abs(B * W) + np.abs(aa)).astype(np.float64), sn2))

    def block(r0):
        r1 = min(n, r0 + rows)
        t, dt = _diffs(x[r0:r1], x)
        sums = [np.zeros(nh, dtype=LD) for _ in mats]
        bars = [np.zeros(nh) for _ in mats]
        for q in range(Q):
            comp = _Component(w[q], m[:, q], v[:, q], t, dt)
            terms = [(q, comp.T, comp.dT)]
            for j in range(D):
                terms.append((Q + j * Q + q, comp.Tm[j], comp.dTm[j]))
                terms.append((Q + Q * D + j * Q + q, comp.Tv[j], comp.dTv[j]))
            for h, val, dval in terms:
                av = np.abs(val).astype(np.float64)
                bv = _bar(val, dval) + TINY
                for k, (Qm, aQ, rQ, _) in enumerate(mats):
                    sums[k][h] += np.sum(Qm[r0:r1] * val)
                    bars[k][h] += C * EPS * Lr * float(np.sum(rQ[r0:r1] * av)) + float(np.sum(aQ[r0:r1] * bv))
        return sums, bars

    with ThreadPoolExecutor(max_workers=threads) as ex:
        parts = list(ex.map(block, range(0, n, rows)))
    out = []
    for k, (Qm, aQ, rQ, sn2) in enumerate(mats):
        sums = np.zeros(nh + 1, dtype=LD)
        bars = np.zeros(nh + 1)
        for ps, pb in parts:
            sums[:nh] += ps[k]
            bars[:nh] += pb[k]
        bars[:nh] += TINY
        sums[nh] = LD(sn2) * np.trace(Qm)
        bars[nh] = C * EPS * Lr * float(sn2) * float(np.sum(np.diag(rQ))) + TINY
        out.append((sums, bars))
    return out
