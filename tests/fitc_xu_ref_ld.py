"""Long-double reference of the FITC objective as a function of the inducing inputs xu, and of its gradient w.r.t. xu (test
infrastructure, CPU only; the reference project never differentiates w.r.t. xu, so nothing here is ported).

    nlz_exact(kind, hyp, log_sn, x, y, m, xu)          FITC_Exact's nlZ (csrc/fitc.hip) in long double, with its own Cholesky
    grad_exact(..., dt=LD | float64, mutant=None)      the analytic gradient d nlZ / d xu (nu, D): long double, or the float64 numpy
                                                       restatement (and its single-slip mutants)
    grad_sites(kind, hyp, snu2, x, xu, ttau, tnu, dt)  the same adjoint for FITC_EP from given final sites (the quantities of
                                                       tests/fitc_ep_cpu.py: d0, t = 1 / (1 + d0 w), s = w t, t o b)
    contract(kind, hyp, rows, cols, A, dt)             out[j, k] = 2 scale_k sum_i A_ji k'(s_ji) (r~_jk - c~_ik) alone
    contract_bars(kind, hyp, rows, cols, A)            (bar, T): first-order rounding bar and sum of absolute terms per entry
    tolerance(bar, T, ncols, e64)                      the rule every device comparison uses

Mathematics.  With B = iKuu Ku, A = I + V diag(s) V' = La La', W = La^-1 V diag(s), al the long alpha, w = B al, cw = colsum(W o W)
(s = 1 / g for FITC_Exact, the EP site weights for FITC_EP), every hyper-gradient of the device is
    dnlZ = 1/2 (dk0 sum(s) - w'R al - sum_j v_j al_j^2 - sum_j cw_j v_j - <R W', B W'>),  R = 2 dKu - dKuu B,  v = ddiagK - colsum(R o B).
For a coordinate of xu, ddiagK = 0, hence dnlZ = <G, R>, G = 1/2 (-w al' + B diag(al^2 + cw) - (B W') W), and
    dnlZ = <2 G, dKu> + <C, dKuu>,  C = -G B'.
A kernel k(s) of the scaled squared distance s = sum_k scale_k^2 (a_k - b_k)^2 gives, in scaled coordinates,
    d nlZ / d u_jk = 2 scale_k [ sum_i 2 G_ji k'(s(u_j, x_i)) (u~_jk - x~_ik) + sum_l (C_jl + C_lj) k'(s(u_j, u_l)) (u~_jk - u~_lk) ].

Tolerance of entry (j, k) of a device result against the long-double value (tolerance()):
    bar_jk                  the first-order propagated rounding of the scaled coordinates, of s and of k' (contract_bars)
  + ncols 2^-53 T_jk        the summation bound, T_jk = sum_i |term_jik|
  + 4 2^-53 T_jk            four ulps of the sum of absolute terms
  + 8 e64                   e64 = max |float64 restatement - long double| MEASURED on the case's own inputs
and every case asserts that max tolerance <= CAP max |gradient| (CAP = 1e-5): a tolerance any wrong gradient fits under tests nothing.
"""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53
CAP = 1e-5
FACTOR = 8.0
KP_ULPS = 4.0                     # the device's exp / log / sqrt chains: a few ulps on k'
KINDS = ("RBF", "RBFunit", "RBFard", "RQ", "RQard", "Matern3", "Matern5", "Matern7")
MUTANTS = ("no_kuu", "c_unsym", "dku_factor", "no_cw", "drop64", "ard_scale", "rbf_kprime")


def nhyp(kind, D):
    return {"RBF": 2, "RBFunit": 1, "RBFard": D + 1, "RQ": 3, "RQard": D + 2}.get(kind, 2)


def _as(a, dt):
    a = np.asarray(a)
    return a if a.dtype == dt else a.astype(np.float64).astype(dt)


def kernel(kind, hyp, D, dt=LD, kprime_of=None):
    """(scale (D,), sf2, k, k1, k2): the kernel as a function of the scaled squared distance, its first and second derivative.
    kprime_of: take k1 / k2 from another kind (the mutant 'k' of RBF used for Matern 5')."""
    h = _as(hyp, dt)
    one, half = dt(1), dt(0.5)
    if kind in ("RBF", "RBFunit", "RBFard"):
        if kind == "RBFard":
            scale, sf2 = np.exp(-h[:D]), np.exp(2 * h[D])
        else:
            scale, sf2 = np.ones(D, dtype=dt) / np.exp(h[0]), (np.exp(2 * h[1]) if kind == "RBF" else one)
        k = lambda s: sf2 * np.exp(-half * s)
        k1 = lambda s: -half * sf2 * np.exp(-half * s)
        k2 = lambda s: dt(0.25) * sf2 * np.exp(-half * s)
    elif kind in ("RQ", "RQard"):
        if kind == "RQard":
            scale, sf2, al = np.exp(-h[:D]), np.exp(2 * h[D]), np.exp(h[D + 1])
        else:
            scale, sf2, al = np.ones(D, dtype=dt) / np.exp(h[0]), np.exp(2 * h[1]), np.exp(h[2])
        base = lambda s: one + half * s / al
        k = lambda s: sf2 * base(s) ** (-al)
        k1 = lambda s: -half * sf2 * base(s) ** (-al - one)
        k2 = lambda s: sf2 * (al + one) / (4 * al) * base(s) ** (-al - 2)
    elif kind in ("Matern3", "Matern5", "Matern7"):
        d = int(kind[-1])
        scale, sf2 = np.sqrt(dt(d)) * np.ones(D, dtype=dt) / np.exp(h[0]), np.exp(2 * h[1])
        if d == 3:
            k = lambda s: sf2 * (one + np.sqrt(s)) * np.exp(-np.sqrt(s))
            k1 = lambda s: -half * sf2 * np.exp(-np.sqrt(s))
            k2 = lambda s: sf2 * np.exp(-np.sqrt(s)) / (4 * np.sqrt(s))          # unbounded at s = 0: contract_bars guards it
        elif d == 5:
            k = lambda s: sf2 * (one + np.sqrt(s) + s / 3) * np.exp(-np.sqrt(s))
            k1 = lambda s: -sf2 * (one + np.sqrt(s)) / 6 * np.exp(-np.sqrt(s))
            k2 = lambda s: sf2 / 12 * np.exp(-np.sqrt(s))
        else:
            k = lambda s: sf2 * (one + np.sqrt(s) + 2 * s / 5 + s * np.sqrt(s) / 15) * np.exp(-np.sqrt(s))
            k1 = lambda s: -sf2 * (3 + 3 * np.sqrt(s) + s) / 30 * np.exp(-np.sqrt(s))
            k2 = lambda s: sf2 * (one + np.sqrt(s)) / 60 * np.exp(-np.sqrt(s))
    else:
        raise ValueError(kind)
    if kprime_of is not None:
        _, _, _, k1, k2 = kernel(kprime_of, hyp, D, dt)
    return scale, sf2, k, k1, k2


def sqdist(a, b):
    """sum_k (a_jk - b_ik)^2 in the difference form, coordinates in order."""
    s = np.zeros((a.shape[0], b.shape[0]), dtype=a.dtype)
    for k in range(a.shape[1]):
        df = a[:, k, None] - b[None, :, k]
        s += df * df
    return s


def chol(B):
    """Lower Cholesky factor, column by column, in the dtype of B."""
    n = B.shape[0]
    L = np.zeros_like(B)
    for j in range(n):
        v = B[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError("pivot %d is not positive" % (j + 1))
        L[j:, j] = v / np.sqrt(v[0])
    return L


def solve_lower(L, X):
    """L^-1 X by forward substitution."""
    Y = np.array(X, dtype=L.dtype, copy=True)
    for i in range(L.shape[0]):
        if i:
            Y[i] -= L[i, :i] @ Y[:i]
        Y[i] /= L[i, i]
    return Y


def solve_upper(U, X):
    """U^-1 X by back substitution."""
    Y = np.array(X, dtype=U.dtype, copy=True)
    n = U.shape[0]
    for i in range(n - 1, -1, -1):
        if i < n - 1:
            Y[i] -= U[i, i + 1:] @ Y[i + 1:]
        Y[i] /= U[i, i]
    return Y


def _core(kind, hyp, snu2, x, xu, dt, kprime_of=None):
    x, xu = _as(x, dt), _as(xu, dt)
    D = x.shape[1]
    scale, sf2, k, k1, k2 = kernel(kind, hyp, D, dt, kprime_of)
    xs, us = x * scale, xu * scale
    Sux, Suu = sqdist(us, xs), sqdist(us, us)
    Kuu = k(Suu) + dt(snu2) * np.eye(xu.shape[0], dtype=dt)
    Luu = chol(Kuu)
    V = solve_lower(Luu, k(Sux))                                   # Luu^-1 Ku
    return dict(scale=scale, kss=sf2, k1=k1, xs=xs, us=us, Sux=Sux, Suu=Suu, Luu=Luu, V=V, dt=dt)


def nlz_exact(kind, hyp, log_sn, x, y, m, xu, dt=LD):
    """FITC_Exact's negative log marginal likelihood (Core/inf.py:398-428 as csrc/fitc.hip computes it)."""
    sn2 = np.exp(2 * dt(log_sn))
    c = _core(kind, hyp, dt(1e-6) * sn2, x, xu, dt)
    V = c["V"]
    n = V.shape[1]
    g = c["kss"] + sn2 - (V * V).sum(axis=0)
    r = (_as(y, dt).reshape(n) - _as(m, dt).reshape(n)) / np.sqrt(g)
    Vs = V / np.sqrt(g)
    La = chol(np.eye(V.shape[0], dtype=dt) + Vs @ Vs.T)
    be = solve_lower(La, Vs @ r)
    return np.log(np.diag(La)).sum() + (np.log(g).sum() + n * np.log(2 * dt(np.pi)) + r @ r - be @ be) / 2


def contract(kind, hyp, rows, cols, A, dt=LD, scale_slip=False, kprime_of=None):
    """out[j, k] = 2 scale_k sum_i A_ji k'(s_ji) (r~_jk - c~_ik), columns summed in order."""
    rows, cols, A = _as(rows, dt), _as(cols, dt), _as(A, dt)
    D = rows.shape[1]
    scale, _, _, k1, _ = kernel(kind, hyp, D, dt, kprime_of)
    rs, cs = rows * scale, cols * scale
    Wt = A * k1(sqdist(rs, cs))
    out = np.zeros((rows.shape[0], D), dtype=dt)
    for k in range(D):
        sk = scale[(k + 1) % D] if (scale_slip and k == 0) else scale[k]
        out[:, k] = 2 * sk * (Wt * (rs[:, k, None] - cs[None, :, k])).sum(axis=1)
    return out


def contract_bars(kind, hyp, rows, cols, A):
    """(bar, T) per entry, float64.  T_jk = sum_i |term_jik|.  bar_jk: what the device's roundings do to first order -- the scaled
    coordinates (one rounding each: the difference is off by 2^-53 (|r~| + |c~|)), s (that, and D + 2 roundings of the sum) through
    k'', the evaluation of k' (KP_ULPS) and the products."""
    rows, cols, A = _as(rows, np.float64), _as(cols, np.float64), np.abs(_as(A, np.float64))
    D = rows.shape[1]
    scale, _, _, k1, k2 = kernel(kind, hyp, D, np.float64)
    rs, cs = rows * scale, cols * scale
    s = sqdist(rs, cs)
    ds = (D + 2) * EPS * s
    for k in range(D):
        ds += 2 * np.abs(rs[:, k, None] - cs[None, :, k]) * EPS * (np.abs(rs[:, k, None]) + np.abs(cs[None, :, k]))
    with np.errstate(divide="ignore", invalid="ignore"):
        a1, a2 = np.abs(k1(s)), np.where(s > 0, np.abs(k2(s)), 0.0)
    bar, T = np.zeros((rows.shape[0], D)), np.zeros((rows.shape[0], D))
    for k in range(D):
        df = np.abs(rs[:, k, None] - cs[None, :, k])
        ddf = EPS * (np.abs(rs[:, k, None]) + np.abs(cs[None, :, k]))
        pre = 2 * scale[k] * A
        T[:, k] = (pre * a1 * df).sum(axis=1)
        bar[:, k] = (pre * (a2 * ds * df + a1 * (ddf + (KP_ULPS + 3) * EPS * df))).sum(axis=1)
    return bar, T


def tolerance(bar, T, ncols, e64):
    return bar + (ncols + 4) * EPS * T + FACTOR * e64


def _adjoint(c, svec, tb, mutant=None):
    """(2 G (nu, n), C + C' (nu, nu)) from the FITC quantities: svec = 1 / g or the EP site weights s, tb = svec o (y - m) or t o b."""
    dt, V, Luu = c["dt"], c["V"], c["Luu"]
    nu = V.shape[0]
    Vd = V * svec
    La = chol(np.eye(nu, dtype=dt) + Vd @ V.T)
    h = solve_upper(La.T, solve_lower(La, V @ tb))                 # A^-1 V tb
    al = tb - svec * (V.T @ h)
    Bm = solve_upper(Luu.T, V)                                     # iKuu Ku
    W = solve_lower(La, Vd)
    w = Bm @ al
    cw = (W * W).sum(axis=0)
    if mutant == "no_cw":
        cw = np.zeros_like(cw)
    G2 = -np.outer(w, al) + Bm * (al * al + cw) - (Bm @ W.T) @ W   # 2 G
    C = -(G2 @ Bm.T) / 2
    # C = -1/2 (-w w' + B diag(al^2 + cw) B' - (B W')(B W')') is symmetric up to rounding, so "not symmetrised" can only slip by
    # leaving the transposed term out: u_j moves row j AND column j of Kuu
    S = C if mutant == "c_unsym" else C + C.T
    if mutant == "dku_factor":
        G2 = G2 / 2
    return G2, S


def _grad(kind, hyp, c, svec, tb, mutant, x, xu):
    G2, S = _adjoint(c, svec, tb, mutant)
    dt = c["dt"]
    kp = "RBF" if mutant == "rbf_kprime" else None
    slip = mutant == "ard_scale"
    xcols = x[:-64] if mutant == "drop64" else x
    g = contract(kind, hyp, xu, xcols, G2[:, :xcols.shape[0]], dt, slip, kp)
    if mutant != "no_kuu":
        g = g + contract(kind, hyp, xu, xu, S, dt, slip, kp)
    return g


def grad_exact(kind, hyp, log_sn, x, y, m, xu, dt=LD, mutant=None):
    """d nlZ / d xu of FITC_Exact, (nu, D)."""
    sn2 = np.exp(2 * dt(log_sn))
    c = _core(kind, hyp, dt(1e-6) * sn2, x, xu, dt)
    n = c["V"].shape[1]
    g = c["kss"] + sn2 - (c["V"] * c["V"]).sum(axis=0)
    res = _as(y, dt).reshape(n) - _as(m, dt).reshape(n)
    return _grad(kind, hyp, c, 1 / g, res / g, mutant, x, xu)


def grad_sites(kind, hyp, snu2, x, xu, ttau, tnu, dt=LD, mutant=None):
    """d nlZ / d xu of FITC_EP at the given final sites, (nu, D): d0 = diagK - colsum(V o V), t = 1 / (1 + d0 w), s = w t, the long
    alpha from t o b (tests/fitc_ep_cpu.py; the prior mean sits inside tnu)."""
    c = _core(kind, hyp, snu2, x, xu, dt)
    n = c["V"].shape[1]
    w, b = _as(ttau, dt).reshape(n), _as(tnu, dt).reshape(n)
    d0 = c["kss"] - (c["V"] * c["V"]).sum(axis=0)
    t = 1 / (1 + d0 * w)
    return _grad(kind, hyp, c, w * t, t * b, mutant, x, xu)


def grad_bars(kind, hyp, G2, S, x, xu):
    """(bar, T) of the two contractions of a full gradient, from the adjoint of the long-double side."""
    b1, T1 = contract_bars(kind, hyp, xu, x, G2)
    b2, T2 = contract_bars(kind, hyp, xu, xu, S)
    return b1 + b2, T1 + T2


def exact_case(kind, hyp, log_sn, x, y, m, xu):
    """(gradient in long double rounded to float64, tolerance (nu, D), e64) of a FITC_Exact case: the unit the GPU tests assert in."""
    g_ld = grad_exact(kind, hyp, log_sn, x, y, m, xu, LD)
    g_64 = grad_exact(kind, hyp, log_sn, x, y, m, xu, np.float64)
    e64 = float(np.abs(g_64.astype(LD) - g_ld).max())
    sn2 = np.exp(2 * np.float64(log_sn))
    c = _core(kind, hyp, 1e-6 * sn2, x, xu, np.float64)
    n = c["V"].shape[1]
    g = c["kss"] + sn2 - (c["V"] * c["V"]).sum(axis=0)
    res = _as(y, np.float64).reshape(n) - _as(m, np.float64).reshape(n)
    G2, S = _adjoint(c, 1 / g, res / g)
    bar, T = grad_bars(kind, hyp, G2, S, x, xu)
    return g_ld.astype(np.float64), tolerance(bar, T, n + xu.shape[0], e64), e64


def sites_case(kind, hyp, snu2, x, xu, ttau, tnu):
    g_ld = grad_sites(kind, hyp, snu2, x, xu, ttau, tnu, LD)
    g_64 = grad_sites(kind, hyp, snu2, x, xu, ttau, tnu, np.float64)
    e64 = float(np.abs(g_64.astype(LD) - g_ld).max())
    c = _core(kind, hyp, snu2, x, xu, np.float64)
    n = c["V"].shape[1]
    w, b = _as(ttau, np.float64).reshape(n), _as(tnu, np.float64).reshape(n)
    d0 = c["kss"] - (c["V"] * c["V"]).sum(axis=0)
    t = 1 / (1 + d0 * w)
    G2, S = _adjoint(c, w * t, t * b)
    bar, T = grad_bars(kind, hyp, G2, S, x, xu)
    return g_ld.astype(np.float64), tolerance(bar, T, n + xu.shape[0], e64), e64


def central_difference(f, xu, e):
    """Central differences of a scalar function of xu in long double, entry by entry."""
    xu = _as(xu, LD)
    g = np.zeros_like(xu)
    for j in range(xu.shape[0]):
        for k in range(xu.shape[1]):
            up, dn = xu.copy(), xu.copy()
            up[j, k] += e
            dn[j, k] -= e
            g[j, k] = (f(up) - f(dn)) / (2 * LD(e))
    return g
