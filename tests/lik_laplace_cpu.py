"""CPU restatement of EP.evaluate (Core/inf.py:731-806, _epComputeParams :174-189) with lik.Laplace, for the lik.Laplace
tests.  Not a test module.

The moments are pygps_amd.lik.Laplace's EP mode (the reference's arithmetic, elementwise).  The sweep is the reference's
per-site loop with rank-1 updates of Sigma, the parameters are recomputed after every sweep, warm start as inf.py:744-753.
Gradients: ``point="f"`` (the library's default) evaluates dlZ and dlZhyp at the cavity of f, nu_n / tau_n + m;
``point="reference"`` at the reference's nu_n / tau_n (dnlZ.lik as inf.py:796-798; the mean gradient stays per site)."""
import numpy as np

from oracle.gp_oracle import jitchol, solve_chol
from pygps_amd import inf, lik


def _params(K, y, ttau, tnu, L_, m):
    """inf.py:174-189 with the reference's column vectors, jitchol and LU solve."""
    n = len(y)
    ttau, tnu, m, yc = ttau[:, None], tnu[:, None], m[:, None], y[:, None]
    ssi = np.sqrt(ttau)
    L = jitchol(np.eye(n) + (ssi @ ssi.T) * K).T
    V = np.linalg.solve(L.T, np.tile(ssi, (1, n)) * K)
    Sigma = K - V.T @ V
    mu = Sigma @ tnu
    ds = np.diag(Sigma).reshape(n, 1)
    tau_n = 1 / ds - ttau
    nu_n = mu / ds - tnu + m * tau_n
    lZ = L_.evaluate(yc, nu_n / tau_n, 1 / tau_n, inf.EP())
    nlZ = (np.log(np.diag(L)).sum() - lZ.sum() - (tnu.T @ (Sigma @ tnu)) / 2
           - ((nu_n - m * tau_n).T @ ((ttau / tau_n * (nu_n - m * tau_n) - 2 * tnu) / (ttau + tau_n))) / 2
           + (tnu ** 2 / (tau_n + ttau)).sum() / 2.0 - np.log(1.0 + ttau / tau_n).sum() / 2.0)
    return Sigma, mu.ravel(), float(nlZ[0, 0]), L


def ep_laplace_fit(K, y, m, log_sn, dm=(), dK=(), last_ttau=None, last_tnu=None, tol=1e-4, max_sweep=10, point="f"):
    """Dense EP with lik.Laplace(log_sn).  K (n, n), y, m (n,), dm: mean derivative vectors, dK: covariance derivative
    matrices.  Returns a dict with nlZ, ttau, tnu, alpha, sW, sweeps, dnlZ_mean, dnlZ_cov, dnlZ_lik."""
    L_ = lik.Laplace(log_sn)
    y = np.asarray(y, dtype=float).ravel()
    m = np.asarray(m, dtype=float).ravel()
    n = len(y)
    nlZ0 = -L_.evaluate(y, m, np.diag(K).copy(), inf.EP()).sum()
    if last_ttau is None:
        ttau, tnu, Sigma, mu, nlZ = np.zeros(n), np.zeros(n), K.copy(), np.zeros(n), nlZ0
    else:
        ttau, tnu = np.array(last_ttau, dtype=float).ravel(), np.array(last_tnu, dtype=float).ravel()
        Sigma, mu, nlZ, _ = _params(K, y, ttau, tnu, L_, m)
        if nlZ > nlZ0:
            ttau, tnu, Sigma, mu, nlZ = np.zeros(n), np.zeros(n), K.copy(), np.zeros(n), nlZ0
    nlZ_old, sweep = np.inf, 0
    while (abs(nlZ - nlZ_old) > tol and sweep < max_sweep) or sweep < 2:
        nlZ_old = nlZ
        sweep += 1
        for i in range(n):
            tau_ni = 1 / Sigma[i, i] - ttau[i]
            nu_ni = mu[i] / Sigma[i, i] + m[i] * tau_ni - tnu[i]
            _, dlZ, d2lZ = (float(v) for v in L_.evaluate(y[i], nu_ni / tau_ni, 1 / tau_ni, inf.EP(), None, 3))
            ttau_old = ttau[i]
            ttau[i] = max(-d2lZ / (1 + d2lZ / tau_ni), 0)
            tnu[i] = (dlZ + (m[i] - nu_ni / tau_ni) * d2lZ) / (1 + d2lZ / tau_ni)
            ds2 = ttau[i] - ttau_old
            si = Sigma[:, i].copy()
            Sigma = Sigma - ds2 / (1 + ds2 * si[i]) * np.dot(si[:, None], si[None, :])
            mu = np.dot(Sigma, tnu[:, None]).ravel()            # (n, 1) operands: the reference's BLAS call
        Sigma, mu, nlZ, L = _params(K, y, ttau, tnu, L_, m)
    sW = np.sqrt(ttau)
    alpha = (tnu[:, None] - sW[:, None] * solve_chol(L, sW[:, None] * (K @ tnu[:, None]))).ravel()
    out = dict(nlZ=nlZ, ttau=ttau, tnu=tnu, alpha=alpha, sW=sW, sweeps=sweep, L=L)
    ds = np.diag(Sigma)
    tau_n = 1 / ds - ttau
    nu_n = mu / ds - tnu
    at = nu_n / tau_n + (m if point == "f" else 0.0)
    F = np.outer(alpha, alpha) - sW[:, None] * solve_chol(L, np.diag(sW))
    out["dnlZ_cov"] = np.array([-(F * d).sum() / 2 for d in dK])
    out["dnlZ_lik"] = np.array([-L_.evaluate(y, at, 1 / tau_n, inf.EP(), 0).sum()])
    dlZ = L_.evaluate(y, at, 1 / tau_n, inf.EP(), None, 2)[1]
    out["dnlZ_mean"] = np.array([-(dlZ @ np.asarray(d, dtype=float).ravel()) for d in dm])
    return out
