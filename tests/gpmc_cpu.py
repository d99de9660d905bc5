"""CPU restatement of GPMC's two loops (Core/gp.py:829-901) over the oracle's binary fits: test infrastructure only.

``fit_and_predict`` is fitAndPredict: per pair (i, j), in the reference's order, createBinaryClass's rows, a cold
``oracle.gp_oracle.ep_fit`` (or ``laplace_fit``), ``predict`` and the vote arithmetic of gp.py:854-862.
``optimize_and_predict`` is optimizeAndPredict with GPC's defaults (Zero mean, lik.Erf, EP, Minimize with 40 line
searches): the CG minimiser of the package (pygps_amd.minimize, host code) drives the oracle's nlZ and gradient with the
warm-started site parameters EP keeps between evaluations, then one more fit at the optimum; with ``chained`` every pair
starts from the previous pair's optimum, as the reference's shared kernel object makes it (gp.py:886)."""
import numpy as np

from oracle import gp_oracle as O


def pairs(n_class):
    return [(i, j) for i in range(n_class) for j in range(i + 1, n_class)]


def binary_class(x_all, y_all, i, j):
    """Rows of class i in data order, then those of class j; labels +1 / -1; also the row numbers."""
    t = np.asarray(y_all).reshape(-1)
    ci = [r for r in range(len(t)) if t[r] == i]
    cj = [r for r in range(len(t)) if t[r] == j]
    idx = np.array(ci + cj, dtype=np.int64)
    y = np.concatenate([np.ones(len(ci)), -np.ones(len(cj))]).reshape(-1, 1)
    return x_all[idx], y, idx


def add_votes(votes, ym, i, j):
    """gp.py:855-861."""
    ym = np.asarray(ym, dtype=float).reshape(-1, 1) + 1
    vote_i = np.zeros_like(votes)
    vote_j = np.zeros_like(votes)
    vote_i[:, i:i + 1] = ym
    vote_j[:, j:j + 1] = 2 - ym
    votes += vote_i
    votes += vote_j
    return votes


def normalise(votes):
    return votes / votes.sum(axis=1)[:, np.newaxis]


def _predict_ym(kind, hyp, para, x, fit, xs, ms):
    return O.predict(kind, hyp, para, 0.0, x, fit["alpha"], fit["L"], fit["sW"], xs, ms, gauss=False)[0]


def fit_and_predict(kind, hyp, para, x_all, y_all, n_class, xs, mean=lambda x: np.zeros((x.shape[0], 1)), laplace=False):
    """votes (ns, n_class), {pair: nlZ}, {pair: sweeps or Newton steps}, {pair: ym}."""
    votes = np.zeros((xs.shape[0], n_class))
    nlZ, iters, yms = {}, {}, {}
    ms = mean(xs)
    for i, j in pairs(n_class):
        x, y, _ = binary_class(x_all, y_all, i, j)
        if laplace:
            fit = O.laplace_fit(kind, hyp, para, x, y, mean(x), nargout=2)
            iters[(i, j)] = int(fit["newton_steps"])
        else:
            fit = O.ep_fit(kind, hyp, para, x, y, mean(x), nargout=2)
            iters[(i, j)] = int(fit["sweeps"])
        nlZ[(i, j)] = float(fit["nlZ"])
        yms[(i, j)] = _predict_ym(kind, hyp, para, x, fit, xs, ms)
        add_votes(votes, yms[(i, j)], i, j)
    return normalise(votes), nlZ, iters, yms


def optimize_and_predict(kind, hyp0, para, x_all, y_all, n_class, xs, chained, num_iters=40):
    """votes, {pair: nlZ at the optimum}, {pair: optimised hyp}; Zero mean."""
    from pygps_amd import minimize
    votes = np.zeros((xs.shape[0], n_class))
    nlZ, hyps = {}, {}
    hyp = np.array(hyp0, dtype=float)
    ms = np.zeros((xs.shape[0], 1))
    for i, j in pairs(n_class):
        x, y, _ = binary_class(x_all, y_all, i, j)
        m = np.zeros((x.shape[0], 1))
        state = {"ttau": None, "tnu": None}

        def objective(h):
            out = O.ep_fit(kind, np.asarray(h, dtype=float), para, x, y, m, last_ttau=state["ttau"], last_tnu=state["tnu"])
            state["ttau"], state["tnu"] = out["ttau"], out["tnu"]
            return out["nlZ"], np.asarray(out["dnlZ_cov"], dtype=float)

        start = hyp.copy() if chained else np.array(hyp0, dtype=float)
        best = minimize.run(objective, start, length=num_iters)[0]
        fit = O.ep_fit(kind, np.asarray(best, dtype=float), para, x, y, m, last_ttau=state["ttau"], last_tnu=state["tnu"])
        hyp = np.asarray(best, dtype=float).copy()
        nlZ[(i, j)] = float(fit["nlZ"])
        hyps[(i, j)] = hyp.copy()
        add_votes(votes, _predict_ym(kind, hyp, para, x, fit, xs, ms), i, j)
    return normalise(votes), nlZ, hyps
