"""Likelihoods on the path (reference: pyGPs/Core/lik.py -- Gauss :123-198, Erf :236-366).

``Gauss`` is the type gate and noise source of Exact inference (Core/inf.py:354,360) and supplies
the predictive moments (Core/gp.py:422-427); ``Erf`` supplies the probit predictive and the EP site
moments; ``Laplace`` (Core/lik.py:370-580) is the heavy-tailed regression likelihood of EP.  Both have the Laplace mode (lp and its derivatives in f, Core/lik.py:175-197, 274-293); the
Laplace fit itself evaluates them on the device (csrc/erf_lik.h).  All of it is O(N) scalar host work."""
import numpy as np
from scipy.special import erf as _erf
from scipy.special import erfc as _erfc


class Likelihood(object):
    def __init__(self):
        self.hyp = []

    def evaluate(self, y=None, mu=None, s2=None, inffunc=None, der=None, nargout=1):
        raise NotImplementedError


def _take(values, nargout):
    return values[0] if nargout <= 1 else tuple(values[:nargout])


class Gauss(Likelihood):
    """hyp = [log_sigma]"""

    def __init__(self, log_sigma=np.log(0.1)):
        self.hyp = [log_sigma]

    def evaluate(self, y=None, mu=None, s2=None, inffunc=None, der=None, nargout=1):
        from . import inf
        sn2 = np.exp(2. * self.hyp[0])
        if inffunc is None:                                   # prediction mode (lik.py:134-158)
            if y is None:
                y = np.zeros_like(mu)
            if s2 is not None and np.linalg.norm(s2) > 0:
                lp = self.evaluate(y, mu, s2, inf.EP())
            else:
                lp = -(y - mu) ** 2 / sn2 / 2 - np.log(2. * np.pi * sn2) / 2.
                s2 = np.zeros_like(s2) if s2 is not None else 0.0
            return _take((lp, mu, s2 + sn2), nargout)
        if isinstance(inffunc, inf.EP):                       # lik.py:160-176
            if der is None:
                v = sn2 + s2
                return _take((-(y - mu) ** 2 / v / 2. - np.log(2 * np.pi * v) / 2., (y - mu) / v, -1 / v), nargout)
            return ((y - mu) ** 2 / (sn2 + s2) - 1) / (1 + s2 / sn2)
        if isinstance(inffunc, inf.Laplace):                  # lik.py:175-197
            if y is None:
                y = 0
            if der is None:
                r = y - mu
                lp = -r ** 2 / (2 * sn2) - np.log(2 * np.pi * sn2) / 2.
                return _take((lp, r / sn2, -np.ones_like(r) / sn2, np.zeros_like(r)), nargout)
            return (y - mu) ** 2 / sn2 - 1, 2 * (mu - y) / sn2, 2 * np.ones_like(mu) / sn2
        raise Exception("Incorrect inference in lik.Gauss\n")


class Erf(Likelihood):
    """Cumulative Gaussian (probit) likelihood for labels in {+1,-1}; no hyper-parameters."""

    def __init__(self):
        self.hyp = []

    @staticmethod
    def _logphi(z, p):
        """log Phi(z) with the asymptotic branch below -6.2 and a blend on [-6.2,-5.5] (lik.py:354-366)."""
        z = np.asarray(z, dtype=float)
        lp = np.zeros_like(z)
        lo, hi = -6.2, -5.5
        safe = z > hi
        far = z < lo
        rest = ~safe
        mid = rest & ~far
        lam = 1. / (1. + np.exp(25. * (0.5 - (z[mid] - lo) / (hi - lo))))
        lp[safe] = np.log(p[safe])
        zr = z[rest]
        lp[rest] = -np.log(np.pi) / 2. - zr ** 2 / 2. - np.log(np.sqrt(zr ** 2 / 2. + 2.) - zr / np.sqrt(2.))
        lp[mid] = (1 - lam) * lp[mid] + lam * np.log(p[mid])
        return lp

    @staticmethod
    def _ratio(f, p):
        """N(f)/Phi(f), switched to its tight upper bound below -6, blended on [-6,-5] (lik.py:341-352)."""
        f = np.asarray(f, dtype=float)
        out = np.zeros_like(f)
        ok = f > -5
        out[ok] = (np.exp(-f[ok] ** 2 / 2) / np.sqrt(2 * np.pi)) / p[ok]
        far = f < -6
        out[far] = np.sqrt(f[far] ** 2 / 4 + 1) - f[far] / 2
        mid = ~ok & ~far
        t = f[mid]
        lam = -5. - t
        out[mid] = (1 - lam) * (np.exp(-t ** 2 / 2) / np.sqrt(2 * np.pi)) / p[mid] + lam * (np.sqrt(t ** 2 / 4 + 1) - t / 2)
        return out

    def cumGauss(self, y=None, f=None, nargout=1):
        yf = f if y is None else y * f
        p = (1. + _erf(yf / np.sqrt(2.))) / 2.
        return (p, self._logphi(yf, p)) if nargout > 1 else p

    def evaluate(self, y=None, mu=None, s2=None, inffunc=None, der=None, nargout=1):
        from . import inf
        if y is not None:
            y = np.sign(y)
            y = np.where(y == 0, 1.0, y)
        else:
            y = 1
        if inffunc is None:                                   # prediction mode (lik.py:251-269)
            y = y * np.ones_like(mu)
            if s2 is not None and np.linalg.norm(s2) > 0:
                lp = self.evaluate(y, mu, s2, inf.EP())
                p = np.exp(lp)
            else:
                p, lp = self.cumGauss(y, mu, 2)
            return _take((lp, 2 * p - 1, 4 * p * (1 - p)), nargout)
        if isinstance(inffunc, inf.Laplace):                  # lik.py:274-293
            if der is not None:
                return []
            f = mu
            yf = y * f
            p, lp = self.cumGauss(y, f, 2)
            if nargout <= 1:
                return lp
            n_p = self._ratio(yf, p)                          # N / Phi from Phi itself (the EP mode passes exp(log Phi))
            dlp = y * n_p
            d2lp = -n_p ** 2 - yf * n_p
            d3lp = 2 * y * n_p ** 3 + 3 * f * n_p ** 2 + y * (f ** 2 - 1) * n_p
            return _take((lp, dlp, d2lp, d3lp), nargout)
        if isinstance(inffunc, inf.EP):                       # lik.py:295-313
            if der is not None:
                return []
            z = mu / np.sqrt(1 + s2)
            lZ = self.cumGauss(y, z, 2)[1]
            if nargout <= 1:
                return lZ
            z = z * y
            n_p = self._ratio(z, np.exp(lZ))
            dlZ = y * n_p / np.sqrt(1. + s2)
            d2lZ = -n_p * (z + n_p) / (1. + s2)
            return _take((lZ, dlZ, d2lZ), nargout)
        raise Exception("Incorrect inference in lik.Erf\n")


class Laplace(Likelihood):
    """Laplacian likelihood for robust regression, p(y | f) = exp(-|y - f| / b) / (2 b) with b = sn / sqrt(2);
    hyp = [log_sigma].  Inference: EP only (GPR.useLikelihood("Laplace"), inf.EP; the site moments run on the device,
    csrc/laplace_lik.h).  The EP mode here is the same arithmetic on the host, vectorised, for prediction and the tests.

    Deviations from the reference, deliberately:
      - "idlik" (1e3 sn < sqrt(s2), value mode): the reference indexes the single array returned by lik.Gauss in prediction
        mode and raises IndexError; here lik.Gauss's EP moments with the Laplacian's variance sn^2, log N(y | mu, s2 + sn^2)
        and its derivatives in mu (the delta-peak limit with s2 alone would make EP's site precision infinite).
      - "idgau" (1e3 sqrt(s2) < sn): the reference calls Laplace(log_hyp=...) and raises TypeError; here the Laplace density
        at mu (lZ, dlZ, d2lZ = lp, dlp, 0) and, for the hyper-parameter derivative, the Laplace-mode lp_dhyp.
      - value mode with nargout >= 2 is elementwise; the reference takes the first element's dlZ for every element
        (_expABz_expAx returns y[0]) and raises for nargout = 3 on vectors.
      - Laplace mode: lp = -|y - f| / b - log(2 b); the reference returns +|y - f| / b - log(2 b).  inf.Laplace does not
        accept this likelihood, as in the reference ("ONLY works with EP")."""

    def __init__(self, log_sigma=np.log(0.1)):
        self.hyp = [log_sigma]

    @staticmethod
    def _logphi(z):
        """log Phi(z), asymptotics below -6.2, logistic blend on [-6.2, -5.5] (lik.py:546-559)."""
        z = np.asarray(z, dtype=float)
        with np.errstate(all="ignore"):
            p = np.log(0.5 * (1. + _erf(z / np.sqrt(2.))))
            asym = -0.5 * (np.log(np.pi) + z ** 2) - np.log(np.sqrt(2. + 0.5 * (z ** 2)) - z / np.sqrt(2))
            lam = 1. / (1. + np.exp(25. * (0.5 - (z - (-6.2)) / ((-5.5) - (-6.2)))))
            return np.where(z > -5.5, p, np.where(z < -6.2, asym, (1 - lam) * asym + lam * p))

    @staticmethod
    def _lerfc(t):
        """log erfc(t), the tight bound above 25, a logistic blend on [20, 25] (lik.py:519-531)."""
        t = np.asarray(t, dtype=float)
        with np.errstate(all="ignore"):
            safe = np.log(_erfc(t))
            bound = np.log(2 / np.sqrt(np.pi)) - t ** 2 - np.log(t + np.sqrt(t ** 2 + 4 / np.pi))
            lam = 1 / (1 + np.exp(12 * (0.5 - (t - 20) / (25 - 20))))
            return np.where(t < 20, safe, np.where(t > 25, bound, lam * bound + (1 - lam) * safe))

    @staticmethod
    def _expABz_expAx(a1, a2, b1, b2):
        mx = np.maximum(a1, a2)
        e1, e2 = np.exp(a1 - mx), np.exp(a2 - mx)
        return (e1 * b1 + e2 * b2) / (e1 + e2)

    def _regimes(self, y, mu, s2):
        sn = np.exp(self.hyp[0])
        y, mu, s2 = np.broadcast_arrays(np.asarray(y, dtype=float), np.asarray(mu, dtype=float), np.asarray(s2, dtype=float))
        with np.errstate(invalid="ignore"):
            idlik = (1e3 * sn) < np.sqrt(s2)
            idgau = (1e3 * np.sqrt(s2)) < sn
        return sn, y, mu, s2, idlik, idgau

    def _ep_value(self, y, mu, s2):
        """lZ, dlZ, d2lZ elementwise (lik.py:450-487)."""
        sn, y, mu, s2, idlik, idgau = self._regimes(y, mu, s2)
        b = sn / np.sqrt(2)
        with np.errstate(all="ignore"):
            tvar = s2 / (sn ** 2 + 1e-16)
            tmu = (mu - y) / (sn + 1e-16)
            zp = (tmu + np.sqrt(2) * tvar) / np.sqrt(tvar)
            zm = (tmu - np.sqrt(2) * tvar) / np.sqrt(tvar)
            lpp, lpm = self._logphi(-zp), self._logphi(zm)
            ap = lpp + np.sqrt(2) * tmu
            am = lpm - np.sqrt(2) * tmu
            mx = np.maximum(ap, am)
            lZ = np.log(np.exp(ap - mx) + np.exp(am - mx)) + mx + tvar - np.log(sn * np.sqrt(2.))
            lqp = -0.5 * zp ** 2 - 0.5 * np.log(2 * np.pi) - lpp
            lqm = -0.5 * zm ** 2 - 0.5 * np.log(2 * np.pi) - lpm
            dap = -np.exp(lqp - 0.5 * np.log(s2)) + np.sqrt(2) / sn
            dam = np.exp(lqm - 0.5 * np.log(s2)) - np.sqrt(2) / sn
            dlZ = self._expABz_expAx(ap, am, dap, dam)
            a = np.sqrt(8.) / sn / np.sqrt(s2)
            bp = 2. / sn ** 2 - (a - zp / s2) * np.exp(lqp)
            bm = 2. / sn ** 2 - (a + zm / s2) * np.exp(lqm)
            d2lZ = self._expABz_expAx(ap, am, bp, bm) - dlZ ** 2
            r = y - mu
            v = sn * sn + s2
            lZ = np.where(idlik, -r * r / v / 2. - np.log(2. * np.pi * v) / 2., np.where(idgau, -np.abs(r) / b - np.log(2. * b), lZ))
            dlZ = np.where(idlik, r / v, np.where(idgau, np.sign(r) / b, dlZ))
            d2lZ = np.where(idlik, -1. / v, np.where(idgau, 0.0, d2lZ))
        return lZ, dlZ, d2lZ

    def _ep_dhyp(self, y, mu, s2):
        """d lZ / d log sn elementwise (lik.py:488-512)."""
        sn, y, mu, s2, idlik, idgau = self._regimes(y, mu, s2)
        with np.errstate(all="ignore"):
            tmu = (mu - y) / (sn + 1e-16)
            tvar = s2 / (sn ** 2 + 1e-16)
            zp = (tvar + tmu / np.sqrt(2)) / np.sqrt(tvar)
            vp = tvar + np.sqrt(2) * tmu
            zm = (tvar - tmu / np.sqrt(2)) / np.sqrt(tvar)
            vm = tvar - np.sqrt(2) * tmu
            dzp = (-s2 / sn + tmu * sn / np.sqrt(2)) / np.sqrt(s2)
            dvp = -2 * tvar - np.sqrt(2) * tmu
            dzm = (-s2 / sn - tmu * sn / np.sqrt(2)) / np.sqrt(s2)
            dvm = -2 * tvar + np.sqrt(2) * tmu
            lezp, lezm = self._lerfc(zp), self._lerfc(zm)
            vmax = np.maximum(vp + lezp, vm + lezm)
            ep = np.exp(vp + lezp - vmax)
            em = np.exp(vm + lezm - vmax)
            dap = ep * (dvp - 2 / np.sqrt(np.pi) * np.exp(-zp ** 2 - lezp) * dzp)
            dam = em * (dvm - 2 / np.sqrt(np.pi) * np.exp(-zm ** 2 - lezm) * dzm)
            out = (dap + dam) / (ep + em) - 1
            out = np.where(idlik, 0.0, np.where(idgau, np.abs(y - mu) / (sn / np.sqrt(2)) - 1, out))
        return out

    def evaluate(self, y=None, mu=None, s2=None, inffunc=None, der=None, nargout=1):
        from . import inf
        sn = np.exp(self.hyp[0])
        b = sn / np.sqrt(2)
        if y is None:
            y = np.zeros_like(mu)
        if inffunc is None:                                   # prediction mode (lik.py:386-405)
            if s2 is not None and np.linalg.norm(s2) > 0:
                lp = self.evaluate(y, mu, s2, inf.EP())
            else:
                lp = -np.abs(y - mu) / b - np.log(2 * b)
                s2 = np.zeros_like(s2) if s2 is not None else 0.0
            return _take((lp, mu, s2 + sn ** 2), nargout)
        if isinstance(inffunc, inf.EP):                       # lik.py:432-512
            if der is None:
                return _take(self._ep_value(y, mu, s2), nargout)
            return self._ep_dhyp(y, mu, s2)
        if isinstance(inffunc, inf.Laplace):                  # lik.py:407-431 (lp with the sign of a log-density)
            r = y - mu
            if der is None:
                return _take((-np.abs(r) / b - np.log(2 * b), np.sign(r) / b, np.zeros_like(r), np.zeros_like(r)), nargout)
            return np.abs(r) / b - 1, np.sign(mu - y) / b, np.zeros(np.shape(mu))
        raise Exception("Incorrect inference in lik.Laplace\n")
