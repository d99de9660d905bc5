"""Model facade (reference: pyGPs/Core/gp.py -- GP :62-527, GPR :533-635, GPC :641-732, GPMC :738-932, FITC :934-1235).

Same public surface for the pieces that call the hot path: ``setData``, ``setPrior``, ``setNoise``,
``setOptimizer``, ``optimize``, ``getPosterior``, ``predict``, ``predict_with_posterior`` and the
result attributes ``nlZ, dnlZ, posterior, ym, ys2, fm, fs2, lp``; ``GPMC`` is the one-vs-one multi-class wrapper.
Plotting is out of scope.
"""
import logging
from copy import deepcopy

import numpy as np

from . import _lib, conf, cov, inf, lik, mean, opt


def _col(a):
    a = np.asarray(a)
    return a.reshape(a.shape[0], 1) if a.ndim == 1 else a


class GP(object):
    """Base class for GP models."""

    def __init__(self):
        super(GP, self).__init__()
        self.usingDefaultMean = True
        self.meanfunc = None
        self.covfunc = None
        self.likfunc = None
        self.inffunc = None
        self.optimizer = None
        self.nlZ = None
        self.dnlZ = None
        self.posterior = None
        self.x = None
        self.y = None
        self.xs = None
        self.ys = None
        self.ym = None
        self.ys2 = None
        self.fm = None
        self.fs2 = None
        self.lp = None
        self.logger = logging.getLogger(__name__)

    def __repr__(self):
        return str(type(self)) + ": model.nlZ, model.dnlZ, model.posterior, model.{mean,cov,lik}func.hyp, model.ym/ys2/fm/fs2/lp"

    # ---- data / prior -------------------------------------------------------------------------------
    def setData(self, x, y):
        """Set training inputs (n,D) and targets (n,1); 1-d arrays are reshaped.  While the default
        mean is in use it is replaced by Const(mean(y))  (Core/gp.py:133-156)."""
        assert x.shape[0] == y.shape[0], "number of inputs and labels does not match"
        self.x = _col(x)
        self.y = _col(y)
        if self.usingDefaultMean:
            self.meanfunc = mean.Const(np.mean(y))

    def setPrior(self, mean=None, kernel=None):
        from . import mean as _mean
        if mean is not None:
            assert isinstance(mean, _mean.Mean), "mean function is not an instance of pygps_amd.mean.Mean"
            self.meanfunc = mean
            self.usingDefaultMean = False
        if kernel is not None:
            assert isinstance(kernel, cov.Kernel), "cov function is not an instance of pygps_amd.cov.Kernel"
            self.covfunc = kernel
            if type(kernel) is cov.Pre:                    # a precomputed matrix alone keeps the model's zero mean (Core/gp.py:221-222)
                self.usingDefaultMean = False

    def setOptimizer(self, method, num_restarts=None, min_threshold=None, meanRange=None, covRange=None, likRange=None):
        conf_ = None
        if (num_restarts is not None) or (min_threshold is not None):
            conf_ = conf.random_init_conf(self.meanfunc, self.covfunc, self.likfunc)
            conf_.num_restarts = num_restarts
            conf_.min_threshold = min_threshold
            if meanRange is not None:
                conf_.meanRange = meanRange
            if covRange is not None:
                conf_.covRange = covRange
            if likRange is not None:
                conf_.likRange = likRange
        if method == "Minimize":
            self.optimizer = opt.Minimize(self, conf_)
        elif method == "ShardedMinimize":
            self.optimizer = opt.ShardedMinimize(self, conf_)
        else:
            raise Exception("Optimization method is not set correctly in setOptimizer")

    # ---- training -----------------------------------------------------------------------------------
    def _take_xy(self, x, y):
        if x is not None and y is not None:
            assert x.shape[0] == y.shape[0], "number of inputs and labels does not match"
        if x is not None:
            self.x = _col(x)
        if y is not None:
            self.y = _col(y)
        if self.usingDefaultMean and self.meanfunc is None:
            self.meanfunc = mean.Const(np.mean(y))

    def optimize(self, x=None, y=None, numIterations=40):
        """Learn the hyper-parameters; then refresh the posterior (Core/gp.py:251-285)."""
        self._take_xy(x, y)
        optimalHyp, optimalNlZ = self.optimizer.findMin(self.x, self.y, numIters=numIterations)
        self.nlZ = optimalNlZ
        self.optimizer._apply_in_objects(optimalHyp)
        self.getPosterior()

    def getPosterior(self, x=None, y=None, der=True):
        """nlZ, dnlZ, post = getPosterior(x, y) ; nlZ, post = getPosterior(x, y, der=False)
        (Core/gp.py:289-345)."""
        self._take_xy(x, y)
        if isinstance(self.likfunc, lik.Erf):
            labels = np.unique(np.asarray(self.y))
            if np.any((labels != 1) & (labels != -1)):
                raise Exception("You attempt classification using labels different from {+1,-1}")
        if not der:
            post, nlZ = self.inffunc.evaluate(self.meanfunc, self.covfunc, self.likfunc, self.x, self.y, 2)
            self.nlZ = nlZ
            self.posterior = deepcopy(post)
            return nlZ, post
        post, nlZ, dnlZ = self.inffunc.evaluate(self.meanfunc, self.covfunc, self.likfunc, self.x, self.y, 3)
        self.nlZ = nlZ
        self.dnlZ = deepcopy(dnlZ)
        self.posterior = deepcopy(post)
        return nlZ, dnlZ, post

    # ---- prediction ---------------------------------------------------------------------------------
    def _latent(self, post, xs):
        """fmu, fs2 for the (alpha, sW, L) parametrisation, on the device (Core/gp.py:395-417)."""
        L = post.L
        fitc = getattr(post, "fitc", None)
        if fitc is not None:                               # dense-L parametrisation of FITC (Core/gp.py:404-417)
            xs = _lib.f64(xs)
            ns = xs.shape[0]
            ms = _lib.f64(self.meanfunc.getMean(xs)).reshape(ns)
            fmu = np.empty(ns)
            fs2 = np.empty(ns)
            _lib.check(_lib.load().pgp_fitc_predict(fitc.ctx, fitc.handle, _lib.ptr(xs), ns, _lib.ptr(ms), _lib.ptr(fmu),
                                                    _lib.ptr(fs2)), "pgp_fitc_predict")
            return fmu.reshape(ns, 1), fs2.reshape(ns, 1)
        if type(L).__name__ == "DistributedFactor":            # a sharded fit: collective predict on the distributed posterior
            xs = _lib.f64(xs)
            return L.predict(xs, self.meanfunc.getMean(xs))
        if not isinstance(L, inf.DeviceFactor):
            raise NotImplementedError("pygps_amd: predict needs a posterior produced by pygps_amd inference "
                                      "(device-resident factor); there is no CPU fallback")
        xs = _lib.f64(xs)
        ns = xs.shape[0]
        ms = _lib.f64(self.meanfunc.getMean(xs)).reshape(ns)
        fmu = np.empty(ns)
        fs2 = np.empty(ns)
        if getattr(L, "dense", False):
            # a covariance function that is not a device program (inf.Exact._evaluate_dense): the cross-covariance block is
            # built by getCovMatrix and handed in; solve and reductions on the device (pgp_predict_dense)
            Ks = _lib.f64(self.covfunc.getCovMatrix(x=self.x, z=xs, mode="cross"))
            kss = _lib.f64(self.covfunc.getCovMatrix(z=xs, mode="self_test")).reshape(ns)
            _lib.check(_lib.load().pgp_predict_dense(L.ctx, L.handle, _lib.ptr(Ks), ns, _lib.ptr(kss), _lib.ptr(ms), _lib.ptr(fmu),
                                                     _lib.ptr(fs2)), "pgp_predict_dense")
            return fmu.reshape(ns, 1), fs2.reshape(ns, 1)
        for leaf in self.covfunc._pre_leaves():            # cov.Pre: the M1 the cross block is read from must be THIS model's,
            leaf._check_train(self.x)                      # whatever the context held last (another model may have fitted since)
            leaf._check_test(xs)
            leaf._bind_pre(L.ctx, test=True)
        rc = _lib.load().pgp_predict(L.ctx, L.handle, _lib.ptr(xs), ns, _lib.ptr(ms), _lib.ptr(fmu), _lib.ptr(fs2))
        if rc == -99:
            raise NotImplementedError("pygps_amd: the device predict path is not built in this version")
        _lib.check(rc, "pgp_predict")
        return fmu.reshape(ns, 1), fs2.reshape(ns, 1)

    def _predict(self, post, xs, ys):
        xs = _col(xs)
        self.xs = xs
        if ys is not None:
            ys = _col(ys)
            self.ys = ys
        fmu, fs2 = self._latent(post, xs)
        lp, ymu, ys2 = self.likfunc.evaluate(ys, fmu, fs2, None, None, 3)
        self.ym, self.ys2, self.lp, self.fm, self.fs2 = ymu, ys2, lp, fmu, fs2
        return (ymu, ys2, fmu, fs2, None) if ys is None else (ymu, ys2, fmu, fs2, lp)

    def predict(self, xs, ys=None):
        """ym, ys2, fm, fs2, lp = predict(xs[, ys])   (Core/gp.py:349-437)"""
        if self.posterior is None:
            self.getPosterior()
        return self._predict(self.posterior, xs, ys)

    def predict_with_posterior(self, post, xs, ys=None):
        """Same with an explicitly given posterior (Core/gp.py:441-527)."""
        return self._predict(post, xs, ys)

    # ---- the joint posterior: covariances between test points, and draws (no reference counterpart) -----------------
    def _noise_var(self, noise):
        if not noise:
            return 0.0
        if not isinstance(self.likfunc, lik.Gauss):
            raise Exception("noise=True adds the Gaussian noise variance sn2 and exists for lik.Gauss only; this model's "
                            "likelihood is %s" % type(self.likfunc).__name__)
        return float(np.exp(2.0 * self.likfunc.hyp[0]))

    @staticmethod
    def _draws(ns, nsamples, rng, z):
        """The (ns, nsamples) standard normal draws: `z` as given, else from `rng` (a Generator or a seed) on the host."""
        if z is not None:
            z = _lib.f64(z)
            if z.ndim == 1:
                z = np.ascontiguousarray(z.reshape(ns, 1))
            if z.ndim != 2 or z.shape[0] != ns or z.shape[1] < 1:
                raise Exception("z must hold one row of standard normal draws per test point: shape (%d, nsamples)" % ns)
            return z
        if int(nsamples) < 1:
            raise Exception("nsamples must be at least 1")
        if not isinstance(rng, np.random.Generator):
            rng = np.random.default_rng(rng)
        return _lib.f64(rng.standard_normal((ns, int(nsamples))))

    @staticmethod
    def _check_ns(ns):
        if ns < 1 or ns > _lib.JOINT_MAX_POINTS:
            raise Exception("the joint posterior is formed for 1 to %d test points at once; got %d" % (_lib.JOINT_MAX_POINTS, ns))

    @staticmethod
    def _check_joint(rc, what):
        if rc > 0:
            raise np.linalg.LinAlgError("joint covariance not positive definite: first bad pivot %d; pass a larger jitter" % rc)
        # the point count is the fourth argument of pgp_predict_joint, the fifth of pgp_predict_joint_dense, the third of pgp_sample_mvn
        count = {"pgp_predict_joint": -4, "pgp_predict_joint_dense": -5, "pgp_sample_mvn": -3}[what]
        _lib.check(rc, what, {count: "the joint posterior is formed for 1 to %d test points at once" % _lib.JOINT_MAX_POINTS,
                              -8: "draws need z with at least one column",
                              -13: "cov.Pre carries no k(xs, xs): the joint posterior is not defined for it"})

    def _joint(self, post, xs, noise, jitter, z, want_cov, want_chol):
        """fmu (ns, 1), fcov | None, Lc | None, F | None, jitter through the route `predict` takes for this posterior."""
        L = post.L
        if getattr(post, "fitc", None) is not None:
            raise NotImplementedError("pygps_amd: the joint predictive covariance of a FITC posterior is not built")
        if type(L).__name__ == "DistributedFactor":
            raise NotImplementedError("pygps_amd: the joint predictive covariance of a sharded posterior is not built")
        if not isinstance(L, inf.DeviceFactor):
            raise NotImplementedError("pygps_amd: predict_joint needs a posterior produced by pygps_amd inference "
                                      "(device-resident factor); there is no CPU fallback")
        if self.covfunc._pre_leaves():
            raise NotImplementedError("pygps_amd: a tree with a cov.Pre leaf carries no k(xs, xs); its joint posterior is not built")
        xs = _lib.f64(_col(xs))
        ns = xs.shape[0]
        self._check_ns(ns)
        sn2 = self._noise_var(noise)
        ms = _lib.f64(self.meanfunc.getMean(xs)).reshape(ns)
        dense = bool(getattr(L, "dense", False))
        Ks = Kss = None
        if dense:
            Ks = _lib.f64(self.covfunc.getCovMatrix(x=self.x, z=xs, mode="cross"))
            Kss = np.array(self.covfunc.getCovMatrix(x=xs, mode="train"), dtype=np.float64, order="C")
            Kss[np.diag_indices(ns)] = np.asarray(self.covfunc.getCovMatrix(z=xs, mode="self_test"), dtype=np.float64).reshape(ns)
        if jitter is None:
            if noise:
                jitter = 0.0
            else:
                kss = Kss.diagonal() if dense else np.asarray(self.covfunc.getCovMatrix(z=xs, mode="self_test")).reshape(ns)
                jitter = 1e-8 * float(np.mean(kss))
        jitter = float(jitter)
        fmu = np.empty(ns)
        fcov = np.empty((ns, ns)) if want_cov else None
        Lc = np.empty((ns, ns)) if want_chol else None
        F = np.empty((ns, z.shape[1])) if z is not None else None
        nsamp = z.shape[1] if z is not None else 0
        dll = _lib.load()
        if dense:
            rc = dll.pgp_predict_joint_dense(L.ctx, L.handle, _lib.ptr(Ks), _lib.ptr(Kss), ns, _lib.ptr(ms), sn2, jitter, _lib.ptr(z),
                                             nsamp, _lib.ptr(fmu), _lib.ptr(fcov), _lib.ptr(Lc), _lib.ptr(F), None)
            self._check_joint(rc, "pgp_predict_joint_dense")
        else:
            rc = dll.pgp_predict_joint(L.ctx, L.handle, _lib.ptr(xs), ns, _lib.ptr(ms), sn2, jitter, _lib.ptr(z), nsamp,
                                       _lib.ptr(fmu), _lib.ptr(fcov), _lib.ptr(Lc), _lib.ptr(F), None)
            self._check_joint(rc, "pgp_predict_joint")
        return fmu.reshape(ns, 1), fcov, Lc, F, jitter

    def predict_joint(self, xs, noise=False):
        """fmu (ns, 1), fcov (ns, ns) = predict_joint(xs): the joint posterior of the latent f at the test points,
        fcov = Kss - V'V with V = L^-1 (sW o Ks), formed on the device.  diag(fcov) is `predict`'s fs2 (clipped at 0 like it, the
        off-diagonal entries untouched) and fcov is exactly symmetric.  noise=True (lik.Gauss only) adds sn2 to the diagonal: the
        covariance of y.  Up to 16384 test points per call.  Exact, EP and Laplace posteriors; FITC, sharded posteriors and trees
        with a cov.Pre leaf raise NotImplementedError."""
        sn2 = self._noise_var(noise)                       # (refuses a likelihood without a noise variance before any device work)
        if self.posterior is None:
            self.getPosterior()
        fmu, fcov, _, _, _ = self._joint(self.posterior, xs, False, 0.0, None, True, False)
        if sn2:
            fcov[np.diag_indices(fcov.shape[0])] += sn2
        return fmu, fcov

    def sample_posterior(self, xs, nsamples=1, rng=None, z=None, noise=False, jitter=None, return_chol=False):
        """F (ns, nsamples) = sample_posterior(xs, nsamples): draws F = fmu 1' + Lc z from the joint posterior at xs, with
        Lc Lc' = fcov + (noise + jitter) I factorised on the device.  z (ns, nsamples): the standard normal draws to use; otherwise
        they come from `rng` (an np.random.Generator or a seed; default np.random.default_rng()) on the host.  noise=True
        (lik.Gauss only) draws y instead of the latent f.  jitter=None means 1e-8 * mean(diag Kss) for latent draws -- the
        convention of other fp64 GP libraries -- and 0 with noise=True; jitter=0.0 is allowed.  A covariance that is not
        numerically positive definite raises numpy.linalg.LinAlgError naming the pivot.  return_chol=True returns
        (F, Lc, fmu, jitter) with the lower factor Lc, exact zeros above its diagonal."""
        self._noise_var(noise)
        if self.posterior is None:
            self.getPosterior()
        xs = _col(xs)
        z = self._draws(xs.shape[0], nsamples, rng, z)
        fmu, _, Lc, F, jitter = self._joint(self.posterior, xs, noise, jitter, z, False, return_chol)
        return (F, Lc, fmu, jitter) if return_chol else F

    def sample_prior(self, xs, nsamples=1, rng=None, z=None, jitter=None, return_chol=False):
        """F (ns, nsamples) = sample_prior(xs, nsamples): draws m(xs) 1' + Lc z from the prior, Lc Lc' = k(xs, xs) + jitter I
        ('train' mode) factorised on the device; needs no data.  z, rng, jitter, return_chol as `sample_posterior`."""
        xs = _lib.f64(_col(xs))
        ns = xs.shape[0]
        self._check_ns(ns)
        z = self._draws(ns, nsamples, rng, z)
        K = _lib.f64(self.covfunc.getCovMatrix(x=xs, mode="train"))
        ms = _lib.f64(self.meanfunc.getMean(xs)).reshape(ns)
        if jitter is None:
            jitter = 1e-8 * float(np.mean(K.diagonal()))
        jitter = float(jitter)
        F = np.empty((ns, z.shape[1]))
        Lc = np.empty((ns, ns)) if return_chol else None
        rc = _lib.load().pgp_sample_mvn(_lib.ctx(), _lib.ptr(K), ns, _lib.ptr(ms), jitter, _lib.ptr(z), z.shape[1], _lib.ptr(Lc),
                                        _lib.ptr(F))
        self._check_joint(rc, "pgp_sample_mvn")
        return (F, Lc, ms.reshape(ns, 1), jitter) if return_chol else F


class GPR(GP):
    """Gaussian-process regression: Zero mean, RBF, Gauss likelihood, Exact inference, Minimize."""

    def __init__(self):
        super(GPR, self).__init__()
        self.meanfunc = mean.Zero()
        self.covfunc = cov.RBF()
        self.likfunc = lik.Gauss()
        self.inffunc = inf.Exact()
        self.optimizer = opt.Minimize(self)

    def setNoise(self, log_sigma):
        self.likfunc = lik.Gauss(log_sigma)

    def useInference(self, newInf):
        """'Laplace' or 'EP' (Core/gp.py:611-622), or 'LOO': the leave-one-out log pseudo-likelihood as the objective of
        optimize() / getPosterior() (inf.LOO; no reference counterpart)."""
        if newInf == "Laplace":
            self.inffunc = inf.Laplace()
        elif newInf == "EP":
            self.inffunc = inf.EP()
        elif newInf == "LOO":
            self.inffunc = inf.LOO()
        else:
            raise Exception('Possible inf values are "Laplace", "EP", "LOO".')

    def predict_loo(self, x=None, y=None):
        """ymu, ys2, fmu, fs2, lp = predict_loo([x, y]): the leave-one-out predictive at every training point, each (n, 1) as
        predict returns them.  Point i is predicted from the other n - 1 with the model's current hyper-parameters, in closed
        form from one factorisation (inf.LOO; the value-only device call: nothing O(n^3) beyond the factorisation).  ymu / ys2
        are for the observation y_i (noise included), fmu = ymu, fs2 = ys2 - sn2, lp = log N(y_i | ymu_i, ys2_i).  Works
        whatever inference the model uses, provided that is Exact or LOO on lik.Gauss on one GPU; EP / Laplace cavity LOO,
        FITC and sharded fits are out of scope."""
        self._take_xy(x, y)
        if not isinstance(self.inffunc, inf.Exact) or not isinstance(self.likfunc, lik.Gauss):
            raise Exception("predict_loo needs Exact or LOO inference with Gaussian likelihood")
        loo = inf.LOO()
        loo.device = self.inffunc.device
        if getattr(self.inffunc, "sharded", False):
            raise NotImplementedError("pygps_amd: leave-one-out inference runs on one GPU (no sharded fit)")
        loo.evaluate(self.meanfunc, self.covfunc, self.likfunc, self.x, self.y, 2)
        mu, s2, lp = loo.last_loo
        sn2 = float(np.exp(2.0 * self.likfunc.hyp[0]))
        return mu, s2, mu.copy(), s2 - sn2, lp

    def useLikelihood(self, newLik):
        """'Laplace': lik.Laplace with EP inference (Core/gp.py:624-635)."""
        if newLik == "Laplace":
            self.likfunc = lik.Laplace()
            self.inffunc = inf.EP()
        else:
            raise Exception('Possible lik values are "Laplace".')


class GPC(GP):
    """Binary GP classification: Zero mean, RBF, Erf likelihood, EP inference, Minimize."""

    def __init__(self):
        super(GPC, self).__init__()
        self.meanfunc = mean.Zero()
        self.covfunc = cov.RBF()
        self.likfunc = lik.Erf()
        self.inffunc = inf.EP()
        self.optimizer = opt.Minimize(self)

    def useInference(self, newInf):
        """'Laplace' or 'EP' (Core/gp.py:708-717; the reference's GPC also accepts only these)."""
        if newInf == "Laplace":
            self.inffunc = inf.Laplace()
        elif newInf == "EP":
            self.inffunc = inf.EP()
        else:
            raise Exception('Possible inf values are "Laplace", "EP".')


class GP_FITC(GP):
    """Base class of the FITC models (Core/gp.py:934-1008)."""

    def __init__(self):
        super(GP_FITC, self).__init__()
        self.u = None                                      # inducing points

    def setData(self, x, y, value_per_axis=5):
        """Training data; without user-given inducing points a regular grid with ``value_per_axis`` values per input
        dimension is used (Core/gp.py:944-983)."""
        import itertools
        assert x.shape[0] == y.shape[0], "number of inputs and labels does not match"
        self.x = _col(x)
        self.y = _col(y)
        if self.usingDefaultMean:
            self.meanfunc = mean.Const(np.mean(y))
        axes = [np.linspace(np.min(self.x[:, k]), np.max(self.x[:, k]), value_per_axis) for k in range(self.x.shape[1])]
        if self.u is None:
            self.u = np.array(list(itertools.product(*axes)))
            self.covfunc = self.covfunc.fitc(self.u)

    def learnInducing(self, flag=True):
        """Treat the inducing inputs as parameters: getPosterior also returns dnlZ.xu and optimize() moves them together with the
        hyper-parameters (Snelson & Ghahramani's pseudo-inputs).  Call after the covariance function is set (setData / setPrior);
        a later setPrior(kernel=...) builds a new FITC covariance and clears the flag."""
        if not isinstance(self.covfunc, cov.FITCOfKernel):
            raise Exception("To learn the inducing points, please call setData() or setPrior(kernel, inducing_points) first!")
        self.covfunc.learn_inducing = bool(flag)

    def setPrior(self, mean=None, kernel=None, inducing_points=None):
        if kernel is not None:
            if inducing_points is not None:
                self.covfunc = kernel.fitc(inducing_points)
                self.u = inducing_points
            elif self.u is not None:
                self.covfunc = kernel.fitc(self.u)
            else:
                raise Exception("To use default inducing points, please call setData() first!")
        if mean is not None:
            self.meanfunc = mean
            self.usingDefaultMean = False


class GPR_FITC(GP_FITC):
    """Sparse GP regression with the FITC approximation (Core/gp.py:1010-1100)."""

    def __init__(self):
        super(GPR_FITC, self).__init__()
        self.meanfunc = mean.Zero()
        self.covfunc = cov.RBF()
        self.likfunc = lik.Gauss()
        self.inffunc = inf.FITC_Exact()
        self.optimizer = opt.Minimize(self)
        self.u = None

    def setNoise(self, log_sigma):
        self.likfunc = lik.Gauss(log_sigma)

    def useInference(self, newInf):
        raise Exception('FITC_Laplace / FITC_EP are out of scope of pygps_amd.')

    def useLikelihood(self, newLik):
        """'Laplace': lik.Laplace with FITC_EP inference (Core/gp.py:1104-1114)."""
        if newLik == "Laplace":
            self.likfunc = lik.Laplace()
            self.inffunc = inf.FITC_EP()
        else:
            raise Exception('Possible lik values are "Laplace".')


class GPC_FITC(GP_FITC):
    """Sparse binary GP classification with the FITC approximation (Core/gp.py:1117-1235): Zero mean, RBF, Erf
    likelihood, FITC_EP inference, Minimize."""

    def __init__(self):
        super(GPC_FITC, self).__init__()
        self.meanfunc = mean.Zero()
        self.covfunc = cov.RBF()
        self.likfunc = lik.Erf()
        self.inffunc = inf.FITC_EP()
        self.optimizer = opt.Minimize(self)
        self.u = None

    def useInference(self, newInf):
        """The reference accepts only 'Laplace' here (Core/gp.py:1192-1202), i.e. FITC_Laplace, which is not built."""
        if newInf == "Laplace":
            raise NotImplementedError("pygps_amd: FITC_Laplace (GPC_FITC.useInference('Laplace')) is not implemented")
        raise Exception('Possible inf values are "Laplace".')


class GPMC(object):
    """One-vs-one multi-class classification (Core/gp.py:738-932): a binary GPC with lik.Erf for each of the
    n_class (n_class - 1) / 2 pairs of classes, combined by votes.  Zero mean, RBF, EP inference.

    ``fitAndPredict`` / ``optimizeAndPredict`` return the (ns, n_class) matrix of normalised votes.  Two routes produce it
    (``last_route`` says which one the last call took):

      - "pairs": the reference's loop, a ``GPC`` per pair on the pair's rows (getPosterior or optimize, then predict), votes
        added on the host.  Always for ``optimizeAndPredict`` (the hyper-parameters differ per pair), for ``fitAndPredict``
        with ``GPMC(n_class, shared_kernel=False)`` and whenever the shared route cannot run.
      - "shared" (``fitAndPredict`` only): all pairs share mean, kernel and hyper-parameters, so K(x_all, x_all) and
        K(x_all, xs) are assembled ONCE on the device and every pair works on a gathered submatrix (pgp_gpmc_fit_predict,
        csrc/gpmc.hip).  Taken when the kernel is a device functor or device program and the shared matrices fit into
        ``shared_memory_limit`` bytes (default: the quarter of the device memory that ``DeviceFactor.reserve`` guards).

    ``pair_nlZ`` / ``pair_iters`` (EP sweeps or Newton steps), dicts keyed (i, j), are set by both routes; ``pair_hyp`` (the
    optimised covariance hyper-parameters per pair) by ``optimizeAndPredict``.

    Deviations from the reference, deliberately:
      - ``useInference("Laplace")`` takes effect for every pair.  The reference stores ``self.inffunc`` but its loops test
        ``self.newInf``, which nothing ever sets, so the call is silently ignored there (equivalent to never making it).
      - a class in range(n_class) without a training point raises a plain Exception naming the class before any device work;
        the reference goes on and fails later inside a pair."""

    def __init__(self, n_class, shared_kernel=True):
        self.meanfunc = mean.Zero()                # default prior mean
        self.covfunc = cov.RBF()                   # default prior covariance
        self.n_class = n_class                     # number of different classes
        self.x_all = None
        self.y_all = None
        self.newInf = None                         # new inference? -> call useInference
        self.newLik = None                         # new likelihood? -> call useLikelihood
        self.newPrior = False
        self.shared_kernel = bool(shared_kernel)
        self.shared_memory_limit = None            # bytes the shared route may take; None: a quarter of the device memory
        self.device = None
        self.pair_nlZ = {}
        self.pair_iters = {}
        self.pair_hyp = {}
        self.last_route = None

    def setPrior(self, mean=None, kernel=None):
        from . import mean as _mean
        if mean is not None:
            assert isinstance(mean, _mean.Mean), "mean function is not an instance of pygps_amd.mean.Mean"
            self.meanfunc = mean
            self.usingDefaultMean = False
        if kernel is not None:
            assert isinstance(kernel, cov.Kernel), "cov function is not an instance of pygps_amd.cov.Kernel"
            self.covfunc = kernel
        self.newPrior = True

    def useInference(self, newInf):
        """'Laplace' (Core/gp.py:776-785); unlike the reference's, this call takes effect (class docstring)."""
        if newInf == "Laplace":
            self.inffunc = inf.Laplace()
            self.newInf = "Laplace"
        else:
            raise Exception('Possible inf values are "Laplace".')

    def useLikelihood(self, newLik):
        if newLik == "Logistic":
            raise Exception("Logistic likelihood is currently not implemented.")
        else:
            raise Exception('Possible lik values are "Logistic".')

    def setData(self, x, y):
        assert x.shape[0] == y.shape[0], "number of inputs and labels does not match"
        if x.ndim == 1:
            x = np.reshape(x, (x.shape[0], 1))
        if y.ndim == 1:
            y = np.reshape(y, (y.shape[0], 1))
        self.x_all = x
        self.y_all = y

    # ---- the pairs ----------------------------------------------------------------------------------------
    def pairs(self):
        """The pairs in the order they are processed: (0,1), (0,2), ..., (n_class-2, n_class-1)."""
        return [(i, j) for i in range(self.n_class) for j in range(i + 1, self.n_class)]

    def _pair_index(self, i, j):
        t = np.asarray(self.y_all).reshape(-1)
        ci = np.flatnonzero(t == i)
        cj = np.flatnonzero(t == j)
        return np.concatenate([ci, cj]), len(ci)

    def createBinaryClass(self, i, j):
        """x, y of the rows of class i (in data order, labelled +1) followed by those of class j (-1)  (Core/gp.py:905-928)."""
        idx, n1 = self._pair_index(i, j)
        y = np.concatenate((np.ones((1, n1)), -np.ones((1, len(idx) - n1))), axis=1).T
        return self.x_all[idx, :], y

    def _check_classes(self):
        t = np.asarray(self.y_all).reshape(-1)
        for k in range(self.n_class):
            if not np.any(t == k):
                raise Exception("GPMC: class %d has no training point" % k)

    def _prior(self):
        """Mean and kernel every pair's GPC starts with: the user's objects after setPrior, else GPC's defaults."""
        if self.newPrior:
            return self.meanfunc, self.covfunc
        return mean.Zero(), cov.RBF()

    @staticmethod
    def add_votes(votes, ym, i, j):
        """gp.py:854-861 for one pair: ym + 1 into column i, 2 - (ym + 1) into column j."""
        a = np.asarray(ym, dtype=float).reshape(-1) + 1
        votes[:, i] += a
        votes[:, j] += 2 - a
        return votes

    def _new_pair_model(self):
        model = GPC()
        if self.newPrior:
            model.setPrior(mean=self.meanfunc, kernel=self.covfunc)
        if self.newInf:
            model.useInference(self.newInf)
        if self.device is not None:
            model.inffunc.device = self.device
        return model

    @staticmethod
    def _iters(model):
        return int(model.inffunc.newton_steps if isinstance(model.inffunc, inf.Laplace) else model.inffunc.sweeps)

    def shared_bytes(self, ns):
        """Device bytes of the shared route: K_all, one batch of Ks_all with the largest pair's block of it, the pairs'
        factors and the largest pair's fit scratch."""
        r128 = lambda v: (int(v) + 127) // 128 * 128
        n = self.x_all.shape[0]
        np_ = r128(n)
        t = np.asarray(self.y_all).reshape(-1)
        cnt = [int(np.sum(t == k)) for k in range(self.n_class)]
        sizes = [r128(cnt[i] + cnt[j]) for i, j in self.pairs()]
        nsb = max(128, min(65536, r128(ns), max(16384, (1 << 34) // (8 * np_) // 128 * 128)))      # predict_batch_points
        big = max(sizes)
        return 8 * (np_ * np_ + np_ * nsb + big * nsb + sum((s + 128) * s for s in sizes) + 5 * big * big)

    def choose_route(self, ns, device_bytes=None):
        """"shared" or "pairs" for fitAndPredict on ns test points.  device_bytes: the device's memory (asked of the device
        only when it is needed and not given)."""
        if not self.shared_kernel:
            return "pairs"
        m, k = self._prior()
        if isinstance(k, cov.Kernel) and k._dot_leaves():
            return "pairs"                                # the shared engine predicts with one scalar k(z, z)
        if isinstance(k, cov._Composite):
            if not k._on_device():
                return "pairs"
        elif not isinstance(k, cov.Kernel) or isinstance(k, cov.FITCOfKernel) or getattr(k, "_kind", None) is None:
            return "pairs"
        from . import mean as _mean
        if not isinstance(m, _mean.Mean):
            return "pairs"
        limit = self.shared_memory_limit
        if limit is None:
            if device_bytes is None:
                dev = _lib.default_device() if self.device is None else self.device
                device_bytes = _lib.device_memory_bytes(dev)
            limit = 0.25 * device_bytes - inf.DeviceFactor.live_bytes
        return "shared" if self.shared_bytes(ns) <= limit else "pairs"

    # ---- the two routes -----------------------------------------------------------------------------------
    def _by_pairs(self, xs, optimize):
        self.last_route = "pairs"
        votes = np.zeros((xs.shape[0], self.n_class))
        for i, j in self.pairs():
            x, y = self.createBinaryClass(i, j)
            model = self._new_pair_model()
            if optimize:
                model.optimize(x, y)
                self.pair_hyp[(i, j)] = [float(v) for v in model.covfunc.hyp]
            else:
                model.getPosterior(x, y)
            self.pair_nlZ[(i, j)] = float(model.nlZ)
            self.pair_iters[(i, j)] = self._iters(model)
            self.add_votes(votes, model.predict(xs)[0], i, j)
        votes /= votes.sum(axis=1)[:, np.newaxis]
        return votes

    def _shared(self, xs):
        import ctypes as C
        self.last_route = "shared"
        dev = _lib.default_device() if self.device is None else self.device
        ctx = _lib.ctx(dev)
        meanfunc, covfunc = self._prior()
        kind, para, flags = covfunc._bind(ctx)
        x = _lib.f64(self.x_all)
        n = x.shape[0]
        xs = _lib.f64(xs)
        ns = xs.shape[0]
        if xs.shape[1] != x.shape[1]:
            raise Exception("GPMC: test inputs have %d columns, training inputs %d" % (xs.shape[1], x.shape[1]))
        labels = np.ascontiguousarray(np.asarray(self.y_all).reshape(n), dtype=np.int32)
        inf._Resident.ensure(x, labels.astype(np.float64), dev)
        m_all = _lib.f64(meanfunc.getMean(x)).reshape(n)
        ms = _lib.f64(meanfunc.getMean(xs)).reshape(ns)
        hyp = _lib.f64(np.asarray(covfunc.hyp, dtype=float))
        pairs = self.pairs()
        votes = np.empty((ns, self.n_class))
        nlZ = np.zeros(len(pairs))
        iters = np.zeros(len(pairs), dtype=np.int32)
        bad = np.full(2, -1, dtype=np.int32)
        i32 = C.POINTER(C.c_int32)
        rc = _lib.load().pgp_gpmc_fit_predict(ctx, kind, _lib.ptr(hyp), len(hyp), int(para), int(flags),
                                              1 if self.newInf == "Laplace" else 0, labels.ctypes.data_as(i32), int(self.n_class),
                                              _lib.ptr(m_all), _lib.ptr(xs), ns, _lib.ptr(ms), _lib.ptr(votes), _lib.ptr(nlZ),
                                              iters.ctypes.data_as(i32), bad.ctypes.data_as(i32))
        if rc == _lib.ERR_LAPLACE_WNEG:
            raise NotImplementedError("pygps_amd: Laplace met W < 0 (the reference's LU branch is not restated)")
        _lib.check(rc, "pgp_gpmc_fit_predict" + (" (pair %d, %d)" % (bad[0], bad[1]) if bad[0] >= 0 else ""))
        for k, p in enumerate(pairs):
            self.pair_nlZ[p] = float(nlZ[k])
            self.pair_iters[p] = int(iters[k])
        return votes

    def fitAndPredict(self, xs):
        """Fit every pair at the current hyper-parameters and predict xs (nn, D): the (nn, n_class) matrix of normalised votes,
        row = test point, column = class  (Core/gp.py:829-863)."""
        if xs.ndim == 1:
            xs = np.reshape(xs, (xs.shape[0], 1))
        cov.refuse_pre(self._prior()[1], "GPMC (every pair of classes fits on its own subset of x)")
        self._check_classes()
        self.pair_nlZ, self.pair_iters, self.pair_hyp = {}, {}, {}
        if self.choose_route(xs.shape[0]) == "shared":
            return self._shared(xs)
        return self._by_pairs(xs, optimize=False)

    def optimizeAndPredict(self, xs):
        """Optimise every pair's hyper-parameters, then predict xs  (Core/gp.py:867-901).  With a user prior every pair's GPC
        receives the same kernel and mean objects, so one pair's optimum is the next pair's starting point, as in the
        reference; without one every pair starts from GPC's defaults."""
        if xs.ndim == 1:
            xs = np.reshape(xs, (xs.shape[0], 1))
        cov.refuse_pre(self._prior()[1], "GPMC (every pair of classes fits on its own subset of x)")
        self._check_classes()
        self.pair_nlZ, self.pair_iters, self.pair_hyp = {}, {}, {}
        return self._by_pairs(xs, optimize=True)
