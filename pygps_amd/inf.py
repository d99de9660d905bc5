"""Inference engines on the hot path (reference: pyGPs/Core/inf.py -- postStruct :59-89,
dnlZStruct :93-128, Inference :133-172, Exact :345-384, Laplace :459-564, EP :723-806).

``Exact.evaluate`` keeps the reference's signature and result types but the whole body -- kernel
assembly, Cholesky, solves, nlZ and all hyper-gradients -- is ONE call into the device pipeline
(``pgp_exact_fit``).  x and y stay resident on the GPU between calls (the optimiser only changes
hyp, Core/opt.py:70-75); ``post.L`` is a lazy host view of the device-resident factor so that a fit
is not a PCIe benchmark.  No CPU fallback.
"""
import contextlib
import ctypes as C
import hashlib
import logging
import weakref

import numpy as np

from . import _lib, cov as _cov, lik as _lik

try:                                    # fast content hash for the residency check
    import xxhash

    def _digest(a):
        return xxhash.xxh3_64_intdigest(memoryview(a).cast("B"))
except Exception:                       # pragma: no cover
    def _digest(a):
        return hashlib.blake2b(memoryview(a).cast("B"), digest_size=8).digest()


class postStruct(object):
    """Posterior parametrisation N(m + K alpha, (K^-1 + W)^-1): alpha (n,1), sW (n,1), L (n,n) =
    chol(I + sW sW' o K) as the UPPER factor (Core/inf.py:59-89)."""

    def __init__(self):
        self.alpha = np.array([])
        self.L = np.array([])
        self.sW = np.array([])

    def __repr__(self):
        return ("posterior: to get the parameters of the posterior distribution use:\n"
                "model.posterior.alpha\nmodel.posterior.L\nmodel.posterior.sW\n"
                "See documentation and gpml book chapter 2.3 and chapter 3.4.3 for these parameters.")

    def __str__(self):
        return ("posterior distribution described by alpha, sW and L\n"
                "See documentation and gpml book chapter 2.3 and chapter 3.4.3 for these parameters\n"
                "alpha:\n" + str(self.alpha) + "\nL:\n" + str(np.asarray(self.L)) + "\nsW:\n" + str(self.sW))


class dnlZStruct(object):
    """Partial derivatives of nlZ w.r.t. mean / cov / lik hyper-parameters (Core/inf.py:93-128)."""

    def __init__(self, m, c, l):
        self.mean = [0 for _ in range(len(m.hyp))] if m.hyp is not None else []
        self.cov = [0 for _ in range(len(c.hyp))] if c.hyp is not None else []
        self.lik = [0 for _ in range(len(l.hyp))] if l.hyp is not None else []
        self.xu = None          # (nu, D) d nlZ / d inducing inputs: the FITC fits with FITCOfKernel.learn_inducing

    def __str__(self):
        return ("Derivatives of mean, cov and lik functions:\nmean:" + str(self.mean) + "\ncov:" + str(self.cov)
                + "\nlik:" + str(self.lik))

    def __repr__(self):
        return ("dnlZ: to get the derivatives of mean, cov and lik functions use:\n"
                "model.dnlZ.mean\nmodel.dnlZ.cov\nmodel.dnlZ.lik")

    def accumulateDnlZ(self, other):
        self.mean = [a + b for a, b in zip(self.mean, other.mean)]
        self.cov = [a + b for a, b in zip(self.cov, other.cov)]
        self.lik = [a + b for a, b in zip(self.lik, other.lik)]
        return self


class DeviceFactor(object):
    """``post.L``: the (n,n) upper Cholesky factor R (R'R = I + sW sW' o K), resident on the GPU.

    Behaves like a read-only numpy array -- shape/len/indexing/np.asarray/.T all work and trigger ONE
    device->host copy (2 GiB at n=16384) on first touch; exact zeros below the diagonal, as
    Core/gp.py:393 requires.  ``copy.deepcopy`` shares the handle (the buffer is never rewritten).
    ``predict`` uses the handle directly and never materialises it."""
    ndim = 2
    dtype = np.dtype(np.float64)
    #: True on the factors of the dense path (inf.Exact._evaluate_dense sets it on the instance).  A CLASS attribute so that
    #: `predict`'s test never reaches __getattr__, which forwards unknown names to the host copy (an n x n D2H transfer).
    dense = False
    #: bytes of factor buffers ((n + 128) n doubles each: factor + rhs rows) held by live DeviceFactor objects.
    #: Models sit in reference cycles (model <-> optimizer), so a dropped model frees its factor only when the cyclic
    #: garbage collector runs; `reserve` forces a collection before the device fills up with unreachable factors.
    live_bytes = 0
    # RLock: the finalizer below can run from the cyclic GC on the very thread that is inside `with _live_lock`
    _live_lock = __import__("threading").RLock()

    def __init__(self, handle, n, device, slot=0):
        self._h = handle
        self._n = int(n)
        self._dev = device
        self._slot = slot
        self._host = None
        nbytes = DeviceFactor.nbytes_for(n)
        with DeviceFactor._live_lock:
            DeviceFactor.live_bytes += nbytes
        # the context handle and the entry point are captured NOW: a finalizer may fire (cyclic GC) while this thread
        # holds _lib's module lock inside ctx()/load(), so it must not look either of them up again
        self._ctx = _lib.ctx(device, slot)
        self._fin = weakref.finalize(self, DeviceFactor._release, _lib.load().pgp_factor_free, self._ctx, handle, nbytes)

    @staticmethod
    def nbytes_for(n):
        np_ = (int(n) + 127) // 128 * 128
        return (np_ + 128) * np_ * 8

    @staticmethod
    def reserve(n, device):
        """Called before a fit: collect unreachable models when their factors hold more than a quarter of the HBM."""
        if DeviceFactor.live_bytes + DeviceFactor.nbytes_for(n) > 0.25 * _lib.device_memory_bytes(device):
            import gc
            gc.collect()

    @staticmethod
    def _release(free_fn, ctx_handle, handle, nbytes=0):
        with DeviceFactor._live_lock:
            DeviceFactor.live_bytes -= nbytes
        try:
            free_fn(ctx_handle, handle)     # pgp_factor_free: takes the context's own pool mutex, no Python lock
        except Exception:       # interpreter shutdown
            pass

    @property
    def ctx(self):
        """The context that owns the device buffers of this factor."""
        return self._ctx

    @property
    def handle(self):
        return self._h

    @property
    def shape(self):
        return (self._n, self._n)

    @property
    def size(self):
        return self._n * self._n

    def __len__(self):
        return self._n

    def host(self):
        if self._host is None:
            out = np.empty((self._n, self._n))
            _lib.check(_lib.load().pgp_factor_to_host(self.ctx, self._h, _lib.ptr(out)), "pgp_factor_to_host")
            out.setflags(write=False)
            self._host = out
        return self._host

    def __array__(self, dtype=None, copy=None):
        a = self.host()
        return a if dtype is None else a.astype(dtype)

    def __getitem__(self, idx):
        return self.host()[idx]

    @property
    def T(self):
        return self.host().T

    def __deepcopy__(self, memo):
        return self

    def __copy__(self):
        return self

    def __getattr__(self, name):            # any other ndarray attribute/method
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self.host(), name)

    def __repr__(self):
        return "DeviceFactor(n=%d, on device %d%s)" % (self._n, self._dev, ", materialised" if self._host is not None else "")


class Inference(object):
    """Base class (Core/inf.py:133-172)."""

    def __init__(self):
        self.logger = logging.getLogger(__name__)

    def evaluate(self, meanfunc, covfunc, likfunc, x, y, nargout=1):
        raise NotImplementedError


class _Resident(object):
    """Tracks which (x, y) the device context currently holds."""
    key = {}

    @classmethod
    def ensure(cls, x, y, device):
        k = (x.shape, _digest(x), _digest(y))
        where = (device, _lib.current_slot())
        if cls.key.get(where) != k:
            _lib.check(_lib.load().pgp_set_data(_lib.ctx(device), _lib.ptr(x), x.shape[0], x.shape[1], _lib.ptr(y)),
                       "pgp_set_data")
            cls.key[where] = k

    @classmethod
    def invalidate(cls, device=None):
        for k in [k for k in cls.key if device is None or k[0] == device]:
            cls.key.pop(k, None)


def _device_kernel(covfunc, ctx):
    """(kind, para, flags) of ``covfunc`` on context ``ctx`` (composites register their device program there)."""
    if not isinstance(covfunc, _cov.Kernel):
        raise NotImplementedError("pygps_amd: covfunc must be a pygps_amd.cov.Kernel (got %s); there is no CPU fallback"
                                  % type(covfunc).__name__)
    return covfunc._bind(ctx)


def _dense_route(covfunc):
    """True for covariance functions that are not device programs: K and the derivative matrices come from getCovMatrix /
    getDerMatrix.  Trees over the program limits -- and every tree that holds a cov.Pre with ``device_leaf = False``."""
    return isinstance(covfunc, (_cov._Composite, _cov.Pre)) and not covfunc._on_device()


def _check_pre(covfunc, x):
    """cov.Pre leaves: M2 must be the matrix of these training inputs."""
    if isinstance(covfunc, _cov.Kernel):
        for leaf in covfunc._pre_leaves():
            leaf._check_train(x)


def _mean_inputs(meanfunc, x):
    n = x.shape[0]
    m = _lib.f64(meanfunc.getMean(x)).reshape(n)
    nm = len(meanfunc.hyp) if meanfunc.hyp else 0
    dm = None
    if nm:
        dm = np.empty((nm, n))
        for i in range(nm):
            dm[i] = np.asarray(meanfunc.getDerMatrix(x, i), dtype=float).reshape(n)
    return m, dm, nm


class _Inputs(object):
    """What ``_prepare`` hands an engine: dev, ctx, lib, x (n, D), y (n), m, dm, nm, hyp, dense and -- unless dense -- kind,
    para, flags of the bound kernel."""


def _prepare(device, meanfunc, covfunc, x, y, dense_ok=True, reserve=True, resident=True, inner=False):
    """The inputs every engine prepares, in the order of their side effects: the cov.Pre check, the kernel bound to the
    context (``covfunc.covfunc`` with ``inner``: the FITC engines), room for the factor, (x, y) resident on the device.
    ``dense_ok``: covariance trees that are not device programs take the dense route instead of raising."""
    p = _Inputs()
    p.dev = _lib.default_device() if device is None else device
    kernel = covfunc.covfunc if inner else covfunc
    _check_pre(kernel, x)                           # (a host check: raises before anything reaches the device)
    p.dense = dense_ok and _dense_route(kernel)
    p.lib, p.ctx = _lib.load(), _lib.ctx(p.dev)
    if not p.dense:
        p.kind, p.para, p.flags = _device_kernel(kernel, p.ctx)
    p.x = _lib.f64(x)
    p.n, p.D = p.x.shape
    p.y = _lib.f64(y).reshape(p.n)
    if reserve:
        DeviceFactor.reserve(p.n, p.dev)
    if resident:
        _Resident.ensure(p.x, p.y, p.dev)
    p.m, p.dm, p.nm = _mean_inputs(meanfunc, p.x)
    p.hyp = _lib.f64(np.asarray(covfunc.hyp, dtype=float))
    return p


def _want(nargout):
    return int(min(max(nargout, 1), 3))


def _lik_args(likfunc, accepted, refusal):
    """(lik, likhyp, nlik) of the C entry points for a likelihood among the classes ``accepted``; NotImplementedError(refusal)
    for any other."""
    for cls, code in ((_lik.Erf, _lib.LIK_ERF), (_lik.Laplace, _lib.LIK_LAPLACE), (_lik.Gauss, _lib.LIK_GAUSS)):
        if cls in accepted and isinstance(likfunc, cls):
            if cls is _lik.Erf:
                return code, None, 0
            return code, _lib.f64(np.asarray(likfunc.hyp, dtype=float).reshape(-1)), 1
    raise NotImplementedError(refusal)


_OPTION_DEFAULTS = {b"ep_tol_exp": 4, b"ep_max_sweep": 10, b"laplace_tol_exp": 6}


@contextlib.contextmanager
def _options(lib, ctx, values):
    """Context options {name: value} for the block; back at the library's defaults on exit, raised or not."""
    try:
        for name, v in values.items():
            _lib.check(lib.pgp_set_option(ctx, name, int(v)), "pgp_set_option")
        yield
    finally:
        for name in values:
            lib.pgp_set_option(ctx, name, _OPTION_DEFAULTS[name])


def _ep_options(tol_exp):
    """The private sweep tolerance of EP / FITC_EP (gradient checks): with it, as many sweeps as it takes."""
    return {} if tol_exp is None else {b"ep_tol_exp": tol_exp, b"ep_max_sweep": 1000}


def _dense_cov_grads(lib, ctx, covfunc, x, n, log_sn):
    """The dense route's covariance gradients, one derivative matrix at a time (Core/inf.py:376-377, 536-541, 780-786), against
    what the dense fit with want = 3 that directly precedes left in the workspace."""
    g, out = np.zeros(1), []
    for h in range(len(covfunc.hyp)):
        dK = _lib.f64(covfunc.getDerMatrix(x=x, mode="train", der=h))
        _lib.check(lib.pgp_dense_grad_term(ctx, _lib.ptr(dK), n, log_sn, _lib.ptr(g)), "pgp_dense_grad_term")
        out.append(np.float64(g[0]))
    return out


def _dnlZ(meanfunc, covfunc, likfunc, g, nm, nc, nlik, cov=None):
    """dnlZStruct from g = [mean (nm) | cov (nc) | lik (nlik) ...]; ``cov`` replaces the middle part (dense route: nc = 0)."""
    d = dnlZStruct(meanfunc, covfunc, likfunc)
    d.mean = [np.float64(v) for v in g[:nm]]
    d.cov = [np.float64(v) for v in g[nm:nm + nc]] if cov is None else cov
    d.lik = [np.float64(v) for v in g[nm + nc:nm + nc + nlik]]
    return d


def _returns(nargout, post, nlZ, dnlZ, always_nlZ=False):
    """post | (post, nlZ) | (post, nlZ, dnlZ) by nargout; EP and Laplace return (post, nlZ) at nargout = 1 too (always_nlZ)."""
    if nargout > 2:
        return post, nlZ, dnlZ
    if nargout > 1 or always_nlZ:
        return post, nlZ
    return post


def _posterior(alpha, sW, L, dense=False):
    post = postStruct()
    post.alpha, post.sW, post.L = alpha, sW, L
    if dense:
        post.L.dense = True                          # predict hands the cross-covariance block in (GP._latent)
    return post


class Exact(Inference):
    """Exact inference for a Gaussian likelihood (Core/inf.py:345-384)."""

    def __init__(self, sharded=False, gather_factor=False):
        """sharded: False = one GPU (the reference's unit of work); True or a ``sharded.Comm`` = ONE fit over every rank of
        the process group (one process per GPU, all ranks call with the same model; pygps_amd/sharded.py).  gather_factor:
        a sharded fit also returns post.L as a host array on every rank (n^2 doubles; moderate n)."""
        self.name = "Exact inference"
        self.device = None
        self.sharded = sharded
        self.gather_factor = gather_factor

    def _evaluate_sharded(self, meanfunc, covfunc, likfunc, x, y, nargout):
        from . import sharded as _sh
        comm = self.sharded if isinstance(self.sharded, _sh.Comm) else _sh.default_comm(self.device)
        dev = comm.device
        kind, para, flags = _device_kernel(covfunc, comm.ctx)
        x = _lib.f64(x)
        n = x.shape[0]
        y = _lib.f64(y).reshape(n)
        _Resident.ensure(x, y, dev)
        m, dm, nm = _mean_inputs(meanfunc, x)
        nc = len(covfunc.hyp)
        log_sn = float(likfunc.hyp[0])
        alpha, nlz, g, ms6, Lh, fh = _sh.exact_fit(comm, kind, para, flags, covfunc.hyp, log_sn, m, dm, nm, n, nargout,
                                                   gather_factor=self.gather_factor, keep_factor=not self.gather_factor)
        self.last_ms = ms6[:4]
        self.last_bytes = {"peak_device_bytes": int(ms6[4]), "factor_device_bytes": int(ms6[5])}
        # the multi-rank timers of this rank: stall of the compute stream waiting for panels, time inside the broadcasts
        self.last_comm = {"wait_panel_ms": float(ms6[6]), "bcast_ms": float(ms6[7]), "bcast_bytes": float(ms6[8]),
                          "bcast_max_ms": float(ms6[9]),
                          "bcast_GBs": float(ms6[8]) / max(float(ms6[7]), 1e-9) / 1e6 if ms6[7] > 0 else 0.0,
                          "wait_share": float(ms6[6]) / max(float(ms6[1]), 1e-9) if ms6[1] > 0 else 0.0}
        post = _posterior(alpha.reshape(n, 1), np.ones((n, 1)) / np.sqrt(np.exp(2 * log_sn)),
                          Lh if Lh is not None else _sh.DistributedFactor(n, comm, fh))
        dnlZ = _dnlZ(meanfunc, covfunc, likfunc, g, nm, nc, 1) if nargout > 2 else None
        return _returns(nargout, post, np.float64(nlz), dnlZ)

    def _evaluate_dense(self, p, meanfunc, covfunc, likfunc, nargout):
        """Covariance functions that are not device programs (a tree with more than two ARD leaves or more than 8 leaves /
        products, Core/cov.py:230-328): K and the derivative matrices come from getCovMatrix / getDerMatrix (the children's
        device-built matrices combined on the host), the factorisation with the fused inverse, alpha, nlZ and every Hadamard
        sum sum(Q o dK_h) / 2 run on the device (csrc/dense.hip).  Costs PCIe traffic (n^2 doubles per matrix), never raises."""
        n, nm = p.n, p.nm
        log_sn = float(likfunc.hyp[0])
        K = _lib.f64(covfunc.getCovMatrix(x=p.x, mode="train"))
        r = _lib.f64(p.y - p.m)
        alpha = np.empty(n)
        nlZ = np.zeros(1)
        glik = np.zeros(1)
        fh = C.c_void_p()
        DeviceFactor.reserve(n, p.dev)
        gvec = self._call_dense(p.lib, p.ctx, K, n, r, p.m, log_sn, _want(nargout), alpha, nlZ, glik, fh)
        del K
        post = _posterior(alpha.reshape(n, 1), np.ones((n, 1)) / np.sqrt(np.exp(2 * log_sn)),
                          DeviceFactor(fh, n, p.dev, _lib.current_slot()), dense=True)
        dnlZ = None
        if nargout > 2:
            cov = _dense_cov_grads(p.lib, p.ctx, covfunc, p.x, n, log_sn)
            g = [-(p.dm[i] @ gvec) for i in range(nm)] + [glik[0]]                # Core/inf.py:378-381
            dnlZ = _dnlZ(meanfunc, covfunc, likfunc, g, nm, 0, 1, cov=cov)
        return _returns(nargout, post, np.float64(nlZ[0]), dnlZ)

    # the two device calls, as hooks: inf.LOO overrides them (and nothing else of evaluate / _evaluate_dense)
    def _call_dense(self, lib, ctx, K, n, r, m, log_sn, want, alpha, nlZ, glik, fh):
        """The dense route's fit; returns the vector v of the mean gradients -v' dm_h (alpha)."""
        _lib.check(lib.pgp_exact_fit_dense(ctx, _lib.ptr(K), n, _lib.ptr(r), log_sn, want, _lib.ptr(alpha), _lib.ptr(nlZ),
                                           _lib.ptr(glik), C.byref(fh)), "pgp_exact_fit_dense")
        return alpha

    def _call_program(self, ctx, kind, hyp, nc, para, flags, log_sn, m, dm, nm, want, n, alpha, nlZ, g, fh):
        rc = _lib.load().pgp_exact_fit(ctx, kind, _lib.ptr(hyp), nc, int(para), int(flags), log_sn, _lib.ptr(m), _lib.ptr(dm), nm,
                                       want, _lib.ptr(alpha), _lib.ptr(nlZ), _lib.ptr(g), C.byref(fh))
        _lib.check(rc, "pgp_exact_fit")

    _gauss_only = "Exact inference only possible with Gaussian likelihood"

    def evaluate(self, meanfunc, covfunc, likfunc, x, y, nargout=1):
        if not isinstance(likfunc, _lik.Gauss):
            raise Exception(self._gauss_only)
        if self.sharded:
            _cov.refuse_pre(covfunc, "a sharded fit (the panels of a distributed factor are assembled per rank)")
            _cov.refuse_dot(covfunc, "a sharded fit")
            _check_pre(covfunc, x)
            if _dense_route(covfunc):
                raise NotImplementedError("pygps_amd: a sharded fit needs a covariance function that runs as a device program")
            return self._evaluate_sharded(meanfunc, covfunc, likfunc, x, y, nargout)
        dense = _dense_route(covfunc)       # that route hands r = y - m in and makes room for its factor behind getCovMatrix
        p = _prepare(self.device, meanfunc, covfunc, x, y, reserve=not dense, resident=not dense)
        if p.dense:
            return self._evaluate_dense(p, meanfunc, covfunc, likfunc, nargout)
        n, nm, nc = p.n, p.nm, len(p.hyp)
        log_sn = float(likfunc.hyp[0])
        alpha = np.empty(n)
        nlZ = np.zeros(1)
        g = np.zeros(nm + nc + 1)
        fh = C.c_void_p()
        self._call_program(p.ctx, p.kind, p.hyp, nc, p.para, p.flags, log_sn, p.m, p.dm, nm, _want(nargout), n, alpha, nlZ, g, fh)
        post = _posterior(alpha.reshape(n, 1), np.ones((n, 1)) / np.sqrt(np.exp(2 * log_sn)),
                          DeviceFactor(fh, n, p.dev, _lib.current_slot()))
        dnlZ = _dnlZ(meanfunc, covfunc, likfunc, g, nm, nc, 1) if nargout > 2 else None
        return _returns(nargout, post, np.float64(nlZ[0]), dnlZ)


class LOO(Exact):
    """Leave-one-out inference for a Gaussian likelihood (GPML's infLOO; Rasmussen & Williams 5.4.2; the reference has none).

    The posterior is the exact fit's own -- predict, predict_joint and the samplers work on it unchanged; bit for bit where both
    take the same route to alpha: always with gradients, value-only with the fused inverse (the default) -- but ``nlZ`` is the
    negative LOO log pseudo-likelihood -sum_i log p(y_i | x, y_-i, hyp) and ``dnlZ`` its gradient (mean | cov | lik), both
    in closed form from the one factorisation (pgp_loo_fit, csrc/loo.hip; pgp_loo_fit_dense for covariance trees that are not
    device programs).  After every evaluate with nargout >= 2: ``last_loo = (mu, s2, lp)``, each (n, 1) -- the LOO
    predictive mean, variance (noise included) and log density of every training point -- and ``last_nlZ_marginal``.

    Out of scope: EP / Laplace cavity LOO (lik.Gauss only), FITC, sharded fits."""

    def __init__(self, sharded=False):
        super(LOO, self).__init__(sharded=sharded)
        self.name = "Leave-one-out inference"
        self.last_loo = None
        self.last_nlZ_marginal = None

    _gauss_only = "LOO inference only possible with Gaussian likelihood"

    def _keep(self, n, mu, s2, lp, nlz2, want):
        if want > 1:
            self.last_loo = (mu.reshape(n, 1), s2.reshape(n, 1), lp.reshape(n, 1))
            self.last_nlZ_marginal = np.float64(nlz2[1])

    def _call_dense(self, lib, ctx, K, n, r, m, log_sn, want, alpha, nlZ, glik, fh):
        """pgp_loo_fit_dense: the device is handed r = y - m only, so m is added back to the LOO means here; the covariance
        gradients come from pgp_dense_grad_term against the S the fit left; the mean gradients are -u' dm_h."""
        mu, s2, lp, u = np.empty(n), np.empty(n), np.empty(n), np.empty(n)
        nlz2 = np.zeros(2)
        _lib.check(lib.pgp_loo_fit_dense(ctx, _lib.ptr(K), n, _lib.ptr(r), log_sn, want, _lib.ptr(alpha), _lib.ptr(mu), _lib.ptr(s2),
                                         _lib.ptr(lp), _lib.ptr(nlz2), _lib.ptr(glik), _lib.ptr(u), C.byref(fh)), "pgp_loo_fit_dense")
        nlZ[0] = nlz2[0]
        self._keep(n, mu + m, s2, lp, nlz2, want)
        return u

    def _call_program(self, ctx, kind, hyp, nc, para, flags, log_sn, m, dm, nm, want, n, alpha, nlZ, g, fh):
        mu, s2, lp = np.empty(n), np.empty(n), np.empty(n)
        nlz2 = np.zeros(2)
        rc = _lib.load().pgp_loo_fit(ctx, kind, _lib.ptr(hyp), nc, int(para), int(flags), log_sn, _lib.ptr(m), _lib.ptr(dm), nm, want,
                                     _lib.ptr(alpha), _lib.ptr(mu), _lib.ptr(s2), _lib.ptr(lp), _lib.ptr(nlz2), _lib.ptr(g),
                                     C.byref(fh))
        _lib.check(rc, "pgp_loo_fit")
        nlZ[0] = nlz2[0]
        self._keep(n, mu, s2, lp, nlz2, want)

    def evaluate(self, meanfunc, covfunc, likfunc, x, y, nargout=1):
        if self.sharded and isinstance(likfunc, _lik.Gauss):
            raise NotImplementedError("pygps_amd: leave-one-out inference runs on one GPU (the distributed strips of B^-1 of a "
                                      "sharded fit are out of scope)")
        return super(LOO, self).evaluate(meanfunc, covfunc, likfunc, x, y, nargout)


class EP(Inference):
    """Expectation propagation with the probit likelihood or lik.Laplace (Core/inf.py:723-806).  The site-parameter
    state (last_ttau / last_tnu) persists on the object across calls and warm-starts the next one,
    exactly like the reference.

    Both likelihoods run through pgp_ep_fit_lik (pgp_ep_fit_dense_lik for covariance trees that are not device programs).
    With lik.Laplace the mean and likelihood gradients are evaluated at the cavity of f, nu_n / tau_n + m; the reference
    evaluates them at nu_n / tau_n (inf.py:788-798), which is off by m wherever the mean is not zero, and takes the first
    site's dlZ for every site in the mean gradient.  ``reference_compat = True`` moves both, dnlZ.lik and the mean gradient,
    to the reference's point nu_n / tau_n (the mean gradient stays per site).  lik.Erf keeps the reference's point for its
    mean gradient whatever this flag says: that is what the G8 / G14 recordings pin."""

    def __init__(self):
        self.name = "Expectation Propagation"
        self.last_ttau = None
        self.last_tnu = None
        self.device = None
        self.sweeps = 0
        self.reference_compat = False
        self._tol_exp = None            # private: sweep tolerance 10^-_tol_exp instead of the reference's 1e-4 (gradient checks)

    def evaluate(self, meanfunc, covfunc, likfunc, x, y, nargout=1):
        lik, likhyp, nlik = _lik_args(likfunc, (_lik.Laplace, _lik.Erf),
                                      "pygps_amd: EP runs on the device for lik.Erf and lik.Laplace only (no CPU fallback)")
        # covariance functions that are not device programs (Core/cov.py:230-328 composes anything): K and the derivative
        # matrices come from getCovMatrix / getDerMatrix, the sweeps, the posterior, alpha, nlZ and every Hadamard sum
        # 1/2 sum((sW sW' o B^-1 - alpha alpha') o dK_h) (Core/inf.py:780-786) run on the device
        p = _prepare(self.device, meanfunc, covfunc, x, y)
        lib, ctx, n, nm, dense = p.lib, p.ctx, p.n, p.nm, p.dense
        nc = 0 if dense else len(p.hyp)
        warm = self.last_ttau is not None
        ttau = _lib.f64(self.last_ttau).reshape(n).copy() if warm else np.zeros(n)
        tnu = _lib.f64(self.last_tnu).reshape(n).copy() if warm else np.zeros(n)
        alpha = np.empty(n)
        sW = np.empty(n)
        nlZ = np.zeros(1)
        g = np.zeros(nm + nc + 1)
        sweeps = C.c_int()
        fh = C.c_void_p()
        tail = (lik, _lib.ptr(likhyp), nlik, int(bool(self.reference_compat)), _lib.ptr(p.m), _lib.ptr(p.dm), nm, _want(nargout),
                int(warm), _lib.ptr(ttau), _lib.ptr(tnu), _lib.ptr(alpha), _lib.ptr(sW), _lib.ptr(nlZ), _lib.ptr(g),
                C.byref(sweeps), C.byref(fh))
        with _options(lib, ctx, _ep_options(self._tol_exp)):
            if dense:
                K = _lib.f64(covfunc.getCovMatrix(x=p.x, mode="train"))
                rc = lib.pgp_ep_fit_dense_lik(ctx, _lib.ptr(K), *tail)
                del K
            else:
                rc = lib.pgp_ep_fit_lik(ctx, p.kind, _lib.ptr(p.hyp), nc, int(p.para), int(p.flags), *tail)
        if rc == -99:
            raise NotImplementedError("pygps_amd: the device EP path is not built in this version")
        _lib.check(rc, "pgp_ep_fit_dense_lik" if dense else "pgp_ep_fit_lik")
        self.sweeps = sweeps.value
        if self.sweeps == 10:
            logging.getLogger(__name__).warning("maximum number of sweeps reached in function infEP")
        self.last_ttau = ttau.reshape(n, 1)
        self.last_tnu = tnu.reshape(n, 1)
        post = _posterior(alpha.reshape(n, 1), sW.reshape(n, 1), DeviceFactor(fh, n, p.dev, _lib.current_slot()), dense)
        dnlZ = None
        if nargout > 2:
            cov = _dense_cov_grads(lib, ctx, covfunc, p.x, n, 0.0) if dense else None
            dnlZ = _dnlZ(meanfunc, covfunc, likfunc, g, nm, nc, nlik, cov=cov)
        return _returns(nargout, post, np.float64(nlZ[0]), dnlZ, always_nlZ=True)


class Laplace(Inference):
    """Laplace's approximation to the posterior (Core/inf.py:459-564) with lik.Erf or lik.Gauss: the Newton iteration in f
    with Brent's line search, the posterior and the gradients with their implicit part, all in ONE device call
    (csrc/laplace.hip).  ``last_alpha`` persists across calls and warm-starts the next one as the reference's does
    (inf.py:474-497); one of another length starts cold.  ``newton_steps``: Newton steps of the last call;
    ``last_steps``: (step size, objective, evaluations) of each of its line searches."""

    def __init__(self):
        self.name = "Laplace's Approximation"
        self.last_alpha = None
        self.device = None
        self.newton_steps = 0
        self.last_steps = np.zeros((0, 3))
        self._tol_exp = None            # private: Newton tolerance 10^-_tol_exp instead of the reference's 1e-6 (gradient checks)

    def _lik_args(self, likfunc):
        return _lik_args(likfunc, (_lik.Erf, _lik.Gauss),
                         "pygps_amd: Laplace runs on the device for lik.Erf and lik.Gauss only (no CPU fallback)")

    def evaluate(self, meanfunc, covfunc, likfunc, x, y, nargout=1):
        lik, likhyp, nlik = self._lik_args(likfunc)
        p = _prepare(self.device, meanfunc, covfunc, x, y)
        lib, ctx, n, nm, dense = p.lib, p.ctx, p.n, p.nm, p.dense
        nc = 0 if dense else len(p.hyp)
        last = None if self.last_alpha is None else np.asarray(self.last_alpha, dtype=float).reshape(-1)
        warm = last is not None and last.shape[0] == n
        alpha = _lib.f64(last).copy() if warm else np.zeros(n)
        sW = np.empty(n)
        nlZ = np.zeros(1)
        g = np.zeros(nm + nc + nlik + 1)
        steps = C.c_int()
        trace = np.zeros((20, 3))
        fh = C.c_void_p()
        tail = (lik, _lib.ptr(likhyp), nlik, _lib.ptr(p.m), _lib.ptr(p.dm), nm, _want(nargout), int(warm), _lib.ptr(alpha),
                _lib.ptr(sW), _lib.ptr(nlZ), _lib.ptr(g), C.byref(steps), _lib.ptr(trace), C.byref(fh))
        with _options(lib, ctx, {} if self._tol_exp is None else {b"laplace_tol_exp": self._tol_exp}):
            if dense:
                K = _lib.f64(covfunc.getCovMatrix(x=p.x, mode="train"))
                rc = lib.pgp_laplace_fit_dense(ctx, _lib.ptr(K), *tail)
                del K
            else:
                rc = lib.pgp_laplace_fit(ctx, p.kind, _lib.ptr(p.hyp), nc, int(p.para), int(p.flags), *tail)
        if rc == _lib.ERR_LAPLACE_WNEG:
            raise NotImplementedError("pygps_amd: Laplace met W < 0 (the reference's LU branch is not restated)")
        _lib.check(rc, "pgp_laplace_fit_dense" if dense else "pgp_laplace_fit")
        self.newton_steps = steps.value
        self.last_steps = trace[:self.newton_steps].copy()
        self.last_alpha = alpha.reshape(n, 1)                   # inf.py:513
        post = _posterior(alpha.reshape(n, 1).copy(), sW.reshape(n, 1), DeviceFactor(fh, n, p.dev, _lib.current_slot()), dense)
        dnlZ = None
        if nargout > 2:
            cov = _dense_cov_grads(lib, ctx, covfunc, p.x, n, 0.0) if dense else None
            dnlZ = _dnlZ(meanfunc, covfunc, likfunc, g, nm, nc, nlik, cov=cov)
        return _returns(nargout, post, np.float64(nlZ[0]), dnlZ, always_nlZ=True)


class FITCPosterior(object):
    """Device handle of a FITC posterior (alpha, dense L, inducing coordinates) for predict; freed with the object."""

    def __init__(self, handle, device, slot):
        self.handle = handle
        self._dev = device
        self._slot = slot
        self._ctx = _lib.ctx(device, slot)                # captured now: the finalizer must not take _lib's lock
        self._fin = weakref.finalize(self, FITCPosterior._free, _lib.load().pgp_fitc_free, self._ctx, handle.value)

    @property
    def ctx(self):
        return self._ctx

    @staticmethod
    def _free(free_fn, ctx_handle, h):
        try:
            free_fn(ctx_handle, C.c_void_p(h))
        except Exception:
            pass

    def __deepcopy__(self, memo):
        return self                                      # the device object is immutable; share it


def _fitc_inputs(device, meanfunc, covfunc, x, y, nargout, not_fitc):
    """The FITC engines' checks (``not_fitc`` is raised unless covfunc is a FITC covariance) and inputs: beside ``_prepare``'s,
    xu (nu, D), nu and dxu -- the (nu, D) output of the gradient w.r.t. the inducing inputs, or None where it is not asked for."""
    if not isinstance(covfunc, _cov.FITCOfKernel):
        raise not_fitc
    _cov.refuse_pre(covfunc.covfunc, "the FITC approximation (fitc(u) of a precomputed matrix has no meaning)")
    _cov.refuse_dot(covfunc.covfunc, "the FITC approximation")
    if covfunc.learn_inducing:
        covfunc._check_learn_inducing()
    p = _prepare(device, meanfunc, covfunc, x, y, dense_ok=False, reserve=False, inner=True)
    p.xu = _lib.f64(covfunc.inducingInput)
    if p.xu.shape[1] != p.D:
        raise Exception('Dimensionality of inducing inputs must match training inputs')
    p.nu = p.xu.shape[0]
    p.dxu = np.zeros((p.nu, p.D)) if (covfunc.learn_inducing and nargout > 2) else None
    return p


class FITC_Exact(Inference):
    """FITC approximation to the posterior GP (Core/inf.py:386-455): exact inference with
    Kt = Q + diag(K - Q), Q = Ku' inv(Kuu + snu2 I) Ku, snu2 = sn2 / 1e6.  One device call (csrc/fitc.hip)."""

    def __init__(self):
        self.name = 'FICT exact inference'
        self.device = None

    def evaluate(self, meanfunc, covfunc, likfunc, x, y, nargout=1):
        if not isinstance(likfunc, _lik.Gauss):
            raise Exception('Exact inference only possible with Gaussian likelihood')
        p = _fitc_inputs(self.device, meanfunc, covfunc, x, y, nargout, Exception('Only covFITC supported.'))
        n, nm, nu, nc = p.n, p.nm, p.nu, len(p.hyp)
        log_sn = float(likfunc.hyp[0])
        alpha = np.empty(nu)
        Lm = np.empty((nu, nu))
        nlZ = np.zeros(1)
        g = np.zeros(nm + nc + 1)
        fh = C.c_void_p()
        args = (p.ctx, p.kind, _lib.ptr(p.hyp), nc, int(p.para), int(p.flags), log_sn, _lib.ptr(p.xu), nu,
                _lib.ptr(p.m), _lib.ptr(p.dm), nm, _want(nargout), _lib.ptr(alpha),
                _lib.ptr(Lm), _lib.ptr(nlZ), _lib.ptr(g), C.byref(fh))
        if p.dxu is None:
            rc = p.lib.pgp_fitc_fit(*args)
        else:
            rc = p.lib.pgp_fitc_fit_xu(*(args + (_lib.ptr(p.dxu),)))
        _lib.check(rc, "pgp_fitc_fit")
        # post.L = Sigma - inv(Kuu): dense, not triangular (inf.py:424)
        post = _posterior(alpha.reshape(nu, 1), np.ones((n, 1)) / np.sqrt(np.exp(2 * log_sn)), Lm)
        post.fitc = FITCPosterior(fh, p.dev, _lib.current_slot())
        dnlZ = None
        if nargout > 2:
            dnlZ = _dnlZ(meanfunc, covfunc, likfunc, g, nm, nc, 1)
            dnlZ.xu = p.dxu
        return _returns(nargout, post, np.float64(nlZ[0]), dnlZ)


class FITC_EP(Inference):
    """FITC-EP approximation to the posterior GP (Core/inf.py:810-944): EP with lik.Erf or lik.Laplace on Kt = Q + diag(K - Q),
    Q = Ku' inv(Kuu + snu2 I) Ku, snu2 = 1e-6 for Erf (no noise hyper-parameter) and 1e-6 sn2 for Laplace (inf.py:837-841).
    One device call (csrc/fitc.hip, pgp_fitc_ep_fit_lik): 128-site block sweeps in O(n nu) memory.  ``last_ttau`` / ``last_tnu`` persist across
    calls and warm-start the next one as the reference's do (inf.py:857-870); ones of another length start cold.
    ``sweeps``: EP sweeps of the last call.

    One deviation: at 10 sweeps this logs the warning "maximum number of sweeps reached" as inf.EP does, where the reference
    raises AttributeError (FITC_EP.__init__ never sets self.logger, inf.py:823-826).

    With lik.Laplace, dnlZ.lik = -sum dlZhyp + snu2 (covariance-like term) (inf.py:925-936).  The reference evaluates dlZhyp at
    nu_n / tau_n + m, but _epfitcZ's nu_n already carries m tau_n, so a non-zero mean counts twice; the default is the cavity
    nu_n / tau_n (central differences agree), ``reference_compat = True`` reproduces the reference's point."""

    def __init__(self):
        self.name = 'FITC Expectation Propagation'
        self.last_ttau = None
        self.last_tnu = None
        self.device = None
        self.sweeps = 0
        self.reference_compat = False
        self._tol_exp = None            # private: sweep tolerance 10^-_tol_exp instead of the reference's 1e-4 (gradient checks)

    def evaluate(self, meanfunc, covfunc, likfunc, x, y, nargout=1):
        lik, likhyp, nlik = _lik_args(likfunc, (_lik.Laplace, _lik.Erf),
                                      "pygps_amd: FITC_EP runs on the device for lik.Erf and lik.Laplace only (no CPU fallback)")
        p = _fitc_inputs(self.device, meanfunc, covfunc, x, y, nargout, NotImplementedError(
            "pygps_amd: FITC_EP needs a FITC covariance (covfunc.fitc(u)); only covFITC is supported"))
        n, nm, nu, nc = p.n, p.nm, p.nu, len(p.hyp)
        warm = (self.last_ttau is not None and self.last_tnu is not None
                and np.asarray(self.last_ttau).size == n and np.asarray(self.last_tnu).size == n)
        ttau = _lib.f64(np.asarray(self.last_ttau, dtype=float)).reshape(n).copy() if warm else np.zeros(n)
        tnu = _lib.f64(np.asarray(self.last_tnu, dtype=float)).reshape(n).copy() if warm else np.zeros(n)
        alpha = np.empty(nu)
        Lm = np.empty((nu, nu))
        nlZ = np.zeros(1)
        g = np.zeros(nm + nc + nlik)
        sweeps = C.c_int()
        fh = C.c_void_p()
        with _options(p.lib, p.ctx, _ep_options(self._tol_exp)):
            args = (p.ctx, p.kind, _lib.ptr(p.hyp), nc, int(p.para), int(p.flags), lik, _lib.ptr(likhyp), nlik,
                    int(bool(self.reference_compat)), _lib.ptr(p.xu), nu, _lib.ptr(p.m), _lib.ptr(p.dm), nm, _want(nargout),
                    int(warm), _lib.ptr(ttau), _lib.ptr(tnu), _lib.ptr(alpha), _lib.ptr(Lm),
                    _lib.ptr(nlZ), _lib.ptr(g), C.byref(sweeps), C.byref(fh))
            if p.dxu is None:
                rc = p.lib.pgp_fitc_ep_fit_lik(*args)
            else:
                rc = p.lib.pgp_fitc_ep_fit_lik_xu(*(args + (_lib.ptr(p.dxu),)))
        _lib.check(rc, "pgp_fitc_ep_fit_lik")
        self.sweeps = sweeps.value
        if self.sweeps == 10:
            logging.getLogger(__name__).warning("maximum number of sweeps reached in function infEP")
        self.last_ttau = ttau.reshape(n, 1)                     # inf.py:899-900
        self.last_tnu = tnu.reshape(n, 1)
        # post.L = -R0'V inv(Kt + diag(1/ttau)) V'R0: dense, not triangular (inf.py:908); post.sW: inf.py:902
        post = _posterior(alpha.reshape(nu, 1), np.sqrt(ttau).reshape(n, 1), Lm)
        post.fitc = FITCPosterior(fh, p.dev, _lib.current_slot())
        dnlZ = None
        if nargout > 2:
            dnlZ = _dnlZ(meanfunc, covfunc, likfunc, g, nm, nc, nlik)
            dnlZ.xu = p.dxu
        return _returns(nargout, post, np.float64(nlZ[0]), dnlZ)
