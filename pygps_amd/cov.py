"""Covariance functions: the drop-in classes for the three kernels on the hot path
(reference: pyGPs/Core/cov.py -- Kernel :61-226, RBF :786-828, RBFard :872-938, Matern :1078-1182).

Same constructor signatures, same ``hyp`` (log-space list, read fresh on every call: the optimiser
overwrites it, Core/opt.py:88) and ``para`` attributes, same ``getCovMatrix(x, z, mode)`` /
``getDerMatrix(x, z, mode, der)`` contract and the same exceptions.  The arithmetic runs in the HIP
tile kernel behind ``pgp_cov`` (csrc/assemble.hip); there is no numpy fallback.
"""
import logging

import numpy as np

from . import _lib

_MODES = {"train": _lib.MODE_TRAIN, "cross": _lib.MODE_CROSS, "self_test": _lib.MODE_SELF_TEST}


class Kernel(object):
    """Base class: argument checks (Core/cov.py:115-154) and operator overloading (:160-202)."""
    _kind = None            # PGP_COV_* for the kernels that have a device functor
    #: Matern only -- reproduce the reference's derivative-of-K quirk (Core/cov.py:1173-1177).
    reference_compat = False

    def __init__(self):
        self.hyp = []
        self.para = []
        self.logger = logging.getLogger(__name__)

    def __repr__(self):
        return (str(type(self)) + ": to get the kernel matrix or kernel derviatives use: \n"
                "model.covfunc.getCovMatrix()\nmodel.covfunc.getDerMatrix()")

    # -- contract ------------------------------------------------------------------------------
    def getCovMatrix(self, x=None, z=None, mode=None):
        raise NotImplementedError

    def getDerMatrix(self, x=None, z=None, mode=None, der=None):
        raise NotImplementedError

    def checkInputGetCovMatrix(self, x, z, mode):
        if mode is None:
            raise Exception("Specify the mode: 'train' or 'cross'")
        if x is None and z is None:
            raise Exception("Specify at least one: training input (x) or test input (z) or both.")
        if mode == "cross" and (x is None or z is None):
            raise Exception("Specify both: training input (x) and test input (z) for cross covariance.")

    def checkInputGetDerMatrix(self, x, z, mode, der):
        self.checkInputGetCovMatrix(x, z, mode)
        if der is None:
            raise Exception("Specify the index of parameters of the derivatives.")

    # -- composition (host-side sums/products of device-built matrices) -----------------------------
    def __add__(self, other):
        return SumOfKernel(self, other)

    def __mul__(self, other):
        if isinstance(other, (int, float)):
            return ScaleOfKernel(self, other)
        if isinstance(other, Kernel):
            return ProductOfKernel(self, other)
        logging.getLogger(__name__).error("only numbers and Kernels are supported operand types for *")

    __rmul__ = __mul__

    def fitc(self, inducingInput):
        """Covariance function for the FITC approximation (Core/cov.py:195-202)."""
        return FITCOfKernel(self, inducingInput)

    # -- device dispatch ---------------------------------------------------------------------------
    def _device_params(self):
        """(kind, para, flags) of the device functor."""
        return self._kind, 0, 0

    def _program(self, h0):
        """Postfix device program of this (sub)tree whose first hyper has flat index ``h0``:
        ``(tokens, n_leaves, n_products, n_scales)`` -- or None when a leaf cannot be part of a program."""
        if self._kind is None:
            return None
        kind, para, flags = self._device_params()
        ard = 1 if self._kind in (_lib.COV_RBFARD, _lib.COV_RQARD) else 0
        if ard and len(self.hyp) - (1 if self._kind == _lib.COV_RBFARD else 2) > _lib.PROG_MAX_ARD_DIM:
            return None
        dot = 1 if self._kind in (_lib.COV_LINEAR, _lib.COV_POLY) else 0
        return [_lib.PROG_LEAF, int(kind), int(para), int(flags), int(h0)], 1, 1, ard * 1000 + dot * 100000

    def _pre_leaves(self):
        """The cov.Pre leaves of this (sub)tree."""
        return []

    def _dot_leaves(self):
        """The dot-product leaves (Linear, Poly, LINard) of this (sub)tree: k(x, x) differs from point to point."""
        return []

    def _on_device(self):
        return True

    def _bind(self, ctx):
        """Select this kernel on context ``ctx``: returns (kind, para, flags) for the C entry points."""
        if self._kind is None:
            raise NotImplementedError(
                "pygps_amd: %s has no device covariance functor; there is no CPU fallback" % type(self).__name__)
        return self._device_params()

    _WRONG_DER = "Wrong derivative index"
    _BAD_PARA = "invalid kernel parameter"
    _OVER_LIMIT = "the covariance function exceeds the limits of the device code; there is no CPU fallback"

    def _device_eval(self, x, z, mode, der):
        if mode not in _MODES:
            raise Exception("Specify the mode: 'train' or 'cross'")
        kind, para, flags = self._bind(_lib.ctx())
        xa = None if x is None else _lib.f64(x)
        za = None if z is None else _lib.f64(z)
        if mode == "self_test":
            xa = None
        if mode == "train":
            za = None
        ref = xa if xa is not None else za
        n = 0 if xa is None else xa.shape[0]
        m = 0 if za is None else za.shape[0]
        d = ref.shape[1]
        hyp = _lib.f64(np.asarray(self.hyp, dtype=float))
        shape = {"train": (n, n), "cross": (n, m), "self_test": (m, 1)}[mode]
        out = np.empty(shape)
        rc = _lib.load().pgp_cov(_lib.ctx(), kind, _MODES[mode], -1 if der is None else int(der), _lib.ptr(xa), n,
                                 _lib.ptr(za), m, d, _lib.ptr(hyp), len(hyp), int(para), int(flags), _lib.ptr(out))
        _lib.check(rc, "pgp_cov", {-4: self._WRONG_DER, -11: "number of hyperparameters does not match the input dimension",
                                   -12: self._BAD_PARA, -13: self._OVER_LIMIT})
        return out


class RBF(Kernel):
    """Squared exponential, isotropic.  hyp = [log_ell, log_sigma]   (Core/cov.py:786-828)"""
    _kind = _lib.COV_RBF
    _WRONG_DER = "Calling for a derivative in RBF that does not exist"

    def __init__(self, log_ell=0., log_sigma=0.):
        self.hyp = [log_ell, log_sigma]
        self.para = []

    def getCovMatrix(self, x=None, z=None, mode=None):
        self.checkInputGetCovMatrix(x, z, mode)
        return self._device_eval(x, z, mode, None)

    def getDerMatrix(self, x=None, z=None, mode=None, der=None):
        self.checkInputGetDerMatrix(x, z, mode, der)
        return self._device_eval(x, z, mode, der)


class RBFard(Kernel):
    """Squared exponential with ARD.  hyp = log_ell_list + [log_sigma]   (Core/cov.py:872-938)"""
    _kind = _lib.COV_RBFARD
    _WRONG_DER = "Wrong derivative index in RDFard"

    def __init__(self, D=None, log_ell_list=None, log_sigma=0.):
        if log_ell_list is None:
            self.hyp = [0. for _ in range(D)] + [log_sigma]
        else:
            self.hyp = list(log_ell_list) + [log_sigma]
        self.para = []

    def getCovMatrix(self, x=None, z=None, mode=None):
        self.checkInputGetCovMatrix(x, z, mode)
        return self._device_eval(x, z, mode, None)

    def getDerMatrix(self, x=None, z=None, mode=None, der=None):
        self.checkInputGetDerMatrix(x, z, mode, der)
        return self._device_eval(x, z, mode, der)


class Matern(Kernel):
    """Matern, nu = d/2, d in {1,3,5,7}.  hyp = [log_ell, log_sigma], para = [d]  (Core/cov.py:1078-1182)

    ``getDerMatrix`` returns the mathematically correct derivative by default; set
    ``reference_compat = True`` to reproduce the reference's result bit-for-bit in structure
    (it applies dmfunc/mfunc to K instead of t, Core/cov.py:1173-1177 -- SURVEY Q4)."""
    _kind = _lib.COV_MATERN
    _WRONG_DER = "Wrong derivative value in Matern"

    def __init__(self, log_ell=0., d=3, log_sigma=0.):
        self.hyp = [log_ell, log_sigma]
        self.para = [d]
        self.logger = logging.getLogger(__name__)

    def _d(self):
        d = self.para[0]
        if np.abs(d - np.round(d)) < 1e-8:
            d = int(round(d))
        d = int(d)
        if d not in (1, 3, 5, 7):
            logging.getLogger(__name__).warning("d is neither 1,3,5 nor 7. We set it to d=3. ")
            d = 3
        return d

    def _device_params(self):
        return self._kind, self._d(), (_lib.FLAG_MATERN_REFERENCE_DER if self.reference_compat else 0)

    def getCovMatrix(self, x=None, z=None, mode=None):
        self.checkInputGetCovMatrix(x, z, mode)
        return self._device_eval(x, z, mode, None)

    def getDerMatrix(self, x=None, z=None, mode=None, der=None):
        self.checkInputGetDerMatrix(x, z, mode, der)
        return self._device_eval(x, z, mode, der)


class _DeviceKernel(Kernel):
    def getCovMatrix(self, x=None, z=None, mode=None):
        self.checkInputGetCovMatrix(x, z, mode)
        return self._device_eval(x, z, mode, None)

    def getDerMatrix(self, x=None, z=None, mode=None, der=None):
        self.checkInputGetDerMatrix(x, z, mode, der)
        return self._device_eval(x, z, mode, der)


class RBFunit(_DeviceKernel):
    """Squared exponential with unit magnitude.  hyp = [log_ell]   (Core/cov.py:832-869)"""
    _kind = _lib.COV_RBFUNIT
    _WRONG_DER = "Wrong derivative index in RDFunit"

    def __init__(self, log_ell=0.):
        self.hyp = [log_ell]
        self.para = []


class RQ(_DeviceKernel):
    """Rational quadratic, isotropic.  hyp = [log_ell, log_sigma, log_alpha]   (Core/cov.py:1304-1347)"""
    _kind = _lib.COV_RQ
    _WRONG_DER = "Wrong derivative index in covRQ"

    def __init__(self, log_ell=0., log_sigma=0., log_alpha=0.):
        self.hyp = [log_ell, log_sigma, log_alpha]
        self.para = []


class PiecePoly(_DeviceKernel):
    """Piecewise polynomial kernel with compact support.  hyp = [log_ell, log_sigma], para = [v], v in {0,1,2,3}
    (Core/cov.py:683-782)"""
    _kind = _lib.COV_PIECEPOLY
    _WRONG_DER = "Wrong derivative entry in PiecePoly"

    def __init__(self, log_ell=0., v=2, log_sigma=0.):
        self.hyp = [log_ell, log_sigma]
        self.para = [v]

    def _device_params(self):
        v = self.para[0]
        if np.abs(v - np.round(v)) < 1e-8:
            v = int(round(v))
        assert int(v) in range(4)                      # only degrees 0,1,2,3 (Core/cov.py:737)
        return self._kind, int(v), 0


class RQard(_DeviceKernel):
    """Rational quadratic with ARD.  hyp = log_ell_list + [log_sigma, log_alpha]   (Core/cov.py:1356-1425)

    The length-scale derivatives are the mathematically correct ones by default.  ``reference_compat = True``
    reproduces what the reference returns: all-zero matrices on 'train' (a missing transpose makes cdist see one
    1 x n point, :1415-1416) and coordinates multiplied instead of divided by ell_k on 'cross' (:1418)."""
    _kind = _lib.COV_RQARD
    _WRONG_DER = "Wrong derivative index in covRQard"

    def _device_params(self):
        return self._kind, 0, (_lib.FLAG_MATERN_REFERENCE_DER if self.reference_compat else 0)

    def __init__(self, D=None, log_ell_list=None, log_sigma=0., log_alpha=0.):
        if log_ell_list is None:
            self.hyp = [0. for _ in range(D)] + [log_sigma, log_alpha]
        else:
            self.hyp = list(log_ell_list) + [log_sigma, log_alpha]
        self.para = []


class Gabor(_DeviceKernel):
    """Gabor kernel h(t) = exp(-t^2/(2 ell^2)) cos(2 pi t / p).  hyp = [log_ell, log_p]   (Core/cov.py:392-450).
    Like the reference, the period is p = exp(2 * log_p) (:416) and the "derivatives" are dp*K and tan(dp)*dp*K
    (:441-445)."""
    _kind = _lib.COV_GABOR
    _WRONG_DER = "Wrong derivative entry in Gabor"

    def __init__(self, log_ell=0., log_p=0.):
        self.hyp = [log_ell, log_p]
        self.para = []


class Periodic(_DeviceKernel):
    """Smooth periodic kernel for 1-d inputs.  hyp = [log_ell, log_p, log_sigma]   (Core/cov.py:1186-1250)"""
    _kind = _lib.COV_PERIODIC
    _WRONG_DER = "Wrong derivative index in covPeriodic"
    _BAD_PARA = "periodic covariance can only be used for 1d data"

    def __init__(self, log_ell=0., log_p=0., log_sigma=0.):
        self.hyp = [log_ell, log_p, log_sigma]
        self.para = []

    def _device_eval(self, x, z, mode, der):
        for a in (x, z):                                   # Core/cov.py:1201-1204
            if a is not None:
                assert np.shape(a)[1] == 1, 'periodic covariance can only be used for 1d data'
        return super(Periodic, self)._device_eval(x, z, mode, der)


class Noise(_DeviceKernel):
    """White noise.  hyp = [log_sigma]   (Core/cov.py:1254-1300): s2*I on 'train', s2 where |x-z|^2 < 1e-9 on
    'cross', zeros on 'self_test'."""
    _kind = _lib.COV_NOISE
    _WRONG_DER = "Wrong derivative index in covNoise"

    def __init__(self, log_sigma=0.):
        self.hyp = [log_sigma]
        self.para = []


class Const(_DeviceKernel):
    """Constant kernel.  hyp = [log_sigma]   (Core/cov.py:941-982).  As in the reference the variance is
    exp(log_sigma) (:951, not squared), the training matrix carries a 1e-10 diagonal jitter (:957) and the
    derivative is 2*sf2 (:979)."""
    _kind = _lib.COV_CONST
    _WRONG_DER = "Wrong derivative entry in covConst"

    def __init__(self, log_sigma=0.):
        self.hyp = [log_sigma]
        self.para = []


class _DotKernel(_DeviceKernel):
    """Kernels of the dot product p = sum_k x_k z_k.  Not functions of a distance: their diagonal and k(z, z) differ from point to
    point, so 'self_test' is a genuine vector, predict takes k(z, z) per test point and EP reads K_ii off the assembled matrix
    (csrc/sqdist_tile.h CovSpec::diag_per_point).  FITC, sharded fits and GPMC's shared route assume one scalar k(x, x) and refuse
    them (``refuse_dot``)."""

    def _dot_leaves(self):
        return [self]

    def _n_der(self, x, z):
        return len(self.hyp)

    def getDerMatrix(self, x=None, z=None, mode=None, der=None):
        self.checkInputGetDerMatrix(x, z, mode, der)
        if der >= self._n_der(x, z):                     # on the host, before any device call
            raise Exception(self._WRONG_DER)
        self._device_params()
        return self._device_eval(x, z, mode, der)

    def getCovMatrix(self, x=None, z=None, mode=None):
        self.checkInputGetCovMatrix(x, z, mode)
        self._device_params()
        return self._device_eval(x, z, mode, None)


class Linear(_DotKernel):
    """Linear kernel sf2 (x . z).  hyp = [log_sigma]   (Core/cov.py:986-1024).  As in the reference -- and like ``Const`` -- the
    variance is exp(log_sigma) (:997, not squared), the training matrix carries a 1e-10 diagonal jitter (:1003) and the derivative
    is 2 sf2 (x . z) (:1021; the reference's 1e-16 on its diagonal is dropped).  A leaf of device programs; alone it runs as a
    one-leaf program, for any input dimension."""
    _kind = _lib.COV_LINEAR
    _WRONG_DER = "Wrong derivative index in covLinear"

    def __init__(self, log_sigma=0.):
        self.hyp = [log_sigma]
        self.para = []


class Poly(_DotKernel):
    """Polynomial kernel sf2 (c + x . z)^d.  hyp = [log_c, log_sigma], para = [d], integer d >= 1   (Core/cov.py:623-679).
    c = exp(log_c), sf2 = exp(2 log_sigma); 1e-10 diagonal jitter inside the power on 'train' (:649).  ``getDerMatrix(der=2)``
    ("the degree") returns zeros (:675-676).  A leaf of device programs, any input dimension."""
    _kind = _lib.COV_POLY
    _WRONG_DER = "Wrong derivative entry in Poly"
    _BAD_PARA = "Poly needs an integer degree d >= 1"

    def __init__(self, log_c=0., d=2, log_sigma=0.):
        self.hyp = [log_c, log_sigma]
        self.para = [d]

    def _n_der(self, x, z):
        return 3

    def _device_params(self):
        d = self.para[0]
        if np.abs(d - np.round(d)) < 1e-8:             # Core/cov.py:640-643
            d = int(round(d))
        assert d >= 1.
        return self._kind, int(d), 0


class LINard(_DotKernel):
    """Linear kernel with ARD: sum_k x_k z_k / ell_k^2 (GPML covLINard), 1e-10 diagonal jitter on 'train'.  hyp = log_ell_list
    (Core/cov.py:1028-1074).  Derivative w.r.t. log ell_k: -2 x_k z_k / ell_k^2.

    Deviation from the reference, which ignores ell on 'train' and 'self_test' and divides by ell once on 'cross' (:1047-1053), so
    that its derivatives do not differentiate its own value; the two agree in every mode at ell = 1, the default hypers.  There is no
    ``reference_compat`` for it.

    Alone it runs on the device with 1 / ell_k folded into the coordinates, for any D with at most 255 hypers.  Not a leaf of a
    device program: trees that contain it combine the children's device-built matrices and fit through the dense route."""
    _kind = _lib.COV_LINARD
    _WRONG_DER = "Wrong derivative index in covLINard"
    _OVER_LIMIT = "pygps_amd: cov.LINard runs on the device for at most 255 length-scales; there is no CPU fallback"

    def __init__(self, D=None, log_ell_list=None):
        if log_ell_list is None:
            self.hyp = [0. for _ in range(D)]
        else:
            self.hyp = log_ell_list
        self.para = []

    def _n_der(self, x, z):
        ref = x if x is not None else z
        return np.shape(ref)[1]                           # Core/cov.py:1063: der < D

    def _program(self, h0):
        return None                                       # its length-scales live in the coordinates of a one-leaf program


def refuse_dot(covfunc, what):
    """FITC and sharded fits assume one scalar k(x, x) for all points; dot-product kernels have none."""
    if isinstance(covfunc, Kernel) and covfunc._dot_leaves():
        raise NotImplementedError("pygps_amd: the dot-product kernels (cov.Linear, cov.Poly, cov.LINard) cannot be used with %s: "
                                  "their k(x, x) differs from point to point" % what)


class SM(Kernel):
    """Gaussian spectral mixture kernel (Wilson & Adams 2013; Core/cov.py:454-619):

        k(x, z) = sum_q w_q prod_j exp(-2 pi^2 v_jq t_j^2) cos(2 pi m_jq t_j),   t_j = x_j - z_j

    hyp = [log w (Q) | log m (D x Q, row-major) | log sqrt(v) (D x Q, row-major)], para = [Q].  For D = 1 this is what the
    reference computes; for D > 1 it is the documented product over the coordinates (GPML's covSM) with the hyper layout of
    the reference's ``getCovMatrix`` for the value and the derivatives alike -- the reference itself sums partial products
    there and decodes ``der`` against a transposed layout (deviations).  The derivative w.r.t. log m_jq is taken in
    the leave-one-out form w E prod_{j' != j} c_j' (-a sin a) instead of the reference's -a tan(a) K: the same away from the
    poles of tan, finite at them.

    Evaluated by tile code of its own on the device (csrc/sqdist_tile.h sm_elem, csrc/grad.hip hadamard_sm_kernel) for
    D <= 16 and Q (1 + 2 D) <= 255; beyond that every call raises.  Not a leaf of a device program: trees that contain it
    (``SM + Noise``, ``SM * RBF``) combine the children's device-built matrices and fit through the dense route."""
    _kind = _lib.COV_SM
    _WRONG_DER = "Wrong derivative entry in SM"
    _BAD_PARA = "SM needs Q >= 1 mixture components"
    _OVER_LIMIT = "pygps_amd: cov.SM runs on the device for D <= 16 and Q (1 + 2 D) <= 255; there is no CPU fallback"
    MAX_D = 16                   # csrc/sqdist_tile.h SM_MAXD: one staged slab of coordinates per tile
    MAX_HYP = 255                # the library's cap on covariance hypers (SM_MAXHYP)

    def __init__(self, Q=0, hyps=[], D=None):
        if D:
            self.hyp = list(np.random.random(Q * (1 + 2 * D)))
        else:
            self.hyp = hyps
        self.para = [Q]

    def initSMhypers(self, x, y):
        """Initialise the hypers as the reference documents it (Core/cov.py:488-519; the reference's own body raises TypeError
        on every call): weights std(y) / Q; per coordinate, means uniform in (0, Nyquist frequency] with Nyquist = 0.5 / (smallest
        non-zero shift), and sqrt(v) = 1 / (largest shift * uniform).  Draws from ``np.random`` in the reference's order
        (per coordinate: ``ranf(Q)`` for the means, then ``ranf(Q)`` for the scales).  Host only."""
        x = np.atleast_2d(np.asarray(x, dtype=float))
        y = np.atleast_2d(np.asarray(y, dtype=float))
        n, D = x.shape
        Q = self.para[0]
        w = np.std(y) / Q
        m = np.ones((D, Q))
        s = np.ones((D, Q))
        for i in range(D):
            shift = np.abs(x[:, i][:, None] - x[:, i][None, :])
            nz = shift[shift > 0]
            minshift = max(nz.min() if nz.size else 1.0, 1e-6)
            maxshift = max(nz.max() if nz.size else 1.0, 1e-6)
            m[i, :] = 0.5 / minshift * np.random.ranf(Q)
            s[i, :] = 1. / np.abs(maxshift * np.random.ranf(Q))
        self.hyp = [float(np.log(w))] * Q + [float(v) for v in np.log(m.ravel())] + [float(v) for v in np.log(s.ravel())]

    def _check_limits(self, D=None):
        Q = int(self.para[0])
        nh = len(self.hyp)
        if D is None and Q > 0:
            D = (nh // Q - 1) // 2
        if D is not None and D > self.MAX_D:
            raise Exception("pygps_amd: cov.SM runs on the device for input dimension D <= %d (got D = %d); there is no CPU "
                            "fallback" % (self.MAX_D, D))
        if nh > self.MAX_HYP or (D is not None and Q * (1 + 2 * D) > self.MAX_HYP):
            raise Exception("pygps_amd: cov.SM runs on the device for Q (1 + 2 D) <= %d hyperparameters (got %d); there is no "
                            "CPU fallback" % (self.MAX_HYP, max(nh, Q * (1 + 2 * (D or 0)))))

    def _device_params(self):
        self._check_limits()
        return self._kind, int(self.para[0]), 0

    def _program(self, h0):
        return None                                       # own tile code, not a functor of one squared distance

    def _dim(self, x, z, mode):
        ref = z if mode == 'self_test' else x
        if ref is None:
            return                                        # _device_eval raises the reference's message
        D = np.shape(ref)[1]
        assert self.para[0] == len(self.hyp) / (1 + 2 * D)        # Core/cov.py:528 (true division: a ragged hyp fails here)
        self._check_limits(D)

    def getCovMatrix(self, x=None, z=None, mode=None):
        self.checkInputGetCovMatrix(x, z, mode)
        self._dim(x, z, mode)
        return self._device_eval(x, z, mode, None)

    def getDerMatrix(self, x=None, z=None, mode=None, der=None):
        self.checkInputGetDerMatrix(x, z, mode, der)
        self._dim(x, z, mode)
        if der < 0 or der >= len(self.hyp):
            raise Exception(self._WRONG_DER)
        return self._device_eval(x, z, mode, der)


class Pre(Kernel):
    """Precomputed kernel matrix (Core/cov.py:1429-1455).  ``M2``: train x train, symmetric.  ``M1``: (train + 1) x test, the
    cross-covariances with the test points; its last row holds the test points' self-covariances.  ``hyp = []``: nothing is
    optimised.  Used alone (with a dummy ``x = zeros((n, 1))``) or inside ``+``, ``*`` and ``* number`` trees.

    ``getCovMatrix`` slices the host arrays as the reference does, after checking that ``x`` / ``z`` have as many rows as the
    matrices (the reference returns all of M1 whatever ``xs`` is and so breaks silently beyond the 1000 test points of one
    of its predict batches, Core/gp.py:395-406; here predict takes any number of test points, all of them at once).

    Inside fits and predict the matrices are a RESIDENT LEAF of the device program: M2 is uploaded once per context and read
    by the assembly and gradient tile kernels on every evaluation, M1 once per predict.  Residency is keyed on per-object
    tokens that change when ``M1`` / ``M2`` are rebound (``k.M2 = ...``); the n^2 doubles are never hashed.  After changing
    an array IN PLACE call ``touch()``.  ``Pre.device_leaf = False`` (class or instance) sends every tree that holds the
    kernel down the dense route instead (K and the derivative matrices built on the host per evaluation): the A/B switch.

    One Pre per device program; a tree with two of them fits through the dense route.  FITC, sharded fits and GPMC refuse it."""
    _kind = _lib.COV_PRE
    #: False: not a leaf of the device program -- every tree holding this kernel takes the dense route
    device_leaf = True
    _token_counter = __import__("itertools").count(1)
    # context handle -> [token of the M2 it holds, token of the M1 it holds].  Contexts live as long as the process (one per
    # device and fit stream, _lib.ctx), so the table is never pruned; an entry is read and written only by the thread that
    # drives that context, under the GIL, so it takes no lock.
    _resident = {}

    def __init__(self, M1, M2):
        self.hyp = []
        self.para = []
        self._M1 = self._M2 = None
        self.M2 = M2
        self.M1 = M1

    @property
    def M1(self):
        return self._M1

    @M1.setter
    def M1(self, value):
        if value is not None:
            value = np.asarray(value)
            if value.ndim != 2:
                raise Exception("cov.Pre: M1 must be a (train + 1) x test matrix")
            if self._M2 is not None and value.shape[0] != self._M2.shape[0] + 1:
                raise Exception("cov.Pre: M1 must have one row more than M2 (its last row holds the test self-covariances): "
                                "M1 is %d x %d, M2 is %d x %d" % (value.shape + self._M2.shape))
        self._M1 = value
        self._tok1 = next(Pre._token_counter)

    @property
    def M2(self):
        return self._M2

    @M2.setter
    def M2(self, value):
        value = np.asarray(value)
        if value.ndim != 2 or value.shape[0] != value.shape[1]:
            raise Exception("cov.Pre: M2 must be a square (train x train) matrix, got shape %s" % (value.shape,))
        if self._M1 is not None and self._M1.shape[0] != value.shape[0] + 1:
            raise Exception("cov.Pre: M1 must have one row more than M2 (its last row holds the test self-covariances): "
                            "M1 is %d x %d, M2 is %d x %d" % (self._M1.shape + value.shape))
        self._M2 = value
        self._tok2 = next(Pre._token_counter)
        self._sym_checked = None

    def _check_symmetric(self):
        """The device program reads M2's lower triangle and mirrors it, the dense route and ``getCovMatrix`` use the whole
        matrix: an asymmetric M2 would fit differently on the two.  Checked once per binding (per token), O(n^2)."""
        if self._sym_checked != self._tok2:
            if not np.allclose(self._M2, self._M2.T, rtol=1e-10, atol=1e-12 * float(np.max(np.abs(self._M2)))):
                raise Exception("cov.Pre: M2 must be symmetric")
            self._sym_checked = self._tok2

    def touch(self):
        """The arrays were changed in place: upload them again before the next fit / predict."""
        self._tok1 = next(Pre._token_counter)
        self._tok2 = next(Pre._token_counter)

    def _check_train(self, x):
        if x is not None and np.shape(x)[0] != self._M2.shape[0]:
            raise Exception("cov.Pre: M2 is %d x %d but there are %d training inputs"
                            % (self._M2.shape[0], self._M2.shape[1], np.shape(x)[0]))

    def _check_test(self, z):
        if self._M1 is None:
            raise Exception("cov.Pre: no M1 (cross-covariances with the test points) was given")
        if z is not None and np.shape(z)[0] != self._M1.shape[1]:
            raise Exception("cov.Pre: M1 has %d columns but there are %d test inputs" % (self._M1.shape[1], np.shape(z)[0]))

    def getCovMatrix(self, x=None, z=None, mode=None):
        if mode == 'self_test':           # Core/cov.py:1443-1445
            self._check_test(z)
            A = self._M1[-1, :]
            return np.reshape(A, (A.shape[0], 1))
        if mode == 'train':               # :1446-1447
            self._check_train(x)
            return self._M2
        if mode == 'cross':               # :1448-1449
            self._check_train(x)
            self._check_test(z)
            return self._M1[:-1, :]
        raise Exception("Specify the mode: 'train' or 'cross'")

    def getDerMatrix(self, x=None, z=None, mode=None, der=None):
        if der is not None:               # Core/cov.py:1453-1455
            raise Exception("Error: NO optimization in precomputed kernel matrix")
        return 0

    def _pre_leaves(self):
        return [self]

    def _on_device(self):
        return bool(self.device_leaf)

    def _program(self, h0):
        if not self.device_leaf:
            return None
        return [_lib.PROG_LEAF, int(self._kind), 0, 0, int(h0)], 1, 1, 0

    def _bind_pre(self, ctx, test=False):
        """Make context ``ctx`` hold this object's M2 (and, for predict, its M1).  Uploads only when the context holds
        something else: another Pre's matrices, or this one's before a rebind / ``touch()``."""
        key = ctx.value if hasattr(ctx, "value") else ctx
        held = Pre._resident.setdefault(key, [None, None])
        n = self._M2.shape[0]
        if held[0] != self._tok2:
            # (predict after another model used the context uploads M2 again although pgp_predict reads M1 alone: pgp_set_pre
            # ties an M1 to the M2 of its n; one n^2 copy per switch between models, none while one model keeps the context)
            self._check_symmetric()
            held[0] = held[1] = None
            _lib.check(_lib.load().pgp_set_pre(ctx, _lib.ptr(_lib.f64(self._M2)), n, None, 0), "pgp_set_pre")
            held[0] = self._tok2
        if test and held[1] != self._tok1:
            held[1] = None
            M1 = _lib.f64(self._M1)
            _lib.check(_lib.load().pgp_set_pre(ctx, None, n, _lib.ptr(M1), M1.shape[1]), "pgp_set_pre")
            held[1] = self._tok1

    def _bind(self, ctx):
        if not self.device_leaf:
            raise NotImplementedError("pygps_amd: cov.Pre with device_leaf = False runs through the dense route only")
        self._bind_pre(ctx)
        return self._kind, 0, 0


def refuse_pre(covfunc, what):
    """FITC, sharded fits and GPMC have no meaning for / no code path with a precomputed matrix."""
    if isinstance(covfunc, Kernel) and covfunc._pre_leaves():
        raise NotImplementedError("pygps_amd: cov.Pre cannot be used with %s" % what)


# ---- composites (Core/cov.py:230-328) ---------------------------------------------------------------------
# A tree whose leaves all have isotropic device functors is evaluated in ONE pass of the tile kernel as a device
# program (sum of products of leaf functors, csrc/sqdist_tile.h CovProgram) -- in getCovMatrix/getDerMatrix and,
# more importantly, inside Exact/EP fits and predict.  Up to TWO leaves may be ARD kernels (RBFard / RQard, D <= 64): each
# gets its own weighted distance, accumulated beside the shared one.  Linear / Poly leaves share ONE further accumulator, the
# dot product (any D), which counts against the same budget of two.  Trees with three ARD leaves (or more than 8 leaves /
# products) still offer getCovMatrix/getDerMatrix by combining the children's device-built matrices.
class _Composite(Kernel):
    _kind = _lib.COV_COMPOSITE

    def _tokens(self):
        pr = self._program(0)
        if pr is None or pr[1] > _lib.PROG_MAX or pr[2] > _lib.PROG_MAX or pr[3] % 1000 > _lib.PROG_MAX:
            return None                                   # too many leaves / products / Scale nodes
        # beside the shared r^2 a program carries at most two more accumulators: one per ARD leaf, one for ALL Linear / Poly leaves
        n_ard, n_dot = pr[3] % 100000 // 1000, pr[3] // 100000
        if n_ard + (1 if n_dot else 0) > 2:
            return None
        if len(self._pre_leaves()) > 1:
            return None                                   # more than one cov.Pre leaf
        if n_dot and self._pre_leaves():
            return None                                   # the Pre tile and the dot product do not share a program
        return pr[0]

    def _bind(self, ctx):
        tok = self._tokens()
        if tok is None:
            raise NotImplementedError(
                "pygps_amd: this composite kernel cannot run as a device program (more than two ARD leaves, an unsupported "
                "leaf, or more than %d leaves/products); there is no CPU fallback" % _lib.PROG_MAX)
        arr = (_lib.C.c_int32 * len(tok))(*tok)
        _lib.check(_lib.load().pgp_set_composite(ctx, arr, len(tok)), "pgp_set_composite")
        for leaf in self._pre_leaves():                   # (one at most on this route) its M2 resident on the same context
            leaf._bind_pre(ctx)
        return _lib.COV_COMPOSITE, 0, 0

    def _on_device(self):
        return self._tokens() is not None

    def _matrices_on_device(self):
        # a cov.Pre leaf is part of the device program of fits and predict; getCovMatrix / getDerMatrix of such a tree combine
        # the children's matrices on the host (Pre slices its arrays, the other leaves are device-built)
        return self._on_device() and not self._pre_leaves()

    def getCovMatrix(self, x=None, z=None, mode=None):
        self.checkInputGetCovMatrix(x, z, mode)
        if self._matrices_on_device():
            return self._device_eval(x, z, mode, None)
        return self._host_cov(x, z, mode)

    def getDerMatrix(self, x=None, z=None, mode=None, der=None):
        self.checkInputGetDerMatrix(x, z, mode, der)
        if der >= len(self.hyp):
            raise Exception(self._WRONG_DER)
        if self._matrices_on_device():
            return self._device_eval(x, z, mode, der)
        return self._host_der(x, z, mode, der)


class _Pair(_Composite):
    _op = None

    def __init__(self, cov1, cov2):
        self.cov1, self.cov2 = cov1, cov2
        self.para = []

    @property
    def hyp(self):
        return list(self.cov1.hyp) + list(self.cov2.hyp)

    @hyp.setter
    def hyp(self, value):
        n1 = len(self.cov1.hyp)
        assert len(value) == n1 + len(self.cov2.hyp)
        self.cov1.hyp = list(value[:n1])
        self.cov2.hyp = list(value[n1:])

    def _pre_leaves(self):
        return self.cov1._pre_leaves() + self.cov2._pre_leaves()

    def _dot_leaves(self):
        return self.cov1._dot_leaves() + self.cov2._dot_leaves()

    def _program(self, h0):
        a = self.cov1._program(h0)
        b = self.cov2._program(h0 + len(self.cov1.hyp))
        if a is None or b is None:
            return None
        nprod = a[2] + b[2] if self._op == _lib.PROG_SUM else a[2] * b[2]
        return a[0] + b[0] + [self._op], a[1] + b[1], nprod, a[3] + b[3]     # [3]: Scale nodes + 1000 per ARD leaf + 100000 per dot leaf


class SumOfKernel(_Pair):
    """Sum of two kernels (Core/cov.py:265-296)."""
    _op = _lib.PROG_SUM
    _WRONG_DER = "Error: der out of range for covSum"

    def _host_cov(self, x, z, mode):
        return self.cov1.getCovMatrix(x, z, mode) + self.cov2.getCovMatrix(x, z, mode)

    def _host_der(self, x, z, mode, der):
        n1 = len(self.cov1.hyp)
        if der < n1:
            return self.cov1.getDerMatrix(x, z, mode, der)
        return self.cov2.getDerMatrix(x, z, mode, der - n1)


class ProductOfKernel(_Pair):
    """Product of two kernels (Core/cov.py:230-261)."""
    _op = _lib.PROG_PRODUCT
    _WRONG_DER = "Error: der out of range for covProduct"

    def _host_cov(self, x, z, mode):
        return self.cov1.getCovMatrix(x, z, mode) * self.cov2.getCovMatrix(x, z, mode)

    def _host_der(self, x, z, mode, der):
        n1 = len(self.cov1.hyp)
        if der < n1:
            return self.cov1.getDerMatrix(x, z, mode, der) * self.cov2.getCovMatrix(x, z, mode)
        return self.cov2.getDerMatrix(x, z, mode, der - n1) * self.cov1.getCovMatrix(x, z, mode)


class ScaleOfKernel(_Composite):
    """Scaled kernel exp(h) * k (Core/cov.py:299-328).  As in the reference, the number given to ``k * number`` IS the
    log-space hyper h (:303), and the derivative w.r.t. h is returned as 2 * exp(h) * k (:324)."""
    _WRONG_DER = "Error: der out of range for covScale"

    def __init__(self, cov, scalar):
        self.cov = cov
        self.para = []
        self._scale = [scalar]

    @property
    def hyp(self):
        return self._scale + list(self.cov.hyp)

    @hyp.setter
    def hyp(self, value):
        assert len(value) == 1 + len(self.cov.hyp)
        self._scale = [value[0]]
        self.cov.hyp = list(value[1:])

    def _pre_leaves(self):
        return self.cov._pre_leaves()

    def _dot_leaves(self):
        return self.cov._dot_leaves()

    def _program(self, h0):
        a = self.cov._program(h0 + 1)
        if a is None:
            return None
        return a[0] + [_lib.PROG_SCALE, int(h0)], a[1], a[2], a[3] + 1

    def _host_cov(self, x, z, mode):
        return np.exp(self._scale[0]) * self.cov.getCovMatrix(x, z, mode)

    def _host_der(self, x, z, mode, der):
        if der == 0:
            return 2. * np.exp(self._scale[0]) * self.cov.getCovMatrix(x, z, mode)
        return np.exp(self._scale[0]) * self.cov.getDerMatrix(x, z, mode, der - 1)


class FITCOfKernel(Kernel):
    """Covariance "function" of the FITC approximation (Core/cov.py:332-390): instead of a full matrix it returns the
    (cross-)covariances with the inducing inputs xu -- 'train': (diag K, Kuu, Ku), 'cross': k(xu, z), 'self_test':
    k(z, z).  inf.FITC_Exact does not call these (the whole fit is one device call); they exist for API parity.

    ``learn_inducing`` (GP_FITC.learnInducing): the FITC fits also return d nlZ / d inducingInput as ``dnlZ.xu`` and the optimiser
    moves the inducing inputs with the hyper-parameters (no reference counterpart; GPML's hyp.xu)."""

    learn_inducing = False
    #: kernels that are a function of one scaled squared distance with a derivative on the device (csrc/sqdist_tile.h cov_dvalue_ds)
    _XU_KINDS = (_lib.COV_RBF, _lib.COV_RBFARD, _lib.COV_RBFUNIT, _lib.COV_RQ, _lib.COV_RQARD, _lib.COV_MATERN)

    def __init__(self, cov, inducingInput):
        refuse_pre(cov, "the FITC approximation (fitc(u) of a precomputed matrix has no meaning)")
        refuse_dot(cov, "the FITC approximation")
        self.inducingInput = np.asarray(inducingInput, dtype=float)
        self.covfunc = cov
        self.para = []

    def _check_learn_inducing(self):
        """Raise unless the gradient w.r.t. the inducing inputs is built for the wrapped kernel (host check, no device work)."""
        k = self.covfunc
        ok = isinstance(k, Kernel) and not isinstance(k, _Composite) and getattr(k, "_kind", None) in self._XU_KINDS
        if ok and k._kind == _lib.COV_MATERN and k._d() == 1:
            ok = False
        if not ok:
            name = type(k).__name__ + (" with d = 1" if isinstance(k, Matern) else "")
            raise NotImplementedError("pygps_amd: learning the inducing inputs is not built for %s (RBF, RBFunit, RBFard, RQ, RQard "
                                      "and Matern d = 3, 5, 7 only; there is no CPU fallback)" % name)

    @property
    def hyp(self):
        return self.covfunc.hyp

    @hyp.setter
    def hyp(self, value):
        self.covfunc.hyp = value

    def _bind(self, ctx):
        return self.covfunc._bind(ctx)

    def _check_dim(self, x):
        if x is not None and self.inducingInput.shape[1] != np.shape(x)[1]:
            raise Exception('Dimensionality of inducing inputs must match training inputs')

    def getCovMatrix(self, x=None, z=None, mode=None):
        self.checkInputGetCovMatrix(x, z, mode)
        xu = self.inducingInput
        self._check_dim(x)
        if mode == 'self_test':
            return self.covfunc.getCovMatrix(z=z, mode='self_test')
        if mode == 'train':
            return (self.covfunc.getCovMatrix(z=x, mode='self_test'), self.covfunc.getCovMatrix(x=xu, mode='train'),
                    self.covfunc.getCovMatrix(x=xu, z=x, mode='cross'))
        return self.covfunc.getCovMatrix(x=xu, z=z, mode='cross')

    def getDerMatrix(self, x=None, z=None, mode=None, der=None):
        self.checkInputGetDerMatrix(x, z, mode, der)
        xu = self.inducingInput
        self._check_dim(x)
        if mode == 'self_test':
            return self.covfunc.getDerMatrix(z=z, mode='self_test', der=der)
        if mode == 'train':
            return (self.covfunc.getDerMatrix(z=x, mode='self_test', der=der),
                    self.covfunc.getDerMatrix(x=xu, mode='train', der=der),
                    self.covfunc.getDerMatrix(x=xu, z=x, mode='cross', der=der))
        return self.covfunc.getDerMatrix(x=xu, z=z, mode='cross', der=der)
