// Laplacian likelihood, EP-mode moments -- reference: Core/lik.py Laplace.evaluate :432-512, _lerfc :519-531,
// _expABz_expAx :533-544, _logphi :546-559, _logsum2exp :561-572.  Shared by the EP site chains (csrc/ep.hip), the
// per-site terms and gradients of EP, and the test hook (csrc/testhooks.hip).
//
//   p(y | f) = exp(-|y - f| / b) / (2 b),   b = sn / sqrt 2,   sn = exp(hyp[0])
//   Z(y, mu, s2) = int p(y | f) N(f | mu, s2) df;  lZ, dlZ, d2lZ = log Z and its derivatives in mu;  dlZhyp = d lZ / d log sn.
//
// Three regimes, as in the reference (fac = 1e3):
//   idlik  fac sn < sqrt s2:   the likelihood is narrow against the cavity: Z -> N(y | mu, s2 + sn^2) (sn^2 = 2 b^2 is the
//                              Laplacian's variance).
//   idgau  fac sqrt s2 < sn:   the Gaussian is a delta peak: Z -> p(y | mu).
//   interior: the reference's log-space formulation (two log Phi / log erfc terms combined by logsum2exp / expABz_expAx).
// Deviations from the reference, deliberately:
//   - idlik, value mode: the reference evaluates lik.Gauss in PREDICTION mode with (y, mu) swapped and indexes the single
//     returned array as if it were (lZ, dlZ, d2lZ), which raises IndexError.  Here: lik.Gauss's EP moments with the
//     Laplacian's variance, lZ = log N(y | mu, s2 + sn^2), dlZ = (y - mu) / (s2 + sn^2), d2lZ = -1 / (s2 + sn^2).  The bare
//     delta-peak limit (s2 alone) would give the EP site update 1 + d2lZ / tau_ni = 0, an infinite site precision; this one
//     gives ttau = 1 / sn^2.  (Derivative mode: 0, as the reference; the exact derivative of this limit is below 1e-6.)
//   - idgau: the reference calls Laplace(log_hyp=...), a keyword the constructor does not have (TypeError).  Here: the
//     Laplace log-density at mu and its derivatives, lZ = -|y - mu| / b - log 2b, dlZ = sign(y - mu) / b, d2lZ = 0, and for
//     dlZhyp the Laplace-mode lp_dhyp = |y - mu| / b - 1.
//   - value mode is a per-site function here; the reference's vector calls with nargout >= 2 take the first site's dlZ for
//     every site (_expABz_expAx returns y[0]) and fail for nargout = 3 (reshape to (1, 2)).
#pragma once
#include <cmath>
#ifdef __HIPCC__
#define PGP_HD __host__ __device__
#else
#define PGP_HD
#endif

#define LAP_SQRT2 1.4142135623730951
#define LAP_FAC 1e3

// log Phi(z) (lik.py:546-559): asymptotic expansion below -6.2, logistic blend on [-6.2, -5.5]
PGP_HD inline double lap_logphi(double z) {
    const double zmin = -6.2, zmax = -5.5;
    if (z > zmax) return log(0.5 * (1.0 + erf(z / LAP_SQRT2)));
    const double asym = -0.5 * (log(M_PI) + z * z) - log(sqrt(2.0 + 0.5 * (z * z)) - z / LAP_SQRT2);
    if (z < zmin) return asym;
    const double lam = 1.0 / (1.0 + exp(25.0 * (0.5 - (z - zmin) / (zmax - zmin))));
    return (1.0 - lam) * asym + lam * log(0.5 * (1.0 + erf(z / LAP_SQRT2)));
}

// log erfc(t) (lik.py:519-531): the tight bound above 25, a logistic blend on [20, 25]
PGP_HD inline double lap_lerfc(double t) {
    const double tmin = 20.0, tmax = 25.0;
    if (t < tmin) return log(erfc(t));
    const double bound = log(2.0 / sqrt(M_PI)) - t * t - log(t + sqrt(t * t + 4.0 / M_PI));
    if (t > tmax) return bound;
    const double lam = 1.0 / (1.0 + exp(12.0 * (0.5 - (t - tmin) / (tmax - tmin))));
    return lam * bound + (1.0 - lam) * log(erfc(t));
}

// (exp(a1) b1 + exp(a2) b2) / (exp(a1) + exp(a2)) with the maximum subtracted (lik.py:533-544, two columns)
PGP_HD inline double lap_expABz_expAx(double a1, double a2, double b1, double b2) {
    const double mx = a1 > a2 ? a1 : a2;
    const double e1 = exp(a1 - mx), e2 = exp(a2 - mx);
    return (e1 * b1 + e2 * b2) / (e1 + e2);
}

// log(exp(a1) + exp(a2)) with the maximum subtracted (lik.py:561-572)
PGP_HD inline double lap_logsum2exp(double a1, double a2) {
    const double mx = a1 > a2 ? a1 : a2;
    return log(exp(a1 - mx) + exp(a2 - mx)) + mx;
}

// value mode (lik.py:450-487): lZ, dlZ, d2lZ at the cavity (y, mu, s2) for noise sn; dlZ / d2lZ may be null
PGP_HD inline void laplace_ep_moments(double y, double mu, double s2, double sn, double* lZ, double* dlZ, double* d2lZ) {
    if (LAP_FAC * sn < sqrt(s2)) {                                     // idlik: the Gaussian limit, lik.Gauss's EP mode
        const double r = y - mu, v = sn * sn + s2;
        *lZ = -r * r / v / 2.0 - log(2.0 * M_PI * v) / 2.0;
        if (dlZ) *dlZ = r / v;
        if (d2lZ) *d2lZ = -1.0 / v;
        return;
    }
    if (LAP_FAC * sqrt(s2) < sn) {                                     // idgau: the Laplace density at mu
        const double b = sn / LAP_SQRT2, r = y - mu;
        *lZ = -fabs(r) / b - log(2.0 * b);
        if (dlZ) *dlZ = (r > 0.0 ? 1.0 : (r < 0.0 ? -1.0 : 0.0)) / b;
        if (d2lZ) *d2lZ = 0.0;
        return;
    }
    // substitution to unit variance, zero mean Laplacian
    const double tvar = s2 / (sn * sn + 1e-16);
    const double tmu = (mu - y) / (sn + 1e-16);
    const double stv = sqrt(tvar);
    const double zp = (tmu + LAP_SQRT2 * tvar) / stv;
    const double zm = (tmu - LAP_SQRT2 * tvar) / stv;
    const double lpp = lap_logphi(-zp), lpm = lap_logphi(zm);
    const double ap = lpp + LAP_SQRT2 * tmu;
    const double am = lpm - LAP_SQRT2 * tmu;
    *lZ = lap_logsum2exp(ap, am) + tvar - log(sn * LAP_SQRT2);
    if (!dlZ && !d2lZ) return;
    const double hl2pi = 0.5 * log(2.0 * M_PI);
    const double lqp = -0.5 * (zp * zp) - hl2pi - lpp;                // log(N(zp) / Phi(-zp))
    const double lqm = -0.5 * (zm * zm) - hl2pi - lpm;
    const double hls2 = 0.5 * log(s2);
    const double dap = -exp(lqp - hls2) + LAP_SQRT2 / sn;
    const double dam = exp(lqm - hls2) - LAP_SQRT2 / sn;
    const double d1 = lap_expABz_expAx(ap, am, dap, dam);
    if (dlZ) *dlZ = d1;
    if (d2lZ) {
        const double a = sqrt(8.0) / sn / sqrt(s2);
        const double bp = 2.0 / (sn * sn) - (a - zp / s2) * exp(lqp);
        const double bm = 2.0 / (sn * sn) - (a + zm / s2) * exp(lqm);
        *d2lZ = lap_expABz_expAx(ap, am, bp, bm) - d1 * d1;
    }
}

// derivative mode (lik.py:488-512): d lZ / d log sn at the cavity (y, mu, s2)
PGP_HD inline double laplace_ep_dlZhyp(double y, double mu, double s2, double sn) {
    if (LAP_FAC * sn < sqrt(s2)) return 0.0;                          // idlik
    if (LAP_FAC * sqrt(s2) < sn) return fabs(y - mu) / (sn / LAP_SQRT2) - 1.0;   // idgau: Laplace-mode lp_dhyp
    const double tmu = (mu - y) / (sn + 1e-16), tvar = s2 / (sn * sn + 1e-16);
    const double stv = sqrt(tvar), ss2 = sqrt(s2);
    const double zp = (tvar + tmu / LAP_SQRT2) / stv, vp = tvar + LAP_SQRT2 * tmu;
    const double zm = (tvar - tmu / LAP_SQRT2) / stv, vm = tvar - LAP_SQRT2 * tmu;
    const double dzp = (-s2 / sn + tmu * sn / LAP_SQRT2) / ss2;
    const double dvp = -2.0 * tvar - LAP_SQRT2 * tmu;
    const double dzm = (-s2 / sn - tmu * sn / LAP_SQRT2) / ss2;
    const double dvm = -2.0 * tvar + LAP_SQRT2 * tmu;
    const double lezp = lap_lerfc(zp), lezm = lap_lerfc(zm);
    const double xp = vp + lezp, xm = vm + lezm;
    const double vmax = xp > xm ? xp : xm;
    const double ep = exp(xp - vmax), em = exp(xm - vmax);
    const double c = 2.0 / sqrt(M_PI);
    const double dap = ep * (dvp - c * exp(-(zp * zp) - lezp) * dzp);
    const double dam = em * (dvm - c * exp(-(zm * zm) - lezm) * dzm);
    return (dap + dam) / (ep + em) - 1.0;
}
