"""The long-double reference of leave-one-out inference (tests/loo_ref_ld.py) checked on its own, on the CPU.

(a) The closed form equals n brute-force refits in long double (mu, s2, lp), at n = 12 and 40, for RBF and for the sum kernel
    RBF + Periodic (d = 1) with a constant mean.  Both sides are long double (2^-64) on matrices with cond(K + sn2 I) <= 1e4: the
    bound asserted is 1e-13 of each quantity's scale (measured: <= 1.3e-16).
(b) The reference gradient -- 1/2 sum(S o dK_h) / sn2, tr S, -u' dm -- against central differences of the reference's own
    nlZ_loo in long double with h = 1e-5, for the cov, lik and mean hypers, n = 40.  Measured disagreement relative to the largest
    gradient component: 2.1e-10 (RBF), 1.18e-8 (RBF + Periodic: the periodic leaf's larger third derivative in the h^2 term of
    the difference); asserted at 100 x the measured value, 2.1e-8 and 1.18e-6.
(c) The tolerance rejects every single-slip mutant of the device arithmetic restated in fp64 numpy (loo_ref_ld.device_form64)
    and passes the unmutated form (worst 0.125 of the tolerance).  |mutant - reference| / tol on the field the mutant damages,
    dense route (no bar) / program route (with the kernel's rounding bar), RBF d = 3, n = 129:
        w_neighbour_c 1.6e10 / 7.6e8   mirror_tile 6.6e10 / 2.7e9   u_lower_only 2.0e11 / 3.3e9   g_padding inf / inf
        rank2_sign_tile 3.1e11 / 1.7e10   gg_fp32_chunk 6.0e3 / 321   trace_np 6.3e12 / 1.9e9   s2_unscaled 1.6e14 / 2.9e13
    The weakest rejection is gg_fp32_chunk on the program route at 321 (one 16-deep k-chunk of one tile from fp32 operands).
    Two mutants leave every live output as it is, because g = 0 on the padding makes S exactly zero there: g_padding only
    writes an identity into S's padding rows, so the field it is judged on is Spad, those rows, which must be exact zeros;
    trace_np is the trace over np of a workspace whose padding still holds B^-1's identity (the product not having written
    those rows) -- over a correct S the trace over np equals the trace over n bit for bit.
"""
import numpy as np
import pytest

import kernel_ref_ld as KR
import loo_ref_ld as R
from oracle import gp_oracle as O

LD = R.LD
SUM = ("sum", ("leaf", O.RBF, 0), ("leaf", O.PERIODIC, 0))
KERNELS = dict(rbf=(O.RBF, np.array([0.2, 0.0])), sum=(SUM, np.array([0.2, 0.0, 0.1, 0.3, -0.5])))
LOG_SN = float(np.log(0.2))
MEASURED_FD = dict(rbf=2.1e-10, sum=1.18e-8)        # (b): measured here, see the module docstring


def _data(n, d=1):
    rng = np.random.RandomState(7 + n)
    x = rng.randn(n, d)
    y = np.sin(x.sum(axis=1)) + 0.2 * rng.randn(n) + 0.7
    return x, y


def _b(kind, hyp, x, log_sn):
    sn2 = LD(np.exp(2 * LD(log_sn)))
    K, barK = KR.ref_matrix(kind, hyp, 0, x=x, mode="train")
    B = K / sn2
    B[np.diag_indices_from(B)] += 1
    return K, B, float(sn2)


@pytest.mark.parametrize("n", [12, 40])
@pytest.mark.parametrize("name", ["rbf", "sum"])
def test_closed_form_equals_brute_force(name, n):
    kind, hyp = KERNELS[name]
    x, y = _data(n)
    c = 0.7
    K, B, sn2 = _b(kind, hyp, x, LOG_SN)
    v = R.loo_formulas(R.F.ld_fit(B, y - c, sn2)["Binv"], R.F.ld_fit(B, y - c, sn2)["alpha"], R._ld(y), sn2)
    mu, s2, lp = R.brute_force(K, y, np.full(n, c), sn2)
    worst = {}
    for f, want, scale in (("mu", mu, np.abs(y) + np.abs(v["q"])), ("s2", s2, s2), ("lp", lp, 1 + np.abs(lp))):
        worst[f] = float(np.max(np.abs(v[f] - want) / scale))
    print("loo_ref brute force %s n=%d: %s" % (name, n, worst))
    assert max(worst.values()) <= 1e-13, worst


def _nlz(kind, hyp, x, y, c, log_sn):
    K, B, sn2 = _b(kind, hyp, x, log_sn)
    q = R.F.ld_fit(B, R._ld(y) - LD(c), sn2)
    # (ld_fit rounds r to fp64 first; the mean's difference quotient needs it in long double)
    Binv = q["Binv"]
    alpha = (Binv @ (R._ld(y) - LD(c))) / LD(sn2)
    return R.loo_formulas(Binv, alpha, R._ld(y), sn2), sn2


@pytest.mark.parametrize("name", ["rbf", "sum"])
def test_gradient_against_central_differences(name):
    kind, hyp = KERNELS[name]
    n = 40
    x, y = _data(n)
    c, h = 0.7, 1e-5
    v, sn2 = _nlz(kind, hyp, x, y, c, LOG_SN)
    S = v["S"]
    grad = [np.sum(S * KR.ref_matrix(kind, hyp, 0, x=x, mode="train", der=k)[0]) / (2 * LD(sn2)) for k in range(len(hyp))]
    grad += [np.trace(S), -np.sum(v["u"])]

    def f(dh, dl, dc):
        return _nlz(kind, hyp + dh, x, y, c + dc, LOG_SN + dl)[0]["nlZ"]
    fd = []
    for k in range(len(hyp)):
        e = np.zeros(len(hyp))
        e[k] = h
        fd.append((f(e, 0, 0) - f(-e, 0, 0)) / (2 * LD(h)))
    z = np.zeros(len(hyp))
    fd += [(f(z, h, 0) - f(z, -h, 0)) / (2 * LD(h)), (f(z, 0, h) - f(z, 0, -h)) / (2 * LD(h))]
    grad, fd = np.array(grad, dtype=LD), np.array(fd, dtype=LD)
    rel = float(np.max(np.abs(grad - fd)) / np.max(np.abs(grad)))
    print("loo_ref gradient %s: disagreement %.3g of the largest component" % (name, rel))
    assert rel <= 100 * MEASURED_FD[name], (rel, grad, fd)


_REFS = {}


def _refs(n=129):
    """(dense-route reference: B = K/sn2 + I from the fp64 K, no bar; program-route reference: long-double B with its bar)."""
    if n not in _REFS:
        rng = np.random.RandomState(n)
        x = rng.randn(n, 3)
        y = np.sin(x.sum(axis=1)) + 0.2 * rng.randn(n) + 0.7
        sn2 = float(np.exp(2 * LOG_SN))
        hyp = np.array([np.log(np.sqrt(3.0)), 0.0])
        B, barB = R.program_b(O.RBF, hyp, 0, x, sn2)
        r = y - 0.7
        _REFS[n] = (R.reference(R._f64(B), r, sn2, y=y), R.reference(B, r, sn2, y=y, barB=barB))
    return _REFS[n]


def _cpu_input(ref):
    B64 = R._f64(ref.B)
    Bi = np.linalg.inv(B64)
    Bi = 0.5 * (Bi + Bi.T)
    return Bi, (Bi @ ref.r) / ref.sn2


def test_unmutated_form_passes():
    for ref in _refs():
        Bi, alpha = _cpu_input(ref)
        rr = ref.ratios(R.device_form64(Bi, alpha, ref.y, ref.sn2))
        print("loo_ref unmutated: %s   E_cpu / 2^-53 %s" % (rr, {f: v / R.EPS for f, v in ref.e_cpu.items()}))
        assert max(rr.values()) <= 1.0, rr


WEAKEST = {}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_tolerance_rejects_every_mutant(mutant):
    for route, ref in zip(("dense", "program"), _refs()):
        Bi, alpha = _cpu_input(ref)
        f = R.MUTANT_FIELD[mutant]
        ratio = ref.ratios(R.device_form64(Bi, alpha, ref.y, ref.sn2, mutant=mutant), fields=[f])[f]
        WEAKEST[(mutant, route)] = ratio
        print("loo_ref mutant %-16s %-8s field %-5s ratio %.3g" % (mutant, route, f, ratio))
        assert ratio > 1.0, (mutant, route, ratio)
