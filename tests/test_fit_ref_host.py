"""CPU: the long-double fit reference of tests/fit_ref_ld.py and its tolerance, checked against themselves before the device is
held to them (tests/test_gpu_fit_ld.py).

Two matrices, both through the kernel reference (kernel_ref_ld.ref_matrix) so that the input bar is the program route's:
  rbf700   n = 700, d = 5, RBF at ell = sqrt(d), sn = 0.1: cond(B) = 4e4; 768 padded rows, panels of 512 + 256
  line513  n = 513 sorted points of [0, 1], RBF at ell = 0.05, sn = 0.1: cond(B) = 1e6; one live column in the last panel

* the three fp64 CPU evaluations (LAPACK, blocked_fit64 at panel 512 and 128) sit at <= 1/8 of the tolerance in every field --
  by construction, asserted;
* the first-order bars cover what a perturbation of B by its bar with random signs does to every field;
* every single-slip mutant of blocked_fit64 is rejected (ratio > 1) in the field it damages:
      tu_fp32            one 16-deep k-chunk of one 128 x 128 trailing-update tile from fp32-rounded operands             (L)
      solve_fp32         the same inside a panel solve (rows below the first leaf times its explicit inverse)          (L)
      eet_last_tile      the last panel's share E_p E_p' left out of one 64 x 64 tile of B^-1                          (Binv)
      eet_first_tile     the first panel's share left out of one 64 x 64 tile (the joint product of the first panels)  (Binv)
      e_unsolved         one leaf's rows of E not multiplied by the leaf's inverse                                     (Binv)
      alpha_last_block   alpha = E z / sn2 without z's last 128-block                                                  (alpha)
      logdet_short       the log-determinant without the last pivot                                                    (nlZ)
      binv_ragged        B^-1's last live row read from the padded identity                                            (Binv)
  Smallest rejection factor over both matrices and both panel widths: 95 (tu_fp32 on line513, panel 512, in L; 146 on rbf700);
  every other mutant is rejected by more than 1e5.
* the gap this closes: the same tu_fp32 fit PASSES the suite's max-norm thresholds (1e-8 for L, 1e-7 for alpha, 1e-9 for nlZ: the
  N = 8192 spot sample of tests/test_gpu_core.py) -- L is off by 9.1e-10, alpha by 6.0e-9, nlZ by 6.2e-10 of their max norms --
  and fails the bar on L by 146 x.
"""
import numpy as np
import pytest

import fit_ref_ld as F
from conftest import relerr
from oracle import gp_oracle as O

SN2 = 0.01
_REF = {}
REJECTION = {}


def _case(name):
    if name not in _REF:
        if name == "rbf700":
            x, y = F.P.reg_data(700, 5, 700)
            hyp = np.array([np.log(np.sqrt(5.0)), 0.1])
            r = y.ravel() - y.mean()
        else:
            t, y, _ = F.sorted_1d_matrix(513)
            x = t[:, None]
            hyp = np.array([np.log(0.05), 0.5 * np.log(SN2 * 1e6 / (0.125 * 513))])
            r = y
        B, barB = F.program_b(O.RBF, hyp, 0, x, SN2)
        _REF[name] = (F.reference(B, r, SN2, barB), B, barB, r)
    return _REF[name]


CASES = ("rbf700", "line513")


@pytest.mark.parametrize("name", CASES)
def test_cpu_evaluations_sit_at_an_eighth_of_the_tolerance(name):
    ref, B, barB, r = _case(name)
    cond = np.linalg.cond(F._f64(B))
    assert (2e4 < cond < 8e4) if name == "rbf700" else (5e5 < cond < 2e6), cond
    for form, fit in zip(F.CPU_FORMS, F.cpu_fits(F._f64(B), r, SN2)):
        rr = ref.ratios(fit)
        print("fit_ref %-8s %-12s" % (name, form), " ".join("%s %.3g (E_cpu %.3g eps)" % (f, rr[f][0], ref.e_cpu_form[form][f] / F.EPS)
                                                            for f in F.FIELDS))
        for f in F.FIELDS:
            assert rr[f][0] <= 1.0 / F.SOLVE_FACTOR, (name, form, f, rr[f])
        assert np.all(np.triu(fit["L"], 1) == 0)


@pytest.mark.parametrize("name", CASES)
def test_propagated_bars_cover_a_perturbation_of_b_by_its_bar(name):
    ref, B, barB, r = _case(name)
    rng = np.random.RandomState(5)
    n = ref.n
    S = np.triu(rng.choice([-1.0, 1.0], size=(n, n)))
    S = S + np.triu(S, 1).T
    q = F.ld_fit(B + F._ld(S * barB), r, SN2)
    for f in F.FIELDS:
        d = np.abs(q[f] - getattr(ref, f)).astype(np.float64)
        bar = ref.bar[f]
        if f == "L":
            d, bar = d[ref.low], bar[ref.low]
        worst = float(np.max(d / bar))
        print("fit_ref %-8s bar of %-6s covers the perturbation: %.3g" % (name, f, worst))
        # L_00 = sqrt(B_00) moves by exactly its bar; the long-double difference of two factors is itself rounded at 2^-64 |L|,
        # up to 2^-64 / (16 2^-53) = 3e-5 of a bar of 16 ulps
        assert worst <= 1.0 + 1e-4, (name, f, worst)
        assert worst > 1e-4, (name, f, worst)            # ... and is no gross overestimate: random signs reach this much of it


@pytest.mark.parametrize("panel", [512, 128])
@pytest.mark.parametrize("mutant", F.MUTANTS)
@pytest.mark.parametrize("name", CASES)
def test_single_slip_mutants_are_rejected(name, mutant, panel):
    ref, B, barB, r = _case(name)
    fit = F.blocked_fit64(F._f64(B), r, SN2, F.LEAF, panel, mutant=mutant)
    f = F.MUTANT_FIELD[mutant]
    worst = ref.ratios(fit)[f][0]
    REJECTION[(name, mutant, panel)] = worst
    print("fit_ref %-8s panel %3d mutant %-17s rejected in %-5s by %.3g" % (name, panel, mutant, f, worst))
    assert worst > 1.0, (name, mutant, panel, f, worst)


def test_the_fp32_chunk_passes_the_max_norm_thresholds_and_fails_the_bar():
    """The gap: one fp32 k-chunk in one trailing tile is invisible to 1e-8 / 1e-7 / 1e-9 in the max norm."""
    ref, B, barB, r = _case("rbf700")
    fit = F.blocked_fit64(F._f64(B), r, SN2, F.LEAF, F.PANEL, mutant="tu_fp32")
    eL, ea, ez = relerr(fit["L"], F._f64(ref.L)), relerr(fit["alpha"], F._f64(ref.alpha)), relerr(fit["nlZ"], float(ref.nlZ))
    rr = ref.ratios(fit)
    print("fit_ref tu_fp32 on rbf700: max-norm errors L %.3g alpha %.3g nlZ %.3g; ratios" % (eL, ea, ez),
          " ".join("%s %.3g" % (f, rr[f][0]) for f in F.FIELDS))
    assert eL < 1e-8 and ea < 1e-7 and ez < 1e-9
    assert rr["L"][0] > 1.0


def test_large_n_functionals_reject_the_mutants_too():
    """The O(n^2) functionals of the large-n cases on rbf700, with the probes used at size (fit_ref_ld.default_probes): the CPU
    fits pass by construction, a mutant fit fails the functional that sees its field."""
    ref, B, barB, r = _case("rbf700")
    B64 = F._f64(B)
    lref = F.large_reference(B64, r, SN2, probes=F.default_probes(700))
    for form, fit in zip(F.CPU_FORMS, F.cpu_fits(B64, r, SN2)):
        rr = F.large_ratios(lref, B64, fit)
        assert max(rr.values()) <= 1.0 / F.SOLVE_FACTOR, (form, rr)
    # (eet_last_tile drops a 64-tile that none of the default rows crosses: the +-1 vector is the probe that sees every tile)
    sees = dict(tu_fp32="resid_col", solve_fp32="resid_col", eet_last_tile="inv_vec", eet_first_tile="left_inv_row", e_unsolved="left_inv_row",
                alpha_last_block="solve_resid", logdet_short="nlZ", binv_ragged="left_inv_row")
    for mutant, fn in sees.items():
        fit = F.blocked_fit64(B64, r, SN2, F.LEAF, F.PANEL, mutant=mutant)
        rr = F.large_ratios(lref, B64, fit)
        print("fit_ref large-n functionals, mutant %-17s" % mutant, " ".join("%s %.3g" % kv for kv in rr.items()))
        assert rr[fn] > 1.0, (mutant, rr)


def test_gradient_term_against_a_plain_sum():
    ref, B, barB, r = _case("line513")
    rng = np.random.RandomState(1)
    dK = rng.randn(513, 513)
    dK = dK + dK.T
    val, tol = ref.grad_term(dK)
    Q = F._f64(ref.Binv) / SN2 - np.outer(F._f64(ref.alpha), F._f64(ref.alpha))
    assert abs(0.5 * float(np.sum(Q * dK)) - float(val)) <= tol
