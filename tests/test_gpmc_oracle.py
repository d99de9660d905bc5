"""CPU: the restatement of GPMC's two loops over the oracle's binary fits (tests/gpmc_cpu.py) pinned to the reference's
recordings (G24, tests/golden/make_golden_gpmc.py).  Bars: those tests/test_oracle_golden.py applies to the oracle's EP
(nlZ 1e-10, 1e-9 for a composite tree; predictions 1e-9); sweep / Newton-step counts are equal."""
import numpy as np
import pytest

import gpmc_cpu
import gpmc_data
from conftest import golden, relerr

FIT = ["fit_default", "fit_laplace", "fit_ard_const", "fit_program", "fit_c5_uneven", "fit_c10_d64"]


@pytest.mark.parametrize("name", FIT)
def test_fit_and_predict_restatement_matches_the_reference(name):
    g = golden("G24_" + name)
    x, y, xs = gpmc_data.blobs(**gpmc_data.SHAPES[name])
    kind, hyp, para, c = gpmc_data.oracle_prior(name)
    C = int(g["n_class"])
    votes, nlZ, iters, _ = gpmc_cpu.fit_and_predict(kind, hyp, para, x, y, C, xs, mean=lambda a: c * np.ones((a.shape[0], 1)),
                                                    laplace=name == "fit_laplace")
    P = gpmc_cpu.pairs(C)
    assert len(P) == len(g["pair_nlZ"])
    assert [iters[p] for p in P] == [int(v) for v in g["pair_iters"]]
    bar = 1e-9 if isinstance(kind, tuple) else 1e-10
    for k, p in enumerate(P):
        assert abs(nlZ[p] - g["pair_nlZ"][k]) <= bar * abs(g["pair_nlZ"][k]), p
    assert np.max(np.abs(votes - g["votes"]) / g["votes"]) < 1e-9
    assert np.max(np.abs(votes.sum(axis=1) - 1)) < 1e-14


@pytest.mark.parametrize("name,chained", [("opt_default", False), ("opt_prior", True)])
def test_optimize_and_predict_restatement_matches_the_reference(name, chained):
    """The CG minimiser amplifies rounding differences between two implementations of the same objective, so the bars
    are the project's for optimised results (tests/test_gpu_fitc_ep.py: hypers 1e-3, nlZ 1e-5, predictions 1e-4); what
    the restatement gives on the recording machine is far inside them (hypers 0, nlZ 0, votes 0: it reproduces the
    reference's evaluations bit for bit)."""
    g = golden("G24_" + name)
    x, y, xs = gpmc_data.blobs(**gpmc_data.SHAPES[name])
    kind, hyp0, para, _ = gpmc_data.oracle_prior(name)
    C = int(g["n_class"])
    votes, nlZ, hyps = gpmc_cpu.optimize_and_predict(kind, hyp0, para, x, y, C, xs, chained=chained)
    P = gpmc_cpu.pairs(C)
    for k, p in enumerate(P):
        assert relerr(hyps[p], g["pair_hyp"][k]) < 1e-3, p
        assert abs(nlZ[p] - g["pair_nlZ"][k]) <= 1e-5 * abs(g["pair_nlZ"][k]), p
    assert np.max(np.abs(votes - g["votes"]) / g["votes"]) < 1e-4
    if chained:                                          # the last pair's optimum is what the shared kernel object ends with
        assert relerr(hyps[P[-1]], g["final_cov_hyp"]) < 1e-3
        assert relerr(hyps[P[0]], g["pair_hyp"][-1]) > 1e-2           # ... and the pairs' optima do differ
