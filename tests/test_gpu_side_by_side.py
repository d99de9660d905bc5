"""GPU: exact fits that run SIDE BY SIDE on two fit streams of one device (two host threads, one context each -- the mode bench.py
times with --streams 2 and the restart / K-fold searches put their users in) against the LONE fit of the same step, bit for bit.

The two contexts share the device's yield table, the device gate and the once-per-process state of the library; nothing here is a
tolerance: the kernels, their tiles and the k-order inside a tile do not depend on what runs beside them, so any difference between
a fit beside a neighbour and the same fit alone is a bug.  The only tolerances in this file are the existing ones against the
reference's own numbers (G6, tests/test_gpu_core.py).

`run_side_by_side` is the harness; it FAILS ("did not run side by side") when the host intervals of the paired calls do not
intersect, so that no test passes because the calls serialised."""
import contextlib
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from conftest import ROOT, golden, relerr, synth_cls, synth_reg

pytestmark = pytest.mark.gpu

D = 16
N_BARRIER = 6                      # barrier-released fits per thread, and as many free-running ones behind them
G6 = "G6"                          # the step at the reference's own (unperturbed) hyper-parameters, N = 8192 only
OPTION_DEFAULTS = {"sched": -1, "nb_outer": 0, "predict_inverse": 1, "tud_tile": 64}


def hyp_for(step, rank=0, d=D):
    """bench.py hyp_for: the cfg-2 point, nudged so that no two steps repeat."""
    eps = 1e-3 * ((step * 7 + rank * 13) % 101) / 101.0
    return np.array([np.log(np.sqrt(d)) + eps, 0.0 - eps]), float(np.log(0.1) + 0.5 * eps)


_DATA = {}


def _data(N):
    if N not in _DATA:
        x, y = synth_reg(N, D)
        x = np.ascontiguousarray(x)
        yv = np.ascontiguousarray(y).ravel()
        _DATA[N] = (x, yv, np.full(N, yv.mean()), np.ones((1, N)))
    return _DATA[N]


def _step_inputs(N, step):
    """(x, y, mean vector, dm, cov hyp, log sn) of one step: bench.py's constant mean y.mean(), or G6's own numbers."""
    x, yv, m, dm = _data(N)
    if step == G6:
        g = golden("G6_rbf_d16_N%d" % N)
        return x, yv, float(g["mean_hyp"][0]) * np.ones(N), dm, np.array(g["cov_hyp"], dtype=float), float(g["lik_hyp"][0])
    hyp, log_sn = hyp_for(step, 0, D)
    return x, yv, m, dm, hyp, log_sn


def exact_fit(lib, x, yv, m, dm, hyp, log_sn, factor=False, status_only=False):
    """One pgp_exact_fit (RBF, want = 3) through the C ABI on the calling thread's context, as _fit in tests/test_gpu_core.py does.
    status_only: the raw return code of pgp_exact_fit instead of the results."""
    from pygps_amd import _lib, inf
    ctx = _lib.ctx()                                  # the thread's slot; inside concurrent_fit_streams() this sets the hint on it
    n, d = x.shape
    _lib.check(lib.pgp_set_data(ctx, _lib.ptr(x), n, d, _lib.ptr(yv)))
    inf._Resident.key.pop((_lib.default_device(), _lib.current_slot()), None)     # the package's record of what this context holds
    hyp = _lib.f64(hyp)
    nmean = 0 if dm is None else dm.shape[0]
    alpha = np.zeros(n); nlZ = np.zeros(1); dn = np.zeros(nmean + len(hyp) + 1)
    fh = C.c_void_p()
    rc = lib.pgp_exact_fit(ctx, _lib.COV_RBF, _lib.ptr(hyp), len(hyp), 0, 0, float(log_sn), _lib.ptr(m), _lib.ptr(dm), nmean, 3,
                           _lib.ptr(alpha), _lib.ptr(nlZ), _lib.ptr(dn), C.byref(fh) if factor else None)
    if status_only:
        return rc
    _lib.check(rc)
    out = dict(nlZ=nlZ, alpha=alpha, dnlZ=dn)
    if factor:
        L = np.empty((n, n))
        try:
            _lib.check(lib.pgp_factor_to_host(ctx, fh, _lib.ptr(L)))
        finally:
            lib.pgp_factor_free(ctx, fh)
        out["L"] = L
    return out


def step_job(lib, N, step, factor=False):
    """factor "sample": the factor is downloaded, and only G6's sample of its entries kept (a factor is 0.5 GB on the host)."""
    args = _step_inputs(N, step)
    if factor != "sample":
        return lambda: exact_fit(lib, *args, factor=factor)
    idx = golden("G6_rbf_d16_N%d" % N)["L_flat_idx"]

    def job():
        r = exact_fit(lib, *args, factor=True)
        r["L_sample"] = r.pop("L").ravel()[idx]
        return r
    return job


def run_side_by_side(jobs, n_barrier=None, hint=False, join_timeout=180.0):
    """jobs[k]: the callables of host thread k, run in order inside _lib.fit_stream(k) (hint: and inside
    _lib.concurrent_fit_streams()).  The first n_barrier calls of every thread (default: the first half) are released together by a
    barrier, pair by pair; the rest run free, so that the relative phase of the threads drifts.  Returns (results, intervals):
    results[k][i] what jobs[k][i] returned, intervals[k][i] = (perf_counter on entry, on exit).  An exception of a thread is raised
    here; threads that do not finish in join_timeout seconds fail the test (they are daemons: nothing waits for them again).
    With two or more threads, all but one of the barrier-released pairs must intersect on the host clock."""
    from pygps_amd import _lib
    nthr = len(jobs)
    if n_barrier is None:
        n_barrier = min(len(j) for j in jobs) // 2
    assert all(len(j) >= n_barrier for j in jobs)
    barrier = threading.Barrier(nthr)
    results = [[None] * len(j) for j in jobs]
    intervals = [[None] * len(j) for j in jobs]
    errs = []

    def body(k):
        try:
            with _lib.fit_stream(k), (_lib.concurrent_fit_streams() if hint else contextlib.nullcontext()):
                for i, f in enumerate(jobs[k]):
                    if i < n_barrier:
                        barrier.wait(timeout=join_timeout)
                    t0 = time.perf_counter()
                    results[k][i] = f()
                    intervals[k][i] = (t0, time.perf_counter())
        except BaseException as e:                                   # noqa: B902 -- handed to the main thread below
            errs.append((k, e))
            barrier.abort()

    ths = [threading.Thread(target=body, args=(k,), daemon=True) for k in range(nthr)]
    deadline = time.monotonic() + join_timeout
    [t.start() for t in ths]
    for t in ths:
        t.join(max(0.0, deadline - time.monotonic()))
    stuck = [k for k, t in enumerate(ths) if t.is_alive()]
    if stuck:
        pytest.fail("host threads %s did not finish within %.0f s" % (stuck, join_timeout), pytrace=False)
    real = [e for _, e in errs if not isinstance(e, threading.BrokenBarrierError)]
    if real or errs:
        raise (real or [e for _, e in errs])[0]
    if nthr >= 2 and n_barrier > 0:
        met = 0
        for i in range(n_barrier):
            lo = max(intervals[k][i][0] for k in range(nthr))
            hi = min(intervals[k][i][1] for k in range(nthr))
            met += lo < hi
        if met < n_barrier - 1:
            pytest.fail("did not run side by side: only %d of %d barrier-released step pairs intersect on the host clock: %r"
                        % (met, n_barrier, [[(round(1e3 * (a - intervals[0][0][0]), 3), round(1e3 * (b - intervals[0][0][0]), 3))
                                             for a, b in iv[:n_barrier]] for iv in intervals]), pytrace=False)
    return results, intervals


@contextlib.contextmanager
def options(lib, slots, **opts):
    """pgp_set_option on the contexts of the given fit-stream slots; every option back to its default on the way out."""
    from pygps_amd import _lib
    hs = [_lib.ctx(slot=s) for s in slots]
    try:
        for h in hs:
            for k, v in opts.items():
                _lib.check(lib.pgp_set_option(h, k.encode(), int(v)))
        yield hs
    finally:
        for h in hs:
            for k in opts:
                lib.pgp_set_option(h, k.encode(), OPTION_DEFAULTS[k])


# ---- the lone reference: slot 0, no second thread, the effective schedule set explicitly; computed once per (N, schedule, panel
# width, step) and shared (the factors are not kept: 0.5 GB each) -----------------------------------------------------------------
_LONE = {}
SMALL = ("nlZ", "alpha", "dnlZ")


def effective_sched(N):
    """What sweep_plan makes of the hint `concurrent_streams`: sched 1 from nblk = 56 on, the default schedule below."""
    return 1 if (N + 127) // 128 >= 56 else -1


def lone(lib, N, sched, nb_outer, steps, factor_steps=(), **more):
    """{step: results} of lone fits on slot 0; the steps of factor_steps carry "L".  A step that was computed before is not run
    again unless its factor is asked for -- and then has to reproduce what it gave the first time."""
    out = {}
    with options(lib, (0,), sched=sched, nb_outer=nb_outer, **more):
        for s in steps:
            key = (N, sched, nb_outer, s) + tuple(sorted(more.items()))
            if key not in _LONE or s in factor_steps:
                r = step_job(lib, N, s, factor=s in factor_steps)()
                small = {k: r[k] for k in SMALL}
                if key in _LONE:
                    assert_same(small, _LONE[key], "lone fit repeated, step %s" % (s,))
                _LONE[key] = small
                out[s] = r
            else:
                out[s] = _LONE[key]
    return out


def assert_same(got, ref, what, keys=SMALL):
    for k in keys:
        assert np.array_equal(got[k], ref[k]), "%s: %s differs (max |diff| %.3g)" % (what, k, float(np.max(np.abs(got[k] - ref[k]))))


def yield_table(lib, slots=(1, 0)):
    """The device's yield table once the contexts of all slots are idle (the hook drains the streams of the context it is given)."""
    from pygps_amd import _lib
    tab = np.empty(4096, dtype=np.uint32)
    for s in slots:
        tab[:] = 0xFFFFFFFF
        assert lib.pgp_test_yield_table(_lib.ctx(slot=s), tab.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    return tab


def assert_yield_table_clear(lib):
    tab = yield_table(lib)
    bad = np.flatnonzero(tab)
    assert bad.size == 0, "yield marks left behind (CU key: count) %r" % ({int(i): int(tab[i]) for i in bad[:16]},)


def thread_steps(k, extra=()):
    """Thread k's steps: k, k + 2, ... -- even steps on thread 0, odd ones on thread 1, so the two contexts never hold the same
    numbers at the same time; N_BARRIER (+ extra) barrier-released, then as many free-running."""
    a = [k + 2 * i for i in range(N_BARRIER)] + list(extra)
    b = [k + 2 * (N_BARRIER + i) for i in range(N_BARRIER)] + list(extra)
    return a, b


def good_fit_jobs(lib, N, k, extra=(), factor=True):
    """Thread k's jobs of a side-by-side run of good fits, and the step of each; the last barrier-released bench step downloads L."""
    a, b = thread_steps(k, extra)
    l_step = a[N_BARRIER - 1]
    steps = a + b
    jobs = [step_job(lib, N, s, factor="sample" if s == G6 else (factor and i == N_BARRIER - 1)) for i, s in enumerate(steps)]
    return jobs, steps, len(a), l_step


def assert_thread_equals_lone(results, steps, ref, what):
    for r, s in zip(results, steps):
        assert_same(r, ref[s], "%s, step %s" % (what, s))
        if "L" in r:
            assert np.array_equal(r["L"], ref[s]["L"]), "%s, step %s: the factor differs" % (what, s)
        if "L_sample" in r:
            assert np.array_equal(r["L_sample"], ref[s]["L"].ravel()[golden("G6_rbf_d16_N8192")["L_flat_idx"]]), (what, s)


SIDE_BY_SIDE_CASES = [
    pytest.param(7168, "hint", 0, id="N7168-hint"),                  # nblk = 56: the first size where the hint becomes sched 1; 14 panels
    pytest.param(7168, "hint", 8, id="N7168-hint-nb_outer8"),        # 1024-wide panels under sched 1
    pytest.param(8192, "sched1", 0, id="N8192-sched1"),              # what bench.py sets: explicit sched = 1 on both contexts, no hint
    pytest.param(4608, "hint", 0, id="N4608-hint"),                  # nblk = 36: the hint falls back to the default (sched 2, s_pan, two Dk halves)
    pytest.param(7040, "hint", 6, id="N7040-hint-nb_outer6"),        # nblk = 55, one below the threshold: 768-wide panels and a partial last one under sched 0
    pytest.param(7100, "hint", 6, id="N7100-hint-nb_outer6"),        # ragged: np = 7168 with 68 padding rows, sched 1, a partial last panel
]


@pytest.mark.parametrize("N,mode,nb_outer", SIDE_BY_SIDE_CASES)
def test_two_exact_fits_side_by_side_equal_the_lone_fit(lib, N, mode, nb_outer):
    """Two host threads, one context each, 6 barrier-released + 6 free-running fits per thread (thread 0 the even steps of bench.py's
    hyp_for, thread 1 the odd ones): nlZ, alpha and dnlZ of EVERY step, and the factor of each thread's last barrier-released step,
    equal the lone fit of that step on slot 0 (no second thread, the same effective schedule set explicitly) bit for bit; afterwards
    the device's yield table is all zeros.  In the N = 8192 case each thread also fits G6's own hyper-parameters beside the other
    one, and that fit meets the tolerances of test_cholesky_sweep_variants_agree_with_the_reference against the reference's numbers
    (Core/inf.py:353-384): the benchmark's point, in the benchmark's mode."""
    extra = (G6,) if N == 8192 else ()
    sched = 1 if mode == "sched1" else effective_sched(N)
    per_thread = [good_fit_jobs(lib, N, k, extra) for k in range(2)]
    all_steps = sorted({s for _, st, _, _ in per_thread for s in st if s != G6}) + list(extra)
    ref = lone(lib, N, sched, nb_outer, all_steps, factor_steps=[p[3] for p in per_thread] + list(extra))
    with options(lib, (0, 1), nb_outer=nb_outer, sched=1 if mode == "sched1" else -1):
        results, _ = run_side_by_side([p[0] for p in per_thread], n_barrier=per_thread[0][2], hint=mode == "hint")
        assert_yield_table_clear(lib)
    for k in range(2):
        assert_thread_equals_lone(results[k], per_thread[k][1], ref, "thread %d" % k)
    if extra:
        g = golden("G6_rbf_d16_N%d" % N)
        for got in [ref[G6]] + [r for k in range(2) for r, s in zip(results[k], per_thread[k][1]) if s == G6]:
            assert relerr(got["nlZ"][0], g["nlZ"]) < 1e-9
            assert relerr(got["alpha"][g["alpha_idx"]], g["alpha_sample"]) < 1e-7
            assert relerr(got["dnlZ"], np.concatenate([g["dnlZ_mean"], g["dnlZ_cov"], g["dnlZ_lik"]])) < 1e-7
            assert relerr(got["L_sample"] if "L_sample" in got else got["L"].ravel()[g["L_flat_idx"]], g["L_sample"]) < 1e-8


@pytest.mark.parametrize("N", [7168, 8192])
def test_schedules_of_the_sweep_against_each_other(lib, N):
    """Lone fits on slot 0, two steps, nlZ, alpha, dnlZ and the whole factor.  What holds, and is asserted:
      * every schedule reproduces itself bit for bit (sched = 1, sched = 0, the default);
      * sched = 1 and sched = 0 give the same bits: the same launches with the same arguments, queued on other streams;
      * the default schedule (sched 2 at these sizes) does NOT give those bits.  The one launch that differs is TU_d, the next
        panel's diagonal block: 64-tiles, which start their accumulators from C, where TU_a's 128 x 128 LDS-DMA tiles of sched 0 / 1
        fold C in during the k-loop ("lazy C", csrc/gemm_tile.h) -- another order of the same sum.  With tud_tile = 128 the default
        schedule gives sched 1's bits.  As it ships it agrees with sched 1 within the tolerances the suite holds every schedule to
        against the reference's own numbers (test_cholesky_sweep_variants_agree_with_the_reference: nlZ 1e-9, alpha 1e-7, dnlZ
        1e-7, L 1e-8), here over the WHOLE of alpha and L.  Largest relative differences seen on an MI355X (N = 7168 / 8192, steps
        0 / 1): nlZ 1.6e-15, alpha 3.9e-13, dnlZ 3.1e-14, L 1.3e-14."""
    keys = SMALL + ("L",)
    tol = dict(nlZ=1e-9, alpha=1e-7, dnlZ=1e-7, L=1e-8)
    for s in (0, 1):
        base = lone(lib, N, 1, 0, (s,), factor_steps=(s,))[s]
        for sched, more in ((1, {}), (0, {}), (-1, {}), (-1, dict(tud_tile=128))):
            if sched != 1:
                got = lone(lib, N, sched, 0, (s,), factor_steps=(s,), **more)[s]
                what = "N %d, step %d, sched %d %s against sched 1" % (N, s, sched, more)
                rel = {k: relerr(got[k], base[k]) for k in keys}
                print(what, rel)
                if sched == -1 and not more:
                    for k in keys:
                        assert rel[k] < tol[k], (what, k, rel[k])
                else:
                    assert_same(got, base, what, keys)
            else:
                got = base
            if not more:
                again = lone(lib, N, sched, 0, (s,), factor_steps=(s,))[s]
                assert_same(again, got, "N %d, step %d, sched %d against itself" % (N, s, sched), keys)
                del again
            del got


def test_a_neighbour_that_is_not_positive_definite(lib):
    """Thread 1 fits duplicated rows at log sf = 40, log sn = -40 on every step (the construction at the end of
    test_exact_fit_matern_and_nonpd, at N = 7168): pgp_exact_fit returns a status > 0 and its NaNs have run through chain kernels
    that mark the shared yield table.  Thread 0's good fits beside it equal the lone fits bit for bit, the table is clear
    afterwards, and a good lone fit on slot 1 then equals slot 0's."""
    from pygps_amd import _lib
    N = 7168
    jobs0, steps0, nb, l_step = good_fit_jobs(lib, N, 0)
    ref = lone(lib, N, effective_sched(N), 0, steps0 + [1], factor_steps=[l_step])
    xx = np.zeros((N, D)); yy = np.zeros(N); mz = np.zeros(N)
    bad_fit = lambda: exact_fit(lib, xx, yy, mz, None, np.array([0.0, 40.0]), -40.0, status_only=True)
    results, _ = run_side_by_side([jobs0, [bad_fit] * len(jobs0)], n_barrier=nb, hint=True)
    assert_yield_table_clear(lib)
    assert all(isinstance(rc, int) and rc > 0 for rc in results[1]), results[1]
    assert_thread_equals_lone(results[0], steps0, ref, "thread 0 beside the failing fits")
    with options(lib, (1,), sched=effective_sched(N)), _lib.fit_stream(1):
        assert_same(step_job(lib, N, 1)(), ref[1], "lone fit on slot 1 after the failing fits")
    assert_yield_table_clear(lib)


def test_exact_fits_beside_predicts(lib):
    """The K-fold mode (valid.sharded_k_fold): thread 0 fits at N = 7168 while thread 1 predicts 2501 points from a GPR posterior
    (n = 3000, d = 7: the data of test_predict_product_form_equals_the_blocked_solve) held on its own slot, alternating the product
    form (predict_inverse 2: the fold kernel, which polls the yield table) and the blocked solve (0).  fmu and fs2 equal the same
    call made alone, per form; the fits equal the lone fits; the yield table is clear."""
    import pygps_amd as pyGPs
    from pygps_amd import _lib
    N = 7168
    jobs0, steps0, nb, l_step = good_fit_jobs(lib, N, 0, factor=False)
    ref = lone(lib, N, effective_sched(N), 0, steps0)
    n, d, ns = 3000, 7, 2501
    x, y = synth_reg(n, d, seed=11)
    rng = np.random.RandomState(5)
    xs = rng.randn(ns, d)
    xs[:300] = x[rng.randint(0, n, 300)] + 1e-3 * rng.randn(300, d)
    m = pyGPs.GPR()
    m.setPrior(kernel=pyGPs.cov.RBF(np.log(np.sqrt(d)), 0.2))
    m.setNoise(np.log(0.05))
    m.setData(x, y)
    with options(lib, (1,), predict_inverse=1) as (h1,):

        def predict(mode):
            _lib.check(lib.pgp_set_option(h1, b"predict_inverse", mode))
            out = m.predict(xs)
            return mode, np.array(out[2]), np.array(out[3])
        with _lib.fit_stream(1):
            m.getPosterior()
            alone = {mode: predict(mode) for mode in (2, 0)}
        assert not np.array_equal(alone[2][2], alone[0][2])           # two code paths, not one: the option reached the context
        jobs1 = [(lambda mode=(2, 0)[i % 2]: predict(mode)) for i in range(len(jobs0))]
        results, _ = run_side_by_side([jobs0, jobs1], n_barrier=nb, hint=True)
        assert_yield_table_clear(lib)
    for i, (mode, fmu, fs2) in enumerate(results[1]):
        assert mode == (2, 0)[i % 2]
        assert np.array_equal(fmu, alone[mode][1]), "predict %d (form %d): fmu differs from the lone call" % (i, mode)
        assert np.array_equal(fs2, alone[mode][2]), "predict %d (form %d): fs2 differs from the lone call" % (i, mode)
    assert_thread_equals_lone(results[0], steps0, ref, "fits beside predicts")


def test_an_exact_fit_beside_an_ep_fit(lib):
    """Thread 0 runs exact fits at N = 4608 (four to a call: a call lasts about as long as one block sweep of the neighbour) and
    holds the device gate SHARED for each; thread 1 runs GPC + EP fits on synth_cls(1024, 8) (the model of
    test_two_ep_fits_at_once_on_two_fit_streams), whose block sweeps take the gate EXCLUSIVELY.  Both threads finish -- within a
    time sized from the lone calls -- and both sides equal their lone results bit for bit."""
    import pygps_amd as pyGPs
    N, burst = 4608, 4
    ncall = 2 * N_BARRIER
    ref = lone(lib, N, -1, 0, range(ncall * burst))
    xc, yc = synth_cls(1024, 8)

    def ep_fit():
        mc = pyGPs.GPC()
        mc.setPrior(kernel=pyGPs.cov.RBF(np.log(np.sqrt(8.0)), 0.0))
        nlZ, dnlZ, post = mc.getPosterior(xc, yc)
        return nlZ, np.array(post.alpha)

    def burst_job(i):
        fits = [step_job(lib, N, i * burst + j) for j in range(burst)]
        return lambda: [f() for f in fits]
    ep_fit()                                                            # warm: the lone times below size the time limit
    t0 = time.perf_counter(); ep_alone = ep_fit(); t_ep = time.perf_counter() - t0
    t0 = time.perf_counter(); burst_job(0)(); t_ex = time.perf_counter() - t0
    limit = 30.0 + 20.0 * ncall * (t_ep + t_ex)                         # 20 x the serial time of everything, + start-up
    results, _ = run_side_by_side([[burst_job(i) for i in range(ncall)], [ep_fit] * ncall], n_barrier=N_BARRIER, join_timeout=limit)
    assert_yield_table_clear(lib)
    for i, fits in enumerate(results[0]):
        for j, r in enumerate(fits):
            assert_same(r, ref[i * burst + j], "exact fit %d beside EP" % (i * burst + j))
    for i, (nlZ, alpha) in enumerate(results[1]):
        assert nlZ == ep_alone[0] and np.array_equal(alpha, ep_alone[1]), "EP fit %d beside exact fits differs from the lone fit" % i


def digest(r):
    return hashlib.sha256(b"".join(np.ascontiguousarray(r[k]).tobytes() for k in SMALL)).hexdigest()


COLD_N, COLD_BARRIER = 7168, 2


def _cold_start_child():
    """The body of the child process of test_cold_start_...: its FIRST device work is the two threads' first fits, released together."""
    from pygps_amd import _lib
    lib = _lib.load()
    steps = [[k + 2 * i for i in range(COLD_BARRIER)] for k in range(2)]
    jobs = [[step_job(lib, COLD_N, s) for s in steps[k]] for k in range(2)]        # host work only: no context exists yet
    results, _ = run_side_by_side(jobs, n_barrier=COLD_BARRIER, hint=True)
    out = {str(s): digest(r) for k in range(2) for s, r in zip(steps[k], results[k])}
    out["yield_marks"] = int(np.count_nonzero(yield_table(lib)))
    print("COLD " + json.dumps(out))


def test_cold_start_of_two_fit_streams_in_a_fresh_process(lib):
    """The once-per-process state (the second context's creation, func_max_dynamic_lds, the exp table) is long warm when the other
    tests run; a fresh child process makes the (N = 7168, hint) case its first device work, both threads released by a barrier, two
    fits per thread, no warm-up.  The sha256 of (nlZ, alpha, dnlZ) of every step equals that of this process's lone fits."""
    ref = lone(lib, COLD_N, effective_sched(COLD_N), 0, range(2 * COLD_BARRIER))
    code = ("import sys; sys.path[:0] = [%r, %r]; import conftest; import test_gpu_side_by_side as t; t._cold_start_child()"
            % (os.path.join(ROOT, "tests"), ROOT))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    p = subprocess.run(cmd, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    assert p.returncode == 0, "child exit status %d\n%s" % (p.returncode, p.stdout[-4000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("COLD ")]
    assert len(lines) == 1, p.stdout[-4000:]
    got = json.loads(lines[0][5:])
    assert got.pop("yield_marks") == 0
    assert got == {str(s): digest(ref[s]) for s in range(2 * COLD_BARRIER)}
