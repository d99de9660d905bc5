"""Launch census of the Cholesky sweep: for every case of tests/golden/G26_sweep_census.json, one fit with profiling on, and
the launches and flops of every profile class (pygps_amd._lib.profile()).

    python tools/record_sweep_census.py --commit <hash> [--out FILE]     record: rewrites the JSON's "census" entries
    python tools/record_sweep_census.py --dump DIR                       save every case's results to DIR/<id>.npz (bit comparisons
                                                                         between two builds; arrays over 1 MiB as their SHA-256)

The JSON carries the case list; this recorder and tests/test_gpu_sweep_census.py both iterate it (run_case below is the one
runner).  Only the public C ABI is used, so the file runs unchanged against another build of the library (PYGPS_AMD_LIB)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
JSON_PATH = os.path.join(ROOT, "tests", "golden", "G26_sweep_census.json")

# library defaults of every option a case may set: each case puts back what it set
DEFAULTS = {"sched": -1, "nb_outer": 0, "lookahead": 1, "s_pan": -1, "s_pan_direct": 1, "s_pan_out": 1, "leaf_first": 0,
            "pair_launch": 1, "eet_overlap": 3, "eet_first": -1, "concurrent_streams": 0, "ep_sigma_under": 1, "ep_fused": 2,
            "ep_final_rebuild": 0}


def synth(N, d, seed, classify):
    """the draw order of tests/conftest.py synth_reg / synth_cls"""
    rng = np.random.RandomState(seed)
    x = rng.randn(N, d)
    w = rng.randn(d, 1)
    if classify:
        y = np.sign(x @ w / np.sqrt(d) + 0.3 * rng.randn(N, 1))
        y[y == 0] = 1
    else:
        y = np.sin(x @ w / np.sqrt(d)) + 0.1 * rng.randn(N, 1)
    return x, y


def _exact_fit(lib, _lib, ctx, N, want):
    """data and hyperparameters of test_gpu_skip_zeros._fit_all: RBF, d = 16, synth_reg(N, 16, seed=N)"""
    d = 16
    x, y = synth(N, d, N, False)
    x = _lib.f64(x); y = _lib.f64(y).ravel()
    hyp = _lib.f64(np.array([np.log(np.sqrt(d)), 0.2])); m = np.full(N, float(y.mean())); dm = np.ones((1, N))
    _lib.check(lib.pgp_set_data(ctx, _lib.ptr(x), N, d, _lib.ptr(y)))
    alpha = np.zeros(N); nlZ = np.zeros(1); g = np.zeros(4); fh = C.c_void_p()
    yield                                                    # ---- profiled from here
    _lib.check(lib.pgp_exact_fit(ctx, 0, _lib.ptr(hyp), 2, 0, 0, float(np.log(0.1)), _lib.ptr(m), _lib.ptr(dm), 1, want,
                                 _lib.ptr(alpha), _lib.ptr(nlZ), _lib.ptr(g), C.byref(fh)), "pgp_exact_fit")
    yield                                                    # ---- to here
    L = np.zeros((N, N))
    _lib.check(lib.pgp_factor_to_host(ctx, fh, _lib.ptr(L)))
    lib.pgp_factor_free(ctx, fh)
    yield dict(nlZ=nlZ, alpha=alpha, dnlZ=g, L=np.tril(L))


def _potrf(lib, _lib, ctx, N):
    """pgp_potrf of B = K + I, K the RBF matrix (ell^2 = 16) of synth_reg(N, 16, seed=N)'s points"""
    x, _ = synth(N, 16, N, False)
    sq = (x * x).sum(1)
    A = np.exp(-0.5 * np.maximum(sq[:, None] + sq[None, :] - 2.0 * (x @ x.T), 0.0) / 16.0) + np.eye(N)
    A = _lib.f64(0.5 * (A + A.T)); L = np.zeros((N, N))
    yield
    _lib.check(lib.pgp_potrf(ctx, _lib.ptr(A), N, _lib.ptr(L)), "pgp_potrf")
    yield
    yield dict(L=L)


def _ep_fit(lib, _lib, ctx, N):
    """cold-start pgp_ep_fit (its cases set ep_final_rebuild: the parameter recomputation, whose sweep carries the dense rows, runs
    once) on the data of test_gpu_api.test_ep_variants_agree_with_the_reference: synth_cls(N, 32), RBF, zero mean"""
    x, y = synth(N, 32, 0, True)
    x = _lib.f64(x); y = _lib.f64(y).ravel()
    _lib.check(lib.pgp_set_data(ctx, _lib.ptr(x), N, 32, _lib.ptr(y)))
    hyp = _lib.f64(np.array([np.log(np.sqrt(32.0)), 0.0]))
    ttau, tnu, alpha, sW, nz, g = np.zeros(N), np.zeros(N), np.empty(N), np.empty(N), np.zeros(1), np.zeros(3)
    sweeps, fh = C.c_int(), C.c_void_p()
    mv, dm = np.zeros(N), np.zeros(N)
    yield
    _lib.check(lib.pgp_ep_fit(ctx, _lib.COV_RBF, _lib.ptr(hyp), 2, 0, 0, _lib.ptr(mv), _lib.ptr(dm), 0, 3, 0, _lib.ptr(ttau),
                              _lib.ptr(tnu), _lib.ptr(alpha), _lib.ptr(sW), _lib.ptr(nz), _lib.ptr(g), C.byref(sweeps), C.byref(fh)),
               "pgp_ep_fit")
    yield
    L = np.zeros((N, N))
    _lib.check(lib.pgp_factor_to_host(ctx, fh, _lib.ptr(L)))
    lib.pgp_factor_free(ctx, fh)
    yield dict(nlZ=nz, alpha=alpha, dnlZ=g, L=np.tril(L), ttau=ttau, tnu=tnu, sW=sW, sweeps=np.array([sweeps.value]))


def run_case(case):
    """One case: its options set, ONE call of its entry point with profiling on, the options put back.
    Returns ({class: {launches, flops}}, {name: array})."""
    from pygps_amd import _lib, inf
    lib, ctx = _lib.load(), _lib.ctx()
    N = int(case["N"])
    steps = {"exact_fit": lambda: _exact_fit(lib, _lib, ctx, N, int(case.get("want", 3))),
             "potrf": lambda: _potrf(lib, _lib, ctx, N),
             "ep_fit": lambda: _ep_fit(lib, _lib, ctx, N)}[case["entry"]]()
    try:
        for k, v in case["options"].items():
            _lib.check(lib.pgp_set_option(ctx, k.encode(), int(v)), k)
        next(steps)
        _lib.check(lib.pgp_set_profiling(ctx, 1))
        _lib.check(lib.pgp_profile_reset(ctx))
        try:
            next(steps)
        finally:
            lib.pgp_set_profiling(ctx, 0)
        prof = _lib.profile()
        arrays = next(steps)
    finally:
        for k in case["options"]:
            lib.pgp_set_option(ctx, k.encode(), DEFAULTS[k])
        inf._Resident.invalidate()                           # the case put data of its own on the context
    return {name: dict(launches=int(v["launches"]), flops=float(v["flops"])) for name, v in prof.items()}, arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="record: the hash of the commit whose library this is")
    ap.add_argument("--out", default=JSON_PATH)
    ap.add_argument("--dump", help="directory for <id>.npz with every case's results; arrays over 1 MiB as their SHA-256")
    args = ap.parse_args()
    assert args.commit or args.dump
    doc = json.load(open(JSON_PATH))
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    for case in doc["cases"]:
        case["census"], arrays = run_case(case)
        print(case["id"], {k: v["launches"] for k, v in case["census"].items() if v["launches"]}, flush=True)
        if args.dump:
            small = {k: v if v.nbytes <= 1 << 20 else np.frombuffer(hashlib.sha256(np.ascontiguousarray(v).tobytes()).digest(), np.uint8)
                     for k, v in arrays.items()}
            np.savez(os.path.join(args.dump, case["id"] + ".npz"), **small)
    if args.commit:
        doc["parent_commit"] = args.commit
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
