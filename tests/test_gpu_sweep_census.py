"""The Cholesky sweep (csrc/sweep.hip) queues what the parent commit queued: for every case of golden/G26_sweep_census.json -- the
exact fit over panel counts, panel widths, the three schedules and their options, pgp_potrf, and EP's sweeps with dense
right-hand-side rows -- ONE call with profiling on, and per profile class the number of launches (exactly) and the flops (to
1e-12 relative: a sum of a few hundred positive doubles, reordering costs at most n 2^-53) equal the figures
tools/record_sweep_census.py took from the parent commit's library.  ms and bytes are not compared.

The JSON carries the case list; the recorder and this test run it through the same function (run_case)."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT

DOC = json.load(open(os.path.join(GOLDEN, "G26_sweep_census.json")))
CASES = DOC["cases"]


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("record_sweep_census", os.path.join(ROOT, "tools", "record_sweep_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_recorded_case_list_is_complete():
    """27 cases at least (the issue's list), every one with a recorded census, and the commit they were recorded from"""
    assert len(CASES) >= 27
    assert len({c["id"] for c in CASES}) == len(CASES)
    assert isinstance(DOC["parent_commit"], str) and len(DOC["parent_commit"]) == 40
    for c in CASES:
        assert c.get("census") and sum(v["launches"] for v in c["census"].values()) > 0, c["id"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_launch_census_equals_the_parent_commits(lib, recorder, case):
    got, _ = recorder.run_case(case)
    want = case["census"]
    print(case["id"], {k: (v["launches"], v["flops"]) for k, v in got.items() if v["launches"]})
    assert set(got) == set(want)
    for name in want:
        assert got[name]["launches"] == want[name]["launches"], (name, got[name], want[name])
        assert abs(got[name]["flops"] - want[name]["flops"]) <= 1e-12 * abs(want[name]["flops"]), (name, got[name], want[name])
