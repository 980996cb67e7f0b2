"""The batch planner on the host (splinterdb_amd/csrc/rf_batch_plan.h, CPU only).

tests/c/plan_check.cpp is a stand-alone program around the header: it plans batches without a
device and checks the invariants the kernels rely on (geometry bounds, running bases, the K5
workgroup map, tile cuts of chained batches, the in-place / decode decision for old filters,
and that an import derives the same probe plan as the build). Its "ref" lines are compared
here with the CPU oracle's routing_filter_add.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "splinterdb_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "plan_check.cpp")
EXE = os.path.join(ROOT, "tests", "c", "plan_check")


def run_plan_check(args=()):
    """plan_check's output (built first when its sources are newer); args: its "line" rows"""
    deps = [SRC, os.path.join(CSRC, "rf_batch_plan.h"), os.path.join(CSRC, "rf_plan.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-I", CSRC, SRC, "-o", EXE], check=True)
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    return r.stdout


@pytest.fixture(scope="module")
def plan_check_output():
    return run_plan_check()


def test_planner_invariants(plan_check_output):
    assert "plan_check: OK" in plan_check_output


def test_geometry_matches_the_oracle(plan_check_output, oracle):
    rows = [tuple(int(x) for x in ln.split()[1:]) for ln in plan_check_output.splitlines() if ln.startswith("ref ")]
    assert sorted((lis, n) for lis, n, *_ in rows) == sorted((lis, n) for lis in (4, 8) for n in (1, 300, 5000, 70000))
    rng = np.random.default_rng(7)
    for lis, n, lnb, num_indices, vs in rows:
        f = oracle.filter_add(oracle.make_config(26, lis), rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32))
        assert f.num_fingerprints == n
        assert (num_indices, vs) == (f.num_indices, f.value_size), (lis, n)
        assert num_indices == 1 << (lnb - lis)
