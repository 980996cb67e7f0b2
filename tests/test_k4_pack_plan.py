"""Which bitmap batches are built packed (k4_pack_batch in splinterdb_amd/csrc/rf_batch_plan.h,
CPU only), and the shapes of tests/test_gpu_k4_pack.py against the oracle.

tests/c/k4_pack_check.cpp is a stand-alone program around the header: it plans batches without a
device, checks the decision on each (C2 packs; C3, an incremental batch, a chained batch, rvs 6
and the small index sizes do not) and, in a sweep over every (fingerprint, log_index_size, n,
value) the planner accepts, that the decision is the predicate's and that the bound on a coarse
bucket's staged bodies holds and fits the staging area. Its "case" lines are read here.
"""
import os
import subprocess

import pytest

import k4_pack_cases as C
from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "splinterdb_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "k4_pack_check.cpp")
EXE = os.path.join(ROOT, "tests", "c", "k4_pack_check")

# name -> (packs, rvs of the first filter)
EXPECTED = {"c2": (1, 4), "c3": (0, 6), "mixed": (0, 2), "incremental": (0, 4), "chained": (0, 5)}
EXPECTED.update({s.name: (int(s.packs), s.rvs) for s in C.SHAPES})


@pytest.fixture(scope="module")
def check_output():
    deps = [SRC, os.path.join(CSRC, "rf_batch_plan.h"), os.path.join(CSRC, "rf_plan.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-I", CSRC, SRC, "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    return r.stdout


def test_predicate_checks(check_output):
    assert "k4_pack_check: OK" in check_output


def test_decision_per_case(check_output):
    rows = {}
    for ln in check_output.splitlines():
        if ln.startswith("case "):
            _, name, packs, rvs = ln.split()
            rows[name] = (int(packs), int(rvs))
    assert rows == EXPECTED


def test_sweep_reaches_packed_plans(check_output):
    (ln,) = [ln for ln in check_output.splitlines() if ln.startswith("sweep ")]
    _, plans, packed = ln.split()
    assert int(plans) > 1000 and int(packed) > 100


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: s.name)
def test_oracle_geometry(oracle, shape):
    """the oracle builds each shape with the remainder width and key width its case claims"""
    of = oracle.filter_add(oracle.make_config(fingerprint_size=shape.fp, log_index_size=shape.lis),
                           shape.hashes(), value=shape.value)
    assert C.geometry(shape.fp, shape.lis, of.num_indices, of.value_size) == (shape.rvs, shape.bits)
