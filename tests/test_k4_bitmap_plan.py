"""Which batches take K4's bitmap kernel (k4_bitmap_batch in splinterdb_amd/csrc/rf_batch_plan.h,
CPU only).

tests/c/k4_bitmap_check.cpp is a stand-alone program around the header: it plans batches without
a device and checks the decision on each -- C2 takes the bitmap (16-bit key), C3 does not (19
bits), nor fp_size + value_size = 32, nor an index narrower than a bitmap word, nor a batch with
one ineligible filter, nor any incremental or chained batch. Its "case" lines are read here.
"""
import os
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "splinterdb_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "k4_bitmap_check.cpp")
EXE = os.path.join(ROOT, "tests", "c", "k4_bitmap_check")

# name -> (takes the bitmap kernel, widest in-bucket key of the batch in bits)
EXPECTED = {
    "c2": (1, 16),
    "c3": (0, 19),
    "fp26_value63": (0, 22),
    "narrow_index": (0, 13),
    "s_20000": (1, 16),
    "s_40000_v1": (1, 16),
    "s_100000_v3": (1, 16),
    "s_100000": (1, 14),
    "s_300000": (1, 12),
    "mixed": (0, 19),
    "incremental32": (0, 16),
    "incremental_mixed": (0, 16),
    "incremental64": (0, 22),
    "chained": (0, 17),
    "single_run": (1, 16),
}


@pytest.fixture(scope="module")
def check_output():
    deps = [SRC, os.path.join(CSRC, "rf_batch_plan.h"), os.path.join(CSRC, "rf_plan.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-I", CSRC, SRC, "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    return r.stdout


def test_predicate_checks(check_output):
    assert "k4_bitmap_check: OK" in check_output


def test_decision_per_case(check_output):
    rows = {}
    for ln in check_output.splitlines():
        if ln.startswith("case "):
            _, name, eligible, bits = ln.split()
            rows[name] = (int(eligible), int(bits))
    assert rows == EXPECTED
