"""Member updates of a filter set, the parts that need no device (CPU only).

tests/c/set_update_check.cpp is a stand-alone program around the host-only planner
splinterdb_amd/csrc/rf_set_plan.h, built here with the address and undefined-behaviour
sanitizers and run as its own process: the last entry of a repeated id wins, the cuts into
launches of at most 64 entries, num_members, a refused call leaving every output as it was, and
the seed rule of the keys forms as members come and go.

The C ABI's refusals that touch no device are called directly: a NULL set is EINVAL for
rf_amd_filter_set_update, rf_amd_filter_set_destroy_on(NULL) is OK as
rf_amd_batch_destroy_on(NULL) is, and the capacity of no set is 0.
"""
import os
import subprocess

import pytest

from conftest import ROOT
from splinterdb_amd import engine as E

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "splinterdb_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "set_update_check.cpp")
EXE = os.path.join(ROOT, "tests", "c", "set_update_check")


@pytest.fixture(scope="module")
def set_update_check_output():
    deps = [SRC, os.path.join(CSRC, "rf_set_plan.h"), os.path.join(CSRC, "rf_plan.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", CSRC, SRC, "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_planner(set_update_check_output):
    assert "set_update_check: OK" in set_update_check_output
    assert "CHECK failed" not in set_update_check_output


def test_null_set_is_refused_without_a_device():
    L = E.load_library()
    assert L.rf_amd_filter_set_update(None, None, None, None, 0, None) == E.STATUS_BAD_PARAM
    assert L.rf_amd_filter_set_update(None, None, None, None, 3, None) == E.STATUS_BAD_PARAM
    assert b"null filter set" in L.rf_amd_last_error()
    assert L.rf_amd_filter_set_destroy_on(None, None) == 0
    assert L.rf_amd_batch_destroy_on(None, None) == 0
    assert L.rf_amd_filter_set_capacity(None) == 0
    assert L.rf_amd_filter_set_num_members(None) == 0
