"""Member kinds of a filter set and the existence calls, the parts that need no device (CPU only).

tests/c/set_kind_check.cpp is a stand-alone program around the host-only planner
splinterdb_amd/csrc/rf_set_plan.h, built here with the address and undefined-behaviour
sanitizers and run as its own process, exactly as test_set_update_plan.py builds its program: kind
2 (RF_AMD_MEMBER_UNFILTERED) in the planner, the last entry of a repeated id winning across kinds,
the seed rule of the keys forms ignoring unfiltered slots, num_members growing past an unfiltered
id, and a refused call leaving the kinds as they were.

The C ABI's refusals that touch no device are called directly: every rf_amd_filter_set_exists_*
call with a NULL set is EINVAL.
"""
import os
import subprocess

import pytest

from conftest import ROOT
from splinterdb_amd import engine as E

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "splinterdb_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "set_kind_check.cpp")
EXE = os.path.join(ROOT, "tests", "c", "set_kind_check")


@pytest.fixture(scope="module")
def set_kind_check_output():
    deps = [SRC, os.path.join(CSRC, "rf_set_plan.h"), os.path.join(CSRC, "rf_plan.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", CSRC, SRC, "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_planner(set_kind_check_output):
    assert "set_kind_check: OK" in set_kind_check_output
    assert "CHECK failed" not in set_kind_check_output


def test_exists_calls_refuse_a_null_set_without_a_device():
    L = E.load_library()
    x = 8  # a non-null address that nothing reads: every call below is refused first
    calls = [
        lambda n: L.rf_amd_filter_set_exists_keys(None, x, 24, x, 3, n, x, None),
        lambda n: L.rf_amd_filter_set_exists_var_keys(None, x, x, x, 3, n, x, None),
        lambda n: L.rf_amd_filter_set_exists_hashes(None, x, x, 3, n, x, None),
        lambda n: L.rf_amd_filter_set_exists_keys_ragged(None, x, 24, x, x, n, x, None),
        lambda n: L.rf_amd_filter_set_exists_var_keys_ragged(None, x, x, x, x, n, x, None),
        lambda n: L.rf_amd_filter_set_exists_hashes_ragged(None, x, x, x, n, x, None),
    ]
    for call in calls:
        for n in (10, 0):
            assert call(n) == E.STATUS_BAD_PARAM
            assert b"null filter set" in L.rf_amd_last_error()


def test_python_names():
    assert repr(E.UNFILTERED) == "UNFILTERED" and E.UNFILTERED is not None
    assert (E.EXISTS_FILTER_HIT, E.EXISTS_UNFILTERED) == (1, 2)
    assert (E.KIND_FILTER, E.KIND_NULL, E.KIND_UNFILTERED) == (0, 1, 2)
    for name in ("exists_keys", "exists_var_keys", "exists_hashes", "exists_keys_ragged", "exists_var_keys_ragged",
                 "exists_hashes_ragged", "exists_routed", "exists_var_routed"):
        assert callable(getattr(E.FilterSet, name))
