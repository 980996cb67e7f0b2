"""Range maps, the parts that need no device (CPU only).

tests/c/range_plan_check.cpp is a stand-alone program around the host-only planner
splinterdb_amd/csrc/rf_range_plan.h, built here with the address and undefined-behaviour
sanitizers and run as its own process: the refusals of rf_amd_range_map_create, R = 1 with NULL
boundary arrays, list offsets rebased to 0, max_list, the packed image, the scratch size of a
route call non-decreasing in n, and the kernel's search steps over the image against a
transcription of the reference's find_pivot loop on 180,000 random cases.

The C ABI's refusals that touch no device are called directly: a NULL map is EINVAL for both
route calls, rf_amd_range_map_destroy_on(NULL) is OK, and no map has 0 ranges.
"""
import os
import subprocess

import pytest

from conftest import ROOT
from splinterdb_amd import engine as E

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "splinterdb_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "range_plan_check.cpp")
EXE = os.path.join(ROOT, "tests", "c", "range_plan_check")


@pytest.fixture(scope="module")
def range_plan_check_output():
    deps = [SRC, os.path.join(CSRC, "rf_range_plan.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", CSRC, SRC, "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_planner(range_plan_check_output):
    assert "range_plan_check: OK" in range_plan_check_output
    assert "CHECK failed" not in range_plan_check_output
    assert "180000 cases" in range_plan_check_output


def test_null_map_is_refused_without_a_device():
    L = E.load_library()
    assert L.rf_amd_range_map_route_keys(None, None, 24, 0, None, None, None, 0, None, None, None) == E.STATUS_BAD_PARAM
    assert b"null range map" in L.rf_amd_last_error()
    assert L.rf_amd_range_map_route_keys(None, None, 24, 5, None, None, None, 0, None, None, None) == E.STATUS_BAD_PARAM
    assert L.rf_amd_range_map_route_var_keys(None, None, None, 5, None, None, None, 0, None, None,
                                             None) == E.STATUS_BAD_PARAM
    assert b"null range map" in L.rf_amd_last_error()
    assert L.rf_amd_range_map_destroy_on(None, None) == 0
    L.rf_amd_range_map_destroy(None)
    assert L.rf_amd_range_map_num_ranges(None) == 0
    assert L.rf_amd_range_map_max_list(None) == 0


def test_scratch_bytes_without_a_device():
    """callable without a device, 8-byte multiples, non-decreasing, 12 bytes per tile at least"""
    tile = E.diag_range_tile()
    last = 0
    for n in [0, 1, tile - 1, tile, tile + 1, 2381, 1 << 20, (1 << 24) + 1, 1 << 40, (1 << 56) - 1]:
        s = E.range_route_scratch_bytes(n)
        assert s >= last and s % 8 == 0 and s >= 12 * ((n + tile - 1) // tile)
        last = s
    assert E.diag_range_lds_ranges() >= 2
