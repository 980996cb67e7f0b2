"""The group-by-branch call, the parts that need no device (CPU only).

tests/c/by_branch_check.cpp is a stand-alone program around the host-only plan
splinterdb_amd/csrc/rf_by_branch_plan.h, built here with the address and undefined-behaviour
sanitizers and run as its own process, exactly as test_set_kind_plan.py builds its program: the
pass count on both sides of every num_members at which it changes, the scratch sections aligned,
disjoint and non-decreasing in cap, and every refusal.

The C ABI's parts that touch no device are called directly: the sizing, the two diagnostics and
the refusal of a NULL engine.
"""
import os
import subprocess

import pytest

from conftest import ROOT
from splinterdb_amd import engine as E

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "splinterdb_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "by_branch_check.cpp")
EXE = os.path.join(ROOT, "tests", "c", "by_branch_check")


@pytest.fixture(scope="module")
def by_branch_check_output():
    deps = [SRC, os.path.join(CSRC, "rf_by_branch_plan.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", CSRC, SRC, "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_plan(by_branch_check_output):
    assert "by_branch_check: OK" in by_branch_check_output
    assert "CHECK failed" not in by_branch_check_output


def test_passes_and_tile_through_the_abi():
    tile = E.diag_by_branch_tile()
    assert tile >= 256 and tile % 256 == 0
    # the key has bit_length(num_members - 1) + 6 bits and a pass sorts 8 of them
    for nm in (1, 2, 4, 5, 64, 1024, 1025, 1 << 18, (1 << 18) + 1, 1 << 26):
        assert E.diag_by_branch_passes(nm) == ((nm - 1).bit_length() + 6 + 7) // 8, nm
    assert E.diag_by_branch_passes(0) == 0 and E.diag_by_branch_passes((1 << 26) + 1) == 0


def test_scratch_bytes_through_the_abi():
    tile = E.diag_by_branch_tile()
    last = 0
    for cap in (0, 1, tile - 1, tile, tile + 1, 3 * tile + 77, 1 << 24, (1 << 32) - 1):
        b = E.found_by_branch_scratch_bytes(cap, 64)
        tiles = (cap + tile - 1) // tile
        assert b % 8 == 0 and b >= max(8, 16 * cap + 2 * 4 * 256 * tiles) and b >= last, cap
        assert b == E.found_by_branch_scratch_bytes(cap, 1) == E.found_by_branch_scratch_bytes(cap, 1 << 26)
        last = b


def test_refuses_a_null_engine_without_a_device():
    L = E.load_library()
    x = 8  # a non-null, 8-byte aligned address that nothing reads: the call is refused first
    for cap in (10, 0):
        assert L.rf_amd_found_by_branch(None, x, x, x, cap, 4, x, x, x, x, 3, x, x, None) == E.STATUS_BAD_PARAM
        assert b"null engine" in L.rf_amd_last_error()


def test_python_names():
    for name in ("found_by_branch", "found_by_branch_host", "found_by_branch_scratch_bytes", "by_branch_sort_key",
                 "diag_by_branch_tile", "diag_by_branch_passes"):
        assert callable(getattr(E, name))
    assert callable(E.FilterSet.group_by_branch)
