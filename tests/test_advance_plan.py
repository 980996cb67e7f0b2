"""The stepwise hand-out of per-key candidates, the parts that need no device (CPU only).

tests/c/advance_check.cpp is a stand-alone program around the host-only plan
splinterdb_amd/csrc/rf_advance_plan.h, built here with the address and undefined-behaviour
sanitizers and run as its own process, exactly as test_by_branch_plan.py builds its program: the
scratch sections aligned, disjoint and non-decreasing in n, one key's take against its definition,
and every refusal in the header's order.

The sizing is also called through the C ABI, which needs no device.
"""
import os
import subprocess

import pytest

from conftest import ROOT
from splinterdb_amd import engine as E

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "splinterdb_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "advance_check.cpp")
EXE = os.path.join(ROOT, "tests", "c", "advance_check")


@pytest.fixture(scope="module")
def advance_check_output():
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("rf_advance_plan.h", "rf_per_key_plan.h", "rf_range_plan.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", CSRC, SRC, "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_plan(advance_check_output):
    assert "advance_check: OK" in advance_check_output
    assert "CHECK failed" not in advance_check_output


def test_scratch_bytes_through_the_abi():
    tile = E.diag_per_key_tile()
    last = 0
    for n in (0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 77, 1 << 24, (1 << 56) - 1):
        b = E.found_advance_scratch_bytes(n)
        tiles = (n + tile - 1) // tile
        assert b % 8 == 0 and b >= max(8, 12 * tiles) and b >= last, n
        last = b
    # nothing is kept per key
    assert E.found_advance_scratch_bytes(1 << 24) < 16 * (1 << 24) // tile + 64
