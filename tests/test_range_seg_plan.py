"""Range maps made from segments, the parts that need no device (CPU only).

tests/c/range_seg_check.cpp is a stand-alone program around the host-only planner
splinterdb_amd/csrc/rf_range_seg_plan.h, built here with the address and undefined-behaviour
sanitizers and run as its own process: every refusal of rf_amd_range_map_create_segments and of
rf_amd_range_map_update_segments with nothing written, the legal edge cases, max_list = the
largest path capacity, the host flatten against a naive concatenation, 300 random update steps
applied to the plan's image (the launches' arguments scattered, then flattened) against the naive
model, and the cut of an update into launches and pieces.

The C ABI's refusals that touch no device are called directly -- a NULL map is EINVAL for the
update whatever count is, and has no segments -- and E.range_segment_lists is checked against
hand-made tables. A flat map needs a device to exist: its refusal is in
test_gpu_range_segments.py.
"""
import os
import subprocess

import pytest

from conftest import ROOT
from splinterdb_amd import engine as E

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "splinterdb_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "range_seg_check.cpp")
EXE = os.path.join(ROOT, "tests", "c", "range_seg_check")


@pytest.fixture(scope="module")
def range_seg_check_output():
    deps = [SRC, os.path.join(CSRC, "rf_range_seg_plan.h"), os.path.join(CSRC, "rf_range_plan.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", CSRC, SRC, "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_planner(range_seg_check_output):
    assert "range_seg_check: OK" in range_seg_check_output
    assert "CHECK failed" not in range_seg_check_output
    assert "update sequences: 300 steps" in range_seg_check_output


def test_null_map_is_refused_without_a_device():
    L = E.load_library()
    B = E.STATUS_BAD_PARAM
    assert L.rf_amd_range_map_update_segments(None, None, None, None, 0, None) == B
    assert b"null range map" in L.rf_amd_last_error()
    import numpy as np
    ids, off = np.array([0, 1], dtype=np.uint32), np.array([0, 1, 2], dtype=np.uint64)
    assert L.rf_amd_range_map_update_segments(None, ids.ctypes.data, ids.ctypes.data, off.ctypes.data, 2, None) == B
    assert b"null range map" in L.rf_amd_last_error()
    assert L.rf_amd_range_map_num_segments(None) == 0


def test_launch_ids_without_a_device():
    """one launch's ids and the piece's header fill 4,096 bytes of arguments at the most"""
    per = E.diag_range_seg_launch_ids()
    assert 64 < per and 4 * per < 4096


def test_create_segments_needs_an_engine():
    L = E.load_library()
    import ctypes
    h = ctypes.c_void_p(1)
    assert L.rf_amd_range_map_create_segments(None, 1, None, None, None, None, 0, None, None, None,
                                              ctypes.byref(h)) != 0
    assert b"no engine" in L.rf_amd_last_error()


def test_range_segment_lists():
    segs = [[1, 2], [], [7], [9, 9, 9]]
    paths = [[], [0], [0, 1, 2], [0, 2, 0], [3, 1], [1]]
    assert E.range_segment_lists(paths, segs) == [[], [1, 2], [1, 2, 7], [1, 2, 7, 1, 2], [9, 9, 9], []]
    assert E.range_segment_lists([], segs) == []
    assert E.range_segment_lists([[]], []) == [[]]
    import numpy as np
    got = E.range_segment_lists([np.array([2, 0])], [np.array([5], dtype=np.uint32), [], (6, 4)])
    assert got == [[6, 4, 5]] and all(type(i) is int for i in got[0])
    with pytest.raises(IndexError):
        E.range_segment_lists([[4]], segs)
    # what range_route_host makes of it: the lists of the ranges the keys fall into
    rg, off, member, total = E.range_route_host([b"b", b"d"], E.range_segment_lists([[0, 2], [], [3, 0]], segs),
                                                [b"a", b"b", b"c", b"z"])
    assert rg.tolist() == [0, 1, 1, 2] and off.tolist() == [0, 3, 3, 3, 8] and total == 8
    assert member.tolist() == [1, 2, 7, 9, 9, 9, 1, 2]
