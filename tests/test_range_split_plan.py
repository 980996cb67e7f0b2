"""Range maps that follow node splits, the parts that need no device (CPU only).

tests/c/range_split_check.cpp is a stand-alone program around the host-only planner
splinterdb_amd/csrc/rf_range_split_plan.h, built here with the address and undefined-behaviour
sanitizers and run as its own process: the create with room and its refusals, random sequences of
splits and set_paths applied to the plan's image by the host mirror of the splice and compared
byte for byte with a plan rebuilt from a naive model after every edit, every refusal of an edit
with its code and nothing changed, the cut into launches at the exact word limits, and
RF_AMD_ENOSPC at exactly one past each room field.

The C ABI's refusals that touch no device are called directly, and the Python model of an edit
(E.range_split_host, E.range_set_paths_host) is checked against hand-made tables. A flat or
roomless map needs a device to exist: its refusals are in test_gpu_range_split.py.
"""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT
from splinterdb_amd import engine as E

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "splinterdb_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "range_split_check.cpp")
EXE = os.path.join(ROOT, "tests", "c", "range_split_check")


@pytest.fixture(scope="module")
def range_split_check_output():
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("rf_range_split_plan.h", "rf_range_seg_plan.h", "rf_range_plan.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", CSRC, SRC, "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_planner(range_split_check_output):
    out = range_split_check_output
    assert "range_split_check: OK" in out
    assert "CHECK failed" not in out
    for part in ("create with room: OK", "refusals: OK", "edit sequences: 360 steps", "cuts: OK", "room: OK"):
        assert part in out


def test_null_map_is_refused_without_a_device():
    L = E.load_library()
    B = E.STATUS_BAD_PARAM
    assert E.STATUS_NO_SPACE == 28
    off = (ctypes.c_uint64 * 2)(0, 0)
    assert L.rf_amd_range_map_split(None, 0, 1, None, None, None, off, None) == B
    assert b"null range map" in L.rf_amd_last_error()
    assert L.rf_amd_range_map_set_paths(None, 0, 1, None, off, None) == B
    assert b"null range map" in L.rf_amd_last_error()
    assert L.rf_amd_range_map_set_paths(None, 0, 0, None, None, None) == B


def test_create_with_room_needs_an_engine():
    L = E.load_library()
    h = ctypes.c_void_p(1)
    room = E.RangeRoom(ranges=4, bound_bytes=8, path_entries=8, list_ids=8, max_list=8)
    assert L.rf_amd_range_map_create_segments_room(None, 1, None, None, None, None, 0, None, None, None,
                                                   ctypes.byref(room), ctypes.byref(h)) != 0
    assert b"no engine" in L.rf_amd_last_error()
    assert ctypes.sizeof(E.RangeRoom) == 40  # rf_amd_range_room: uint32, 3 x uint64, uint32, padded


def test_splice_words_without_a_device():
    """one launch's words and the rest of its arguments fill 4,096 bytes at the most"""
    W = E.diag_range_splice_words()
    assert 64 < W and 4 * W < 4096
    assert E.range_splice_words([], [[]]) == 2
    assert E.range_splice_words([b"", b"a", b"abcd", b"abcde"], [[1, 2], [], [3], [], []]) == 16 + 3 + 10 + 3


def test_edit_models():
    bounds, paths = [b"b", b"d"], [[0, 1], [0, 2], [0]]
    b2, p2 = E.range_split_host(bounds, paths, 1, [b"c", b"cc"], [[0, 3], [], [0, 4]])
    assert b2 == [b"b", b"c", b"cc", b"d"] and p2 == [[0, 1], [0, 3], [], [0, 4], [0]]
    assert (bounds, paths) == ([b"b", b"d"], [[0, 1], [0, 2], [0]]), "the inputs are left alone"
    b3, p3 = E.range_split_host(b2, p2, 0, [b""], [[], [5]])  # the empty key as the first boundary
    assert b3 == [b"", b"b", b"c", b"cc", b"d"] and p3[:3] == [[], [5], [0, 3]] and len(p3) == 6
    b4, p4 = E.range_split_host(b3, p3, 5, [b"e"], [[7], [8]])  # the last range
    assert b4[-2:] == [b"d", b"e"] and p4[-3:] == [[0, 4], [7], [8]]
    assert E.range_split_host(b4, p4, 2, [], [[9]]) == (b4, p4[:2] + [[9]] + p4[3:])  # pieces == 1
    assert sorted(b4) == b4
    with pytest.raises(ValueError):
        E.range_split_host(bounds, paths, 0, [b"a"], [[0]])
    assert E.range_set_paths_host(p2, 1, [[], [1, 1]]) == [[0, 1], [], [1, 1], [0, 4], [0]]
    assert E.range_set_paths_host(p2, 0, [[6] + p for p in p2]) == [[6, 0, 1], [6, 0, 3], [6], [6, 0, 4], [6, 0]]
    # what range_route_host makes of a split: the keys of the old range fall into the new ones
    segs = [[1], [2], [3], [4], [5]]
    keys = [b"a", b"b", b"bz", b"c", b"cb", b"cc", b"d"]
    rg = E.range_route_host(b2, E.range_segment_lists(p2, segs), keys)[0]
    assert rg.tolist() == [0, 1, 1, 2, 2, 3, 4]
