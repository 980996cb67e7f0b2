"""The global-memory XXH32 helpers of splinterdb_amd/csrc/rf_device.h on the host (CPU only).

tests/c/hash_check.cpp is a stand-alone program around the header, built here with the address
and undefined-behaviour sanitizers and run directly. For every key length 0..300, four seeds and
key bases at byte offsets 0, 1, 2, 3, 4 and 8 it compares xxh32_unaligned,
xxh32_unaligned_prefetch and, where they apply, xxh32_words and xxh32_24 with a byte-at-a-time
XXH32 of its own; every key ends where its heap block ends, so a load past the key's last byte
aborts the run. It then hashes keys laid back to back with the reader fixed_kind() (rf_plan.h)
picks for their base, so a reader chosen for keys less aligned than its loads need is a
misaligned load the sanitizer stops at. Its "ref" lines are compared here with the CPU oracle,
which pins the program's own XXH32.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "splinterdb_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "hash_check.cpp")
EXE = os.path.join(ROOT, "tests", "c", "hash_check")

REF_LENS = [1, 3, 4, 15, 16, 17, 24, 31, 33, 100, 127, 128, 129, 300]
SEEDS = [42, 0, 0xFFFFFFFF, 7]


def key_bytes(n):
    """hash_check.cpp's key of length n (key_byte)"""
    i = np.arange(n, dtype=np.uint64)
    return ((((i + 1) * 2654435761 + n * 40503) & 0xFFFFFFFF) >> 24).astype(np.uint8)


@pytest.fixture(scope="module")
def hash_check_output():
    deps = [SRC, os.path.join(CSRC, "rf_device.h"), os.path.join(CSRC, "rf_plan.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", CSRC, SRC, "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_helpers_match_bytewise_xxh32_and_stay_inside_the_key(hash_check_output):
    assert "hash_check: OK" in hash_check_output
    assert "MISMATCH" not in hash_check_output


def test_ref_lines_match_the_oracle(hash_check_output, oracle):
    rows = [tuple(int(x) for x in ln.split()[1:]) for ln in hash_check_output.splitlines() if ln.startswith("ref ")]
    assert sorted((n, s) for n, s, _ in rows) == sorted((n, s) for n in REF_LENS for s in SEEDS)
    for n, seed, h in rows:
        assert h == int(oracle.hash_fixed(key_bytes(n), n, seed=seed)[0]), (n, seed)
