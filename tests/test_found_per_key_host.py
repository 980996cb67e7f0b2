"""The key-aware compaction, the parts that need no device (CPU only).

E.found_per_key_host and E.found_per_key_host_fixed, the numpy mirrors of
rf_amd_found_per_key_ragged and rf_amd_found_per_key, against a plain transcription of the loop
they serve (trunk_ondisk_bundle_merge_lookup, src/trunk.c:6057-6060): key by key, pair by pair of
the key's list, routing_filter_get_next_value until nothing is left.

tests/c/per_key_check.cpp is a stand-alone program around the host-only header
splinterdb_amd/csrc/rf_per_key_plan.h, built here with the address and undefined-behaviour
sanitizers and run as its own process: the scratch layout, the tile counts, the widths and every
argument check. The C ABI's refusals that touch no device are called directly.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from splinterdb_amd import engine as E

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "splinterdb_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "per_key_check.cpp")
EXE = os.path.join(ROOT, "tests", "c", "per_key_check")

WORDS = np.array([0, 1, 1 << 63, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
IDS = np.array([0, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)


def loop_reference(found, member, off):
    """the consumer's loop: (key_off, cand, cand_key) as Python lists"""
    key_off, cand, cand_key = [0], [], []
    for i in range(len(off) - 1):
        for p in range(int(off[i]), int(off[i + 1])):
            word = int(found[p])
            while True:
                # the next value of what is left of the word: the reference's own mask is an int
                # shift and goes wrong from value 31 up (test_multiget_host.py), so the value
                # handed out is cleared here instead of being passed back as last_value
                v = E.routing_filter_get_next_value(word, E.ROUTING_NOT_FOUND)
                if v == E.ROUTING_NOT_FOUND:
                    break
                word &= ~(1 << v)
                cand.append((int(member[p]) << 8) | v)
                cand_key.append(i)
        key_off.append(len(cand))
    return key_off, cand, cand_key


def random_csr(rng, n, first):
    """n list lengths 0-9 with empty lists at the start, at the end and in runs"""
    cnt = rng.integers(0, 10, size=n)
    cnt[rng.random(n) < 0.3] = 0
    cnt[0] = 0
    cnt[-1] = 0
    if n > 40:
        cnt[20:33] = 0
    off = np.full(n + 1, first, dtype=np.uint64)
    np.cumsum(cnt.astype(np.uint64), out=off[1:])
    off[1:] += np.uint64(first)
    return off


def random_words(rng, m):
    w = rng.integers(0, 1 << 64, size=m, dtype=np.uint64) & rng.integers(0, 1 << 64, size=m, dtype=np.uint64)
    pick = rng.random(m)
    w[pick < 0.4] = WORDS[rng.integers(0, len(WORDS), size=int((pick < 0.4).sum()))]
    return w


def random_ids(rng, m):
    ids = rng.integers(0, 1 << 32, size=m, dtype=np.uint64).astype(np.uint32)
    pick = rng.random(m) < 0.3
    ids[pick] = IDS[rng.integers(0, len(IDS), size=int(pick.sum()))]
    return ids


def check_equal(got, want, what):
    key_off, cand, cand_key = got
    assert key_off.dtype == np.uint64 and cand.dtype == np.uint64 and cand_key.dtype == np.int64, what
    assert key_off.tolist() == want[0], what
    assert cand.tolist() == want[1], what
    assert cand_key.tolist() == want[2], what


@pytest.mark.parametrize("first", [0, 1000])
@pytest.mark.parametrize("n", [1, 5, 64, 200])
def test_ragged_mirror_against_the_loop(n, first):
    rng = np.random.default_rng(100 * n + first)
    off = random_csr(rng, n, first)
    m = int(off[-1]) + 7  # words and ids above the last pair, and below the first
    found, member = random_words(rng, m), random_ids(rng, m)
    found[:first] = WORDS[3]
    found[int(off[-1]):] = WORDS[3]
    want = loop_reference(found, member, off)
    if n >= 64:
        assert len(want[1]) > 64 and set(WORDS.tolist()) <= set(found[first:int(off[-1])].tolist())
    check_equal(E.found_per_key_host(found, member, off), want, (n, first))


def test_ragged_mirror_nothing_found_and_no_keys():
    off = np.array([3, 3, 5, 5], dtype=np.uint64)
    got = E.found_per_key_host(np.zeros(6, dtype=np.uint64), np.arange(6, dtype=np.uint32), off)
    check_equal(got, ([0, 0, 0, 0], [], []), "all zero")
    got = E.found_per_key_host(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.array([0], dtype=np.uint64))
    check_equal(got, ([0], [], []), "n == 0")


@pytest.mark.parametrize("with_member", [False, True])
@pytest.mark.parametrize("K", [1, 4, 16, 65])
def test_fixed_mirror_against_the_loop(K, with_member):
    rng = np.random.default_rng(K)
    n = 37
    found = random_words(rng, n * K)
    member = random_ids(rng, n * K) if with_member else None
    ids = member if with_member else np.tile(np.arange(K, dtype=np.uint32), n)
    want = loop_reference(found, ids, np.arange(n + 1) * K)
    check_equal(E.found_per_key_host_fixed(found, member, K), want, (K, with_member))


def test_records_agree_with_found_candidates():
    """record j of the mirror and record j of E.found_candidates describe the same (pair, value)"""
    rng = np.random.default_rng(5)
    off = random_csr(rng, 100, 0)
    found, member = random_words(rng, int(off[-1])), random_ids(rng, int(off[-1]))
    _, cand, cand_key = E.found_per_key_host(found, member, off)
    rec = E.found_candidates(found)
    assert (cand & np.uint64(0xFF) == rec & np.uint64(0xFF)).all()
    assert (cand >> np.uint64(8) == member[(rec >> np.uint64(8)).astype(np.int64)]).all()
    assert (cand_key == E.ragged_pair_keys(off, rec >> np.uint64(8))).all()


# ---- the C ABI without a device ----------------------------------------------------------------
def test_scratch_bytes_without_a_device():
    tile = E.diag_per_key_tile()
    last = 0
    for n in [0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 1 << 20, 1 << 40, (1 << 56) - 1]:
        s = E.found_per_key_scratch_bytes(n)
        assert s >= last and s % 8 == 0 and s >= 4 * n + 12 * ((n + tile - 1) // tile), n
        last = s


def test_refusals_that_touch_no_device():
    L = E.load_library()
    B = E.STATUS_BAD_PARAM
    x = 8  # a non-null address that nothing reads: every call below is refused first

    def fixed(e=x, K=4, n=10):
        return L.rf_amd_found_per_key(e, x, x, K, n, x, x, x, 8, x, x, None)

    def ragged(e=x, n=10):
        return L.rf_amd_found_per_key_ragged(e, x, x, x, n, x, x, x, 8, x, x, None)

    for call, msg in [(lambda: fixed(e=None), b"engine"), (lambda: ragged(e=None), b"engine"),
                      (lambda: fixed(e=None, n=0), b"engine"), (lambda: ragged(e=None, n=0), b"engine"),
                      (lambda: fixed(n=1 << 56), b"2^56"), (lambda: ragged(n=1 << 56), b"2^56"),
                      (lambda: fixed(K=0), b"K"), (lambda: fixed(K=65536), b"K"),
                      (lambda: fixed(K=0, n=0), b"K")]:
        assert call() == B
        assert msg in L.rf_amd_last_error(), (msg, L.rf_amd_last_error())


@pytest.fixture(scope="module")
def per_key_check_output():
    deps = [SRC, os.path.join(CSRC, "rf_per_key_plan.h"), os.path.join(CSRC, "rf_range_plan.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", CSRC, SRC, "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_plan_header(per_key_check_output):
    assert "per_key_check: OK" in per_key_check_output
    assert "CHECK failed" not in per_key_check_output
