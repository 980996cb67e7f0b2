"""range_route_host, the host mirror of a route call and the GPU tests' oracle for routing (CPU
only): its ranges against a direct transcription of the reference's find_pivot loop
(trunk_ondisk_node_find_pivot, src/trunk.c:5892-5928, with less_than_or_equal; pivot 0 is the
node's lower bound, -infinity here) under slice_lex_cmp (src/util.h:67-81) written out byte by
byte, and its CSR against a plain loop. Nothing of the reference is read."""
import numpy as np
import pytest

from splinterdb_amd import engine as E

ALPHABET = [0x00, 0x61, 0x7F, 0x80, 0xFF]
LENS = [0, 1, 2, 7, 8, 9, 10, 16, 17, 40]


def slice_lex_cmp(a: bytes, b: bytes) -> int:
    """unsigned memcmp over the common length, then the shorter key first"""
    for x, y in zip(a, b):
        if x != y:
            return -1 if x < y else 1
    return (len(a) > len(b)) - (len(a) < len(b))


def find_pivot(boundaries, key: bytes) -> int:
    """the last pivot <= key among (-inf, boundaries...): the reference's binary search"""
    lo, hi = 0, len(boundaries) + 1
    while lo + 1 < hi:
        mid = (lo + hi) // 2
        if slice_lex_cmp(key, boundaries[mid - 1]) < 0:
            hi = mid
        else:
            lo = mid
    return lo


def rand_key(rng, nsym=5):
    return bytes(ALPHABET[i] for i in rng.integers(0, nsym, size=LENS[rng.integers(0, len(LENS))]))


def rand_table(rng, nb, nsym=5):
    bounds = sorted({rand_key(rng, nsym) for _ in range(nb)})
    lists = [rng.integers(0, 50, size=rng.integers(0, 5)).tolist() for _ in range(len(bounds) + 1)]
    return bounds, lists


def rand_probe_keys(rng, bounds, n, nsym=5):
    keys = []
    for _ in range(n):
        how = rng.integers(0, 10)
        b = bounds[rng.integers(0, len(bounds))] if bounds else b""
        if how < 3:
            keys.append(b)                                  # equal to a boundary
        elif how == 3:
            keys.append(b[:rng.integers(0, len(b))] if b else b)  # a proper prefix
        elif how == 4:
            keys.append(b + bytes([ALPHABET[rng.integers(0, 5)]]))  # a byte appended
        else:
            keys.append(rand_key(rng, nsym))
    return keys


def test_bytes_order_is_slice_lex_cmp():
    rng = np.random.default_rng(1)
    ks = [rand_key(rng, 2 + i % 4) for i in range(400)]
    for a in ks[:200]:
        for b in ks[200:260]:
            assert ((a > b) - (a < b)) == slice_lex_cmp(a, b)
    assert b"\x7f" < b"\x80" and b"ab" < b"ab\0" < b"ab\0\0" and b"" < b"\0"


@pytest.mark.parametrize("seed", range(6))
def test_ranges_match_find_pivot(seed):
    rng = np.random.default_rng(100 + seed)
    for _ in range(12):
        bounds, lists = rand_table(rng, int(rng.integers(0, 120)), nsym=2 if seed % 2 else 5)
        keys = rand_probe_keys(rng, bounds, 300, nsym=2 if seed % 2 else 5)
        rg, off, member, total = E.range_route_host(bounds, lists, keys)
        want = np.array([find_pivot(bounds, k) for k in keys], dtype=np.uint32)
        assert (rg == want).all()
        # the CSR: key i owns its range's list, in list order
        assert off[0] == 0 and off[-1] == total == len(member)
        at = 0
        for i, r in enumerate(want):
            assert off[i] == at
            assert member[at:at + len(lists[r])].tolist() == lists[r]
            at += len(lists[r])
        assert at == total


def test_equal_key_goes_right_and_the_empty_boundary():
    bounds = [b"", b"ab", b"ab\0", b"ab\0\0", b"b"]
    lists = [[1], [2, 3], [], [4], [5, 6, 7], [8]]
    rg, off, member, total = E.range_route_host(bounds, lists, [b"", b"a", b"ab", b"aa", b"ab\0\0", b"zz", b"ab\0"])
    assert rg.tolist() == [1, 1, 2, 1, 4, 5, 3]
    assert off.tolist() == [0, 2, 4, 4, 6, 9, 10, 11] and total == 11
    assert member.tolist() == [2, 3, 2, 3, 2, 3, 5, 6, 7, 8, 4]
    # R = 1: no boundary, every key in range 0; no keys at all
    rg, off, member, total = E.range_route_host([], [[7, 7]], [b"x", b""])
    assert rg.tolist() == [0, 0] and member.tolist() == [7, 7, 7, 7] and total == 4
    rg, off, member, total = E.range_route_host([b"a"], [[1], []], [])
    assert rg.size == 0 and off.tolist() == [0] and total == 0
    with pytest.raises(ValueError):
        E.range_route_host([b"a"], [[1]], [b"x"])
