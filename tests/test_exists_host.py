"""The existence multi-get's host mirror (CPU only): E.exists_host and E.exists_host_fixed, the
numpy mirrors of rf_amd_filter_set_exists_*_ragged and rf_amd_filter_set_exists_*, against a
plain transcription of the reference's lookup of one key under lookup_result_is_existence
(SPLINTERDB_LOOKUP_MIGHT_EXIST): trunk_ondisk_bundle_merge_lookup (src/trunk.c:6020-6087) bundle
by bundle, newest first, with lookup_result_note_filter_hit and lookup_result_should_continue
(src/lookup_result.h:149-169).

The byte's contract: the reference's final answer equals (byte & 1) or "some unfiltered bundle's
branch holds the key", and byte == 0 coincides with "no branch was consulted and nothing was
found". Lists of filter, NULL and unfiltered bundles with random words and random truth for the
unfiltered branches, empty lists and lists of 300 members among them.
"""
import numpy as np
import pytest

from splinterdb_amd import engine as E

F, NUL, U = E.KIND_FILTER, E.KIND_NULL, E.KIND_UNFILTERED


def reference_existence_lookup(kinds, words, holds):
    """One key through its bundles. kinds[j]: what bundle j is; words[j]: routing_filter_lookup's
    found_values of the key in bundle j's maplet (read for filters only); holds[j]: whether the
    one branch of unfiltered bundle j holds the key. Returns (might exist, branches consulted)."""
    found = False  # merge_accumulator_message_class(&result->value) != MESSAGE_TYPE_INVALID
    consulted = 0
    for j, kind in enumerate(kinds):
        if kind != F:  # routing_filters_equal(&bndl->maplet, &NULL_ROUTING_FILTER), :6020-6022
            num_branches = 1 if kind == U else 0
            found_values = 1 if num_branches == 1 else 0
        else:
            found_values = int(words[j])
            if found_values != 0:
                # lookup_result_note_filter_hit: the class becomes MESSAGE_TYPE_UPDATE, and
                # lookup_result_should_continue is then false: return STATUS_OK (:6036-6043)
                found = True
                return found, consulted
        idx = E.routing_filter_get_next_value(found_values, E.ROUTING_NOT_FOUND)
        while idx != E.ROUTING_NOT_FOUND:  # :6057-6060
            consulted += 1  # btree_lookup_and_merge of bndl->branches[idx]
            if holds[j]:
                found = True
            if found:  # !lookup_result_should_continue(result), :6085
                return found, consulted
            idx = E.routing_filter_get_next_value(found_values, idx)
    return found, consulted


def random_case(rng, n, nm, first, long_lists=()):
    """a set of nm members of random kinds, n keys' lists (lengths 0-9, empty ones at both ends and
    in a run, the long ones placed) from pair `first` on, ids past the end included, words mostly
    zero, and random truth for every pair's branch"""
    kinds = rng.integers(0, 3, size=nm)
    kinds[:3] = [F, NUL, U]
    cnt = rng.integers(0, 10, size=n)
    cnt[rng.random(n) < 0.2] = 0
    cnt[0] = cnt[-1] = 0
    if n > 40:
        cnt[20:33] = 0
    for k, ln in long_lists:
        cnt[k] = ln
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(cnt.astype(np.uint64), out=off[1:])
    off += np.uint64(first)
    m = int(off[-1]) + 5
    member = rng.integers(0, nm + 2, size=m).astype(np.uint32)
    words = np.where(rng.random(m) < 0.15, rng.integers(1, 1 << 64, size=m, dtype=np.uint64), np.uint64(0))
    words[rng.random(m) < 0.02] = np.uint64(1) << np.uint64(63)
    # outside the offsets' range: what must not be read
    member[:first] = 2
    words[:first] = 1
    member[int(off[-1]):] = 2
    words[int(off[-1]):] = 1
    holds = rng.random(m) < 0.25
    return kinds, member, off, words, holds


def check_case(kinds, member, off, words, holds):
    got = E.exists_host(words, kinds, member, off)
    n = len(off) - 1
    assert got.dtype == np.uint8 and got.shape == (n,)
    seen = set()
    for i in range(n):
        lo, hi = int(off[i]), int(off[i + 1])
        ids = member[lo:hi]
        list_kinds = [int(kinds[g]) if g < len(kinds) else NUL for g in ids]  # past the end: no bundle
        found, consulted = reference_existence_lookup(list_kinds, words[lo:hi], holds[lo:hi])
        byte = int(got[i])
        assert byte in (0, 1, 2, 3), (i, byte)
        branch_holds = any(h for k, h in zip(list_kinds, holds[lo:hi]) if k == U)
        assert found == bool(byte & 1 or branch_holds), (i, byte, found, branch_holds)
        assert (byte == 0) == (consulted == 0 and not found), (i, byte, consulted, found)
        if byte == 2:  # the caller's part: the list's unfiltered bundles decide
            assert found == branch_holds and consulted >= 1
        seen.add(byte)
    return seen


@pytest.mark.parametrize("first", [0, 1000])
@pytest.mark.parametrize("n", [1, 5, 64, 200])
def test_mirror_against_the_reference_lookup(n, first):
    rng = np.random.default_rng(1000 * n + first)
    seen = check_case(*random_case(rng, n, 9, first))
    if n >= 64:
        assert seen == {0, 1, 2, 3}


def test_lists_of_300_members():
    rng = np.random.default_rng(300)
    kinds, member, off, words, holds = random_case(rng, 64, 9, 7, long_lists=((10, 300), (11, 300), (12, 300), (40, 300)))
    # key 10: NULL members only; key 11: the only hit is the last id; key 12: only an unfiltered id, the last
    for k in (10, 11, 12):
        lo, hi = int(off[k]), int(off[k + 1])
        member[lo:hi] = 1
        words[lo:hi] = 0
    member[int(off[12]) - 1], words[int(off[12]) - 1] = 0, 5
    member[int(off[13]) - 1] = 2
    got = E.exists_host(words, kinds, member, off)
    assert (got[10], got[11], got[12]) == (0, E.EXISTS_FILTER_HIT, E.EXISTS_UNFILTERED)
    check_case(kinds, member, off, words, holds)


def test_empty_lists_and_no_keys():
    kinds = [F, U]
    off = np.array([3, 3, 5, 5], dtype=np.uint64)
    got = E.exists_host(np.ones(6, dtype=np.uint64), kinds, np.array([1, 1, 1, 9, 0, 1], dtype=np.uint32), off)
    assert got.tolist() == [0, 1, 0]  # key 1: id 9 is past the end, id 0 a filter with a word
    got = E.exists_host(np.zeros(0, dtype=np.uint64), kinds, np.zeros(0, dtype=np.uint32), np.array([0], dtype=np.uint64))
    assert got.shape == (0,)
    got = E.exists_host(np.ones(4, dtype=np.uint64), [], np.zeros(4, dtype=np.uint32), np.array([0, 2, 4], dtype=np.uint64))
    assert got.tolist() == [0, 0]  # a set without members


def test_words_of_other_kinds_are_not_read():
    kinds = [NUL, U, F]
    member = np.array([0, 1, 2, 0, 1, 0], dtype=np.uint32)
    off = np.array([0, 3, 5, 6], dtype=np.uint64)
    words = np.array([7, 7, 0, 7, 7, 7], dtype=np.uint64)
    assert E.exists_host(words, kinds, member, off).tolist() == [2, 2, 0]
    words[2] = 1 << 40
    assert E.exists_host(words, kinds, member, off).tolist() == [3, 2, 0]


@pytest.mark.parametrize("with_member", [False, True])
@pytest.mark.parametrize("K", [1, 4, 9, 65])
def test_fixed_mirror(K, with_member):
    rng = np.random.default_rng(K)
    n, nm = 37, 9
    kinds = rng.integers(0, 3, size=nm)
    words = np.where(rng.random(n * K) < 0.1, rng.integers(1, 1 << 64, size=n * K, dtype=np.uint64), np.uint64(0))
    member = rng.integers(0, nm + 2, size=n * K).astype(np.uint32) if with_member else None
    ids = member if with_member else np.tile(np.arange(K, dtype=np.uint32), n)
    want = E.exists_host(words, kinds, ids, np.arange(n + 1, dtype=np.uint64) * np.uint64(K))
    got = E.exists_host_fixed(words, kinds, member, K)
    assert got.tolist() == want.tolist()
    check_case(kinds, ids, np.arange(n + 1, dtype=np.uint64) * np.uint64(K), words, rng.random(n * K) < 0.25)
