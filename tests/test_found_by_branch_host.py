"""The host mirror of rf_amd_found_by_branch (E.found_by_branch_host, CPU only) against a plain
transcription of what the call is for: a dict from (member, value) to the list of the positions j
of that branch's records in input order, walked with its keys sorted. The mirror is the oracle of
every GPU test of the call (test_gpu_found_by_branch.py)."""
import numpy as np
import pytest

from splinterdb_amd import engine as E


def transcription(cand, num_members, cand_key=None):
    """records -> (order, order_key, branch, branch_off) by a dict of lists; ids are masked to the
    bit width of num_members - 1 and values to 6 bits, as the call's sort key does"""
    mb = (num_members - 1).bit_length()
    groups = {}
    for j, c in enumerate(int(x) for x in cand):
        groups.setdefault(((c >> 8) & ((1 << mb) - 1), c & 63), []).append(j)
    order, branch, off = [], [], [0]
    for k in sorted(groups):
        branch.append(int(cand[groups[k][0]]))
        order += groups[k]
        off.append(len(order))
    okey = None if cand_key is None else [int(cand_key[j]) for j in order]
    return order, okey, branch, off


def check(cand, num_members, cand_key=None):
    cand = np.asarray(cand, dtype=np.uint64)
    order, okey, branch, off = E.found_by_branch_host(cand, num_members, cand_key)
    w_order, w_okey, w_branch, w_off = transcription(cand, num_members, cand_key)
    assert order.dtype == np.uint32 and branch.dtype == np.uint64 and off.dtype == np.uint64
    assert order.tolist() == w_order and branch.tolist() == w_branch and off.tolist() == w_off
    if cand_key is None:
        assert okey is None
    else:
        assert okey.dtype == np.uint64 and okey.tolist() == w_okey
    return order, okey, branch, off


def records(rng, m, num_members, id_limit=None):
    ids = rng.integers(0, id_limit or num_members, size=m, dtype=np.uint64)
    return (ids << np.uint64(8)) | rng.integers(0, 64, size=m, dtype=np.uint64)


@pytest.mark.parametrize("num_members", [1, 2, 4, 5, 64, 1000, 1 << 18, 1 << 26])
def test_random(num_members):
    rng = np.random.default_rng(num_members)
    cand = records(rng, 3000, num_members)
    cand[:500] = records(rng, 500, min(num_members, 3))  # long runs too
    key = np.sort(rng.integers(0, 1 << 40, size=3000, dtype=np.uint64))
    order, okey, branch, off = check(cand, num_members, key)
    assert sorted(order.tolist()) == list(range(3000))
    for u in range(len(branch)):  # a run is one branch, in input order: the batch's key order
        run = order[int(off[u]):int(off[u + 1])]
        assert (np.diff(run.astype(np.int64)) > 0).all() and (cand[run] == branch[u]).all()
        assert (np.diff(okey[int(off[u]):int(off[u + 1])].astype(np.int64)) >= 0).all()
    check(cand, num_members)


def test_ids_at_or_above_num_members_are_masked():
    # 5 members: 3 bits. Id 8 sorts as id 0 and id 13 as id 5, behind the records before them; the
    # branch table keeps the full record of a run's first element
    cand = np.array([(13 << 8) | 2, (8 << 8) | 1, (0 << 8) | 1, (5 << 8) | 2, (0xFFFFFFFF << 8) | 63, (7 << 8) | 63],
                    dtype=np.uint64)
    order, _, branch, off = check(cand, 5)
    assert order.tolist() == [1, 2, 0, 3, 4, 5]
    assert branch.tolist() == [(8 << 8) | 1, (13 << 8) | 2, (0xFFFFFFFF << 8) | 63] and off.tolist() == [0, 2, 4, 6]
    # bits 6 and 7 of the value byte are no part of the key
    order, _, branch, off = check(np.array([(1 << 8) | 0x83, (1 << 8) | 3], dtype=np.uint64), 2)
    assert order.tolist() == [0, 1] and branch.tolist() == [(1 << 8) | 0x83] and off.tolist() == [0, 2]
    rng = np.random.default_rng(3)
    check(records(rng, 2000, 5, id_limit=1 << 32), 5)
    check(records(rng, 2000, 1 << 26, id_limit=1 << 32), 1 << 26)


def test_one_member():
    rng = np.random.default_rng(1)
    order, _, branch, off = check(records(rng, 1000, 1), 1)
    assert len(branch) == 64 and (branch >> np.uint64(8) == 0).all()
    # every id is masked to 0 bits: the value alone groups
    order, _, branch, off = check(np.array([(9 << 8) | 5, (3 << 8) | 5, 4], dtype=np.uint64), 1)
    assert order.tolist() == [2, 0, 1] and branch.tolist() == [4, (9 << 8) | 5] and off.tolist() == [0, 1, 3]


def test_empty_and_single():
    order, okey, branch, off = check(np.zeros(0, dtype=np.uint64), 7, np.zeros(0, dtype=np.uint64))
    assert order.size == 0 and okey.size == 0 and branch.size == 0 and off.tolist() == [0]
    order, okey, branch, off = check(np.array([(6 << 8) | 63], dtype=np.uint64), 7, np.array([11], dtype=np.uint64))
    assert order.tolist() == [0] and okey.tolist() == [11] and off.tolist() == [0, 1]


def test_refuses_num_members_outside_the_call():
    for nm in (0, (1 << 26) + 1):
        with pytest.raises(ValueError):
            E.found_by_branch_host(np.zeros(3, dtype=np.uint64), nm)
