"""The ragged multi-get's host mirror: E.ragged_pair_keys (the key that owns each pair of a CSR
of per-key member lists) against a plain loop over the offsets, alone and composed with
E.found_candidates, whose record indices are pair positions relative to offsets[0]."""
import numpy as np
import pytest

from splinterdb_amd import engine as E


def loop_keys(off, pair_index):
    """the definition: pair p (relative to off[0]) belongs to the key k with off[k] <= p < off[k+1]"""
    out = []
    for q in pair_index:
        p = int(q) + int(off[0])
        hit = [k for k in range(len(off) - 1) if int(off[k]) <= p < int(off[k + 1])]
        assert len(hit) == 1, (p, hit)
        out.append(hit[0])
    return np.array(out, dtype=np.int64)


CASES = {
    "plain": ([2, 3, 1], 0),
    "empty_start_middle_end": ([0, 0, 2, 0, 0, 0, 3, 1, 0, 0], 0),
    "first_offset_not_zero": ([0, 4, 0, 1, 7, 0], 1000),
    "one_long_list": ([0, 300, 1], 17),
    "single_key": ([5], 3),
}


@pytest.mark.parametrize("name", list(CASES))
def test_ragged_pair_keys_vs_loop(name):
    counts, first = CASES[name]
    off = (np.concatenate([[0], np.cumsum(counts)]) + first).astype(np.uint64)
    m = int(off[-1] - off[0])
    every = np.arange(m, dtype=np.uint64)
    got = E.ragged_pair_keys(off, every)
    assert got.dtype == np.int64
    assert (got == loop_keys(off, every)).all()
    assert (got == np.repeat(np.arange(len(counts)), counts)).all()
    # both sides of every list boundary, in any order and repeated
    rel = off.astype(np.int64) - int(off[0])
    edge = np.concatenate([rel - 1, rel, rel])
    edge = edge[(edge >= 0) & (edge < m)][::-1]
    assert (E.ragged_pair_keys(off, edge) == loop_keys(off, edge)).all()
    assert (np.asarray(counts)[got] > 0).all(), "an empty list owns a pair"
    # int64 offsets (a torch tensor's dtype) are taken as they are
    assert (E.ragged_pair_keys(off.view(np.int64), every) == got).all()


def test_ragged_pair_keys_no_pairs():
    off = np.array([7, 7, 7], dtype=np.uint64)
    assert E.ragged_pair_keys(off, np.zeros(0, dtype=np.uint64)).shape == (0,)


def test_composed_with_found_candidates():
    """records of the words of a ragged probe -> (key, position in the key's list, value)"""
    rng = np.random.default_rng(5)
    counts = rng.integers(0, 6, size=200)
    counts[[0, 1, 50, 51, 52, 199]] = 0
    counts[77] = 130
    off = (np.concatenate([[0], np.cumsum(counts)]) + 1000).astype(np.uint64)
    m = int(off[-1] - off[0])
    words = np.where(rng.random(m) < 0.3, np.uint64(1) << rng.integers(0, 64, size=m).astype(np.uint64), np.uint64(0))
    words |= np.where(rng.random(m) < 0.1, np.uint64(1) << rng.integers(0, 64, size=m).astype(np.uint64), np.uint64(0))
    rec = E.found_candidates(words)
    key = E.ragged_pair_keys(off, rec >> np.uint64(8))
    want = []
    for k in range(len(counts)):
        for j in range(counts[k]):
            w = int(words[int(off[k]) - 1000 + j])
            want += [(k, j, v) for v in range(63, -1, -1) if w >> v & 1]
    slot = (rec >> np.uint64(8)).astype(np.int64) + 1000 - off.astype(np.int64)[key]
    got = list(zip(key.tolist(), slot.tolist(), (rec & np.uint64(0xff)).tolist()))
    assert got == want and len(want) > 50
    assert any(a[:2] == b[:2] for a, b in zip(got, got[1:])), "no word with two values"
