"""Host side of the multi-get: E.found_candidates, the numpy mirror of rf_amd_found_compact (the
set bits of found_values words as records index << 8 | value, index ascending, value descending
within a word -- routing_filter_get_next_value's order, src/routing_filter.h:94-105), and the
scratch sizing, which needs no device."""
import numpy as np

from splinterdb_amd import engine as E


def fixed_words():
    rng = np.random.default_rng(5)
    sparse = np.zeros(1000, dtype=np.uint64)
    hit = rng.random(1000) < 0.15
    for _ in range(2):  # words with one or two bits
        bit = rng.integers(0, 64, size=1000).astype(np.uint64)
        sparse |= np.where(hit & (rng.random(1000) < 0.6), np.uint64(1) << bit, np.uint64(0))
    head = np.array([0, 1, 1 << 63, 0xFFFFFFFFFFFFFFFF, (1 << 5) | (1 << 3) | 1], dtype=np.uint64)
    return np.concatenate([head, sparse])


def test_found_candidates_order_and_count():
    w = fixed_words()
    c = E.found_candidates(w)
    assert c.dtype == np.uint64
    idx, val = (c >> np.uint64(8)).astype(np.int64), (c & np.uint64(0xFF)).astype(np.int64)
    assert (np.diff(idx) >= 0).all()
    same = np.diff(idx) == 0
    assert (np.diff(val)[same] < 0).all()
    assert len(c) == sum(bin(int(x)).count("1") for x in w)
    assert (val < 64).all() and (idx < len(w)).all()
    assert len(c) > 69 and same.sum() > 63  # the sparse words took part, some with two bits


def test_found_candidates_values_per_word():
    w = fixed_words()
    c = E.found_candidates(w)
    idx, val = (c >> np.uint64(8)).astype(np.int64), (c & np.uint64(0xFF)).astype(np.int64)
    low = 0
    for i, x in enumerate(int(x) for x in w):
        got = val[idx == i].tolist()
        assert got == [b for b in range(63, -1, -1) if x >> b & 1], i
        if x < (1 << 31):  # the reference's walk (its `1 << last_value` is an int shift)
            seq, last = [], E.ROUTING_NOT_FOUND
            while True:
                last = E.routing_filter_get_next_value(x, last)
                if last == E.ROUTING_NOT_FOUND:
                    break
                seq.append(last)
            assert got == seq, i
            low += bool(seq)
    assert low > 10
    assert E.found_candidates(np.zeros(0, dtype=np.uint64)).size == 0
    assert E.found_candidates(np.zeros(7, dtype=np.uint64)).size == 0
    five = E.found_candidates(np.array([(1 << 5) | (1 << 3) | 1], dtype=np.uint64))
    assert five.tolist() == [5, 3, 0]


def test_found_compact_scratch_bytes_needs_no_device():
    L = E.load_library()
    f = L.rf_amd_found_compact_scratch_bytes
    assert f(0) <= 64
    prev = f(0)
    for m in [1, 63, 64, 65, 4095, 4096, 4097, 1 << 20, (1 << 20) + 1, 1 << 30, 1 << 40, (1 << 56) - 1]:
        cur = f(m)
        assert cur >= prev, m
        prev = cur
    assert E.found_compact_scratch_bytes(1 << 20) == f(1 << 20)
