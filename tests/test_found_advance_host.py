"""The host mirror of rf_amd_found_advance (E.found_advance_host, CPU only) against a plain
transcription of the loop it stands for: trunk_ondisk_bundle_merge_lookup (src/trunk.c:6057-6087)
walks a key's candidates in order and stops behind the first definitive one (:6085). The mirror is
the oracle of every GPU test of the call (test_gpu_found_advance.py).

Every case takes the mirror as a parameter, so that test_cases_bite can hand it three broken
mirrors -- the source of found_advance_host with one line changed, compiled in memory -- and see
the named case fail."""
import inspect

import numpy as np
import pytest

from splinterdb_amd import engine as E


def transcription(key_off, cand_cap, definitive):
    """per key, the record indices the reference's loop looks up: in order, out behind the first
    definitive one"""
    looks = []
    for i in range(len(key_off) - 1):
        mine = []
        for j in range(int(key_off[i]), min(int(key_off[i + 1]), cand_cap)):
            mine.append(j)
            if definitive[j]:
                break
        looks.append(mine)
    return looks


def drive(mirror, key_off, cand, cand_cap, width, definitive, out_cap):
    """the consumer's loop over the mirror: advance, look the written records up, mark the keys
    that met a definitive record. definitive None: done is never passed. Returns per key the list
    of (step, record index) of its lookups; cand[j] == 3 * j + 1 names the record."""
    n = len(key_off) - 1
    looks = [[] for _ in range(n)]
    done = None if definitive is None else np.zeros(n, dtype=np.uint8)
    cursor = None
    for step in range(10 ** 6):
        before = np.zeros(n, dtype=np.uint32) if cursor is None else cursor
        out_cand, out_key, count, cursor = mirror(key_off, cand, cand_cap, width, done, cursor, out_cap)
        assert out_cand.dtype == np.uint64 and out_key.dtype == np.uint64 and cursor.dtype == np.uint32
        assert out_cand.size == out_key.size == min(count, out_cap) and cursor.size == n
        assert (np.diff(out_key.astype(np.int64)) >= 0).all()  # batch order
        assert (np.bincount(out_key.astype(np.int64), minlength=n) == cursor - before).all()
        if count == 0:
            return looks
        for c, k in zip(out_cand.tolist(), out_key.tolist()):
            assert c % 3 == 1
            j = c // 3
            looks[k].append((step, j))
            if definitive is not None and definitive[j]:
                done[k] = 1
    raise AssertionError("the steps do not end")


def random_csr(rng, n, mean, cut):
    """n keys with geometric record counts, some of them long; cut: cand_cap below the total"""
    cnt = rng.geometric(1.0 / (1.0 + mean), size=n) - 1
    if n:
        cnt[rng.integers(0, n, size=max(1, n // 20))] += rng.integers(5, 200, size=max(1, n // 20))
    key_off = np.concatenate(([0], np.cumsum(cnt))).astype(np.uint64)
    total = int(key_off[-1])
    cand = (3 * np.arange(total, dtype=np.uint64) + 1)
    cand_cap = total if not cut else int(rng.integers(0, total + 1))
    return key_off, cand, cand_cap


def worlds():
    rng = np.random.default_rng(7)
    for n, mean, cut in ((0, 1, False), (1, 3, False), (50, 0.3, False), (200, 2.0, False), (200, 2.0, True),
                         (333, 5.0, True)):
        key_off, cand, cand_cap = random_csr(rng, n, mean, cut)
        definitive = rng.random(cand.size) < 0.3
        yield key_off, cand, cand_cap, definitive


def case_width_one_is_the_loop(mirror):
    for key_off, cand, cand_cap, definitive in worlds():
        want = transcription(key_off, cand_cap, definitive)
        for out_cap in (1 << 40, 7):
            got = drive(mirror, key_off, cand, cand_cap, 1, definitive, out_cap)
            assert [[j for _, j in g] for g in got] == want
            if out_cap > cand.size:  # nothing is cut: lookup s of a key is made in step s
                assert all([s for s, _ in g] == list(range(len(g))) for g in got)


def case_wider_steps_extend_the_loop(mirror):
    for key_off, cand, cand_cap, definitive in worlds():
        want = transcription(key_off, cand_cap, definitive)
        for width in (2, 3, 64):
            for out_cap in (1 << 40, 11):
                got = drive(mirror, key_off, cand, cand_cap, width, definitive, out_cap)
                for g, w in zip(got, want):
                    js = [j for _, j in g]
                    assert js[:len(w)] == w  # a prefix-extension
                    extras = g[len(w):]
                    assert len(extras) <= width - 1
                    if extras:  # all in the step that held the definitive record
                        assert definitive[w[-1]]
                        assert {s for s, _ in extras} == {g[len(w) - 1][0]}
                        assert [j for _, j in extras] == list(range(w[-1] + 1, w[-1] + 1 + len(extras)))


def case_every_record_once_for_any_out_cap(mirror):
    for key_off, cand, cand_cap, _ in worlds():
        for width in (1, 3, 64, (1 << 32) - 1):
            for out_cap in (1, 2, 5, 64, 1 << 40):
                got = drive(mirror, key_off, cand, cand_cap, width, None, out_cap)
                for i, g in enumerate(got):
                    assert [j for _, j in g] == list(range(int(key_off[i]), min(int(key_off[i + 1]), cand_cap)))


def case_nothing_at_or_past_cand_cap(mirror):
    # 3 keys of 4 records; the cap inside key 1 and at the boundary behind it
    key_off = np.array([0, 4, 8, 12], dtype=np.uint64)
    cand = 3 * np.arange(12, dtype=np.uint64) + 1
    for cand_cap, want in ((6, [4, 2, 0]), (8, [4, 4, 0]), (0, [0, 0, 0]), (12, [4, 4, 4]), (99, [4, 4, 4])):
        out_cand, out_key, count, cursor = mirror(key_off, cand, cand_cap, 64, None, None, 100)
        assert count == sum(want) and cursor.tolist() == want
        assert out_cand.tolist() == [3 * j + 1 for i in range(3) for j in range(4 * i, 4 * i + want[i])]


CASES = {f.__name__: f for f in (case_width_one_is_the_loop, case_wider_steps_extend_the_loop,
                                 case_every_record_once_for_any_out_cap, case_nothing_at_or_past_cand_cap)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_mirror(case):
    CASES[case](E.found_advance_host)


# one line of the mirror changed -> the case that must notice
MUTATIONS = {
    "cursor advanced by take": ("new_cursor = cur + wr", "new_cursor = cur + take",
                                "case_every_record_once_for_any_out_cap"),
    "done ignored": ("    if done is not None:\n", "    if False:\n", "case_width_one_is_the_loop"),
    "no clamp at cand_cap": ("e = np.minimum(off[1:], cand_cap)", "e = off[1:]", "case_nothing_at_or_past_cand_cap"),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_cases_bite(name):
    old, new, case = MUTATIONS[name]
    src = inspect.getsource(E.found_advance_host)
    assert src.count(old) == 1
    scope = dict(vars(E))
    exec(compile(src.replace(old, new), "<mutated mirror>", "exec"), scope)
    with pytest.raises(AssertionError):
        CASES[case](scope["found_advance_host"])
    CASES[case](E.found_advance_host)  # and the mirror as it stands passes it


def test_take_is_bounded_and_cursors_past_the_end_stay():
    key_off = np.array([0, 3, 3, 10], dtype=np.uint64)
    cand = 3 * np.arange(10, dtype=np.uint64) + 1
    cursor = np.array([5, 0, 2], dtype=np.uint32)  # past key 0's end; nothing to pass in key 1
    out_cand, out_key, count, new = E.found_advance_host(key_off, cand, 10, 2, None, cursor, 100)
    assert count == 2 and out_key.tolist() == [2, 2] and out_cand.tolist() == [16, 19] and new.tolist() == [5, 0, 4]
    done = np.array([0, 0, 1], dtype=np.uint8)
    out_cand, out_key, count, new = E.found_advance_host(key_off, cand, 10, 2, done, cursor, 100)
    assert count == 0 and out_cand.size == 0 and new.tolist() == [5, 0, 2]
    # out_cap 0: the true total, nothing written, no cursor moves
    out_cand, out_key, count, new = E.found_advance_host(key_off, cand, 10, 64, None, None, 0)
    assert count == 10 and out_cand.size == 0 and new.tolist() == [0, 0, 0]
    for width in (0, 1 << 32):
        with pytest.raises(ValueError):
            E.found_advance_host(key_off, cand, 10, width, None, None, 5)
    assert E.ADVANCE_MAX_TAKE == 65535 * 64


def test_refuses_a_null_engine_without_a_device():
    L = E.load_library()
    x = 8  # a non-null, 8-byte aligned address that nothing reads: the call is refused first
    for n in (10, 0):
        rc = L.rf_amd_found_advance(None, x, x, 100, n, 1, E.ADVANCE_FIRST, None, x, x, x, 100, x, x, None)
        assert rc == E.STATUS_BAD_PARAM
        assert b"null engine" in L.rf_amd_last_error()


def test_python_names():
    for name in ("found_advance", "found_advance_host", "found_advance_scratch_bytes"):
        assert callable(getattr(E, name))
    assert E.ADVANCE_FIRST == 1
    assert callable(E.FilterSet.lookup_steps) and callable(E.LookupSteps.step)
    assert "rf_amd_found_advance" in E.EXPORTED and "rf_amd_found_advance_scratch_bytes" in E.EXPORTED
