"""The stepwise hand-out of per-key candidates: rf_amd_found_advance (k_advance_count,
k_range_scan, k_advance_emit), E.found_advance and FilterSet.lookup_steps. The oracle of every
buffer is the host mirror (E.found_advance_host, checked against a plain transcription of the
reference's loop in test_found_advance_host.py): d_out_cand, d_out_key, *d_out_count and d_cursor
must equal it byte for byte, and every output lies between sentinel words that must stay as they
were. The call works on any CSR of records, so most cases are synthetic and need no filter; the
end-to-end test runs in test_gpu_multiget's world."""
import numpy as np
import pytest

import test_gpu_multiget as MG
import test_gpu_range_route as RR
from splinterdb_amd import engine as E
from test_gpu_multiget import world  # noqa: F401  (the fixture; a fresh instance for this module)
from test_gpu_range_route import routed  # noqa: F401  (keys and oracle words of both key forms)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = MG.N
SENT = 512
TILE = E.diag_per_key_tile()
BIG = 3 * TILE + 77  # three whole tiles and a partial one
SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, BIG]
ALL = (1 << 32) - 1  # the width that means all
WIDTHS = [1, 2, 64, ALL]
LONG = 5000  # more than a row's step of 256 positions and more than any width but ALL
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
POISON = 0xDEADBEEF


def dev(a):
    """a host array on the device; unsigned words travel as the signed type of their width"""
    a = np.array(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return MG.dev(a if signed is None else a.view(signed))


# ---- the per-key record counts: (n, rng) -> n counts -------------------------------------------
def all_empty(n, rng):
    return np.zeros(n, dtype=np.int64)


def all_one(n, rng):
    return np.ones(n, dtype=np.int64)


def alternating(n, rng):
    return np.where(np.arange(n) & 1, 3, 0).astype(np.int64)


def geometric(n, rng):
    """mean 1.1"""
    return (rng.geometric(1.0 / 2.1, size=n) - 1).astype(np.int64)


def one_long(n, rng):
    c = np.zeros(n, dtype=np.int64)
    if n:
        c[n // 2] = LONG
    return c


def last_only(n, rng):
    c = np.zeros(n, dtype=np.int64)
    if n:
        c[-1] = 70
    return c


DISTS = [all_empty, all_one, alternating, geometric, one_long, last_only]


def csr(cnt, rng):
    """(key_off uint64[n + 1], cand uint64[total]) with records that name their position"""
    key_off = np.concatenate(([0], np.cumsum(cnt))).astype(np.uint64)
    total = int(key_off[-1])
    cand = (rng.integers(0, 1 << 20, size=total, dtype=np.uint64) << np.uint64(40)) | \
        (np.arange(total, dtype=np.uint64) << np.uint64(8)) | rng.integers(0, 64, size=total, dtype=np.uint64)
    return key_off, cand


def dones(n, cnt, rng):
    """None, all set, random at 50 %, exactly the keys that have records"""
    return [None, np.ones(n, dtype=np.uint8), (rng.random(n) < 0.5).astype(np.uint8) * np.uint8(0x80),
            (cnt > 0).astype(np.uint8)]


# ---- one call between sentinels ----------------------------------------------------------------
def sentinel_buf(k, dtype=torch.int64):
    return torch.full((SENT + k + SENT,), -7, dtype=dtype, device="cuda:0")


def inner(buf, k, what):
    a = buf.cpu().numpy()
    assert (a[:SENT] == -7).all() and (a[SENT + k:] == -7).all(), "wrote outside " + what
    return a[SENT:SENT + k]


class Inputs:
    """a CSR on the device, uploaded once: d_cand holds cand[:cand_cap] and one word that no call
    may read"""

    def __init__(self, key_off, cand, cand_cap=None):
        self.key_off, self.cand = key_off, cand
        self.n = len(key_off) - 1
        self.cand_cap = len(cand) if cand_cap is None else cand_cap
        self.d_key_off = dev(key_off)
        self.d_cand = dev(np.append(cand[:self.cand_cap], ONES))


def raw_call(x, width, flags, done, cursor, out_cap, with_key=True, null_out=False, stream=None):
    """one call through the C ABI on outputs between sentinels; cursor: the n values before the
    call (None: poison, for FIRST). done travels to an odd address. Returns (out_cand
    uint64[out_cap] or None, out_key uint64[out_cap] or None, count, cursor uint32[n])"""
    L = E.load_library()
    n = x.n
    d_cursor = sentinel_buf(n, torch.int32)
    before = np.full(n, POISON, dtype=np.uint32) if cursor is None else np.asarray(cursor, dtype=np.uint32)
    d_cursor[SENT:SENT + n] = dev(before)
    d_out = None if null_out else sentinel_buf(out_cap)
    d_key = sentinel_buf(out_cap) if with_key and not null_out else None
    d_count = sentinel_buf(1)
    d_done = None
    if done is not None:
        d_done = torch.zeros(n + 9, dtype=torch.uint8, device="cuda:0")
        assert (d_done.data_ptr() + 1) % 2 == 1
        d_done[1:1 + n] = dev(np.asarray(done, dtype=np.uint8))
    scratch = torch.empty(E.found_advance_scratch_bytes(n) // 8, dtype=torch.int64, device="cuda:0")

    def at(b, size=8):
        return None if b is None else b.data_ptr() + size * SENT
    torch.cuda.synchronize()
    rc = L.rf_amd_found_advance(E.default_engine().h, x.d_key_off.data_ptr(), x.d_cand.data_ptr(), x.cand_cap, n,
                                width, flags, None if d_done is None else d_done.data_ptr() + 1, at(d_cursor, 4),
                                at(d_out), at(d_key), out_cap, at(d_count), scratch.data_ptr(), stream)
    assert rc == 0, L.rf_amd_last_error()
    torch.cuda.synchronize()
    return (None if d_out is None else inner(d_out, out_cap, "d_out_cand[0, out_cap)").view(np.uint64),
            None if d_key is None else inner(d_key, out_cap, "d_out_key[0, out_cap)").view(np.uint64),
            int(inner(d_count, 1, "d_out_count")[0]),
            inner(d_cursor, n, "d_cursor[0, n)").view(np.uint32))


def check(got, x, width, first, done, cursor, out_cap, what):
    out, key, count, cur = got
    w_out, w_key, w_count, w_cur = E.found_advance_host(x.key_off, x.cand, x.cand_cap, width, done,
                                                        None if first else cursor, out_cap)
    assert count == w_count, (what, "count", count, w_count)
    assert cur.tobytes() == w_cur.tobytes(), (what, "cursor", np.flatnonzero(cur != w_cur)[:8].tolist())
    m = min(count, out_cap)
    assert m == len(w_out)
    if out is not None:
        bad = np.flatnonzero(out[:m] != w_out)
        assert bad.size == 0, (what, "out_cand", bad.size, bad[:8].tolist())
        assert (out[m:].view(np.int64) == -7).all(), (what, "wrote past the records")
    if key is not None:
        assert key[:m].tobytes() == w_key.tobytes(), (what, "out_key")
        assert (key[m:].view(np.int64) == -7).all(), (what, "wrote past the keys")
    return w_count


def run_case(x, width, what, first=False, done=None, cursor=None, out_cap=None, **kw):
    """one call and its check; cursor None: zeros without FIRST, poison with it; out_cap None: the
    mirror's total and 5 words more"""
    if cursor is None and not first:
        cursor = np.zeros(x.n, dtype=np.uint32)
    if out_cap is None:
        out_cap = E.found_advance_host(x.key_off, x.cand, x.cand_cap, width, done, None if first else cursor,
                                       0)[2] + 5
    got = raw_call(x, width, E.ADVANCE_FIRST if first else 0, done, None if first else cursor, out_cap, **kw)
    check(got, x, width, first, done, cursor, out_cap, what)
    return got


# ---- every size, distribution, width and done --------------------------------------------------
def test_cases_exist():
    rng = np.random.default_rng(0)
    assert BIG > 3 * TILE and BIG % TILE and TILE % 256 == 0 and LONG > 4 * 64 and LONG > 64
    g = geometric(100000, rng)
    assert abs(g.mean() - 1.1) < 0.02 and (g == 0).any() and g.max() > 8
    assert one_long(BIG, rng).sum() == LONG and last_only(BIG, rng)[-1] > 0 and last_only(BIG, rng)[:-1].sum() == 0
    assert alternating(4, rng).tolist() == [0, 3, 0, 3]


@pytest.mark.parametrize("dist", DISTS, ids=lambda f: f.__name__)
def test_sizes(dist):
    """every n, width and done of this distribution, from cursors at 0 and from cursors anywhere
    up to one past the key's end"""
    rng = np.random.default_rng(11 + DISTS.index(dist))
    for n in SIZES:
        cnt = dist(n, rng)
        x = Inputs(*csr(cnt, rng))
        for wi, width in enumerate(WIDTHS):
            for di, done in enumerate(dones(n, cnt, rng)):
                cursor = None if (wi + di) & 1 else rng.integers(0, cnt + 2, size=n).astype(np.uint32)
                got = run_case(x, width, (dist.__name__, n, width, di), done=done, cursor=cursor)
                if di in (1, 3):
                    assert got[2] == 0


def test_n_zero_writes_the_count_alone():
    x = Inputs(np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64))
    for first in (False, True):
        out, key, count, cur = run_case(x, 3, "n 0", first=first, out_cap=4)
        assert count == 0 and (out.view(np.int64) == -7).all() and (key.view(np.int64) == -7).all()
    # and with every pointer NULL that may be
    L = E.load_library()
    d_count = sentinel_buf(1)
    rc = L.rf_amd_found_advance(E.default_engine().h, None, None, 10, 0, 1, 0, None, None, None, None, 0,
                                d_count.data_ptr() + 8 * SENT, None, None)
    assert rc == 0, L.rf_amd_last_error()
    torch.cuda.synchronize()
    assert inner(d_count, 1, "d_out_count")[0] == 0


# ---- caps, cursors and grids -------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """BIG keys with geometric counts and one long key in the second tile, made once and
    read-only, and random definitive flags for the records"""
    rng = np.random.default_rng(42)
    cnt = geometric(BIG, rng)
    cnt[TILE + 100] = LONG
    key_off, cand = csr(cnt, rng)
    definitive = rng.random(cand.size) < 0.3
    for a in (cnt, key_off, cand, definitive):
        a.setflags(write=False)
    return Inputs(key_off, cand), cnt, definitive


def test_out_cap(big):
    x, cnt, _ = big
    total = int(x.key_off[-1])
    cut = int(x.key_off[TILE + 100]) + LONG // 2  # in the middle of the long key
    for out_cap in (1, cut, total, total + 9):
        out, key, count, cur = run_case(x, ALL, ("out_cap", out_cap), out_cap=out_cap)
        assert count == total and int(cur.astype(np.int64).sum()) == min(total, out_cap)
    assert cur.tolist() == cnt.tolist()
    out, key, count, cur = run_case(x, ALL, "cut", out_cap=cut)
    assert cur[TILE + 100] == LONG // 2 and (cur[TILE + 101:] == 0).all() and (cur[:TILE + 100] == cnt[:TILE + 100]).all()
    # out_cap 0 with NULL outputs: the count, and no cursor moves
    for first in (False, True):
        out, key, count, cur = run_case(x, ALL, "out_cap 0", first=first, out_cap=0, null_out=True)
        assert count == total and not cur.any()
    # with a narrower step too: the cut lands between two keys' single records
    for width in (1, 2):
        run_case(x, width, ("out_cap", width), out_cap=TILE + 7)
        run_case(x, width, ("out_cap", width, "first"), first=True, out_cap=TILE + 7)


def test_a_cut_key_gets_the_rest(big):
    """out_cap below the total, no done: the steps hand out every record once and in order"""
    x, cnt, _ = big
    total = int(x.key_off[-1])
    cursor, seen = np.zeros(BIG, dtype=np.uint32), []
    for step in range(20):
        out, key, count, cursor = run_case(x, ALL, ("rest", step), cursor=cursor, out_cap=3000)
        if count == 0:
            break
        seen.append(out[:min(count, 3000)])
    assert step == -(-total // 3000) and cursor.tolist() == cnt.tolist()
    # a step's records are in batch order and the steps follow each other: the whole list, in order
    assert np.concatenate(seen).tobytes() == x.cand.tobytes()


def test_cand_cap_below_the_last_offset(big):
    x, cnt, _ = big
    k = TILE + 100
    inside, boundary = int(x.key_off[k]) + 1234, int(x.key_off[k + 1])
    assert cnt[k + 1:].sum() > 0
    for cap in (inside, boundary, int(x.key_off[3]), 0):
        y = Inputs(x.key_off, x.cand, cap)
        for width in (1, ALL):
            out, key, count, cur = run_case(y, width, ("cand_cap", cap, width))
            assert count <= cap and (cap == 0 or count > 0)
        assert int(cur.astype(np.int64).sum()) == cap  # ALL: every record below the cap and none past it
        # cursors at the cap and past it take nothing
        cursor = np.minimum(cnt, 3).astype(np.uint32)
        run_case(y, 2, ("cand_cap", cap, "cursors"), cursor=cursor)


def test_first_ignores_the_cursors(big):
    x, cnt, definitive = big
    done = (np.random.default_rng(3).random(BIG) < 0.5).astype(np.uint8)
    for width in WIDTHS:
        a = run_case(x, width, ("first", width), first=True, done=done)
        b = run_case(x, width, ("zeroed", width), done=done)
        for p, q in zip(a, b):
            assert np.array_equal(p, q)
    # every one of the n cursors is written: keys that take nothing get 0
    out, key, count, cur = run_case(x, 1, "first, all done", first=True, done=np.ones(BIG, dtype=np.uint8))
    assert count == 0 and not cur.any()


def test_cursors_past_the_end_stay(big):
    x, cnt, _ = big
    rng = np.random.default_rng(4)
    cursor = (cnt + rng.integers(0, 3, size=BIG)).astype(np.uint32)  # at the end, and 1 and 2 past it
    cursor[7] = 0xFFFFFFFF
    out, key, count, cur = run_case(x, 64, "past the end", cursor=cursor)
    assert count == 0 and cur.tolist() == cursor.tolist()
    cursor[TILE + 100] = LONG - 1  # one key with one record left
    out, key, count, cur = run_case(x, 64, "one left", cursor=cursor)
    assert count == 1 and out[0] == x.cand[int(x.key_off[TILE + 100]) + LONG - 1] and key[0] == TILE + 100


def transcription(key_off, cand_cap, definitive, width):
    """the reference's loop taken `width` candidates at a time: per key the record indices looked
    up, in order, out behind the step that held the first definitive one (width 1:
    trunk_ondisk_bundle_merge_lookup itself)"""
    looks = []
    for i in range(len(key_off) - 1):
        mine, j, end = [], int(key_off[i]), min(int(key_off[i + 1]), cand_cap)
        while j < end:
            step = list(range(j, min(j + width, end)))
            mine += step
            j += width
            if any(definitive[s] for s in step):
                break
        looks.append(mine)
    return looks


@pytest.mark.parametrize("width", [1, 3])
def test_drive_to_completion(big, width):
    """advance, look up, mark done, until the count is 0: the union of the steps is the
    transcription's lookups, key by key and in order"""
    x, cnt, definitive = big
    want = transcription(x.key_off, x.cand_cap, definitive, width)
    index_of = {int(c): j for j, c in enumerate(x.cand)}
    looks = [[] for _ in range(BIG)]
    done, cursor = np.zeros(BIG, dtype=np.uint8), None
    for step in range(-(-LONG // width) + 2):
        out, key, count, cursor = run_case(x, width, ("drive", width, step), first=step == 0, done=done,
                                           cursor=cursor)
        if count == 0:
            break
        for c, k in zip(out[:count].tolist(), key[:count].tolist()):
            j = index_of[c]
            looks[k].append(j)
            if definitive[j]:
                done[k] = 1
    assert count == 0 and looks == want
    assert step == max(-(-len(w) // width) for w in want)  # as many steps as the longest walk


@pytest.mark.parametrize("blocks", [1, 3])
def test_grid_stride_loops(big, blocks):
    """four tiles on one and on three workgroups: both tile loops run more than once"""
    x, cnt, definitive = big
    rng = np.random.default_rng(blocks)
    done = (rng.random(BIG) < 0.5).astype(np.uint8)
    try:
        E.diag_fanout_max_blocks(blocks)
        for width in WIDTHS:
            run_case(x, width, (blocks, width), done=done,
                     cursor=rng.integers(0, cnt + 2, size=BIG).astype(np.uint32))
            run_case(x, width, (blocks, width, "first"), first=True)
        run_case(x, ALL, (blocks, "cut"), out_cap=int(x.key_off[TILE + 100]) + 77)
    finally:
        E.diag_fanout_max_blocks(0)


def test_two_runs_give_identical_bytes(big):
    x, cnt, _ = big
    done = (np.random.default_rng(5).random(BIG) < 0.5).astype(np.uint8)
    cursor = np.minimum(cnt, 1).astype(np.uint32)
    a = raw_call(x, 3, 0, done, cursor, 500)
    b = raw_call(x, 3, 0, done, cursor, 500)
    for p, q in zip(a, b):
        assert np.array_equal(p, q)
    assert a[2] > 500  # and the cut was real


def test_without_out_key(big):
    x, cnt, _ = big
    for first in (False, True):
        got = run_case(x, 2, ("no keys", first), first=first, with_key=False)
        assert got[1] is None and got[2] > 2 * TILE  # records of more than one tile


def test_on_a_stream_of_the_callers(big):
    x, cnt, _ = big
    s = torch.cuda.Stream()
    run_case(x, 2, "stream", first=True, stream=s.cuda_stream)


# ---- the Python call and the refusals ----------------------------------------------------------
def test_python_call(big):
    x, cnt, _ = big
    done = (np.random.default_rng(6).random(BIG) < 0.5).astype(np.uint8)
    w_out, w_key, w_count, w_cur = E.found_advance_host(x.key_off, x.cand, x.cand_cap, 2, done, None, 1 << 40)
    d_cursor = torch.full((BIG,), 77, dtype=torch.int32, device="cuda:0")
    d_out = torch.empty(w_count, dtype=torch.int64, device="cuda:0")
    d_key = torch.empty(w_count, dtype=torch.int64, device="cuda:0")
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    E.found_advance(x.d_key_off, x.d_cand, x.cand_cap, BIG, 2, E.ADVANCE_FIRST, dev(done), d_cursor, d_out, d_key,
                    w_count, d_count)
    torch.cuda.synchronize()
    assert int(d_count.item()) == w_count
    assert d_out.cpu().numpy().view(np.uint64).tobytes() == w_out.tobytes()
    assert d_key.cpu().numpy().view(np.uint64).tobytes() == w_key.tobytes()
    assert d_cursor.cpu().numpy().view(np.uint32).tobytes() == w_cur.tobytes()
    with pytest.raises(ValueError):
        E.found_advance(x.d_key_off, x.d_cand, x.cand_cap, BIG, 2, 0, None, d_cursor, d_out[:8], d_key, w_count,
                        d_count)


def test_errors(big):
    x, cnt, _ = big
    L = E.load_library()
    h = E.default_engine().h
    B = E.STATUS_BAD_PARAM
    t = {k: torch.zeros(m, dtype=torch.int64, device="cuda:0")
         for k, m in (("cursor", BIG), ("out", 64), ("key", 64), ("count", 1), ("done", BIG))}
    t["scr"] = torch.zeros(E.found_advance_scratch_bytes(BIG) // 8, dtype=torch.int64, device="cuda:0")
    p = {k: v.data_ptr() for k, v in t.items()}
    p["off"], p["cand"] = x.d_key_off.data_ptr(), x.d_cand.data_ptr()

    def call(e=h, off=p["off"], c=p["cand"], cc=x.cand_cap, n=BIG, w=1, f=0, d=p["done"], cu=p["cursor"],
             o=p["out"], k=p["key"], oc=64, ct=p["count"], s=p["scr"]):
        return L.rf_amd_found_advance(e, off, c, cc, n, w, f, d, cu, o, k, oc, ct, s, None)

    def refused(text, **kw):
        assert call(**kw) == B, kw
        assert text in L.rf_amd_last_error(), (kw, L.rf_amd_last_error())

    assert call() == 0 and call(f=E.ADVANCE_FIRST) == 0
    refused(b"engine", e=None)
    refused(b"2^56", n=1 << 56)
    refused(b"width", w=0)
    refused(b"flag", f=2)
    refused(b"flag", f=E.ADVANCE_FIRST | 0x100)
    refused(b"count", ct=None)
    refused(b"output records", o=None)
    refused(b"aligned", s=p["scr"] + 4)
    refused(b"key offsets", off=None)
    refused(b"cursors", cu=None)
    refused(b"scratch", s=None)
    refused(b"candidate records", c=None)
    # the order: width before the flags, the flags before the count
    refused(b"width", w=0, f=2, ct=None)
    refused(b"flag", f=2, ct=None)
    # the neighbouring legal calls
    assert call(d=None) == 0 and call(k=None) == 0 and call(o=None, k=None, oc=0) == 0
    assert call(c=None, cc=0) == 0 and call(w=ALL) == 0
    assert call(off=None, c=None, cu=None, s=None, n=0) == 0 and call(n=0, s=p["scr"] + 4) == B
    torch.cuda.synchronize()


# ---- in the world of the multi-get -------------------------------------------------------------
def walk_steps(fset, per_key, cand, want, is_definitive):
    """lookup_steps(width=1) grouped by branch until the count is 0. want: the transcription's
    lookups per key; is_definitive(key, member, value) -> bool arrays. Step s must hold exactly
    lookup s of every key that has one, as records and as the runs' (key, member, value)."""
    steps = fset.lookup_steps(per_key, width=1)
    d_done = torch.zeros(N, dtype=torch.uint8, device="cuda:0")
    finished = set()
    last = max(len(x) for x in want)
    for s in range(last + 1):
        d_out, d_key, count, group = steps.step(d_done)
        expect = sorted((i, int(cand[x[s]]) >> 8, int(cand[x[s]]) & 0xFF) for i, x in enumerate(want) if len(x) > s)
        assert count == len(expect), s
        if count == 0:
            break
        out, key = d_out.cpu().numpy().view(np.uint64), d_key.cpu().numpy()
        ids, values = (out >> np.uint64(8)).astype(np.int64), (out & np.uint64(0xFF)).astype(np.int64)
        assert sorted(zip(key.tolist(), ids.tolist(), values.tolist())) == expect
        d_order, d_okey, d_branch, d_boff, runs = group
        order, okey, boff = d_order.cpu().numpy(), d_okey.cpu().numpy(), d_boff.cpu().numpy()
        branch = d_branch.cpu().numpy().view(np.uint64)
        g = E.found_by_branch_host(out, fset.num_members, key)
        assert runs == len(g[2]) and order.view(np.uint32).tobytes() == g[0].tobytes()
        triples = []
        for u in range(runs):
            b = int(branch[u])
            run_keys = okey[int(boff[u]):int(boff[u + 1])].tolist()
            assert run_keys == sorted(run_keys)  # batch order within a branch
            assert (out[order[int(boff[u]):int(boff[u + 1])]] == branch[u]).all()
            triples += [(k, b >> 8, b & 0xFF) for k in run_keys]
        assert sorted(triples) == expect
        assert not finished & set(key.tolist())  # no key after its definitive record
        hit = key[is_definitive(key, ids, values)]
        finished |= set(hit.tolist())
        d_done[dev(hit)] = 1
    assert count == 0 and s == last
    return s


def test_lookup_steps_end_to_end(world, routed):  # noqa: F811
    """multiget_routed_per_key, then lookup_steps(width=1) grouped by branch, a key being done
    when a record names the filter its key came from: per step the runs hold exactly the (key,
    member, value) of the reference's loop, and no key appears after its own member. A second
    walk, where only B0's older value is definitive, takes the keys through longer lists."""
    w, r = world, routed
    rg, off, member, total = r.host["keys"]
    pairs = RR.want_pairs(r.words["keys"], off, member)
    key_off, cand, cand_key = E.found_per_key_host(pairs, member, off)
    third = N // 3
    own = np.full(N, -1, dtype=np.int64)  # the member a key was added to: A1 and B0
    own[:third], own[third:2 * third] = 1, 3
    rmap = E.RangeMap(*r.table["keys"])
    per_key = w.set.multiget_routed_per_key(rmap, *RR.routed_inputs(w, r, "keys"), N)
    assert per_key[2] == len(cand)

    def own_member(key, ids, values):
        return ids == own[key]

    def older_value_of_b(key, ids, values):  # B0 holds its first 100,000 keys with values 7 and 2
        return (ids == 3) & (values == 2)

    ids, values = (cand >> np.uint64(8)).astype(np.int64), (cand & np.uint64(0xFF)).astype(np.int64)
    for rule in (own_member, older_value_of_b):
        definitive = rule(cand_key, ids, values)
        want = transcription(key_off, len(cand), definitive, 1)
        assert definitive.any() and sum(len(x) for x in want) < len(cand)  # the exit saves lookups
        steps = walk_steps(w.set, per_key, cand, want, rule)
        assert steps >= (1 if rule is own_member else 2)
    # without the grouping, and wider: one step of everything is the per-key list itself
    d_out, d_key, count, group = w.set.lookup_steps(per_key, width=ALL).step(by_branch=False)
    assert group is None and count == len(cand)
    assert d_out.cpu().numpy().view(np.uint64).tobytes() == cand.tobytes()
    assert (d_key.cpu().numpy() == cand_key).all()
    rmap.close()
