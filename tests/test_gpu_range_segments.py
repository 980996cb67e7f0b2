"""Range maps made from segments: rf_amd_range_map_create_segments and
rf_amd_range_map_update_segments (k_range_seg_scatter, k_range_seg_len, k_range_scan,
k_range_seg_emit). The route calls are those of test_gpu_range_route.py, whose helpers build the
boundaries and keys and run a route call between sentinels. The oracle everywhere is
E.range_route_host(bounds, E.range_segment_lists(paths, current lists), keys), compared exactly:
ranges, every offset, every id and the total. The end-to-end test runs in test_gpu_multiget's
world and compares with E.found_candidates of the oracle's routing_filter_lookup words."""
from types import SimpleNamespace

import numpy as np
import pytest

import test_gpu_range_route as RR
from splinterdb_amd import engine as E
from test_gpu_multiget import world  # noqa: F401  (the fixture; a fresh instance for this module)
from test_gpu_range_route import check_route, key_buffers, make_bounds, make_keys, raw_route

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = RR.N  # 64 * 37 + 13
TILE = E.diag_range_tile()
PER = E.diag_range_seg_launch_ids()  # ids of one update launch that holds one list
R_TILES = 3 * TILE + 77              # three whole flatten tiles and a partial one
RS = [1, 2, 65, 1000, R_TILES]
MAX_LIST = 65535

# the placed segments; the leaves follow
ROOT, CAP0, EMPTY, FULL, L63, L64, L65, L300, LOOSE, BIG, LONG, LAST, TA, TB = range(14)
ROOT_CAP = 40
LEAF0, NLEAF, LEAF_CAP = 14, 80, 9
THR = E.diag_range_seg_thread_ids()  # the longest list the flatten expands by one thread


def make_case(seed, R, fixed_len=None):
    """boundaries, N keys, S segments and R paths of 0 to 5 segments. ROOT (2 of 40 ids) is in
    every non-empty path; CAP0 has cap == 0, EMPTY len == 0, FULL len == cap, L63 .. L300 those
    lengths, LOOSE is in no path, BIG makes one path's capacities sum to exactly 65,535 with 4
    ids in it, LONG has room for three update launches and more, LAST is only in the path of the
    last range; with ROOT's 2 ids TA makes a list of exactly THR ids and TB one of THR + 1. With
    R >= 65 the placed paths sit on ranges that keys fall into, and half of the keys are
    boundaries, those of the last ranges among them."""
    rng = np.random.default_rng(seed)
    c = SimpleNamespace(R=R, n=N, fixed_len=fixed_len)
    c.bounds = make_bounds(rng, R, fixed_len)
    assert len(c.bounds) == R - 1
    keys = make_keys(rng, c.bounds, N, fixed_len)
    pool = [b for b in c.bounds if fixed_len is None or len(b) == fixed_len]
    if pool:
        take = pool[-120:] + [pool[i] for i in rng.permutation(len(pool))[:N // 2 - 120]]
        keys[:len(take)] = take
        keys = [keys[i] for i in rng.permutation(N)]
    c.keys = keys
    caps = [ROOT_CAP, 0, 10, 7, 63, 70, 65, 300, 5, MAX_LIST - ROOT_CAP, 3 * PER + 10, LEAF_CAP, THR - 2, THR - 1]
    lens = [2, 0, 0, 7, 63, 64, 65, 300, 3, 4, 5, 6, THR - 2, THR - 1]
    caps += [LEAF_CAP] * NLEAF
    lens += rng.integers(0, LEAF_CAP + 1, size=NLEAF).tolist()
    c.caps = caps
    c.lists = [rng.integers(0, 1000, size=n).tolist() for n in lens]
    c.S = len(caps)
    common = [CAP0, EMPTY, FULL] + list(range(LEAF0, LEAF0 + NLEAF))
    paths = []
    for r in range(R):
        k = int(rng.integers(0, 6))
        paths.append([ROOT] + rng.choice(common, size=k - 1).tolist() if k else [])
    placed = [[ROOT, BIG], [ROOT, FULL, FULL], [ROOT, LONG], [], [ROOT, CAP0, EMPTY, L63, L64],
              [ROOT, L65, L300, LEAF0], [ROOT, L64, L300, L300, L300], [ROOT, TA], [ROOT, TB]]
    rg = E.range_route_host(c.bounds, [[]] * R, keys)[0]
    c.placed = {}
    if R >= 65:
        first = next(int(r) for r in rg if r != R - 1)  # BIG: the range of one of the first keys
        hit = [int(r) for r in np.unique(rg) if r not in (R - 1, first)]
        spots = [first] + rng.choice(hit, size=len(placed) - 1, replace=False).tolist()
    else:
        spots = list(range(R))
    for i, (r, p) in enumerate(zip(spots, placed)):
        paths[r] = p
        c.placed[i] = r
    paths[R - 1] = [ROOT, LAST] if R > 2 else paths[R - 1]
    c.paths = paths
    c.max_list = max(sum(caps[s] for s in p) for p in paths)
    assert c.max_list <= MAX_LIST
    return c


def oracle_of(c, lists, n=None):
    """the case with the host mirror's answer for the segments' lists `lists` (first n keys)"""
    o = SimpleNamespace(**vars(c))
    if n is not None:
        o.n, o.keys = n, c.keys[:n]
    o.flat = E.range_segment_lists(c.paths, lists)
    o.rg, o.off, o.member, o.total = E.range_route_host(c.bounds, o.flat, o.keys)
    return o


def new_map(c, lists=None):
    return E.RangeMap.from_segments(c.bounds, c.paths, c.lists if lists is None else lists, c.caps)


@pytest.fixture(scope="module")
def cases():
    """the cases by (R, fixed_len), made once and read-only, with the oracle of the initial lists"""
    cache = {}

    def get(R, fixed_len=None):
        key = (R, fixed_len)
        if key not in cache:
            c = make_case(31 * R + (fixed_len or 0), R, fixed_len)
            cache[key] = (c, oracle_of(c, c.lists))
        return cache[key]
    return get


def route(m, o, args=None, **kw):
    return raw_route(m, o, key_buffers(o) if args is None else args, **kw)


# ---- the cases say what they claim -----------------------------------------------------------
@pytest.mark.parametrize("R", [1000, R_TILES])
def test_placed_cases_exist(cases, R):
    c, o = cases(R)
    assert R_TILES > 3 * TILE and R_TILES % TILE and N == 64 * 37 + 13 and c.n == N
    lens = [len(x) for x in c.lists]
    assert {len(p) for p in c.paths} == set(range(6))
    assert all(p[0] == ROOT for p in c.paths if p) and sum(1 for p in c.paths if not p) > 10
    used = {s for p in c.paths for s in p}
    assert LOOSE not in used and used >= set(range(c.S)) - {LOOSE}
    assert any(len(set(p)) < len(p) for p in c.paths), "a segment twice in one path"
    assert c.caps[CAP0] == 0 and lens[EMPTY] == 0 < c.caps[EMPTY] and lens[FULL] == c.caps[FULL] > 0
    assert [lens[s] for s in (L63, L64, L65, L300)] == [63, 64, 65, 300]
    assert lens[ROOT] == 2 < c.caps[ROOT]
    big = c.paths[c.placed[0]]
    assert big == [ROOT, BIG] and sum(c.caps[s] for s in big) == MAX_LIST == c.max_list and lens[BIG] == 4
    assert c.caps[LONG] > 3 * PER
    assert sum(1 for p in c.paths if LAST in p) == 1 and LAST in c.paths[R - 1]
    # the placed ranges and the last one are among the keys' ranges; most ranges of R = 1000 are
    hit = set(o.rg.tolist())
    assert set(c.placed.values()) <= hit and R - 1 in hit
    assert R != 1000 or len(hit) > 900
    if R == R_TILES:
        assert sum(1 for r in hit if r >= 3 * TILE) > 50, "keys in the partial last tile"
        assert all(any(t * TILE <= r < (t + 1) * TILE for r in hit) for t in range(4))
    cnt = np.diff(o.off.astype(np.int64))
    assert {0, 2, 2 + 4, 2 + 14, THR, THR + 1}.issubset(cnt.tolist()) and cnt.max() >= 2 + 64 + 900
    # most lists are a thread's, the placed long ones a wave's; with the root grown to its 40 ids
    # (test_update_sequence) every list is a wave's
    assert (cnt[cnt > 0] <= THR).mean() > 0.5 and len(set(cnt[cnt > THR].tolist())) >= 4 and ROOT_CAP > THR
    assert o.total < 200000, "the route outputs stay small"


# ---- create ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed_len", [None, 24], ids=["var", "keys24"])
@pytest.mark.parametrize("R", RS)
def test_create_equals_flat_map(cases, R, fixed_len):
    """the route output's bytes equal those of a flat map made from the flattened lists"""
    c, o = cases(R, fixed_len)
    m, flat = new_map(c), E.RangeMap(c.bounds, o.flat)
    assert m.num_ranges == flat.num_ranges == R and m.num_segments == c.S and flat.num_segments == 0
    assert m.max_list == c.max_list and flat.max_list == max(len(x) for x in o.flat)
    args = key_buffers(o)
    a = route(m, o, args, pair_cap=o.total + 100)
    b = route(flat, o, args, pair_cap=o.total + 100)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    assert a[3] == b[3]
    check_route(a, o, (R, fixed_len), cap=o.total + 100)
    m.close()
    flat.close()


def test_create_refusals_and_edges():
    def einval(fn):
        with pytest.raises(E.PlatformStatusError) as ei:
            fn()
        assert ei.value.code == E.STATUS_BAD_PARAM

    F = E.RangeMap.from_segments
    einval(lambda: F([b"b", b"a"], [[0], [0], [0]], [[1]]))
    einval(lambda: F([b"a"], [[0], [1]], [[1]]))                      # a path entry >= num_segments
    einval(lambda: F([b"a"], [[0], [0]], [[1, 2]], [1]))              # a list longer than its capacity
    einval(lambda: F([b"a"], [[0, 1], [0]], [[], []], [65535, 1]))    # capacities over the limit
    einval(lambda: F([b"a"], [[0, 0], [0]], [[]], [32768]))
    m = F([b"a"], [[0, 1], [0]], [[], []], [65535, 0])
    assert m.max_list == 65535 and m.num_segments == 2
    m.close()
    m = F([b"a"], [[], []], [])                                       # no segments at all
    assert m.num_segments == 0 and m.max_list == 0
    m.update_segments([], [])
    einval(lambda: m.update_segments([0], [[]]))
    m.close()


# ---- updates ---------------------------------------------------------------------------------
def apply(m, lists, ids, new, stream=None):
    """the update on the map and on the model (in the call's order: the last entry wins)"""
    m.update_segments(ids, new, stream=stream)
    for s, x in zip(ids, new):
        lists[s] = list(x)


@pytest.mark.parametrize("R,fixed_len", [(1, None), (2, None), (65, 24), (1000, None), (R_TILES, None),
                                         (R_TILES, 24)])
def test_update_sequence(cases, R, fixed_len):
    c, o = cases(R, fixed_len)
    rng = np.random.default_rng(R)
    m = new_map(c)
    lists = [list(x) for x in c.lists]
    args = key_buffers(o)
    ids_of = lambda n: rng.integers(0, 1000, size=n).tolist()  # noqa: E731

    def check(what):
        now = oracle_of(c, lists)
        check_route(route(m, now, args, pair_cap=now.total + 64), now, (R, what), cap=now.total + 64)
        return now

    check("created")
    apply(m, lists, [ROOT], [ids_of(ROOT_CAP)])        # every later range's loff shifts
    grown = check("root grown to its capacity")
    assert R < 65 or grown.total > o.total + 30 * 1000
    apply(m, lists, [ROOT], [[]])
    check("root shrunk to nothing")
    apply(m, lists, [LAST], [ids_of(LEAF_CAP)])        # a leaf of the last range alone
    check("leaf of the last tile")
    leaves = (LEAF0 + rng.permutation(NLEAF)[:70]).tolist()
    apply(m, lists, leaves, [ids_of(int(rng.integers(0, LEAF_CAP + 1))) for _ in leaves])
    check("70 segments in one call")
    apply(m, lists, [LONG], [ids_of(PER + 1)])         # two pieces over two launches
    check("one id over a launch")
    apply(m, lists, [EMPTY, LONG, ROOT], [ids_of(3), ids_of(3 * PER), ids_of(5)])
    check("three launches' worth behind another list")
    apply(m, lists, [EMPTY, FULL, EMPTY, ROOT, EMPTY], [ids_of(9), ids_of(2), [], ids_of(1), ids_of(10)])
    assert len(lists[EMPTY]) == 10
    check("a repeated id: the last entry wins")
    apply(m, lists, [LOOSE, CAP0], [ids_of(5), []])    # a segment in no path, and one without room
    same = check("segments that change no list")
    assert same.total == oracle_of(c, lists).total
    assert m.max_list == c.max_list
    m.close()


def test_stream_order_without_a_host_wait(cases):
    """route A, update, route B on one stream, one synchronisation: A is the old table's, B the
    new one's"""
    c, o = cases(R_TILES, 24)
    m = new_map(c)
    lists = [list(x) for x in c.lists]
    lists[ROOT] = list(range(100, 100 + ROOT_CAP))
    lists[LAST] = []
    lists[L64] = [5] * 70
    new = oracle_of(c, lists)
    s = torch.cuda.Stream()
    h = s.cuda_stream
    d_keys, key_len = key_buffers(o)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        a = m.route_keys(d_keys, key_len, c.n, pair_cap=o.total, stream=h)
        m.update_segments([ROOT, LAST, L64], [lists[ROOT], lists[LAST], lists[L64]], stream=h)
        b = m.route_keys(d_keys, key_len, c.n, pair_cap=new.total, stream=h)
    s.synchronize()
    for got, want, what in ((a, o, "before the update"), (b, new, "after the update")):
        d_range, d_off, d_member, d_total = got
        check_route((d_range.cpu().numpy().view(np.uint32), d_off.cpu().numpy().view(np.uint64),
                     d_member.cpu().numpy().view(np.uint32), int(d_total.item())), want, what)
    assert new.total != o.total and not np.array_equal(new.off, o.off)
    m.close_on(h)
    s.synchronize()


def test_max_list_is_the_path_capacity_bound(cases):
    """max_list does not move with the lists, and with pair_cap = n * max_list nothing overflows
    once every segment is full (the first 96 keys: one of them in the 65,535-id range)"""
    c, o = cases(1000)
    n = 96
    m = new_map(c)
    assert m.max_list == c.max_list == MAX_LIST > max(len(x) for x in o.flat)
    rng = np.random.default_rng(5)
    lists = [rng.integers(0, 1000, size=cap).tolist() for cap in c.caps]
    m.update_segments(list(range(c.S)), lists)
    assert m.max_list == MAX_LIST
    full = oracle_of(c, lists, n=n)
    cnt = np.diff(full.off.astype(np.int64))
    assert cnt.max() == MAX_LIST and full.total <= n * m.max_list
    check_route(route(m, full, pair_cap=n * m.max_list), full, "every segment full", cap=n * m.max_list)
    m.update_segments(list(range(c.S)), [[] for _ in range(c.S)])
    none = oracle_of(c, [[] for _ in range(c.S)], n=n)
    assert none.total == 0 and m.max_list == MAX_LIST
    check_route(route(m, none, pair_cap=64), none, "every segment empty", cap=64)
    m.close()


def test_update_errors_change_nothing(cases):
    c, o = cases(1000)
    m = new_map(c)
    L = E.load_library()
    B = E.STATUS_BAD_PARAM
    u32 = lambda x: np.array(x, dtype=np.uint32)  # noqa: E731
    u64 = lambda x: np.array(x, dtype=np.uint64)  # noqa: E731
    seg, ids, off = u32([ROOT, EMPTY]), u32(list(range(20))), u64([0, 5, 9])

    def upd(h=m.h, s=seg.ctypes.data, i=ids.ctypes.data, f=off.ctypes.data, count=2):
        return L.rf_amd_range_map_update_segments(h, s, i, f, count, None)

    assert upd(h=None) == B and b"null range map" in L.rf_amd_last_error()
    assert upd(s=None) == B and upd(f=None) == B and upd(i=None) == B
    bad = u32([ROOT, c.S])
    assert upd(s=bad.ctypes.data) == B and b"num_segments" in L.rf_amd_last_error()
    last_bad = u32([ROOT, EMPTY, 0xFFFFFFFF])       # the entries before a bad one are not applied
    assert upd(s=last_bad.ctypes.data, f=u64([0, 5, 9, 9]).ctypes.data, count=3) == B
    long_ = u64([0, 5, 5 + c.caps[EMPTY] + 1])      # one id over the segment's capacity
    assert upd(f=long_.ctypes.data) == B and b"capacity" in L.rf_amd_last_error()
    nocap = u32([ROOT, CAP0])
    assert upd(s=nocap.ctypes.data) == B
    dec = u64([5, 9, 8])
    assert upd(f=dec.ctypes.data) == B and b"decrease" in L.rf_amd_last_error()
    assert upd(count=0) == 0 and upd(s=None, i=None, f=None, count=0) == 0
    flat = E.RangeMap(c.bounds[:1], [[1], [2]])
    assert flat.num_segments == 0
    assert upd(h=flat.h) == B and b"flat" in L.rf_amd_last_error()
    assert upd(h=flat.h, count=0) == B
    with pytest.raises(E.PlatformStatusError):
        flat.update_segments([0], [[1]])
    flat.close()
    check_route(route(m, o), o, "after the refused updates")
    assert upd() == 0  # and the same arrays are a legal call
    lists = [list(x) for x in c.lists]
    lists[ROOT], lists[EMPTY] = list(range(5)), list(range(5, 9))
    now = oracle_of(c, lists)
    check_route(route(m, now), now, "after the legal update")
    m.close()


@pytest.mark.parametrize("blocks", [1, 2])
def test_grid_stride_loops(cases, blocks):
    """four flatten tiles and three route tiles on one and two workgroups"""
    c, o = cases(R_TILES)
    m = new_map(c)
    lists = [list(x) for x in c.lists]
    try:
        E.diag_fanout_max_blocks(blocks)
        apply(m, lists, [ROOT, LAST, LONG], [list(range(ROOT_CAP)), [8, 9], list(range(PER + 7))])
        now = oracle_of(c, lists)
        check_route(route(m, now), now, ("capped", blocks))
    finally:
        E.diag_fanout_max_blocks(0)
    apply(m, lists, [ROOT], [[3]])
    now = oracle_of(c, lists)
    check_route(route(m, now), now, ("cap lifted", blocks))
    m.close()


def test_two_maps_give_identical_bytes(cases):
    c, o = cases(R_TILES)
    args = key_buffers(o)
    rng = np.random.default_rng(8)
    steps = [([ROOT, LEAF0 + 3], [rng.integers(0, 99, size=31).tolist(), [1, 2, 3]]),
             ([LONG, ROOT, LAST], [rng.integers(0, 99, size=2 * PER + 3).tolist(), [4], []]),
             ([EMPTY, EMPTY], [[1], [2, 3]])]
    outs = []
    for _ in range(2):
        m = new_map(c)
        lists = [list(x) for x in c.lists]
        for ids, new in steps:
            apply(m, lists, ids, new)
        now = oracle_of(c, lists)
        outs.append(route(m, now, args, pair_cap=now.total + 100))
        check_route(outs[-1], now, "the sequence", cap=now.total + 100)
        m.close()
    for x, y in zip(outs[0][:3], outs[1][:3]):
        assert x.tobytes() == y.tobytes()
    assert outs[0][3] == outs[1][3]


# ---- in the world of the multi-get -----------------------------------------------------------
def test_multiget_routed_follows_an_update(world):  # noqa: F811
    """a set with room and a segmented map over its member ids; then, on one stream, a member
    update of the set and the update of the segments that name the changed slots"""
    w = world
    rng = np.random.default_rng(99)
    n = RR.N
    pk = np.ascontiguousarray(w.pk).reshape(n, -1).view(np.uint8).reshape(n, 24)
    keys = [bytes(pk[i]) for i in range(n)]
    bounds = sorted({keys[i] for i in rng.choice(n, size=30, replace=False)})
    R = len(bounds) + 1
    # slot -> the world's member whose filter sits there (None: no filter); slots 6 and 7 are room
    slot = [0, 1, None, 3, 4, 5, None, None]
    fs = E.FilterSet(w.members, capacity=8)
    seg_lists = [[0, 3], [1], [2, 5], [4], [7, 1]]  # 0: the root's; ids of empty slots among them
    caps = [4, 3, 4, 2, 2]
    paths = [[0] + rng.choice([1, 2, 3, 4], size=int(rng.integers(0, 3)), replace=False).tolist() for _ in range(R)]
    paths[2] = []
    rmap = E.RangeMap.from_segments(bounds, paths, seg_lists, caps)
    d_keys = RR.dev(w.pk)

    def want_of(seg_lists):
        rg, off, member, total = E.range_route_host(bounds, E.range_segment_lists(paths, seg_lists), keys)
        key = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
        src = np.array([-1 if slot[i] is None else slot[i] for i in member], dtype=np.int64)
        words = np.where(src >= 0, w.words["keys"][np.maximum(src, 0), key], np.uint64(0))
        cand = E.found_candidates(words)
        return cand, E.ragged_pair_keys(off, cand >> np.uint64(8))

    def check(seg_lists, stream=None):
        want, want_key = want_of(seg_lists)
        assert len(want) > 100
        d_cand, count, d_key = fs.multiget_routed(rmap, d_keys, 24, n, stream=stream)
        assert count == len(want)
        assert (d_cand[:count].cpu().numpy().view(np.uint64) == want).all()
        assert (d_key.cpu().numpy() == want_key).all()
        return want

    before = check(seg_lists)
    s = torch.cuda.Stream()
    h = s.cuda_stream
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        # a compaction's outcome: C's filter moves from slot 4 to slot 6, D's filter fills slot 2
        fs.update([6, 4, 2], [w.members[4], None, w.members[5]], stream=h)
        slot[6], slot[4], slot[2] = 4, None, 5
        seg_lists[3] = [6]
        seg_lists[0] = [0, 3, 2, 6]
        rmap.update_segments([3, 0], [seg_lists[3], seg_lists[0]], stream=h)
        after = check(seg_lists, stream=h)
    assert not np.array_equal(after, before)
    rmap.close_on(h)
    assert rmap.h is None
    fs.close_on(h)
    s.synchronize()
