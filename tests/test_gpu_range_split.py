"""Range maps that follow node splits: rf_amd_range_map_create_segments_room,
rf_amd_range_map_split and rf_amd_range_map_set_paths (k_range_splice, then the flatten of
test_gpu_range_segments.py). Every test keeps the Python model of the map -- its boundaries, paths
and segment lists, edited by E.range_split_host / E.range_set_paths_host -- beside the map, and
the oracle everywhere is E.range_route_host(bounds, E.range_segment_lists(paths, lists), keys),
compared exactly: ranges, every offset, every id and the total, with the route call's buffers
between sentinels (test_gpu_range_route's raw_route). Half of the keys of every check are
boundaries of the current table, the newest ones among them. The end-to-end test runs in
test_gpu_multiget's world and compares with E.found_candidates of the oracle's
routing_filter_lookup words."""
import bisect
from types import SimpleNamespace

import numpy as np
import pytest

import test_gpu_range_route as RR
from splinterdb_amd import engine as E
from test_gpu_multiget import world  # noqa: F401  (the fixture; a fresh instance for this module)
from test_gpu_range_route import check_route, key_buffers, make_bounds, make_keys, rand_bytes, raw_route

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = RR.N  # 64 * 37 + 13
TILE = E.diag_range_tile()
LDS_R = E.diag_range_lds_ranges()
W = E.diag_range_splice_words()  # the words of new elements one splice launch carries
NO_SPACE, BAD = E.STATUS_NO_SPACE, E.STATUS_BAD_PARAM

# the segments: ROOT is in most paths, NEWROOT and the SPAREs start in none, ZERO has no room
ROOT, NEWROOT, ZERO, SPARE0, SPARE1, LEAF0 = 0, 1, 2, 3, 4, 5
NLEAF = 40
CAPS = [6, 4, 0, 5, 5] + [j % 4 for j in range(NLEAF)]
S = len(CAPS)
BIG = dict(ranges=LDS_R + 200, bound_bytes=1 << 18, path_entries=1 << 16, list_ids=1 << 20, max_list=400)


def seg_lists(rng):
    lists = [rng.integers(0, 1000, size=int(rng.integers(0, c + 1))).tolist() for c in CAPS]
    lists[ROOT], lists[NEWROOT], lists[SPARE0], lists[SPARE1] = [11, 12], [], [], []
    return lists


def rand_path(rng, most=4):
    k = int(rng.integers(0, most + 1))
    return [ROOT] + (LEAF0 + rng.integers(0, NLEAF, size=k - 1)).tolist() if k else []


class Live:
    """a map with room and the Python model of it, edited together"""

    def __init__(self, rng, bounds, paths=None, room=None, lists=None, caps=None):
        self.rng = rng
        self.bounds = [bytes(b) for b in bounds]
        self.paths = [rand_path(rng) for _ in range(len(bounds) + 1)] if paths is None else [list(p) for p in paths]
        self.lists = seg_lists(rng) if lists is None else [list(x) for x in lists]
        self.caps = CAPS if caps is None else caps
        self.map = E.RangeMap.from_segments(self.bounds, self.paths, self.lists, self.caps, room=room or BIG)
        assert self.map.num_ranges == len(self.paths)

    def split(self, r, new_bounds, new_paths, stream=None):
        self.map.split(r, new_bounds, new_paths, stream=stream)
        self.bounds, self.paths = E.range_split_host(self.bounds, self.paths, r, new_bounds, new_paths)
        assert self.map.num_ranges == len(self.paths) == len(self.bounds) + 1
        assert self.bounds == sorted(self.bounds) and len(set(self.bounds)) == len(self.bounds)

    def set_paths(self, first, new_paths, stream=None):
        self.map.set_paths(first, new_paths, stream=stream)
        self.paths = E.range_set_paths_host(self.paths, first, new_paths)
        assert self.map.num_ranges == len(self.paths)

    def update(self, ids, new, stream=None):
        self.map.update_segments(ids, new, stream=stream)
        for s, x in zip(ids, new):
            self.lists[s] = list(x)

    def keys(self, newest=(), fixed_len=None):
        """N keys, half of them boundaries of the current table, the newest ones first"""
        keys = make_keys(self.rng, self.bounds, N, fixed_len)
        fits = lambda b: fixed_len is None or len(b) == fixed_len  # noqa: E731
        pool = [b for b in self.bounds if fits(b)]
        if pool:
            take = [b for b in newest if fits(b)][:N // 4]
            take += [pool[i] for i in self.rng.integers(0, len(pool), size=N // 2 - len(take))]
            keys[:len(take)] = take
            keys = [keys[i] for i in self.rng.permutation(N)]
        return keys

    def oracle(self, keys, fixed_len=None):
        o = SimpleNamespace(n=len(keys), keys=keys, fixed_len=fixed_len, R=len(self.paths), bounds=self.bounds)
        o.flat = E.range_segment_lists(self.paths, self.lists)
        o.rg, o.off, o.member, o.total = E.range_route_host(self.bounds, o.flat, keys)
        return o

    def check(self, what, newest=(), fixed_len=None, stream=None):
        o = self.oracle(self.keys(newest, fixed_len), fixed_len)
        got = raw_route(self.map, o, key_buffers(o), pair_cap=o.total + 64, stream=stream)
        check_route(got, o, what, cap=o.total + 64)
        return o

    def range_between(self, lo, hi):
        """the range whose boundaries are lo and hi"""
        r = bisect.bisect_right(self.bounds, lo)
        assert self.bounds[r - 1] == lo and self.bounds[r] == hi
        return r

    def lo_hi(self, r):
        return (self.bounds[r - 1] if r else None), (self.bounds[r] if r < len(self.bounds) else None)


def inside(rng, lo, hi, count, most=4):
    """count keys strictly between lo (None: no lower boundary) and hi (None: no upper), sorted;
    None where the range is too narrow for the tries made"""
    out = set()
    for _ in range(40 * count + 40):
        if len(out) == count:
            return sorted(out)
        k = (lo or b"") + rand_bytes(rng, int(rng.integers(1, most + 1)))
        if (lo is None or k > lo) and (hi is None or k < hi):
            out.add(k)
    return sorted(out) if len(out) == count else None


def roomy_range(live, count, lo_r=1, hi_r=None, most=4):
    """a range in [lo_r, hi_r) wide enough for `count` new boundaries, and those boundaries"""
    hi_r = len(live.paths) - 1 if hi_r is None else hi_r
    for r in live.rng.permutation(np.arange(lo_r, hi_r)):
        nb = inside(live.rng, *live.lo_hi(int(r)), count, most)
        if nb is not None:
            return int(r), nb
    raise AssertionError("no range wide enough")


def raises(code, fn):
    with pytest.raises(E.PlatformStatusError) as ei:
        fn()
    assert ei.value.code == code, ei.value
    return str(ei.value)


# ---- growth and position ---------------------------------------------------------------------
def test_first_boundaries_of_a_map_of_one_range():
    rng = np.random.default_rng(1)
    live = Live(rng, [], paths=[[ROOT, LEAF0 + 3]])  # created with NULL boundary arrays
    assert live.map.num_ranges == 1 and live.map.max_list == BIG["max_list"]
    live.check("one range")
    first = b"\x61\x7f"
    live.split(0, [first], [[ROOT, LEAF0 + 3], [ROOT, LEAF0 + 5, LEAF0 + 6]])  # R from 1 to 2
    assert live.map.num_ranges == 2
    live.check("the first boundary", newest=[first])
    live.split(0, [b""], [[], [ROOT, LEAF0 + 3]])  # the zero-length key: range 0 is empty from here on
    o = live.check("a zero-length first boundary", newest=[b""])
    assert live.bounds == [b"", first] and (o.rg > 0).all() and b"" in o.keys
    live.split(1, [], [[ROOT, LEAF0 + 9, LEAF0 + 9]])  # pieces == 1: the path alone
    live.split(2, [], [[]])
    assert live.map.num_ranges == 3
    live.check("pieces == 1")
    raises(BAD, lambda: live.map.split(0, [b"\x00"], [[], []]))  # nothing lies below the empty key
    live.map.close()


@pytest.mark.parametrize("fixed_len", [None, 24], ids=["var", "keys24"])
def test_split_first_last_and_middle(fixed_len):
    rng = np.random.default_rng(2)
    live = Live(rng, make_bounds(rng, 65, fixed_len))
    live.check("created", fixed_len=fixed_len)
    hi = live.bounds[0]
    nb = sorted({hi[:k] for k in range(max(0, len(hi) - 2), len(hi))})  # proper prefixes lie below
    live.split(0, nb, [rand_path(rng) for _ in range(len(nb) + 1)])
    live.check("range 0", newest=nb, fixed_len=fixed_len)
    last = len(live.paths) - 1
    nb = sorted(set(inside(rng, live.bounds[-1], None, 3) + [b"\xff" * 30]))
    live.split(last, nb, [rand_path(rng) for _ in range(len(nb) + 1)])
    live.check("the last range", newest=nb, fixed_len=fixed_len)
    r, nb = roomy_range(live, 2, lo_r=20, hi_r=40)
    if fixed_len:  # a new boundary of the keys' length, so that keys equal it
        lo = live.bounds[r - 1]
        wide = [b for b in [(lo + rand_bytes(rng, 24))[:24]] if lo < b < live.bounds[r]]
        nb = sorted(set(nb + wide))
    live.split(r, nb, [rand_path(rng) for _ in range(len(nb) + 1)])
    o = live.check("a middle range", newest=nb, fixed_len=fixed_len)
    assert len(live.paths) >= 65 + 4 + 2 and (fixed_len or set(range(r, r + 3)) & set(o.rg.tolist()))
    live.map.close()


# ---- boundary content ------------------------------------------------------------------------
def test_new_boundary_lengths_and_tie_runs():
    rng = np.random.default_rng(3)
    live = Live(rng, [])
    nb = [b"\x20", b"\x30" * 7, b"\x40" * 8, b"\x50" * 9, b"\x60" * 105]
    assert [len(b) for b in nb] == [1, 7, 8, 9, 105]
    live.split(0, nb, [rand_path(rng) or [ROOT] for _ in range(6)])
    o = live.check("boundaries of 1, 7, 8, 9 and 105 bytes", newest=nb)
    assert set(o.rg.tolist()) == set(range(6))
    # new boundaries that share their 8-byte prefix with both neighbours
    T = b"\x45" * 8
    ends = [T + b"\x10", T + b"\x90"]
    live.split(live.range_between(nb[2], nb[3]), ends, [[ROOT, LEAF0 + j] for j in range(3)])
    live.check("the ends of a tie run", newest=ends)
    tie = [T + b"\x20", T + b"\x20\x00", T + b"\x61", T + b"\x61" * 20, T + b"\x80"]
    r = live.range_between(*ends)
    live.split(r, tie, [[ROOT, LEAF0 + 10 + j] for j in range(6)])
    run = ends[:1] + tie + ends[1:]
    assert live.bounds[r - 1:r + 6] == run and len({b[:8] for b in run}) == 1
    near = [b + x for b in run for x in (b"", b"\x00", b"\xff")] + [b[:-1] for b in run] + [T, T[:7]]
    o = live.check("inside a tie run", newest=near)
    assert set(range(r - 1, r + 7)) <= set(o.rg.tolist())
    live.map.close()


# ---- threshold crossings ---------------------------------------------------------------------
@pytest.mark.parametrize("R0,edge", [(TILE - 1, TILE), (LDS_R - 1, LDS_R)], ids=["flatten-tile", "lds-prefixes"])
def test_split_across_a_threshold(R0, edge):
    """one split takes R from one below the edge to one above it: a second flatten tile, and the
    route kernel's other prefix search"""
    rng = np.random.default_rng(R0)
    live = Live(rng, make_bounds(rng, R0))
    assert live.map.num_ranges == R0 == edge - 1
    o = live.check("one below")
    assert len(set(o.rg.tolist())) > 500
    r, nb = roomy_range(live, 2, lo_r=R0 // 2)
    live.split(r, nb, [[ROOT, LEAF0], [ROOT, LEAF0 + 1, LEAF0 + 2], [ROOT]])
    assert live.map.num_ranges == edge + 1
    o = live.check("one above", newest=nb + live.bounds[r - 1:r] + live.bounds[-3:])
    assert (o.rg >= edge - 1).any() and {r, r + 1, r + 2} <= set(o.rg.tolist())
    live.update([ROOT], [[1, 2, 3, 4, 5]])  # the flatten alone, at the new R
    live.check("an update above the edge")
    live.map.close()


def test_three_splice_launches():
    rng = np.random.default_rng(5)
    live = Live(rng, make_bounds(rng, 65))
    r, nb = roomy_range(live, 59, most=5)
    new_paths = [[ROOT] + (LEAF0 + rng.integers(0, NLEAF, size=29)).tolist() for _ in range(60)]
    words = E.range_splice_words(nb, new_paths)
    assert 2 * W < words < 3 * W and words % W > 8, "three launches, the last one partly filled"
    assert max(sum(CAPS[s] for s in p) for p in new_paths) <= BIG["max_list"]
    live.split(r, nb, new_paths)
    o = live.check("three launches", newest=nb)
    assert len(set(range(r, r + 60)) & set(o.rg.tolist())) > 50
    first = r + 3
    long_paths = [[ROOT] + [LEAF0 + 4 * j for j in range(10)] * 9 for _ in range(25)] + [[], [ROOT]]
    assert E.range_splice_words([], long_paths) > 2 * W
    live.set_paths(first, long_paths)
    live.check("set_paths of three launches", newest=nb)
    live.map.close()


# ---- sequencing ------------------------------------------------------------------------------
def test_edits_back_to_back_on_one_stream():
    """three splits with nothing between them (the structural copies come round to the first
    again) and a checked route; then splits interleaved with update_segments, a spare segment
    being filled and named by the next split, with nothing between them either"""
    rng = np.random.default_rng(6)
    live = Live(rng, make_bounds(rng, 65))
    s = torch.cuda.Stream()
    h = s.cuda_stream
    torch.cuda.synchronize()
    newest = []
    with torch.cuda.stream(s):
        for count in (3, 1, 2):
            r, nb = roomy_range(live, count)
            live.split(r, nb, [rand_path(rng) for _ in range(count + 1)], stream=h)
            newest += nb
        live.check("three splits", newest=newest, stream=h)
        # a leaf split as the caller runs it: the spare segments receive the new leaves' ids
        r, nb = roomy_range(live, 1)
        old = live.paths[r]
        live.update([SPARE0, SPARE1], [[2901, 2902, 2903], [2904]], stream=h)
        live.split(r, nb, [old + [SPARE0], old + [SPARE1]], stream=h)
        live.update([ROOT], [[7, 8, 9, 10, 11, 12]], stream=h)
        r2, nb2 = roomy_range(live, 2)
        live.split(r2, nb2, [[SPARE1], [], [ROOT, SPARE0, SPARE0]], stream=h)
        live.update([SPARE0], [[2905]], stream=h)
        o = live.check("splits between updates", newest=nb + nb2, stream=h)
    assert 2905 in o.member.tolist() and 2904 in o.member.tolist() and 2901 not in o.member.tolist()
    live.map.close_on(h)
    s.synchronize()


def test_stream_order_without_a_host_wait():
    """route A, split, route B on one stream, one synchronisation: A is the old table's with the
    old range numbers, B the new one's"""
    rng = np.random.default_rng(7)
    live = Live(rng, make_bounds(rng, TILE - 1, 24))
    r, nb = roomy_range(live, 4, lo_r=5, hi_r=200)
    new_paths = [[ROOT, LEAF0 + j, LEAF0 + 1] for j in range(5)]
    model = SimpleNamespace(bounds=live.bounds, paths=live.paths)
    model.bounds, model.paths = E.range_split_host(live.bounds, live.paths, r, nb, new_paths)
    keys = live.keys(newest=[b for b in model.bounds[r:r + 200] if len(b) == 24], fixed_len=24)
    old = live.oracle(keys, 24)
    s = torch.cuda.Stream()
    h = s.cuda_stream
    d_keys, key_len = key_buffers(old)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        a = live.map.route_keys(d_keys, key_len, N, pair_cap=old.total, stream=h)
        live.split(r, nb, new_paths, stream=h)
        new = live.oracle(keys, 24)
        b = live.map.route_keys(d_keys, key_len, N, pair_cap=new.total, stream=h)
    s.synchronize()
    for got, want, what in ((a, old, "before the split"), (b, new, "after the split")):
        d_range, d_off, d_member, d_total = got
        check_route((d_range.cpu().numpy().view(np.uint32), d_off.cpu().numpy().view(np.uint64),
                     d_member.cpu().numpy().view(np.uint32), int(d_total.item())), want, what)
    assert (new.rg != old.rg).sum() > 100 and live.map.num_ranges == TILE + 3
    live.map.close_on(h)
    s.synchronize()


# ---- set_paths -------------------------------------------------------------------------------
def test_set_paths_across_a_tile_edge_and_a_new_root():
    rng = np.random.default_rng(8)
    R = TILE + 40
    live = Live(rng, make_bounds(rng, R))
    first = TILE - 10
    grown = [p + [LEAF0 + 7, LEAF0 + 7, LEAF0 + 11] for p in live.paths[first:first + 7]]
    shrunk = [p[:1] for p in live.paths[first + 7:first + 14]]
    new_paths = grown + shrunk + [[] for _ in range(6)]
    live.set_paths(first, new_paths)
    o = live.check("an index split's run", newest=live.bounds[first - 2:first + 21])
    assert len(set(range(first, first + 20)) & set(o.rg.tolist())) == 20
    live.update([NEWROOT], [[2801, 2802, 2803]])
    live.set_paths(0, [[NEWROOT] + p for p in live.paths])  # a new root level: every range
    o = live.check("a new root level")
    assert (np.diff(o.off.astype(np.int64)) >= 3).all() and live.map.num_ranges == R
    live.set_paths(R - 1, [[]])
    live.set_paths(0, [])  # count == 0: nothing
    live.check("the last range alone")
    live.map.close()


# ---- room ------------------------------------------------------------------------------------
SMALL_CAPS = [4, 1, 2, 5, 0]


def small_live(rng, room):
    """4 ranges, 4 boundary bytes, 5 path entries, 15 list ids, largest path capacity 6"""
    return Live(rng, [b"b", b"d", b"dd"], paths=[[0, 1], [0, 2], [0], []], room=room,
                lists=[[1, 2], [3], [], [9], []], caps=SMALL_CAPS)


def route_bytes(live, o, args):
    got = raw_route(live.map, o, args, pair_cap=o.total + 64)
    return [x.tobytes() for x in got[:3]] + [got[3]]


FILL = (1, [b"c", b"cc"], [[0], [0, 3], [0, 2]])  # to 6 ranges, 7 bytes, 8 entries, 28 ids, capacity 9
ONE_PAST = {
    "ranges": lambda m: m.split(5, [b"e"], [[], []]),
    "bound_bytes": lambda m: m.split(5, [b"e"], [[], []]),
    "path_entries": lambda m: m.set_paths(5, [[4]]),
    "list_ids": lambda m: m.set_paths(5, [[1]]),
}


@pytest.mark.parametrize("field", list(ONE_PAST))
def test_room_filled_exactly_then_one_past(field):
    rng = np.random.default_rng(9)
    full = dict(ranges=6, bound_bytes=7, path_entries=8, list_ids=28, max_list=9)
    room = dict(ranges=100, bound_bytes=100, path_entries=100, list_ids=1000, max_list=9)
    room[field] = full[field]
    live = small_live(rng, room)
    live.check("created")
    live.split(*FILL)  # exactly full in `field`
    o = live.check("exactly full", newest=FILL[1])
    args = key_buffers(o)
    before = route_bytes(live, o, args)
    msg = raises(NO_SPACE, lambda: ONE_PAST[field](live.map))
    assert "room." + field in msg
    assert live.map.num_ranges == 6
    assert route_bytes(live, o, args) == before
    live.split(2, [], [[0, 3]])  # a full map still takes an edit that does not grow it
    live.set_paths(0, [[1, 0]])
    live.check("after the refusal")
    live.map.close()


def test_create_with_room_refusals():
    rng = np.random.default_rng(10)
    used = dict(ranges=4, bound_bytes=4, path_entries=5, list_ids=15, max_list=6)
    live = small_live(rng, used)  # a room that is exactly the table
    assert live.map.max_list == 6
    live.check("no room to spare")
    raises(NO_SPACE, lambda: live.map.split(1, [b"c"], [[0], [0]]))
    live.set_paths(1, [[2, 0]])
    live.check("an edit of the same size")
    live.map.close()
    for field in used:
        raises(BAD, lambda: small_live(rng, dict(used, **{field: used[field] - 1})))
    raises(BAD, lambda: small_live(rng, dict(used, max_list=65536)))
    live = small_live(rng, dict(used, max_list=65535))
    assert live.map.max_list == 65535
    live.map.close()


# ---- refusals --------------------------------------------------------------------------------
def test_malformed_edits_change_nothing():
    rng = np.random.default_rng(11)
    live = small_live(rng, dict(ranges=100, bound_bytes=100, path_entries=100, list_ids=1000, max_list=9))
    o = live.check("created")
    args = key_buffers(o)
    before = route_bytes(live, o, args)
    m = live.map
    # ranges: (-inf, b) [b, d) [d, dd) [dd, +inf)
    bad_calls = {
        "range >= R": lambda: m.split(4, [], [[0]]),
        "pieces == 0": lambda: m.split(1, [], []),
        "equal to the lower boundary": lambda: m.split(1, [b"b"], [[0], [0]]),
        "below the lower boundary": lambda: m.split(1, [b"a"], [[0], [0]]),
        "equal to the upper boundary": lambda: m.split(1, [b"d"], [[0], [0]]),
        "above the upper boundary": lambda: m.split(1, [b"c", b"e"], [[0], [0], [0]]),
        "equal new boundaries": lambda: m.split(1, [b"c", b"c"], [[0], [0], [0]]),
        "descending new boundaries": lambda: m.split(1, [b"cc", b"c"], [[0], [0], [0]]),
        "a zero-length boundary that is not the first": lambda: m.split(1, [b""], [[0], [0]]),
        "below the last range": lambda: m.split(3, [b"dd"], [[0], [0]]),
        "above range 0": lambda: m.split(0, [b"b"], [[0], [0]]),
        "a path entry >= num_segments": lambda: m.split(1, [b"c"], [[0], [5]]),
        "a path over room.max_list": lambda: m.split(1, [b"c"], [[0], [0, 3, 1]]),
        "first + count > R": lambda: m.set_paths(2, [[0], [0], [0]]),
        "first > R": lambda: m.set_paths(5, []),
        "set_paths entry >= num_segments": lambda: m.set_paths(2, [[0], [7]]),
        "set_paths over room.max_list": lambda: m.set_paths(2, [[3, 3]]),
    }
    for what, call in bad_calls.items():
        raises(BAD, call)
        assert m.num_ranges == 4, what
    L = E.load_library()
    u64 = lambda x: np.array(x, dtype=np.uint64)  # noqa: E731
    bb, path = np.frombuffer(b"cccc", dtype=np.uint8), np.zeros(4, dtype=np.uint32)
    up, down = u64([0, 1, 2]), u64([2, 1, 2])

    def split(h=m.h, b=bb.ctypes.data, bo=up.ctypes.data, p=path.ctypes.data, po=up.ctypes.data):
        return L.rf_amd_range_map_split(h, 1, 2, b, bo, p, po, None)

    assert split(h=None) == BAD and b"null range map" in L.rf_amd_last_error()
    assert split(bo=down.ctypes.data) == BAD and b"decrease" in L.rf_amd_last_error()
    assert split(po=down.ctypes.data) == BAD and b"decrease" in L.rf_amd_last_error()
    assert split(b=None) == BAD and split(bo=None) == BAD and split(p=None) == BAD and split(po=None) == BAD
    assert L.rf_amd_range_map_set_paths(m.h, 1, 2, None, up.ctypes.data, None) == BAD
    assert L.rf_amd_range_map_set_paths(m.h, 1, 2, path.ctypes.data, None, None) == BAD
    # a flat map, and a map made from segments without room
    flat = E.RangeMap([b"c"], [[1], [2]])
    roomless = E.RangeMap.from_segments(live.bounds, live.paths, live.lists, SMALL_CAPS)
    for other, word in ((flat, b"flat"), (roomless, b"without room")):
        assert split(h=other.h) == BAD and word in L.rf_amd_last_error()
        assert L.rf_amd_range_map_set_paths(other.h, 0, 1, path.ctypes.data, up.ctypes.data, None) == BAD
        assert L.rf_amd_range_map_set_paths(other.h, 0, 0, None, None, None) == BAD
        raises(BAD, lambda: other.split(0, [], [[]]))
    check_route(raw_route(roomless, o, args, pair_cap=o.total + 64), o, "the roomless map", cap=o.total + 64)
    flat.close()
    roomless.close()
    assert m.num_ranges == 4 and route_bytes(live, o, args) == before
    assert split() == 0  # and the same arrays are a legal call: "c" with paths [0], [0]
    assert L.rf_amd_range_map_num_ranges(m.h) == 5
    live.bounds, live.paths = E.range_split_host(live.bounds, live.paths, 1, [b"c"], [[0], [0]])
    live.check("after the legal call", newest=[b"c"])
    m.close()


@pytest.mark.parametrize("blocks", [1, 2])
def test_grid_stride_loops(blocks):
    """the splice's copy of more than two tiles of ranges on one and two workgroups"""
    rng = np.random.default_rng(12)
    live = Live(rng, make_bounds(rng, 2 * TILE + 77))
    r, nb = roomy_range(live, 3, lo_r=TILE // 2, hi_r=TILE)
    try:
        E.diag_fanout_max_blocks(blocks)
        live.split(r, nb, [rand_path(rng) for _ in range(4)])
        live.check(("capped", blocks), newest=nb)
    finally:
        E.diag_fanout_max_blocks(0)
    live.set_paths(r, [[ROOT], []])
    live.check(("cap lifted", blocks), newest=nb)
    live.map.close()


# ---- in the world of the multi-get -----------------------------------------------------------
def test_multiget_routed_follows_a_split(world):  # noqa: F811
    """test_gpu_range_segments' end-to-end case with a leaf split in it: on one stream, a member
    update of the set, the update of the spare segments the new leaves get, and the split that
    names them; then both routed multi-gets"""
    w = world
    rng = np.random.default_rng(98)
    n = RR.N
    pk = np.ascontiguousarray(w.pk).reshape(n, -1).view(np.uint8).reshape(n, 24)
    keys = [bytes(pk[i]) for i in range(n)]
    picked = sorted({keys[i] for i in rng.choice(n, size=31, replace=False)})
    assert len(picked) > 16
    held = picked[15]  # the boundary the split brings in
    bounds = [b for b in picked if b != held]
    R = len(bounds) + 1
    slot = [0, 1, None, 3, 4, 5, None, None]  # slot -> the world's member whose filter sits there
    fs = E.FilterSet(w.members, capacity=8)
    # 0: the root's; 5 and 6: the spare segments of a split, in no path yet
    seg = [[0, 3], [1], [2, 5], [4], [7, 1], [], []]
    caps = [4, 3, 4, 2, 2, 3, 3]
    paths = [[0] + rng.choice([1, 2, 3, 4], size=int(rng.integers(0, 3)), replace=False).tolist() for _ in range(R)]
    paths[2] = []
    r = 15  # the range that holds `held`
    paths[r] = [0, 3]
    room = dict(ranges=R + 4, bound_bytes=24 * (R + 4), path_entries=4 * (R + 4), list_ids=16 * (R + 4), max_list=16)
    rmap = E.RangeMap.from_segments(bounds, paths, seg, caps, room=room)
    assert rmap.max_list == 16
    d_keys = RR.dev(w.pk)

    def want_of():
        rg, off, member, total = E.range_route_host(bounds, E.range_segment_lists(paths, seg), keys)
        key = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
        src = np.array([-1 if slot[i] is None else slot[i] for i in member], dtype=np.int64)
        words = np.where(src >= 0, w.words["keys"][np.maximum(src, 0), key], np.uint64(0))
        return words, off, member

    def check(stream=None):
        words, off, member = want_of()
        want = E.found_candidates(words)
        want_key = E.ragged_pair_keys(off, want >> np.uint64(8))
        assert len(want) > 100
        d_cand, count, d_key = fs.multiget_routed(rmap, d_keys, 24, n, stream=stream)
        assert count == len(want)
        assert (d_cand[:count].cpu().numpy().view(np.uint64) == want).all()
        assert (d_key.cpu().numpy() == want_key).all()
        key_off, cand, cand_key = E.found_per_key_host(words, member, off)
        d_key_off, d_cand, count, d_cand_key = fs.multiget_routed_per_key(rmap, d_keys, 24, n, stream=stream)
        assert count == len(cand)
        assert (d_key_off.cpu().numpy().view(np.uint64) == key_off).all()
        assert (d_cand[:count].cpu().numpy().view(np.uint64) == cand).all()
        assert (d_cand_key[:count].cpu().numpy() == cand_key).all()
        return want

    before = check()
    s = torch.cuda.Stream()
    h = s.cuda_stream
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        # the leaf of range r splits in two at `held`: C's filter moves from slot 4 to slot 6, which
        # both new leaves name, and the root takes an incorporated bundle, D's filter, in slot 2
        fs.update([6, 4, 2], [w.members[4], None, w.members[5]], stream=h)
        slot[6], slot[4], slot[2] = 4, None, 5
        seg[5], seg[6], seg[0] = [6], [7, 6], [0, 3, 2]
        rmap.update_segments([5, 6, 0], [seg[5], seg[6], seg[0]], stream=h)
        rmap.split(r, [held], [[0, 5], [0, 6]], stream=h)
        bounds, paths = E.range_split_host(bounds, paths, r, [held], [[0, 5], [0, 6]])
        assert rmap.num_ranges == R + 1 and bounds == picked
        after = check(stream=h)
    assert not np.array_equal(after, before)
    rmap.close_on(h)
    assert rmap.h is None
    fs.close_on(h)
    s.synchronize()
