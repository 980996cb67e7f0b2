"""Range maps: rf_amd_range_map_route_keys / _route_var_keys (k_range_find, k_range_scan,
k_range_emit) and FilterSet.multiget_routed / multiget_var_routed. The oracle of routing is
E.range_route_host (bisect over `bytes`, checked against the reference's find_pivot loop in
test_range_host.py): d_range, every offset, every id and *d_total must equal it exactly. The
buffers of a route call lie between sentinel words that must stay as they were. The end-to-end
tests run in test_gpu_multiget's world and compare with E.found_candidates of the oracle's
routing_filter_lookup words of each key in its range's members."""
from types import SimpleNamespace

import numpy as np
import pytest

import test_gpu_multiget as MG
import test_gpu_multiget_var as MV
from splinterdb_amd import engine as E
from test_gpu_multiget import world  # noqa: F401  (the fixture; a fresh instance for this module)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = MG.N  # 64 * 37 + 13
SENT = 512
ALPHABET = [0x00, 0x61, 0x7F, 0x80, 0xFF]  # bytes at or above 0x80 catch a signed compare
LENS = [0, 1, 2, 7, 8, 9, 10, 16, 17, 40]
TILE = E.diag_range_tile()
LDS_R = E.diag_range_lds_ranges()  # the largest R searched in LDS
N_TILES = 3 * TILE + 77            # three whole scan tiles and a partial one
RS = [1, 2, 3, 64, 65, 1000, LDS_R, LDS_R + 1]
WIDE = 200  # keys of the wide empty range: a whole wave and a run across a wave boundary


def dev(a):
    return MG.dev(np.array(a))


def rand_bytes(rng, n):
    return bytes(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), size=n))


def make_bounds(rng, R, extra_len=None):
    """R - 1 distinct boundaries, sorted: the placed ones first (the trailing-zero family, a run
    of seven that share their first 8 bytes), then random ones, four in ten of them behind one of
    six 8-byte heads so that runs of equal prefixes are everywhere"""
    if R == 2:
        return [b""]  # the empty key as the only boundary: range 0 is empty
    lens = LENS + ([extra_len] if extra_len else [])
    heads = [rand_bytes(rng, 8) for _ in range(5)] + [b"\x61\x7f" + bytes(6)]
    placed = [b"\x61\x7f", b"\x61\x7f\0", b"\x61\x7f\0\0"]
    tie = heads[0]
    placed += [tie, tie + b"\0", tie + b"\x61", tie + b"\x7f", tie + b"\x80", tie + b"\x80\0", tie + b"\xff" * 9]
    if extra_len:
        placed += [rand_bytes(rng, extra_len) for _ in range(4)]
        if extra_len > 8:
            placed.append(tie + rand_bytes(rng, extra_len - 8))
    out = set(placed[:R - 1]) if R - 1 < len(placed) else set(placed)
    while len(out) < R - 1:
        ln = lens[rng.integers(0, len(lens))]
        if rng.random() < 0.4 and ln >= 8:
            out.add(heads[rng.integers(0, len(heads))] + rand_bytes(rng, ln - 8))
        else:
            out.add(rand_bytes(rng, ln))
    return sorted(out)


def make_keys(rng, bounds, n, fixed_len=None):
    """n keys: three in ten equal to a boundary, then proper prefixes of boundaries, boundaries
    with a byte appended, zero-length keys and random ones; fixed_len: every key of that length
    (the equal ones from the boundaries of that length, the others cut or filled up to it)"""
    pool = [b for b in bounds if fixed_len is None or len(b) == fixed_len]
    keys = []
    for _ in range(n):
        how = rng.random()
        b = bounds[rng.integers(0, len(bounds))] if bounds else b""
        if how < 0.3 and pool:
            k = pool[rng.integers(0, len(pool))]
        elif how < 0.4:
            k = b[:rng.integers(0, max(1, len(b)))]
        elif how < 0.5:
            k = b + rand_bytes(rng, 1)
        elif how < 0.55:
            k = b""
        else:
            k = rand_bytes(rng, LENS[rng.integers(0, len(LENS))])
        if fixed_len is not None and len(k) != fixed_len:
            k = (b + rand_bytes(rng, fixed_len))[:fixed_len] if how < 0.5 else (k + rand_bytes(rng, fixed_len))[:fixed_len]
        keys.append(k)
    return keys


def make_case(seed, R, n, fixed_len=None, in_order=True, ends_empty=True, long_key=False):
    """a table of R ranges, n keys and the host mirror's answer. Lists have 0-9 ids; with R >= 64
    three ranges that keys fall into have exactly 64, 128 and 300, and one range with an empty
    list holds WIDE equal keys; there the ranges of the smallest and the largest key have empty
    lists (ends_empty) or lists of 3 and 5 ids."""
    rng = np.random.default_rng(seed)
    c = SimpleNamespace(R=R, n=n, fixed_len=fixed_len)
    c.bounds = make_bounds(rng, R, fixed_len)
    assert len(c.bounds) == R - 1
    keys = make_keys(rng, c.bounds, n, fixed_len)
    wide = None
    if R >= 64:
        pool = [j for j, b in enumerate(c.bounds) if fixed_len is None or len(b) == fixed_len]
        wide = pool[len(pool) // 2] + 1  # the range to the right of that boundary
        at = int(rng.integers(0, n - WIDE))
        keys[at:at + WIDE] = [c.bounds[wide - 1]] * WIDE
    if long_key:  # past any 4 KiB window; decided behind the bytes of a 40-byte boundary
        b40 = [b for b in c.bounds if len(b) == 40]
        keys[n // 2] = (b40[0] if b40 else b"\x61") + rand_bytes(rng, 5000)
        keys[n // 2] = keys[n // 2][:5000]
    if in_order:
        keys.sort()
    c.keys = keys
    lists = [rng.integers(0, 8, size=rng.integers(0, 10)).tolist() for _ in range(R)]
    rg, _, _, _ = E.range_route_host(c.bounds, lists, keys)
    r_first, r_last = int(rg[keys.index(min(keys))]), int(rg[keys.index(max(keys))])
    c.placed = {}
    if R >= 64:
        hit = [int(r) for r in np.unique(rg) if r not in (r_first, r_last, wide)]
        for r, ln in zip(rng.choice(hit, size=3, replace=False), (64, 128, 300)):
            lists[int(r)] = rng.integers(0, 8, size=ln).tolist()
            c.placed[ln] = int(r)
        lists[wide] = []
    c.wide = wide
    if R < 64:  # a few ranges hold every key: none of them empty
        lists = [x or [r + 1] for r, x in enumerate(lists)]
    elif wide not in (r_first, r_last):
        lists[r_first] = [] if ends_empty else [1, 2, 3]
        lists[r_last] = [] if ends_empty else [4, 5, 6, 7, 0]
    c.lists = lists
    c.rg, c.off, c.member, c.total = E.range_route_host(c.bounds, lists, keys)
    c.max_list = max(len(x) for x in lists)
    return c


def key_buffers(c, shift=0, first=0):
    """the device inputs of a case: (d_bytes, d_offsets) for the variable-length form, (d_keys,
    key_len) for the fixed one; the bytes start `shift` bytes off a 16-byte boundary"""
    data = np.frombuffer(b"".join(c.keys), dtype=np.uint8)
    if c.fixed_len is None:
        offs = np.zeros(c.n + 1, dtype=np.uint64)
        np.cumsum(np.array([len(k) for k in c.keys], dtype=np.uint64), out=offs[1:])
        return MV.dev_var(data, offs, shift=shift, first=first)
    buf = torch.full((len(data) + 32,), 0xEE, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    buf[shift:shift + len(data)] = dev(data)
    return buf[shift:], c.fixed_len


def raw_route(rmap, c, args, n=None, pair_cap=None, null_member=False, stream=None):
    """one route call through the C ABI on buffers between sentinels: returns (range, off, member
    below pair_cap, total) as numpy arrays after checking every sentinel word"""
    L = E.load_library()
    n = c.n if n is None else n
    cap = c.total if pair_cap is None else pair_cap
    d_range = torch.full((SENT + n + SENT,), -7, dtype=torch.int32, device="cuda:0")
    d_off = torch.full((SENT + n + 1 + SENT,), -7, dtype=torch.int64, device="cuda:0")
    d_member = torch.full((SENT + cap + SENT,), -7, dtype=torch.int32, device="cuda:0")
    d_total = torch.full((3,), -7, dtype=torch.int64, device="cuda:0")
    scratch = torch.empty(E.range_route_scratch_bytes(n) // 8, dtype=torch.int64, device="cuda:0")
    out = (d_range.data_ptr() + 4 * SENT, d_off.data_ptr() + 8 * SENT,
           None if null_member else d_member.data_ptr() + 4 * SENT, cap, d_total.data_ptr() + 8, scratch.data_ptr(),
           stream)
    if c.fixed_len is None:
        rc = L.rf_amd_range_map_route_var_keys(rmap.h, args[0].data_ptr(), args[1].data_ptr(), n, *out)
    else:
        rc = L.rf_amd_range_map_route_keys(rmap.h, args[0].data_ptr(), args[1], n, *out)
    assert rc == 0, L.rf_amd_last_error()
    torch.cuda.synchronize()
    r, o, m, t = (x.cpu().numpy() for x in (d_range, d_off, d_member, d_total))
    assert (r[:SENT] == -7).all() and (r[SENT + n:] == -7).all(), "wrote outside d_range"
    assert (o[:SENT] == -7).all() and (o[SENT + n + 1:] == -7).all(), "wrote outside d_member_off"
    assert (m[:SENT] == -7).all() and (m[SENT + cap:] == -7).all(), "wrote at or past d_member[pair_cap)"
    assert t[0] == -7 and t[2] == -7, "wrote outside d_total"
    return (r[SENT:SENT + n].view(np.uint32), o[SENT:SENT + n + 1].view(np.uint64),
            m[SENT:SENT + cap].view(np.uint32), int(t[1]))


def check_route(got, c, what, cap=None):
    r, o, m, t = got
    bad = np.flatnonzero(r != c.rg)
    assert bad.size == 0, (what, "range", bad.size, bad[:8].tolist(), r[bad[:8]], c.rg[bad[:8]],
                           [c.keys[i][:12] for i in bad[:4]])
    assert (o == c.off).all(), (what, "offsets", np.flatnonzero(o != c.off)[:8])
    assert t == c.total, (what, "total", t, c.total)
    k = c.total if cap is None else min(cap, c.total)
    bad = np.flatnonzero(m[:k] != c.member[:k])
    assert bad.size == 0, (what, "ids", bad.size, bad[:8].tolist())
    if cap is not None and cap > c.total:
        assert (m.view(np.int32)[c.total:] == -7).all(), (what, "wrote past the pairs")


@pytest.fixture(scope="module")
def maps():
    """cases and their resident maps by key, made once and read-only; closed at the end"""
    cache = {}

    def get(R, n=N, fixed_len=None, in_order=True, ends_empty=True, long_key=False):
        key = (R, n, fixed_len, in_order, ends_empty, long_key)
        if key not in cache:
            seed = sum(int(x or 0) * p for x, p in zip(key, (7, 11, 13, 17, 19, 23)))
            c = make_case(seed, R, n, fixed_len, in_order, ends_empty, long_key)
            cache[key] = (c, E.RangeMap(c.bounds, c.lists))
        return cache[key]
    yield get
    for _, m in cache.values():
        m.close()


# ---- the cases say what they claim -----------------------------------------------------------
def test_placed_cases_exist(maps):
    c, m = maps(1000)
    assert m.num_ranges == 1000 and m.max_list == 300 == c.max_list
    b = c.bounds
    assert {len(x) for x in b} >= set(LENS)
    assert b"\x61\x7f" in b and b"\x61\x7f\0" in b and b"\x61\x7f\0\0" in b
    pre = [x[:8].ljust(8, b"\0") for x in b]
    run = max(sum(1 for y in pre if y == x) for x in set(pre))
    assert run >= 5, "a run of boundaries that share their first 8 bytes"
    assert any(len(x) >= 8 and x[:8] == y[:8] and x != y for x, y in zip(b, b[1:]))
    assert any(v >= 0x80 for x in b for v in x)
    # keys: about three in ten equal to a boundary, on the boundary's right side
    bset = set(b)
    eq = np.array([k in bset for k in c.keys])
    assert 0.2 < eq.mean() < 0.6
    for i in np.flatnonzero(eq)[:50]:
        assert b[c.rg[i] - 1] == c.keys[i]
    assert any(len(k) == 0 for k in c.keys)
    assert any(any(x.startswith(k) and x != k for x in b) for k in c.keys if k)
    # lists: 0-9 and the placed 64, 128, 300; in key order a whole wave and a run across a wave
    # boundary own no pairs; key 0 and key n - 1 have empty lists
    cnt = np.diff(c.off.astype(np.int64))
    assert set(range(10)) <= set(cnt.tolist()) and {64, 128, 300} <= set(cnt.tolist())
    assert cnt[0] == 0 and cnt[-1] == 0
    wide = np.flatnonzero(c.rg == c.wide)
    assert wide.size >= WIDE and (np.diff(wide) == 1).all() and (cnt[wide] == 0).all()
    assert wide[-1] // 64 - wide[0] // 64 >= 2, "a whole wave inside the run, and a crossing"
    c2, _ = maps(1000, ends_empty=False)
    cnt2 = np.diff(c2.off.astype(np.int64))
    assert cnt2[0] > 0 and cnt2[-1] > 0
    cs, _ = maps(1000, in_order=False)
    assert cs.keys != sorted(cs.keys)
    # R = 2 cut by the empty key: nothing is below it
    ce, _ = maps(2)
    assert ce.bounds == [b""] and (ce.rg == 1).all()
    assert N_TILES > 3 * TILE and N_TILES % TILE and N > 2 * TILE


# ---- variable-length keys --------------------------------------------------------------------
@pytest.mark.parametrize("in_order", [True, False], ids=["key_order", "shuffled"])
@pytest.mark.parametrize("R", RS)
def test_route_var_keys(maps, R, in_order):
    c, m = maps(R, in_order=in_order)
    check_route(raw_route(m, c, key_buffers(c)), c, (R, in_order))


def test_route_var_keys_ends_own_pairs(maps):
    c, m = maps(1000, ends_empty=False)
    check_route(raw_route(m, c, key_buffers(c)), c, "ends own pairs")


def test_var_long_key_and_unaligned_base(maps):
    """one key of 5,000 B, d_offsets[0] = 1000, d_bytes 5 bytes off a 16-byte boundary"""
    c, m = maps(1000, long_key=True)
    assert max(len(k) for k in c.keys) == 5000
    args = key_buffers(c, shift=5, first=1000)
    assert args[0].data_ptr() % 16 == 5 and int(args[1][0]) == 1000
    check_route(raw_route(m, c, args), c, "long key, shifted")


@pytest.mark.parametrize("in_order", [True, False], ids=["key_order", "shuffled"])
def test_several_scan_tiles(maps, in_order):
    c, m = maps(1000, n=N_TILES, in_order=in_order)
    check_route(raw_route(m, c, key_buffers(c)), c, ("tiles", in_order))


@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_small_n(maps, n):
    """the first n keys of a larger case: the oracle's answer is a prefix of the whole"""
    c, m = maps(65, in_order=False)
    sub = SimpleNamespace(**vars(c))
    sub.n, sub.keys = n, c.keys[:n]
    sub.rg, sub.off, sub.member, sub.total = E.range_route_host(c.bounds, c.lists, sub.keys)
    check_route(raw_route(m, sub, key_buffers(sub)), sub, n)


# ---- fixed-length keys -----------------------------------------------------------------------
@pytest.mark.parametrize("in_order", [True, False], ids=["key_order", "shuffled"])
@pytest.mark.parametrize("key_len,shift", [(24, 0), (5, 1), (13, 1)])
def test_route_keys(maps, key_len, shift, in_order):
    c, m = maps(1000, fixed_len=key_len, in_order=in_order)
    assert all(len(k) == key_len for k in c.keys)
    bset = set(c.bounds)
    eq = np.mean([k in bset for k in c.keys])
    assert eq > 0.2, eq
    args = key_buffers(c, shift=shift)
    assert args[0].data_ptr() % 16 == shift
    check_route(raw_route(m, c, args), c, (key_len, shift, in_order))


@pytest.mark.parametrize("R", [1, 2, LDS_R, LDS_R + 1])
def test_route_keys_other_tables(maps, R):
    c, m = maps(R, fixed_len=24, in_order=False)
    check_route(raw_route(m, c, key_buffers(c)), c, R)


# ---- pair_cap --------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed_len", [None, 24])
def test_pair_cap(maps, fixed_len):
    c, m = maps(1000, fixed_len=fixed_len)
    args = key_buffers(c)
    assert c.total > 1000
    full = c.n * m.max_list
    assert full > c.total
    for cap in (c.total, full, c.total // 2, c.total - 1, 1):
        # below the total: the ids below the cap, the true offsets and total, nothing at or past
        # d_member[cap) (raw_route's sentinels)
        check_route(raw_route(m, c, args, pair_cap=cap), c, ("cap", cap), cap=cap)
    check_route(raw_route(m, c, args, pair_cap=0, null_member=True), c, "cap 0, NULL d_member", cap=0)


def test_n_zero(maps):
    c, m = maps(65)
    args = key_buffers(c)
    r, o, mem, t = raw_route(m, c, args, n=0, pair_cap=8)
    assert r.size == 0 and o.tolist() == [0] and t == 0
    assert (mem.view(np.int32) == -7).all()
    d_range, d_off, d_member, d_total = m.route_var_keys(None, None, 0)
    torch.cuda.synchronize()
    assert d_off.tolist() == [0] and d_total.item() == 0 and d_range.numel() == 0 and d_member.numel() == 0


# ---- grid-stride loops, repeatability --------------------------------------------------------
@pytest.mark.parametrize("fixed_len", [None, 24])
@pytest.mark.parametrize("blocks", [1, 2])
def test_grid_stride_loops(maps, blocks, fixed_len):
    """three tiles (and four) on one and two workgroups: every loop of the three kernels runs
    more than once in a workgroup"""
    try:
        E.diag_fanout_max_blocks(blocks)
        for n in (N, N_TILES):
            c, m = maps(1000, n=n, fixed_len=fixed_len)
            check_route(raw_route(m, c, key_buffers(c)), c, (blocks, n))
    finally:
        E.diag_fanout_max_blocks(0)


def test_two_runs_give_identical_bytes(maps):
    c, m = maps(1000, in_order=False)
    args = key_buffers(c)
    a = raw_route(m, c, args, pair_cap=c.total + 100)
    b = raw_route(m, c, args, pair_cap=c.total + 100)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    assert a[3] == b[3]


# ---- the Python calls ------------------------------------------------------------------------
def test_python_route_calls(maps):
    c, m = maps(1000, in_order=False)
    d_bytes, d_offs = key_buffers(c)
    d_range, d_off, d_member, d_total = m.route_var_keys(d_bytes, d_offs, c.n)
    torch.cuda.synchronize()
    assert d_member.numel() == c.n * m.max_list  # pair_cap None: never overflows
    got = (d_range.cpu().numpy().view(np.uint32), d_off.cpu().numpy().view(np.uint64),
           d_member.cpu().numpy().view(np.uint32), int(d_total.item()))
    check_route(got, c, "route_var_keys")
    c, m = maps(1000, fixed_len=24)
    d_keys, key_len = key_buffers(c)
    d_range, d_off, d_member, d_total = m.route_keys(d_keys, key_len, c.n, pair_cap=c.total)
    torch.cuda.synchronize()
    got = (d_range.cpu().numpy().view(np.uint32), d_off.cpu().numpy().view(np.uint64),
           d_member.cpu().numpy().view(np.uint32), int(d_total.item()))
    check_route(got, c, "route_keys")


def test_errors(maps):
    c, m = maps(65)
    L = E.load_library()
    d_bytes, d_offs = key_buffers(c)
    n = c.n
    rg = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
    mem = torch.zeros(c.total, dtype=torch.int32, device="cuda:0")
    tot = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    scr = torch.zeros(E.range_route_scratch_bytes(n) // 8, dtype=torch.int64, device="cuda:0")
    p = SimpleNamespace(b=d_bytes.data_ptr(), o=d_offs.data_ptr(), r=rg.data_ptr(), f=off.data_ptr(),
                        m=mem.data_ptr(), t=tot.data_ptr(), s=scr.data_ptr())
    B = E.STATUS_BAD_PARAM

    def var(h=m.h, b=p.b, o=p.o, n=n, r=p.r, f=p.f, mm=p.m, cap=c.total, t=p.t, s=p.s):
        return L.rf_amd_range_map_route_var_keys(h, b, o, n, r, f, mm, cap, t, s, None)

    def keys(h=m.h, b=p.b, kl=24, n=10, r=p.r, f=p.f, mm=p.m, cap=c.total, t=p.t, s=p.s):
        return L.rf_amd_range_map_route_keys(h, b, kl, n, r, f, mm, cap, t, s, None)

    assert var() == 0 and keys() == 0
    assert var(h=None) == B and keys(h=None) == B
    assert keys(kl=0) == B
    assert var(n=1 << 56) == B and keys(n=1 << 56) == B
    assert var(b=None) == B and var(o=None) == B and var(r=None) == B and var(f=None) == B
    assert var(t=None) == B and var(s=None) == B and var(mm=None) == B
    assert keys(b=None) == B and keys(r=None) == B and keys(f=None) == B and keys(t=None) == B
    assert keys(s=None) == B and keys(mm=None) == B
    assert var(mm=None, cap=0) == 0 and keys(mm=None, cap=0) == 0
    assert var(n=0, b=None, o=None, r=None, mm=None, s=None) == 0  # n == 0: the outputs it writes only
    torch.cuda.synchronize()

    def einval(fn):
        with pytest.raises(E.PlatformStatusError) as ei:
            fn()
        assert ei.value.code == E.STATUS_BAD_PARAM

    einval(lambda: E.RangeMap([b"b", b"a"], [[1], [2], [3]]))
    einval(lambda: E.RangeMap([b"a", b"a"], [[1], [2], [3]]))
    einval(lambda: E.RangeMap([b"\x80", b"\x7f"], [[1], [2], [3]]))
    einval(lambda: E.RangeMap([b"a"], [[1], [0] * 65536]))
    E.RangeMap([b"a"], [[1], [0] * 65535]).close()
    one = E.RangeMap([], [[]])
    assert one.num_ranges == 1 and one.max_list == 0
    one.close()


# ---- in the world of the multi-get -----------------------------------------------------------
NM = 6  # the world's set: (A0, A1, None, B0, C0, D0); ids 6 and 7 are past the end


@pytest.fixture(scope="module")
def routed(world, oracle):  # noqa: F811
    """boundaries drawn from the world's 24-byte probe keys and from variable-length probes, lists
    over ids 0-7, and the oracle's word of every pair"""
    w = world
    rng = np.random.default_rng(777)
    r = SimpleNamespace()
    pk = np.ascontiguousarray(w.pk).reshape(N, -1).view(np.uint8).reshape(N, 24)
    r.keys = [bytes(pk[i]) for i in range(N)]
    third = N // 3
    lens = rng.integers(0, 61, size=N)
    lens[rng.random(N) < 0.1] = 0
    lens[:2 * third] = 24
    vdata, r.voffs = MV.rand_keys(rng, lens)
    vdata[r.voffs[:2 * third].astype(np.int64)[:, None] + np.arange(24)] = pk[:2 * third]
    r.vdata = vdata
    r.vkeys = [bytes(vdata[int(a):int(b)]) for a, b in zip(r.voffs[:-1], r.voffs[1:])]
    vh = oracle.hash_var(r.vdata, r.voffs)
    r.words = {"keys": w.words["keys"], "var": MV.member_words(w.ofs, vh)}

    def table(keys):
        pick = rng.choice(N, size=40, replace=False)
        bounds = sorted({keys[i] for i in pick[:30]} | {keys[i][:int(rng.integers(1, 9))] for i in pick[30:] if keys[i]})
        lists = [rng.integers(0, NM + 2, size=rng.integers(0, 10)).tolist() for _ in range(len(bounds) + 1)]
        lists[3] = list(range(NM + 2))  # every member, the None member and the ids past the end
        return bounds, lists
    r.table = {"keys": table(r.keys), "var": table(r.vkeys)}
    r.host = {"keys": E.range_route_host(*r.table["keys"], r.keys), "var": E.range_route_host(*r.table["var"], r.vkeys)}
    return r


def want_pairs(words, off, member):
    key = np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))
    ok = member < NM
    return np.where(ok, words[np.where(ok, member, 0), key], np.uint64(0))


def routed_inputs(w, r, form):
    if form == "keys":
        return (dev(w.pk), 24)
    return MV.dev_var(r.vdata, r.voffs, shift=3)


@pytest.mark.parametrize("form", ["keys", "var"])
def test_multiget_routed_end_to_end(world, routed, form):  # noqa: F811
    w, r = world, routed
    rg, off, member, total = r.host[form]
    assert (member == 2).any() and (member >= NM).any() and total > N
    want = E.found_candidates(want_pairs(r.words[form], off, member))
    want_key = E.ragged_pair_keys(off, want >> np.uint64(8))
    assert len(want) > 16
    rmap = E.RangeMap(*r.table[form])
    fn = w.set.multiget_routed if form == "keys" else w.set.multiget_var_routed
    for cap in (16, len(want), None):  # 16: too small, the count is still the total and the second pass runs
        d_cand, count, d_key = fn(rmap, *routed_inputs(w, r, form), N, cap=cap)
        assert count == len(want), (cap, count, len(want))
        assert (d_cand[:count].cpu().numpy().view(np.uint64) == want).all(), cap
        assert d_key.shape == (count,) and (d_key.cpu().numpy() == want_key).all(), cap
    rmap.close()


def test_route_output_outlives_the_map(world, routed):  # noqa: F811
    """route on a stream of the caller's, release the map behind it on that stream, then the
    ragged probe of the route call's output: the output is a copy"""
    w, r = world, routed
    rg, off, member, total = r.host["keys"]
    s = torch.cuda.Stream()
    h = s.cuda_stream
    with torch.cuda.stream(s):
        d_keys = dev(w.pk)
        rmap = E.RangeMap(*r.table["keys"])
        d_range, d_off, d_member, d_total = rmap.route_keys(d_keys, 24, N, stream=h)
        rmap.close_on(h)
        assert rmap.h is None
        d_found = torch.full((N * rmap.max_list + SENT,), -7, dtype=torch.int64, device="cuda:0")
        w.set.probe_keys_ragged(d_keys, 24, d_member, d_off, N, d_found, stream=h)
        # a new map may take the released block while the probe is still queued
        other = E.RangeMap(*r.table["var"])
    s.synchronize()
    torch.cuda.synchronize()
    assert int(d_total.item()) == total
    assert (d_range.cpu().numpy().view(np.uint32) == rg).all()
    assert (d_off.cpu().numpy().view(np.uint64) == off).all()
    assert (d_member[:total].cpu().numpy().view(np.uint32) == member).all()
    got = d_found.cpu().numpy()
    assert (got[total:] == -7).all()
    assert (got[:total].view(np.uint64) == want_pairs(r.words["keys"], off, member)).all()
    other.close()
