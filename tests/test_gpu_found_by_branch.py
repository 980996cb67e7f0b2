"""The group-by-branch call: rf_amd_found_by_branch (k_bb_hist, k_bb_scan, k_bb_scatter per digit
pass; k_bb_heads, k_bb_scan, k_bb_emit for the run table) and FilterSet.group_by_branch. The
oracle of every buffer is the host mirror (E.found_by_branch_host, checked against a plain
transcription in test_found_by_branch_host.py): d_order, d_order_key, d_branch, d_branch_off and
*d_num_branches must equal it byte for byte, and every output lies between sentinel words that
must stay as they were. The call works on any records, so most cases are synthetic and need no
filter; the end-to-end test runs in test_gpu_multiget's world."""
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
TILE = E.diag_by_branch_tile()
BIG = 3 * TILE + 77  # three whole tiles and a partial one
SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, BIG]
MAX_MEMBERS = 1 << 26
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def pass_boundaries():
    """the largest num_members of every pass count, read from the library: the count is
    non-decreasing in num_members, so each is found by bisection"""
    top = E.diag_by_branch_passes(MAX_MEMBERS)
    out = []
    for p in range(1, top):
        lo, hi = 1, MAX_MEMBERS  # passes(lo) <= p < passes(hi)
        assert E.diag_by_branch_passes(lo) <= p
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if E.diag_by_branch_passes(mid) <= p:
                lo = mid
            else:
                hi = mid
        out.append(lo)
    return out


BOUNDS = pass_boundaries()
MEMBERS = sorted({1, MAX_MEMBERS} | {b + d for b in BOUNDS for d in (0, 1)})


def dev(a):
    """a host array on the device; unsigned words travel as the signed type of their width"""
    a = np.array(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return MG.dev(a if signed is None else a.view(signed))


def rec(ids, values):
    return (np.asarray(ids, dtype=np.uint64) << np.uint64(8)) | np.asarray(values, dtype=np.uint64)


def from_keys(keys):
    keys = np.asarray(keys, dtype=np.uint64)
    return rec(keys >> np.uint64(6), keys & np.uint64(63))


# ---- the record distributions: (m, num_members, rng) -> m records ------------------------------
def one_branch(m, nm, rng):
    return rec(np.full(m, nm // 2), np.full(m, 5))


def own_branch(m, nm, rng):
    """every record its own branch where the members have that many; else each branch m / (64 *
    num_members) times, in a shuffled order"""
    space = nm * 64
    if space <= 1 << 20:
        perm = rng.permutation(space)
        return from_keys(perm[np.arange(m) % space])
    return from_keys(rng.permutation(np.unique(rng.integers(0, space, size=2 * m + 8)))[:m])


def alternating(m, nm, rng):
    j = np.arange(m)
    return rec(np.where(j & 1, 0, nm - 1), np.where(j & 1, 63, 0))


def extremes(m, nm, rng):
    hi = rng.random(m) < 0.5
    return rec(np.where(hi, nm - 1, 0), np.where(hi, 63, 0))


def highest_digit(m, nm, rng):
    """keys that are equal below the last pass's digit"""
    shift = 8 * (E.diag_by_branch_passes(nm) - 1)
    top = (((nm - 1) << 6) | 63) >> shift
    low = (((nm - 1) << 6) | 63) & ((1 << shift) - 1) & 0x2A
    return from_keys((rng.integers(0, top + 1, size=m, dtype=np.uint64) << np.uint64(shift)) | np.uint64(low))


def uniform(m, nm, rng):
    return rec(rng.integers(0, nm, size=m, dtype=np.uint64), rng.integers(0, 64, size=m, dtype=np.uint64))


def wild(m, nm, rng):
    """ids of all 32 bits and value bytes of all 8: the call masks both"""
    return rec(rng.integers(0, 1 << 32, size=m, dtype=np.uint64), rng.integers(0, 256, size=m, dtype=np.uint64))


DISTS = [one_branch, own_branch, alternating, extremes, highest_digit, uniform, wild]


# ---- one call between sentinels ----------------------------------------------------------------
def sentinel_buf(k, dtype=torch.int64):
    return torch.full((SENT + k + SENT,), -7, dtype=dtype, device="cuda:0")


def inner(buf, k, what):
    a = buf.cpu().numpy()
    assert (a[:SENT] == -7).all() and (a[SENT + k:] == -7).all(), "wrote outside " + what
    return a[SENT:SENT + k]


def raw_call(d_cand, d_cand_key, count, cap, nm, branch_cap, with_key=True, null_branch=False):
    """one call through the C ABI on outputs between sentinels; returns (order uint32[cap],
    order_key uint64[cap] or None, branch uint64[branch_cap] or None, branch_off
    uint64[branch_cap + 1] or None, num_branches)"""
    L = E.load_library()
    d_count = dev(np.array([count], dtype=np.uint64))
    d_order, d_runs = sentinel_buf(cap, torch.int32), sentinel_buf(1)
    d_okey = sentinel_buf(cap) if with_key else None
    d_branch = None if null_branch else sentinel_buf(branch_cap)
    d_boff = None if null_branch else sentinel_buf(branch_cap + 1)
    scratch = torch.empty(E.found_by_branch_scratch_bytes(cap, nm) // 8, dtype=torch.int64, device="cuda:0")

    def at(b, width=8):
        return None if b is None else b.data_ptr() + width * SENT
    rc = L.rf_amd_found_by_branch(E.default_engine().h, E._dptr(d_cand), E._dptr(d_cand_key) if with_key else None,
                                  d_count.data_ptr(), cap, nm, at(d_order, 4), at(d_okey), at(d_branch), at(d_boff),
                                  branch_cap, at(d_runs), scratch.data_ptr(), None)
    assert rc == 0, L.rf_amd_last_error()
    torch.cuda.synchronize()
    return (inner(d_order, cap, "d_order[0, cap)").view(np.uint32),
            None if d_okey is None else inner(d_okey, cap, "d_order_key[0, cap)").view(np.uint64),
            None if d_branch is None else inner(d_branch, branch_cap, "d_branch[0, branch_cap)").view(np.uint64),
            None if d_boff is None else inner(d_boff, branch_cap + 1, "d_branch_off[0, branch_cap]").view(np.uint64),
            int(inner(d_runs, 1, "d_num_branches")[0]))


def check(got, cand, cand_key, count, cap, nm, branch_cap, what):
    order, okey, branch, boff, runs = got
    m = min(count, cap)
    w_order, w_okey, w_branch, w_off = E.found_by_branch_host(cand[:m], nm, None if okey is None else cand_key[:m])
    assert runs == len(w_branch), (what, "num_branches", runs, len(w_branch))
    bad = np.flatnonzero(order[:m] != w_order)
    assert bad.size == 0, (what, "order", bad.size, bad[:8].tolist(), order[bad[:4]], w_order[bad[:4]])
    assert (order[m:].view(np.int32) == -7).all(), (what, "wrote past the order")
    if okey is not None:
        assert okey[:m].tobytes() == w_okey.tobytes(), (what, "order_key")
        assert (okey[m:].view(np.int64) == -7).all(), (what, "wrote past the order's keys")
    k = min(runs, branch_cap)
    if branch is not None:
        assert branch[:k].tobytes() == w_branch[:k].tobytes(), (what, "branch")
        assert (branch[k:].view(np.int64) == -7).all(), (what, "wrote past the branches")
        assert boff[:k].tobytes() == w_off[:k].tobytes() and boff[k] == m, (what, "branch_off", boff[:k + 1][-4:])
        assert (boff[k + 1:].view(np.int64) == -7).all(), (what, "wrote past the branch offsets")


def run_case(cand, nm, what, count=None, cap=None, branch_cap=None, with_key=True, null_branch=False, keys=None):
    """one call over cand and its check; branch_cap None: the true number of runs"""
    count = len(cand) if count is None else count
    cap = len(cand) if cap is None else cap
    if keys is None:
        keys = np.arange(len(cand), dtype=np.uint64) * np.uint64(3) + np.uint64(1 << 40)
    if branch_cap is None:
        branch_cap = len(E.found_by_branch_host(cand[:min(count, cap)], nm)[2])
    # one word more than the call may read, so that no records is still a buffer
    got = raw_call(dev(np.append(cand, ONES)), dev(np.append(keys, ONES)), count, cap, nm, branch_cap, with_key,
                   null_branch)
    check(got, cand, keys, count, cap, nm, branch_cap, what)
    return got


# ---- the cases say what they claim -------------------------------------------------------------
def test_cases_exist():
    assert len(BOUNDS) == E.diag_by_branch_passes(MAX_MEMBERS) - 1 >= 1
    for p, b in enumerate(BOUNDS):
        assert E.diag_by_branch_passes(b) == p + 1 and E.diag_by_branch_passes(b + 1) == p + 2
    assert 1 in MEMBERS and MAX_MEMBERS in MEMBERS and len(MEMBERS) == 2 + 2 * len(BOUNDS)
    rng = np.random.default_rng(0)
    nm = BOUNDS[-1] + 1
    host = E.found_by_branch_host
    assert len(host(one_branch(BIG, nm, rng), nm)[2]) == 1
    assert len(host(own_branch(BIG, nm, rng), nm)[2]) == BIG
    assert len(host(alternating(BIG, nm, rng), nm)[2]) == 2 and len(host(extremes(BIG, nm, rng), nm)[2]) == 2
    k = E.by_branch_sort_key(highest_digit(BIG, nm, rng), nm)
    shift = 8 * (E.diag_by_branch_passes(nm) - 1)
    assert len(set((k & ((1 << shift) - 1)).tolist())) == 1 and len(set((k >> shift).tolist())) > 1
    assert (k >> 6).max() < nm
    w = wild(BIG, 5, rng)
    assert (w >> np.uint64(8)).max() > 1 << 31 and (w & np.uint64(0xC0)).any()
    assert BIG > 3 * TILE and BIG % TILE and TILE % 256 == 0


# ---- every size, pass count and distribution ---------------------------------------------------
@pytest.mark.parametrize("dist", DISTS, ids=lambda f: f.__name__)
@pytest.mark.parametrize("nm", MEMBERS)
def test_sizes(nm, dist):
    """every record count at this num_members and distribution; 2^26 itself runs at the largest
    count with all of them"""
    rng = np.random.default_rng(nm % 1000 + 7 * DISTS.index(dist))
    for m in SIZES:
        run_case(dist(m, nm, rng), nm, (nm, dist.__name__, m))


def test_m_zero_writes_two_words():
    cand = uniform(8, 5, np.random.default_rng(1))
    order, okey, branch, boff, runs = run_case(cand, 5, "count 0", count=0, branch_cap=4)
    assert runs == 0 and boff[0] == 0
    assert (order.view(np.int32) == -7).all() and (branch.view(np.int64) == -7).all()
    # cap 0 with NULL records, order and scratch
    L = E.load_library()
    d_count, d_runs, d_boff = dev(np.array([9], dtype=np.uint64)), sentinel_buf(1), sentinel_buf(3)
    rc = L.rf_amd_found_by_branch(E.default_engine().h, None, None, d_count.data_ptr(), 0, 5, None, None,
                                  d_boff.data_ptr() + 8 * SENT, d_boff.data_ptr() + 8 * SENT, 2,
                                  d_runs.data_ptr() + 8 * SENT, None, None)
    assert rc == 0, L.rf_amd_last_error()
    torch.cuda.synchronize()
    assert inner(d_runs, 1, "d_num_branches")[0] == 0
    assert inner(d_boff, 3, "d_branch_off").tolist() == [0, -7, -7]


# ---- caps and grids ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """BIG uniform records over 300 members and their keys, made once and read-only"""
    rng = np.random.default_rng(42)
    cand = uniform(BIG, 300, rng)
    keys = np.sort(rng.integers(0, 1 << 50, size=BIG, dtype=np.uint64))
    cand.setflags(write=False)
    keys.setflags(write=False)
    return cand, keys


def test_count_above_cap(big):
    cand, keys = big
    for cap in (2 * TILE + 5, 1, TILE):
        run_case(cand, 300, ("count above cap", cap), count=BIG + 1000, cap=cap, keys=keys)
    run_case(cand, 300, "count 2^40", count=1 << 40, cap=BIG, keys=keys)


def test_count_far_below_cap(big):
    """cap of 40 tiles and 100 live records: the grid is sized from cap, and every tile but the
    first does nothing"""
    cand, keys = big
    cap = 40 * TILE
    pad = np.full(cap, np.uint64(0xFFFFFFFFFFFFFFFF))
    pad[:BIG] = cand
    kpad = np.zeros(cap, dtype=np.uint64)
    kpad[:BIG] = keys
    for count in (100, TILE + 1):
        run_case(pad, 300, ("count below cap", count), count=count, cap=cap, keys=kpad)


def test_branch_cap(big):
    cand, keys = big
    runs = len(E.found_by_branch_host(cand, 300)[2])
    assert runs > 2 * TILE  # the heads of more than one tile
    for bc in (0, 1, runs - 1, runs, runs + 9, runs // 2):
        got = run_case(cand, 300, ("branch_cap", bc), branch_cap=bc, keys=keys)
        assert got[4] == runs
    got = run_case(cand, 300, "branch_cap 0, NULL table", branch_cap=0, null_branch=True, keys=keys)
    assert got[4] == runs and got[2] is None


def test_without_order_key(big):
    cand, keys = big
    for nm in (3, 300):  # the single pass is the first and the last
        got = run_case(cand, nm, ("no keys", nm), with_key=False, keys=keys)
        assert got[1] is None


@pytest.mark.parametrize("blocks", [1, 3])
def test_grid_stride_loops(big, blocks):
    """four tiles on one and on three workgroups: every tile loop runs more than once"""
    cand, keys = big
    try:
        E.diag_fanout_max_blocks(blocks)
        for nm in (3, 300, BOUNDS[-1] + 1):
            run_case(cand, nm, (blocks, nm), keys=keys)
        run_case(own_branch(BIG, 1 << 20, np.random.default_rng(blocks)), 1 << 20, (blocks, "own"))
    finally:
        E.diag_fanout_max_blocks(0)


@pytest.mark.parametrize("blocks", [0, 3])
def test_several_scan_chunks(blocks):
    """a pass's 256 counts per tile are scanned in chunks of 8,192, the counts of 32 tiles: record
    counts that fill one chunk exactly, start a second and reach into a third, on the full grid
    and on three workgroups"""
    rng = np.random.default_rng(5 + blocks)
    try:
        E.diag_fanout_max_blocks(blocks)
        for m in (32 * TILE, 32 * TILE + 1, 65 * TILE + 3):
            for nm in (3, 300):
                run_case(uniform(m, nm, rng), nm, ("chunks", blocks, m, nm))
        run_case(own_branch(65 * TILE + 3, 1 << 20, rng), 1 << 20, ("chunks", blocks, "own"))
    finally:
        E.diag_fanout_max_blocks(0)


def test_two_runs_give_identical_bytes(big):
    cand, keys = big
    d_cand, d_keys = dev(cand), dev(keys)
    runs = len(E.found_by_branch_host(cand, 300)[2])
    a = raw_call(d_cand, d_keys, BIG, BIG, 300, runs)
    b = raw_call(d_cand, d_keys, BIG, BIG, 300, runs)
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()
    assert a[4] == b[4]


def test_stable_within_a_branch(big):
    """within one run d_order ascends: the records keep the batch's key order"""
    cand, keys = big
    order, okey, branch, boff, runs = run_case(cand, 300, "stable", keys=keys)
    inside = np.ones(BIG, dtype=bool)
    inside[boff[:runs].astype(np.int64)] = False
    d = np.diff(order.astype(np.int64), prepend=-1)
    assert (d[inside] > 0).all()
    assert (np.diff(okey.astype(np.int64), prepend=0)[inside] >= 0).all()
    assert sorted(order.tolist()) == list(range(BIG))


# ---- the Python call and the refusals ----------------------------------------------------------
def test_python_call(big):
    cand, keys = big
    want = E.found_by_branch_host(cand, 300, keys)
    runs = len(want[2])
    d_order = torch.empty(BIG, dtype=torch.int32, device="cuda:0")
    d_okey = torch.empty(BIG, dtype=torch.int64, device="cuda:0")
    d_branch = torch.empty(runs, dtype=torch.int64, device="cuda:0")
    d_boff = torch.empty(runs + 1, dtype=torch.int64, device="cuda:0")
    d_runs = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    E.found_by_branch(dev(cand), dev(keys), dev(np.array([BIG], dtype=np.uint64)), BIG, 300, d_order, d_okey,
                      d_branch, d_boff, runs, d_runs)
    torch.cuda.synchronize()
    got = (d_order.cpu().numpy().view(np.uint32), d_okey.cpu().numpy().view(np.uint64),
           d_branch.cpu().numpy().view(np.uint64), d_boff.cpu().numpy().view(np.uint64))
    assert int(d_runs.item()) == runs and all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
    with pytest.raises(ValueError):
        E.found_by_branch(dev(cand), dev(keys), d_runs, BIG, 300, d_order[:8], d_okey, d_branch, d_boff, runs, d_runs)


def test_errors(big):
    cand, keys = big
    L = E.load_library()
    h = E.default_engine().h
    B = E.STATUS_BAD_PARAM
    t = {k: torch.zeros(n, dtype=torch.int64, device="cuda:0")
         for k, n in (("order", BIG), ("okey", BIG), ("branch", 16), ("boff", 17), ("runs", 1), ("count", 1))}
    t["scr"] = torch.zeros(E.found_by_branch_scratch_bytes(BIG, 300) // 8, dtype=torch.int64, device="cuda:0")
    t["cand"], t["key"] = dev(cand), dev(keys)
    p = {k: v.data_ptr() for k, v in t.items()}

    def call(e=h, c=p["cand"], k=p["key"], n=p["count"], cap=BIG, nm=300, o=p["order"], ok=p["okey"],
             b=p["branch"], bo=p["boff"], bc=16, r=p["runs"], s=p["scr"]):
        return L.rf_amd_found_by_branch(e, c, k, n, cap, nm, o, ok, b, bo, bc, r, s, None)

    assert call() == 0
    assert call(e=None) == B and call(n=None) == B and call(r=None) == B
    assert call(nm=0) == B and call(nm=MAX_MEMBERS + 1) == B
    assert b"num_members" in L.rf_amd_last_error()
    assert call(cap=1 << 32) == B
    assert call(c=None) == B and call(o=None) == B and call(s=None) == B
    assert call(b=None) == B and call(bo=None) == B
    assert call(s=p["scr"] + 4) == B
    assert call(k=None) == B and call(ok=None) == B
    assert b"both or neither" in L.rf_amd_last_error()
    assert call(k=None, ok=None) == 0 and call(b=None, bo=None, bc=0) == 0
    assert call(c=None, k=None, o=None, ok=None, s=None, cap=0) == 0
    torch.cuda.synchronize()


# ---- in the world of the multi-get -------------------------------------------------------------
def test_group_by_branch_end_to_end(world, routed):  # noqa: F811
    """multiget_routed_per_key then group_by_branch: the mirror applied to the oracle's records,
    and per run the (key, member, value) of the reference's lookups"""
    w, r = world, routed
    rg, off, member, total = r.host["keys"]
    pairs = RR.want_pairs(r.words["keys"], off, member)
    _, cand, cand_key = E.found_per_key_host(pairs, member, off)
    assert len(cand) > 16
    want = E.found_by_branch_host(cand, w.set.num_members, cand_key)
    # the reference's lookups, pair by pair: key i found value v in member id
    pair_key = np.repeat(np.arange(N), np.diff(off.astype(np.int64)))
    lookups = {}
    for p in np.flatnonzero(pairs):
        for v in range(64):
            if (int(pairs[p]) >> v) & 1:
                lookups.setdefault((int(member[p]), v), []).append(int(pair_key[p]))
    assert len(lookups) == len(want[2]) > 1
    rmap = E.RangeMap(*r.table["keys"])
    per_key = w.set.multiget_routed_per_key(rmap, *RR.routed_inputs(w, r, "keys"), N)
    for bc in (1, None):  # 1: too small, the number of runs is the true one and the call runs again
        if bc is None:
            d_order, d_okey, d_branch, d_boff, runs = w.set.group_by_branch(per_key)
        else:
            d_order, d_okey, d_branch, d_boff, runs = w.set._group_by_branch(per_key, None, bc)
        got = (d_order.cpu().numpy().view(np.uint32), d_okey.cpu().numpy().view(np.uint64),
               d_branch.cpu().numpy().view(np.uint64), d_boff.cpu().numpy().view(np.uint64))
        assert runs == len(want[2])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want)), bc
        seen = {}
        for u in range(runs):
            b = int(got[2][u])
            seen[(b >> 8, b & 0xFF)] = sorted(got[1][int(got[3][u]):int(got[3][u + 1])].tolist())
        assert seen == {k: sorted(v) for k, v in lookups.items()}
    rmap.close()


def test_group_by_branch_without_records(world):  # noqa: F811
    """a batch of keys that no member holds: no records, no runs, d_branch_off == [0]; on the
    current stream and on a raw stream handle, and for a per-key result made with cap 0"""
    w = world
    member = np.full(N, len(w.members) + 1, dtype=np.uint32)  # an id past the end finds nothing
    per_key = w.set.multiget_per_key(dev(w.pk), 24, dev(member), 1, N)
    assert per_key[2] == 0 and per_key[1].numel() > 0
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    empty = (per_key[0], per_key[1][:0], 0, per_key[3][:0])
    for pk, stream in ((per_key, None), (per_key, side.cuda_stream), (empty, None)):
        d_order, d_okey, d_branch, d_boff, runs = w.set.group_by_branch(pk, stream=stream)
        assert runs == 0 and d_order.numel() == 0 and d_okey.numel() == 0 and d_branch.numel() == 0
        assert d_order.dtype == torch.int32 and d_boff.cpu().tolist() == [0]
