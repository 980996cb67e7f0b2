"""The key-aware compaction: rf_amd_found_per_key / _ragged (k_per_key_count, k_range_scan,
k_per_key_emit) and FilterSet.multiget_*_per_key. The oracle of every buffer is the host mirror
(E.found_per_key_host, checked against the consumer's loop in test_found_per_key_host.py):
d_key_off, *d_count, d_cand below min(total, cap) and d_cand_key must equal it exactly, and every
output lies between sentinel words that must stay as they were. The calls work on any words, so
most cases are synthetic and need no filter; the end-to-end tests run in test_gpu_multiget's world
and compare with the mirror applied to the oracle's routing_filter_lookup words."""
from types import SimpleNamespace

import numpy as np
import pytest

import test_gpu_multiget as MG
import test_gpu_range_route as RR
from splinterdb_amd import engine as E
from test_gpu_multiget import world  # noqa: F401  (the fixture; a fresh instance for this module)
from test_gpu_range_route import routed  # noqa: F401  (keys and oracle words of both key forms)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = MG.N  # 64 * 37 + 13
SENT = 512
TILE = E.diag_per_key_tile()
N_TILES = 3 * TILE + 77  # three whole tiles and a partial one
FIRST = 1000             # d_member_off[0] of every ragged case
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
WORDS = np.array([0, 1, 1 << 63, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
IDS = np.array([0, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)
PLACED = {10: 1, 11: 63, 12: 64, 13: 65, 14: 128, 15: 300, 500: 65535}  # key -> list length
FULL_KEY = 15  # every word of its 300 pairs all ones: 19,200 records over many steps


def dev(a):
    """a host array on the device; unsigned words travel as the signed type of their width"""
    a = np.array(a)  # a writable copy: the cases' arrays are read-only
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return MG.dev(a if signed is None else a.view(signed))


def rand_words(rng, m):
    """a sixth each of 0, 1, 1 << 63, all ones and random words of density 1/64 and 1/2"""
    kind = rng.integers(0, 6, size=m)
    w = WORDS[np.minimum(kind, 3)].copy()
    sparse = np.packbits(rng.random((m, 64)) < 1 / 64, axis=1, bitorder="little").view(np.uint64).reshape(-1)
    w[kind == 4] = sparse[kind == 4]
    w[kind == 5] = rng.integers(0, 1 << 64, size=m, dtype=np.uint64)[kind == 5]
    return w


def rand_ids(rng, m):
    ids = rng.integers(0, 1 << 32, size=m, dtype=np.uint64).astype(np.uint32)
    pick = rng.random(m) < 0.3
    ids[pick] = IDS[rng.integers(0, len(IDS), size=int(pick.sum()))]
    return ids


def make_case(n, seed):
    """n keys' lists from pair FIRST on: lengths 0-9 and the PLACED ones, empty lists at key 0 and
    n - 1, a whole wave of them (192..255) and a run across a wave boundary (256..330); the words
    of the second tile all zero; all-ones words and ids below the first and above the last pair"""
    rng = np.random.default_rng(seed)
    c = SimpleNamespace(n=n)
    cnt = rng.integers(0, 10, size=n)
    for k, ln in PLACED.items():
        cnt[k] = ln
    cnt[0] = cnt[n - 1] = 0
    cnt[192:331] = 0
    cnt[191] = cnt[331] = 2
    cnt[n - 2] = 3
    c.off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(cnt.astype(np.uint64), out=c.off[1:])
    c.off += np.uint64(FIRST)
    last = int(c.off[n])
    c.found = np.full(last + FIRST, ONES, dtype=np.uint64)
    c.member = np.full(last + FIRST, 0xFFFFFFFF, dtype=np.uint32)
    c.found[FIRST:last] = rand_words(rng, last - FIRST)
    c.member[FIRST:last] = rand_ids(rng, last - FIRST)
    c.found[int(c.off[FULL_KEY]):int(c.off[FULL_KEY + 1])] = ONES
    c.found[int(c.off[TILE]):int(c.off[2 * TILE])] = 0
    c.found[last - 1] = ONES  # cap = total - 1 falls inside this word's records
    c.want = E.found_per_key_host(c.found, c.member, c.off)
    c.total = int(c.want[0][-1])
    c.d_found, c.d_member, c.d_off = dev(c.found), dev(c.member), dev(c.off)
    for a in (c.found, c.member, c.off, *c.want):
        a.setflags(write=False)
    return c


@pytest.fixture(scope="module")
def cases():
    """the two ragged cases and their answers, made once and read-only"""
    return {N: make_case(N, 1), N_TILES: make_case(N_TILES, 2)}


def sentinel_buf(k):
    return torch.full((SENT + k + SENT,), -7, dtype=torch.int64, device="cuda:0")


def inner(buf, k, what):
    a = buf.cpu().numpy()
    assert (a[:SENT] == -7).all() and (a[SENT + k:] == -7).all(), "wrote outside " + what
    return a[SENT:SENT + k]


def raw_call(n, cap, fixed=None, ragged=None, null_cand=False, with_key=True):
    """one call through the C ABI on outputs between sentinels. fixed = (d_found, d_member or
    None, K); ragged = (d_found, d_member, d_member_off) as the probe took them. Returns
    (key_off uint64[n + 1], cand uint64[cap] or None, cand_key int64[cap] or None, count)."""
    L = E.load_library()
    d_key_off, d_count = sentinel_buf(n + 1), sentinel_buf(1)
    d_cand = None if null_cand else sentinel_buf(cap)
    d_cand_key = sentinel_buf(cap) if with_key and not null_cand else None
    scratch = torch.empty(E.found_per_key_scratch_bytes(n) // 8, dtype=torch.int64, device="cuda:0")
    out = (n, d_key_off.data_ptr() + 8 * SENT, None if d_cand is None else d_cand.data_ptr() + 8 * SENT,
           None if d_cand_key is None else d_cand_key.data_ptr() + 8 * SENT, cap, d_count.data_ptr() + 8 * SENT,
           scratch.data_ptr(), None)
    if fixed is not None:
        rc = L.rf_amd_found_per_key(E.default_engine().h, E._dptr(fixed[0]), E._dptr(fixed[1]), fixed[2], *out)
    else:
        rc = L.rf_amd_found_per_key_ragged(E.default_engine().h, *(E._dptr(x) for x in ragged), *out)
    assert rc == 0, L.rf_amd_last_error()
    torch.cuda.synchronize()
    return (inner(d_key_off, n + 1, "d_key_off").view(np.uint64),
            None if d_cand is None else inner(d_cand, cap, "d_cand[0, cap)").view(np.uint64),
            None if d_cand_key is None else inner(d_cand_key, cap, "d_cand_key[0, cap)"),
            int(inner(d_count, 1, "d_count")[0]))


def check(got, want, cap, what):
    key_off, cand, cand_key, count = got
    w_off, w_cand, w_key = want
    total = int(w_off[-1])
    assert count == total, (what, "count", count, total)
    assert (key_off == w_off).all(), (what, "offsets", np.flatnonzero(key_off != w_off)[:8])
    k = min(cap, total)
    if cand is not None:
        bad = np.flatnonzero(cand[:k] != w_cand[:k])
        assert bad.size == 0, (what, "records", bad.size, bad[:8].tolist(), cand[bad[:4]], w_cand[bad[:4]])
        assert (cand[k:].view(np.int64) == -7).all(), (what, "wrote past the records")
    if cand_key is not None:
        bad = np.flatnonzero(cand_key[:k] != w_key[:k])
        assert bad.size == 0, (what, "keys", bad.size, bad[:8].tolist())
        assert (cand_key[k:] == -7).all(), (what, "wrote past the records' keys")


def ragged_args(c, a=0):
    """the call over the keys from a on: the probe's d_found and d_member, the offsets from a"""
    return c.d_found, c.d_member, c.d_off[a:]


# ---- the cases say what they claim -----------------------------------------------------------
def test_placed_cases_exist(cases):
    c = cases[N]
    cnt = np.diff(c.off.astype(np.int64))
    assert {0, 1, 63, 64, 65, 128, 300, 65535} <= set(cnt.tolist())
    assert cnt[0] == 0 and cnt[-1] == 0 and (cnt[192:331] == 0).all() and cnt[191] > 0 and cnt[331] > 0
    live = c.found[FIRST:int(c.off[-1])]
    assert set(WORDS.tolist()) <= set(live.tolist())
    pop = np.array([bin(int(x)).count("1") for x in live[:4000]])
    assert (pop == 1).sum() > 400 and (pop == 2).sum() > 20 and ((pop > 20) & (pop < 44)).sum() > 300
    assert set(IDS.tolist()) <= set(c.member[FIRST:int(c.off[-1])].tolist())
    key_off = c.want[0].astype(np.int64)
    assert key_off[FULL_KEY + 1] - key_off[FULL_KEY] == 300 * 64
    assert key_off[2 * TILE] == key_off[TILE] and c.off[2 * TILE] - c.off[TILE] > TILE  # a tile of zero words
    assert int(c.off[0]) == FIRST and (c.found[:FIRST] == ONES).all() and (c.found[int(c.off[-1]):] == ONES).all()
    assert c.want[2][-1] == N - 2 and c.want[2][-2] == N - 2  # the last word has more than one record
    assert N > 2 * TILE and N_TILES > 3 * TILE and N_TILES % TILE
    assert (c.want[1] >> np.uint64(8)).max() == 0xFFFFFFFF  # an id's top bit survives the shift


# ---- the ragged form ---------------------------------------------------------------------------
def test_ragged(cases):
    c = cases[N]
    check(raw_call(c.n, c.total, ragged=ragged_args(c)), c.want, c.total, "ragged")


@pytest.mark.parametrize("n,a", [(1, 15), (1, 0), (63, 190), (64, 192), (65, 191), (64, 500 - 63), (65, 0)])
def test_small_n(cases, n, a):
    """n keys from key a of the larger case: a sub-range of its CSR, d_member_off[0] wherever key
    a's list starts -- the whole wave of empty lists, the longest list as a row's last key"""
    c = cases[N]
    want = E.found_per_key_host(c.found, c.member, c.off[a:a + n + 1])
    total = int(want[0][-1])
    check(raw_call(n, total + 8, ragged=ragged_args(c, a)), want, total + 8, (n, a))


def test_n_zero(cases):
    c = cases[N]
    key_off, cand, cand_key, count = raw_call(0, 8, ragged=ragged_args(c))
    assert key_off.tolist() == [0] and count == 0
    assert (cand.view(np.int64) == -7).all() and (cand_key == -7).all()
    key_off, cand, cand_key, count = raw_call(0, 8, fixed=(None, None, 4))
    assert key_off.tolist() == [0] and count == 0 and (cand.view(np.int64) == -7).all()


@pytest.mark.parametrize("blocks", [1, 2])
def test_grid_stride_loops(cases, blocks):
    """three tiles (and four) on one and two workgroups: every loop of both kernels runs more than
    once in a workgroup"""
    try:
        E.diag_fanout_max_blocks(blocks)
        for n in (N, N_TILES):
            c = cases[n]
            check(raw_call(c.n, c.total, ragged=ragged_args(c)), c.want, c.total, (blocks, n))
        w = cases[N].found[FIRST:FIRST + N_TILES * 4]
        check(raw_call(N_TILES, 100000, fixed=(dev(w), None, 4)), E.found_per_key_host_fixed(w, None, 4), 100000,
              (blocks, "fixed"))
    finally:
        E.diag_fanout_max_blocks(0)


def test_several_tiles(cases):
    c = cases[N_TILES]
    check(raw_call(c.n, c.total, ragged=ragged_args(c)), c.want, c.total, "tiles")


def test_cap(cases):
    """the offsets and *d_count are the true values whatever cap is; nothing at or past cap"""
    c = cases[N]
    assert c.total > 20000
    for cap in (1, c.total - 1, c.total, c.total + 512, c.total // 2):
        check(raw_call(c.n, cap, ragged=ragged_args(c)), c.want, cap, ("cap", cap))
    check(raw_call(c.n, 0, ragged=ragged_args(c), null_cand=True), c.want, 0, "cap 0, NULL d_cand")


def test_no_cand_key(cases):
    c = cases[N]
    got = raw_call(c.n, c.total, ragged=ragged_args(c), with_key=False)
    assert got[2] is None
    check(got, c.want, c.total, "NULL d_cand_key")


def test_two_runs_give_identical_bytes(cases):
    c = cases[N]
    a = raw_call(c.n, c.total + 100, ragged=ragged_args(c))
    b = raw_call(c.n, c.total + 100, ragged=ragged_args(c))
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    assert a[3] == b[3]


def test_agrees_with_found_compact(cases):
    """record j here and record j of rf_amd_found_compact on the same words: the same value, and
    the id of that record's pair"""
    c = cases[N]
    m = int(c.off[-1]) - FIRST
    d_cand = torch.empty(c.total, dtype=torch.int64, device="cuda:0")
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    E.found_compact(c.d_found[FIRST:], m, d_cand, d_count)
    torch.cuda.synchronize()
    assert int(d_count.item()) == c.total
    rec = d_cand.cpu().numpy().view(np.uint64)
    _, cand, _, _ = raw_call(c.n, c.total, ragged=ragged_args(c))
    assert (cand & np.uint64(0xFF) == rec & np.uint64(0xFF)).all()
    assert (cand >> np.uint64(8) == c.member[FIRST + (rec >> np.uint64(8)).astype(np.int64)]).all()


# ---- the fixed form ----------------------------------------------------------------------------
@pytest.mark.parametrize("with_member", [False, True], ids=["slots", "ids"])
@pytest.mark.parametrize("K", [1, 4, 16, 65])
def test_fixed(cases, K, with_member):
    c = cases[N]
    last = int(c.off[-1])
    w = np.resize(c.found[FIRST:last], N * K)  # any words do: the live words of the ragged case, repeated
    member = np.resize(c.member[FIRST:last], N * K) if with_member else None
    want = E.found_per_key_host_fixed(w, member, K)
    total = int(want[0][-1])
    got = raw_call(N, total + 8, fixed=(dev(w), None if member is None else dev(member), K))
    check(got, want, total + 8, (K, with_member))
    if not with_member:
        assert (want[1] >> np.uint64(8)).max() == K - 1


# ---- the Python calls --------------------------------------------------------------------------
def test_python_calls(cases):
    c = cases[N]

    def outputs(cap):
        return (torch.empty(c.n + 1, dtype=torch.int64, device="cuda:0"),
                torch.empty(cap, dtype=torch.int64, device="cuda:0"),
                torch.empty(cap, dtype=torch.int64, device="cuda:0"),
                torch.zeros(1, dtype=torch.int64, device="cuda:0"))

    def host(o):
        torch.cuda.synchronize()
        return (o[0].cpu().numpy().view(np.uint64), o[1].cpu().numpy().view(np.uint64), o[2].cpu().numpy(),
                int(o[3].item()))

    o = outputs(c.total)
    E.found_per_key_ragged(c.d_found, c.d_member, c.d_off, c.n, *o)
    got = host(o)
    assert got[3] == c.total and all((x == y).all() for x, y in zip(got[:3], c.want))
    w = c.found[FIRST:FIRST + 4 * c.n]
    want = E.found_per_key_host_fixed(w, None, 4)
    o = outputs(int(want[0][-1]))
    E.found_per_key(dev(w), None, 4, c.n, *o)
    got = host(o)
    assert got[3] == int(want[0][-1]) and all((x == y).all() for x, y in zip(got[:3], want))


def test_errors(cases):
    c = cases[N]
    L = E.load_library()
    n = c.n
    ko = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
    cand = torch.zeros(c.total, dtype=torch.int64, device="cuda:0")
    key = torch.zeros(c.total, dtype=torch.int64, device="cuda:0")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    scr = torch.zeros(E.found_per_key_scratch_bytes(n) // 8, dtype=torch.int64, device="cuda:0")
    p = SimpleNamespace(f=c.d_found.data_ptr(), m=c.d_member.data_ptr(), o=c.d_off.data_ptr(), ko=ko.data_ptr(),
                        c=cand.data_ptr(), k=key.data_ptr(), t=cnt.data_ptr(), s=scr.data_ptr())
    h = E.default_engine().h
    B = E.STATUS_BAD_PARAM

    def ragged(e=h, f=p.f, m=p.m, o=p.o, n=n, ko=p.ko, cc=p.c, k=p.k, cap=c.total, t=p.t, s=p.s):
        return L.rf_amd_found_per_key_ragged(e, f, m, o, n, ko, cc, k, cap, t, s, None)

    def fixed(e=h, f=p.f + 8 * FIRST, m=p.m + 4 * FIRST, K=4, n=n, ko=p.ko, cc=p.c, k=p.k, cap=c.total, t=p.t, s=p.s):
        return L.rf_amd_found_per_key(e, f, m, K, n, ko, cc, k, cap, t, s, None)

    assert ragged() == 0 and fixed() == 0
    assert ragged(e=None) == B and fixed(e=None) == B
    assert ragged(n=1 << 56) == B and fixed(n=1 << 56) == B
    assert ragged(ko=None) == B and ragged(t=None) == B and fixed(ko=None) == B and fixed(t=None) == B
    assert ragged(f=None) == B and ragged(s=None) == B and fixed(f=None) == B and fixed(s=None) == B
    assert ragged(m=None) == B and ragged(o=None) == B
    assert ragged(cc=None) == B and fixed(cc=None) == B
    assert b"candidate" in L.rf_amd_last_error()
    assert fixed(K=0) == B and fixed(K=65536) == B
    assert ragged(s=p.s + 4) == B
    assert ragged(cc=None, k=None, cap=0) == 0 and fixed(cc=None, k=None, cap=0) == 0
    assert fixed(m=None) == 0 and ragged(k=None) == 0 and fixed(k=None) == 0
    assert ragged(n=0, f=None, m=None, o=None, s=None) == 0 and fixed(n=0, f=None, m=None, s=None) == 0
    torch.cuda.synchronize()


# ---- in the world of the multi-get -------------------------------------------------------------
NM = RR.NM


def table_65(rng, keys):
    """65 ranges cut by 64 of the probe keys, lists over ids 0-7 (the None member and two ids
    past the end among them), one with every id"""
    bounds = sorted(set(keys[i] for i in rng.permutation(len(keys))[:200]))[:64]
    assert len(bounds) == 64
    lists = [rng.integers(0, NM + 2, size=rng.integers(0, 10)).tolist() for _ in range(65)]
    lists[3] = list(range(NM + 2))
    return bounds, lists


def check_multiget(got, want, cap):
    d_key_off, d_cand, count, d_cand_key = got
    total = int(want[0][-1])
    assert count == total, (cap, count, total)
    assert (d_key_off.cpu().numpy().view(np.uint64) == want[0]).all(), cap
    assert d_cand.numel() >= count and d_cand_key.numel() >= count
    assert (d_cand[:count].cpu().numpy().view(np.uint64) == want[1]).all(), cap
    assert (d_cand_key[:count].cpu().numpy() == want[2]).all(), cap


@pytest.mark.parametrize("form", ["keys", "var"])
def test_multiget_routed_per_key(world, routed, form):  # noqa: F811
    w, r = world, routed
    keys = r.keys if form == "keys" else r.vkeys
    bounds, lists = table_65(np.random.default_rng(65), keys)
    rg, off, member, total = E.range_route_host(bounds, lists, keys)
    assert (member == 2).any() and (member >= NM).any() and total > N
    want = E.found_per_key_host(RR.want_pairs(r.words[form], off, member), member, off)
    assert len(want[1]) > 16
    rmap = E.RangeMap(bounds, lists)
    assert rmap.num_ranges == 65
    fn = w.set.multiget_routed_per_key if form == "keys" else w.set.multiget_var_routed_per_key
    for cap in (16, len(want[1]), None):  # 16: too small, the count is the total and the second pass runs
        check_multiget(fn(rmap, *RR.routed_inputs(w, r, form), N, cap=cap), want, cap)
    # the same CSR through the ragged form, its offsets starting at 0
    if form == "keys":
        got = w.set.multiget_ragged_per_key(dev(w.pk), 24, dev(member), dev(off), N)
    else:
        got = w.set.multiget_var_ragged_per_key(*RR.routed_inputs(w, r, form), dev(member), dev(off), N)
    check_multiget(got, want, "ragged")
    rmap.close()


def test_multiget_per_key_fixed(world, routed):  # noqa: F811
    w, r = world, routed
    member = np.random.default_rng(4).integers(0, NM + 2, size=(N, 4)).astype(np.uint32)
    want = E.found_per_key_host_fixed(MG.want_words(w, "keys", member), member.reshape(-1), 4)
    assert len(want[1]) > 16
    for cap in (16, None):
        check_multiget(w.set.multiget_per_key(dev(w.pk), 24, dev(member.reshape(-1)), 4, N, cap=cap), want, cap)
    got = w.set.multiget_var_per_key(*RR.routed_inputs(w, r, "var"), dev(member.reshape(-1)), 4, N)
    vwords = r.words["var"]
    ok = member < NM
    vw = np.where(ok, vwords[np.where(ok, member, 0), np.arange(N)[:, None]], np.uint64(0)).reshape(-1)
    check_multiget(got, E.found_per_key_host_fixed(vw, member.reshape(-1), 4), "var")
    # every member, the id being the slot
    want = E.found_per_key_host_fixed(MG.want_words(w, "keys", None), None, len(w.members))
    check_multiget(w.set.multiget_per_key(dev(w.pk), 24, None, len(w.members), N), want, "all members")
