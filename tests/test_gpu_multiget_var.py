"""The multi-get and the grouped probe for variable-length keys: rf_amd_filter_set_probe_var_keys
(k_probe_fanout<IN_VAR>: the wave's keys through wave_hash_var's 4 KiB LDS window),
FilterSet.multiget_var, rf_amd_batch_probe_var_keys_runs and rf_amd_filter_lookup_var_keys.
The reference is the CPU oracle throughout: rfo_hash_var of the keys, then routing_filter_lookup
(src/routing_filter.c:985-1073) of every member, and every word must be equal. Outputs are
pre-filled with -7 and carry a sentinel tail; the key bytes lie between 0xEE bytes, so a hash
that read outside its key differs. rf_amd_diag_fanout_max_blocks caps the fan-out's grid so
that the kernel's grid-stride loop runs, for the fixed-length kinds and the hashes as well."""
from types import SimpleNamespace

import numpy as np
import pytest

from splinterdb_amd import engine as E
from splinterdb_amd import keys as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = 64 * 37 + 13
SENT = 4096
PAD = 64  # 0xEE bytes before and after the key bytes (a multiple of 16: `shift` is the alignment)
GIANTS = (4081, 4082, 4096, 5000, 9000)  # both sides of "fits the 4 KiB window", and straight from global
PROFILES = {"a": (8, 100), "b": (0, 15), "c": (200, 300), "d": (8, 100)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def rand_keys(rng, lens):
    """random key bytes of the given lengths as (bytes, n + 1 offsets)"""
    offs = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(lens, dtype=np.uint64), out=offs[1:])
    return rng.integers(0, 256, size=int(offs[-1]), dtype=np.uint8), offs


def pool_lens(rng, n, giants=False):
    """a member's key lengths: 60 % 8-100, 20 % 0-15, 20 % 200-300, so that every probe profile
    finds own keys of its lengths; giants: the last five are GIANTS"""
    c = rng.random(n)
    lens = np.where(c < 0.6, rng.integers(8, 101, size=n),
                    np.where(c < 0.8, rng.integers(0, 16, size=n), rng.integers(200, 301, size=n)))
    if giants:
        lens[-len(GIANTS):] = GIANTS
    return lens


def concat_pools(pools):
    """several (bytes, offsets) pairs as one, and each one's first key number"""
    first, base, datas, offs = [], 0, [], []
    for d, o in pools:
        first.append(sum(len(x) for x in offs))
        datas.append(d)
        offs.append(o[:-1] + np.uint64(base))
        base += int(o[-1])
    return np.concatenate(datas), np.concatenate(offs + [np.array([base], dtype=np.uint64)]), first


def clustered_hashes(rng, fps, lis, n):
    """test_gpu_multiget's overflowing filter: 16 clusters of 150 fingerprints in 4 neighbouring
    buckets, so their probe lines overflow and lookups walk the image"""
    lnb = max(int(n).bit_length() - 1, lis)
    rem, sh = fps - lnb, 32 - fps
    h = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    k = 0
    for c in range(16):
        b0 = int(rng.integers(0, (1 << lnb) - 4))
        for j in range(150):
            fp = ((b0 + j % 4) << rem) | (j * 7919 % (1 << rem))
            h[k] = np.uint32((fp << sh) | (j & ((1 << sh) - 1)))
            k += 1
    return h, k, 32 - lnb


def giant_places(n):
    """(position, length) of profile d's long keys among n keys (n % 64 != 0): every length in
    lane 0, in lane 63, mid-wave and in the last, partial wave"""
    last = n // 64 * 64
    assert n % 64 >= len(GIANTS) and last >= 64 * 12
    out = []
    for j, ln in enumerate(GIANTS):
        out += [(64 * (1 + 2 * j), ln), (64 * (2 + 2 * j) + 63, ln), (64 * (1 + 2 * j) + 29 + j, ln), (last + j, ln)]
    return out


def make_probes(w, oracle, rng, name, n):
    """n probe keys of a length profile: the first third members' own keys of those lengths
    (A1's and B's twice-added ones, alternating), then keys whose hashes fall into D's
    clustered buckets (lengths 8-15: not in profile c), the rest fresh; profile d = a with
    GIANTS placed by giant_places, those in lane 0 and mid-wave being A1's own keys"""
    lo, hi = PROFILES[name]
    lens = rng.integers(lo, hi + 1, size=n)
    if name == "b":
        lens[rng.random(n) < 0.12] = 0
    fresh = rand_keys(rng, lens)
    fresh_giants = rand_keys(rng, [ln for _, ln in giant_places(n)])
    data, offs, (fA, fB, fF, fD, fG) = concat_pools([w.poolA, w.poolB, fresh, w.nearD, fresh_giants])
    ids = fF + np.arange(n, dtype=np.int64)
    third = n // 3
    lenA, lenB = np.diff(w.poolA[1]).astype(np.int64), np.diff(w.poolB[1]).astype(np.int64)
    ownA = 5000 + np.flatnonzero((lenA[5000:] >= lo) & (lenA[5000:] <= hi))  # A1's
    ownB = np.flatnonzero((lenB[:100000] >= lo) & (lenB[:100000] <= hi))    # B's twice-added
    ids[0:third:2] = fA + rng.choice(ownA, size=len(ids[0:third:2]))
    ids[1:third:2] = fB + rng.choice(ownB, size=len(ids[1:third:2]))
    if name != "c":
        nd = min(100, n // 8, len(w.nearD[1]) - 1)
        ids[third:third + nd] = fD + np.arange(nd)
    if name == "d":
        for j, (pos, ln) in enumerate(giant_places(n)):
            own = j % 4 in (0, 2)
            ids[pos] = fA + 75000 - len(GIANTS) + GIANTS.index(ln) if own else fG + j
    pdata, poffs = K.gather_var(data, offs, ids)
    p = SimpleNamespace(name=name, n=n, data=pdata, offs=poffs)
    plen = np.diff(poffs).astype(np.int64)
    if name == "d":
        assert all(plen[pos] == ln for pos, ln in giant_places(n))
    else:
        assert plen.min() >= lo and plen.max() <= hi
    if name == "b":
        assert (plen == 0).mean() >= 0.05
    if name == "c":
        assert plen[:64].sum() > 3 * 4096  # a wave's keys refill the window several times
    p.h = oracle.hash_var(pdata, poffs)
    p.words = member_words(w.ofs, p.h)
    p.words.setflags(write=False)
    return p


def member_words(ofs, h):
    return np.stack([of.lookup_hashes(h) if of is not None else np.zeros(len(h), dtype=np.uint64) for of in ofs])


def dev_var(data, offs, shift=0, first=0):
    """the keys in device memory between 0xEE bytes: the bytes pointer (`shift` bytes off a
    16-byte boundary; the keys start `first` bytes after it) and the offsets"""
    buf = np.full(PAD + shift + first + len(data) + PAD, 0xEE, dtype=np.uint8)
    at = PAD + shift + first
    buf[at:at + len(data)] = data
    t = dev(buf)
    assert t.data_ptr() % 16 == 0
    return t[PAD + shift:], dev((offs + np.uint64(first)).view(np.int64))


@pytest.fixture(scope="module")
def world(oracle):
    """batches A-D built from variable-length keys (D from clustered hashes), their oracle
    filters, the set (A0, A1, None, B0, C0, D0), and per length profile N probe keys with the
    oracle's words of every probe in every member; read-only"""
    rng = np.random.default_rng(2025)
    w = SimpleNamespace()
    cfg8, o8 = E.routing_config_init(log_index_size=8), oracle.make_config(log_index_size=8)
    cfg9, o9 = E.routing_config_init(log_index_size=9), oracle.make_config(log_index_size=9)

    def built(cfg, sizes, values, pool, old=None):
        b = E.FilterBatch(cfg, sizes, values, old=old)
        d_bytes, d_offs = dev_var(pool[0], pool[1][:sum(sizes) + 1])
        b.build_var_keys(d_bytes, d_offs)
        torch.cuda.synchronize()
        return b
    # A: two filters, values 0 and 5; A1 ends with the GIANTS
    w.poolA = rand_keys(rng, pool_lens(rng, 75000, giants=True))
    ha = oracle.hash_var(*w.poolA)
    w.A = built(cfg8, [5000, 70000], [0, 5], w.poolA)
    oA0, oA1 = oracle.filter_add(o8, ha[:5000], value=0), oracle.filter_add(o8, ha[5000:], value=5)
    w.imgA1 = w.A.image(1)
    # B: 200,001 keys with value 2, the first 100,000 again with value 7 (words with two bits)
    w.poolB = rand_keys(rng, pool_lens(rng, 200001))
    hb = oracle.hash_var(*w.poolB)
    w.B_old = built(cfg8, [200001], [2], w.poolB)
    w.B = built(cfg8, [100000], [7], w.poolB, old=[(w.B_old, 0)])
    oB = oracle.filter_add(o8, hb[:100000], value=7, old=oracle.filter_add(o8, hb, value=2))
    # C: log_index_size 9, value 63
    poolC = rand_keys(rng, pool_lens(rng, 1 << 17))
    w.C = built(cfg9, [1 << 17], [63], poolC)
    oC = oracle.filter_add(o9, oracle.hash_var(*poolC), value=63)
    # D: clustered hashes, overflowed probe lines; nearD: keys whose hashes fall into the
    # clusters' buckets, so the var form too reaches lines that cannot answer
    hd, kd, bsh = clustered_hashes(rng, 26, 8, 400000)
    w.D = E.FilterBatch(cfg8, [400000], [3])
    w.D.build_hashes(dev(hd))
    oD = oracle.filter_add(o8, hd, value=3)
    cand = rand_keys(rng, rng.integers(8, 16, size=1 << 20))
    hit = np.flatnonzero(np.isin(oracle.hash_var(*cand) >> np.uint32(bsh), np.unique(hd[:kd] >> np.uint32(bsh))))
    assert len(hit) >= 100
    w.nearD = K.gather_var(cand[0], cand[1], hit)
    torch.cuda.synchronize()
    w.cfg8, w.o8 = cfg8, o8
    w.ofs = [oA0, oA1, None, oB, oC, oD]
    w.members = [(w.A, 0), (w.A, 1), None, (w.B, 0), (w.C, 0), (w.D, 0)]
    w.set = E.FilterSet(w.members)
    w.prof = {name: make_probes(w, oracle, rng, name, N) for name in PROFILES}
    # fixed-length probes for the grid-stride test: the first third A1's own keys of that length
    w.fixed = {}
    lenA = np.diff(w.poolA[1]).astype(np.int64)
    for kl in (24, 17, 16):
        pk = rng.integers(0, 256, size=(N, kl), dtype=np.uint8)
        own = 5000 + np.flatnonzero(lenA[5000:] == kl)
        pick = rng.choice(own, size=N // 3)
        pk[:N // 3] = w.poolA[0][w.poolA[1][pick].astype(np.int64)[:, None] + np.arange(kl)]
        h = oracle.hash_fixed(pk.reshape(-1), kl)
        w.fixed[kl] = SimpleNamespace(keys=pk, h=h, words=member_words(w.ofs, h))
    # member ids of every K, ids past the end included
    w.member = {k: rng.integers(0, len(w.members) + 2, size=(N, k)).astype(np.uint32) for k in (1, 3, 5, 8)}
    yield w
    w.set.close()


def want_words(words, member, n=N, nm=6):
    """the oracle's word of every (key, slot) of the first n keys; member None: slot j is member j"""
    if member is None:
        return np.ascontiguousarray(words[:, :n].T).reshape(-1)
    member = member[:n]
    ok = member < nm
    return np.where(ok, words[np.where(ok, member, 0), np.arange(n)[:, None]], np.uint64(0)).reshape(-1)


def read_found(found, m):
    torch.cuda.synchronize()
    out = found.cpu().numpy()
    assert (out[m:] == -7).all(), "wrote past d_found[n * K)"
    return out[:m].view(np.uint64)


def run_var(w, p, member, k, n=N, shift=0, first=0, fset=None):
    found = torch.full((n * k + SENT,), -7, dtype=torch.int64, device="cuda:0")
    d_bytes, d_offs = dev_var(p.data[:int(p.offs[n])], p.offs[:n + 1], shift, first)
    dm = None if member is None else dev(member[:n].reshape(-1))
    (fset or w.set).probe_var_keys(d_bytes, d_offs, dm, k, n, found)
    return read_found(found, n * k)


def check(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, bad[:8].tolist(), got[bad[:4]], want[bad[:4]])


# ---- 1: the fan-out against the oracle -----------------------------------------------------
@pytest.mark.parametrize("name", list(PROFILES))
@pytest.mark.parametrize("k", [1, 3, 5, 8, None])
def test_fanout_var_vs_oracle(world, name, k):
    w, p = world, world.prof[name]
    member = None if k is None else w.member[k]
    kk = len(w.members) if k is None else k
    got = run_var(w, p, member, kk)
    check(got, want_words(p.words, member), (name, k))
    g2 = got.reshape(N, kk)
    if member is not None:
        assert (g2[member >= len(w.members)] == 0).all() and (member >= len(w.members)).any()
        assert (g2[member == 2] == 0).all() and (member == 2).any()  # the None member
    else:
        third = N // 3
        assert (g2[:, 2] == 0).all()
        plain = np.ones(N, dtype=bool)  # not one of profile d's long keys
        if name == "d":
            plain[[pos for pos, _ in giant_places(N)]] = False
        assert (g2[0:third:2, 1] >> np.uint64(5) & np.uint64(1))[plain[0:third:2]].all(), "A1's own keys not found"
        assert (g2[1:third:2, 3] & np.uint64(0x84) == np.uint64(0x84))[plain[1:third:2]].all(), \
            "B's twice-added keys: two bits"
        if name != "c":
            assert (g2[third:third + 100, 5] >> np.uint64(3) & np.uint64(1)).any(), "no probe of D found anything"
        if name == "d":
            own = [pos for j, (pos, _) in enumerate(giant_places(N)) if j % 4 in (0, 2)]
            assert (g2[own, 1] >> np.uint64(5) & np.uint64(1)).all(), "A1's long keys not found"


def test_world_reaches_overflowed_lines_and_zero_length_keys(world):
    w = world
    lines = w.D.debug_lines()
    assert (lines[:, :16] == 0xFF).all(axis=1).any(), "D has no overflowed probe line"
    assert (np.diff(w.prof["b"].offs) == 0).sum() >= N // 20


# ---- 2: base alignment and first offset ----------------------------------------------------
@pytest.mark.parametrize("shift,first", [(0, 0), (1, 0), (8, 0), (15, 0), (0, 37), (5, 37)])
def test_fanout_var_base_and_first_offset(world, shift, first):
    w, p = world, world.prof["d"]
    check(run_var(w, p, w.member[3], 3, shift=shift, first=first), want_words(p.words, w.member[3]), (shift, first))


# ---- 3: sizes ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, N])
def test_fanout_var_sizes(world, n):
    w, p = world, world.prof["a"]
    check(run_var(w, p, w.member[3], 3, n=n), want_words(p.words, w.member[3], n), n)
    check(run_var(w, p, None, 6, n=n), want_words(p.words, None, n), n)


def test_fanout_var_n_zero(world):
    w = world
    w.set.probe_var_keys(None, None, None, 6, 0, None)
    found = torch.full((SENT,), -7, dtype=torch.int64, device="cuda:0")
    d_bytes, d_offs = dev_var(w.prof["a"].data, w.prof["a"].offs)
    w.set.probe_var_keys(d_bytes, d_offs, dev(w.member[3].reshape(-1)), 3, 0, found)
    read_found(found, 0)


# ---- 4: agreement with the hashes form -----------------------------------------------------
@pytest.mark.parametrize("name", ["a", "d"])
def test_fanout_var_equals_hashes_form(world, name):
    w, p = world, world.prof[name]
    for member, kk in ((w.member[3], 3), (None, 6)):
        found = torch.full((N * kk + SENT,), -7, dtype=torch.int64, device="cuda:0")
        w.set.probe_hashes(dev(p.h), None if member is None else dev(member.reshape(-1)), kk, N, found)
        assert (run_var(w, p, member, kk) == read_found(found, N * kk)).all()


# ---- 6: multiget_var -----------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, None])
def test_multiget_var(world, k):
    w, p = world, world.prof["a"]
    member = None if k is None else w.member[k]
    kk = len(w.members) if k is None else k
    want = E.found_candidates(want_words(p.words, member))
    assert len(want) > 16
    d_bytes, d_offs = dev_var(p.data, p.offs)
    dm = None if member is None else dev(member.reshape(-1))
    for cap in (16, len(want), None):  # 16: too small, the second pass runs
        d_cand, count = w.set.multiget_var(d_bytes, d_offs, dm, kk, N, cap=cap)
        assert count == len(want)
        assert (d_cand[:count].cpu().numpy().view(np.uint64) == want).all()


# ---- 7: the grid-stride loop, every kind ---------------------------------------------------
@pytest.mark.parametrize("form", ["var", "keys24", "keys17", "keys16", "hashes"])
@pytest.mark.parametrize("blocks", [1, 2])
def test_fanout_grid_stride_loop(world, blocks, form):
    """2,381 keys on 1 or 2 workgroups of 4 waves: 10 or 5 chunks per wave"""
    w = world
    try:
        E.diag_fanout_max_blocks(blocks)
        for member, kk in ((w.member[3], 3), (None, 6)):
            dm = None if member is None else dev(member.reshape(-1))
            if form == "var":
                p = w.prof["c"]
                got, words = run_var(w, p, member, kk), p.words
            else:
                found = torch.full((N * kk + SENT,), -7, dtype=torch.int64, device="cuda:0")
                if form == "hashes":
                    p = w.prof["a"]
                    w.set.probe_hashes(dev(p.h), dm, kk, N, found)
                else:
                    p = w.fixed[int(form[4:])]
                    w.set.probe_keys(dev(p.keys), p.keys.shape[1], dm, kk, N, found)
                got, words = read_found(found, N * kk), p.words
            check(got, want_words(words, member), (blocks, form, kk))
            if member is None and form != "hashes":
                assert (got.reshape(N, kk)[:N // 3:2, 1] >> np.uint64(5) & np.uint64(1)).all()
    finally:
        E.diag_fanout_max_blocks(0)


# ---- 8: errors -----------------------------------------------------------------------------
def test_fanout_var_errors(world, oracle):
    w, p = world, world.prof["a"]
    found = torch.zeros(N * 8, dtype=torch.int64, device="cuda:0")
    d_bytes, d_offs = dev_var(p.data, p.offs)
    dm = dev(w.member[3].reshape(-1))

    def einval(fn):
        with pytest.raises(E.PlatformStatusError) as ei:
            fn()
        assert ei.value.code == E.STATUS_BAD_PARAM

    einval(lambda: w.set.probe_var_keys(d_bytes, d_offs, dm, 0, N, found))            # K == 0
    einval(lambda: w.set.probe_var_keys(d_bytes, d_offs, None, 5, N, found))          # all-members, K != 6
    einval(lambda: w.set.probe_var_keys(d_bytes, d_offs, dm, 3, (1 << 56) // 3 + 1, found))  # n K >= 2^56
    einval(lambda: w.set.probe_var_keys(None, d_offs, dm, 3, N, found))
    einval(lambda: w.set.probe_var_keys(d_bytes, None, dm, 3, N, found))
    einval(lambda: w.set.probe_var_keys(d_bytes, d_offs, dm, 3, N, None))
    # members hashed with different seeds: no var form, the hashes form works
    cfg7 = E.routing_config_init(log_index_size=8, seed=7)
    own = (p.data[:int(p.offs[1000])], p.offs[:1001])
    hs = oracle.hash_var(*own, seed=7)
    S = E.FilterBatch(cfg7, [1000], [9])
    S.build_var_keys(*dev_var(*own))
    torch.cuda.synchronize()
    mixed = E.FilterSet([(w.A, 1), (S, 0)])
    einval(lambda: mixed.probe_var_keys(d_bytes, d_offs, None, 2, N, found))
    ph = p.h.copy()
    ph[:1000] = hs
    mixed.probe_hashes(dev(ph), None, 2, N, found)
    torch.cuda.synchronize()
    got = found.cpu().numpy()[:2 * N].view(np.uint64).reshape(N, 2)
    oS = oracle.filter_add(oracle.make_config(log_index_size=8, seed=7), hs, value=9)
    assert (got[:, 0] == w.ofs[1].lookup_hashes(ph)).all()
    assert (got[:, 1] == oS.lookup_hashes(ph)).all()
    assert (got[:1000, 1] >> np.uint64(9) & np.uint64(1)).all()
    mixed.close()
    S.close()


# ---- 9: probes grouped by filter -----------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "d"])
def test_probe_var_keys_runs(world, oracle, name):
    """run boundaries inside a wave and an empty run; the second call re-uploads the bounds"""
    w = world
    rng = np.random.default_rng(11)
    sizes, values = [3000, 2000, 4000, 1000, 2500], [1, 0, 9, 33, 4]
    first = np.concatenate([[0], np.cumsum(sizes)])
    b = E.FilterBatch(w.cfg8, sizes, values)
    b.build_var_keys(*dev_var(w.poolA[0], w.poolA[1][:sum(sizes) + 1]))
    torch.cuda.synchronize()
    ha = oracle.hash_var(w.poolA[0][:int(w.poolA[1][sum(sizes)])], w.poolA[1][:sum(sizes) + 1])
    ofs = [oracle.filter_add(w.o8, ha[first[f]:first[f + 1]], value=values[f]) for f in range(5)]
    for counts in ([130, 0, 64, 1, 700], [1, 200, 0, 694, 0]):
        n = sum(counts)
        fid = np.repeat(np.arange(5, dtype=np.uint32), counts)
        p = make_probes(w, oracle, rng, name, n)
        # every other probe the filter's own key (profile d's long keys stay)
        own = np.arange(0, n, 2)
        own = own[np.diff(p.offs).astype(np.int64)[own] <= 300]
        ids = np.arange(n, dtype=np.int64) + sum(sizes)
        ids[own] = first[fid[own]] + rng.integers(0, 1000, size=len(own))
        data, offs, _ = concat_pools([(w.poolA[0][:int(w.poolA[1][sum(sizes)])], w.poolA[1][:sum(sizes) + 1]),
                                      (p.data, p.offs)])
        pdata, poffs = K.gather_var(data, offs, ids)
        h = oracle.hash_var(pdata, poffs)
        want = np.zeros(n, dtype=np.uint64)
        for f in range(5):
            want[fid == f] = ofs[f].lookup_hashes(h[fid == f])
        assert (want[own] >> np.array(values, dtype=np.uint64)[fid[own]] & np.uint64(1)).all()
        d_bytes, d_offs = dev_var(pdata, poffs, shift=3)
        found = torch.full((n + SENT,), -7, dtype=torch.int64, device="cuda:0")
        b.probe_var_keys_runs(d_bytes, d_offs, counts, found)
        got = read_found(found, n)
        check(got, want, (name, counts))
        found = torch.full((n + SENT,), -7, dtype=torch.int64, device="cuda:0")
        b.probe_var_keys(d_bytes, d_offs, dev(fid), n, found)
        assert (read_found(found, n) == got).all()
    b.close()


# ---- 10: the host-buffer form --------------------------------------------------------------
def test_routing_filter_lookup_var_keys(world, oracle):
    w = world
    rng = np.random.default_rng(12)
    n = 3000
    lens = rng.integers(8, 101, size=n)
    lens[rng.random(n) < 0.03] = 0
    lens[1777] = 5000
    fresh = rand_keys(rng, lens)
    data, offs, (fA, fF) = concat_pools([w.poolA, fresh])
    ids = fF + np.arange(n, dtype=np.int64)
    ids[0:1000:2] = fA + 5000 + rng.integers(0, 70000 - len(GIANTS), size=500)  # A1's own keys
    ids[1777] = fA + 75000 - len(GIANTS) + GIANTS.index(5000)
    pdata, poffs = K.gather_var(data, offs, ids)
    assert (np.diff(poffs) == 0).sum() >= 20 and np.diff(poffs).max() == 5000
    base = 1_000_003
    host = np.full(base + len(pdata) + PAD, 0xEE, dtype=np.uint8)
    host[base:base + len(pdata)] = pdata
    want = w.ofs[1].lookup_hashes(oracle.hash_var(pdata, poffs))
    got = E.routing_filter_lookup_var_keys(w.cfg8, w.imgA1, host, poffs + np.uint64(base))
    check(got, want, "host form")
    assert (got[0:1000:2] >> np.uint64(5) & np.uint64(1)).all() and got[1777] >> np.uint64(5) & np.uint64(1)
    assert (E.routing_filter_lookup_var_keys(w.cfg8, None, host, poffs + np.uint64(base)) == 0).all()


# ---- 5: trim (last: it releases A's work buffers) ------------------------------------------
def test_set_survives_trim_of_a_member_var(world):
    w, p = world, world.prof["d"]
    before = run_var(w, p, None, len(w.members))
    assert E.load_library().rf_amd_batch_trim(w.A.h, None) == 0
    # the released work buffers go back to the pool: a new build takes and overwrites them
    junk = E.FilterBatch(w.cfg8, [5000, 70000], [1, 2])
    junk.build_keys(dev(K.random_keys(75000, seed=105)), 24)
    torch.cuda.synchronize()
    after = run_var(w, p, None, len(w.members))
    assert (after == before).all()
    check(after, want_words(p.words, None), "after trim")
    junk.close()
