"""The multi-get's device form: a resident filter set over several batches, fan-out probes of
every key against K members (rf_amd_filter_set_probe_*), the compaction of found_values words
into an ordered candidate list (rf_amd_found_compact), and both chained (FilterSet.multiget).
Every found word is compared with the oracle's routing_filter_lookup (src/routing_filter.c:
985-1073) of that member, every candidate record with E.found_candidates of the oracle's words."""
from types import SimpleNamespace

import numpy as np
import pytest

from splinterdb_amd import engine as E
from splinterdb_amd import keys as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = 64 * 37 + 13
SENT = 4096


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def clustered_hashes(rng, fps, lis, n):
    """the filter of test_gpu_probe_fast's overflowed-lines test: 16 clusters of 150 fingerprints
    in 4 neighbouring buckets, so their probe lines overflow and lookups walk the image"""
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
    return h, k, sh


@pytest.fixture(scope="module")
def world(oracle):
    """batches A-D, their oracle filters, the set (A0, A1, None, B0, C0, D0), the probes (hashes
    and 24-byte keys) and the oracle's words of every probe in every member; read-only"""
    rng = np.random.default_rng(2024)
    w = SimpleNamespace()
    cfg8, o8 = E.routing_config_init(log_index_size=8), oracle.make_config(log_index_size=8)
    cfg9, o9 = E.routing_config_init(log_index_size=9), oracle.make_config(log_index_size=9)
    # A: two filters, values 0 and 5
    ka = K.random_keys(75000, seed=101)
    ha = oracle.hash_fixed(ka.reshape(-1), 24)
    w.A = E.FilterBatch(cfg8, [5000, 70000], [0, 5])
    w.A.build_keys(dev(ka), 24)
    oA0, oA1 = oracle.filter_add(o8, ha[:5000], value=0), oracle.filter_add(o8, ha[5000:], value=5)
    # B: 200,001 keys with value 2, the first 100,000 again with value 7 (words with two bits)
    kb = K.random_keys(200001, seed=102)
    hb = oracle.hash_fixed(kb.reshape(-1), 24)
    w.B_old = E.FilterBatch(cfg8, [200001], [2])
    w.B_old.build_keys(dev(kb), 24)
    w.B = E.FilterBatch(cfg8, [100000], [7], old=[(w.B_old, 0)])
    w.B.build_keys(dev(kb[:100000]), 24)
    oB = oracle.filter_add(o8, hb[:100000], value=7, old=oracle.filter_add(o8, hb, value=2))
    # C: log_index_size 9, value 63
    kc = K.random_keys(1 << 17, seed=103)
    hc = oracle.hash_fixed(kc.reshape(-1), 24)
    w.C = E.FilterBatch(cfg9, [1 << 17], [63])
    w.C.build_keys(dev(kc), 24)
    oC = oracle.filter_add(o9, hc, value=63)
    # D: clustered hashes, overflowed probe lines
    hd, kd, sh = clustered_hashes(rng, 26, 8, 400000)
    w.D = E.FilterBatch(cfg8, [400000], [3])
    w.D.build_hashes(dev(hd))
    oD = oracle.filter_add(o8, hd, value=3)
    torch.cuda.synchronize()
    w.cfg8 = cfg8
    w.ofs = [oA0, oA1, None, oB, oC, oD]
    w.members = [(w.A, 0), (w.A, 1), None, (w.B, 0), (w.C, 0), (w.D, 0)]
    w.set = E.FilterSet(w.members)
    third = N // 3
    # hashes form: a third from A1's keys, a third from B's twice-added keys, then D's clustered
    # hashes, their one-bit neighbours, and random hashes
    ph = rng.integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32)
    ph[:third] = ha[5000 + rng.integers(0, 70000, size=third)]
    ph[third:2 * third] = hb[rng.integers(0, 100000, size=third)]
    pick = rng.integers(0, kd, size=300)
    ph[2 * third:2 * third + 300] = hd[pick]
    ph[2 * third + 300:2 * third + 600] = hd[pick] ^ np.uint32(1 << sh)
    # keys form: the same thirds as keys, the rest random keys
    pk = K.random_keys(N, seed=104)
    pk[:third] = ka[5000 + rng.integers(0, 70000, size=third)]
    pk[third:2 * third] = kb[rng.integers(0, 100000, size=third)]
    w.ph, w.pk = ph, pk
    w.pkh = oracle.hash_fixed(pk.reshape(-1), 24)

    def member_words(h):
        return np.stack([of.lookup_hashes(h) if of is not None else np.zeros(len(h), dtype=np.uint64)
                         for of in w.ofs])
    w.words = {"hashes": member_words(ph), "keys": member_words(w.pkh)}
    for a in w.words.values():
        a.setflags(write=False)
    # member ids of every K, ids past the end included
    w.member = {k: rng.integers(0, len(w.members) + 2, size=(N, k)).astype(np.uint32) for k in (1, 3, 5, 8)}
    yield w
    w.set.close()


def want_words(w, form, member):
    """the oracle's word of every (key, slot); member None: slot j is member j"""
    words = w.words[form]
    if member is None:
        return np.ascontiguousarray(words.T).reshape(-1)
    ok = member < len(w.members)
    g = np.where(ok, member, 0)
    return np.where(ok, words[g, np.arange(N)[:, None]], np.uint64(0)).reshape(-1)


def run_probe(w, form, member, k, keys=None):
    found = torch.full((N * k + SENT,), -7, dtype=torch.int64, device="cuda:0")
    dm = None if member is None else dev(member.reshape(-1))
    if form == "hashes":
        w.set.probe_hashes(dev(w.ph), dm, k, N, found)
    else:
        w.set.probe_keys(dev(w.pk) if keys is None else keys, 24, dm, k, N, found)
    torch.cuda.synchronize()
    out = found.cpu().numpy()
    assert (out[N * k:] == -7).all(), "wrote past d_found[n * K)"
    return out[:N * k].view(np.uint64)


@pytest.mark.parametrize("form", ["hashes", "keys"])
@pytest.mark.parametrize("k", [1, 3, 5, 8, None])
def test_fanout_vs_oracle(world, form, k):
    w = world
    member = None if k is None else w.member[k]
    kk = len(w.members) if k is None else k
    got = run_probe(w, form, member, kk)
    want = want_words(w, form, member)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (form, k, bad.size, bad[:8].tolist(), got[bad[:4]], want[bad[:4]])
    if member is not None:
        assert (got.reshape(N, kk)[member >= len(w.members)] == 0).all()
        assert (got.reshape(N, kk)[member == 2] == 0).all()  # the None member
        assert (member >= len(w.members)).any() and (member == 2).any()
    if k is None:
        assert (got.reshape(N, kk)[:, 2] == 0).all()
        two = np.array([bin(int(x)).count("1") for x in got]) >= 2
        assert two.any(), "no word with two bits set: batch B's path was not reached"
        if form == "hashes":
            assert got.reshape(N, kk)[:, 5].any(), "no probe of D found anything"


def test_fanout_reaches_two_bit_words_and_overflowed_lines(world):
    """the oracle's words themselves: B's twice-added keys carry values 2 and 7, D's clustered
    hashes are found (so the comparisons above covered both)"""
    w = world
    third = N // 3
    assert (w.words["hashes"][3, third:2 * third] & np.uint64(0x84) == np.uint64(0x84)).all()
    assert (w.words["keys"][3, third:2 * third] & np.uint64(0x84) == np.uint64(0x84)).all()
    assert (w.words["hashes"][5, 2 * third:2 * third + 300] >> np.uint64(3) & np.uint64(1)).all()
    lines = w.D.debug_lines()
    assert (lines[:, :16] == 0xFF).all(axis=1).any(), "D has no overflowed probe line"


@pytest.mark.parametrize("k", [3, None])
def test_fanout_keys_not_16_byte_aligned(world, k):
    w = world
    buf = torch.zeros(N * 24 + 16, dtype=torch.uint8, device="cuda:0")
    buf[8:8 + N * 24] = dev(w.pk.reshape(-1).view(np.uint8))
    member = None if k is None else w.member[k]
    got = run_probe(w, "keys", member, len(w.members) if k is None else k, keys=buf[8:])
    assert (got == want_words(w, "keys", member)).all()


@pytest.mark.parametrize("key_len", [16, 13, 40])
def test_fanout_other_key_lengths(world, oracle, key_len):
    """word-aligned and byte-aligned key lengths (the hash paths of rf_amd_batch_probe_keys):
    a member built from such keys, half of the probes its own keys"""
    w = world
    own = K.random_keys(3000, key_len=key_len, seed=200 + key_len)
    b = E.FilterBatch(w.cfg8, [3000], [4])
    b.build_keys(dev(own), key_len)
    torch.cuda.synchronize()
    hown = oracle.hash_fixed(own.reshape(-1), key_len)
    ofs = [oracle.filter_add(oracle.make_config(log_index_size=8), hown, value=4), w.ofs[1], w.ofs[5]]
    fs = E.FilterSet([(b, 0), (w.A, 1), (w.D, 0)])
    pk = K.random_keys(N, key_len=key_len, seed=300 + key_len)
    pk[: N // 2] = own[np.random.default_rng(key_len).integers(0, 3000, size=N // 2)]
    ph = oracle.hash_fixed(pk.reshape(-1), key_len)
    words = np.stack([of.lookup_hashes(ph) for of in ofs])
    for member in (None, w.member[3] % 5):  # ids 3 and 4 are past the end
        kk = 3
        found = torch.full((N * kk + SENT,), -7, dtype=torch.int64, device="cuda:0")
        fs.probe_keys(dev(pk), key_len, None if member is None else dev(member.reshape(-1)), kk, N, found)
        torch.cuda.synchronize()
        out = found.cpu().numpy()
        assert (out[N * kk:] == -7).all()
        got = out[:N * kk].view(np.uint64).reshape(N, kk)
        if member is None:
            want = words.T
        else:
            ok = member < 3
            want = np.where(ok, words[np.where(ok, member, 0), np.arange(N)[:, None]], np.uint64(0))
        assert (got == want).all(), (key_len, int((got != want).sum()))
        if member is None:
            assert (got[: N // 2, 0] >> np.uint64(4) & np.uint64(1)).all()
    fs.close()
    b.close()


def test_set_survives_trim_of_a_member(world):
    w = world
    before = run_probe(w, "keys", None, len(w.members))
    rc = E.load_library().rf_amd_batch_trim(w.A.h, None)
    assert rc == 0
    # the released work buffers go back to the pool: a new build takes and overwrites them
    junk = E.FilterBatch(w.cfg8, [5000, 70000], [1, 2])
    junk.build_keys(dev(K.random_keys(75000, seed=105)), 24)
    torch.cuda.synchronize()
    after = run_probe(w, "keys", None, len(w.members))
    assert (after == before).all()
    assert (after == want_words(w, "keys", None)).all()
    junk.close()


def test_errors(world, oracle):
    w = world
    found = torch.zeros(N * 8, dtype=torch.int64, device="cuda:0")
    unbuilt = E.FilterBatch(w.cfg8, [10], [0])

    def einval(fn):
        with pytest.raises(E.PlatformStatusError) as ei:
            fn()
        assert ei.value.code == E.STATUS_BAD_PARAM

    einval(lambda: E.FilterSet([(w.A, 0), (unbuilt, 0)]))
    einval(lambda: E.FilterSet([(w.A, 2)]))
    einval(lambda: w.set.probe_hashes(dev(w.ph), dev(w.member[3].reshape(-1)), 0, N, found))
    einval(lambda: w.set.probe_keys(dev(w.pk), 24, dev(w.member[3].reshape(-1)), 0, N, found))
    einval(lambda: w.set.probe_hashes(dev(w.ph), None, 5, N, found))
    einval(lambda: w.set.probe_keys(dev(w.pk), 24, None, 7, N, found))
    # members hashed with different seeds: no keys form, the hashes form works
    cfg7 = E.routing_config_init(log_index_size=8, seed=7)
    ks = K.random_keys(3000, seed=106)
    hs = oracle.hash_fixed(ks.reshape(-1), 24, seed=7)
    S = E.FilterBatch(cfg7, [3000], [9])
    S.build_keys(dev(ks), 24)
    torch.cuda.synchronize()
    mixed = E.FilterSet([(w.A, 1), (S, 0)])
    einval(lambda: mixed.probe_keys(dev(w.pk), 24, None, 2, N, found))
    ph = w.ph.copy()
    ph[:1000] = hs[:1000]
    mixed.probe_hashes(dev(ph), None, 2, N, found)
    torch.cuda.synchronize()
    got = found.cpu().numpy()[:2 * N].view(np.uint64).reshape(N, 2)
    oS = oracle.filter_add(oracle.make_config(log_index_size=8, seed=7), hs, value=9)
    assert (got[:, 0] == w.ofs[1].lookup_hashes(ph)).all()
    assert (got[:, 1] == oS.lookup_hashes(ph)).all()
    assert (got[:1000, 1] >> np.uint64(9) & np.uint64(1)).all()
    mixed.close()
    S.close()
    unbuilt.close()


def compact(d_found, m, cap):
    """one rf_amd_found_compact into a buffer of cap records followed by sentinels"""
    buf = torch.full((cap + SENT,), -7, dtype=torch.int64, device="cuda:0")
    cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda:0")
    E.found_compact(d_found, m, buf[:cap], cnt)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), int(cnt.item())


def compaction_inputs(w):
    rng = np.random.default_rng(77)
    big = 3 * E.FOUND_COMPACT_TILE + 17
    sparse = np.where(rng.random(big) < 0.1, np.uint64(1) << rng.integers(0, 64, size=big).astype(np.uint64),
                      np.uint64(0))
    sparse |= np.where(rng.random(big) < 0.02, np.uint64(1) << rng.integers(0, 64, size=big).astype(np.uint64),
                       np.uint64(0))
    return {
        "zero": np.zeros(big, dtype=np.uint64),
        "ones": np.full(big, ~np.uint64(0), dtype=np.uint64),
        "random": rng.integers(0, 1 << 64, size=big, dtype=np.uint64),
        "sparse": sparse,
        "probe_all_members": want_words(w, "hashes", None)[:big],
        "probe_k8": want_words(w, "keys", w.member[8])[:big],
    }


@pytest.mark.parametrize("kind", ["zero", "ones", "random", "sparse", "probe_all_members", "probe_k8"])
def test_found_compact_vs_host_mirror(world, kind):
    T = E.FOUND_COMPACT_TILE
    L = E.load_library()
    assert L.rf_amd_found_compact_scratch_bytes(T) < L.rf_amd_found_compact_scratch_bytes(T + 1)  # T is the tile
    words = compaction_inputs(world)[kind]
    assert len(words) == 3 * T + 17
    d_words = dev(words.view(np.int64))
    for m in (0, 1, 63, 64, 65, T - 1, T + 1, 3 * T + 17):
        want = E.found_candidates(words[:m]).view(np.int64)
        count = len(want)
        for cap in (count + 5, count // 2, 0):
            buf, got_count = compact(d_words, m, cap)
            assert got_count == count, (kind, m, cap, got_count, count)
            k = min(cap, count)
            assert (buf[:k] == want[:k]).all(), (kind, m, cap)
            assert (buf[k:] == -7).all(), (kind, m, cap, "wrote past the records")
        again, _ = compact(d_words, m, count + 5)
        first, _ = compact(d_words, m, count + 5)
        assert again.tobytes() == first.tobytes()


@pytest.mark.parametrize("k", [3, None])
def test_multiget_end_to_end(world, k):
    w = world
    member = None if k is None else w.member[k]
    kk = len(w.members) if k is None else k
    want = E.found_candidates(want_words(w, "keys", member))
    assert len(want) > 16
    dm = None if member is None else dev(member.reshape(-1))
    d_cand, count = w.set.multiget(dev(w.pk), 24, dm, kk, N, cap=16)  # too small: the retry runs
    assert count == len(want)
    assert (d_cand[:count].cpu().numpy().view(np.uint64) == want).all()
    d_cand, count = w.set.multiget(dev(w.pk), 24, dm, kk, N, cap=len(want))  # fits at once
    assert count == len(want)
    assert (d_cand[:count].cpu().numpy().view(np.uint64) == want).all()
