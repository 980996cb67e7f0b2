"""The ragged multi-get: rf_amd_filter_set_probe_{keys,var_keys,hashes}_ragged
(k_probe_fanout_ragged<KIND>: per-key member lists of any length as a CSR, d_found[p] answering
d_member[p]) and FilterSet.multiget_ragged / multiget_var_ragged. The world is
test_gpu_multiget's: batches A-D, the set (A0, A1, None, B0, C0, D0), N = 64 * 37 + 13 probes as
hashes and 24-byte keys, plus variable-length probes built with test_gpu_multiget_var's helpers.
The expected word of every pair is the oracle's routing_filter_lookup (src/routing_filter.c:
985-1073) of that key in that member, 0 for the None member and for ids past the end. d_member
and d_found are whole arrays around [off[0], off[n]): -7 fills d_found, and what lies outside the
offsets' range must stay -7."""
from types import SimpleNamespace

import numpy as np
import pytest

import test_gpu_multiget as MG
import test_gpu_multiget_var as MV
from splinterdb_amd import engine as E
from splinterdb_amd import keys as K
from test_gpu_multiget import world  # noqa: F401  (the fixture; a fresh instance for this module)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, SENT = MG.N, MG.SENT
NM = 6  # members of the set
FORMS = ["hashes", "keys", "var"]
EMPTY_WAVE = (192, 256)    # keys 192..255: a whole wave without pairs
EMPTY_CROSS = (256, 331)   # keys 256..330: an empty run across a wave boundary
AT64, AT128, AT300 = 400, 500, 600  # keys with exactly 64, 128 and 300 ids; AT300 + 1 has 1


def dev(a):
    return MG.dev(np.array(a))  # a copy: the fixtures' arrays are read-only


def offsets_of(counts, first=0):
    off = np.zeros(len(counts) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(counts, dtype=np.uint64), out=off[1:])
    return off + np.uint64(first)


@pytest.fixture(scope="module")
def rag(world, oracle):  # noqa: F811
    """the variable-length probes and their words, the ragged counts and ids; read-only"""
    w = world
    rng = np.random.default_rng(4242)
    r = SimpleNamespace()
    # the world's probes in a shuffled order, so that neighbouring keys come from different
    # sources (A1's keys, B's keys, D's clusters, random) and a pair given to the wrong
    # neighbour gets another word
    order = rng.permutation(N)
    r.ph, r.pk = w.ph[order], w.pk[order]
    # variable-length probes: the 24-byte probe keys that are A1's and B's own as they are, then
    # lengths 0-60 with zero-length keys, and one key past the 4 KiB window
    third = N // 3
    own = order < 2 * third
    lens = rng.integers(0, 61, size=N)
    lens[rng.random(N) < 0.1] = 0
    lens[own] = 24
    r.long_key = int(np.flatnonzero(~own)[40])
    lens[r.long_key] = 5000
    r.vdata, r.voffs = MV.rand_keys(rng, lens)
    r.vdata[r.voffs[:-1][own].astype(np.int64)[:, None] + np.arange(24)] = r.pk[own].reshape(-1, 24).view(np.uint8)
    assert (np.diff(r.voffs) == 0).sum() >= 20 and np.diff(r.voffs).max() > 4096
    r.vh = oracle.hash_var(r.vdata, r.voffs)
    assert (r.vh[own] == w.pkh[order][own]).all()
    r.words = {"hashes": w.words["hashes"][:, order], "keys": w.words["keys"][:, order],
               "var": MV.member_words(w.ofs, r.vh)}
    for a in r.words.values():
        a.setflags(write=False)
    # ragged counts 0..9 and the placed cases
    c = rng.integers(0, 10, size=N)
    c[0] = c[N - 1] = 0
    c[EMPTY_WAVE[0]:EMPTY_WAVE[1]] = 0
    c[EMPTY_CROSS[0]:EMPTY_CROSS[1]] = 0
    c[AT64], c[AT128], c[AT300], c[AT300 + 1] = 64, 128, 300, 1
    c[r.long_key] = max(c[r.long_key], 2)  # the long key owns pairs
    r.counts = c
    r.member = rng.integers(0, NM + 2, size=int(c.sum())).astype(np.uint32)
    # small n: key 0 owns pairs
    r.counts_small = rng.integers(0, 6, size=N)
    r.counts_small[0] = 3
    r.member_small = rng.integers(0, NM + 2, size=int(r.counts_small.sum())).astype(np.uint32)
    for a in (r.counts, r.member, r.counts_small, r.member_small):
        a.setflags(write=False)
    return r


def want_pairs(words, counts, member, nm=NM):
    """the oracle's word of every pair: key of pair p in member[p]"""
    key = np.repeat(np.arange(len(counts)), counts)
    ok = member < nm
    return np.where(ok, words[np.where(ok, member, 0), key], np.uint64(0))


def inputs(w, r, form, n=N, shift=0):
    """the device inputs of a form's first n probes"""
    if form == "hashes":
        return (dev(r.ph[:n]),)
    if form == "keys":
        return (dev(r.pk[:n]), 24)
    return MV.dev_var(r.vdata[:int(r.voffs[n])], r.voffs[:n + 1], shift=shift)


def run_ragged(fset, form, args, counts, member, first=0, junk=None):
    """one ragged probe over whole arrays: d_member and d_found hold `first` words before the
    offsets' range and SENT after it; returns the words of the range"""
    n = len(counts)
    off = offsets_of(counts, first)
    m = int(off[-1]) - first
    assert m == len(member)
    whole = np.full(first + m + SENT, NM + 1 if junk is None else junk, dtype=np.uint32)
    whole[first:first + m] = member
    found = torch.full((first + m + SENT,), -7, dtype=torch.int64, device="cuda:0")
    fn = {"hashes": fset.probe_hashes_ragged, "keys": fset.probe_keys_ragged, "var": fset.probe_var_keys_ragged}[form]
    fn(*args, dev(whole), dev(off.view(np.int64)), n, found)
    torch.cuda.synchronize()
    out = found.cpu().numpy()
    assert (out[:first] == -7).all(), "wrote before d_found[off[0]]"
    assert (out[first + m:] == -7).all(), "wrote past d_found[off[n])"
    return out[first:first + m].view(np.uint64)


def check(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, bad[:8].tolist(), got[bad[:4]], want[bad[:4]])


# ---- uniform lists: the oracle's words and, bit for bit, the fixed-K call's -----------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", [1, 3, 5])
def test_uniform_lists(world, rag, form, k):  # noqa: F811
    w, r = world, rag
    member = w.member[k].reshape(-1)
    counts = np.full(N, k)
    args = inputs(w, r, form)
    got = run_ragged(w.set, form, args, counts, member)
    check(got, want_pairs(r.words[form], counts, member), (form, k))
    found = torch.full((N * k + SENT,), -7, dtype=torch.int64, device="cuda:0")
    fixed = {"hashes": w.set.probe_hashes, "keys": w.set.probe_keys, "var": w.set.probe_var_keys}[form]
    fixed(*args, dev(member), k, N, found)
    assert got.tobytes() == MV.read_found(found, N * k).tobytes()


# ---- ragged lists, every form ---------------------------------------------------------------
def test_placed_cases_exist(rag):
    c, m = rag.counts, rag.member
    assert c[0] == 0 and c[N - 1] == 0
    assert (c[EMPTY_WAVE[0]:EMPTY_WAVE[1]] == 0).all() and EMPTY_WAVE[0] % 64 == 0 and EMPTY_WAVE[1] % 64 == 0
    assert (c[EMPTY_CROSS[0]:EMPTY_CROSS[1]] == 0).all() and EMPTY_CROSS[0] // 64 != (EMPTY_CROSS[1] - 1) // 64
    assert c[EMPTY_CROSS[1]:EMPTY_CROSS[1] + 64].any(), "the crossing run's second wave owns pairs"
    assert (c[AT64], c[AT128], c[AT300], c[AT300 + 1]) == (64, 128, 300, 1) and 300 > 64 * 2
    assert c.max() == 300 and set(range(10)) <= set(c.tolist())
    assert (m == NM).any() and (m == NM + 1).any() and (m == 2).any()
    # what a search that lets an empty list steal its successor's first pair would give
    key = np.repeat(np.arange(N), c)
    first_of_list = np.flatnonzero(np.diff(key, prepend=-1) > 0)
    stolen = first_of_list[c[key[first_of_list] - 1] == 0]
    assert stolen.size > 100
    for form in FORMS:
        want = want_pairs(rag.words[form], c, m)
        assert (np.array([bin(int(x)).count("1") for x in want]) >= 2).any(), (form, "no word with two bits set")
        ok = m[stolen] < NM
        thief = np.where(ok, rag.words[form][np.where(ok, m[stolen], 0), key[stolen] - 1], np.uint64(0))
        assert (thief != want[stolen]).sum() >= 10, (form, "a stolen pair would not show")


@pytest.mark.parametrize("form", FORMS)
def test_ragged_lists(world, rag, form):  # noqa: F811
    w, r = world, rag
    got = run_ragged(w.set, form, inputs(w, r, form), r.counts, r.member)
    want = want_pairs(r.words[form], r.counts, r.member)
    check(got, want, form)
    assert (got[r.member >= NM] == 0).all() and (got[r.member == 2] == 0).all()
    assert (np.array([bin(int(x)).count("1") for x in got]) >= 2).any()
    if form == "var":  # the zero-length keys and the key past the window own pairs
        vlen = np.repeat(np.diff(r.voffs).astype(np.int64), r.counts)
        assert (vlen == 0).any() and (vlen > 4096).any()


def test_var_base_not_aligned(world, rag):  # noqa: F811
    w, r = world, rag
    got = run_ragged(w.set, "var", inputs(w, r, "var", shift=5), r.counts, r.member)
    check(got, want_pairs(r.words["var"], r.counts, r.member), "shift 5")


# ---- bounds ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_bounds_first_offset_1000(world, rag, form):  # noqa: F811
    """off[0] = 1000 inside whole arrays: run_ragged checks the sentinels on both sides"""
    w, r = world, rag
    got = run_ragged(w.set, form, inputs(w, r, form), r.counts, r.member, first=1000, junk=1)
    check(got, want_pairs(r.words[form], r.counts, r.member), form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("first", [0, 1000])
def test_all_lists_empty_writes_nothing(world, rag, form, first):  # noqa: F811
    w, r = world, rag
    got = run_ragged(w.set, form, inputs(w, r, form), np.zeros(N, dtype=np.int64), np.zeros(0, dtype=np.uint32),
                     first=first, junk=1)
    assert got.size == 0


# ---- small n --------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_n(world, rag, form, n):  # noqa: F811
    w, r = world, rag
    counts = r.counts_small[:n]
    member = r.member_small[:int(counts.sum())]
    got = run_ragged(w.set, form, inputs(w, r, form, n=n), counts, member, first=7, junk=1)
    assert got.size >= 3
    check(got, want_pairs(r.words[form][:, :n], counts, member), (form, n))


# ---- key kinds ------------------------------------------------------------------------------
def test_keys_not_16_byte_aligned(world, rag):  # noqa: F811
    w, r = world, rag
    buf = torch.zeros(N * 24 + 16, dtype=torch.uint8, device="cuda:0")
    buf[8:8 + N * 24] = dev(r.pk.reshape(-1).view(np.uint8))
    assert buf[8:].data_ptr() % 16 == 8
    got = run_ragged(w.set, "keys", (buf[8:], 24), r.counts, r.member)
    check(got, want_pairs(r.words["keys"], r.counts, r.member), "base % 16 == 8")


@pytest.mark.parametrize("key_len", [8, 13, 40])
def test_other_key_lengths(world, rag, oracle, key_len):  # noqa: F811
    """word-aligned and byte-aligned key lengths, hashed by oracle.hash_fixed: a member built
    from such keys, half of the probes its own keys"""
    w, r = world, rag
    own = K.random_keys(3000, key_len=key_len, seed=200 + key_len)
    b = E.FilterBatch(w.cfg8, [3000], [4])
    b.build_keys(dev(own), key_len)
    torch.cuda.synchronize()
    hown = oracle.hash_fixed(own.reshape(-1), key_len)
    ofs = [oracle.filter_add(oracle.make_config(log_index_size=8), hown, value=4), w.ofs[1], w.ofs[5]]
    fs = E.FilterSet([(b, 0), (w.A, 1), (w.D, 0)])
    pk = K.random_keys(N, key_len=key_len, seed=300 + key_len)
    pk[: N // 2] = own[np.random.default_rng(key_len).integers(0, 3000, size=N // 2)]
    words = np.stack([of.lookup_hashes(oracle.hash_fixed(pk.reshape(-1), key_len)) for of in ofs])
    member = r.member % 5  # ids 3 and 4 are past the end
    got = run_ragged(fs, "keys", (dev(pk), key_len), r.counts, member, first=1000)
    want = want_pairs(words, r.counts, member, nm=3)
    check(got, want, key_len)
    own_pairs = (np.repeat(np.arange(N), r.counts) < N // 2) & (member == 0)
    assert own_pairs.any() and (got[own_pairs] >> np.uint64(4) & np.uint64(1)).all()
    fs.close()
    b.close()


# ---- the grid-stride loop -------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("blocks", [1, 2])
def test_grid_stride_loop(world, rag, blocks, form):  # noqa: F811
    """2,381 keys on 1 or 2 workgroups of 4 waves: 10 or 5 chunks per wave, the empty wave and
    the long lists among them"""
    w, r = world, rag
    try:
        E.diag_fanout_max_blocks(blocks)
        got = run_ragged(w.set, form, inputs(w, r, form), r.counts, r.member, first=1000)
    finally:
        E.diag_fanout_max_blocks(0)
    check(got, want_pairs(r.words[form], r.counts, r.member), (blocks, form))


# ---- end to end -----------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["keys", "var"])
def test_multiget_ragged_end_to_end(world, rag, form):  # noqa: F811
    w, r = world, rag
    first = 1000
    off = offsets_of(r.counts, first)
    whole = np.full(first + len(r.member), 1, dtype=np.uint32)
    whole[first:] = r.member
    want = E.found_candidates(want_pairs(r.words[form], r.counts, r.member))
    want_key = E.ragged_pair_keys(off, want >> np.uint64(8))
    assert len(want) > 16 and (r.counts[want_key] > 0).all()
    fn = w.set.multiget_ragged if form == "keys" else w.set.multiget_var_ragged
    for cap in (16, len(want), None):  # 16: too small, the count is still the total and the second pass runs
        d_cand, count, d_key = fn(*inputs(w, r, form), dev(whole), dev(off.view(np.int64)), N, cap=cap)
        assert count == len(want), (cap, count, len(want))
        assert (d_cand[:count].cpu().numpy().view(np.uint64) == want).all(), cap
        assert d_key.shape == (count,) and (d_key.cpu().numpy() == want_key).all(), cap


def test_multiget_ragged_no_pairs(world, rag):  # noqa: F811
    w, r = world, rag
    off = dev(np.full(N + 1, 1000, dtype=np.int64))
    d_cand, count, d_key = w.set.multiget_ragged(*inputs(w, r, "keys"), dev(np.zeros(4, dtype=np.uint32)), off, N)
    assert count == 0 and d_key.numel() == 0


# ---- errors ---------------------------------------------------------------------------------
def test_errors(world, rag, oracle):  # noqa: F811
    w, r = world, rag
    L = E.load_library()
    off = dev(offsets_of(r.counts).view(np.int64))
    dm = dev(r.member)
    found = torch.zeros(len(r.member), dtype=torch.int64, device="cuda:0")
    d_h, (d_k, _), (d_b, d_o) = inputs(w, r, "hashes")[0], inputs(w, r, "keys"), inputs(w, r, "var")

    def einval(fn):
        with pytest.raises(E.PlatformStatusError) as ei:
            fn()
        assert ei.value.code == E.STATUS_BAD_PARAM

    s = w.set
    # a NULL set
    p = [x.data_ptr() for x in (d_h, d_k, d_b, d_o, dm, off, found)]
    assert L.rf_amd_filter_set_probe_hashes_ragged(None, p[0], p[4], p[5], N, p[6], None) == E.STATUS_BAD_PARAM
    assert L.rf_amd_filter_set_probe_keys_ragged(None, p[1], 24, p[4], p[5], N, p[6], None) == E.STATUS_BAD_PARAM
    assert L.rf_amd_filter_set_probe_var_keys_ragged(None, p[2], p[3], p[4], p[5], N, p[6], None) == E.STATUS_BAD_PARAM
    # key_len == 0
    einval(lambda: s.probe_keys_ragged(d_k, 0, dm, off, N, found))
    # with n > 0: a NULL input, d_member, d_member_off or d_found
    einval(lambda: s.probe_hashes_ragged(None, dm, off, N, found))
    einval(lambda: s.probe_hashes_ragged(d_h, None, off, N, found))
    einval(lambda: s.probe_hashes_ragged(d_h, dm, None, N, found))
    einval(lambda: s.probe_hashes_ragged(d_h, dm, off, N, None))
    einval(lambda: s.probe_keys_ragged(None, 24, dm, off, N, found))
    einval(lambda: s.probe_keys_ragged(d_k, 24, None, off, N, found))
    einval(lambda: s.probe_keys_ragged(d_k, 24, dm, None, N, found))
    einval(lambda: s.probe_keys_ragged(d_k, 24, dm, off, N, None))
    einval(lambda: s.probe_var_keys_ragged(None, d_o, dm, off, N, found))
    einval(lambda: s.probe_var_keys_ragged(d_b, None, dm, off, N, found))
    einval(lambda: s.probe_var_keys_ragged(d_b, d_o, None, off, N, found))
    einval(lambda: s.probe_var_keys_ragged(d_b, d_o, dm, None, N, found))
    einval(lambda: s.probe_var_keys_ragged(d_b, d_o, dm, off, N, None))
    # n >= 2^56
    einval(lambda: s.probe_hashes_ragged(d_h, dm, off, 1 << 56, found))
    einval(lambda: s.probe_keys_ragged(d_k, 24, dm, off, 1 << 56, found))
    einval(lambda: s.probe_var_keys_ragged(d_b, d_o, dm, off, 1 << 56, found))
    # n == 0 is OK with NULL pointers, and touches nothing with real ones
    s.probe_hashes_ragged(None, None, None, 0, None)
    s.probe_keys_ragged(None, 24, None, None, 0, None)
    s.probe_var_keys_ragged(None, None, None, None, 0, None)
    sent = torch.full((SENT,), -7, dtype=torch.int64, device="cuda:0")
    s.probe_keys_ragged(d_k, 24, dm, off, 0, sent)
    MV.read_found(sent, 0)
    # members hashed with different seeds: no keys forms, the hashes form works
    cfg7 = E.routing_config_init(log_index_size=8, seed=7)
    ks = K.random_keys(3000, seed=106)
    hs = oracle.hash_fixed(ks.reshape(-1), 24, seed=7)
    S = E.FilterBatch(cfg7, [3000], [9])
    S.build_keys(dev(ks), 24)
    torch.cuda.synchronize()
    mixed = E.FilterSet([(w.A, 1), (S, 0)])
    einval(lambda: mixed.probe_keys_ragged(d_k, 24, dm, off, N, found))
    einval(lambda: mixed.probe_var_keys_ragged(d_b, d_o, dm, off, N, found))
    ph = r.ph.copy()
    ph[:1000] = hs[:1000]
    member = r.member % 3  # id 2 is past the end
    got = run_ragged(mixed, "hashes", (dev(ph),), r.counts, member)
    oS = oracle.filter_add(oracle.make_config(log_index_size=8, seed=7), hs, value=9)
    words = np.stack([w.ofs[1].lookup_hashes(ph), oS.lookup_hashes(ph)])
    check(got, want_pairs(words, r.counts, member, nm=2), "mixed seeds, hashes form")
    hit = (np.repeat(np.arange(N), r.counts) < 1000) & (member == 1)
    assert hit.any() and (got[hit] >> np.uint64(9) & np.uint64(1)).all()
    mixed.close()
    S.close()
