"""Filter sets that follow compactions: rf_amd_filter_set_create_cap, stream-ordered member
updates (rf_amd_filter_set_update) and the stream-ordered destroy (rf_amd_filter_set_destroy_on).

Every found word is compared with the oracle's routing_filter_lookup (src/routing_filter.c:
985-1073) of the member that should sit in that slot at that point in stream order: through
probe_hashes with K in {3, 8} and ids past the end, through probe_hashes_ragged with lists of 0
to 9 ids, and -- where the test knows the member count -- through the all-members form, which
reads every slot for every key. All found buffers carry sentinels past their end."""
from types import SimpleNamespace

import numpy as np
import pytest

import reject_cases as R
from splinterdb_amd import engine as E
from splinterdb_amd import keys as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = 64 * 37 + 13
SENT = 4096
TF, TN = 150, 300  # batch T: filters, hashes of each
PER_LAUNCH = 64    # SET_UPD_PER_LAUNCH (rf_plan.h)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def clustered_hashes(rng, fps, lis, n):
    """16 clusters of 150 fingerprints in 4 neighbouring buckets: their probe lines overflow and
    lookups walk the image"""
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
    return h, k


@pytest.fixture(scope="module")
def world(oracle):
    """batches A, C, D and T, the oracle's filter of each of their filters by name ("A0", "A1",
    "C0", "D0", "T0".."T149"), the probes (hashes and 24-byte keys) and the oracle's words of
    every probe in every named filter; read-only"""
    rng = np.random.default_rng(2025)
    w = SimpleNamespace()
    w.oracle = oracle
    w.cfg8, w.o8 = E.routing_config_init(log_index_size=8), oracle.make_config(log_index_size=8)
    cfg9, o9 = E.routing_config_init(log_index_size=9), oracle.make_config(log_index_size=9)
    of = {}
    ka = K.random_keys(75000, seed=101)
    ha = oracle.hash_fixed(ka.reshape(-1), 24)
    w.A = E.FilterBatch(w.cfg8, [5000, 70000], [0, 5])
    w.A.build_keys(dev(ka), 24)
    of["A0"], of["A1"] = oracle.filter_add(w.o8, ha[:5000], value=0), oracle.filter_add(w.o8, ha[5000:], value=5)
    kc = K.random_keys(1 << 17, seed=103)
    hc = oracle.hash_fixed(kc.reshape(-1), 24)
    w.C = E.FilterBatch(cfg9, [1 << 17], [63])
    w.C.build_keys(dev(kc), 24)
    of["C0"] = oracle.filter_add(o9, hc, value=63)
    hd, kd = clustered_hashes(rng, 26, 8, 400000)
    w.D = E.FilterBatch(w.cfg8, [400000], [3])
    w.D.build_hashes(dev(hd))
    of["D0"] = oracle.filter_add(w.o8, hd, value=3)
    ht = rng.integers(0, 1 << 32, size=TF * TN, dtype=np.uint64).astype(np.uint32)
    w.T = E.FilterBatch(w.cfg8, [TN] * TF, [f % 64 for f in range(TF)])
    w.T.build_hashes(dev(ht))
    for f in range(TF):
        of[f"T{f}"] = oracle.filter_add(w.o8, ht[f * TN:(f + 1) * TN], value=f % 64)
    torch.cuda.synchronize()
    w.member = {"A0": (w.A, 0), "A1": (w.A, 1), "C0": (w.C, 0), "D0": (w.D, 0)}
    w.member.update({f"T{f}": (w.T, f) for f in range(TF)})
    # hashes: 12 of every filter of T, then A1's, C's, D's clustered ones, A0's, random ones
    ph = rng.integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32)
    at = 0
    for f in range(TF):
        ph[at:at + 12] = ht[f * TN + rng.integers(0, TN, size=12)]
        at += 12
    for src, cnt in ((ha[5000:], 150), (hc, 150), (hd[:kd], 150), (ha[:5000], 60)):
        ph[at:at + cnt] = src[rng.integers(0, len(src), size=cnt)]
        at += cnt
    assert at < N
    # keys: a third each of A1's and C's keys, then A0's and random keys
    pk = K.random_keys(N, seed=104)
    third = N // 3
    pk[:third] = ka[5000 + rng.integers(0, 70000, size=third)]
    pk[third:2 * third] = kc[rng.integers(0, 1 << 17, size=third)]
    pk[2 * third:2 * third + 100] = ka[rng.integers(0, 5000, size=100)]
    w.ph, w.pk = ph, pk
    w.pkh = oracle.hash_fixed(pk.reshape(-1), 24)
    w.words = {name: f.lookup_hashes(ph) for name, f in of.items()}
    w.kwords = {name: of[name].lookup_hashes(w.pkh) for name in ("A0", "A1", "C0", "D0")}
    for a in list(w.words.values()) + list(w.kwords.values()) + [w.ph, w.pk, w.pkh]:
        a.setflags(write=False)
    w.of = of
    assert all(w.words[f"T{f}"][12 * f:12 * f + 12].all() for f in range(TF))
    yield w


def members_of(w, names):
    return [None if nm is None else w.member[nm] for nm in names]


def words_of(w, names, words=None):
    words = w.words if words is None else words
    return [None if nm is None else words[nm] for nm in names]


class Probes:
    """One round of probes of a set, prepared ahead (every input and found buffer is on the
    device before launch(), which only queues kernels) and checked after the caller's
    synchronisation. Member ids range over [0, hi): hi is the set's capacity + 2, so ids past
    num_members and past the capacity are among them. all_k: also the all-members form, which
    needs the member count at the time the probes run."""

    def __init__(self, ph, hi, seed, all_k=None):
        rng = np.random.default_rng([seed, hi])
        self.n, self.hi, self.all_k = len(ph), hi, all_k
        self.d_h = dev(ph)
        self.ids = {k: rng.integers(0, hi, size=(self.n, k)).astype(np.uint32) for k in (3, 8)}
        self.counts = rng.integers(0, 10, size=self.n)
        self.rmember = rng.integers(0, hi, size=int(self.counts.sum())).astype(np.uint32)
        off = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.uint64)
        self.d_ids = {k: dev(v.reshape(-1)) for k, v in self.ids.items()}
        self.d_rm, self.d_off = dev(self.rmember), dev(off.view(np.int64))
        self.size = {3: self.n * 3, 8: self.n * 8, "ragged": len(self.rmember)}
        if all_k:
            self.size["all"] = self.n * all_k
        self.found = {k: torch.full((m + SENT,), -7, dtype=torch.int64, device="cuda:0") for k, m in self.size.items()}
        torch.cuda.synchronize()

    def launch(self, fs, stream=None):
        for k in (3, 8):
            fs.probe_hashes(self.d_h, self.d_ids[k], k, self.n, self.found[k], stream=stream)
        fs.probe_hashes_ragged(self.d_h, self.d_rm, self.d_off, self.n, self.found["ragged"], stream=stream)
        if self.all_k:
            fs.probe_hashes(self.d_h, None, self.all_k, self.n, self.found["all"], stream=stream)
        return self

    def check(self, slot_words, num_members, tag):
        """slot_words[g]: the oracle's words of the member in slot g (None: an empty slot);
        slots at and past num_members find nothing whatever they hold"""
        tab = np.zeros((self.hi, self.n), dtype=np.uint64)
        for g, wd in enumerate(slot_words[:num_members]):
            if wd is not None:
                tab[g] = wd
        key = np.arange(self.n)
        want = {3: tab[self.ids[3], key[:, None]].reshape(-1), 8: tab[self.ids[8], key[:, None]].reshape(-1),
                "ragged": tab[self.rmember, np.repeat(key, self.counts)]}
        if self.all_k:
            assert self.all_k == num_members, tag
            want["all"] = np.ascontiguousarray(tab[:self.all_k].T).reshape(-1)
        for k, m in self.size.items():
            out = self.found[k].cpu().numpy()
            assert (out[m:] == -7).all(), (tag, k, "wrote past the found words")
            got = out[:m].view(np.uint64)
            bad = np.flatnonzero(got != want[k])
            assert bad.size == 0, (tag, k, bad.size, bad[:8].tolist(), got[bad[:4]], want[k][bad[:4]])
        return want


def probe_now(w, fs, names, tag, all_members=True, ph=None, words=None):
    """one round of probes on the current stream, waited for and compared"""
    p = Probes(w.ph if ph is None else ph, fs.capacity + 2, 1, all_k=fs.num_members if all_members else None)
    p.launch(fs)
    torch.cuda.synchronize()
    return p.check(words_of(w, names, words), fs.num_members, tag)


def einval(fn):
    with pytest.raises(E.PlatformStatusError) as ei:
        fn()
    assert ei.value.code == E.STATUS_BAD_PARAM


def fresh_batch(w, seed, n=5000, value=9, cfg=None):
    """a batch of one filter of n hashes, a quarter of the probes among them: (unbuilt batch, its
    hashes on the device, the oracle's words of the probes)"""
    rng = np.random.default_rng(seed)
    h = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    h[:len(w.ph[::4])] = w.ph[::4]
    words = w.oracle.filter_add(w.o8, h, value=value).lookup_hashes(w.ph)
    assert (words[::4] >> np.uint64(value) & np.uint64(1)).all()
    b = E.FilterBatch(cfg or w.cfg8, [n], [value])
    d_h = dev(h)
    torch.cuda.synchronize()
    return b, d_h, words


# ---- 1. replace and clear ----------------------------------------------------------------------
def test_replace_and_clear(world):
    w = world
    names = ["A0", "A1", None, "C0"]
    fs = E.FilterSet(members_of(w, names), capacity=8)
    assert (fs.capacity, fs.num_members) == (8, 4)
    probe_now(w, fs, names, "before")
    replaced = fs.update([1, 2, 0], members_of(w, ["D0", "A1", None]))
    assert replaced == [w.member["A1"], None, w.member["A0"]]
    assert fs.num_members == 4
    after = [None, "D0", "A1", "C0"]
    want = probe_now(w, fs, after, "after")
    assert want["all"].reshape(N, 4)[:, 3].tobytes() == w.words["C0"].tobytes()  # member 3 untouched
    assert want["all"].reshape(N, 4)[:, 1].any() and not want["all"].reshape(N, 4)[:, 0].any()
    fs.close()


# ---- 2. append ---------------------------------------------------------------------------------
def test_append(world):
    w = world
    names = ["A0", "A1", None, "C0"]
    fs = E.FilterSet(members_of(w, names), capacity=8)
    before = Probes(w.ph, 10, 2).launch(fs)
    torch.cuda.synchronize()
    before.check(words_of(w, names), 4, "before")
    assert (before.ids[8] == 7).any() and (before.rmember == 7).any()  # id 7 is probed, and finds nothing
    fs.update([6, 4], members_of(w, ["D0", "T17"]))
    assert fs.num_members == 7
    assert E.load_library().rf_amd_filter_set_num_members(fs.h) == 7
    names = ["A0", "A1", None, "C0", "T17", None, "D0", None]
    want = probe_now(w, fs, names, "appended")
    assert not want["all"].reshape(N, 7)[:, 5].any()  # slot 5 was never set
    # id 8 is the capacity: refused, and nothing has changed
    einval(lambda: fs.update([5, 8], members_of(w, ["A0", "A0"])))
    assert fs.num_members == 7 and fs.capacity == 8
    again = probe_now(w, fs, names, "after the refused call")
    assert all(again[k].tobytes() == want[k].tobytes() for k in want)
    fs.close()


# ---- 3. stream order, one synchronisation --------------------------------------------------------
def test_stream_order(world):
    w = world
    names = ["A0", "A1", None, "C0"]
    fs = E.FilterSet(members_of(w, names), capacity=8)
    b, d_h, xwords = fresh_batch(w, 31)
    p1, p2, p3 = (Probes(w.ph, 10, 30 + i, all_k=4) for i in range(3))
    S = torch.cuda.Stream()
    s = S.cuda_stream
    torch.cuda.synchronize()
    p1.launch(fs, stream=s)
    b.build_hashes(d_h, stream=s)
    old = fs.update([1], [(b, 0)], stream=s)
    p2.launch(fs, stream=s)
    fs.update([1], old, stream=s)
    p3.launch(fs, stream=s)
    S.synchronize()
    assert old == [w.member["A1"]]
    p1.check(words_of(w, names), 4, "before the update")
    p2.check([w.words["A0"], xwords, None, w.words["C0"]], 4, "between the updates")
    p3.check(words_of(w, names), 4, "after the update back")
    fs.close()
    b.close()


# ---- 4. error bits in stream order ---------------------------------------------------------------
@pytest.mark.parametrize("which", ["past", "limit"])
def test_error_bits_in_stream_order(world, which):
    """the member's build is queued, not finished, when the update is called: the host has never
    seen its error bits. Past the limit the member finds nothing although its keys are in the
    input; at the limit it finds every key."""
    w = world
    case = R.FRESH_BY_NAME["fp26_page"]
    assert (case.fp, case.lis, case.n, case.value) == (26, 8, 9000, 0)
    index = R.positions(case.nidx)["middle"]
    h = case.hashes(case.past if which == "past" else case.limit, index)
    ph = h[np.random.default_rng(4).integers(0, h.size, size=N)]
    words = {"A0": w.of["A0"].lookup_hashes(ph),
             "X": np.zeros(N, dtype=np.uint64) if which == "past" else w.oracle.filter_add(w.o8, h, value=0).lookup_hashes(ph)}
    fs = E.FilterSet(members_of(w, ["A0", None]), capacity=4)
    b = E.FilterBatch(w.cfg8, [case.n], [case.value])
    d_h = dev(h)
    p = Probes(ph, 6, 40, all_k=2)
    S = torch.cuda.Stream()
    s = S.cuda_stream
    torch.cuda.synchronize()
    b.build_hashes(d_h, stream=s)
    fs.update([1], [(b, 0)], stream=s)
    p.launch(fs, stream=s)
    S.synchronize()
    want = p.check([words["A0"], words["X"]], 2, which)
    member1 = want["all"].reshape(N, 2)[:, 1]
    if which == "past":
        assert not member1.any()
        assert b.info(0).error == case.bits
    else:
        assert (member1 & np.uint64(1)).all()  # value 0: every key of the input is found
        assert b.info(0).error == 0
    fs.close()
    b.close()


# ---- 5. more than one launch ---------------------------------------------------------------------
@pytest.mark.parametrize("count", [63, 64, 65, 150])
def test_more_than_one_launch(world, count):
    """one call names `count` filters of T at ids 0..count-1 in a shuffled order; 10 of the ids
    come a second time, and their earlier entries name other filters"""
    w = world
    rng = np.random.default_rng(count)
    fs = E.FilterSet([], capacity=160)
    assert (fs.capacity, fs.num_members) == (160, 0)
    ids = rng.permutation(count)
    final = {int(g): f"T{(int(g) * 7 + 3) % TF}" for g in ids}
    entries = [(int(g), final[int(g)]) for g in ids]
    # an earlier, losing entry of 10 ids, at a random place before the winning one
    for g in rng.choice(count, size=10, replace=False):
        at = [i for i, e in enumerate(entries) if e[0] == int(g)][-1]
        entries.insert(int(rng.integers(0, at + 1)), (int(g), f"T{(int(g) * 7 + 4) % TF}"))
    assert len(entries) == count + 10 and len(entries) > PER_LAUNCH
    replaced = fs.update([g for g, _ in entries], members_of(w, [nm for _, nm in entries]))
    assert replaced == [None] * len(entries)
    assert fs.num_members == count
    probe_now(w, fs, [final[g] for g in range(count)], ("launches", count))
    fs.close()


def test_single_entry_second_launch_range(world):
    """capacity 65, id 64 alone: the last slot of the table is written and nothing next to it"""
    w = world
    fs = E.FilterSet(members_of(w, ["A0"]), capacity=65)
    fs.update([64], members_of(w, ["T3"]))
    assert fs.num_members == 65
    probe_now(w, fs, ["A0"] + [None] * 63 + ["T3"], "id 64 of 65")
    fs.close()


# ---- 6. the seed rule follows the membership -----------------------------------------------------
def test_seed_rule(world):
    w = world
    names = ["A0", "A1", None]
    fs = E.FilterSet(members_of(w, names), capacity=4)
    cfg43 = E.routing_config_init(log_index_size=8, seed=43)
    b43, d_h, xwords = fresh_batch(w, 61, cfg=cfg43)
    b43.build_hashes(d_h)
    torch.cuda.synchronize()

    def keys_probe(names_now):
        found = torch.full((N * 3 + SENT,), -7, dtype=torch.int64, device="cuda:0")
        fs.probe_keys(dev(w.pk), 24, None, 3, N, found)
        torch.cuda.synchronize()
        out = found.cpu().numpy()
        assert (out[N * 3:] == -7).all()
        want = np.stack([np.zeros(N, dtype=np.uint64) if nm is None else w.kwords[nm] for nm in names_now], axis=1)
        assert (out[:N * 3].view(np.uint64).reshape(N, 3) == want).all(), names_now
        return want

    keys_probe(names)
    fs.update([2], [(b43, 0)])
    found = torch.zeros(N * 3, dtype=torch.int64, device="cuda:0")
    einval(lambda: fs.probe_keys(dev(w.pk), 24, None, 3, N, found))
    p = Probes(w.ph, 6, 60, all_k=3).launch(fs)
    torch.cuda.synchronize()
    p.check([w.words["A0"], w.words["A1"], xwords], 3, "a seed-43 member, hashes form")
    fs.update([2], members_of(w, ["C0"]))
    want = keys_probe(["A0", "A1", "C0"])
    assert want[:, 1].any() and want[:, 2].any()
    fs.close()
    b43.close()


# ---- 7. refusals ---------------------------------------------------------------------------------
def test_refusals(world):
    w = world
    L = E.load_library()
    names = ["A0", "A1", None, "C0"]
    fs = E.FilterSet(members_of(w, names), capacity=8)
    want = probe_now(w, fs, names, "before")
    unbuilt = E.FilterBatch(w.cfg8, [10], [0])
    one = np.array([5], dtype=np.uint32)
    import ctypes
    hs = (ctypes.c_void_p * 1)(w.A.h.value)
    refusals = {
        "unbuilt": lambda: fs.update([0, 5], [w.member["D0"], (unbuilt, 0)]),
        "filter index": lambda: fs.update([0, 5], [w.member["D0"], (w.A, 2)]),
        "null ids": lambda: E._check(L.rf_amd_filter_set_update(fs.h, None, ctypes.addressof(hs), None, 1, None)),
        "null batches": lambda: E._check(L.rf_amd_filter_set_update(fs.h, one.ctypes.data, None, None, 1, None)),
    }
    for tag, call in refusals.items():
        einval(call)
        assert (fs.num_members, L.rf_amd_filter_set_num_members(fs.h)) == (4, 4), tag
        again = probe_now(w, fs, names, tag)
        assert all(again[k].tobytes() == want[k].tobytes() for k in want), tag
    # the keys forms are as legal as before
    found = torch.zeros(N * 4, dtype=torch.int64, device="cuda:0")
    fs.probe_keys(dev(w.pk), 24, None, 4, N, found)
    torch.cuda.synchronize()
    assert (found.cpu().numpy().view(np.uint64).reshape(N, 4)[:, 1] == w.kwords["A1"]).all()
    # no entries: OK, with or without arrays
    assert fs.update([], []) == []
    assert L.rf_amd_filter_set_update(fs.h, None, None, None, 0, None) == 0
    assert fs.num_members == 4
    probe_now(w, fs, names, "after count == 0")
    unbuilt.close()
    fs.close()


# ---- 8. no allocation ----------------------------------------------------------------------------
def test_updates_do_not_allocate(world):
    w = world
    fs = E.FilterSet(members_of(w, ["A0", "A1"]), capacity=128)
    eng = E.default_engine()
    before = eng.pool_stats()
    for r in range(20):
        ids = [(r * 5 + j) % 128 for j in range(70)]
        fs.update(ids, members_of(w, [f"T{(g + r) % TF}" for g in ids]))
    after = eng.pool_stats()
    assert (after["hits"], after["misses"]) == (before["hits"], before["misses"])
    names = [None] * 128
    for r in range(20):
        for g in [(r * 5 + j) % 128 for j in range(70)]:
            names[g] = f"T{(g + r) % TF}"
    assert fs.num_members == 128
    probe_now(w, fs, names, "after 20 updates")
    fs.close()


# ---- 9. stream-ordered destroy -------------------------------------------------------------------
def test_close_on_stream(world):
    w = world
    n1, n2 = ["A0", "A1", None, "C0"], ["D0", "T5", "A1"]
    fs1 = E.FilterSet(members_of(w, n1), capacity=8)
    p1, p2 = Probes(w.ph, 10, 90, all_k=4), Probes(w.ph, 5, 91, all_k=3)
    S = torch.cuda.Stream()
    s = S.cuda_stream
    torch.cuda.synchronize()
    p1.launch(fs1, stream=s)
    fs1.close_on(s)
    assert fs1.h is None
    fs2 = E.FilterSet(members_of(w, n2))
    p2.launch(fs2, stream=s)
    S.synchronize()
    p1.check(words_of(w, n1), 4, "the set closed behind its probe")
    p2.check(words_of(w, n2), 3, "the set created after it")
    fs1.close()  # closed already: nothing to do
    fs2.close_on(s)
    S.synchronize()


# ---- 10. a trimmed member ------------------------------------------------------------------------
def test_trimmed_member(world):
    w = world
    b, d_h, xwords = fresh_batch(w, 101, n=20000, value=11)
    b.build_hashes(d_h)
    torch.cuda.synchronize()
    assert E.load_library().rf_amd_batch_trim(b.h, None) == 0
    # the released work buffers go back to the pool: a new build takes and overwrites them
    junk = E.FilterBatch(w.cfg8, [20000], [1])
    junk.build_hashes(dev(np.random.default_rng(102).integers(0, 1 << 32, size=20000, dtype=np.uint64).astype(np.uint32)))
    torch.cuda.synchronize()
    fs = E.FilterSet(members_of(w, ["A0", None]), capacity=2)
    fs.update([1], [(b, 0)])
    p = Probes(w.ph, 4, 100, all_k=2).launch(fs)
    torch.cuda.synchronize()
    p.check([w.words["A0"], xwords], 2, "a trimmed member")
    fs.close()
    junk.close()
    b.close()
