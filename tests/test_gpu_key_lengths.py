"""Key-length and alignment sweep of every kernel that hashes fixed-length keys on the device.

fixed_kind() (splinterdb_amd/csrc/rf_plan.h) picks one of three readers from the key length
and the alignment of the key buffer's base:
  IN_KEYS24  length 24, base 8-byte aligned (the probe kernels stage the keys through LDS only when
             the base is also 16-byte aligned: full waves by LDS-DMA, a ragged wave by plain loads
             that end on an 8-byte half for an odd key count),
  IN_KEYS_W  length % 4 == 0, base 4-byte aligned (xxh32_words),
  IN_KEYS_B  everything else (xxh32_unaligned; k_hash, k_probe and k_probe_fanout take
             xxh32_unaligned_prefetch for 16..128 bytes, with its own tail decoder).

The reference throughout is the CPU oracle (oracle.hash_fixed, oracle.filter_add chained through
old=, OracleFilter.lookup_hashes); every comparison is exact equality.

A shifted base is a slice at byte offset s of a device uint8 tensor whose own base is 256-byte
aligned (asserted), so s is the alignment of the keys. The bytes around the keys are 0xEE, not
zero: a hash that took in a byte from outside its key would differ from the oracle's.
"""
import numpy as np
import pytest

from splinterdb_amd import engine as E
from splinterdb_amd import keys as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILE_KEYS = 16384  # RF_TILE_KEYS (splinterdb_amd/csrc/rf_plan.h): keys per partition tile
LIS = 8
SENT32 = 0x5A5A5A5A
SENT64 = -7
PAD = 64  # sentinel words after every output

# (a) every tail residue 0..15 with 0, 1 and 2 stripes, then both sides of every stripe count up
# to 8 (16 * k - 1, 16 * k, 16 * k + 1), the 128/129 edge of xxh32_unaligned_prefetch, and beyond
HASH_LENS = list(range(1, 41)) + [47, 48, 49, 63, 64, 65, 79, 80, 81, 111, 112, 113, 127, 128, 129, 130,
                                  143, 144, 145, 255, 256, 257]
HASH_SHIFTS = [0, 1, 2, 4, 8]
HASH_N = 357  # one full 256-thread block, one full wave, one ragged wave

# (b), (c): (key length, base shift). Length 24: the 16-aligned default, IN_KEYS24 at a base that is
# 8- but not 16-byte aligned, IN_KEYS_W, IN_KEYS_B.
KEY_CASES = [(n, 0) for n in (3, 4, 7, 8, 12, 15, 16, 17, 20, 23, 25, 28, 31, 32, 33, 48, 49, 100, 127, 128, 129)]
KEY_CASES += [(24, 0), (24, 8), (24, 4), (24, 1)]
FANOUT_CASES = [(17, 0), (31, 0), (49, 0), (129, 0), (24, 8), (24, 4)]
HOST_LENS = [7, 17, 40]


def case_id(c):
    return f"len{c[0]}_shift{c[1]}"


def dev(a):
    return torch.from_numpy(np.array(a)).to("cuda:0")  # a copy: the shared inputs are read-only


def place(host, shift):
    """`host` (uint8) at byte offset `shift` of a fresh device buffer with 16 spare bytes after it"""
    flat = np.array(host, dtype=np.uint8).reshape(-1)
    buf = torch.full((shift + flat.size + 16,), 0xEE, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 256 == 0
    view = buf[shift:shift + flat.size]
    view.copy_(torch.from_numpy(flat))
    assert view.data_ptr() == buf.data_ptr() + shift
    return view


def expected_kind(key_len, shift):
    """fixed_kind() of a base whose alignment is `shift` (0: 256 bytes)"""
    if key_len == 24 and shift % 8 == 0:
        return "IN_KEYS24"
    if key_len % 4 == 0 and shift % 4 == 0:
        return "IN_KEYS_W"
    return "IN_KEYS_B"


def test_cases_reach_every_reader():
    """the lists above against the dispatch they are meant to cover (no device work)"""
    kinds = {expected_kind(n, s) for n in HASH_LENS for s in HASH_SHIFTS}
    assert kinds == {"IN_KEYS24", "IN_KEYS_W", "IN_KEYS_B"}
    assert {n % 16 for n in HASH_LENS if 16 <= n <= 128} == set(range(16))  # every tail residue, prefetch form
    assert {n // 16 for n in HASH_LENS if 16 <= n <= 128} == set(range(1, 9))  # stripe counts 1..8
    assert {128, 129} <= set(HASH_LENS)
    assert [expected_kind(*c) for c in KEY_CASES[-4:]] == ["IN_KEYS24", "IN_KEYS24", "IN_KEYS_W", "IN_KEYS_B"]
    assert {expected_kind(*c) for c in KEY_CASES[:-4]} == {"IN_KEYS_W", "IN_KEYS_B"}


# ---- (a) rf_amd_hash_keys -------------------------------------------------------------------
@pytest.mark.parametrize("key_len", HASH_LENS, ids=lambda n: f"len{n}")
def test_hash_keys(oracle, key_len):
    """k_hash<KIND>: shifts 0, 1, 2, 4, 8 at seed 42, seeds 0 and 0xFFFFFFFF at shift 0; every launch
    of the length is issued before the one synchronisation"""
    keys = K.random_keys(HASH_N, key_len=key_len, seed=100 + key_len)
    runs = [(s, 42) for s in HASH_SHIFTS] + [(0, 0), (0, 0xFFFFFFFF)]
    outs = []
    for shift, seed in runs:
        d_keys = place(keys, shift)
        out = torch.full((HASH_N + PAD,), SENT32, dtype=torch.int32, device="cuda:0")
        E.hash_keys(E.routing_config_init(seed=seed), d_keys, key_len, HASH_N, out)
        outs.append((d_keys, out))
    torch.cuda.synchronize()
    want = {seed: oracle.hash_fixed(keys.reshape(-1), key_len, seed=seed) for seed in (42, 0, 0xFFFFFFFF)}
    for (shift, seed), (_, out) in zip(runs, outs):
        got = out.cpu().numpy()
        assert (got[HASH_N:] == SENT32).all(), (key_len, shift, seed, "wrote past d_hashes[n)")
        bad = np.flatnonzero(got[:HASH_N].view(np.uint32) != want[seed])
        assert bad.size == 0, (key_len, shift, seed, expected_kind(key_len, shift), bad.size, bad[:8].tolist())


# ---- (b) builds from fixed-length keys --------------------------------------------------------
class BuildData:
    """the keys and oracle filters of one key length (shared by its shifts and forms, read-only)"""

    def __init__(self, oracle, key_len):
        rng = np.random.default_rng(key_len)
        self.ocfg = oracle.make_config(log_index_size=LIS)
        self.oracle = oracle

        def hashed(keys):
            keys.setflags(write=False)
            return keys, oracle.hash_fixed(keys.reshape(-1), key_len)
        # fresh: a full tile, a ragged tile and a tiny filter whose keys start mid-buffer
        self.fresh_sizes, self.fresh_values = [TILE_KEYS + 37, 5], [0, 3]
        self.fresh_keys, self.fresh_h = hashed(K.random_keys(sum(self.fresh_sizes), key_len=key_len, seed=1000 + key_len))
        self.fresh_of = self.filters(self.fresh_h, self.fresh_sizes, self.fresh_values, None)
        # incremental: a tenth of filter 0's new keys repeat its old keys
        self.inc_sizes = [3001, 1]
        new = K.random_keys(sum(self.inc_sizes), key_len=key_len, seed=2000 + key_len)
        rep = rng.choice(3001, size=300, replace=False)
        new[rep] = self.fresh_keys[rng.integers(0, self.fresh_sizes[0], size=300)]
        self.inc_keys, self.inc_h = hashed(new)
        # chained: runs of 700, 1 and 1300 keys per filter
        self.chain_runs = [[(700, 1), (1, 2), (1300, 5)], [(700, 0), (1, 3), (1300, 4)]]
        self.chain_keys, self.chain_h = hashed(K.random_keys(2 * 2001, key_len=key_len, seed=3000 + key_len))

    def filters(self, h, sizes, values, olds):
        out, s = [], 0
        for f, (n, v) in enumerate(zip(sizes, values)):
            out.append(self.oracle.filter_add(self.ocfg, h[s:s + n], value=v, old=olds[f] if olds else None))
            s += n
        return out

    def chain_filters(self):
        out, s = [], 0
        for runs in self.chain_runs:
            of = None
            for n, v in runs:
                of = self.oracle.filter_add(self.ocfg, self.chain_h[s:s + n], value=v, old=of)
                s += n
            out.append(of)
        return out


_build_data = {}


def build_data(oracle, key_len):
    if key_len not in _build_data:
        _build_data[key_len] = BuildData(oracle, key_len)
    return _build_data[key_len]


def assert_batch_equals(batch, ofs, what):
    for f, of in enumerate(ofs):
        inf = batch.info(f)
        assert inf.error == 0, (what, f, inf.error)
        got = (inf.num_fingerprints, inf.num_unique, inf.value_size, inf.num_indices, inf.num_pages)
        want = (of.num_fingerprints, of.num_unique, of.value_size, of.num_indices, of.num_pages)
        assert got == want, (what, f, got, want)
        img = batch.image(f)
        assert (img.pages == of.pages()).all(), (what, f, "page bytes differ from the oracle")
        assert (img.slots == of.slots()[: of.num_indices]).all(), (what, f, "index slots differ from the oracle")


@pytest.mark.parametrize("form", ["fresh", "incremental", "chained"])
@pytest.mark.parametrize("case", KEY_CASES, ids=case_id)
def test_build_keys(oracle, case, form):
    """rf_amd_batch_build_keys with KIND = fixed_kind(base, key length); fingerprint size 26. The
    partition kernels each form reaches (launch_build_t in rf_kernels.hip, by way of do_build):
      fresh        k_hash_scatter<KIND, FL = false, RUNS = false> (k_hash_count<KIND, uint32_t> is
                   launched behind it as the spill fallback and returns at once);
      incremental  values 4 and 6 (26 + value_size <= 31: 32-bit flagged entries)
                   k_hash_scatter<KIND, FL = true, RUNS = false>, then values 33 and 40
                   (value_size 6: 64-bit entries) k_hash_count<KIND, uint64_t, FL = true>;
      chained      k_hash_scatter<KIND, FL = false, RUNS = true>.
    Pages, slots and info (num_unique included) of every filter equal the oracle's."""
    key_len, shift = case
    d = build_data(oracle, key_len)
    cfg = E.routing_config_init(log_index_size=LIS)
    what = (key_len, shift, expected_kind(key_len, shift), form)
    batches = []
    try:
        if form in ("fresh", "incremental"):
            fresh = E.FilterBatch(cfg, d.fresh_sizes, d.fresh_values)
            batches.append(fresh)
            fk = place(d.fresh_keys, shift)
            fresh.build_keys(fk, key_len)
        if form == "fresh":
            torch.cuda.synchronize()
            assert_batch_equals(fresh, d.fresh_of, what)
        elif form == "incremental":
            nk = place(d.inc_keys, shift)
            for values in ([4, 6], [33, 40]):
                inc = E.FilterBatch(cfg, d.inc_sizes, values, old=[(fresh, 0), (fresh, 1)])
                batches.append(inc)
                inc.build_keys(nk, key_len)
                torch.cuda.synchronize()
                assert_batch_equals(inc, d.filters(d.inc_h, d.inc_sizes, values, d.fresh_of), what + (tuple(values),))
        else:
            ch = E.FilterBatch.chained(cfg, d.chain_runs)
            batches.append(ch)
            ck = place(d.chain_keys, shift)
            ch.build_keys(ck, key_len)
            torch.cuda.synchronize()
            assert_batch_equals(ch, d.chain_filters(), what)
    finally:
        torch.cuda.synchronize()
        for b in reversed(batches):
            b.close()


# ---- (c) probes with fixed-length keys --------------------------------------------------------
NPROBE = 300  # host forms; the device forms take the first 287


class ProbeWorld:
    """one key length: a two-filter batch built from the oracle's hashes of its keys, the probes
    (even positions: an inserted key of the probe's filter; odd: a random key; filter ids in blocks
    of 5) and the oracle's word of every probe in both filters"""

    def __init__(self, oracle, key_len):
        self.key_len = key_len
        self.cfg = E.routing_config_init(log_index_size=LIS)
        ocfg = oracle.make_config(log_index_size=LIS)
        self.sizes, self.values = [3000, 2000], [1, 6]
        self.ins = K.random_keys(sum(self.sizes), key_len=key_len, seed=4000 + key_len)
        h = oracle.hash_fixed(self.ins.reshape(-1), key_len)
        self.batch = E.FilterBatch(self.cfg, self.sizes, self.values)
        self.batch.build_hashes(dev(h))
        torch.cuda.synchronize()
        self.ofs = [oracle.filter_add(ocfg, h[:3000], value=1), oracle.filter_add(ocfg, h[3000:], value=6)]
        i = np.arange(NPROBE)
        self.fid = ((i // 5) % 2).astype(np.uint32)
        pk = K.random_keys(NPROBE, key_len=key_len, seed=5000 + key_len)
        even = i[::2]
        pk[even] = self.ins[self.fid[even] * 3000 + (even * 7) % 2000]
        self.pk = pk
        ph = oracle.hash_fixed(pk.reshape(-1), key_len)
        self.words = np.stack([of.lookup_hashes(ph) for of in self.ofs])  # [filter, probe]
        self.want = np.where(self.fid == 0, self.words[0], self.words[1])
        bit = np.array(self.values, dtype=np.uint64)[self.fid[even]]
        assert ((self.want[even] >> bit) & np.uint64(1)).all()  # the inserted keys are found
        for a in (self.ins, self.pk, self.fid, self.words, self.want):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def probe_world(oracle):
    worlds = {}

    def get(key_len):
        if key_len not in worlds:
            worlds[key_len] = ProbeWorld(oracle, key_len)
        return worlds[key_len]
    yield get
    torch.cuda.synchronize()
    for w in worlds.values():
        w.batch.close()


def new_found(n):
    return torch.full((n + PAD,), SENT64, dtype=torch.int64, device="cuda:0")


def read_found(found, n, what):
    out = found.cpu().numpy()
    assert (out[n:] == SENT64).all(), (what, "wrote past d_found[n)")
    return out[:n].view(np.uint64)


@pytest.mark.parametrize("case", KEY_CASES, ids=case_id)
def test_probe_keys(probe_world, case):
    """k_probe<KIND> with per-probe filter ids, n = 1, 2, 63, 64, 65, 287: for 24-byte keys at a
    16-byte aligned base the ragged staging at odd and even counts (the last probe of an odd count
    is an inserted key, which the 8-byte half must hash right to be found) and the full-wave
    LDS-DMA form; at shift 8 the branch that skips the staging"""
    key_len, shift = case
    w = probe_world(key_len)
    d_keys, d_fid = place(w.pk, shift), dev(w.fid)
    ns = [1, 2, 63, 64, 65, 287]
    founds = [new_found(n) for n in ns]
    for n, found in zip(ns, founds):
        w.batch.probe_keys(d_keys, key_len, d_fid, n, found)
    torch.cuda.synchronize()
    for n, found in zip(ns, founds):
        got = read_found(found, n, (case, n))
        bad = np.flatnonzero(got != w.want[:n])
        assert bad.size == 0, (case, expected_kind(*case), n, bad[:8].tolist(), got[bad[:4]], w.want[bad[:4]])


@pytest.mark.parametrize("case", KEY_CASES, ids=case_id)
def test_probe_keys_runs(probe_world, case):
    """k_probe<KIND> with the filter taken from the probe's position (for 24-byte keys at a
    16-byte aligned base, whole waves of one filter take probe_fast): against the oracle and
    against the per-id form"""
    key_len, shift = case
    w = probe_world(key_len)
    n = 287
    d_keys = place(w.pk, shift)
    for counts in ([65, 222], [0, 287]):
        fid = np.repeat(np.arange(2, dtype=np.uint32), counts)
        by_runs, by_ids = new_found(n), new_found(n)
        w.batch.probe_keys_runs(d_keys, key_len, counts, by_runs)
        w.batch.probe_keys(d_keys, key_len, dev(fid), n, by_ids)
        torch.cuda.synchronize()
        want = np.where(fid == 0, w.words[0, :n], w.words[1, :n])
        got = read_found(by_runs, n, (case, counts))
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (case, expected_kind(*case), counts, bad[:8].tolist(), got[bad[:4]], want[bad[:4]])
        assert (read_found(by_ids, n, (case, counts, "ids")) == got).all(), (case, counts)


@pytest.mark.parametrize("case", FANOUT_CASES, ids=case_id)
def test_fanout_probe_keys(probe_world, case):
    """k_probe_fanout<KIND>, K = 2: every member, and member lists with ids past the end"""
    key_len, shift = case
    w = probe_world(key_len)
    n, kk = 287, 2
    fs = E.FilterSet([(w.batch, 0), (w.batch, 1)])
    try:
        d_keys = place(w.pk, shift)
        i = np.arange(n)
        member = np.stack([i % 3, (i + 1) % 4], axis=1).astype(np.uint32)  # ids 2 and 3 are past the end
        all_found, list_found = new_found(n * kk), new_found(n * kk)
        fs.probe_keys(d_keys, key_len, None, kk, n, all_found)
        fs.probe_keys(d_keys, key_len, dev(member.reshape(-1)), kk, n, list_found)
        torch.cuda.synchronize()
        got = read_found(all_found, n * kk, (case, "all")).reshape(n, kk)
        assert (got == w.words[:, :n].T).all(), (case, expected_kind(*case), int((got != w.words[:, :n].T).sum()))
        ok = member < 2
        want = np.where(ok, w.words[np.where(ok, member, 0), i[:, None]], np.uint64(0))
        got = read_found(list_found, n * kk, (case, "list")).reshape(n, kk)
        assert (got == want).all(), (case, expected_kind(*case), int((got != want).sum()))
    finally:
        torch.cuda.synchronize()
        fs.close()


@pytest.mark.parametrize("key_len", HOST_LENS, ids=lambda n: f"len{n}")
def test_host_key_lookups(probe_world, key_len):
    """the routing_filter.h boundary with host keys: rf_amd_lookup_async, rf_amd_filter_lookup_keys
    and rf_amd_filter_verify funnel into the same k_probe instantiations"""
    w = probe_world(key_len)
    la = E.LookupAsync(w.batch, w.pk, w.fid)
    try:
        assert (la.wait() == w.want).all()
    finally:
        la.close()
    img = w.batch.image(0)
    assert (E.routing_filter_lookup_keys(w.cfg, img, w.pk) == w.words[0]).all()
    own = w.ins[:NPROBE]
    assert E.routing_filter_verify(w.cfg, img, own, w.values[0]) == 0
    with pytest.raises(E.PlatformStatusError) as ei:
        E.routing_filter_verify(w.cfg, img, own, w.values[0] + 1)
    assert ei.value.code == E.STATUS_BAD_PARAM and ei.value.num_missing == NPROBE
