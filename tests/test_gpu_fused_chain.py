"""Fused chain add (rf_amd_batch_create_runs / FilterBatch.chained): the k routing_filter_add
rounds of a compaction chain (src/trunk.c:3815-3868 keeps only the chain's last filter) built
as ONE build over all k runs, each entry tagged with its run's value.

Checker: the reference's own chain (oracle/_ref/libref_rf.so), run 0 added onto the base
filter, run 1 onto that, ... -- pages, slots, num_fingerprints, num_unique, value_size and
num_pages of the last filter compared exactly. Config is fp 26, lis 8 unless noted; batches
hold 2-3 filters. A case's inputs and reference chain are computed once and shared.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLD
from oracle import refimpl as R
from splinterdb_amd import engine as E
from splinterdb_amd import keys as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

needs_ref = pytest.mark.skipif(not R.available(), reason="reference library not built")
NEVER = 20000  # never-inserted ids probed per filter


def chain_ids(g, v, n):
    return (np.uint64(g) << np.uint64(32)) + np.uint64(v + 1) * np.arange(n, dtype=np.uint64)


def rand_ids(rng, n):
    return rng.integers(0, 1 << 62, size=n, dtype=np.uint64)


class Case:
    """ids[f][j] = the ids of run j of filter f, values[j] its value; base = (ids per filter,
    value) of a filter the chain starts from, or None"""

    def __init__(self, ids, values, base=None, lis=8):
        self.ids, self.values, self.base, self.lis = ids, list(values), base, lis
        self.F = len(ids)
        self.cfg = E.routing_config_init(fingerprint_size=26, log_index_size=lis, seed=42)
        self.runs = [[(int(a.size), v) for a, v in zip(ids[f], self.values)] for f in range(self.F)]
        # build input: filter-major, run-minor
        self.keys = np.concatenate([K.ids_keys(a) for f in range(self.F) for a in ids[f]])
        self.want = self.descs = None

    def reference(self, ref):
        """the reference's chain per filter (once): last descriptors and their images"""
        if self.want is None:
            self.descs, self.base_descs = [], []
            for f in range(self.F):
                d = None
                if self.base is not None:
                    d = ref.add(ref.hash_keys(K.ids_keys(self.base[0][f])), value=self.base[1])
                self.base_descs.append(d)
                for a, v in zip(self.ids[f], self.values):
                    d = ref.add(ref.hash_keys(K.ids_keys(a)), value=v, old=d)
                self.descs.append(d)
            self.want = [ref.image(d) for d in self.descs]
        return self.want

    def base_batch(self, eng):
        n = [int(a.size) for a in self.base[0]]
        b = E.FilterBatch(self.cfg, n, [self.base[1]] * self.F, engine=eng)
        b.build_keys(torch.from_numpy(np.concatenate([K.ids_keys(a) for a in self.base[0]]).reshape(-1)).to("cuda:0"), 24)
        return b

    def fused(self, eng):
        """the fused batch; release() closes it and its base batch (no batch may outlive the
        engine, and the cases are cached for the module's lifetime: they hold none)"""
        old = base_b = None
        if self.base is not None:
            base_b = self.base_batch(eng)
            old = [(base_b, f) for f in range(self.F)]
        b = E.FilterBatch.chained(self.cfg, self.runs, old=old, engine=eng)
        b.build_keys(torch.from_numpy(self.keys.reshape(-1)).to("cuda:0"), 24)
        torch.cuda.synchronize()
        b.base_batch = base_b
        return b


def release(b):
    base_b = getattr(b, "base_batch", None)
    b.close()
    if base_b is not None:
        base_b.close()


def make_case(name):
    rng = np.random.default_rng(0xC4A1)
    if name == "equal5":  # 1: overlapping keys across runs; npo_last = 1 (80,000 -> 100,000)
        return Case([[chain_ids(g, v, 20000) for v in range(5)] for g in range(3)], range(5))
    if name == "npo2":  # 2: 60,000 -> 80,000 crosses 2^16
        return Case([[chain_ids(g, v, 20000) for v in range(4)] for g in range(2)], range(4))
    if name == "npo8":  # 3: 30,000 -> 140,000: 2^14 -> 2^17 buckets
        return Case([[rand_ids(rng, n) for n in (10000, 20000, 110000)] for _ in range(2)], (1, 2, 5))
    if name == "ragged":  # 4: tile cuts at run boundaries, around TILE_KEYS = 16384
        return Case([[rand_ids(rng, n) for n in (1, 16384, 16385, 40000)] for _ in range(2)], (0, 1, 2, 3))
    if name == "dups":  # 5: within-run dedupe, cross-run keep
        ids = []
        for _ in range(2):
            a = rand_ids(rng, 10000)
            twice = rng.permutation(np.concatenate([a, a]))
            ids.append([twice, rng.permutation(np.concatenate([a, rand_ids(rng, 10000)]))])
        return Case(ids, (2, 3))
    if name == "base":  # 6: 40,000 + 3 x 20,000
        return Case([[chain_ids(g, v, 20000) for v in (1, 2, 3)] for g in range(2)], (1, 2, 3),
                    base=([chain_ids(g, 0, 40000) for g in range(2)], 0))
    if name == "wide":  # 7: value_size 5 -> 6; 26 + 6 = 32 forces 64-bit entries
        return Case([[rand_ids(rng, 20000) for _ in range(4)] for _ in range(2)], (30, 31, 32, 33),
                    base=([rand_ids(rng, 20000) for _ in range(2)], 29))
    if name == "lis9":  # 9: library default geometry; 60,000 -> 90,000 crosses 2^16
        return Case([[rand_ids(rng, 30000) for _ in range(3)] for _ in range(2)], (0, 1, 2), lis=9)
    raise KeyError(name)


_cases = {}


def get_case(name):
    if name not in _cases:
        _cases[name] = make_case(name)
    return _cases[name]


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ref():
    with R.Stack() as s:
        yield s


def assert_same(b, f, want, desc):
    img = b.image(f)
    got = (img.num_fingerprints, img.num_unique, img.value_size, img.num_pages)
    exp = (desc.num_fingerprints, desc.num_unique, desc.value_size, want.num_pages)
    assert got == exp, (f, got, exp)
    assert img.pages.size == want.pages.size and (img.pages == want.pages).all(), f
    assert (img.slots == want.slots).all(), f


def check_case(c, ref, eng):
    want = c.reference(ref)
    b = c.fused(eng)
    for f in range(c.F):
        assert_same(b, f, want[f], c.descs[f])
    return b


@needs_ref
@pytest.mark.parametrize("name", ["equal5", "npo2", "npo8", "ragged", "dups"])
def test_fused_chain_matches_reference(name, ref, eng):
    """cases 1-5: no base filter (the 32-bit pipeline without old/new flags)"""
    release(check_case(get_case(name), ref, eng))


@needs_ref
@pytest.mark.parametrize("entries", ["in_place", "decode", "wide64"])
def test_fused_chain_onto_base_filter(entries, ref, eng, monkeypatch):
    """case 6: all three old-entry pipelines"""
    if entries == "decode":
        monkeypatch.setenv("RF_AMD_OLD_DECODE", "1")
    if entries == "wide64":
        monkeypatch.setenv("RF_AMD_WIDE64", "1")
    release(check_case(get_case("base"), ref, eng))


@needs_ref
def test_fused_chain_value_size_grows(ref, eng):
    """case 7: values 30..33 onto a value-29 base; 64-bit entries without an env switch"""
    c = get_case("wide")
    b = check_case(c, ref, eng)
    assert b.info(0).value_size == 6
    release(b)


@needs_ref
def test_fused_chain_spill(ref, eng):
    """case 8: 60,000 copies of 50 keys whose fingerprints share their top bits (one coarse
    bucket far over its region: the exact count/scan/scatter fallback and K4b), then a
    normal run; the second filter of the batch has no duplicates"""
    rng = np.random.default_rng(8)
    cand = np.arange(1, 8001, dtype=np.uint64)
    h = ref.hash_keys(K.ids_keys(cand))
    hot = cand[(h >> np.uint32(28)) == 3][:50]
    assert hot.size == 50
    ids = [[rng.permutation(np.tile(hot, 1200)), rand_ids(rng, 20000)],
           [rand_ids(rng, 60000), rand_ids(rng, 20000)]]
    release(check_case(Case(ids, (1, 4)), ref, eng))


@needs_ref
def test_fused_chain_lis9(eng):
    """case 9: the library's default log_index_size"""
    with R.Stack(log_index_size=9) as ref9:
        release(check_case(get_case("lis9"), ref9, eng))


def test_single_run_equals_plain_batch(eng):
    """case 10: k = 1 gives the bytes of FilterBatch(...) of today"""
    cfg = E.routing_config_init(fingerprint_size=26, log_index_size=8, seed=42)
    n, vals = [30000, 17000], [0, 3]
    dk = torch.from_numpy(K.random_keys(sum(n), seed=10).reshape(-1)).to("cuda:0")
    a = E.FilterBatch(cfg, n, vals, engine=eng)
    b = E.FilterBatch.chained(cfg, [[(n[0], vals[0])], [(n[1], vals[1])]], engine=eng)
    a.build_keys(dk, 24)
    b.build_keys(dk, 24)
    torch.cuda.synchronize()
    for f in range(2):
        x, y = a.image(f), b.image(f)
        assert (x.num_fingerprints, x.num_unique, x.value_size, x.num_pages) == \
            (y.num_fingerprints, y.num_unique, y.value_size, y.num_pages)
        assert (x.pages == y.pages).all() and (x.slots == y.slots).all()
    a.close()
    b.close()


@needs_ref
def test_fused_result_as_old_filter(ref, eng):
    """case 11: a single add on top of case 1's fused batch (its sorted entries read in place)"""
    c = get_case("equal5")
    c.reference(ref)
    fused = c.fused(eng)
    n, v = 20000, 5
    ids = [chain_ids(g, v, n) for g in range(c.F)]
    b = E.FilterBatch(c.cfg, [n] * c.F, [v] * c.F, old=[(fused, f) for f in range(c.F)], engine=eng)
    b.build_keys(torch.from_numpy(np.concatenate([K.ids_keys(a) for a in ids]).reshape(-1)).to("cuda:0"), 24)
    torch.cuda.synchronize()
    for f in range(c.F):
        d = ref.add(ref.hash_keys(K.ids_keys(ids[f])), value=v, old=c.descs[f])
        assert_same(b, f, ref.image(d), d)
    b.close()
    release(fused)


@needs_ref
@pytest.mark.parametrize("name", ["equal5", "npo8", "wide"])
def test_fused_chain_probes(name, ref, eng):
    """case 12: every run's keys plus never-inserted ids == ref.lookup_keys, word for word"""
    c = get_case(name)
    c.reference(ref)
    b = c.fused(eng)
    rng = np.random.default_rng(12)
    per = [np.concatenate([K.ids_keys(a) for a in c.ids[f]] +
                          [K.ids_keys(rng.integers(1 << 62, 1 << 63, size=NEVER, dtype=np.uint64))])
           for f in range(c.F)]
    counts = [p.shape[0] for p in per]
    found = torch.empty(sum(counts), dtype=torch.int64, device="cuda:0")
    b.probe_keys_runs(torch.from_numpy(np.concatenate(per).reshape(-1)).to("cuda:0"), 24, counts, found)
    got = found.cpu().numpy().view(np.uint64)
    at = 0
    for f in range(c.F):
        want = ref.lookup_keys(c.descs[f], per[f])
        assert (got[at:at + counts[f]] == want).all(), f
        at += counts[f]
    release(b)


def test_fused_chain_golden(eng):
    """case 13: filters 0 and 1 of the 8 x (2^20-1) compaction chains the reference built"""
    with open(os.path.join(GOLD, "sha256.json")) as fh:
        gold = json.load(fh)
    F, V, n = 2, 8, (1 << 20) - 1
    cfg = E.routing_config_init(fingerprint_size=26, log_index_size=8, seed=42)
    gid = torch.arange(F, device="cuda:0", dtype=torch.int64)[:, None, None] << 32
    vv = torch.arange(1, V + 1, device="cuda:0", dtype=torch.int64)[None, :, None]
    j = torch.arange(n, device="cuda:0", dtype=torch.int64)[None, None, :]
    keys = K.ids_keys_torch((gid + vv * j).reshape(-1), 24)
    b = E.FilterBatch.chained(cfg, [[(n, v) for v in range(V)]] * F, engine=eng)
    b.build_keys(keys, 24)
    torch.cuda.synchronize()
    for f in range(F):
        g = gold[f"chain_f{f}_v{V}_n{n}_lis8"]
        img = b.image(f)
        assert (img.num_fingerprints, img.num_unique, img.num_pages) == \
            (g["num_fingerprints"], g["num_unique"], g["num_pages"])
        assert hashlib.sha256(img.pages.tobytes()).hexdigest() == g["pages_sha256"], f
        assert hashlib.sha256(img.slots.tobytes()).hexdigest() == g["slots_sha256"], f
    assert b.info(0).num_unique == 4254486
    b.close()


def test_fused_chain_errors(eng):
    """case 14: every EINVAL case, raised when the batch is created"""
    cfg = E.routing_config_init(fingerprint_size=26, log_index_size=8, seed=42)
    base = E.FilterBatch(cfg, [1000], [9], engine=eng)  # value_size 4
    base.build_keys(torch.from_numpy(K.random_keys(1000, seed=14).reshape(-1)).to("cuda:0"), 24)
    torch.cuda.synchronize()
    bad = [
        ([[(100, 1), (100, 1)]], None),                     # values not strictly increasing
        ([[(100, 2), (100, 1)]], None),
        ([[(100, 0), (100, 1)], [(100, 3), (50, 2)]], None),  # ... in a later filter
        ([[(100, 7), (100, 12)]], [(base, 0)]),             # bits(v_0) = 3 < old value_size 4
        ([[(100, 0), (0, 1)]], None),                       # zero-length run
        ([[(8388607, 0), (1, 1)]], None),                   # total over routing_filter_max_fingerprints
        ([[(100, 1), (100, 64)]], None),                    # 26 + bits(64) = 33 > 32
    ]
    for runs, old in bad:
        with pytest.raises(E.PlatformStatusError) as ei:
            E.FilterBatch.chained(cfg, runs, old=old, engine=eng)
        assert ei.value.code == E.STATUS_BAD_PARAM, runs
    E.FilterBatch.chained(cfg, [[(100, 8), (100, 12)]], old=[(base, 0)], engine=eng).close()
    base.close()


@needs_ref
def test_host_form_add_runs(ref, eng):
    """case 15: routing_filter_add_runs (host images in and out) on case 6's data"""
    c = get_case("base")
    want = c.reference(ref)
    for f in range(c.F):
        old = E.routing_filter_add(c.cfg, None, ref.hash_keys(K.ids_keys(c.base[0][f])), c.base[1], engine=eng)
        img = E.routing_filter_add_runs(c.cfg, old, [ref.hash_keys(K.ids_keys(a)) for a in c.ids[f]], c.values,
                                        engine=eng)
        d = c.descs[f]
        assert (img.num_fingerprints, img.num_unique, img.value_size, img.num_pages) == \
            (d.num_fingerprints, d.num_unique, d.value_size, want[f].num_pages)
        assert (img.pages == want[f].pages).all() and (img.slots == want[f].slots).all()
