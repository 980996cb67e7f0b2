"""Dense probe lines on the device (tests/probe_dense_cases.py; the CPU side is
tests/test_probe_dense_cases.py): RF_AMD_LINES_DENSE=1 forces the format on small filters of rvs 4,
6, 7 (value bits) and 10, a group size that does not divide the index, an incremental build and
lines that clusters overflow; rf_amd_diag_dense_line_filters proves that every build took it.

The lines K6 cuts, the lines k_plines re-cuts and the lines of an imported batch equal the numpy
restatement byte for byte. Every found word of 200,000 probes per filter (half inserted, half
never inserted) through each lookup path equals the oracle's routing_filter_lookup. With the knob
unset only a filter whose line table outgrows one XCD's L2 goes dense."""
import ctypes

import numpy as np
import pytest

import host_lookup_cases as H
import probe_dense_cases as D
import probe_geometry_cases as P
from splinterdb_amd import engine as E
from splinterdb_amd import keys as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT, PAD = H.SENT, H.PAD
SENT_I64 = SENT - (1 << 64)
# the cases of one (fp, lis) share a batch, a chain is a batch of its own
BATCHES = {}
for _c in D.CASES:
    BATCHES.setdefault((_c.name,) if _c.recipe == "chain" else (_c.fp, _c.lis), []).append(_c)
BATCHES = list(BATCHES.values())
BATCH_IDS = ["+".join(c.name for c in cs) for cs in BATCHES]
# the key-input paths (24-byte and variable-length keys) run on the cases built from keys; the
# chain and the clustered case are made of raw hashes that no key hashes to, so they go through
# every hash-input path only (a key path differs from its hash path by the hashing alone, which
# does not depend on the line format)
KEYED = [c for c in D.CASES if c.recipe == "random"]


def dev(a):
    return torch.from_numpy(np.array(a)).to("cuda:0")


def lib():
    return E.load_library()


def dense_count():
    return lib().rf_amd_diag_dense_line_filters()


def run_found(n, call):
    found = torch.full((n + PAD,), SENT_I64, dtype=torch.int64, device="cuda:0")
    call(found)
    torch.cuda.synchronize()
    out = found.cpu().numpy().view(np.uint64)
    assert (out[n:] == np.uint64(SENT)).all(), "wrote past d_found[n)"
    return out[:n]


def check(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, bad[:8].tolist(), [hex(int(x)) for x in got[bad[:4]]],
                           [hex(int(x)) for x in want[bad[:4]]])


class World:
    def __init__(self, ref):
        self.ref, self.batch, self.where, self.keep = ref, [], {}, []
        for cs in BATCHES:
            cfg = E.routing_config_init(**cs[0].cfg_kw)
            before = dense_count()
            if cs[0].recipe == "chain":
                b = None
                for h, v in ref[cs[0].name].inp.adds:
                    b = E.FilterBatch(cfg, [h.size], [v], old=[(b, 0)] if b is not None else None)
                    b.build_hashes(dev(h))
                    self.keep.append(b)
                built = len(ref[cs[0].name].inp.adds)
            else:
                b = E.FilterBatch(cfg, [c.n for c in cs], [c.value for c in cs])
                b.build_hashes(dev(np.concatenate([ref[c.name].inp.h for c in cs])))
                self.keep.append(b)
                built = len(cs)
            assert dense_count() - before == built, "every filter of the build took the dense format"
            self.batch.append(b)
            for f, c in enumerate(cs):
                self.where[c.name] = (b, f)
        torch.cuda.synchronize()
        self.set = E.FilterSet([self.where[c.name] for c in D.CASES])

    def close(self):
        self.set.close()
        for b in reversed(self.keep):
            b.close()


@pytest.fixture(scope="module")
def world(oracle):
    ref = D.reference(oracle)
    mp = pytest.MonkeyPatch()  # the knob is read when a batch is created or imported
    mp.setenv("RF_AMD_LINES_DENSE", "1")
    mp.delenv("RF_AMD_LINE_SIGMA", raising=False)
    mp.delenv("RF_AMD_DENSE_SIGMA", raising=False)
    w = World(ref)
    yield w
    w.close()
    mp.undo()


def batch_param():
    return pytest.mark.parametrize("bi", range(len(BATCHES)), ids=BATCH_IDS)


def num_lines(b):
    n = ctypes.c_uint64(1 << 40)
    E._check(lib().rf_amd_debug_read_lines(b.h, None, 0, ctypes.byref(n)))
    return n.value


# ---- the lines ---------------------------------------------------------------------------------
@batch_param()
def test_lines(world, bi):
    """as the build left them (K6's cut in assembly), re-cut by k_plines, and cut by k_plines for a
    batch imported from the export; the images are the oracle's"""
    cs, b = BATCHES[bi], world.batch[bi]
    for f, c in enumerate(cs):
        img, o = b.image(f), world.ref[c.name].img
        assert img.num_indices == o.num_indices and (img.pages == o.pages).all() and (img.slots == o.slots).all(), c.name
    want = np.concatenate([world.ref[c.name].lines for c in cs])
    for step in ("built", "rebuilt"):
        assert num_lines(b) == want.shape[0], step
        lines = b.debug_lines()
        bad = np.flatnonzero((lines != want).any(axis=1))
        assert bad.size == 0, (step, bad.size, bad[:8].tolist())
        b.debug_rebuild_lines()
    infos, pbytes, nslots = b.export_sizes()
    d_p = torch.zeros(pbytes, dtype=torch.uint8, device="cuda:0")
    d_s = torch.zeros(nslots, dtype=torch.int64, device="cuda:0")
    b.export(d_p, d_s)
    torch.cuda.synchronize()
    before = dense_count()
    imp = E.FilterBatch.imported(b.cfg, infos, d_p, d_s)
    try:
        assert dense_count() - before == len(cs)
        assert num_lines(imp) == want.shape[0] and (imp.debug_lines() == want).all()
        c = cs[-1]
        r = world.ref[c.name]
        got = run_found(D.PROBES, lambda d: imp.probe_hashes_runs(dev(r.probes), [0] * (len(cs) - 1) + [D.PROBES], d))
        check(got, r.want, ("imported", c.name))
    finally:
        imp.close()


# ---- the lookup paths --------------------------------------------------------------------------
def runs_of(world, cs, tail):
    """every filter's probes run after run; tail: 37 fewer of each, so later runs start off a wave
    boundary and a wave straddles two filters"""
    k = D.PROBES - (37 if tail else 0)
    return ([k] * len(cs), np.concatenate([world.ref[c.name].probes[:k] for c in cs]),
            np.concatenate([world.ref[c.name].want[:k] for c in cs]))


@pytest.mark.parametrize("tail", [False, True], ids=["x64", "tails"])
@batch_param()
def test_probe_hashes_runs(world, bi, tail):
    """hashes in, per-filter runs: the fast path"""
    cs, b = BATCHES[bi], world.batch[bi]
    counts, ph, want = runs_of(world, cs, tail)
    got = run_found(ph.size, lambda d: b.probe_hashes_runs(dev(ph), counts, d))
    check(got, want, (BATCH_IDS[bi], tail))


@batch_param()
def test_probe_hashes_filter_ids(world, bi):
    """per-probe filter ids: grouped by filter (the rotated gather) and shuffled (one lane per probe)"""
    cs, b = BATCHES[bi], world.batch[bi]
    counts, ph, want = runs_of(world, cs, False)
    fid = np.repeat(np.arange(len(cs), dtype=np.uint32), counts)
    for order in (np.arange(ph.size), np.random.default_rng(bi).permutation(ph.size)):
        got = run_found(ph.size, lambda d: b.probe_hashes(dev(ph[order]), dev(fid[order]), ph.size, d))
        check(got, want[order], BATCH_IDS[bi])


def key_probes(world, case, oracle):
    """PROBES 24-byte keys, half the filter's own, half random; and the oracle's words"""
    rng = np.random.default_rng([3, case.fp, case.n, case.value])
    pk = K.random_keys(D.PROBES, seed=int(rng.integers(1 << 30)))
    keys = world.ref[case.name].inp.keys
    pk[: D.PROBES // 2] = keys[rng.integers(0, case.n, size=D.PROBES // 2)]
    pk = pk[rng.permutation(D.PROBES)]
    ph = oracle.hash_fixed(pk.reshape(-1), 24)
    want = world.ref[case.name].of.lookup_hashes(ph)
    assert (want != 0).sum() >= D.PROBES // 2
    return pk, want


@pytest.mark.parametrize("case", KEYED, ids=lambda c: c.name)
def test_probe_keys_runs(world, oracle, case):
    """24-byte keys in, per-filter runs: the fast path as the benchmark takes it"""
    b, f = world.where[case.name]
    pk, want = key_probes(world, case, oracle)
    counts = [0] * b.F
    counts[f] = D.PROBES
    got = run_found(D.PROBES, lambda d: b.probe_keys_runs(dev(pk.reshape(-1)), 24, counts, d))
    check(got, want, case.name)


@pytest.mark.parametrize("case", KEYED, ids=lambda c: c.name)
def test_probe_var_keys(world, oracle, case):
    """variable-length keys: the filter's own 24-byte keys and random keys of 1 to 100 bytes"""
    b, f = world.where[case.name]
    rng = np.random.default_rng([4, case.fp, case.n, case.value])
    n = D.PROBES
    lens = rng.integers(1, 101, size=n)
    own = rng.random(n) < 0.5
    lens[own] = 24
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=offs[1:])
    data = rng.integers(0, 256, size=int(offs[-1]), dtype=np.uint8)
    keys = world.ref[case.name].inp.keys
    at = offs[:-1][own].astype(np.int64)[:, None] + np.arange(24)
    data[at] = keys[rng.integers(0, case.n, size=int(own.sum()))]
    want = world.ref[case.name].of.lookup_hashes(oracle.hash_var(data, offs))
    assert (want[own] != 0).all() and own.sum() > n // 3
    fid = np.full(n, f, dtype=np.uint32)
    got = run_found(n, lambda d: b.probe_var_keys(dev(data), dev(offs.view(np.int64)), dev(fid), n, d))
    check(got, want, case.name)


def pool(world, n):
    """n probes drawn from every case's set, and words[m]: member m's oracle lookup of the pool"""
    ph = np.concatenate([world.ref[c.name].probes[: n // len(D.CASES) + 1] for c in D.CASES])[:n]
    ph = ph[np.random.default_rng(8).permutation(n)]
    return ph, np.stack([world.ref[c.name].of.lookup_hashes(ph) for c in D.CASES])


def test_filter_set_fanout(world):
    """every key against every member (k_probe_fanout), then member lists of 0 to 70 ids
    (k_probe_fanout_ragged): 200,000 pairs and more each"""
    M = len(D.CASES)
    n = D.PROBES // M + 1
    ph, words = pool(world, n)
    got = run_found(n * M, lambda d: world.set.probe_hashes(dev(ph), None, M, n, d))
    check(got, np.ascontiguousarray(words.T).reshape(-1), "every member")
    rng = np.random.default_rng(70)
    counts = rng.choice([0, 1, 2, 7, 70], size=n, p=[0.1, 0.2, 0.2, 0.4, 0.1])
    member = rng.integers(0, M + 1, size=int(counts.sum())).astype(np.uint32)
    key = np.repeat(np.arange(n), counts)
    ok = member < M
    want = np.where(ok, words[np.where(ok, member, 0), key], np.uint64(0))
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    assert member.size >= D.PROBES
    got = run_found(member.size, lambda d: world.set.probe_hashes_ragged(dev(ph), dev(member), dev(off), n, d))
    check(got, want, "ragged")


def test_host_buffer_lookup(world):
    """rf_amd_probe_many_hashes_host over every case: hashes and results in host memory"""
    names = [c.name for c in D.CASES]
    hashes = np.ascontiguousarray(np.concatenate([world.ref[nm].probes for nm in names]))
    want = np.concatenate([world.ref[nm].want for nm in names])
    hs = (ctypes.c_void_p * len(names))(*[world.where[nm][0].h.value for nm in names])
    fi = np.array([world.where[nm][1] for nm in names], dtype=np.uint32)
    c = np.full(len(names), D.PROBES, dtype=np.uint64)
    out = H.sentinel_out(hashes.size)
    rc = lib().rf_amd_probe_many_hashes_host(E.default_engine().h, ctypes.cast(hs, ctypes.c_void_p), fi.ctypes.data,
                                             c.ctypes.data, len(names), hashes.ctypes.data, out.ctypes.data)
    assert rc == 0, lib().rf_amd_last_error()
    H.check_out(out, hashes.size, want, names)


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.name)
def test_small_and_server_lookups(world, case):
    """one lookup in the kernel arguments (k_probe_small) and 32 through the lookup server"""
    b, f = world.where[case.name]
    r = world.ref[case.name]
    hs = (ctypes.c_void_p * 1)(b.h.value)
    fi, c = np.array([f], dtype=np.uint32), np.array([8], dtype=np.uint64)
    hashes = np.ascontiguousarray(r.probes[:8])
    out = H.sentinel_out(8)
    rc = lib().rf_amd_probe_many_hashes_host(E.default_engine().h, ctypes.cast(hs, ctypes.c_void_p), fi.ctypes.data,
                                             c.ctypes.data, 1, hashes.ctypes.data, out.ctypes.data)
    assert rc == 0, lib().rf_amd_last_error()
    H.check_out(out, 8, r.want[:8], case.name)
    got = np.zeros(32, dtype=np.uint64)
    for i in range(32):
        t, o = ctypes.c_uint64(), ctypes.c_uint64(SENT)
        E._check(lib().rf_amd_lookup_submit(b.engine.h, b.h, f, int(r.probes[i]), None, ctypes.byref(t)))
        E._check(lib().rf_amd_lookup_wait(b.engine.h, t.value, ctypes.byref(o)))
        got[i] = o.value
    check(got, r.want[:32], case.name)


# ---- the mode gate -----------------------------------------------------------------------------
def test_mode_gate(monkeypatch):
    """knob unset: batches of C3's shape (2^20 keys) and filters of at most 300,000 keys build no
    dense lines, a filter of C2's shape (8,000,000 keys) builds one -- and answers as the same
    filter does in the current format (knob 0)"""
    monkeypatch.delenv("RF_AMD_LINES_DENSE", raising=False)
    cfg = E.routing_config_init(log_index_size=8)
    before = dense_count()
    for sizes in ([1 << 20] * 3, [300_000, 70_000, 5_000, 1]):
        keys = K.seq_keys_torch(0, sum(sizes), 24, torch.device("cuda", 0))
        b = E.FilterBatch(cfg, sizes, [0] * len(sizes))
        b.build_keys(keys, 24)
        torch.cuda.synchronize()
        b.close()
    assert dense_count() == before
    n = 8_000_000
    keys = K.seq_keys_torch(0, 2 * n, 24, torch.device("cuda", 0))  # the second half was never inserted
    found = {}
    for knob in (None, "0"):
        if knob is not None:
            monkeypatch.setenv("RF_AMD_LINES_DENSE", knob)
        before = dense_count()
        b = E.FilterBatch(cfg, [n], [0])
        b.build_keys(keys[:n], 24)
        assert dense_count() - before == (1 if knob is None else 0)
        assert num_lines(b) == 16384 * (7 if knob is None else 8)
        d = torch.zeros(2 * n, dtype=torch.int64, device="cuda:0")
        b.probe_keys_runs(keys, 24, [2 * n], d)
        torch.cuda.synchronize()
        found[knob] = d
        b.close()
    assert torch.equal(found[None], found["0"])
    assert bool((found[None][:n] & 1).all()) and int((found[None][n:] != 0).sum()) < n // 4
