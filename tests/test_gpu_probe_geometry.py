"""Every lookup entry point over the probe geometry sweep (tests/probe_geometry_cases.py): rem 0
and 1, rvs 0 to 29, value 63, probe-line groups of 1 to 64 buckets and none, log_index_size 3 to
11, overflowed lines, buckets past the 96-bit window, found words of several bits, and members of
every (fingerprint_size, log_index_size) in one filter set.

Every found word is compared bit for bit with oracle.lookup_hashes (routing_filter_lookup,
src/routing_filter.c:985-1073) of the same hash in the same filter. Output buffers are pre-filled
with a sentinel, and the 8 words past the last probe must keep it. The device-only probe lines are
compared with expected_probe_lines, which tests/test_probe_geometry_cases.py checks against the
oracle on the CPU; that file also proves which decode classes the probes used here reach.

The whole file runs three times: with RF_AMD_LINE_SIGMA unset, at the value that gives fp 32 /
lis 3 / n 200 one bucket per line (G == 1), and at the value that leaves no case any lines
(lg_line == 0: every probe walks the image). Both values come from the helper's restatement of
line_log_group, which the CPU tests compare with rf_batch_plan.h itself."""
import ctypes

import numpy as np
import pytest

import host_lookup_cases as H
import probe_geometry_cases as P
from splinterdb_amd import engine as E
from splinterdb_amd import keys as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT, PAD = H.SENT, H.PAD
SENT_I64 = SENT - (1 << 64)
BATCHES = P.batches()
BATCH_IDS = ["+".join(c.name for c in cs) for cs in BATCHES]
KEY_BATCHES = [cs for cs in BATCHES if any(c.recipe == "random" for c in cs)]
KEY_BATCH_IDS = ["+".join(c.name for c in cs) for cs in KEY_BATCHES]
SETTINGS = ["default", "g1", "nolines"]
# rf_amd_probe_many_hashes_host's small path takes at most 8 groups: rvs 0, rem 0 with value bits,
# rvs 1, rvs 29, 64 buckets per line, lis 9, overflowed lines at lis 3, and a chain
TABLE8 = ["fp12_lis4_n5000_v0", "fp12_lis4_n5000_v3", "fp13_lis4_n5000_v0", "fp32_lis3_n9_v0", "fp12_lis8_n100_v1",
          "fp22_lis9_n140000_v0", "clustered_fp32_lis3_rvs22", "chain_fp13_lis4"]


def dev(a):
    return torch.from_numpy(np.array(a)).to("cuda:0")  # a copy: the reference's arrays are read-only


def lib():
    return E.load_library()


def run_found(n, call):
    """call(d_found) on n + PAD sentinel words; the n found words, the pad checked"""
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
    """every case's filter on the default engine: the cases of one (fp, lis) in one batch built from
    hashes, a chain as three batches each added onto the one before"""

    def __init__(self, ref, sigma):
        self.ref, self.sigma = ref, sigma
        self.batch, self.where, self.keep = [], {}, []
        for cs in BATCHES:
            cfg = E.routing_config_init(**cs[0].cfg_kw)
            if cs[0].recipe == "chain":
                b = None
                for h, v in ref[cs[0].name].inp.adds:
                    b = E.FilterBatch(cfg, [h.size], [v], old=[(b, 0)] if b is not None else None)
                    b.build_hashes(dev(h))
                    self.keep.append(b)
            else:
                b = E.FilterBatch(cfg, [c.n for c in cs], [c.value for c in cs])
                b.build_hashes(dev(np.concatenate([ref[c.name].inp.h for c in cs])))
                self.keep.append(b)
            self.batch.append(b)
            for f, c in enumerate(cs):
                self.where[c.name] = (b, f)
        torch.cuda.synchronize()
        self.members = [self.where[c.name] for c in P.CASES]
        self.set = E.FilterSet(self.members)

    def group(self, case):
        return case.group(self.sigma)

    def close(self):
        self.set.close()
        for b in reversed(self.keep):
            b.close()


@pytest.fixture(scope="module", params=SETTINGS)
def world(request, oracle):
    ref = P.reference(oracle)
    g1, none = P.knob_sigmas()
    sigma = {"default": None, "g1": g1, "nolines": none}[request.param]
    mp = pytest.MonkeyPatch()  # the knob is read when a batch is created or imported
    if sigma is None:
        mp.delenv("RF_AMD_LINE_SIGMA", raising=False)
    else:
        mp.setenv("RF_AMD_LINE_SIGMA", repr(sigma))
    w = World(ref, sigma)
    yield w
    w.close()
    mp.undo()


def batch_param(ids=BATCH_IDS, n=len(BATCHES)):
    return pytest.mark.parametrize("bi", range(n), ids=ids)


# ---- a. the lines ------------------------------------------------------------------------------
def expected_lines(w, cs):
    out = []
    for c in cs:
        G, img = w.group(c), w.ref[c.name].img
        if G:
            out.append(P.expected_probe_lines(img.pages, img.slots, img.num_indices, 1 << c.lis, G, c.rvs))
    return np.concatenate(out) if out else np.zeros((0, 64), dtype=np.uint8)


def num_lines(b):
    n = ctypes.c_uint64(1 << 40)
    E._check(lib().rf_amd_debug_read_lines(b.h, None, 0, ctypes.byref(n)))
    return n.value


@batch_param()
def test_lines(world, bi):
    """the batch's line table, filter after filter at the restated group size (the table's, at the
    default margin): as the build left it (K6's cut in assembly, k_plines_list for what K6 leaves),
    re-cut by k_plines, and cut by k_plines for a batch imported from the export. Without lines
    the table is empty. The images are the oracle's."""
    w, cs, b = world, BATCHES[bi], world.batch[bi]
    for f, c in enumerate(cs):
        img, o = b.image(f), w.ref[c.name].img
        assert img.num_indices == o.num_indices and (img.pages == o.pages).all() and (img.slots == o.slots).all(), c.name
        if w.sigma is None:
            assert w.group(c) == c.G > 0
    want = expected_lines(w, cs)
    if w.sigma == P.knob_sigmas()[1]:
        assert want.shape[0] == 0 and num_lines(b) == 0
    if w.sigma == P.knob_sigmas()[0] and P.G1_CASE in cs:
        assert w.group(P.G1_CASE) == 1
    for step in ("built", "rebuilt"):
        assert num_lines(b) == want.shape[0], step
        lines = b.debug_lines() if want.shape[0] else want
        assert lines.shape == want.shape, (step, lines.shape, want.shape)
        bad = np.flatnonzero((lines != want).any(axis=1))
        assert bad.size == 0, (step, bad.size, bad[:8].tolist())
        b.debug_rebuild_lines()
    infos, pbytes, nslots = b.export_sizes()
    d_p = torch.zeros(pbytes, dtype=torch.uint8, device="cuda:0")
    d_s = torch.zeros(nslots, dtype=torch.int64, device="cuda:0")
    b.export(d_p, d_s)
    torch.cuda.synchronize()
    imp = E.FilterBatch.imported(b.cfg, infos, d_p, d_s)
    try:
        assert num_lines(imp) == want.shape[0]
        lines = imp.debug_lines() if want.shape[0] else want
        assert lines.shape == want.shape and (lines == want).all()
        for f, c in enumerate(cs):
            ph = w.ref[c.name].sets.tail
            got = run_found(ph.size, lambda d: imp.probe_hashes(dev(ph), dev(np.full(ph.size, f, np.uint32)), ph.size, d))
            check(got, w.ref[c.name].want_tail, ("imported", c.name))
    finally:
        imp.close()


# ---- b. probe_hashes ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c.name)
def test_probe_hashes_one_filter(world, case):
    """64 k + 37 probes of one filter: full waves take the rotated gather, the last the tail"""
    b, f = world.where[case.name]
    r = world.ref[case.name]
    ph = r.sets.tail
    got = run_found(ph.size, lambda d: b.probe_hashes(dev(ph), dev(np.full(ph.size, f, np.uint32)), ph.size, d))
    check(got, r.want_tail, case.name)


def mixed(w, cs, seed, past=16):
    """the batch's tail sets shuffled together: (hashes, filter ids, words); `past` probes carry
    ids at and past the batch's filter count and find nothing"""
    ref = w.ref
    ph = np.concatenate([ref[c.name].sets.tail for c in cs])
    fid = np.repeat(np.arange(len(cs), dtype=np.uint32), [ref[c.name].sets.tail.size for c in cs])
    want = np.concatenate([ref[c.name].want_tail for c in cs])
    order = np.random.default_rng(seed).permutation(ph.size)
    ph, fid, want = ph[order], fid[order], want[order]
    fid[:past] = [len(cs), len(cs) + 1, 255, 0xFFFFFFFF] * (past // 4)
    want[:past] = 0
    return ph, fid, want


@batch_param()
def test_probe_hashes_mixed_ids(world, bi):
    cs, b = BATCHES[bi], world.batch[bi]
    ph, fid, want = mixed(world, cs, 5)
    got = run_found(ph.size, lambda d: b.probe_hashes(dev(ph), dev(fid), ph.size, d))
    check(got, want, BATCH_IDS[bi])


# ---- c. the runs forms -------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False], ids=["x64", "tails"])
@batch_param()
def test_probe_hashes_runs(world, bi, aligned):
    cs, b = BATCHES[bi], world.batch[bi]
    counts, ph, want = P.runs_layout(world.ref, cs, aligned)
    got = run_found(ph.size, lambda d: b.probe_hashes_runs(dev(ph), counts, d))
    check(got, want, (BATCH_IDS[bi], counts))


def key_probes(w, case, count, seed):
    """count 24-byte keys: half the filter's own (where it was built from keys), half random"""
    rng = np.random.default_rng([seed, count, case.n])
    pk = K.random_keys(count, seed=int(rng.integers(1 << 30)))
    keys = w.ref[case.name].inp.keys
    if keys is not None and count:
        pk[: count // 2] = keys[rng.integers(0, case.n, size=count // 2)]
    return pk


@pytest.mark.parametrize("shift", [0, 8])
@pytest.mark.parametrize("aligned", [True, False], ids=["x64", "tails"])
@batch_param(KEY_BATCH_IDS, len(KEY_BATCHES))
def test_probe_keys_runs(world, oracle, bi, aligned, shift):
    """the filters' own keys (their hashes are oracle.hash_fixed of 24-byte keys) and random keys;
    shift 8: from a key buffer 8 bytes off 16-byte alignment"""
    cs = KEY_BATCHES[bi]
    b = world.where[cs[0].name][0]
    counts = P.run_counts(cs, aligned)
    pk = np.concatenate([key_probes(world, c, k, 11) for c, k in zip(cs, counts)])
    ph = oracle.hash_fixed(pk.reshape(-1), 24)
    at = np.concatenate([[0], np.cumsum(counts)])
    want = np.concatenate([world.ref[c.name].of.lookup_hashes(ph[at[f]:at[f + 1]]) for f, c in enumerate(cs)])
    for f, c in enumerate(cs):
        own = counts[f] // 2 if world.ref[c.name].inp.keys is not None else 0
        assert (want[at[f]:at[f] + own] >> np.uint64(c.value) & np.uint64(1)).all(), c.name
    buf = torch.zeros(pk.size + 32, dtype=torch.uint8, device="cuda:0")
    buf[shift:shift + pk.size] = dev(pk.reshape(-1))
    d_keys = buf[shift:]
    assert d_keys.data_ptr() % 16 == shift
    got = run_found(len(ph), lambda d: b.probe_keys_runs(d_keys, 24, counts, d))
    check(got, want, (KEY_BATCH_IDS[bi], counts, shift))


# ---- d. pairs and variable-length keys ---------------------------------------------------------
@batch_param()
def test_probe_pairs(world, bi):
    cs, b = BATCHES[bi], world.batch[bi]
    ph, fid, want = mixed(world, cs, 6, past=0)
    pairs = (fid.astype(np.uint64) << np.uint64(32)) | ph.astype(np.uint64)
    got = run_found(ph.size, lambda d: b.probe_pairs(dev(pairs.view(np.int64)), ph.size, d))
    check(got, want, BATCH_IDS[bi])


@batch_param(KEY_BATCH_IDS, len(KEY_BATCHES))
def test_probe_var_keys(world, oracle, bi):
    """own keys (24 bytes) and random keys of 1 to 100 bytes, filter ids mixed"""
    cs = KEY_BATCHES[bi]
    b = world.where[cs[0].name][0]
    rng = np.random.default_rng([7, bi])
    n = 64 * 24 + P.TAIL
    fid = rng.integers(0, len(cs), size=n).astype(np.uint32)
    lens = rng.integers(1, 101, size=n)
    own = rng.random(n) < 0.5
    own &= np.array([world.ref[cs[f].name].inp.keys is not None for f in fid])
    lens[own] = 24
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=offs[1:])
    data = rng.integers(0, 256, size=int(offs[-1]), dtype=np.uint8)
    for i in np.flatnonzero(own):
        c = cs[fid[i]]
        data[int(offs[i]):int(offs[i]) + 24] = world.ref[c.name].inp.keys[rng.integers(0, c.n)]
    vh = oracle.hash_var(data, offs)
    want = np.zeros(n, dtype=np.uint64)
    for f, c in enumerate(cs):
        want[fid == f] = world.ref[c.name].of.lookup_hashes(vh[fid == f])
    assert own.sum() > n // 8 and want[own].all() and {1, 100} <= set(lens.tolist())
    got = run_found(n, lambda d: b.probe_var_keys(dev(data), dev(offs.view(np.int64)), dev(fid), n, d))
    check(got, want, KEY_BATCH_IDS[bi])


# ---- e. one filter set over every case ---------------------------------------------------------
def set_want(w, member):
    """words of an (n, K) id array: member m's oracle lookup of the probe, 0 for ids past the end"""
    pool, M = w.ref["pool"], len(P.CASES)
    ok = member < M
    key = np.arange(pool.hashes.size)[:, None]
    return np.where(ok, pool.words[np.where(ok, member, 0), key], np.uint64(0)).reshape(-1)


def test_filter_set_every_member(world):
    """d_member == NULL: slot j is member j, K = the number of members"""
    w, pool, M = world, world.ref["pool"], len(P.CASES)
    n = pool.hashes.size
    got = run_found(n * M, lambda d: w.set.probe_hashes(dev(pool.hashes), None, M, n, d))
    check(got, np.ascontiguousarray(pool.words.T).reshape(-1), "every member")


@pytest.mark.parametrize("k", [1, 3, len(P.CASES)])
def test_filter_set_explicit_ids(world, k):
    w, pool, M = world, world.ref["pool"], len(P.CASES)
    n = pool.hashes.size
    member = np.random.default_rng(k).integers(0, M + 2, size=(n, k)).astype(np.uint32)
    member[::97, 0] = 0xFFFFFFFF
    want = set_want(w, member)
    assert (member >= M).any() and (want[(member < M).reshape(-1)] != 0).any()
    got = run_found(n * k, lambda d: w.set.probe_hashes(dev(pool.hashes), dev(member.reshape(-1)), k, n, d))
    check(got, want, k)
    assert (got[(member >= M).reshape(-1)] == 0).all()


def test_filter_set_ragged(world):
    """member lists of 0, 1, 2 and 70 ids, mixed"""
    w, pool, M = world, world.ref["pool"], len(P.CASES)
    n = pool.hashes.size
    rng = np.random.default_rng(70)
    counts = rng.choice([0, 1, 2, 70], size=n, p=[0.3, 0.3, 0.3, 0.1])
    counts[:4] = [70, 0, 1, 2]
    member = rng.integers(0, M + 2, size=int(counts.sum())).astype(np.uint32)
    key = np.repeat(np.arange(n), counts)
    ok = member < M
    want = np.where(ok, pool.words[np.where(ok, member, 0), key], np.uint64(0))
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    got = run_found(member.size, lambda d: w.set.probe_hashes_ragged(dev(pool.hashes), dev(member), dev(off), n, d))
    check(got, want, "ragged")
    assert set(counts.tolist()) == {0, 1, 2, 70} and (got[~ok] == 0).all()


# ---- f. host and latency paths -----------------------------------------------------------------
@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c.name)
def test_dropin_lookup_on_the_image(world, case):
    """routing_filter_lookup's replacement on the oracle's own image"""
    r = world.ref[case.name]
    of = r.of
    filt = E.RoutingFilter(of.num_fingerprints, of.num_unique, of.value_size, of.num_indices, of.num_pages,
                           r.img.pages, r.img.slots)
    ph = np.array(r.sets.tail)
    out = H.sentinel_out(ph.size)
    fc = filt._c()
    cfg = E.routing_config_init(**case.cfg_kw)
    E._check(lib().rf_amd_filter_lookup_hashes(E.default_engine().h, ctypes.byref(cfg.c()), ctypes.byref(fc),
                                               ph.ctypes.data, ph.size, out.ctypes.data))
    H.check_out(out, ph.size, r.want_tail, case.name)


def many_hashes(w, names, counts, path):
    """one rf_amd_probe_many_hashes_host call: group g probes counts[g] hashes of names[g]'s tail set"""
    ref = w.ref
    hashes = np.ascontiguousarray(np.concatenate([ref[nm].sets.tail[:k] for nm, k in zip(names, counts)]))
    want = np.concatenate([ref[nm].want_tail[:k] for nm, k in zip(names, counts)])
    n = int(sum(counts))
    hs = (ctypes.c_void_p * len(names))(*[w.where[nm][0].h.value for nm in names])
    fi = np.array([w.where[nm][1] for nm in names], dtype=np.uint32)
    c = np.asarray(counts, dtype=np.uint64)
    out = H.sentinel_out(n)
    before = H.paths()
    rc = lib().rf_amd_probe_many_hashes_host(E.default_engine().h, ctypes.cast(hs, ctypes.c_void_p), fi.ctypes.data,
                                             c.ctypes.data, len(names), hashes.ctypes.data, out.ctypes.data)
    assert rc == 0, lib().rf_amd_last_error()
    H.check_out(out, n, want, (names, counts))
    delta = H.paths() - before
    assert (delta == H.one_hot(path)).all(), (counts, path, delta.tolist())


@pytest.mark.parametrize("n", [1, 64, 300])
def test_many_hashes_host(world, n):
    """n = 1 (each of eight differently configured groups in turn) and 64 travel in the kernel
    arguments (k_probe_small), 300 over every case read the mapped buffer (k_probe_groups)"""
    if n == 1:
        for g in range(len(TABLE8)):
            many_hashes(world, TABLE8, [int(j == g) for j in range(len(TABLE8))], "small")
    elif n == 64:
        many_hashes(world, TABLE8, [8] * 8, H.default_path(64, 8))
        assert H.default_path(64, 8) == "small"
    else:
        names = [c.name for c in P.CASES]
        assert len(names) * 15 == n
        many_hashes(world, names, [15] * len(names), "mapped")


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c.name)
def test_lookup_server(world, case):
    """32 single lookups through rf_amd_lookup_submit / _wait"""
    b, f = world.where[case.name]
    r = world.ref[case.name]
    got = np.zeros(32, dtype=np.uint64)
    for i in range(32):
        t, out = ctypes.c_uint64(), ctypes.c_uint64(SENT)
        E._check(lib().rf_amd_lookup_submit(b.engine.h, b.h, f, int(r.sets.tail[i]), None, ctypes.byref(t)))
        E._check(lib().rf_amd_lookup_wait(b.engine.h, t.value, ctypes.byref(out)))
        got[i] = out.value
    check(got, r.want_tail[:32], case.name)
