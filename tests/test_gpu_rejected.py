"""The rejected-filter contract on the engine. A filter is rejected when one index holds more
than 4,096 entries or one index block is larger than a page; the reference overruns a buffer
there, so everything that follows a rejection is this engine's own code.

The inputs come from tests/reject_cases.py and sit exactly on the limits (proved against the
oracle by tests/test_reject_limits.py). At the limit the image and the probes equal the
oracle's bit for bit; one past it the error bits are exactly the expected mask, every consumer
of the rejected filter finds nothing or returns STATUS_BAD_PARAM, a sibling in the same batch
stays exact, rebuilds over and after a rejection are exact, and a filter built on a rejected old
filter is itself rejected without reading the old image."""
import ctypes
import time

import numpy as np
import pytest

import reject_cases as R
from splinterdb_amd import engine as E
from splinterdb_amd import keys as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIB_N = 3000   # the healthy sibling
P = 2000       # probes per image check
# K5's segments wait about a second (LSEG_POLLS) for a predecessor's hand-off; a build of these
# sizes takes milliseconds, so one that takes a quarter of that wait has lost a hand-off
HANDOFF_S = 0.25


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def lib():
    return E.load_library()


def cfgs(oracle, fp, lis):
    return (E.routing_config_init(fingerprint_size=fp, log_index_size=lis),
            oracle.make_config(fingerprint_size=fp, log_index_size=lis))


def same_image(img, of, tag):
    assert (img.num_unique, img.num_pages) == (of.num_unique, of.num_pages), tag
    assert (img.pages == of.pages()).all(), tag
    assert (img.slots == of.slots()[: of.num_indices]).all(), tag


def in_index(rng, nidx, index, n):
    """n random hashes of one index"""
    lg = nidx.bit_length() - 1
    low = rng.integers(0, 1 << (32 - lg), size=n, dtype=np.uint64)
    return ((index << (32 - lg)) | low).astype(np.uint32)


def probe_set(seed, nidx, index, inserted, n=P):
    """half from the clustered index (inserted hashes of it and other hashes of it), the rest
    inserted hashes and random ones"""
    rng = np.random.default_rng(seed)
    lg = nidx.bit_length() - 1
    own = inserted[(inserted >> np.uint32(32 - lg)) == index]
    q = n // 4
    return np.concatenate([own[rng.integers(0, own.size, size=q)], in_index(rng, nidx, index, q),
                           inserted[rng.integers(0, inserted.size, size=q)],
                           rng.integers(0, 1 << 32, size=n - 3 * q, dtype=np.uint64).astype(np.uint32)])


def device_probe(b, f, ph):
    found = torch.zeros(ph.size, dtype=torch.int64, device="cuda:0")
    b.probe_hashes(dev(ph), dev(np.full(ph.size, f, dtype=np.uint32)), ph.size, found)
    torch.cuda.synchronize()
    return found.cpu().numpy().view(np.uint64)


def host_probe(b, fid, ph):
    ph = np.ascontiguousarray(ph, dtype=np.uint32)
    fid = np.ascontiguousarray(np.broadcast_to(np.asarray(fid, dtype=np.uint32), ph.shape))
    out = np.full(ph.size, 0xA5A5, dtype=np.uint64)
    E._check(lib().rf_amd_batch_probe_hashes_host(b.h, ph.ctypes.data, fid.ctypes.data, ph.size, out.ctypes.data))
    return out


def check_exact(b, f, of, ph, tag):
    assert b.info(f).error == 0, tag
    same_image(b.image(f), of, tag)
    assert (device_probe(b, f, ph) == of.lookup_hashes(ph)).all(), tag


def check_rejected(b, f, bits, tag):
    assert b.info(f).error == bits, (tag, b.info(f).error)
    assert b.infos()[f].error == bits, tag
    with pytest.raises(E.PlatformStatusError) as ei:
        b.image(f)
    assert ei.value.code == E.STATUS_BAD_PARAM, tag


class Refs:
    """hashes and the oracle's filters, computed once per module and never changed"""

    def __init__(self, oracle):
        self.oracle = oracle
        self.memo = {}

    def get(self, key, make):
        if key not in self.memo:
            v = make()
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self.memo[key] = v
        return self.memo[key]

    def sibling(self, fp, lis, n=SIB_N, value=0, seed=0):
        def make():
            rng = np.random.default_rng([fp, lis, n, value, seed, 77])
            h = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
            return h, self.oracle.filter_add(self.oracle.make_config(fingerprint_size=fp, log_index_size=lis), h,
                                             value=value)
        return self.get(("sib", fp, lis, n, value, seed), make)

    def fresh(self, case, index):
        """(hashes at the limit, their oracle filter, hashes past the limit)"""
        def make():
            ocfg = self.oracle.make_config(fingerprint_size=case.fp, log_index_size=case.lis)
            h = case.hashes(case.limit, index)
            return h, self.oracle.filter_add(ocfg, h, value=case.value), case.hashes(case.past, index)
        return self.get(("fresh", case.name, index), make)

    def incremental(self, case, index):
        """(old hashes, old oracle filter, new hashes at the limit, merged oracle filter, new
        hashes past the limit)"""
        def make():
            ocfg = self.oracle.make_config(fingerprint_size=case.fp, log_index_size=case.lis)
            ho = case.old_hashes(case.limit[0], index)
            old = self.oracle.filter_add(ocfg, ho, value=case.v_old)
            hn = case.new_hashes(case.limit[1], index)
            return (ho, old, hn, self.oracle.filter_add(ocfg, hn, value=case.v_new, old=old),
                    case.new_hashes(case.past[1], index))
        return self.get(("incr", case.name, index), make)


@pytest.fixture(scope="module")
def refs(oracle):
    return Refs(oracle)


# ---- 2. the limit itself ---------------------------------------------------------------------
def run_fresh(refs, case, index, tag, timed=False):
    cfg, _ = cfgs(refs.oracle, case.fp, case.lis)
    h_lim, of_lim, h_past = refs.fresh(case, index)
    h_sib, of_sib = refs.sibling(case.fp, case.lis)
    ph = probe_set(index, case.nidx, index, h_lim)
    ph_sib = probe_set(index + 1, 2, 0, h_sib)
    b = E.FilterBatch(cfg, [case.n, SIB_N], [case.value, 0])
    b.build_hashes(dev(np.concatenate([h_lim, h_sib])))
    assert b.infos()[0].error == 0, tag
    check_exact(b, 0, of_lim, ph, (tag, "at the limit"))
    check_exact(b, 1, of_sib, ph_sib, (tag, "sibling at the limit"))
    b.close()
    b = E.FilterBatch(cfg, [case.n, SIB_N], [case.value, 0])
    d = dev(np.concatenate([h_past, h_sib]))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b.build_hashes(d)
    err = b.info(0).error
    dt = time.perf_counter() - t0
    assert err == case.bits, (tag, err)
    check_rejected(b, 0, case.bits, (tag, "past the limit"))
    check_exact(b, 1, of_sib, ph_sib, (tag, "sibling past the limit"))
    b.close()
    if timed:
        assert dt < HANDOFF_S, (tag, dt)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("case", R.FRESH, ids=lambda c: c.name)
def test_fresh_limit(refs, case, where):
    run_fresh(refs, case, R.positions(case.nidx)[where], (case.name, where))


@pytest.mark.parametrize("seg,case,index", [(None, R.SEG_512, 100), ("256", R.SEG_512, 100),
                                            ("256", R.SEG_512, 400), ("256", R.SEG_1024, 100),
                                            (None, R.SEG_COUNT, 100), ("256", R.SEG_COUNT, 100),
                                            ("256", R.SEG_COUNT, 400)],
                         ids=["one_wg", "two_wg_seg0", "two_wg_seg1", "four_wg_seg0",
                              "count_one_wg", "count_two_wg_seg0", "count_two_wg_seg1"])
def test_layout_variants(refs, monkeypatch, seg, case, index):
    """k_layout, then k_layout_seg with the oversize index in segment 0 and in segment 1, then
    four segments with three successors behind the failing one: exact bits (a lost hand-off
    would add RF_AMD_ERR_PAGE_CAP) and no wait. The shapes' limit is the page; fp 22 / lis 7 is
    the one shape of at most 100,000 hashes and more than 256 indices whose limit is the count"""
    if seg is not None:
        monkeypatch.setenv("RF_AMD_LAYOUT_SEG", seg)
    run_fresh(refs, case, index, (case.name, seg, index), timed=True)


def run_incremental(refs, case, index, tag):
    cfg, _ = cfgs(refs.oracle, case.fp, case.lis)
    ho, of_old, hn, of_new, hn_past = refs.incremental(case, index)
    h_sib, of_sib = refs.sibling(case.fp, case.lis)
    ph_sib = probe_set(index + 1, 2, 0, h_sib)
    b1 = E.FilterBatch(cfg, [case.n_old], [case.v_old])
    b1.build_hashes(dev(ho))
    check_exact(b1, 0, of_old, probe_set(index, case.nidx, index, ho), (tag, "old"))
    both = np.concatenate([ho, hn])
    b2 = E.FilterBatch(cfg, [case.n_new, SIB_N], [case.v_new, 0], old=[(b1, 0), None])
    b2.build_hashes(dev(np.concatenate([hn, h_sib])))
    assert b2.infos()[0].error == 0, tag
    check_exact(b2, 0, of_new, probe_set(index, case.nidx, index, both), (tag, "at the limit"))
    check_exact(b2, 1, of_sib, ph_sib, (tag, "sibling at the limit"))
    b2.close()
    b2 = E.FilterBatch(cfg, [case.n_new, SIB_N], [case.v_new, 0], old=[(b1, 0), None])
    b2.build_hashes(dev(np.concatenate([hn_past, h_sib])))
    check_rejected(b2, 0, case.bits, (tag, "past the limit"))
    check_exact(b2, 1, of_sib, ph_sib, (tag, "sibling past the limit"))
    b2.close()
    b1.close()


MODES = {"in_place": None, "decode": "RF_AMD_OLD_DECODE", "wide64": "RF_AMD_WIDE64"}


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", R.INCREMENTAL, ids=lambda c: c.name)
def test_incremental_limit(refs, monkeypatch, case, mode, where):
    """old and new entries cluster in one index of the merged geometry: in place (k_cb_merge and
    the sort it hands back to), by image decode, and with 64-bit entries (fp 31 keeps them in
    every mode)"""
    if MODES[mode]:
        monkeypatch.setenv(MODES[mode], "1")
    run_incremental(refs, case, R.positions(case.nidx)[where], (case.name, mode, where))


@pytest.mark.parametrize("case", [R.INCREMENTAL_BY_NAME["fp26_page"], R.INCREMENTAL_BY_NAME["fp19_count"]],
                         ids=lambda c: c.name)
def test_chained_limit(refs, case):
    """two runs of one chained build; their sum crosses the limit in the second run"""
    index = R.positions(case.nidx)["middle"]
    cfg, _ = cfgs(refs.oracle, case.fp, case.lis)
    ho, _, hn, of_new, hn_past = refs.incremental(case, index)
    h_sib, of_sib = refs.sibling(case.fp, case.lis)
    ph_sib = probe_set(3, 2, 0, h_sib)
    runs = [[(case.n_old, case.v_old), (case.n_new, case.v_new)], [(SIB_N, 0)]]
    b = E.FilterBatch.chained(cfg, runs)
    b.build_hashes(dev(np.concatenate([ho, hn, h_sib])))
    check_exact(b, 0, of_new, probe_set(index, case.nidx, index, np.concatenate([ho, hn])), (case.name, "limit"))
    check_exact(b, 1, of_sib, ph_sib, (case.name, "sibling at the limit"))
    b.close()
    b = E.FilterBatch.chained(cfg, runs)
    b.build_hashes(dev(np.concatenate([ho, hn_past, h_sib])))
    check_rejected(b, 0, case.bits, (case.name, "past"))
    check_exact(b, 1, of_sib, ph_sib, (case.name, "sibling past the limit"))
    b.close()


# ---- 3. every consumer of a rejected filter --------------------------------------------------
N3 = 3000  # probes per form


@pytest.fixture(scope="module")
def rej(refs, oracle):
    """one batch [rejected, healthy] and probes that mix the two filter ids: hashes of the
    rejected filter's clustered index (inserted and not), of the healthy filter, and random
    ones; the same as keys (the healthy filter holds the hashes of the first keys of a pool, and
    the pool's keys whose hashes fall into the clustered index stand for that index)"""
    class W:
        pass
    w = W()
    case = R.FRESH_BY_NAME["fp26_page"]
    w.case, w.index = case, R.positions(case.nidx)["middle"]
    w.cfg, w.ocfg = cfgs(oracle, case.fp, case.lis)
    _, _, w.h_bad = refs.fresh(case, w.index)
    pool = K.random_keys(120_000, seed=0xBAD)
    hpool = oracle.hash_fixed(pool.reshape(-1), 24)
    w.n_ok = 9_000
    w.h_ok = hpool[: w.n_ok].copy()
    w.of_ok = oracle.filter_add(w.ocfg, w.h_ok, value=3)
    w.b = E.FilterBatch(w.cfg, [case.n, w.n_ok], [case.value, 3])
    w.b.build_hashes(dev(np.concatenate([w.h_bad, w.h_ok])))
    torch.cuda.synchronize()
    rng = np.random.default_rng(33)
    lg = case.nidx.bit_length() - 1
    t = N3 // 3
    bad_in = w.h_bad[(w.h_bad >> np.uint32(32 - lg)) == w.index]
    w.ph = np.concatenate([bad_in[rng.integers(0, bad_in.size, size=t // 2)], in_index(rng, case.nidx, w.index, t - t // 2),
                           w.h_ok[rng.integers(0, w.n_ok, size=t)],
                           rng.integers(0, 1 << 32, size=N3 - 2 * t, dtype=np.uint64).astype(np.uint32)])
    kin = np.flatnonzero((hpool >> np.uint32(32 - lg)) == w.index)
    assert kin.size >= t
    pick = np.concatenate([kin[:t], rng.integers(0, w.n_ok, size=t), rng.integers(w.n_ok, pool.shape[0], size=N3 - 2 * t)])
    w.pk = np.ascontiguousarray(pool[pick])
    w.pkh = hpool[pick]
    w.fid = rng.integers(0, 2, size=N3).astype(np.uint32)
    w.fid[:4] = [0, 1, 0, 1]

    def want(h, fid):
        return np.where(fid == 1, w.of_ok.lookup_hashes(h), np.uint64(0))
    w.want = want
    w.want_h, w.want_k = want(w.ph, w.fid), want(w.pkh, w.fid)
    assert (w.want_h[w.fid == 1] != 0).sum() >= t // 4 and (w.want_k[w.fid == 1] != 0).sum() >= t // 4
    # the stale answer this contract forbids would be visible: the oracle finds these hashes in
    # a filter that holds them
    for a in (w.ph, w.pk, w.pkh, w.fid, w.want_h, w.want_k, w.h_bad, w.h_ok):
        a.setflags(write=False)
    yield w
    w.b.close()


def found_buf(n):
    return torch.full((n,), -7, dtype=torch.int64, device="cuda:0")


def got(found):
    torch.cuda.synchronize()
    return found.cpu().numpy().view(np.uint64)


def grouped(w, h):
    """the probes ordered by filter id, and the counts per filter"""
    order = np.argsort(w.fid, kind="stable")
    return order, h[order], [int((w.fid == 0).sum()), int((w.fid == 1).sum())]


def test_rejected_bits(rej):
    check_rejected(rej.b, 0, rej.case.bits, "rejected")
    assert rej.b.info(1).error == 0
    same_image(rej.b.image(1), rej.of_ok, "healthy")


def test_probe_hashes(rej):
    f = found_buf(N3)
    rej.b.probe_hashes(dev(rej.ph), dev(rej.fid), N3, f)
    assert (got(f) == rej.want_h).all()


def test_probe_hashes_runs(rej):
    order, h, counts = grouped(rej, rej.ph)
    f = found_buf(N3)
    rej.b.probe_hashes_runs(dev(h), counts, f)
    assert (got(f) == rej.want_h[order]).all()


def test_probe_keys(rej):
    f = found_buf(N3)
    rej.b.probe_keys(dev(rej.pk), 24, dev(rej.fid), N3, f)
    assert (got(f) == rej.want_k).all()


def test_probe_var_keys(rej):
    offs = np.arange(N3 + 1, dtype=np.uint64) * np.uint64(24)
    f = found_buf(N3)
    rej.b.probe_var_keys(dev(rej.pk.reshape(-1)), dev(offs.view(np.int64)), dev(rej.fid), N3, f)
    assert (got(f) == rej.want_k).all()


def test_probe_pairs(rej):
    pairs = (rej.fid.astype(np.uint64) << np.uint64(32)) | rej.ph.astype(np.uint64)
    f = found_buf(N3)
    rej.b.probe_pairs(dev(pairs.view(np.int64)), N3, f)
    assert (got(f) == rej.want_h).all()


def test_batch_probe_hashes_host(rej):
    assert (host_probe(rej.b, rej.fid, rej.ph) == rej.want_h).all()


def _batches(b, g):
    return (ctypes.c_void_p * g)(*([b.h.value] * g))


def test_probe_filters_host(rej):
    w = rej
    fidx = np.array([0, 1], dtype=np.uint32)
    out = np.full(N3, 0xA5A5, dtype=np.uint64)
    ph, grp = np.ascontiguousarray(w.ph), np.ascontiguousarray(w.fid)
    E._check(lib().rf_amd_probe_filters_host(w.b.engine.h, _batches(w.b, 2), fidx.ctypes.data, 2, ph.ctypes.data,
                                             grp.ctypes.data, N3, out.ctypes.data))
    assert (out == w.want_h).all()


@pytest.mark.parametrize("n", [40, N3], ids=["small", "groups"])
def test_probe_many_hashes_host(rej, n):
    """40 probes travel in the kernel arguments (k_probe_small: at most 64 probes of 8 groups),
    3,000 go through k_probe_groups"""
    w = rej
    # the first 40 probes hold clustered hashes only: take every 75th instead
    sel = np.arange(n) * (N3 // n)
    fid, h = w.fid[sel], w.ph[sel]
    order = np.argsort(fid, kind="stable")
    counts = np.array([(fid == 0).sum(), (fid == 1).sum()], dtype=np.uint64)
    assert counts.min() > 0
    fidx = np.array([0, 1], dtype=np.uint32)
    hs = np.ascontiguousarray(h[order])
    out = np.full(n, 0xA5A5, dtype=np.uint64)
    E._check(lib().rf_amd_probe_many_hashes_host(w.b.engine.h, _batches(w.b, 2), fidx.ctypes.data, counts.ctypes.data,
                                                 2, hs.ctypes.data, out.ctypes.data))
    assert (out == w.want(hs, fid[order])).all()


def test_lookup_server(rej):
    w = rej
    n = 600
    sel = np.arange(n) * (N3 // n)
    out = np.zeros(n, dtype=np.uint64)
    for i, j in enumerate(sel):
        t, r = ctypes.c_uint64(), ctypes.c_uint64(0xA5A5)
        E._check(lib().rf_amd_lookup_submit(w.b.engine.h, w.b.h, int(w.fid[j]), int(w.ph[j]), None, ctypes.byref(t)))
        E._check(lib().rf_amd_lookup_wait(w.b.engine.h, t.value, ctypes.byref(r)))
        out[i] = r.value
    assert (out == w.want_h[sel]).all()


def test_lookup_async(rej):
    la = E.LookupAsync(rej.b, rej.pk, filter_id=rej.fid)
    found = la.wait().copy()
    la.close()
    assert (found == rej.want_k).all()


def test_filter_set(rej):
    """the rejected filter as a member ("a member whose build failed finds nothing")"""
    w = rej
    fs = E.FilterSet([(w.b, 0), (w.b, 1)])
    f = found_buf(2 * N3)
    fs.probe_hashes(dev(w.ph), None, 2, N3, f)
    words = got(f).reshape(N3, 2)
    assert (words[:, 0] == 0).all()
    assert (words[:, 1] == w.of_ok.lookup_hashes(w.ph)).all()
    member = np.stack([w.fid, 1 - w.fid], axis=1).astype(np.uint32)
    f = found_buf(2 * N3)
    fs.probe_hashes(dev(w.ph), dev(member.reshape(-1)), 2, N3, f)
    words = got(f).reshape(N3, 2)
    ok = w.of_ok.lookup_hashes(w.ph)
    assert (words == np.where(member == 1, ok[:, None], np.uint64(0))).all()
    wk = np.stack([np.zeros(N3, dtype=np.uint64), w.of_ok.lookup_hashes(w.pkh)], axis=1)
    d_cand, count = fs.multiget(dev(w.pk), 24, None, 2, N3)
    want = E.found_candidates(wk.reshape(-1))
    assert count == want.size and count > 0
    assert (d_cand[:count].cpu().numpy().view(np.uint64) == want).all()
    fs.close()


def _bad_param(rc):
    assert rc == E.STATUS_BAD_PARAM, (rc, lib().rf_amd_last_error().decode())


def test_calls_that_must_refuse(rej, oracle):
    """image, export, estimate and place_image return STATUS_BAD_PARAM, and so does the host form
    of routing_filter_add given the same hashes; the engine is exact afterwards"""
    w = rej
    L = lib()
    with pytest.raises(E.PlatformStatusError) as ei:
        w.b.image(0)
    assert ei.value.code == E.STATUS_BAD_PARAM
    pages = np.zeros(8 * 4096, dtype=np.uint8)
    slots = np.zeros(w.case.nidx, dtype=np.uint64)
    _bad_param(L.rf_amd_batch_read_image(w.b.h, 0, pages.ctypes.data, pages.size, slots.ctypes.data, slots.size))
    d_pages = torch.zeros(64 * 4096, dtype=torch.uint8, device="cuda:0")
    d_slots = torch.zeros(2 * w.case.nidx, dtype=torch.int64, device="cuda:0")
    with pytest.raises(E.PlatformStatusError) as ei:
        w.b.export(d_pages, d_slots)
    assert ei.value.code == E.STATUS_BAD_PARAM
    for members in ([(w.b, 0), (w.b, 1)], [(w.b, 1), (w.b, 0)]):
        with pytest.raises(E.PlatformStatusError) as ei:
            E.batch_estimate_unique_fp(members)
        assert ei.value.code == E.STATUS_BAD_PARAM
    assert E.batch_estimate_unique_fp([(w.b, 1)]) == oracle.estimate_unique_fp(w.ocfg, [w.of_ok])
    table = ctypes.c_void_p()
    E._check(L.rf_amd_host_alloc(w.b.engine.h, 64 * 8, ctypes.byref(table)))
    try:
        ctypes.memset(table.value, 0, 64 * 8)
        _bad_param(L.rf_amd_batch_place_image(w.b.h, 0, table.value, 1, 0, 1, 0, 512, None))
        assert "build failed" in L.rf_amd_last_error().decode()
        assert bytes((ctypes.c_uint8 * 512).from_address(table.value)) == bytes(512)
    finally:
        L.rf_amd_host_free(w.b.engine.h, table.value)
    with pytest.raises(E.PlatformStatusError) as ei:
        E.routing_filter_add(w.cfg, None, w.h_bad, value=w.case.value)
    assert ei.value.code == E.STATUS_BAD_PARAM
    same_image(E.routing_filter_add(w.cfg, None, w.h_ok, value=3), w.of_ok, "host add after a refusal")
    f = found_buf(N3)
    w.b.probe_hashes(dev(w.ph), dev(w.fid), N3, f)
    assert (got(f) == w.want_h).all()


def test_trim_keeps_the_answers(rej, refs):
    """after rf_amd_batch_trim the work buffers go back to the pool and a new build overwrites
    them; the rejected filter still finds nothing, on the device and from the host"""
    w = rej
    b = E.FilterBatch(w.cfg, [w.case.n, w.n_ok], [w.case.value, 3])
    b.build_hashes(dev(np.concatenate([w.h_bad, w.h_ok])))
    f = found_buf(N3)
    b.probe_hashes(dev(w.ph), dev(w.fid), N3, f)
    assert (got(f) == w.want_h).all()
    assert lib().rf_amd_batch_trim(b.h, None) == 0
    junk = E.FilterBatch(w.cfg, [w.case.n, w.n_ok], [0, 0])
    junk.build_hashes(dev(np.concatenate([w.h_ok[: w.case.n], w.h_ok])))
    torch.cuda.synchronize()
    f = found_buf(N3)
    b.probe_hashes(dev(w.ph), dev(w.fid), N3, f)
    assert (got(f) == w.want_h).all()
    assert (host_probe(b, w.fid, w.ph) == w.want_h).all()
    assert b.info(0).error == w.case.bits
    junk.close()
    b.close()


# ---- 4. rebuilds -----------------------------------------------------------------------------
def good_hashes(refs, case, seed):
    def make():
        rng = np.random.default_rng([case.fp, case.lis, case.n, seed, 99])
        h = rng.integers(0, 1 << 32, size=case.n, dtype=np.uint64).astype(np.uint32)
        return h, refs.oracle.filter_add(refs.oracle.make_config(fingerprint_size=case.fp, log_index_size=case.lis),
                                         h, value=case.value)
    return refs.get(("good", case.name, seed), make)


def after_good(b, case, h, of, h_sib, of_sib, tag):
    assert [i.error for i in b.infos()] == [0, 0], tag
    ph = probe_set(7, case.nidx, 5, h)
    check_exact(b, 0, of, ph, tag)
    assert (host_probe(b, 0, ph) == of.lookup_hashes(ph)).all(), tag
    check_exact(b, 1, of_sib, probe_set(8, 2, 0, h_sib), (tag, "sibling"))


def after_rejecting(b, case, stale, h_sib, of_sib, tag):
    """`stale`: hashes an earlier build of the batch inserted (its slots, pages and lines are
    still in memory); plus hashes of the rejecting build itself"""
    check_rejected(b, 0, case.bits, tag)
    assert (device_probe(b, 0, stale) == 0).all(), (tag, "device probes answer from a stale image")
    assert (host_probe(b, 0, stale) == 0).all(), (tag, "host probes answer from a stale image")
    ph_sib = probe_set(8, 2, 0, h_sib)
    check_exact(b, 1, of_sib, ph_sib, (tag, "sibling"))
    assert (host_probe(b, 1, ph_sib) == of_sib.lookup_hashes(ph_sib)).all(), tag


REBUILD = [(None, R.SEG_512, 100), ("256", R.SEG_512, 100), ("256", R.SEG_512, 400), (None, R.FRESH_BY_NAME["fp20_count"], 33)]
REBUILD_IDS = ["one_wg", "two_wg_seg0", "two_wg_seg1", "one_wg_count"]


@pytest.mark.parametrize("seg,case,index", REBUILD, ids=REBUILD_IDS)
def test_rebuild_good_rejecting_good(refs, monkeypatch, seg, case, index):
    """three builds on one batch: pplans.w, outs.error, the host's error read-back, the hand-off
    tags and the self-cleaned counters all carry over from one build to the next"""
    if seg is not None:
        monkeypatch.setenv("RF_AMD_LAYOUT_SEG", seg)
    cfg, _ = cfgs(refs.oracle, case.fp, case.lis)
    h1, of1 = good_hashes(refs, case, 1)
    h3, of3 = good_hashes(refs, case, 3)
    _, _, h_bad = refs.fresh(case, index)
    h_sib, of_sib = refs.sibling(case.fp, case.lis)
    b = E.FilterBatch(cfg, [case.n, SIB_N], [case.value, 0])
    b.build_hashes(dev(np.concatenate([h1, h_sib])))
    after_good(b, case, h1, of1, h_sib, of_sib, "build 1")
    assert (of1.lookup_hashes(h1[:P]) != 0).all()
    b.build_hashes(dev(np.concatenate([h_bad, h_sib])))
    after_rejecting(b, case, np.concatenate([h1[:P], h_bad[:P]]), h_sib, of_sib, "build 2")
    b.build_hashes(dev(np.concatenate([h3, h_sib])))
    after_good(b, case, h3, of3, h_sib, of_sib, "build 3")
    b.close()


@pytest.mark.parametrize("seg,case,index", REBUILD, ids=REBUILD_IDS)
def test_rebuild_rejecting_first(refs, monkeypatch, seg, case, index):
    if seg is not None:
        monkeypatch.setenv("RF_AMD_LAYOUT_SEG", seg)
    cfg, _ = cfgs(refs.oracle, case.fp, case.lis)
    h3, of3 = good_hashes(refs, case, 3)
    _, _, h_bad = refs.fresh(case, index)
    h_sib, of_sib = refs.sibling(case.fp, case.lis)
    b = E.FilterBatch(cfg, [case.n, SIB_N], [case.value, 0])
    b.build_hashes(dev(np.concatenate([h_bad, h_sib])))
    after_rejecting(b, case, h_bad[:P], h_sib, of_sib, "rejecting build")
    b.build_hashes(dev(np.concatenate([h3, h_sib])))
    after_good(b, case, h3, of3, h_sib, of_sib, "good build")
    b.close()


# ---- 5. a rejected filter as `old` -----------------------------------------------------------
@pytest.mark.parametrize("chained", [False, True], ids=["plain", "chained"])
@pytest.mark.parametrize("trim", [False, True], ids=["resident", "trimmed"])
@pytest.mark.parametrize("mode", list(MODES))
def test_rejected_old_filter(refs, oracle, monkeypatch, mode, trim, chained):
    """A filter built on a rejected old filter is rejected with the old bits in its own, finds
    nothing, and its build reads no slot or page of the old filter (there are none: the old
    batch's slot and page memory holds whatever it held before). Its sibling, built on a healthy
    old filter of the same batch, is exact, and so is the next batch of the engine."""
    if MODES[mode]:
        monkeypatch.setenv(MODES[mode], "1")
    case = R.FRESH_BY_NAME["fp26_page"]
    index = R.positions(case.nidx)["middle"]
    cfg, ocfg = cfgs(oracle, case.fp, case.lis)
    _, _, h_bad = refs.fresh(case, index)
    h_old, of_old = good_hashes(refs, case, 1)
    b1 = E.FilterBatch(cfg, [case.n, case.n], [0, 0])
    b1.build_hashes(dev(np.concatenate([h_bad, h_old])))
    if trim:
        assert lib().rf_amd_batch_trim(b1.h, None) == 0
    n_new = 3000
    rng = np.random.default_rng(5)
    hn = rng.integers(0, 1 << 32, size=(3, n_new), dtype=np.uint64).astype(np.uint32)
    if chained:
        b2 = E.FilterBatch.chained(cfg, [[(n_new, 1), (n_new, 2)], [(n_new, 1)]], old=[(b1, 0), (b1, 1)])
    else:
        b2 = E.FilterBatch(cfg, [2 * n_new, n_new], [1, 1], old=[(b1, 0), (b1, 1)])
    b2.build_hashes(dev(hn.reshape(-1)))
    tag = (mode, trim, chained)
    err = b2.info(0).error
    assert err & case.bits == case.bits and b2.infos()[0].error == err, (tag, err)
    with pytest.raises(E.PlatformStatusError):
        b2.image(0)
    lg = case.nidx.bit_length() - 1
    ph = np.concatenate([h_bad[(h_bad >> np.uint32(32 - lg)) == index][:500], h_bad[:500], hn[0, :500], hn[1, :500]])
    assert (device_probe(b2, 0, ph) == 0).all(), tag
    assert (host_probe(b2, 0, ph) == 0).all(), tag
    of_sib = refs.get(("old_sib",), lambda: oracle.filter_add(ocfg, hn[2], value=1, old=of_old))
    check_exact(b2, 1, of_sib, probe_set(9, case.nidx, index, np.concatenate([h_old, hn[2]])), (tag, "sibling"))
    # the old batch is as it was
    assert b1.info(0).error == case.bits
    check_exact(b1, 1, of_old, probe_set(10, case.nidx, index, h_old), (tag, "old sibling"))
    b2.close()
    h3, of3 = good_hashes(refs, case, 3)
    b3 = E.FilterBatch(cfg, [case.n], [0])
    b3.build_hashes(dev(h3))
    check_exact(b3, 0, of3, probe_set(11, case.nidx, index, h3), (tag, "next batch"))
    b3.close()
    b1.close()
