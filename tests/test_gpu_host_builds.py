"""The host-buffer builds of the C ABI -- rf_amd_batch_build_hashes_host and the two-step
rf_amd_batch_stage_begin / _stage_build / _stage_abort, every routing_filter_add of the drop-in
shim -- against the oracle's routing_filter_add: pages, slots, num_unique and num_pages equal,
and equal to the device-pointer build of the same hashes."""
import ctypes

import numpy as np
import pytest

import host_lookup_cases as H
from splinterdb_amd import engine as E

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KW = dict(fingerprint_size=26, log_index_size=8)
SIZES, VALUES = [5, 3000, 20001], [0, 5, 63]
BIG = 300_000  # 1,200,000 bytes: above the staging buffers' initial 1 MiB (262,144 hashes)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def same_image(img, of, tag):
    assert (img.num_unique, img.num_pages, img.num_indices) == (of.num_unique, of.num_pages, of.num_indices), tag
    assert (img.pages == of.pages()).all(), tag
    assert (img.slots == of.slots()[: of.num_indices]).all(), tag


def same_images(a, b, tag):
    assert (a.num_unique, a.num_pages, a.num_fingerprints, a.value_size) == \
        (b.num_unique, b.num_pages, b.num_fingerprints, b.value_size), tag
    assert (a.pages == b.pages).all() and (a.slots == b.slots).all(), tag


def stage_build(b, runs):
    """the two-step build: filter f's hashes written at its run offset of the staging buffer"""
    L = H.lib()
    p = ctypes.c_void_p()
    E._check(L.rf_amd_batch_stage_begin(b.h, ctypes.byref(p)))
    total = int(sum(len(r) for r in runs))
    stage = np.ctypeslib.as_array((ctypes.c_uint32 * total).from_address(p.value))
    at = np.concatenate([[0], np.cumsum([len(r) for r in runs])])
    for f in reversed(range(len(runs))):  # any order: each writer knows its own offset
        stage[at[f]:at[f + 1]] = runs[f]
    del stage
    E._check(L.rf_amd_batch_stage_build(b.h))


@pytest.fixture(scope="module")
def three(oracle):
    """the three filters' hashes and the oracle's filters, computed once"""
    rng = np.random.default_rng(31)
    h = H.rand_hashes(rng, sum(SIZES))
    at = np.concatenate([[0], np.cumsum(SIZES)])
    runs = [h[at[f]:at[f + 1]] for f in range(3)]
    ocfg = oracle.make_config(**KW)
    ofs = [oracle.filter_add(ocfg, runs[f], value=VALUES[f]) for f in range(3)]
    h.setflags(write=False)
    return h, runs, ofs


def test_three_fresh_filters_host_staged_and_device(three):
    h, runs, ofs = three
    cfg = E.routing_config_init(**KW)
    host, staged, device = (E.FilterBatch(cfg, SIZES, VALUES) for _ in range(3))
    H.host_build(host, h)
    stage_build(staged, runs)
    device.build_hashes(dev(h.copy()))  # h is read-only
    torch.cuda.synchronize()
    for f in range(3):
        assert host.info(f).error == 0 and staged.info(f).error == 0
        img_h, img_s, img_d = host.image(f), staged.image(f), device.image(f)
        same_image(img_h, ofs[f], ("host", f))
        same_image(img_s, ofs[f], ("staged", f))
        same_images(img_h, img_d, ("host vs device", f))
        same_images(img_s, img_d, ("staged vs device", f))
        ph = np.concatenate([runs[f][:200], H.rand_hashes(np.random.default_rng(f), 200)])
        out = H.sentinel_out(ph.size)
        fid = np.full(ph.size, f, dtype=np.uint32)
        E._check(H.lib().rf_amd_batch_probe_hashes_host(staged.h, ph.ctypes.data, fid.ctypes.data, ph.size,
                                                        out.ctypes.data))
        H.check_out(out, ph.size, ofs[f].lookup_hashes(ph), ("staged probe", f))
    for b in (host, staged, device):
        b.close()


def test_staging_grows_and_is_reused(oracle, three):
    """a fresh engine's staging buffers start at 1 MiB: a small build, one of 300,000 hashes
    (the buffers are replaced by larger ones), then the small one again -- through both forms"""
    h, runs, ofs = three
    rng = np.random.default_rng(37)
    hb = H.rand_hashes(rng, BIG)
    of_big = oracle.filter_add(oracle.make_config(**KW), hb, value=1)
    cfg = E.routing_config_init(**KW)
    for how in ("host", "staged"):
        eng = E.Engine(0)
        for k, (sizes, values, hashes, rr, want) in enumerate([(SIZES, VALUES, h, runs, ofs), ([BIG], [1], hb, [hb], [of_big]),
                                                               (SIZES, VALUES, h, runs, ofs)]):
            b = E.FilterBatch(cfg, sizes, values, engine=eng)
            if how == "host":
                H.host_build(b, hashes)
            else:
                stage_build(b, rr)
            for f in range(len(sizes)):
                same_image(b.image(f), want[f], (how, k, f))
            b.close()
        eng.close()


def test_stage_abort_releases_the_staging_buffer(three):
    """stage_begin, stage_abort, then a build from the same thread: it completes (the staging
    lock was released) and is exact"""
    h, runs, ofs = three
    L = H.lib()
    b = E.FilterBatch(E.routing_config_init(**KW), SIZES, VALUES)
    p = ctypes.c_void_p()
    E._check(L.rf_amd_batch_stage_begin(b.h, ctypes.byref(p)))
    assert p.value
    np.ctypeslib.as_array((ctypes.c_uint32 * len(h)).from_address(p.value))[:] = 0xDEADBEEF  # abandoned
    L.rf_amd_batch_stage_abort(b.h)
    H.host_build(b, h)
    for f in range(3):
        same_image(b.image(f), ofs[f], ("after abort", f))
    b.close()


@pytest.mark.parametrize("how", ["host", "staged"])
def test_incremental_add_onto_an_old_filter(oracle, how):
    """9,000 hashes with value 2, then 3,000 more (a third of them the old ones again) with the
    wider value 7 onto that filter: the oracle's filter_add(..., old=...)"""
    rng = np.random.default_rng(41)
    ho = H.rand_hashes(rng, 9000)
    hn = np.concatenate([ho[:1000], H.rand_hashes(rng, 2000)])
    ocfg = oracle.make_config(**KW)
    of_old = oracle.filter_add(ocfg, ho, value=2)
    of_new = oracle.filter_add(ocfg, hn, value=7, old=of_old)
    cfg = E.routing_config_init(**KW)
    old = E.FilterBatch(cfg, [ho.size], [2])
    H.host_build(old, ho)
    same_image(old.image(0), of_old, "old")
    new = E.FilterBatch(cfg, [hn.size], [7], old=[(old, 0)])
    if how == "host":
        H.host_build(new, hn)
    else:
        stage_build(new, [hn])
    img = new.image(0)
    same_image(img, of_new, "old + new")
    assert img.value_size == of_new.value_size == 3
    ph = np.concatenate([ho[:1500], hn[1000:1500], H.rand_hashes(rng, 500)])
    out = H.sentinel_out(ph.size)
    E._check(H.lib().rf_amd_batch_probe_hashes_host(new.h, ph.ctypes.data, None, ph.size, out.ctypes.data))
    want = of_new.lookup_hashes(ph)
    H.check_out(out, ph.size, want, "probe of old + new")
    assert (want[:1000] & np.uint64(0x84) == np.uint64(0x84)).all()
    new.close()
    old.close()


def test_build_error_contract(three):
    h, runs, ofs = three
    L = H.lib()
    assert L.rf_amd_batch_build_hashes_host(None, h.ctypes.data) == E.STATUS_BAD_PARAM
    b = E.FilterBatch(E.routing_config_init(**KW), SIZES, VALUES)
    assert L.rf_amd_batch_build_hashes_host(b.h, None) == E.STATUS_BAD_PARAM
    p = ctypes.c_void_p()
    assert L.rf_amd_batch_stage_begin(None, ctypes.byref(p)) == E.STATUS_BAD_PARAM
    assert L.rf_amd_batch_stage_begin(b.h, None) == E.STATUS_BAD_PARAM
    H.host_build(b, h)  # the refusals held no lock and left the batch buildable
    for f in range(3):
        same_image(b.image(f), ofs[f], ("after refusals", f))
    b.close()
