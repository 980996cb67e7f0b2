"""Packed builds: a bitmap build whose every filter has rvs <= 5 and its probe lines cut by K6
(k4_pack_batch) has K4 write each index block's body -- unary encoding and remainder fields, built
from the coarse bucket's bit set -- instead of the sorted entries, and K6 place the bodies in their
pages; a build whose partition spills keeps the sorted entries, chosen on the device. Every image
(num_unique, num_pages, page bytes, slots) and 20,000 probes per case are compared bit-for-bit with
the oracle, the probe lines as built with those k_plines re-cuts from the image, and each case
checks through rf_amd_diag_k4_packed_builds which launch its build took. The geometry each shape
claims is checked against the oracle on the CPU (tests/test_k4_pack_plan.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import k4_pack_cases as C
import reject_cases as R
import test_gpu_part16 as P16  # the inputs with a coarse bucket on its limit
from conftest import ROOT
from splinterdb_amd import engine as E

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

P = 20000
SORT_CAP = 9216  # rf_plan.h
ONE_HASH = 0x9E3779B9


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _hashes(rng, n):
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


def _cfgs(oracle, fp, lis):
    return (E.routing_config_init(fingerprint_size=fp, log_index_size=lis),
            oracle.make_config(fingerprint_size=fp, log_index_size=lis))


def _counters():
    L = E.load_library()
    return np.array([L.rf_amd_diag_k4_packed_builds(), L.rf_amd_diag_k4_bitmap_builds()], dtype=np.int64)


def _build(build, packed, bitmap=True):
    """one build, which must (or must not) be launched packed"""
    before = _counters()
    build()
    assert (_counters() - before).tolist() == [int(packed), int(bitmap)]


def _same_image(img, of, tag):
    assert (img.num_unique, img.num_pages) == (of.num_unique, of.num_pages), tag
    assert (img.pages == of.pages()).all(), tag
    assert (img.slots == of.slots()[: of.num_indices]).all(), tag


def _check_probes(rng, b, f, of, inserted, tag):
    ph = np.concatenate([inserted[rng.integers(0, inserted.size, size=P // 2)],
                         rng.integers(0, 1 << 32, size=P - P // 2, dtype=np.uint64).astype(np.uint32)])
    found = torch.zeros(P, dtype=torch.int64, device="cuda:0")
    b.probe_hashes(dev(ph), dev(np.full(P, f, dtype=np.uint32)), P, found)
    torch.cuda.synchronize()
    assert (found.cpu().numpy().view(np.uint64) == of.lookup_hashes(ph)).all(), tag


def _check_lines(b, tag):
    """the lines the build cut equal those k_plines cuts from the finished image"""
    built = b.debug_lines()
    b.debug_rebuild_lines()
    rebuilt = b.debug_lines()
    assert built.shape == rebuilt.shape and built.shape[0] > 0, tag
    bad = np.flatnonzero((built != rebuilt).any(axis=1))
    assert bad.size == 0, (tag, bad.size, bad[:8].tolist())


def _check_all(rng, b, f, of, inserted, tag):
    _same_image(b.image(f), of, tag)
    _check_probes(rng, b, f, of, inserted, tag)


@pytest.fixture(scope="module")
def shape_refs(oracle):
    """hashes and the oracle's filter per shape, computed once and never changed"""
    out = {}
    for s in C.SHAPES:
        h = s.hashes()
        out[s.name] = (h, oracle.filter_add(oracle.make_config(fingerprint_size=s.fp, log_index_size=s.lis),
                                            h, value=s.value))
    return out


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: s.name)
def test_shapes(oracle, shape_refs, shape):
    h, of = shape_refs[shape.name]
    assert C.geometry(shape.fp, shape.lis, of.num_indices, of.value_size) == (shape.rvs, shape.bits)
    cfg, _ = _cfgs(oracle, shape.fp, shape.lis)
    b = E.FilterBatch(cfg, [shape.n], [shape.value])
    d = dev(h)
    _build(lambda: b.build_hashes(d), packed=shape.packs)
    _check_all(np.random.default_rng(shape.n), b, 0, of, h, shape.name)
    _check_lines(b, shape.name)
    _check_probes(np.random.default_rng(shape.n + 1), b, 0, of, h, (shape.name, "re-cut lines"))


def test_three_filters_one_batch(oracle, shape_refs):
    """filters of different rvs (4, 2, 0) at different region offsets in one packed batch"""
    names = ["s_20000", "s_100000", "s_300000"]
    cfg, _ = _cfgs(oracle, 18, 8)
    b = E.FilterBatch(cfg, [C.BY_NAME[k].n for k in names], [0, 0, 0])
    d = dev(np.concatenate([shape_refs[k][0] for k in names]))
    _build(lambda: b.build_hashes(d), packed=True)
    rng = np.random.default_rng(31)
    for f, k in enumerate(names):
        _check_all(rng, b, f, shape_refs[k][1], shape_refs[k][0], k)
    _check_lines(b, "three")


def test_duplicate_heavy(oracle):
    """20,000 hashes drawn from 2,500 distinct ones: most entries fall on a set bit"""
    rng = np.random.default_rng(12)
    h = _hashes(rng, 2_500)[rng.integers(0, 2_500, size=20_000)]
    cfg, ocfg = _cfgs(oracle, 18, 8)
    of = oracle.filter_add(ocfg, h, value=0)
    b = E.FilterBatch(cfg, [h.size], [0])
    d = dev(h)
    _build(lambda: b.build_hashes(d), packed=True)
    _check_all(rng, b, 0, of, h, "dup")
    _check_lines(b, "dup")


@pytest.mark.parametrize("hot,spills", [(SORT_CAP, False), (SORT_CAP + 1, True)])
def test_bucket_on_its_limit(oracle, hot, spills):
    """9,216 entries fill a coarse bucket's region and pack; 9,217 spill: K4 takes its current
    emission (the bucket goes to K4b) and K6 its entry runs. The host launches both packed: it
    decides before it knows of a spill."""
    h = P16._limit_hashes(hot)
    fills = np.bincount(h >> 30, minlength=4)
    assert fills.tolist() == [3_600, 3_592, hot, 3_592] and (fills.max() > SORT_CAP) == spills
    cfg, ocfg = _cfgs(oracle, 18, 8)
    of = oracle.filter_add(ocfg, h, value=0)
    b = E.FilterBatch(cfg, [h.size], [0])
    d = dev(h)
    _build(lambda: b.build_hashes(d), packed=True)
    _check_all(np.random.default_rng(25), b, 0, of, h, hot)
    _check_lines(b, hot)


def test_format_switches_on_one_batch(oracle):
    """packed, spilled (sorted entries at the scanned starts), packed again: each build over the
    other format's stale bytes in the regions and the counters the last one left"""
    cfg, ocfg = _cfgs(oracle, 18, 8)
    n = 20_000
    spilling = np.full(n, ONE_HASH, dtype=np.uint32)
    clean = _hashes(np.random.default_rng(26), n)
    refs = {id(h): oracle.filter_add(ocfg, h, value=0) for h in (spilling, clean)}
    b = E.FilterBatch(cfg, [n], [0])
    rng = np.random.default_rng(27)
    for step, h in enumerate((clean, spilling, clean)):
        d = dev(h)
        _build(lambda: b.build_hashes(d), packed=True)
        _check_all(rng, b, 0, refs[id(h)], h, step)
        _check_lines(b, step)


# ---- an incremental add onto a packed batch: its image is decoded ------------------------------

MODES = {"in_place": None, "decode": "RF_AMD_OLD_DECODE", "wide64": "RF_AMD_WIDE64"}  # test_gpu_rejected.py


@pytest.mark.parametrize("old_spilled", [False, True], ids=["old_packed", "old_spilled"])
@pytest.mark.parametrize("mode", list(MODES))
def test_add_onto_packed_batch(oracle, monkeypatch, shape_refs, mode, old_spilled):
    """the old batch was launched packed, so it holds no sorted entries the add could read in place
    (whether or not its build spilled, which the host cannot know)"""
    if MODES[mode]:
        monkeypatch.setenv(MODES[mode], "1")
    cfg, ocfg = _cfgs(oracle, 18, 8)
    if old_spilled:
        ho = np.full(20_000, ONE_HASH, dtype=np.uint32)
        of_old = oracle.filter_add(ocfg, ho, value=0)
    else:
        ho, of_old = shape_refs["s_20000"]
    hn = _hashes(np.random.default_rng(41), 8_000)
    of_new = oracle.filter_add(ocfg, hn, value=1, old=of_old)
    b1 = E.FilterBatch(cfg, [ho.size], [0])
    d1 = dev(ho)
    _build(lambda: b1.build_hashes(d1), packed=True)
    b2 = E.FilterBatch(cfg, [hn.size], [1], old=[(b1, 0)])
    d2 = dev(hn)
    _build(lambda: b2.build_hashes(d2), packed=False, bitmap=False)
    _check_all(np.random.default_rng(42), b2, 0, of_new, np.concatenate([ho, hn]), (mode, old_spilled))
    _check_all(np.random.default_rng(43), b1, 0, of_old, ho, (mode, old_spilled, "old"))
    b2.close()
    b1.close()


# ---- a rejected filter inside a packed batch ---------------------------------------------------

# fingerprint 16 / lis 9 with 6,000 hashes: 8 indices of 2^13 distinct fingerprints each and rvs 4,
# so an index can take more than 4,096 entries (RF_AMD_ERR_INDEX_OVERFLOW) in a batch that packs
REJECT = R._fresh("fp16_lis9_count", 16, 9, 6_000, 0)


def test_rejected_filter_in_packed_batch(oracle, shape_refs):
    case = REJECT
    assert (case.rvs, case.nidx, case.limit, case.bits) == (4, 8, 4096, R.ERR_INDEX_OVERFLOW)
    index = R.positions(case.nidx)["middle"]
    cfg, ocfg = _cfgs(oracle, case.fp, case.lis)
    h_sib, of_sib = shape_refs["lis9_count"]
    h_lim, h_past = case.hashes(case.limit, index), case.hashes(case.past, index)
    of_lim = oracle.filter_add(ocfg, h_lim, value=0)
    rng = np.random.default_rng(51)
    for h, rejected in ((h_lim, False), (h_past, True)):
        b = E.FilterBatch(cfg, [case.n, h_sib.size], [0, 0])
        d = dev(np.concatenate([h, h_sib]))
        _build(lambda: b.build_hashes(d), packed=True)
        if rejected:
            assert b.info(0).error == case.bits and b.infos()[0].error == case.bits
            with pytest.raises(E.PlatformStatusError) as ei:
                b.image(0)
            assert ei.value.code == E.STATUS_BAD_PARAM
        else:
            assert b.info(0).error == 0
            _check_all(rng, b, 0, of_lim, h_lim, "at the limit")
        _check_all(rng, b, 1, of_sib, h_sib, ("sibling", rejected))
        b.close()


# ---- export and import -------------------------------------------------------------------------

def test_export_import(oracle, shape_refs):
    h, of = shape_refs["s_100000_v3"]
    s = C.BY_NAME["s_100000_v3"]
    cfg, _ = _cfgs(oracle, s.fp, s.lis)
    b = E.FilterBatch(cfg, [s.n], [s.value])
    d = dev(h)
    _build(lambda: b.build_hashes(d), packed=True)
    lines = b.debug_lines()
    infos, pbytes, nslots = b.export_sizes()
    d_p = torch.zeros(pbytes, dtype=torch.uint8, device="cuda:0")
    d_s = torch.zeros(nslots, dtype=torch.int64, device="cuda:0")
    b.export(d_p, d_s)
    torch.cuda.synchronize()
    imp = E.FilterBatch.imported(b.cfg, infos, d_p, d_s)
    try:
        assert (imp.debug_lines() == lines).all()
        _check_all(np.random.default_rng(61), imp, 0, of, h, "imported")
    finally:
        imp.close()


# ---- the switches, read once per process: children ---------------------------------------------

_CHILD = r"""
import sys
import numpy as np
import torch
from splinterdb_amd import engine as E
lis, fp, v, src, dst = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
h = np.load(src)
L = E.load_library()
b = E.FilterBatch(E.routing_config_init(fingerprint_size=fp, log_index_size=lis), [h.size], [v])
before = (L.rf_amd_diag_k4_packed_builds(), L.rf_amd_diag_k4_bitmap_builds(), L.rf_amd_diag_dense_line_filters())
b.build_hashes(torch.from_numpy(h).to("cuda:0"))
after = (L.rf_amd_diag_k4_packed_builds(), L.rf_amd_diag_k4_bitmap_builds(), L.rf_amd_diag_dense_line_filters())
img = b.image(0)
built = b.debug_lines()
b.debug_rebuild_lines()
np.savez(dst, pages=img.pages, slots=img.slots, nums=np.array([img.num_unique, img.num_pages]),
         counts=np.array(after) - np.array(before), built=built, rebuilt=b.debug_lines())
"""


def _child(tmp_path, shape, h, env):
    src, dst = str(tmp_path / "h.npy"), str(tmp_path / "img.npz")
    np.save(src, h)
    r = subprocess.run([sys.executable, "-c", _CHILD, str(shape.lis), str(shape.fp), str(shape.value), src, dst],
                       cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(dst)


def test_dense_lines(oracle, shape_refs, tmp_path):
    """RF_AMD_LINES_DENSE=1: the packed K6 cuts dense lines (G = 52 buckets here)"""
    s = C.BY_NAME["s_20000"]
    h, of = shape_refs[s.name]
    z = _child(tmp_path, s, h, {"RF_AMD_LINES_DENSE": "1"})
    assert z["counts"].tolist() == [1, 1, 1]
    assert tuple(int(x) for x in z["nums"]) == (of.num_unique, of.num_pages)
    assert (z["pages"] == of.pages()).all() and (z["slots"] == of.slots()[: of.num_indices]).all()
    assert z["built"].shape[0] > 0 and (z["built"] == z["rebuilt"]).all()


def test_pack_switch_gives_the_same_image(oracle, shape_refs, tmp_path):
    """RF_AMD_K4_PACK=0 builds the shape from sorted entries; image and lines equal the packed ones"""
    s = C.BY_NAME["s_100000_v3"]
    h, of = shape_refs[s.name]
    cfg, _ = _cfgs(oracle, s.fp, s.lis)
    b = E.FilterBatch(cfg, [s.n], [s.value])
    d = dev(h)
    _build(lambda: b.build_hashes(d), packed=True)
    img, lines = b.image(0), b.debug_lines()
    _same_image(img, of, "packed")
    z = _child(tmp_path, s, h, {"RF_AMD_K4_PACK": "0"})
    assert z["counts"].tolist()[:2] == [0, 1]
    assert tuple(int(x) for x in z["nums"]) == (img.num_unique, img.num_pages)
    assert (z["pages"] == img.pages).all() and (z["slots"] == img.slots).all()
    assert (z["built"] == lines).all()
