"""K4 by bitmap (k_cb_bitmap): fresh single-run batches whose in-bucket key (bucket-in-coarse-
bucket bits + remainder and value bits) fits 16 bits sort and deduplicate each coarse bucket as a
bit set in LDS instead of the bucket sort. Every image (num_unique, num_pages, page bytes, slots)
and 20,000 probes per case are compared bit-for-bit with the oracle, and each case checks through
rf_amd_diag_k4_bitmap_builds that its build took the kernel it names."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from splinterdb_amd import engine as E

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FP = 18
# (lis, n, value, key bits): the smallest shapes that reach each way the kernel can go wrong
SHAPES = [(8, 20_000, 0, 16),    # 4 coarse buckets; n above 16,810, so K4 bins of one bucket
          (4, 40_000, 1, 16),    # value_size 1
          (8, 100_000, 3, 16),   # value_size 2
          (8, 100_000, 0, 14),   # bitmap smaller than the workgroup's share: threads without a word
          (8, 300_000, 0, 12)]   # no remainder or value bits at all
P = 20000


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _hashes(rng, n):
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


def _cfgs(oracle, lis, fp=FP):
    return (E.routing_config_init(fingerprint_size=fp, log_index_size=lis),
            oracle.make_config(fingerprint_size=fp, log_index_size=lis))


def bitmap_builds():
    return E.load_library().rf_amd_diag_k4_bitmap_builds()


def _build(b, d_hashes, bitmap):
    """one build, which must (or must not) run K4 as the bitmap kernel"""
    before = bitmap_builds()
    b.build_hashes(d_hashes)
    assert bitmap_builds() - before == (1 if bitmap else 0)


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


@pytest.fixture(scope="module")
def shape_refs(oracle):
    """hashes and the oracle's filter per shape, computed once and never changed"""
    out = {}
    for lis, n, v, bits in SHAPES:
        rng = np.random.default_rng(lis * 1000 + n + v)
        h = _hashes(rng, n)
        out[(lis, n, v, bits)] = (h, oracle.filter_add(oracle.make_config(fingerprint_size=FP, log_index_size=lis),
                                                       h, value=v))
    return out


@pytest.mark.parametrize("lis,n,v,bits", SHAPES)
def test_shapes(oracle, shape_refs, lis, n, v, bits):
    h, of = shape_refs[(lis, n, v, bits)]
    # the key: bucket bits inside a coarse bucket (12 here) + remainder + value bits
    lnb = of.num_indices.bit_length() - 1 + lis
    assert min(lnb, 12) + (FP - lnb) + of.value_size == bits
    cfg, _ = _cfgs(oracle, lis)
    b = E.FilterBatch(cfg, [n], [v])
    _build(b, dev(h), bitmap=True)
    _same_image(b.image(0), of, (lis, n, v))
    _check_probes(np.random.default_rng(n), b, 0, of, h, (lis, n, v))


def test_duplicate_heavy(oracle):
    """20,000 hashes drawn from 2,500 distinct ones: most entries fall on a set bit"""
    rng = np.random.default_rng(12)
    h = _hashes(rng, 2_500)[rng.integers(0, 2_500, size=20_000)]
    cfg, ocfg = _cfgs(oracle, 8)
    of = oracle.filter_add(ocfg, h, value=0)
    b = E.FilterBatch(cfg, [h.size], [0])
    _build(b, dev(h), bitmap=True)
    _same_image(b.image(0), of, "dup")
    _check_probes(rng, b, 0, of, h, "dup")


def test_one_hash_spills_to_k4b(oracle):
    """20,000 copies of one hash: a coarse bucket over its region, so the partition spills and
    the bitmap kernel hands the bucket to K4b"""
    rng = np.random.default_rng(13)
    h = np.full(20_000, 0x9E3779B9, dtype=np.uint32)
    cfg, ocfg = _cfgs(oracle, 8)
    of = oracle.filter_add(ocfg, h, value=0)
    b = E.FilterBatch(cfg, [h.size], [0])
    _build(b, dev(h), bitmap=True)
    _same_image(b.image(0), of, "one hash")
    _check_probes(rng, b, 0, of, h, "one hash")


def test_spill_with_live_neighbours(oracle):
    """12,000 copies of one hash among 8,000 others: the partition spills, so every bucket is
    read and written at its scanned start (any parity: the 4-byte copy-out beside the 8-byte
    one), the hot bucket goes to K4b and its neighbours stay with the bitmap kernel"""
    rng = np.random.default_rng(15)
    # the four coarse buckets are the hash's top two bits: 2,001 / 1,999 / the hot one / 4,000
    top = np.repeat(np.array([0, 1, 3], dtype=np.uint32), [2_001, 1_999, 4_000])
    h = np.concatenate([np.full(12_000, 0x9E3779B9, dtype=np.uint32), (_hashes(rng, 8_000) >> 2) | (top << 30)])
    rng.shuffle(h)
    starts = np.cumsum(np.bincount(h >> 30, minlength=4))
    assert starts[0] % 2 == 1 and starts[2] % 2 == 0  # bucket 1 starts odd, bucket 3 even
    cfg, ocfg = _cfgs(oracle, 8)
    of = oracle.filter_add(ocfg, h, value=0)
    b = E.FilterBatch(cfg, [h.size], [0])
    _build(b, dev(h), bitmap=True)
    _same_image(b.image(0), of, "spill")
    _check_probes(rng, b, 0, of, h, "spill")


def test_rebuild_same_batch(oracle, shape_refs):
    """twice on one batch: the counters the first build leaves clean for the second"""
    key = SHAPES[0]
    h, of = shape_refs[key]
    cfg, _ = _cfgs(oracle, key[0])
    b = E.FilterBatch(cfg, [key[1]], [key[2]])
    d = dev(h)
    _build(b, d, bitmap=True)
    img1 = b.image(0)
    _build(b, d, bitmap=True)
    img2 = b.image(0)
    _same_image(img1, of, "first")
    _same_image(img2, of, "second")
    _check_probes(np.random.default_rng(5), b, 0, of, h, "second")


def test_mixed_batch_takes_the_sort(oracle, shape_refs):
    """an eligible filter beside one with an 18-bit key (5,000 fingerprints: one coarse bucket
    of 12 bucket bits and 6 remainder bits): the whole batch falls back to the bucket sort"""
    key = SHAPES[0]
    h0, of0 = shape_refs[key]
    rng = np.random.default_rng(14)
    h1 = _hashes(rng, 5_000)
    cfg, ocfg = _cfgs(oracle, key[0])
    of1 = oracle.filter_add(ocfg, h1, value=0)
    b = E.FilterBatch(cfg, [h0.size, h1.size], [0, 0])
    _build(b, dev(np.concatenate([h0, h1])), bitmap=False)
    _same_image(b.image(0), of0, 0)
    _same_image(b.image(1), of1, 1)
    _check_probes(rng, b, 0, of0, h0, 0)
    _check_probes(rng, b, 1, of1, h1, 1)


_CHILD = r"""
import sys
import numpy as np
import torch
from splinterdb_amd import engine as E
lis, fp, v, src, dst = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
h = np.load(src)
b = E.FilterBatch(E.routing_config_init(fingerprint_size=fp, log_index_size=lis), [h.size], [v])
before = E.load_library().rf_amd_diag_k4_bitmap_builds()
b.build_hashes(torch.from_numpy(h).to("cuda:0"))
img = b.image(0)
np.savez(dst, pages=img.pages, slots=img.slots, nums=np.array([img.num_unique, img.num_pages]),
         bitmap_builds=np.array([E.load_library().rf_amd_diag_k4_bitmap_builds() - before]))
"""


def test_sort_switch_gives_the_same_image(oracle, shape_refs, tmp_path):
    """RF_AMD_K4_BITMAP=0 (read once per process: a child) builds the shape with the bucket sort;
    its image equals the bitmap path's"""
    key = SHAPES[2]
    lis, n, v, _ = key
    h, of = shape_refs[key]
    cfg, _ = _cfgs(oracle, lis)
    b = E.FilterBatch(cfg, [n], [v])
    _build(b, dev(h), bitmap=True)
    img = b.image(0)
    _same_image(img, of, "bitmap")
    src, dst = str(tmp_path / "h.npy"), str(tmp_path / "img.npz")
    np.save(src, h)
    env = dict(os.environ, RF_AMD_K4_BITMAP="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, str(lis), str(FP), str(v), src, dst], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(dst)
    assert int(z["bitmap_builds"][0]) == 0
    assert tuple(int(x) for x in z["nums"]) == (img.num_unique, img.num_pages)
    assert (z["pages"] == img.pages).all() and (z["slots"] == img.slots).all()
