"""The partition's 16-bit format: a fresh single-run build whose K4 is the bitmap kernel
(k_cb_bitmap) partitions its keys as 16-bit in-bucket keys, packed from each coarse bucket's
unchanged region base, and K4 reads them as pairs; after a spill both kernels are back on 32-bit
entries at the scanned starts. Every image (num_unique, num_pages, page bytes, slots) and 20,000
probes per filter are compared bit-for-bit with the oracle, and each case checks through
rf_amd_diag_part16_builds / rf_amd_diag_k4_bitmap_builds which format its build took."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from splinterdb_amd import engine as E
from splinterdb_amd import keys as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FP = 18
LIS = 8
P = 20000
SORT_CAP = 9216  # rf_plan.h: a coarse bucket's region, and the most entries it takes unspilled
ONE_HASH = 0x9E3779B9  # coarse bucket 2 of four


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _hashes(rng, n):
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


def _cfgs(oracle, lis=LIS):
    return (E.routing_config_init(fingerprint_size=FP, log_index_size=lis),
            oracle.make_config(fingerprint_size=FP, log_index_size=lis))


def _counters():
    L = E.load_library()
    return np.array([L.rf_amd_diag_part16_builds(), L.rf_amd_diag_k4_bitmap_builds()], dtype=np.int64)


def _build(build, part16):
    """one build, which must (or must not) partition into 16-bit keys and run K4 by bitmap"""
    before = _counters()
    build()
    assert (_counters() - before).tolist() == ([1, 1] if part16 else [0, 0])


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


def _four_buckets(of, n):
    """2^14 buckets, so 2^(14 - 12) coarse buckets (the hash's top two bits), and n over the load
    factor under which filter_geometry halves their number"""
    return of.num_indices == 1 << (14 - LIS) and n * 1000 > (1026 << 14)


# ---- every input kind the partition is instantiated for -----------------------------------

N_ODD = 20_001  # a last partial tile, and an odd count in some coarse bucket


def _fixed(key_len):
    keys = K.random_keys(N_ODD, key_len, seed=0x5EED + key_len)
    return keys, None


def _var():
    return K.var_keys(N_ODD)


KINDS = {"keys24": lambda: _fixed(24),  # the paired 12-byte loads
         "keys16": lambda: _fixed(16),  # word reads
         "keys13": lambda: _fixed(13),  # byte reads
         "var": _var,
         "hashes": lambda: (None, None)}


@pytest.mark.parametrize("kind", list(KINDS))
def test_input_kinds(oracle, kind):
    cfg, ocfg = _cfgs(oracle)
    keys, offs = KINDS[kind]()
    if kind == "hashes":
        h = _hashes(np.random.default_rng(21), N_ODD)
    elif offs is not None:
        h = oracle.hash_var(keys, offs)
    else:
        h = oracle.hash_fixed(keys.reshape(-1), keys.shape[1])
    assert (np.bincount(h >> 30, minlength=4) % 2 == 1).any()  # an odd bucket: a half-used last pair
    of = oracle.filter_add(ocfg, h, value=0)
    assert _four_buckets(of, N_ODD)
    b = E.FilterBatch(cfg, [N_ODD], [0])
    if kind == "hashes":
        d = dev(h)
        _build(lambda: b.build_hashes(d), part16=True)
    elif offs is not None:
        db, do = dev(keys), dev(offs.view(np.int64))
        _build(lambda: b.build_var_keys(db, do), part16=True)
    else:
        d = dev(keys)
        _build(lambda: b.build_keys(d, keys.shape[1]), part16=True)
    _same_image(b.image(0), of, kind)
    _check_probes(np.random.default_rng(22), b, 0, of, h, kind)


# ---- key widths 16, 14 and 12 in one batch ------------------------------------------------

def test_three_widths_one_batch(oracle):
    """filters at different e_first offsets; under 16 bits the truncated key still carries
    bucket-number bits, which K4 masks"""
    cfg, ocfg = _cfgs(oracle)
    sizes, bits = [20_000, 100_000, 300_000], [16, 14, 12]
    rng = np.random.default_rng(23)
    hs = [_hashes(rng, n) for n in sizes]
    ofs = [oracle.filter_add(ocfg, h, value=0) for h in hs]
    for of, w in zip(ofs, bits):
        lnb = of.num_indices.bit_length() - 1 + LIS
        assert min(lnb, 12) + (FP - lnb) + of.value_size == w
    b = E.FilterBatch(cfg, sizes, [0, 0, 0])
    d = dev(np.concatenate(hs))
    _build(lambda: b.build_hashes(d), part16=True)
    for f in range(3):
        _same_image(b.image(f), ofs[f], f)
        _check_probes(rng, b, f, ofs[f], hs[f], f)


# ---- a coarse bucket exactly on its limit, and one over -----------------------------------

def _limit_hashes(hot):
    """`hot` entries in coarse bucket 2 and 3,600 / 3,592 / 3,592 in buckets 0 / 1 / 3"""
    rng = np.random.default_rng(24)
    top = np.repeat(np.array([0, 1, 2, 3], dtype=np.uint32), [3_600, 3_592, hot, 3_592])
    h = (_hashes(rng, top.size) >> 2) | (top << 30)
    rng.shuffle(h)
    return h


@pytest.mark.parametrize("hot,spills", [(SORT_CAP, False), (SORT_CAP + 1, True)])
def test_bucket_on_its_limit(oracle, hot, spills):
    """9,216 entries fill the region and stay 16-bit; 9,217 spill: the bucket goes to K4b and its
    neighbours are read as 32-bit entries at the scanned starts. The host takes its decision
    before it knows of a spill, so both builds count."""
    h = _limit_hashes(hot)
    fills = np.bincount(h >> 30, minlength=4)
    assert fills.tolist() == [3_600, 3_592, hot, 3_592] and (fills.max() > SORT_CAP) == spills
    cfg, ocfg = _cfgs(oracle)
    of = oracle.filter_add(ocfg, h, value=0)  # the oracle accepts the input
    assert _four_buckets(of, h.size)
    b = E.FilterBatch(cfg, [h.size], [0])
    d = dev(h)
    _build(lambda: b.build_hashes(d), part16=True)
    _same_image(b.image(0), of, hot)
    _check_probes(np.random.default_rng(25), b, 0, of, h, hot)


# ---- both formats in turn on one batch ----------------------------------------------------

def test_format_switches_on_one_batch(oracle):
    """spilled (32-bit entries at scanned starts), clean (16-bit keys in the regions), spilled
    again: each build over the other format's stale bytes and the counters the last one left"""
    cfg, ocfg = _cfgs(oracle)
    n = 20_000
    spilling = np.full(n, ONE_HASH, dtype=np.uint32)
    clean = _hashes(np.random.default_rng(26), n)
    refs = {id(h): oracle.filter_add(ocfg, h, value=0) for h in (spilling, clean)}
    assert _four_buckets(refs[id(clean)], n)
    b = E.FilterBatch(cfg, [n], [0])
    rng = np.random.default_rng(27)
    for step, h in enumerate((spilling, clean, spilling)):
        d = dev(h)
        _build(lambda: b.build_hashes(d), part16=True)
        _same_image(b.image(0), refs[id(h)], step)
        _check_probes(rng, b, 0, refs[id(h)], h, step)


# ---- builds that keep 32-bit entries ------------------------------------------------------

_CHILD = r"""
import sys
import numpy as np
import torch
from splinterdb_amd import engine as E
lis, fp, src, dst = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
keys = np.load(src)
b = E.FilterBatch(E.routing_config_init(fingerprint_size=fp, log_index_size=lis), [keys.shape[0]], [0])
L = E.load_library()
before = (L.rf_amd_diag_part16_builds(), L.rf_amd_diag_k4_bitmap_builds())
b.build_keys(torch.from_numpy(keys).to("cuda:0"), keys.shape[1])
img = b.image(0)
np.savez(dst, pages=img.pages, slots=img.slots, nums=np.array([img.num_unique, img.num_pages]),
         builds=np.array([L.rf_amd_diag_part16_builds() - before[0], L.rf_amd_diag_k4_bitmap_builds() - before[1]]))
"""


def test_sort_switch_keeps_32_bit_entries(oracle, tmp_path):
    """RF_AMD_K4_BITMAP=0 (read once per process: a child) with 24-byte keys in: the bucket sort
    over 32-bit entries, the same image"""
    cfg, ocfg = _cfgs(oracle)
    keys, _ = _fixed(24)
    of = oracle.filter_add(ocfg, oracle.hash_fixed(keys.reshape(-1), 24), value=0)
    src, dst = str(tmp_path / "keys.npy"), str(tmp_path / "img.npz")
    np.save(src, keys)
    env = dict(os.environ, RF_AMD_K4_BITMAP="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, str(LIS), str(FP), src, dst], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(dst)
    assert z["builds"].tolist() == [0, 0]
    assert tuple(int(x) for x in z["nums"]) == (of.num_unique, of.num_pages)
    assert (z["pages"] == of.pages()).all() and (z["slots"] == of.slots()[: of.num_indices]).all()


def test_ineligible_batch_keeps_32_bit_entries(oracle):
    """one filter with an 18-bit key (5,000 fingerprints) beside an eligible one: the whole batch
    takes the bucket sort over 32-bit entries"""
    cfg, ocfg = _cfgs(oracle)
    rng = np.random.default_rng(28)
    hs = [_hashes(rng, 20_000), _hashes(rng, 5_000)]
    ofs = [oracle.filter_add(ocfg, h, value=0) for h in hs]
    b = E.FilterBatch(cfg, [h.size for h in hs], [0, 0])
    d = dev(np.concatenate(hs))
    _build(lambda: b.build_hashes(d), part16=False)
    for f in range(2):
        _same_image(b.image(f), ofs[f], f)
        _check_probes(rng, b, f, ofs[f], hs[f], f)
