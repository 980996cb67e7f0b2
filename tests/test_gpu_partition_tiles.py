"""The fused partition of 24-byte keys (k_hash_scatter, IN_KEYS24) at tile and slot edges: the
first and last key slot, a wave's partial slot, one tile exactly, a one-key second tile, filters
and key buffers that start at 8 mod 16, the flagged (incremental) and chained instantiations,
and a spill out of the ranking loop. Every image is compared byte for byte with the oracle's
routing_filter_add of the same hashes, and every inserted key must be found."""
import numpy as np
import pytest
import torch

from splinterdb_amd import engine as E
from splinterdb_amd import keys as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_image(img, of, what):
    assert (img.num_unique, img.num_pages) == (of.num_unique, of.num_pages), what
    assert (img.pages == of.pages()).all(), what
    assert (img.slots == of.slots()[: of.num_indices]).all(), what


def all_found(b, d_keys, sizes, values, fids=None):
    """sizes[i] keys under values[i] in filter fids[i] (default: filter i)"""
    n = int(sum(sizes))
    fids = np.arange(len(sizes)) if fids is None else np.asarray(fids)
    fid = dev(np.repeat(fids.astype(np.uint32), sizes))
    found = torch.zeros(n, dtype=torch.int64, device=DEV)
    b.probe_keys(d_keys, 24, fid, n, found)
    torch.cuda.synchronize()
    got = found.cpu().numpy().view(np.uint64)
    vals = np.repeat(np.asarray(values, dtype=np.uint64), sizes)
    assert ((got >> vals) & np.uint64(1)).all(), "false negative"


def build_and_check(oracle, sizes, values, offset=0, start=0):
    """one batch from consecutive K.seq_keys, the key buffer's base moved by `offset` bytes"""
    cfg, ocfg = E.routing_config_init(), oracle.make_config()
    keys = K.seq_keys(start, int(sum(sizes)))
    buf = torch.zeros(offset + keys.size, dtype=torch.uint8, device=DEV)
    buf[offset:] = dev(keys.reshape(-1))
    d_keys = buf[offset:]
    assert d_keys.data_ptr() % 16 == offset % 16
    b = E.FilterBatch(cfg, sizes, values)
    b.build_keys(d_keys, 24)
    hashes = oracle.hash_fixed(keys.reshape(-1), 24)
    s = 0
    for f, (n, v) in enumerate(zip(sizes, values)):
        same_image(b.image(f), oracle.filter_add(ocfg, hashes[s:s + n], value=v), (sizes, f))
        s += n
    all_found(b, d_keys, sizes, values)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 16383, 16384, 16385, 32833])
def test_one_filter(oracle, n):
    build_and_check(oracle, [n], [0])


def test_batch_filters_start_at_8_mod_16(oracle):
    sizes = [16385, 70001, 33]
    # the second filter follows an odd number of keys (the third, 86,386 keys in, is aligned again)
    assert (sizes[0] * 24) % 16 == 8 and ((sizes[0] + sizes[1]) * 24) % 16 == 0
    build_and_check(oracle, sizes, [0, 0, 0])


def test_batch_key_buffer_offset_by_8(oracle):
    build_and_check(oracle, [16385, 70001, 33], [0, 0, 0], offset=8)


def test_non_zero_value(oracle):
    build_and_check(oracle, [16385, 70001, 33], [3, 0, 7])


def test_incremental_add_flagged_32bit(oracle):
    """an add onto a built filter with fp_size + value_size <= 31: the FL instantiation"""
    cfg, ocfg = E.routing_config_init(), oracle.make_config()
    n0, n1 = 40000, 32833
    k0, k1 = K.seq_keys(0, n0), K.seq_keys(n0 - 500, n1)  # 500 keys again, under the new value
    b0 = E.FilterBatch(cfg, [n0], [1])
    b0.build_keys(dev(k0), 24)
    of0 = oracle.filter_add(ocfg, oracle.hash_fixed(k0.reshape(-1), 24), value=1)
    same_image(b0.image(0), of0, "base")
    b1 = E.FilterBatch(cfg, [n1], [2], old=[(b0, 0)])
    d1 = dev(k1)
    b1.build_keys(d1, 24)
    of1 = oracle.filter_add(ocfg, oracle.hash_fixed(k1.reshape(-1), 24), value=2, old=of0)
    same_image(b1.image(0), of1, "incremental")
    all_found(b1, d1, [n1], [2])


def test_chained_batch_runs(oracle):
    """FilterBatch.chained: the RUNS instantiation (a tile's value and end come from its run)"""
    cfg, ocfg = E.routing_config_init(), oracle.make_config()
    runs = [[(16385, 0), (2049, 1), (33, 4)], [(65, 2), (20001, 3)]]
    total = sum(c for r in runs for c, _ in r)
    keys = K.seq_keys(0, total)
    d_keys = dev(keys)
    b = E.FilterBatch.chained(cfg, runs)
    b.build_keys(d_keys, 24)
    hashes = oracle.hash_fixed(keys.reshape(-1), 24)
    s = 0
    for f, r in enumerate(runs):
        of = None
        for c, v in r:
            of = oracle.filter_add(ocfg, hashes[s:s + c], value=v, old=of)
            s += c
        same_image(b.image(f), of, f)
    # every key of every run is found under its run's value, in its filter
    all_found(b, d_keys, [c for r in runs for c, _ in r], [v for r in runs for _, v in r],
              fids=[f for f, r in enumerate(runs) for _ in r])


def test_one_key_20000_times_spills(oracle):
    """20,000 copies of one key: one coarse bucket exceeds SORT_CAP, the spill word rises out of
    the ranking loop and the gated kernels rebuild the partition"""
    cfg, ocfg = E.routing_config_init(), oracle.make_config()
    n = 20000
    keys = K.ids_keys(np.full(n, 12345, dtype=np.uint64))
    d_keys = dev(keys)
    b = E.FilterBatch(cfg, [n], [0])
    b.build_keys(d_keys, 24)
    same_image(b.image(0), oracle.filter_add(ocfg, oracle.hash_fixed(keys.reshape(-1), 24), value=0), "spill")
    all_found(b, d_keys, [n], [0])
