"""Inputs that sit exactly on the limits at which a filter is rejected (plain helper module:
no fixtures, no pytest settings).

A filter is rejected when one index holds more than 4,096 entries (RF_AMD_ERR_INDEX_OVERFLOW)
or when one index block is larger than a page (RF_AMD_ERR_BLOCK_TOO_BIG). The block of an index
with c entries takes (oracle/rf_oracle.c:541-544, block_size in rf_kernels.hip)

    bytes(c) = (c + index_size - 1) / 8 + 4 + 2 + (c == 0 ? 3 : (c * rvs - 1) / 8 + 4)

with rvs = fingerprint_size - log2(num_indices) - log_index_size + value_size. `cmax` is the
largest c <= 4096 with bytes(c) <= page_size. The hash arrays built here hold exactly c distinct
fingerprints in a chosen index and no other hash in that index, so an array made for cmax is
accepted and one made for cmax + 1 is rejected; tests/test_reject_limits.py proves both with
the oracle for every case below, and that the geometry is the one cmax was computed from.
"""
from dataclasses import dataclass

import numpy as np

PAGE_SIZE = 4096
FPS_PER_INDEX = 4096  # ROUTING_FPS_PER_PAGE: the reference's fp_buffer
ERR_INDEX_OVERFLOW, ERR_BLOCK_TOO_BIG = 1, 2  # RF_AMD_ERR_* (include/rf_amd.h)


def value_size(value):
    return int(value).bit_length()


def num_indices(n, lis):
    """indices of a filter of n fingerprints (log_num_buckets, oracle/rf_oracle.c:219-223)"""
    return 1 << (max(int(n).bit_length() - 1, lis) - lis)


def rvs_of(fp, lis, n, value):
    """remainder + value bits of an entry of a filter of n fingerprints"""
    return fp - max(int(n).bit_length() - 1, lis) + value_size(value)


def block_bytes(c, lis, rvs):
    rbs = 3 if c * rvs == 0 else (c * rvs - 1) // 8 + 4
    return (c + (1 << lis) - 1) // 8 + 4 + 2 + rbs


def cmax(lis, rvs):
    """the most entries an index can hold"""
    c = FPS_PER_INDEX
    while block_bytes(c, lis, rvs) > PAGE_SIZE:
        c -= 1
    return c


def error_bits(c, lis, rvs):
    """the RF_AMD_ERR_* bits of a filter whose fullest index holds c entries"""
    return ((ERR_INDEX_OVERFLOW if c > FPS_PER_INDEX else 0) |
            (ERR_BLOCK_TOO_BIG if block_bytes(c, lis, rvs) > PAGE_SIZE else 0))


def clustered(fp, lis, nidx, n, c, index, seed):
    """n 32-bit hashes of a filter (or of one add of a chain) whose result has nidx indices:
    exactly c of them, with c distinct fingerprints, lie in `index`; the others are random
    hashes of the other indices (a random hash that falls into `index` keeps its low bits and
    moves to another index). In random order."""
    lg = nidx.bit_length() - 1
    assert nidx == 1 << lg and lg >= 1 and 0 <= index < nidx and c <= min(n, 1 << (fp - lg))
    rng = np.random.default_rng(seed)
    h = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    inside = (h >> (32 - lg)) == index
    other = (index + 1 + rng.integers(0, nidx - 1, size=n, dtype=np.uint64)) % nidx
    h = np.where(inside, (h & ((1 << (32 - lg)) - 1)) | (other << (32 - lg)), h)
    # c distinct fingerprints of `index`; the bits below the fingerprint stay random
    low = rng.choice(1 << (fp - lg), size=c, replace=False).astype(np.uint64)
    h[:c] = (index << (32 - lg)) | (low << (32 - fp)) | (h[:c] & ((1 << (32 - fp)) - 1))
    h = h.astype(np.uint32)
    assert int(((h >> np.uint32(32 - lg)) == index).sum()) == c
    return h[rng.permutation(n)]


def positions(nidx):
    """the chosen index first, in the middle and last"""
    return {"first": 0, "middle": nidx // 2 + 1, "last": nidx - 1}


@dataclass(frozen=True)
class Fresh:
    """one filter built from n hashes: `limit` entries in one index are accepted, `past` are
    rejected with exactly the bits `bits`"""
    name: str
    fp: int
    lis: int
    n: int
    value: int
    nidx: int   # the geometry the limits below were computed from
    rvs: int
    limit: int
    past: int
    bits: int

    def hashes(self, c, index, seed=0):
        return clustered(self.fp, self.lis, self.nidx, self.n, c, index,
                         [self.fp, self.lis, self.n, self.value, c, index, seed])


def _fresh(name, fp, lis, n, value, past=None):
    rvs = rvs_of(fp, lis, n, value)
    lim = cmax(lis, rvs)
    past = lim + 1 if past is None else past
    return Fresh(name, fp, lis, n, value, num_indices(n, lis), rvs, lim, past, error_bits(past, lis, rvs))


# the limit is the entry count (4,096) in the first two, the page in the others; the last is
# past both
FRESH = [
    _fresh("fp20_count", 20, 8, 20_000, 0),
    _fresh("fp22_count", 22, 8, 100_000, 0),
    _fresh("fp26_page", 26, 8, 9_000, 0),
    _fresh("fp26_v5_page", 26, 8, 9_000, 5),
    _fresh("fp32_page", 32, 8, 9_000, 0),
    _fresh("fp22_lis4_page", 22, 4, 9_000, 0),
    _fresh("fp26_both", 26, 8, 9_000, 0, past=4097),
]
FRESH_BY_NAME = {c.name: c for c in FRESH}
# the layout variants (RF_AMD_LAYOUT_SEG=256): fp 22 / lis 4 has 512 indices (two workgroups of
# 256), and with 18,000 hashes 1,024 (four workgroups, so three successors of a failing segment 0)
SEG_512 = FRESH_BY_NAME["fp22_lis4_page"]
SEG_1024 = _fresh("fp22_lis4_1024", 22, 4, 18_000, 0)
# the entry count as the limit of a filter of more than 256 indices: an index holds 2^(lis + rem)
# distinct fingerprints and 4,096 entries fit a page only with rvs <= 6, so lis 7 and 2^16 buckets
SEG_COUNT = _fresh("fp22_lis7_count", 22, 7, 70_000, 0)


@dataclass(frozen=True)
class Incremental:
    """an add of n_new hashes (value v_new) onto a filter of n_old hashes (value v_old): the old
    and the new entries cluster in the same index of the merged geometry, and entries of
    different values never merge, so the index holds c_old + c_new entries. (c_old, c_new) =
    `limit` is accepted and `past` rejected with exactly `bits`; c_old alone is far below the
    old filter's own limit."""
    name: str
    fp: int
    lis: int
    n_old: int
    n_new: int
    v_old: int
    v_new: int
    nidx: int
    rvs: int
    limit: tuple
    past: tuple
    bits: int

    def old_hashes(self, c, index, seed=0):
        return clustered(self.fp, self.lis, self.nidx, self.n_old, c, index,
                         [self.fp, self.lis, self.n_old, self.v_old, c, index, seed, 1])

    def new_hashes(self, c, index, seed=0):
        return clustered(self.fp, self.lis, self.nidx, self.n_new, c, index,
                         [self.fp, self.lis, self.n_new, self.v_new, c, index, seed, 2])


def _incremental(name, fp, lis, n_old, n_new, v_old=0, v_new=1):
    rvs = rvs_of(fp, lis, n_old + n_new, v_new)
    lim = cmax(lis, rvs)
    half = lim // 2
    assert lim == 2 * half
    return Incremental(name, fp, lis, n_old, n_new, v_old, v_new, num_indices(n_old + n_new, lis), rvs,
                       (half, half), (half, half + 1), error_bits(lim + 1, lis, rvs))


# fp 26: the page (rvs 14, 2,162 entries); fp 20: the page (rvs 7, 4,056); fp 19: the entry
# count alone (rvs 6 once the value has widened: 4,096 entries take 3,624 bytes); fp 31: the
# value's bit takes fp_size + value_size to 32, so the build keeps 64-bit entries
INCREMENTAL = [
    _incremental("fp26_page", 26, 8, 9_000, 3_000),
    _incremental("fp20_page", 20, 8, 20_000, 8_000),
    _incremental("fp19_count", 19, 8, 20_000, 8_000),
    _incremental("fp31_wide", 31, 8, 9_000, 3_000),
]
INCREMENTAL_BY_NAME = {c.name: c for c in INCREMENTAL}
