"""Shapes of the packed-build tests (plain helper module: no fixtures, no pytest settings).

A bitmap build is packed (k4_pack_batch, splinterdb_amd/csrc/rf_batch_plan.h) when every filter
has rvs <= 5, an index of at least 2^7 bits of the bit set and its probe lines cut by K6, which
holds a page's blocks in LDS only from log_index_size 8 on. tests/test_k4_pack_plan.py checks on
the CPU that the oracle builds each shape with the geometry claimed here, and that the planner
takes the decision claimed; tests/test_gpu_k4_pack.py builds them.
"""
from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class Shape:
    name: str    # the "case" line of tests/c/k4_pack_check.cpp
    fp: int
    lis: int
    n: int
    value: int
    rvs: int     # remainder + value bits of an entry
    bits: int    # the in-bucket key: bucket bits inside a coarse bucket + rvs
    packs: bool

    def hashes(self):
        rng = np.random.default_rng([self.fp, self.lis, self.n, self.value])
        return rng.integers(0, 1 << 32, size=self.n, dtype=np.uint64).astype(np.uint32)


SHAPES = [
    # the shapes of tests/test_gpu_k4_bitmap.py
    Shape("s_20000", 18, 8, 20_000, 0, 4, 16, True),       # 4 coarse buckets
    Shape("s_40000_v1", 18, 4, 40_000, 1, 4, 16, False),   # lis 4: pages of more blocks than K6 holds
    Shape("s_100000_v3", 18, 8, 100_000, 3, 4, 16, True),  # value_size 2
    Shape("s_100000", 18, 8, 100_000, 0, 2, 14, True),     # a bit set smaller than the workgroup's share
    Shape("s_300000", 18, 8, 300_000, 0, 0, 12, True),     # no fields at all: 32 buckets per word
    # an index of one word of the bit set (wsh 0 < 2): a K4 thread would span four indices
    Shape("lis3", 18, 3, 70_000, 0, 2, 14, False),
    # a bucket's 2^6 bits span two words of the bit set
    Shape("rvs6", 16, 8, 1_500, 0, 6, 16, False),
    # log_index_size 9: 8 indices in one coarse bucket (and the shape whose index can overflow)
    Shape("lis9_count", 16, 9, 6_000, 0, 4, 16, True),
]
BY_NAME = {s.name: s for s in SHAPES}


def geometry(fp, lis, num_indices, value_size):
    """(rvs, in-bucket key bits) of a filter the oracle built with num_indices indices"""
    lnb = num_indices.bit_length() - 1 + lis
    rvs = fp - lnb + value_size
    return rvs, min(lnb, 12) + rvs
