"""Shared builders of the host-buffer lookup tests (plain helper module: no fixtures, no pytest
settings, no torch).

The host-buffer half of the C ABI -- rf_amd_batch_probe_hashes_host, rf_amd_probe_filters_host,
rf_amd_probe_many_hashes_host -- answers every call through probe_groups_host, which sends it
one of three ways: `small` (hashes and up to 8 filter descriptors in the kernel arguments,
n <= 64), `mapped` (the kernel reads the lookup slot's pinned buffer, n <= 32,768) or `copy`
(one H2D copy first). rf_amd_diag_lookup_paths counts the calls of each way, so every call made
through this module states the way it expects and fails when it went another.

`Reference` holds the inputs and the oracle's filters and words (computed once, read-only);
`World` builds the same filters on an engine through rf_amd_batch_build_hashes_host. Run as a
program (tests/test_gpu_host_lookups.py starts it in child processes, one per setting of the
RF_AMD_PROBE_* switches, which the library reads once per process) it builds a world, makes
CHILD_SIZES calls and checks words and ways against the expectation given on the command line.
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from splinterdb_amd import engine as E  # noqa: E402

SENT = 0xA5A5A5A5A5A5A5A5  # output buffers are pre-filled with it
PAD = 8                     # words past n that must survive
SMALL_PROBES, SMALL_GROUPS, MAPPED_MAX_PROBES = 64, 8, 32768
PATHS = ("small", "mapped", "copy")
SHARE = 300                 # own hashes of each member in the pool, and as many random ones
D_N = 16 * 150              # D: the clustered recipe's own minimum (every hash is clustered)
A0, A1, B, C, D, EK = range(6)  # the six members of a group table
E_MEMBER = 4                # the filter of batch E that is member EK
CHILD_SIZES = (1, 64, 65, 300, 32769, 40000)


def lib():
    return E.load_library()


def paths(reset=False):
    """rf_amd_diag_lookup_paths: calls that went small, mapped, copy; calls waited for by sync"""
    out = np.zeros(4, dtype=np.uint64)
    assert lib().rf_amd_diag_lookup_paths(out.ctypes.data, 1 if reset else 0) == 0
    return out.astype(np.int64)


def default_path(n, ng):
    """the way a call of n probes over ng groups goes when no switch is set"""
    if n <= SMALL_PROBES and ng <= SMALL_GROUPS:
        return "small"
    return "mapped" if n <= MAPPED_MAX_PROBES else "copy"


def one_hot(path, sync=0):
    return np.array([int(path == p) for p in PATHS] + [sync], dtype=np.int64)


def clustered_hashes(rng, fps, lis, n):
    """tests/test_gpu_multiget.py's recipe: 16 clusters of 150 fingerprints in 4 neighbouring
    buckets, so their probe lines overflow and lookups walk the image"""
    lnb = max(int(n).bit_length() - 1, lis)
    rem, sh = fps - lnb, 32 - fps
    h = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    k = 0
    for c in range(16):
        b0 = int(rng.integers(0, (1 << lnb) - 4))
        for j in range(150):
            fp = ((b0 + j % 4) << rem) | (j * 7919 % (1 << rem))
            h[k] = np.uint32((fp << sh) | (j & ((1 << sh) - 1)))
            k += 1
    return h, k, sh


def rand_hashes(rng, n):
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


class Reference:
    """The inputs of batches A-E, the oracle's filter of every one of their filters, the probe
    pool and the oracle's word of every (filter, pool hash). Engine-free and read-only."""

    def __init__(self, oracle):
        rng = np.random.default_rng(20261)
        self.kw26, self.kw20 = dict(fingerprint_size=26, log_index_size=8), dict(fingerprint_size=20, log_index_size=6)
        o26, o20 = oracle.make_config(**self.kw26), oracle.make_config(**self.kw20)
        self.hA = rand_hashes(rng, 5 + 5000)
        self.hB = rand_hashes(rng, 20001)
        self.hC = rand_hashes(rng, 30000)
        self.hD, kd, sh = clustered_hashes(rng, 26, 8, D_N)
        assert kd == D_N
        self.sizesE = [200 + 37 * f for f in range(9)]
        self.valuesE = [f + 1 for f in range(9)]
        self.hE = rand_hashes(rng, sum(self.sizesE))
        offE = np.concatenate([[0], np.cumsum(self.sizesE)])
        ofB_old = oracle.filter_add(o26, self.hB, value=2)
        self.ofs = {
            "A0": oracle.filter_add(o26, self.hA[:5], value=0),
            "A1": oracle.filter_add(o26, self.hA[5:], value=5),
            "B": oracle.filter_add(o26, self.hB[:10000], value=7, old=ofB_old),
            "C": oracle.filter_add(o20, self.hC, value=63),
            "D": oracle.filter_add(o26, self.hD, value=3),
        }
        for f in range(9):
            self.ofs[f"E{f}"] = oracle.filter_add(o26, self.hE[offE[f]:offE[f + 1]], value=self.valuesE[f])
        self.member_names = ["A0", "A1", "B", "C", "D", f"E{E_MEMBER}"]
        # the pool: per member SHARE own hashes (A0 has only 5) and SHARE random ones, then D's
        # clustered hashes and their one-bit neighbours, then 20 own hashes of each filter of E
        own = [self.hA[:5][rng.integers(0, 5, size=SHARE)], self.hA[5:][rng.integers(0, 5000, size=SHARE)],
               self.hB[rng.integers(0, 10000, size=SHARE)],  # of the 10,000 added twice
               self.hC[rng.integers(0, 30000, size=SHARE)], self.hD[rng.integers(0, D_N, size=SHARE)],
               self.hE[offE[E_MEMBER]:offE[E_MEMBER + 1]][rng.integers(0, self.sizesE[E_MEMBER], size=SHARE)]]
        pick = rng.integers(0, D_N, size=SHARE)
        self.own = [np.arange(m * SHARE, (m + 1) * SHARE) for m in range(6)]  # pool indices
        self.near = np.arange(13 * SHARE, 14 * SHARE)
        ownE = [self.hE[offE[f]:offE[f + 1]][rng.integers(0, self.sizesE[f], size=20)] for f in range(9)]
        self.ownE = [np.arange(14 * SHARE + 20 * f, 14 * SHARE + 20 * (f + 1)) for f in range(9)]
        self.pool = np.concatenate(own + [rand_hashes(rng, 6 * SHARE), self.hD[pick],
                                          self.hD[pick] ^ np.uint32(1 << sh)] + ownE)
        self.clustered = np.concatenate([self.own[D], np.arange(12 * SHARE, 13 * SHARE)])
        self.names = list(self.ofs)
        self.row = {nm: i for i, nm in enumerate(self.names)}
        self.words = np.stack([self.ofs[nm].lookup_hashes(self.pool) for nm in self.names])
        self.member_words = np.stack([self.words[self.row[nm]] for nm in self.member_names])
        for a in (self.hA, self.hB, self.hC, self.hD, self.hE, self.pool, self.words, self.member_words):
            a.setflags(write=False)

    def check_reach(self):
        """the oracle's own words reach what the comparisons are meant to cover"""
        mw = self.member_words
        assert (mw[B][self.own[B]] & np.uint64(0x84) == np.uint64(0x84)).all(), "B's probes lack two bits"
        assert (mw[D][self.clustered] >> np.uint64(3) & np.uint64(1)).all(), "D's clustered hashes not found"
        for m in range(6):
            assert mw[m][self.own[m]].all(), f"member {m}: an own hash is not found"
        assert (mw[:, 6 * SHARE:12 * SHARE] == 0).any(), "no probe misses"
        assert (mw[C][self.own[C]] >> np.uint64(63) & np.uint64(1)).all(), "C's value 63 is bit 63"
        for f in range(9):
            assert self.words[self.row[f"E{f}"]][self.ownE[f]].all(), f"E{f}: an own hash is not found"


def host_build(b, hashes):
    h = np.ascontiguousarray(hashes, dtype=np.uint32)
    assert h.size == int(np.sum(b.num_new))
    E._check(lib().rf_amd_batch_build_hashes_host(b.h, h.ctypes.data))


class World:
    """batches A-E of a Reference on one engine, built through the host-buffer build"""

    def __init__(self, ref, engine=None):
        self.ref = ref
        self.engine = engine or E.default_engine()
        cfg26, cfg20 = E.routing_config_init(**ref.kw26), E.routing_config_init(**ref.kw20)
        mk = lambda cfg, sizes, values, old=None: E.FilterBatch(cfg, sizes, values, old=old, engine=self.engine)
        self.A = mk(cfg26, [5, 5000], [0, 5])
        host_build(self.A, ref.hA)
        self.B_old = mk(cfg26, [20001], [2])
        host_build(self.B_old, ref.hB)
        self.B = mk(cfg26, [10000], [7], old=[(self.B_old, 0)])
        host_build(self.B, ref.hB[:10000])
        self.C = mk(cfg20, [30000], [63])
        host_build(self.C, ref.hC)
        self.D = mk(cfg26, [D_N], [3])
        host_build(self.D, ref.hD)
        self.E = mk(cfg26, ref.sizesE, ref.valuesE)
        host_build(self.E, ref.hE)
        self.members = [(self.A, 0), (self.A, 1), (self.B, 0), (self.C, 0), (self.D, 0), (self.E, E_MEMBER)]
        self.batches = [self.A, self.B_old, self.B, self.C, self.D, self.E]
        for b in self.batches:
            for f in range(b.F):
                assert b.info(f).error == 0

    def check_reach(self):
        self.ref.check_reach()
        lines = self.D.debug_lines()
        assert (lines[:, :16] == 0xFF).all(axis=1).any(), "D has no overflowed probe line"
        assert not (lines[:, :16] == 0xFF).all(axis=1).all(), "every line of D overflowed"

    def close(self):
        for b in (self.B, self.B_old, self.A, self.C, self.D, self.E):
            b.close()


def make_table(rng, ng):
    """ng groups drawn from the six members, with repeats; 8 or more hold A1, C and D together
    (two routing configs and overflowed lines in one launch) and B"""
    t = rng.integers(0, 6, size=ng)
    if ng >= 8:
        t[rng.permutation(ng)[:4]] = [A1, C, D, B]
    return t


def table_args(w, table):
    ng = len(table)
    hs = (ctypes.c_void_p * max(1, ng))(*[w.members[m][0].h.value for m in table])
    idx = np.array([w.members[m][1] for m in table] + [0], dtype=np.uint32)
    return hs, idx


def sentinel_out(n):
    return np.full(n + PAD, SENT, dtype=np.uint64)


def check_out(out, n, want, tag):
    assert (out[n:] == np.uint64(SENT)).all(), (tag, "wrote past h_found[n)")
    bad = np.flatnonzero(out[:n] != want)
    assert bad.size == 0, (tag, bad.size, bad[:8].tolist(), out[bad[:4]].tolist(), want[bad[:4]].tolist())


def untouched(out):
    return bool((out == np.uint64(SENT)).all())


def draw(w, rng, table, n, null_group=False):
    """n probes over a group table: pool indices, group ids in [0, ng + 2) with ng, 255, 256 and
    0xFFFFFFFF planted on own hashes of group 0's member (an id that wrapped to group 0 would
    find them), D's clustered hashes and B's twice-added ones planted on their groups when the
    table has them, and the oracle's words"""
    ref, ng = w.ref, len(table)
    table = np.asarray(table)
    idx = rng.integers(0, ref.pool.size, size=n)
    gid = rng.integers(0, ng + 2, size=n).astype(np.uint32)
    planted = {}
    if n >= 16 and not null_group:
        q = min(n // 8, 40)
        for k, (m, src) in enumerate(((D, ref.clustered), (B, ref.own[B]))):
            at = np.flatnonzero(table == m)
            if at.size:
                pos = np.arange(8 + k * q, 8 + (k + 1) * q)
                idx[pos] = src[rng.integers(0, src.size, size=q)]
                gid[pos] = at[0]
                planted[m] = pos
    special = [s for j, s in enumerate((ng, 255, 256, 0xFFFFFFFF)) if 2 * j + 1 < n]
    for j, s in enumerate(special):
        idx[2 * j + 1] = ref.own[table[0]][j]
        gid[2 * j + 1] = s
    if null_group:
        gid[:] = 0
    ok = gid < ng
    want = np.where(ok, ref.member_words[table[np.where(ok, gid, 0)], idx], np.uint64(0))
    return np.ascontiguousarray(ref.pool[idx]), gid, want, planted


def probe_filters(w, table, hashes, gid, n, out):
    hs, idx = table_args(w, table)
    return lib().rf_amd_probe_filters_host(w.engine.h, ctypes.cast(hs, ctypes.c_void_p), idx.ctypes.data, len(table),
                                           hashes.ctypes.data if hashes is not None else None,
                                           gid.ctypes.data if gid is not None else None, n,
                                           out.ctypes.data if out is not None else None)


def run_filters(w, table, n, seed, path="default", sync=0, null_group=False, counted=True):
    """one rf_amd_probe_filters_host call, checked against the oracle and against the way it
    was meant to take; returns (want, planted positions)"""
    rng = np.random.default_rng([seed, n, len(table)])
    hashes, gid, want, planted = draw(w, rng, table, n, null_group)
    out = sentinel_out(n)
    before = paths() if counted else None
    rc = probe_filters(w, table, hashes, None if null_group else gid, n, out)
    assert rc == 0, (n, len(table), rc, lib().rf_amd_last_error())
    tag = (n, len(table), path)
    check_out(out, n, want, tag)
    if not null_group and n >= 8:
        assert (gid >= len(table)).any() and (out[:n][gid >= len(table)] == 0).all(), tag
    if counted:
        p = default_path(n, len(table)) if path == "default" else path
        assert (paths() - before == one_hot(p, sync)).all(), (tag, (paths() - before).tolist())
    return want, planted


# ---- a child process of the switch test ------------------------------------------------------
def child_main(expect):
    """expect: {"paths": {n: way}, "sync": calls waited for by sync}"""
    from oracle import oracle as O
    O.lib()
    w = World(Reference(O))
    w.check_reach()
    table = make_table(np.random.default_rng(8), 8)
    paths(reset=True)
    for n in CHILD_SIZES:
        before = paths()
        run_filters(w, table, n, seed=77, counted=False)
        got = paths() - before
        way = expect["paths"][str(n)]
        sync = 1 if expect["sync"] else 0
        assert (got == one_hot(way, sync)).all(), (n, way, got.tolist())
    total = paths()
    assert total[3] == expect["sync"], total.tolist()
    assert total[:3].sum() == len(CHILD_SIZES), total.tolist()
    w.close()
    print("child: OK", json.dumps(expect))


if __name__ == "__main__":
    child_main(json.loads(sys.argv[1]))
