"""The host-buffer lookups of the C ABI -- rf_amd_probe_filters_host, rf_amd_batch_probe_hashes_host
and rf_amd_probe_many_hashes_host, every routing_filter_lookup of the drop-in shim -- against the
oracle's routing_filter_lookup, word for word, on every way probe_groups_host can send a call
(small, mapped, copy), on both sides of each threshold, and with the way each call took read
from rf_amd_diag_lookup_paths. Every output buffer is n + 8 sentinel words: the 8 past n must
survive. Builders and the world are in tests/host_lookup_cases.py."""
import ctypes
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import host_lookup_cases as H
from splinterdb_amd import engine as E

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL = E.STATUS_BAD_PARAM
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 32767, 32768, 32769, 140001]
CASES = [(n, ng) for n in SIZES for ng in ((1, 8, 9, 300) if n <= 65 else (9, 300))]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.fixture(scope="module")
def ref(oracle):
    return H.Reference(oracle)


@pytest.fixture(scope="module")
def world(ref):
    w = H.World(ref)
    yield w
    w.close()


def test_world_reaches_every_property(world):
    """two-bit words, an overflowed line (and lines that did not overflow), every member finds
    its own hashes, some probes miss"""
    world.check_reach()


# ---- rf_amd_probe_filters_host across the size and group boundaries ----------------------------
@pytest.mark.parametrize("n,ng", CASES, ids=[f"n{n}_ng{ng}" for n, ng in CASES])
def test_filters_host_sizes_and_groups(world, n, ng):
    table = H.make_table(np.random.default_rng([ng, n % 7]), ng) if ng > 1 else np.array([n % 6])
    want_path = "small" if n <= 64 and ng <= 8 else ("mapped" if n <= 32768 else "copy")
    assert H.default_path(n, ng) == want_path
    want, planted = H.run_filters(world, table, n, seed=1, path=want_path)
    if n >= 64 and ng >= 8:  # overflowed lines and two-bit words went through this launch
        assert (want[planted[H.D]] >> np.uint64(3) & np.uint64(1)).all()
        assert (want[planted[H.B]] & np.uint64(0x84) == np.uint64(0x84)).all()
    if n >= 257:
        assert want.any() and (want == 0).any()


@pytest.mark.parametrize("n,ng", [(64, 8), (65, 8), (300, 9), (40000, 9)])
def test_filters_host_null_group_array(world, n, ng):
    """h_group == NULL: every probe goes to group 0"""
    table = H.make_table(np.random.default_rng(ng), ng)
    want, _ = H.run_filters(world, table, n, seed=2, null_group=True)
    assert want.any()


def test_small_path_walks_the_image_and_answers_two_bits(world):
    """n = 64 over 8 groups is the largest small call: D's clustered hashes (their lines
    overflowed, so k_probe_small walks the image) and B's twice-added hashes are among the 64"""
    table = H.make_table(np.random.default_rng(5), 8)
    want, planted = H.run_filters(world, table, 64, seed=3, path="small")
    assert planted[H.D].size == 8 and planted[H.B].size == 8
    assert (want[planted[H.D]] >> np.uint64(3) & np.uint64(1)).all()
    assert (want[planted[H.B]] & np.uint64(0x84) == np.uint64(0x84)).all()


# ---- rf_amd_batch_probe_hashes_host ------------------------------------------------------------
def batch_probe(b, hashes, fid, n, out):
    return H.lib().rf_amd_batch_probe_hashes_host(b.h, hashes.ctypes.data if hashes is not None else None,
                                                  fid.ctypes.data if fid is not None else None, n,
                                                  out.ctypes.data if out is not None else None)


def run_batch(w, b, rows, n, ids, seed, path, plant):
    """probe n pool hashes in batch b, whose filter f has the oracle's words rows[f]; plant =
    (pool indices of own hashes, their filter): five probes that must find something"""
    ref, rng = w.ref, np.random.default_rng([seed, n])
    idx = rng.integers(0, ref.pool.size, size=n)
    k0 = 0 if ids is None else len(ids)
    pos = np.arange(k0, k0 + 5)
    idx[pos] = plant[0][:5]
    if ids is None:
        fid, want = None, ref.words[rows[0], idx]
    else:
        fid = np.asarray(ids, dtype=np.uint32)[rng.integers(0, len(ids), size=n)]
        fid[:k0] = np.asarray(ids, dtype=np.uint32)  # every id at least once
        fid[pos] = plant[1]
        ok = fid < len(rows)
        want = np.where(ok, ref.words[np.asarray(rows)[np.where(ok, fid, 0)], idx], np.uint64(0))
        assert (~ok).any() and ok.any()
    hashes = np.ascontiguousarray(ref.pool[idx])
    out = H.sentinel_out(n)
    before = H.paths()
    assert batch_probe(b, hashes, fid, n, out) == 0
    H.check_out(out, n, want, (n, ids, path))
    assert (H.paths() - before == H.one_hot(path)).all(), (n, path, (H.paths() - before).tolist())
    assert want[pos].all()


@pytest.mark.parametrize("n,path", [(40, "small"), (300, "mapped"), (32769, "copy")])
def test_batch_probe_null_ids(world, n, path):
    """h_filter_id == NULL: one group, filter 0"""
    run_batch(world, world.A, [world.ref.row["A0"], world.ref.row["A1"]], n, None, 4, path,
              (world.ref.own[H.A0], 0))


@pytest.mark.parametrize("n,path", [(40, "small"), (300, "mapped")])
def test_batch_probe_ids_past_the_end(world, n, path):
    """ids at or above the batch's two filters find nothing"""
    run_batch(world, world.A, [world.ref.row["A0"], world.ref.row["A1"]], n, [0, 1, 2, 7, 0xFFFFFFFF], 5, path,
              (world.ref.own[H.A1], 1))


def test_batch_probe_nine_filters_is_not_small(world):
    """ids make one group per filter: E's nine groups take 40 probes off the small path"""
    rows = [world.ref.row[f"E{f}"] for f in range(9)]
    run_batch(world, world.E, rows, 40, list(range(11)), 6, "mapped", (world.ref.ownE[8], 8))


# ---- rf_amd_probe_many_hashes_host -------------------------------------------------------------
def run_many(w, table, counts, seed, path):
    ref, rng = w.ref, np.random.default_rng([seed, len(table)])
    n = int(sum(counts))
    gid = np.repeat(np.arange(len(table)), counts)
    idx = rng.integers(0, ref.pool.size, size=n)
    own = rng.random(n) < 0.5  # half of each group's probes are its member's own hashes
    idx[own] = np.asarray(table)[gid[own]] * H.SHARE + rng.integers(0, H.SHARE, size=int(own.sum()))
    hashes = np.ascontiguousarray(ref.pool[idx])
    want = ref.member_words[np.asarray(table)[gid], idx]
    hs, fi = H.table_args(w, table)
    c = np.asarray(counts, dtype=np.uint64)
    out = H.sentinel_out(n)
    before = H.paths()
    rc = H.lib().rf_amd_probe_many_hashes_host(w.engine.h, ctypes.cast(hs, ctypes.c_void_p), fi.ctypes.data,
                                               c.ctypes.data, len(table), hashes.ctypes.data, out.ctypes.data)
    assert rc == 0
    H.check_out(out, n, want, (counts, path))
    delta = H.paths() - before
    assert (delta == (H.one_hot(path) if n else 0)).all(), (counts, path, delta.tolist())
    return out, want


@pytest.mark.parametrize("zero", ["first", "middle", "last"])
def test_many_hashes_zero_count_group(world, zero):
    table = [H.A1, H.C, H.D, H.B, H.EK]
    counts = [7, 30, 11, 40, 19]
    counts[{"first": 0, "middle": 2, "last": 4}[zero]] = 0
    _, want = run_many(world, table, counts, 7, "mapped")  # more than 64 probes
    at = np.cumsum([0] + counts)
    for g in range(5):
        assert counts[g] == 0 or want[at[g]:at[g + 1]].any()


def test_many_hashes_all_counts_zero(world):
    out, _ = run_many(world, [H.A1, H.C, H.D], [0, 0, 0], 8, None)
    assert H.untouched(out)


@pytest.mark.parametrize("total,path", [(64, "small"), (65, "mapped")])
def test_many_hashes_totals_on_the_small_limit(world, total, path):
    run_many(world, [H.A1, H.C, H.D, H.B], [20, 0, 24, total - 44], 9, path)


def test_filters_host_no_groups_finds_nothing(world):
    n = 70
    hashes = np.ascontiguousarray(world.ref.pool[:n])
    out = H.sentinel_out(n)
    before = H.paths()
    rc = H.lib().rf_amd_probe_filters_host(world.engine.h, None, None, 0, hashes.ctypes.data, None, n, out.ctypes.data)
    assert rc == 0
    H.check_out(out, n, np.zeros(n, dtype=np.uint64), "no groups")
    assert (H.paths() == before).all()


# ---- one slot, many shapes ---------------------------------------------------------------------
def test_one_slot_many_shapes(ref):
    """A fresh engine, so its first lookup slot starts with its initial buffers (64 KiB pinned,
    no device buffer), and one thread, so every call takes that slot: multi-block launches back
    to back (the workgroup counter the last workgroup resets), the sequence word, the regrowth
    of the pinned buffer and the allocation and regrowth of the device buffer (40,000 probes
    would fit 1 MiB, 140,001 come first and do not), and the small path in between"""
    eng = E.Engine(0)
    w = H.World(ref, eng)
    try:
        table = H.make_table(np.random.default_rng(11), 8)
        for k, n in enumerate([1, 300, 1, 140001, 64, 40000, 65, 5000, 300]):
            H.run_filters(w, table, n, seed=100 + k)
    finally:
        w.close()
        eng.close()


# ---- concurrency -------------------------------------------------------------------------------
def test_concurrent_callers(world):
    """8 threads, 40 calls each (ctypes releases the GIL during a call), every call checked"""
    sizes = [1, 17, 64, 65, 300, 5000]
    errors, expect = [], np.zeros(4, dtype=np.int64)
    plans = []
    for t in range(8):
        rng = np.random.default_rng([13, t])
        table = H.make_table(rng, [1, 8, 9, 8, 300, 8, 9, 8][t])
        calls = [int(sizes[i]) for i in rng.integers(0, len(sizes), size=40)]
        plans.append((table, calls))
        for n in calls:
            expect += H.one_hot(H.default_path(n, len(table)))

    def worker(t):
        try:
            table, calls = plans[t]
            for k, n in enumerate(calls):
                H.run_filters(world, table, n, seed=1000 * t + k, counted=False)
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((t, repr(e)))

    before = H.paths()
    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors[:3]
    assert (H.paths() - before == expect).all(), ((H.paths() - before).tolist(), expect.tolist())
    assert expect[0] and expect[1]


# ---- a build in flight -------------------------------------------------------------------------
def test_lookup_orders_after_a_build_in_flight(world, oracle):
    """a build issued on the engine stream and not waited for: a host lookup of another batch
    is exact at once, and a host lookup of the batch being built waits for the build"""
    ref, rng = world.ref, np.random.default_rng(17)
    hF = H.rand_hashes(rng, 300_000)
    oF = oracle.filter_add(oracle.make_config(**ref.kw26), hF, value=9)
    n = 300
    phF = H.rand_hashes(rng, n)
    phF[: n // 2] = hF[rng.integers(0, hF.size, size=n // 2)]
    wantF = oF.lookup_hashes(phF)
    idx = rng.integers(0, ref.pool.size, size=n)
    idx[:5] = ref.own[H.A0][:5]
    phA, wantA = np.ascontiguousarray(ref.pool[idx]), ref.words[ref.row["A0"], idx]
    outA, outF = H.sentinel_out(n), H.sentinel_out(n)
    F = E.FilterBatch(E.routing_config_init(**ref.kw26), [hF.size], [9])
    d = dev(hF)
    torch.cuda.synchronize()
    F.build_hashes(d)  # on the engine stream, not waited for
    rcA = batch_probe(world.A, phA, None, n, outA)
    rcF = batch_probe(F, phF, None, n, outF)
    assert (rcA, rcF) == (0, 0)
    H.check_out(outA, n, wantA, "A during F's build")
    H.check_out(outF, n, wantF, "F right after its build was issued")
    assert wantA.any() and (wantF[: n // 2] >> np.uint64(9) & np.uint64(1)).all()
    F.close()


# ---- the error contract ------------------------------------------------------------------------
def test_error_contract(world, ref):
    """every refusal is a host-side argument check: STATUS_BAD_PARAM, output untouched, and the
    next correct call exact"""
    w, n = world, 50
    table = H.make_table(np.random.default_rng(19), 8)
    rng = np.random.default_rng(23)
    hashes, gid, want, _ = H.draw(w, rng, table, n)
    cfg = E.routing_config_init(**ref.kw26)
    unbuilt = E.FilterBatch(cfg, [10], [0])
    eng2 = E.Engine(0)
    foreign = E.FilterBatch(cfg, [5], [0], engine=eng2)
    H.host_build(foreign, ref.hA[:5])

    def groups_with(batch_handle, index):
        hs, fi = H.table_args(w, table)
        hs[3], fi[3] = batch_handle, index
        return hs, fi

    def after_refusal(rc, out, what):
        assert rc == EINVAL, (what, rc)
        assert H.untouched(out), what
        H.run_filters(w, table, n, seed=29)

    L = H.lib()
    for what, (hs, fi) in {"unbuilt group": groups_with(unbuilt.h.value, 0),
                           "foreign group": groups_with(foreign.h.value, 0),
                           "filter index == F": groups_with(w.A.h.value, 2),
                           "filter index > F": groups_with(w.E.h.value, 0xFFFFFFFF)}.items():
        out = H.sentinel_out(n)
        before = H.paths()
        rc = L.rf_amd_probe_filters_host(w.engine.h, ctypes.cast(hs, ctypes.c_void_p), fi.ctypes.data, len(table),
                                         hashes.ctypes.data, gid.ctypes.data, n, out.ctypes.data)
        assert (H.paths() == before).all(), what
        after_refusal(rc, out, what)
    out = H.sentinel_out(n)
    after_refusal(batch_probe(unbuilt, hashes, None, n, out), out, "batch probe of an unbuilt batch")
    after_refusal(H.probe_filters(w, table, None, gid, n, out), out, "NULL hashes")
    after_refusal(H.probe_filters(w, table, hashes, gid, n, None), out, "NULL found")
    after_refusal(batch_probe(w.A, None, None, n, out), out, "batch probe, NULL hashes")
    after_refusal(batch_probe(w.A, hashes, None, n, None), out, "batch probe, NULL found")
    # n == 0 with NULL buffers is OK and touches nothing
    before = H.paths()
    assert H.probe_filters(w, table, None, None, 0, None) == 0
    assert batch_probe(w.A, None, None, 0, None) == 0
    assert (H.paths() == before).all()
    # the foreign batch is sound on its own engine
    out = H.sentinel_out(5)
    h5 = np.ascontiguousarray(ref.hA[:5])
    assert batch_probe(foreign, h5, None, 5, out) == 0
    H.check_out(out, 5, ref.ofs["A0"].lookup_hashes(h5), "foreign batch on its own engine")
    unbuilt.close()
    foreign.close()
    eng2.close()


# ---- the three switches, in fresh child processes ----------------------------------------------
CHILD_TIMEOUT_S = 60  # max(60, 5 x the 0.56 s measured for one child)
SWITCHES = [
    ({"RF_AMD_PROBE_MODE": "mapped"},
     {"paths": {"1": "small", "64": "small", "65": "mapped", "300": "mapped", "32769": "mapped", "40000": "mapped"},
      "sync": 0}),
    ({"RF_AMD_PROBE_MODE": "copy"},
     {"paths": {"1": "small", "64": "small", "65": "copy", "300": "copy", "32769": "copy", "40000": "copy"},
      "sync": 0}),
    ({"RF_AMD_PROBE_SMALL": "0"},
     {"paths": {"1": "mapped", "64": "mapped", "65": "mapped", "300": "mapped", "32769": "copy", "40000": "copy"},
      "sync": 0}),
    ({"RF_AMD_PROBE_WAIT": "sync"},
     {"paths": {"1": "mapped", "64": "mapped", "65": "mapped", "300": "mapped", "32769": "copy", "40000": "copy"},
      "sync": 6}),
    ({"RF_AMD_PROBE_MODE": "copy", "RF_AMD_PROBE_SMALL": "0", "RF_AMD_PROBE_WAIT": "sync"},
     {"paths": {"1": "copy", "64": "copy", "65": "copy", "300": "copy", "32769": "copy", "40000": "copy"},
      "sync": 6}),
]


def test_switches_in_child_processes():
    """RF_AMD_PROBE_MODE, RF_AMD_PROBE_SMALL and RF_AMD_PROBE_WAIT are read once per process, so
    each setting runs in a child of its own (tests/host_lookup_cases.py as a program: the world,
    six calls over an 8-group table, words against the oracle, ways against the expectation).
    The children run one after another and the first that fails ends the test.
    Measured on an MI355X: one child takes 0.34 to 0.56 s of wall time (import, world, six
    calls; it imports no torch). Five times that is under 3 s, so the floor of 60 s is the
    timeout."""
    assert sorted(int(k) for k in SWITCHES[0][1]["paths"]) == sorted(H.CHILD_SIZES)
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_lookup_cases.py")
    for env_add, expect in SWITCHES:
        env = {k: v for k, v in os.environ.items() if not k.startswith("RF_AMD_PROBE_")}
        env.update(env_add)
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, script, json.dumps(expect)], env=env, timeout=CHILD_TIMEOUT_S,
                           capture_output=True, text=True)
        print(f"child {env_add}: {time.perf_counter() - t0:.2f} s")
        assert r.returncode == 0, (env_add, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        assert "child: OK" in r.stdout, (env_add, r.stdout[-2000:])
