"""Stream-ordered release gives the device blocks back to the engine's pool:
rf_amd_batch_destroy_on, rf_amd_filter_set_destroy_on, rf_amd_range_map_destroy_on and
rf_amd_batch_trim park their blocks behind an event on the caller's stream. Once that stream has
been waited for, a reaping rf_amd_engine_pool_trim finds them pooled, and an object of the same
shape takes every one of them back: as many hits as the first creation had misses, no new miss,
nothing left pooled. Each test has an engine of its own, so that no other test's blocks count."""
import numpy as np
import pytest

from splinterdb_amd import engine as E

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REAP = 2 ** 62  # rf_amd_engine_pool_trim keeping this much: reaps the parked blocks, frees nothing


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.fixture
def eng():
    """an engine whose pool takes blocks of these sizes whatever the default limit is"""
    e = E.Engine(0)
    E._check(E.load_library().rf_amd_engine_set_pool_limit(e.h, 1 << 30))
    yield e
    e.close()


def pool_trim(eng, keep):
    E._check(E.load_library().rf_amd_engine_pool_trim(eng.h, keep))


def built_batch(eng, d_h):
    b = E.FilterBatch(E.routing_config_init(log_index_size=8), [d_h.numel()], [3], engine=eng)
    b.build_hashes(d_h)
    torch.cuda.synchronize()
    return b


def hashes(n, seed):
    return dev(np.random.default_rng(seed).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32))


@pytest.mark.parametrize("what", ["batch", "filter_set", "range_map"])
def test_release_on_returns_blocks_to_pool(eng, what):
    L = E.load_library()
    d_h = hashes(1000, 1)
    members = built_batch(eng, hashes(2000, 2)) if what == "filter_set" else None

    def create():
        if what == "batch":
            return built_batch(eng, d_h)
        if what == "filter_set":
            return E.FilterSet([(members, 0), (members, 0)], engine=eng, capacity=8)
        return E.RangeMap([b"f", b"m", b"t"], [[0], [1, 2], [], [3, 4, 5]], engine=eng)

    def release(obj, s):
        if what == "batch":
            obj.close(stream=s)
        else:
            obj.close_on(s)
        assert obj.h is None

    S = torch.cuda.Stream()
    torch.cuda.synchronize()
    pool_trim(eng, 0)
    st0 = eng.pool_stats()
    assert st0["pooled_bytes"] == 0
    obj = create()
    st1 = eng.pool_stats()
    m = st1["misses"] - st0["misses"]
    assert m >= 1
    held = L.rf_amd_batch_device_bytes(obj.h) if what == "batch" else None
    release(obj, S.cuda_stream)
    S.synchronize()
    pool_trim(eng, REAP)
    pooled = eng.pool_stats()["pooled_bytes"]
    assert pooled > 0
    if what == "batch":
        assert pooled == held
    obj = create()
    st2 = eng.pool_stats()
    assert st2["misses"] == st1["misses"]
    assert st2["hits"] == st1["hits"] + m
    assert st2["pooled_bytes"] == 0
    release(obj, S.cuda_stream)
    S.synchronize()
    if members is not None:
        members.close()


def test_batch_trim_returns_blocks_to_pool(eng):
    L = E.load_library()
    S = torch.cuda.Stream()
    torch.cuda.synchronize()
    pool_trim(eng, 0)
    assert eng.pool_stats()["pooled_bytes"] == 0
    b = built_batch(eng, hashes(1000, 3))
    before = L.rf_amd_batch_device_bytes(b.h)
    E._check(L.rf_amd_batch_trim(b.h, S.cuda_stream))
    after = L.rf_amd_batch_device_bytes(b.h)
    assert 0 < after < before
    S.synchronize()
    pool_trim(eng, REAP)
    assert eng.pool_stats()["pooled_bytes"] == before - after
    b.close()
