"""rf_amd_batch_place_image (kernel k_place) at the C ABI: a filter's image pages scattered to
their destinations in registered host memory and its index slots rebased to disk addresses and
spread over index pages, compared byte for byte with rf_amd_batch_read_image (itself pinned to
the oracle by the parity tests). The destination is one anonymous mapping filled with a sentinel
byte: image pages go to a random permutation of its even page slots, the odd ones are guards,
the index pages sit at its end, and after every call the WHOLE mapping must equal the expected
bytes -- so a store to a guard, past an index page's last slot or to a page outside the
requested range fails the comparison. Disk addresses are above 2^40."""
import ctypes
import mmap
from types import SimpleNamespace

import numpy as np
import pytest

import host_lookup_cases as H
from splinterdb_amd import engine as E

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KW = dict(fingerprint_size=26, log_index_size=8)
SIZES, VALUES = [5, 200_000], [0, 3]
SENT = 0xA5
EINVAL = E.STATUS_BAD_PARAM
MAX_INDEX_PAGES = 8


@pytest.fixture(scope="module")
def ctx(oracle):
    """the batch, its images, the registered mapping and the table"""
    c = SimpleNamespace()
    c.L, c.eng, c.P = H.lib(), E.default_engine(), 4096
    rng = np.random.default_rng(43)
    h = H.rand_hashes(rng, sum(SIZES))
    c.b = E.FilterBatch(E.routing_config_init(**KW), SIZES, VALUES)
    H.host_build(c.b, h)
    c.imgs = [c.b.image(f) for f in range(2)]
    ocfg = oracle.make_config(**KW)
    for f, (lo, hi) in enumerate([(0, 5), (5, sum(SIZES))]):  # the expected bytes are the oracle's
        of = oracle.filter_add(ocfg, h[lo:hi], value=VALUES[f])
        assert (c.imgs[f].pages == of.pages()).all() and (c.imgs[f].slots == of.slots()[: of.num_indices]).all()
    assert c.imgs[0].num_indices == 1 and c.imgs[1].num_indices == 512 and c.imgs[1].num_pages >= 20
    c.slots_total = 2 * max(i.num_pages for i in c.imgs) + MAX_INDEX_PAGES
    c.size = c.slots_total * c.P
    c.mm = mmap.mmap(-1, c.size)
    c.other = mmap.mmap(-1, 4 * c.P)  # never registered
    c.anchor = ctypes.c_char.from_buffer(c.mm)
    c.other_anchor = ctypes.c_char.from_buffer(c.other)
    c.base, c.other_base = ctypes.addressof(c.anchor), ctypes.addressof(c.other_anchor)
    assert c.base % c.P == 0
    c.mem = np.ctypeslib.as_array((ctypes.c_uint8 * c.size).from_address(c.base))
    c.mem[:] = SENT
    c.words = c.slots_total + 16
    tp = ctypes.c_void_p()
    E._check(c.L.rf_amd_host_alloc(c.eng.h, 8 * c.words, ctypes.byref(tp)))
    c.table_ptr = tp.value
    c.table = np.ctypeslib.as_array((ctypes.c_uint64 * c.words).from_address(tp.value))
    E._check(c.L.rf_amd_host_register(c.eng.h, c.base, c.size))
    try:
        yield c
    finally:
        c.L.rf_amd_engine_sync(c.eng.h)
        assert c.L.rf_amd_host_unregister(c.eng.h, c.base) == 0
        c.L.rf_amd_host_free(c.eng.h, c.table_ptr)
        c.b.close()
        del c.mem, c.table, c.anchor, c.other_anchor


def layout(c, f, app, seed):
    """fills the table for filter f: destinations (page slot 2 * perm[k] of the mapping), disk
    addresses, index page destinations (the mapping's last pages)"""
    img = c.imgs[f]
    npg, nidx = img.num_pages, img.num_indices
    nip = (nidx + app - 1) // app
    assert nip <= MAX_INDEX_PAGES and 2 * npg + nip <= c.slots_total
    rng = np.random.default_rng([seed, f, app])
    lay = SimpleNamespace(f=f, app=app, npg=npg, nidx=nidx, nip=nip)
    lay.dest_off = (2 * rng.permutation(npg) * c.P).astype(np.uint64)
    lay.disk = (np.uint64(1 << 40) + rng.permutation(1 << 20)[:npg].astype(np.uint64) * np.uint64(3 * c.P))
    lay.idx_off = (c.size - (nip - np.arange(nip)) * c.P).astype(np.uint64)
    c.mem[:] = SENT
    c.table[:] = 0
    c.table[:npg] = np.uint64(c.base) + lay.dest_off
    c.table[npg:2 * npg] = lay.disk
    c.table[2 * npg:2 * npg + nip] = np.uint64(c.base) + lay.idx_off
    assert len(set(lay.disk.tolist())) == npg and (lay.disk > (1 << 40)).all()
    return lay


def expected(c, lay, first, last, with_index):
    """the mapping after image pages [first, last) and, with_index, the index were placed"""
    img, P = c.imgs[lay.f], c.P
    exp = np.full(c.size, SENT, dtype=np.uint8)
    for k in range(first, last):
        o = int(lay.dest_off[k])
        exp[o:o + P] = img.pages[k * P:(k + 1) * P]
    if with_index:
        s = img.slots.astype(np.uint64)
        v = lay.disk[(s // np.uint64(P)).astype(np.int64)] + s % np.uint64(P)
        w = exp.view(np.uint64)
        i = np.arange(lay.nidx)
        w[(lay.idx_off[i // lay.app] // np.uint64(8)).astype(np.int64) + i % lay.app] = v
    return exp


def place(c, lay, first, count, with_index, f=None, app=None, npg=None):
    return c.L.rf_amd_batch_place_image(c.b.h, lay.f if f is None else f, c.table_ptr,
                                        lay.npg if npg is None else npg, first, count, with_index,
                                        lay.app if app is None else app, None)


def fence(c):
    fv = ctypes.c_uint64(0)
    E._check(c.L.rf_amd_engine_fence(c.eng.h, ctypes.byref(fv)))
    E._check(c.L.rf_amd_engine_fence_wait(c.eng.h, fv.value))


def check_mapping(c, lay, exp, tag):
    bad = np.flatnonzero(c.mem != exp)
    if bad.size:
        page = int(bad[0]) // c.P
        kind = ("index page" if page >= c.slots_total - lay.nip else
                "guard" if page % 2 or page >= 2 * lay.npg else f"image page {int(np.flatnonzero(lay.dest_off == page * c.P)[0])}")
        raise AssertionError((tag, f"{bad.size} bytes differ, first at page slot {page} ({kind}) + {int(bad[0]) % c.P}",
                              c.mem[bad[:8]].tolist(), exp[bad[:8]].tolist()))
    assert (c.table[lay.npg:2 * lay.npg] == lay.disk).all(), (tag, "disk addresses changed")


@pytest.mark.parametrize("app", [512, 100])
@pytest.mark.parametrize("f", [0, 1])
def test_whole_image_in_one_call(ctx, f, app):
    """every destination page equals its image page, index word i % app of index page i / app
    is disk[slot / P] + slot % P, guards and the words past the last slot stay sentinel"""
    c = ctx
    lay = layout(c, f, app, 1)
    if (f, app) == (1, 100):
        assert lay.nip == 6 and lay.nidx - 5 * app == 12
    assert place(c, lay, 0, lay.npg, 1) == 0
    fence(c)
    exp = expected(c, lay, 0, lay.npg, True)
    assert (exp != SENT).any()
    check_mapping(c, lay, exp, (f, app))


@pytest.mark.parametrize("f", [0, 1])
def test_three_disjoint_ranges(ctx, f):
    """[0, a) and [a, b) without the index, then [b, num_pages) with it, on one table (the
    entries a call uses are translated in place, so the ranges are disjoint)"""
    c = ctx
    lay = layout(c, f, 100, 2)
    a, b = lay.npg // 3, 2 * lay.npg // 3
    assert place(c, lay, 0, a, 0) == 0
    fence(c)
    check_mapping(c, lay, expected(c, lay, 0, a, False), (f, "after the first range"))
    assert place(c, lay, a, b - a, 0) == 0
    assert place(c, lay, b, lay.npg - b, 1) == 0
    fence(c)
    check_mapping(c, lay, expected(c, lay, 0, lay.npg, True), (f, "after all three"))


@pytest.mark.parametrize("f", [0, 1])
def test_zero_count_calls(ctx, f):
    c = ctx
    lay = layout(c, f, 100, 3)
    assert place(c, lay, 0, 0, 0) == 0  # nothing to do: OK, nothing written
    fence(c)
    check_mapping(c, lay, np.full(c.size, SENT, dtype=np.uint8), (f, "count 0, no index"))
    assert place(c, lay, lay.npg, 0, 1) == 0  # the index only
    fence(c)
    exp = expected(c, lay, 0, 0, True)
    assert (exp != SENT).any()
    check_mapping(c, lay, exp, (f, "count 0, index only"))


def test_refusals_write_nothing_and_keep_the_table(ctx):
    """every refusal is a host-side argument check made before the launch: STATUS_BAD_PARAM, the
    mapping all sentinel, the table as the caller filled it"""
    c = ctx
    lay = layout(c, 1, 100, 4)
    mid = lay.npg // 2
    clean = c.table.copy()
    cases = {
        "destination outside every registered range": ({mid: c.other_base}, {}),
        "destination whose last byte is past the range": ({mid: c.base + c.size - c.P + 16}, {}),
        "index page outside every registered range": ({2 * lay.npg + lay.nip - 1: c.other_base + c.P}, {}),
        "first_page + count > num_pages": ({}, dict(first=1, count=lay.npg)),
        "first_page > num_pages": ({}, dict(first=lay.npg + 1, count=0)),
        "addrs_per_page == 0": ({}, dict(app=0)),
        "addrs_per_page * 8 > page_size": ({}, dict(app=513)),
        "f >= F": ({}, dict(f=2)),
    }
    for what, (poke, kw) in cases.items():
        c.table[:] = clean
        for k, v in poke.items():
            c.table[k] = v
        before = c.table.copy()
        rc = place(c, lay, kw.get("first", 0), kw.get("count", lay.npg), 1, f=kw.get("f"), app=kw.get("app"))
        assert rc == EINVAL, (what, rc)
        fence(c)
        assert (c.table == before).all(), (what, "the table changed")
        assert (c.mem == SENT).all(), (what, "the mapping was written")
    # and the same table, mended, places exactly
    c.table[:] = clean
    assert place(c, lay, 0, lay.npg, 1) == 0
    fence(c)
    check_mapping(c, lay, expected(c, lay, 0, lay.npg, True), "after the refusals")


def test_registration_contract(ctx):
    c = ctx
    L = c.L
    assert L.rf_amd_host_register(c.eng.h, c.base + c.P, 2 * c.P) == EINVAL      # inside
    assert L.rf_amd_host_register(c.eng.h, c.base, c.size) == EINVAL             # the same
    assert L.rf_amd_host_register(c.eng.h, c.base + c.size - c.P, c.P) == EINVAL  # its last page
    assert L.rf_amd_host_unregister(c.eng.h, c.base + c.P) == EINVAL             # not a range's base
    assert L.rf_amd_host_unregister(c.eng.h, c.other_base) == EINVAL             # never registered
    assert L.rf_amd_host_register(c.eng.h, None, c.P) == EINVAL
    assert L.rf_amd_host_register(c.eng.h, c.other_base, 0) == EINVAL
    lay = layout(c, 1, 512, 5)  # the registered range is still the one the placement checks
    assert place(c, lay, 0, lay.npg, 1) == 0
    fence(c)
    check_mapping(c, lay, expected(c, lay, 0, lay.npg, True), "after the registration refusals")
