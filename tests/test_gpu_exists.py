"""The existence multi-get: rf_amd_filter_set_exists_{keys,var_keys,hashes} and their _ragged
forms (the EXISTS instantiations of k_probe_fanout / k_probe_fanout_ragged), FilterSet.exists_routed
and exists_var_routed. Every byte is compared with E.exists_host of the oracle's words
(routing_filter_lookup, src/routing_filter.c:985-1073), the mirror itself being checked against
the reference's existence lookup in test_exists_host.py. The world is test_gpu_multiget's with
test_gpu_multiget_ragged's probes and lists; the set is test_gpu_unfiltered_members'
(A0, UNFILTERED, None, B0, UNFILTERED, D0). d_exists is pre-filled with 0xAB and lies between
guard regions of 0xAB bytes that must stay as they were."""
import numpy as np
import pytest

import test_gpu_multiget as MG
import test_gpu_multiget_ragged as RG
import test_gpu_range_route as RR
import test_gpu_unfiltered_members as UM
from splinterdb_amd import engine as E
from test_gpu_multiget import world  # noqa: F401  (the fixture; a fresh instance for this module)
from test_gpu_multiget_ragged import rag  # noqa: F401
from test_gpu_range_route import routed  # noqa: F401
from test_gpu_unfiltered_members import mixed  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, NM = MG.N, RG.NM
FORMS = RG.FORMS
KINDS = UM.KINDS
WORLD_KINDS = [E.KIND_FILTER, E.KIND_FILTER, E.KIND_NULL, E.KIND_FILTER, E.KIND_FILTER, E.KIND_FILTER]
GUARD = 256
FILL = 0xAB
dev = RG.dev


class Out:
    """n bytes of d_exists, `shift` bytes off a 16-byte boundary, between guard regions"""

    def __init__(self, n, shift=0):
        self.n, self.lo = n, GUARD + shift
        self.buf = torch.full((self.lo + n + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.lo

    def read(self):
        torch.cuda.synchronize()
        a = self.buf.cpu().numpy()
        assert (a[:self.lo] == FILL).all(), "wrote before d_exists"
        assert (a[self.lo + self.n:] == FILL).all(), "wrote at or past d_exists + n"
        return a[self.lo:self.lo + self.n].copy()


def run_ragged(fset, form, args, counts, member, first=0, shift=0):
    """one ragged existence call over whole arrays (d_member holds `first` ids before the offsets'
    range); returns (bytes, whole member array, offsets) for the mirror"""
    n = len(counts)
    off = RG.offsets_of(counts, first)
    whole = np.full(first + len(member) + 64, 1, dtype=np.uint32)  # id 1: unfiltered, were it read
    whole[first:first + len(member)] = member
    out = Out(n, shift)
    fn = {"hashes": fset.exists_hashes_ragged, "keys": fset.exists_keys_ragged,
          "var": fset.exists_var_keys_ragged}[form]
    keep = (dev(whole), dev(off.view(np.int64)))
    fn(*args, *keep, n, out.ptr)
    return out.read(), whole, off


def run_fixed(fset, form, args, member, k, n=N, shift=0):
    out = Out(n, shift)
    fn = {"hashes": fset.exists_hashes, "keys": fset.exists_keys, "var": fset.exists_var_keys}[form]
    keep = None if member is None else dev(member.reshape(-1))
    fn(*args, keep, k, n, out.ptr)
    return out.read()


def pair_words(words, counts, member, first=0):
    """the oracle's word of every pair, indexed by the absolute pair (`first` zeros before)"""
    w = np.zeros(first + len(member) + 64, dtype=np.uint64)
    w[first:first + len(member)] = RG.want_pairs(words, counts, member)
    return w


def check(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


# ---- the fixed forms --------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", [1, 3, 5, None])
def test_fixed_forms(world, rag, mixed, form, k):  # noqa: F811
    w, r = world, rag
    kk = NM if k is None else k
    member = None if k is None else w.member[k]
    got = run_fixed(mixed, form, RG.inputs(w, r, form), member, kk)
    flat = np.tile(np.arange(NM, dtype=np.uint32), N) if k is None else member.reshape(-1)
    words = RG.want_pairs(r.words[form], np.full(N, kk), flat)
    want = E.exists_host_fixed(words, KINDS, None if k is None else flat, kk)
    check(got, want, (form, k))
    if k is None:
        assert (got & 2 == 2).all()
    else:  # one member cannot give both bits
        assert set(got.tolist()) == ({0, 1, 2} if k == 1 else {0, 1, 2, 3})


# ---- the ragged forms -------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_ragged_lists(world, rag, mixed, form, shift):  # noqa: F811
    """lists of 0-9 ids and of 64, 128 and 300, a whole wave of keys without pairs, an empty run
    across a wave boundary, the variable-length key past the 4-KiB window; d_exists at every
    byte alignment"""
    w, r = world, rag
    got, whole, off = run_ragged(mixed, form, RG.inputs(w, r, form), r.counts, r.member, shift=shift)
    want = E.exists_host(pair_words(r.words[form], r.counts, r.member), KINDS, whole, off)
    check(got, want, (form, shift))
    assert (got[r.counts == 0] == 0).all(), "a key without pairs must read 0, not the fill"
    assert (got[RG.EMPTY_WAVE[0]:RG.EMPTY_WAVE[1]] == 0).all() and (got[RG.EMPTY_CROSS[0]:RG.EMPTY_CROSS[1]] == 0).all()
    assert set(got.tolist()) == {0, 1, 2, 3}
    if form == "var":
        assert r.counts[r.long_key] >= 2 and np.diff(r.voffs)[r.long_key] > 4096


@pytest.mark.parametrize("form", FORMS)
def test_bit0_is_any_nonzero_word_of_the_ragged_probe(world, rag, form):  # noqa: F811
    """on the world's set (no unfiltered member), bit for bit against the ragged probe's words
    of the same inputs"""
    w, r = world, rag
    args = RG.inputs(w, r, form)
    words = RG.run_ragged(w.set, form, args, r.counts, r.member)
    got, _, _ = run_ragged(w.set, form, args, r.counts, r.member)
    key = np.repeat(np.arange(N), r.counts)
    hit = np.zeros(N, dtype=np.uint8)
    hit[np.unique(key[words != 0])] = 1
    check(got, hit, form)
    assert hit.any() and not hit.all()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("only", ["filter", "unfiltered"])
def test_long_lists_decided_by_the_last_id(world, rag, mixed, form, only):  # noqa: F811
    """lists of exactly 64, 128 and 300 ids whose only hit (only unfiltered id) is the last"""
    w, r = world, rag
    own_b = np.flatnonzero(r.words[form][3] != 0)  # keys that B0 (member 3) finds
    assert own_b.size > 300
    keys = [int(own_b[own_b.size // 4]), int(own_b[own_b.size // 2]), int(own_b[-1])]
    assert len({k // 64 for k in keys}) == 3
    counts = np.zeros(N, dtype=np.int64)
    counts[keys] = [64, 128, 300]
    rng = np.random.default_rng(5)
    member = rng.choice(np.array([2, NM, NM + 1], dtype=np.uint32), size=int(counts.sum()))  # None and past the end
    member[np.cumsum(counts[counts > 0]) - 1] = 3 if only == "filter" else 4
    got, whole, off = run_ragged(mixed, form, RG.inputs(w, r, form), counts, member, first=1000)
    want = np.zeros(N, dtype=np.uint8)
    want[keys] = E.EXISTS_FILTER_HIT if only == "filter" else E.EXISTS_UNFILTERED
    check(got, want, (form, only))
    check(E.exists_host(pair_words(r.words[form], counts, member, 1000), KINDS, whole, off), want, "mirror")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 63, 65])
def test_small_n(world, rag, mixed, form, n):  # noqa: F811
    w, r = world, rag
    counts = r.counts_small[:n]
    member = r.member_small[:int(counts.sum())]
    args = RG.inputs(w, r, form, n=n)
    got, whole, off = run_ragged(mixed, form, args, counts, member, first=7, shift=1)
    check(got, E.exists_host(pair_words(r.words[form][:, :n], counts, member, 7), KINDS, whole, off), (form, n))
    flat = w.member[3][:n].reshape(-1)
    got = run_fixed(mixed, form, args, w.member[3][:n], 3, n=n, shift=3)
    words = RG.want_pairs(r.words[form][:, :n], np.full(n, 3), flat)
    check(got, E.exists_host_fixed(words, KINDS, flat, 3), (form, n, "fixed"))


@pytest.mark.parametrize("form", FORMS)
def test_n_zero_writes_nothing(world, rag, mixed, form):  # noqa: F811
    w, r = world, rag
    args = RG.inputs(w, r, form)
    got, _, _ = run_ragged(mixed, form, args, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint32))
    assert got.size == 0
    out = Out(64)
    fn = {"hashes": mixed.exists_hashes, "keys": mixed.exists_keys, "var": mixed.exists_var_keys}[form]
    fn(*args, None, NM, 0, out.ptr)
    assert (out.read() == FILL).all()
    nulls = {"hashes": (None,), "keys": (None, 24), "var": (None, None)}[form]
    fn(*nulls, None, NM, 0, None)  # n == 0 is OK with NULL pointers


@pytest.mark.parametrize("form", FORMS)
def test_first_offset_1000(world, rag, mixed, form):  # noqa: F811
    w, r = world, rag
    got, whole, off = run_ragged(mixed, form, RG.inputs(w, r, form), r.counts, r.member, first=1000)
    check(got, E.exists_host(pair_words(r.words[form], r.counts, r.member, 1000), KINDS, whole, off), form)


# ---- the grid-stride loop: a stale per-wave LDS state shows here -----------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("blocks", [1, 2])
def test_grid_stride_loop(world, rag, mixed, blocks, form):  # noqa: F811
    """2,381 keys on 1 or 2 workgroups of 4 waves: 10 or 5 chunks per wave, the empty wave and the
    long lists among them"""
    w, r = world, rag
    args = RG.inputs(w, r, form)
    flat = w.member[3].reshape(-1)
    try:
        E.diag_fanout_max_blocks(blocks)
        got, whole, off = run_ragged(mixed, form, args, r.counts, r.member, first=1000, shift=2)
        got_fixed = run_fixed(mixed, form, args, w.member[3], 3)
    finally:
        E.diag_fanout_max_blocks(0)
    check(got, E.exists_host(pair_words(r.words[form], r.counts, r.member, 1000), KINDS, whole, off), (blocks, form))
    words = RG.want_pairs(r.words[form], np.full(N, 3), flat)
    check(got_fixed, E.exists_host_fixed(words, KINDS, flat, 3), (blocks, form, "fixed"))


# ---- routed -----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["keys", "var"])
def test_exists_routed(world, routed, mixed, form):  # noqa: F811
    """route, then ragged existence, against range_route_host + exists_host"""
    w, r = world, routed
    rg, off, member, total = r.host[form]
    words = RR.want_pairs(r.words[form], off, member)
    want = E.exists_host(words, KINDS, member, off)
    assert {0, 2, 3} <= set(want.tolist())  # the table has some forty lists: not every value need occur
    rmap = E.RangeMap(*r.table[form])
    fn = mixed.exists_routed if form == "keys" else mixed.exists_var_routed
    d_exists = fn(rmap, *RR.routed_inputs(w, r, form), N)
    torch.cuda.synchronize()
    assert d_exists.dtype == torch.uint8 and d_exists.shape == (N,)
    check(d_exists.cpu().numpy(), want, form)
    # the world's set through the same route: no unfiltered bit anywhere
    d_exists = (w.set.exists_routed if form == "keys" else w.set.exists_var_routed)(
        rmap, *RR.routed_inputs(w, r, form), N)
    torch.cuda.synchronize()
    check(d_exists.cpu().numpy(), E.exists_host(words, WORLD_KINDS, member, off), (form, "world"))
    rmap.close()


# ---- refusals ---------------------------------------------------------------------------------
def test_errors(world, rag, mixed):  # noqa: F811
    w, r = world, rag
    off = dev(RG.offsets_of(r.counts).view(np.int64))
    dm = dev(r.member)
    out = Out(N)
    d_h, (d_k, _), (d_b, d_o) = RG.inputs(w, r, "hashes")[0], RG.inputs(w, r, "keys"), RG.inputs(w, r, "var")

    def einval(fn):
        with pytest.raises(E.PlatformStatusError) as ei:
            fn()
        assert ei.value.code == E.STATUS_BAD_PARAM

    s = mixed
    einval(lambda: s.exists_keys(d_k, 0, None, NM, N, out.ptr))
    einval(lambda: s.exists_keys_ragged(d_k, 0, dm, off, N, out.ptr))
    einval(lambda: s.exists_keys(d_k, 24, None, NM - 1, N, out.ptr))  # all members: K must equal num_members
    einval(lambda: s.exists_hashes(d_h, dev(w.member[3].reshape(-1)), 0, N, out.ptr))
    einval(lambda: s.exists_hashes(d_h, None, NM, N, None))
    einval(lambda: s.exists_var_keys(d_b, None, None, NM, N, out.ptr))
    einval(lambda: s.exists_hashes_ragged(d_h, None, off, N, out.ptr))
    einval(lambda: s.exists_hashes_ragged(d_h, dm, None, N, out.ptr))
    einval(lambda: s.exists_var_keys_ragged(d_b, d_o, dm, off, N, None))
    einval(lambda: s.exists_keys_ragged(d_k, 24, dm, off, 1 << 56, out.ptr))
    assert (out.read() == FILL).all(), "a refused call wrote"
    # members hashed with different seeds: no keys forms, the hashes forms work
    cfg7 = E.routing_config_init(log_index_size=8, seed=7)
    S = E.FilterBatch(cfg7, [3000], [9])
    S.build_keys(dev(MG.K.random_keys(3000, seed=106)), 24)
    torch.cuda.synchronize()
    two = E.FilterSet([(w.A, 1), (S, 0), E.UNFILTERED])
    einval(lambda: two.exists_keys(d_k, 24, None, 3, N, out.ptr))
    einval(lambda: two.exists_var_keys_ragged(d_b, d_o, dm, off, N, out.ptr))
    two.exists_hashes(d_h, None, 3, N, out.ptr)
    assert (out.read() & 2 == 2).all()
    # ... and an unfiltered member in the filter's place leaves one seed
    two.update([1], [E.UNFILTERED])
    two.exists_keys(d_k, 24, None, 3, N, out.ptr)
    got = out.read()
    check(got, (r.words["keys"][1] != 0).astype(np.uint8) | np.uint8(2), "after the update")
    two.close()
    S.close()
