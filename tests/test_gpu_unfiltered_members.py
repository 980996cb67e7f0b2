"""Unfiltered members of a filter set (RF_AMD_MEMBER_UNFILTERED, E.UNFILTERED): a bundle without
a maplet that holds one branch, for which trunk_ondisk_bundle_merge_lookup sets found_values = 1
without a filter call (src/trunk.c:6020-6022). The world is test_gpu_multiget's (batches A-D,
N = 64 * 37 + 13 probes) with test_gpu_multiget_ragged's shuffled probes, variable-length keys and
ragged lists; the set is (A0, UNFILTERED, None, B0, UNFILTERED, D0). The expected word of every
pair is the oracle's routing_filter_lookup of that key where the member is a filter, 1 where it is
unfiltered, 0 for None and for ids past the end."""
import numpy as np
import pytest

import test_gpu_multiget as MG
import test_gpu_multiget_ragged as RG
from splinterdb_amd import engine as E
from test_gpu_multiget import world  # noqa: F401  (the fixture; a fresh instance for this module)
from test_gpu_multiget_ragged import rag  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, SENT, NM = MG.N, MG.SENT, RG.NM
FORMS = RG.FORMS
KINDS = [E.KIND_FILTER, E.KIND_UNFILTERED, E.KIND_NULL, E.KIND_FILTER, E.KIND_UNFILTERED, E.KIND_FILTER]
UNF = [g for g, k in enumerate(KINDS) if k == E.KIND_UNFILTERED]  # ids 1 and 4
dev = RG.dev


def members_of(w):
    return [(w.A, 0), E.UNFILTERED, None, (w.B, 0), E.UNFILTERED, (w.D, 0)]


def mixed_words(words):
    """the world's member words (rows A0, A1, None, B0, C0, D0) as the mixed set answers: the
    filters' rows as they are, 1 in the unfiltered rows, 0 in the None row"""
    out = np.array(words)
    out[UNF] = 1
    out[2] = 0
    return out


@pytest.fixture(scope="module")
def mixed(world):  # noqa: F811
    fs = E.FilterSet(members_of(world))
    assert fs.num_members == NM
    yield fs
    fs.close()


def run_fixed(fset, form, args, member, k):
    found = torch.full((N * k + SENT,), -7, dtype=torch.int64, device="cuda:0")
    fn = {"hashes": fset.probe_hashes, "keys": fset.probe_keys, "var": fset.probe_var_keys}[form]
    dm = None if member is None else dev(member.reshape(-1))
    fn(*args, dm, k, N, found)
    return RG.MV.read_found(found, N * k)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", [1, 3, None])
def test_fixed_forms(world, rag, mixed, form, k):  # noqa: F811
    w, r = world, rag
    kk = NM if k is None else k
    member = np.tile(np.arange(NM, dtype=np.uint32), N) if k is None else w.member[k].reshape(-1)
    got = run_fixed(mixed, form, RG.inputs(w, r, form), None if k is None else member, kk)
    want = RG.want_pairs(mixed_words(r.words[form]), np.full(N, kk), member)
    RG.check(got, want, (form, k))
    unf = np.isin(member, UNF)
    assert unf.any() and (got[unf] == 1).all()
    assert (got[member == 2] == 0).all() and (got[member >= NM] == 0).all()
    assert (got[np.isin(member, [0, 3, 5])] > 1).any(), "no filter member found a value other than 0"


@pytest.mark.parametrize("form", FORMS)
def test_ragged_lists(world, rag, mixed, form):  # noqa: F811
    w, r = world, rag
    got = RG.run_ragged(mixed, form, RG.inputs(w, r, form), r.counts, r.member, first=1000, junk=1)
    want = RG.want_pairs(mixed_words(r.words[form]), r.counts, r.member)
    RG.check(got, want, form)
    unf = np.isin(r.member, UNF)
    assert unf.sum() > 100 and (got[unf] == 1).all()
    assert (got[r.member == 2] == 0).all() and (got[r.member >= NM] == 0).all()


@pytest.mark.parametrize("form", ["keys", "var"])
def test_found_per_key_ragged(world, rag, mixed, form):  # noqa: F811
    """the records member << 8 | 0 of the unfiltered members sit at their list positions"""
    w, r = world, rag
    off = RG.offsets_of(r.counts)
    m = len(r.member)
    d_member, d_off = dev(r.member), dev(off.view(np.int64))
    d_found = torch.full((m,), -7, dtype=torch.int64, device="cuda:0")
    fn = mixed.probe_keys_ragged if form == "keys" else mixed.probe_var_keys_ragged
    fn(*RG.inputs(w, r, form), d_member, d_off, N, d_found)
    want_words = RG.want_pairs(mixed_words(r.words[form]), r.counts, r.member)
    key_off, cand, cand_key = E.found_per_key_host(want_words, r.member, off)
    d_key_off = torch.full((N + 1,), -7, dtype=torch.int64, device="cuda:0")
    d_cand = torch.full((len(cand) + SENT,), -7, dtype=torch.int64, device="cuda:0")
    d_cand_key = torch.full((len(cand) + SENT,), -7, dtype=torch.int64, device="cuda:0")
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    E.found_per_key_ragged(d_found, d_member, d_off, N, d_key_off, d_cand[:len(cand)], d_cand_key[:len(cand)], d_count)
    torch.cuda.synchronize()
    assert int(d_count.item()) == len(cand)
    got = d_cand.cpu().numpy()
    assert (got[len(cand):] == -7).all()
    got = got[:len(cand)].view(np.uint64)
    assert (got == cand).all()
    assert (d_key_off.cpu().numpy().view(np.uint64) == key_off).all()
    got_key = d_cand_key.cpu().numpy()[:len(cand)]
    assert (got_key == cand_key).all()
    # an unfiltered pair makes exactly one record, id << 8 | 0, and no filter of this set has id 1
    # or 4: those records, in order, are the unfiltered pairs, in order
    rec = np.isin(got >> np.uint64(8), UNF)
    pair = np.isin(r.member, UNF)
    assert rec.sum() == pair.sum() > 100
    assert (got[rec] == r.member[pair].astype(np.uint64) << np.uint64(8)).all()
    assert (got_key[rec] == np.repeat(np.arange(N), r.counts)[pair]).all()


def test_slot_follows_updates_in_stream_order(world, rag):  # noqa: F811
    """one stream, no host wait: slot 1 goes filter -> unfiltered -> filter -> NULL with a probe
    queued between each; every probe sees its own state, and update returns what the slot held"""
    w, r = world, rag
    s = torch.cuda.Stream()
    h = s.cuda_stream
    states = [(w.A, 1), E.UNFILTERED, (w.A, 1), None]
    rows = [r.words["keys"][1], np.ones(N, dtype=np.uint64), r.words["keys"][1], np.zeros(N, dtype=np.uint64)]
    with torch.cuda.stream(s):
        d_keys = dev(r.pk)
        found = [torch.full((N * NM + SENT,), -7, dtype=torch.int64, device="cuda:0") for _ in states]
    s.synchronize()
    fs = E.FilterSet([(w.A, 0), states[0], None, (w.B, 0), E.UNFILTERED, (w.D, 0)])
    returned = []
    for i, f in enumerate(found):
        if i:
            returned += fs.update([1], [states[i]], stream=h)
        fs.probe_keys(d_keys, 24, None, NM, N, f, stream=h)
    s.synchronize()
    assert returned[0] == (w.A, 1) and returned[1] is E.UNFILTERED and returned[2] == (w.A, 1)
    assert fs.update([1, 4], [None, None], stream=h) == [None, E.UNFILTERED]
    s.synchronize()
    base = mixed_words(r.words["keys"])
    for i, f in enumerate(found):
        want = base.copy()
        want[1] = rows[i]
        got = RG.MV.read_found(f, N * NM)
        RG.check(got, np.ascontiguousarray(want.T).reshape(-1), ("state", i))
    assert rows[0].any()
    fs.close()


@pytest.mark.parametrize("form", ["keys", "var"])
def test_set_without_filters(world, rag, form):  # noqa: F811
    """unfiltered and NULL members only: no seed, the keys forms are legal and answer as a set of
    NULL members does, except for the unfiltered words"""
    w, r = world, rag
    kinds = [E.UNFILTERED, None, E.UNFILTERED]
    fs, nulls = E.FilterSet(kinds), E.FilterSet([None, None, None])
    member = r.member % 5  # ids 3 and 4 are past the end
    args = RG.inputs(w, r, form)
    got = RG.run_ragged(fs, form, args, r.counts, member)
    ref = RG.run_ragged(nulls, form, args, r.counts, member)
    assert (ref == 0).all()
    assert (got == np.isin(member, [0, 2]).astype(np.uint64)).all()
    all_members = run_fixed(fs, form, args, None, 3).reshape(N, 3)
    assert (all_members == np.array([1, 0, 1], dtype=np.uint64)).all()
    assert fs.update([1], [E.UNFILTERED]) == [None]
    torch.cuda.synchronize()
    assert (run_fixed(fs, form, args, None, 3) == 1).all()
    fs.close()
    nulls.close()
