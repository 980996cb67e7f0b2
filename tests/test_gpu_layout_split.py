"""K5 (page layout) over several workgroups per filter: filters with more indices than
RF_AMD_LAYOUT_SEG (default 4,096) are laid out by num_indices / seg workgroups that hand
the open page on to one another, and a build leaves its counters clean for the next one.
Every image (num_unique, num_pages, page bytes, slots) and 20,000 probes per case are
compared bit-for-bit with the oracle."""
import numpy as np
import pytest

from splinterdb_amd import engine as E

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# (lis, fp, n): the smallest shapes with 8,192 / 16,384 indices (the oracle accepts them all)
SHAPES = [(3, 22, (1 << 17) - 1),   # hundreds of blocks per page: the halo case
          (4, 22, 1 << 18),
          (4, 24, 3 << 16),
          (8, 26, 1 << 21),
          (8, 26, (1 << 22) + 12345)]  # C2's geometry at half its size
P = 20000


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _hashes(rng, n, dup=False):
    h = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    if dup and n > 8:
        h = h[rng.integers(0, max(1, n // 8), size=n)]
    return h


def _case(rng):  # the generator of tests/test_gpu_fuzz.py
    fp = int(rng.integers(18, 33))
    lis = int(rng.integers(3, 11)) if rng.random() < 0.85 else int(rng.integers(11, 13))
    cap = min(2 * 4096 * (1 << lis) - 1, (1 << fp) - 1)
    nf = int(rng.integers(1, 4))
    sizes = [max(1, int(np.exp(rng.uniform(0, np.log(cap / 2))))) for _ in range(nf)]
    vmax = min(63, (1 << (32 - fp)) - 1)
    vals = [int(rng.integers(0, vmax + 1)) for _ in range(nf)]
    dup = bool(rng.random() < 0.25)
    incr = bool(rng.random() < 0.4)
    return fp, lis, sizes, vals, dup, incr


def _oracle_add(oracle, ocfg, h, v, old=None):
    try:
        return oracle.filter_add(ocfg, h, value=v, old=old)
    except ValueError:
        return None


def _cfgs(oracle, fp, lis):
    return (E.routing_config_init(fingerprint_size=fp, log_index_size=lis),
            oracle.make_config(fingerprint_size=fp, log_index_size=lis))


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


@pytest.fixture(scope="module")
def shape_refs(oracle):
    """hashes and the oracle's filter per shape, computed once and never changed"""
    out = {}
    for lis, fp, n in SHAPES:
        rng = np.random.default_rng(lis * 100 + fp + n)
        h = _hashes(rng, n)
        out[(lis, fp, n)] = (h, oracle.filter_add(oracle.make_config(fingerprint_size=fp, log_index_size=lis),
                                                  h, value=0))
    return out


@pytest.mark.parametrize("lis,fp,n", SHAPES)
def test_split_shapes(oracle, shape_refs, lis, fp, n):
    h, of = shape_refs[(lis, fp, n)]
    assert of.num_indices > 4096
    cfg, _ = _cfgs(oracle, fp, lis)
    b = E.FilterBatch(cfg, [n], [0])
    b.build_hashes(dev(h))
    _same_image(b.image(0), of, (lis, fp, n))
    _check_probes(np.random.default_rng(n), b, 0, of, h, (lis, fp, n))


def test_rebuild_same_batch(oracle, shape_refs):
    """twice on one batch: the counters the first build leaves and the tagged hand-offs"""
    lis, fp, n = SHAPES[1]
    h, of = shape_refs[(lis, fp, n)]
    cfg, _ = _cfgs(oracle, fp, lis)
    b = E.FilterBatch(cfg, [n], [0])
    d = dev(h)
    b.build_hashes(d)
    img1 = b.image(0)
    b.build_hashes(d)
    img2 = b.image(0)
    _same_image(img1, of, "first")
    _same_image(img2, of, "second")
    _check_probes(np.random.default_rng(5), b, 0, of, h, "second")


def test_mixed_batch(oracle):
    """one split filter, one not, one tiny -- and a duplicate-heavy split one"""
    rng = np.random.default_rng(31)
    lis, fp = 4, 22
    cfg, ocfg = _cfgs(oracle, fp, lis)
    sizes = [1 << 18, 40_000, 1, 1 << 17]
    vals = [3, 0, 7, 1]
    hs = [_hashes(rng, sizes[0]), _hashes(rng, sizes[1]), _hashes(rng, sizes[2]), _hashes(rng, sizes[3], dup=True)]
    ofs = [oracle.filter_add(ocfg, h, value=v) for h, v in zip(hs, vals)]
    assert ofs[0].num_indices > 4096 >= ofs[1].num_indices and ofs[3].num_indices > 4096
    b = E.FilterBatch(cfg, sizes, vals)
    b.build_hashes(dev(np.concatenate(hs)))
    for f, of in enumerate(ofs):
        _same_image(b.image(f), of, f)
    for f in (0, 3):
        _check_probes(rng, b, f, ofs[f], hs[f], f)


def test_incremental_add_wider_value(oracle, shape_refs):
    """npo > 1 (the geometry changes): the num_unique put-back quirk runs inside segments"""
    lis, fp, n = SHAPES[3]
    h1, of1 = shape_refs[(lis, fp, n)]
    rng = np.random.default_rng(8)
    cfg, ocfg = _cfgs(oracle, fp, lis)
    b1 = E.FilterBatch(cfg, [n], [0])
    b1.build_hashes(dev(h1))
    h2 = _hashes(rng, n + n // 4)
    of2 = oracle.filter_add(ocfg, h2, value=5, old=of1)
    assert of2.num_indices > of1.num_indices
    b2 = E.FilterBatch(cfg, [h2.size], [5], old=[(b1, 0)])
    b2.build_hashes(dev(h2))
    _same_image(b2.image(0), of2, "incremental")
    _check_probes(rng, b2, 0, of2, np.concatenate([h1, h2]), "incremental")


@pytest.mark.parametrize("seed", range(40))
def test_fuzz_seg256(oracle, seed, monkeypatch):
    """the fuzz generator's first 40 cases with 256 indices per workgroup (chains of up to 64)"""
    monkeypatch.setenv("RF_AMD_LAYOUT_SEG", "256")
    rng = np.random.default_rng(1000 + seed)
    fp, lis, sizes, vals, dup, incr = _case(rng)
    cfg, ocfg = _cfgs(oracle, fp, lis)
    hs = [_hashes(rng, n, dup) for n in sizes]
    ofs = [_oracle_add(oracle, ocfg, h, v) for h, v in zip(hs, vals)]
    try:
        b = E.FilterBatch(cfg, sizes, vals)
    except E.PlatformStatusError:
        assert any(o is None for o in ofs), "engine rejected a batch the oracle accepts"
        return
    b.build_hashes(dev(np.concatenate(hs)))
    for f, of in enumerate(ofs):
        if of is None:
            with pytest.raises(E.PlatformStatusError):
                b.image(f)
            continue
        _same_image(b.image(f), of, (seed, f))
        _check_probes(rng, b, f, of, hs[f], (seed, f))
    good = [f for f, of in enumerate(ofs) if of is not None]
    if incr and good:
        f0 = good[0]
        n2 = max(1, sizes[f0] // 2)
        v2 = int(rng.integers(vals[f0], min(63, (1 << (32 - fp)) - 1) + 1))
        h2 = _hashes(rng, n2, dup)
        of2 = _oracle_add(oracle, ocfg, h2, v2, old=ofs[f0])
        try:
            b2 = E.FilterBatch(cfg, [n2], [v2], old=[(b, f0)])
            b2.build_hashes(dev(h2))
            img2 = b2.image(0)
        except E.PlatformStatusError:
            assert of2 is None, (seed, "engine rejected an incremental add the oracle accepts")
            return
        assert of2 is not None, (seed, "oracle rejected an incremental add the engine accepts")
        _same_image(img2, of2, (seed, "incremental"))


def test_seg256_segments_without_page_start(oracle, shape_refs, monkeypatch):
    """lis 3 with 256 indices per workgroup: the shape as it is, and with the lowest eighth of
    the hash space empty -- 256 empty blocks of 9 bytes are less than a page, so whole
    segments start no page and only pass the open page on"""
    monkeypatch.setenv("RF_AMD_LAYOUT_SEG", "256")
    lis, fp, n = SHAPES[0]
    h, of = shape_refs[(lis, fp, n)]
    cfg, ocfg = _cfgs(oracle, fp, lis)
    h2 = h | np.uint32(0x20000000)
    of2 = oracle.filter_add(ocfg, h2, value=0)
    page = of2.slots()[: of2.num_indices] // 4096
    assert of2.num_indices == 8192 and any(page[s - 1] == page[s + 255] for s in range(256, 8192, 256))
    for hh, oo, tag in ((h, of, "shape"), (h2, of2, "sparse")):
        b = E.FilterBatch(cfg, [n], [0])
        b.build_hashes(dev(hh))
        _same_image(b.image(0), oo, tag)
        _check_probes(np.random.default_rng(2), b, 0, oo, hh, tag)


def test_error_in_late_segment(oracle, shape_refs):
    """an index over 4,096 entries in the last segment: the filter fails, its sibling does not,
    and the call returns (the segments before it published their hand-offs)"""
    lis, fp, n = SHAPES[3]
    h_ok, of_ok = shape_refs[(lis, fp, n)]
    rng = np.random.default_rng(4)
    cfg, ocfg = _cfgs(oracle, fp, lis)
    nidx = of_ok.num_indices  # 8,192: an index is the hash's top 13 bits
    lg = nidx.bit_length() - 1
    late = nidx - 100  # in the second of two segments
    bad = _hashes(rng, n)
    # 5,000 distinct fingerprints in index `late`
    low = rng.permutation(1 << (fp - lg))[:5000].astype(np.uint32)
    bad[:5000] = (np.uint32(late) << np.uint32(32 - lg)) | (low << np.uint32(32 - fp))
    assert _oracle_add(oracle, ocfg, bad, 0) is None
    b = E.FilterBatch(cfg, [n, n], [0, 0])
    b.build_hashes(dev(np.concatenate([bad, h_ok])))
    with pytest.raises(E.PlatformStatusError):
        b.image(0)
    _same_image(b.image(1), of_ok, "sibling")
    _check_probes(rng, b, 1, of_ok, h_ok, "sibling")


def test_spill_then_clean(oracle):
    """a build whose fused partition spills (K4b runs), then a plain one on the same batch"""
    rng = np.random.default_rng(77)
    cfg, ocfg = _cfgs(oracle, 26, 8)
    n = 300_000
    hot = (np.uint32(0x9E370000) + np.arange(5, dtype=np.uint32) * np.uint32(97))
    h1 = np.concatenate([hot[rng.integers(0, 5, size=12_000)], _hashes(rng, n - 12_000)])
    rng.shuffle(h1)
    h2 = _hashes(rng, n)
    of1 = oracle.filter_add(ocfg, h1, value=0)
    of2 = oracle.filter_add(ocfg, h2, value=0)
    b = E.FilterBatch(cfg, [n], [0])
    b.build_hashes(dev(h1))
    _same_image(b.image(0), of1, "spilled")
    _check_probes(rng, b, 0, of1, h1, "spilled")
    b.build_hashes(dev(h2))
    _same_image(b.image(0), of2, "clean")
    _check_probes(rng, b, 0, of2, h2, "clean")


def test_seg0_equals_default(oracle, shape_refs, monkeypatch):
    """RF_AMD_LAYOUT_SEG=0 (one workgroup per filter) against the default"""
    lis, fp, n = SHAPES[4]
    h, of = shape_refs[(lis, fp, n)]
    cfg, _ = _cfgs(oracle, fp, lis)
    d = dev(h)
    b1 = E.FilterBatch(cfg, [n], [0])
    b1.build_hashes(d)
    img1 = b1.image(0)
    monkeypatch.setenv("RF_AMD_LAYOUT_SEG", "0")
    b0 = E.FilterBatch(cfg, [n], [0])
    b0.build_hashes(d)
    img0 = b0.image(0)
    assert (img0.num_unique, img0.num_pages) == (img1.num_unique, img1.num_pages)
    assert (img0.pages == img1.pages).all() and (img0.slots == img1.slots).all()
    _same_image(img1, of, "default")
