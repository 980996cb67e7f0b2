"""The cases of tests/reject_cases.py against the oracle, on the CPU: at the limit the oracle
accepts, one past it the oracle rejects, and the geometry is the one the limit was computed
from. tests/test_gpu_rejected.py runs the same cases on the engine; a case that drifts off its
limit fails here instead of quietly testing nothing there."""
import pytest

import reject_cases as R

# the limits the cases were found at, written down (not recomputed): name -> (num_indices,
# rvs, entries at the limit, its block's bytes, bits one past it)
FRESH_TABLE = {
    "fp20_count": (64, 6, 4096, 3624, R.ERR_INDEX_OVERFLOW),
    "fp22_count": (256, 6, 4096, 3624, R.ERR_INDEX_OVERFLOW),
    "fp26_page": (32, 13, 2317, 4096, R.ERR_BLOCK_TOO_BIG),
    "fp26_v5_page": (32, 16, 1908, 4095, R.ERR_BLOCK_TOO_BIG),
    "fp32_page": (32, 19, 1622, 4096, R.ERR_BLOCK_TOO_BIG),
    "fp22_lis4_page": (512, 9, 3268, 4096, R.ERR_BLOCK_TOO_BIG),
    "fp26_both": (32, 13, 2317, 4096, R.ERR_INDEX_OVERFLOW | R.ERR_BLOCK_TOO_BIG),
    "fp22_lis4_1024": (1024, 8, 3632, 4096, R.ERR_BLOCK_TOO_BIG),
    "fp22_lis7_count": (512, 6, 4096, 3608, R.ERR_INDEX_OVERFLOW),
}
INCR_TABLE = {
    "fp26_page": (32, 14, (1081, 1081), R.ERR_BLOCK_TOO_BIG),
    "fp20_page": (64, 7, (2028, 2028), R.ERR_BLOCK_TOO_BIG),
    "fp19_count": (64, 6, (2048, 2048), R.ERR_INDEX_OVERFLOW),
    "fp31_wide": (32, 19, (811, 811), R.ERR_BLOCK_TOO_BIG),
}
ALL_FRESH = R.FRESH + [R.SEG_1024, R.SEG_COUNT]


def _accepts(oracle, ocfg, h, value, old=None):
    try:
        return oracle.filter_add(ocfg, h, value=value, old=old)
    except ValueError:
        return None


def test_tables_cover_every_case():
    assert sorted(FRESH_TABLE) == sorted(c.name for c in ALL_FRESH)
    assert sorted(INCR_TABLE) == sorted(c.name for c in R.INCREMENTAL)


@pytest.mark.parametrize("case", ALL_FRESH, ids=lambda c: c.name)
def test_fresh_arithmetic(case):
    nidx, rvs, limit, nbytes, bits = FRESH_TABLE[case.name]
    assert (case.nidx, case.rvs, case.limit, case.bits) == (nidx, rvs, limit, bits)
    assert R.block_bytes(case.limit, case.lis, case.rvs) == nbytes <= R.PAGE_SIZE
    assert case.limit == R.FPS_PER_INDEX or R.block_bytes(case.limit + 1, case.lis, case.rvs) > R.PAGE_SIZE
    assert R.error_bits(case.limit, case.lis, case.rvs) == 0 and R.error_bits(case.past, case.lis, case.rvs) == bits


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("case", ALL_FRESH, ids=lambda c: c.name)
def test_fresh_limit_and_one_past(oracle, case, where):
    ocfg = oracle.make_config(fingerprint_size=case.fp, log_index_size=case.lis)
    index = R.positions(case.nidx)[where]
    of = _accepts(oracle, ocfg, case.hashes(case.limit, index), case.value)
    assert of is not None, "the oracle rejects the input at the limit"
    assert (of.num_indices, of.value_size) == (case.nidx, R.value_size(case.value))
    assert case.rvs == case.fp - (case.nidx.bit_length() - 1) - case.lis + of.value_size
    # the chosen index holds exactly `limit` entries: its block's header counts them
    hdr = int(of.slots()[index])
    pages = of.pages()
    assert int(pages[hdr]) | int(pages[hdr + 1]) << 8 == case.limit
    assert _accepts(oracle, ocfg, case.hashes(case.past, index), case.value) is None, \
        "the oracle accepts the input past the limit"
    # one past the limit is the first rejected count, whatever `past` is
    assert _accepts(oracle, ocfg, case.hashes(case.limit + 1, index), case.value) is None


@pytest.mark.parametrize("index", [100, 400])
@pytest.mark.parametrize("case", [R.SEG_512, R.SEG_COUNT], ids=lambda c: c.name)
def test_seg_512_indices(oracle, case, index):
    """the two-workgroup variants' indices (segment 0 and segment 1 of 256)"""
    ocfg = oracle.make_config(fingerprint_size=case.fp, log_index_size=case.lis)
    assert _accepts(oracle, ocfg, case.hashes(case.limit, index), case.value).num_indices == 512
    assert _accepts(oracle, ocfg, case.hashes(case.past, index), case.value) is None


def test_seg_1024_segment0(oracle):
    case = R.SEG_1024
    ocfg = oracle.make_config(fingerprint_size=case.fp, log_index_size=case.lis)
    assert _accepts(oracle, ocfg, case.hashes(case.limit, 100), case.value).num_indices == 1024
    assert _accepts(oracle, ocfg, case.hashes(case.past, 100), case.value) is None


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("case", R.INCREMENTAL, ids=lambda c: c.name)
def test_incremental_limit_and_one_past(oracle, case, where):
    nidx, rvs, limit, bits = INCR_TABLE[case.name]
    assert (case.nidx, case.rvs, case.limit, case.bits) == (nidx, rvs, limit, bits)
    assert case.past == (limit[0], limit[1] + 1)
    assert R.error_bits(sum(case.limit), case.lis, case.rvs) == 0
    assert R.error_bits(sum(case.past), case.lis, case.rvs) == bits
    ocfg = oracle.make_config(fingerprint_size=case.fp, log_index_size=case.lis)
    index = R.positions(case.nidx)[where]
    old = _accepts(oracle, ocfg, case.old_hashes(case.limit[0], index), case.v_old)
    assert old is not None, "the oracle rejects the old filter"
    of = _accepts(oracle, ocfg, case.new_hashes(case.limit[1], index), case.v_new, old=old)
    assert of is not None, "the oracle rejects the add at the limit"
    assert (of.num_indices, of.value_size) == (case.nidx, R.value_size(case.v_new))
    assert of.num_fingerprints == case.n_old + case.n_new
    hdr = int(of.slots()[index])
    pages = of.pages()
    assert int(pages[hdr]) | int(pages[hdr + 1]) << 8 == sum(case.limit)
    assert _accepts(oracle, ocfg, case.new_hashes(case.past[1], index), case.v_new, old=old) is None, \
        "the oracle accepts the add past the limit"
