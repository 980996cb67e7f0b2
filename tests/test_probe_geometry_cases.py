"""The probe geometry sweep's case table, proven on the CPU with the oracle alone
(tests/probe_geometry_cases.py; the GPU side is tests/test_gpu_probe_geometry.py): the oracle
accepts every case and reports the geometry the table claims; the group column is line_log_group
of rf_batch_plan.h, at the default margin and at both RF_AMD_LINE_SIGMA settings of the sweep;
the probes reach every decode class; and the restated image decode, the restated probe lines and a
lookup from those lines alone all give the oracle's routing_filter_lookup."""
import numpy as np
import pytest

import probe_geometry_cases as P
from test_batch_plan import run_plan_check

MIN_PROBES = 64


@pytest.fixture(scope="module")
def ref(oracle):
    return P.reference(oracle)


def test_table_columns_are_the_derivation():
    assert len(P.TABLE) == 15 and len(P.CLUSTERED) == 3 and len(P.CHAINED) == 2
    for (fp, lis, n, value, rem, rvs, G), c in zip(P.TABLE, P.RANDOM):
        assert (c.fp, c.lis, c.n, c.value) == (fp, lis, n, value)
        assert (c.rem, c.rvs, c.G) == (rem, rvs, G), c.name
    assert {c.G for c in P.CASES} >= {2, 4, 8, 16, 32, 64}
    assert any(c.rem == 0 and c.rvs == 0 for c in P.CASES) and any(c.rem == 0 and c.rvs for c in P.CASES)
    assert {1, 29} <= {c.rvs for c in P.CASES}
    assert sum(c.value == 63 for c in P.CASES) >= 3
    rv = sorted(c.rvs for c in P.CLUSTERED)
    assert rv[0] <= 6 and rv[-1] >= 18 and any(c.lis == 3 for c in P.CLUSTERED)
    for c in P.CHAINED:
        assert [v for _, v in c.adds][:2] == [0, 2] and sum(k for k, _ in c.adds) == c.n
        last = c.adds[-1][1]
        assert last == (63 if c.fp + 6 <= 32 else (1 << (32 - c.fp)) - 1) and last == c.value


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c.name)
def test_oracle_accepts_and_reports_the_geometry(ref, case):
    of = ref[case.name].of
    assert of.num_fingerprints == case.n
    lnb = case.lis + int(of.num_indices).bit_length() - 1
    assert of.num_indices == 1 << (lnb - case.lis)
    rem, vs = case.fp - lnb, of.value_size
    assert (lnb, rem, vs, rem + vs) == (case.lnb, case.rem, case.vs, case.rvs)
    assert 0 <= rem and case.fp + vs <= 32


def test_group_column_is_the_planners(ref):
    """plan_check's `line` rows (rf_batch_plan.h itself) against the table and the restatement, at
    the default margin and at the two knob settings, which the helper derives"""
    g1, none = P.knob_sigmas()
    sigmas = [P.DEFAULT_SIGMA, g1, none]
    args = [f"{c.fp}:{c.lis}:{c.n}:{c.value}:{s!r}" for s in sigmas for c in P.CASES]
    rows = [ln.split()[1:] for ln in run_plan_check(args).splitlines() if ln.startswith("line ")]
    assert len(rows) == len(args)
    it = iter(rows)
    for s in sigmas:
        for c in P.CASES:
            fp, lis, n, value, sigma, lg, lnb, rem, vs, rvs = next(it)
            assert (int(fp), int(lis), int(n), int(value), float(sigma)) == (c.fp, c.lis, c.n, c.value, s)
            assert (int(lnb), int(rem), int(vs), int(rvs)) == (c.lnb, c.rem, c.vs, c.rvs), c.name
            assert int(lg) == P.lg_line_of(c.fp, c.lis, c.n, c.value, s), (c.name, s)
            G = 1 << (int(lg) - 1) if int(lg) else 0
            assert G == c.group(s), (c.name, s)
            if s == P.DEFAULT_SIGMA:
                assert G == c.G and G > 0
            if s == none:
                assert int(lg) == 0
    table_g = {(fp, lis, n, v): G for fp, lis, n, v, _, _, G in P.TABLE}
    for row in rows[: len(P.RANDOM)]:
        key = tuple(int(x) for x in row[:4])
        assert 1 << (int(row[5]) - 1) == table_g[key], key
    assert P.G1_CASE.group(g1) == 1 and g1 not in (P.DEFAULT_SIGMA, none)
    assert any(c.group(g1) > 1 for c in P.CASES)


def test_probe_sets_have_the_asked_shape(ref):
    for c in P.CASES:
        s = ref[c.name].sets
        assert s.run.size % 64 == 0 and s.run.size // 64 >= 24 and s.tail.size == s.run.size + 37
        for ph, want in ((s.run, ref[c.name].want_run), (s.tail, ref[c.name].want_tail)):
            assert (ph == 0).any() and (ph == 0xffffffff).any()
            assert int((want != 0).sum()) >= ph.size // 7 * 2  # own hashes, and with other sub-fp bits
            if c.recipe != "chain":
                assert int((want >> np.uint64(c.value) & np.uint64(1)).sum()) >= ph.size // 7 * 2
            assert (want == 0).any()
    for cs in P.batches():
        counts = P.run_counts(cs, False)
        assert all(k % 64 == 0 for k in P.run_counts(cs, True)) and counts[0] % 64
        if len(cs) >= 2:
            assert 0 < counts[-1] < 64
        if len(cs) >= 3:
            assert 0 in counts
    assert any(len(cs) >= 3 for cs in P.batches())


def test_every_decode_class_is_reached(ref, capsys):
    cov = P.coverage(ref)
    with capsys.disabled():
        print("\nprobes per decode class:")
        for path, row in cov.items():
            print(f"  {path:18s} " + "  ".join(f"{k} {v}" for k, v in row.items()))
    total = {k: sum(row[k] for row in cov.values()) for k in P.CLASSES}
    for k in P.CLASSES:
        assert total[k] >= MIN_PROBES, (k, total[k])
        assert cov["tail sets"][k] >= MIN_PROBES and cov["filter set"][k] >= MIN_PROBES, k
    for k in ("overflow", "window_walk", "loop", "rvs0", "multi"):
        assert cov["runs, full waves"][k] >= MIN_PROBES, (k, cov["runs, full waves"][k])
    assert cov["runs, other waves"]["swar"] >= MIN_PROBES


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c.name)
def test_restatements_give_the_oracles_lookup(ref, case):
    """the image decode the classifier rests on, and a lookup from expected_probe_lines alone,
    against oracle.lookup_hashes: the restated lines are a checked reference"""
    r = ref[case.name]
    for ph, want in ((r.sets.run, r.want_run), (r.sets.tail, r.want_tail)):
        assert (P.lookup(r.dec, case, ph) == want).all()
    g1, _ = P.knob_sigmas()
    for G in sorted({case.G, case.group(g1)}):
        lines = P.expected_probe_lines(r.img.pages, r.img.slots, r.img.num_indices, 1 << case.lis, G, case.rvs)
        assert lines.shape == ((r.img.num_indices << case.lis) // G, 64)
        cl = P.classify(r.img, case, r.sets.tail, G=G, dec=r.dec)
        first6 = np.stack([cl[k] for k in P.CLASSES[:6]])
        assert (first6.sum(axis=0) == 1).all()
        found, ovf = P.line_lookup(lines, case, G, r.sets.tail)
        assert (ovf == cl["overflow"]).all()
        keep = ~(cl["overflow"] | cl["window_walk"])
        assert (found[keep] == r.want_tail[keep]).all()
        assert (found[~ovf] == r.want_tail[~ovf]).all()  # the line holds a window_walk bucket too
        if cl["overflow"].any():
            assert (lines[:, :16] == 0xFF).all(axis=1).any()
