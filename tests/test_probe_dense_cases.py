"""The dense probe-line format on the CPU (tests/probe_dense_cases.py; the GPU side is
tests/test_gpu_probe_dense.py).

The restated lines, cut from the oracle's image, answer every probe they hold exactly as the
oracle's routing_filter_lookup does; the probes they do not hold are exactly those whose bucket
the decoded image says is cut off (or too large for one compare), under 1 % of the uniform cases'
probes; in a line that clusters overflow only the tail buckets are cut. The planner's choice of
format and geometry (rf_batch_plan.h) is checked by tests/c/dense_plan_check.cpp and compared
with the restatement."""
import os
import subprocess

import numpy as np
import pytest

import probe_dense_cases as D
import probe_geometry_cases as P
from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "splinterdb_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "dense_plan_check.cpp")
EXE = os.path.join(ROOT, "tests", "c", "dense_plan_check")


@pytest.fixture(scope="module")
def ref(oracle):
    return D.reference(oracle)


def test_planner_gate_and_geometry():
    """the host-only check: C2 goes dense, C3 / C4 / C5, the compaction chain and small filters do
    not; and the planner's forced geometry of every case is the restatement's"""
    deps = [SRC, os.path.join(CSRC, "rf_batch_plan.h"), os.path.join(CSRC, "rf_plan.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-I", CSRC, SRC, "-o", EXE], check=True)
    fresh = [c for c in D.CASES if c.recipe != "chain"]
    r = subprocess.run([EXE, *[f"{c.fp}:{c.lis}:{c.n}:{c.value}" for c in fresh]], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "dense_plan_check: OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    rows = [tuple(int(x) for x in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("dense ")]
    assert len(rows) == len(fresh)
    for c, (fp, lis, n, value, forced, default, lines) in zip(fresh, rows):
        G, L, U = D.dense_geometry(c)
        assert (G, L, U) == D.CLAIMS[c.name], c.name
        assert forced == 0x80 | (G - 1), (c.name, forced)
        assert lines == (1 << (c.lnb - c.lis)) * L
        assert default == P.lg_line_of(c.fp, c.lis, c.n, c.value) and D.dense_geometry(c, forced=False) is None


def test_geometry_claims():
    for c in D.CASES:
        G, L, U = D.dense_geometry(c)
        assert (G, L, U) == D.CLAIMS[c.name], c.name
        assert L < (1 << c.lis) // c.G, "fewer lines per index than the current format"
        assert U <= D.UNARY_MAX and (U - G) * (1 + c.rvs) <= 512 - G
    lis6 = next(c for c in D.CASES if c.lis == 6)
    assert (1 << lis6.lis) % D.CLAIMS[lis6.name][0], "a group size that does not divide the index"
    assert {c.rvs for c in D.CASES} >= {4, 6, 10} and any(c.vs and c.rvs > c.rem for c in D.CASES)


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.name)
def test_lines_answer_as_the_oracle(ref, case):
    r = ref[case.name]
    assert r.lines.shape == (r.img.num_indices * r.L, 64)
    got, walk = D.dense_line_lookup(r.lines, case, r.G, r.probes)
    assert (got[~walk] == r.want[~walk]).all()
    assert (got[~walk] == P.lookup(r.dec, case, r.probes)[~walk]).all()
    own = np.isin(r.probes, r.inp.h)
    assert own.sum() >= D.PROBES // 2 and (~own).sum() > D.PROBES // 3
    assert (r.want[own] != 0).all(), "an inserted key is always found"
    # the walks are the probes of cut-off buckets (by the decoded image alone) and of buckets
    # whose fields do not fit one 64-bit compare
    B, _ = P.split(case, r.probes)
    cut = D.cut_buckets(r.dec, case, r.G)
    assert (walk == (cut[B] | (r.dec.count[B] * case.rvs > 64))).all()
    print(f"{case.name}: G {r.G} L {r.L} U {r.U}, walk share {walk.mean():.5f}, cut buckets {int(cut.sum())}")
    if case.recipe != "clustered":
        assert walk.mean() < D.WALK_BOUND


def test_truncation_cuts_only_tail_buckets(ref):
    """a group that holds more entries than U - G keeps its head: the cut buckets of a line are a
    suffix of its group, the buckets before them answer from the line"""
    case = D.CLUSTERED
    r = ref[case.name]
    IS, G, U = 1 << case.lis, r.G, r.U
    cut = D.cut_buckets(r.dec, case, G)
    b = np.arange(cut.size)
    group = (b // IS) * r.L + (b % IS) // G
    ends = np.flatnonzero(np.diff(group, append=-1))          # each group's last bucket
    starts = np.concatenate([[0], ends[:-1] + 1])
    n = r.dec.start[ends + 1] - r.dec.start[starts]
    over = np.flatnonzero(n > U - G)
    assert over.size >= 4, "clusters overflow several lines"
    partial = 0
    for k in over:
        c = cut[starts[k]:ends[k] + 1]
        assert c.any() and (np.diff(c.astype(int)) >= 0).all(), "the cut buckets are the group's tail"
        partial += int(not c.all())
    assert partial >= 2, "lines with intact buckets before the cut"
    assert not cut[np.isin(group, over, invert=True)].any()
    # probes into cut and into intact buckets of the over-full lines
    B, _ = P.split(case, r.probes)
    inover = np.isin(group[B], over)
    got, walk = D.dense_line_lookup(r.lines, case, G, r.probes)
    assert (walk & inover).sum() > 100 and (~walk & inover).sum() > 100
    assert (got[~walk] == r.want[~walk]).all()
