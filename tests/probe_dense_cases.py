"""The dense probe-line format, restated (plain helper module beside probe_geometry_cases.py: no
fixtures, no pytest settings, no torch).

A filter whose plan carries LINE_DENSE (rf_plan.h) cuts each index into L = ceil(IS / G) groups of
G <= 64 buckets, the last one shorter, and keeps one 64-byte line per group: bits [0, U) the first
U bits of the group's unary code, bits [U, 512) the first floor((512 - U) / rvs) of its fields.
Nothing marks an over-full line: a probe walks the image only when its own bucket is cut off.
`dense_geometry` restates the planner's choice (rf_batch_plan.h: line_dense_group under
RF_AMD_LINES_DENSE=1), `expected_dense_lines` the bytes, `dense_line_lookup` answers probes from
those bytes alone and says which probes the device must walk instead.

CASES are the filters of tests/test_probe_dense_cases.py (CPU) and tests/test_gpu_probe_dense.py.
"""
import math
from types import SimpleNamespace

import numpy as np

import probe_geometry_cases as P

DENSE_SIGMA = 2.5     # PlanKnobs::dense_sigma
UNARY_MAX = 160       # LINE_UNARY_MAX
MIN_TABLE = 4 << 20   # LINE_DENSE_MIN_TABLE: one XCD's L2
WALK_BOUND = 0.01     # share of uniform probes that may take the image walk (the tests' coverage cap)
PROBES = 200_000      # probes per case and lookup path: half inserted, half never inserted


def unary_bits(G, rvs):
    """line_unary_bits: G terminators and the entries whose unary bits and fields fill 512 bits"""
    return G + min((512 - G) // (1 + rvs), UNARY_MAX - G)


def dense_group(lis, rvs, lam, L_now, sigma=DENSE_SIGMA):
    """line_dense_group: G of the smallest L < L_now that holds mean + sigma sd + 2 entries, or 0"""
    if rvs > 32:
        return 0
    IS = 1 << lis
    for L in range(1, min(L_now, 257)):
        G = -(-IS // L)
        if G > 64:
            continue
        mean = lam * G
        if mean + sigma * math.sqrt(mean) + 2.0 <= unary_bits(G, rvs) - G:
            return G
    return 0


def dense_geometry(case, forced=True):
    """(G, L, U) of the case's dense lines, or None where the planner keeps the current format"""
    g = case.G
    if not g:
        return None
    IS = 1 << case.lis
    L_now = IS // g
    if not forced and (1 << (case.lnb - case.lis)) * L_now * 64 <= MIN_TABLE:
        return None
    G = dense_group(case.lis, case.rvs, case.n / (1 << case.lnb), L_now)
    return (G, -(-IS // G), unary_bits(G, case.rvs)) if G else None


# fp, lis, n, value, recipe: rvs 4, 6 and 10 at lis 8, value bits (rvs 7 > rem 4), a group size
# that does not divide the index (lis 6: groups of 22, 22 and 20 buckets), an incremental build,
# and clusters that overflow their lines. The claimed (G, L, U) are proven by the CPU test.
TABLE = [
    ("rvs4", 20, 8, 70_000, 0, "random", (), (52, 5, 144)),
    ("rvs6", 22, 8, 70_000, 0, "random", (), (43, 6, 110)),
    ("rvs10", 26, 8, 70_000, 0, "random", (), (26, 10, 70)),
    ("value_rvs7", 20, 8, 70_000, 5, "random", (), (37, 7, 96)),
    ("lis6_rvs10", 26, 6, 70_000, 0, "random", (), (22, 3, 66)),
    ("chain_rvs6", 20, 8, 70_000, 2, "chain", ((35_000, 0), (35_000, 2)), (43, 6, 110)),
    ("clustered_rvs10", 26, 8, 70_000, 0, "clustered", (), (26, 10, 70)),
]
CASES = [P.Case("dense_" + name, fp, lis, n, v, recipe, adds) for name, fp, lis, n, v, recipe, adds, _ in TABLE]
CLAIMS = {c.name: t[-1] for c, t in zip(CASES, TABLE)}
UNIFORM = [c for c in CASES if c.recipe != "clustered"]
CLUSTERED = next(c for c in CASES if c.recipe == "clustered")


def expected_dense_lines(pages, slots, num_indices, IS, G, rvs):
    """the dense lines of a filter image, index after index"""
    bits = np.unpackbits(pages, bitorder="little")
    L, U = -(-IS // G), unary_bits(G, rvs)
    nf = (512 - U) // rvs if rvs else 0
    out = np.zeros((num_indices * L, 64), dtype=np.uint8)
    for i in range(num_indices):
        h = int(slots[i])
        c = int(pages[h]) | (int(pages[h + 1]) << 8)
        e0 = (h + 2) * 8
        enc = bits[e0: e0 + c + IS]
        ones = np.flatnonzero(enc)
        r0 = (h + 2 + (c + IS - 1) // 8 + 4) * 8
        for g in range(L):
            last = min(g * G + G, IS) - 1                 # the group's last bucket
            a = 0 if g == 0 else int(ones[g * G - 1]) + 1
            end = int(ones[last]) + 1
            n, E = end - a - (last + 1 - g * G), a - g * G  # entries, first entry
            line = np.zeros(512, dtype=np.uint8)
            keep = min(U, end - a)
            line[:keep] = enc[a:a + keep]
            k = min(n, nf)
            line[U:U + k * rvs] = bits[r0 + E * rvs: r0 + (E + k) * rvs]
            out[i * L + g] = np.packbits(line, bitorder="little")
    return out


def dense_line_lookup(lines, case, G, hashes):
    """(found words, walk) of probes answered from dense lines alone. walk: the probe's bucket is
    cut off -- its terminator is not among the U unary bits or its fields end past bit 512 -- or
    holds more fields than one 64-bit compare takes; the device walks the image for those, and
    their found words here are 0."""
    IS, rvs = 1 << case.lis, case.rvs
    L, U = -(-IS // G), unary_bits(G, rvs)
    B, r = P.split(case, hashes)
    bo = B % IS
    rows = np.unpackbits(lines, axis=1, bitorder="little")[(B // IS) * L + bo // G]
    j, at = bo % G, np.arange(B.size)
    cs = np.cumsum(rows[:, :U], axis=1, dtype=np.int16)
    have_prev = (j == 0) | (cs[:, -1] >= j)
    have_term = cs[:, -1] >= j + 1
    p1 = np.where(j == 0, 0, np.argmax(cs == j[:, None], axis=1) + 1)  # after terminator j - 1
    c = np.where(have_term, np.argmax(cs == (j + 1)[:, None], axis=1) - p1, 0)
    first = U + (p1 - j) * rvs
    walk = ~have_prev | ~have_term | (first + c * rvs > 512) | (c * rvs > 64) | (c >= 64)
    c = np.where(walk, 0, c)
    sh = np.arange(rvs, dtype=np.uint64)

    def ent_at(k, m):
        col = np.where(m, first + k * rvs, 0)[:, None] + np.arange(rvs)
        return (rows[at[:, None], col].astype(np.uint64) << sh).sum(axis=1, dtype=np.uint64)
    return P._scan(case, ent_at, c, r), walk


def cut_buckets(dec, case, G):
    """per bucket (index-major): True where the dense line of its group does not hold the bucket
    whole -- by the decoded image alone, not by the lines"""
    IS, rvs = 1 << case.lis, case.rvs
    U = unary_bits(G, rvs)
    b = np.arange(dec.count.size)
    bo = b % IS
    g0 = b - bo + bo // G * G                      # the group's first bucket
    before = dec.start[b] - dec.start[g0]          # entries of the group before the bucket
    end = before + dec.count + (b - g0) + 1        # unary bits up to and with its terminator
    return (end > U) | (U + (before + dec.count) * rvs > 512)


def probe_hashes(case, h, seed):
    """PROBES hashes, shuffled: half drawn from the filter's own, half uniform (2^32 / 2^fp of
    those repeat a fingerprint; the oracle decides what each finds)"""
    rng = np.random.default_rng([seed, case.fp, case.lis, case.n, case.value])
    own = h[rng.integers(0, h.size, size=PROBES // 2)]
    rnd = rng.integers(0, 1 << 32, size=PROBES - PROBES // 2, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([own, rnd])[rng.permutation(PROBES)]


_REF = None


def reference(oracle):
    """{case name: inputs, oracle filter, image, decoded image, dense geometry, restated lines,
    probes and the oracle's words}. Read-only, computed once per process."""
    global _REF
    if _REF is None:
        ref = {}
        for c in CASES:
            r = SimpleNamespace(case=c, inp=P.inputs(c, oracle))
            r.of = P.oracle_filter(c, r.inp, oracle)
            r.img = P.image_of(r.of)
            r.dec = P.decode_image(r.img, c)
            r.G, r.L, r.U = dense_geometry(c)
            r.lines = expected_dense_lines(r.img.pages, r.img.slots, r.img.num_indices, 1 << c.lis, r.G, c.rvs)
            r.probes = probe_hashes(c, r.inp.h, 1)
            r.want = r.of.lookup_hashes(r.probes)
            for a in (r.inp.h, r.lines, r.probes, r.want):
                a.setflags(write=False)
            ref[c.name] = r
        _REF = ref
    return _REF
