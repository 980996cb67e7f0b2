"""The probe geometry sweep's cases, probes and oracle-side restatements (plain helper module: no
fixtures, no pytest settings, no torch).

A lookup is decoded by one of several pieces of device code (rf_kernels.hip: probe_fast ->
line_decode_u, k_probe's rotated gather -> line_decode_w, probe_line -> line_decode, probe_walk /
probe_group -> probe_stream), and what they do depends on the filter's geometry: rem (remainder
bits), vs (value bits), rvs = rem + vs, the probe-line group G = 2^(lg_line - 1), log_index_size
and the number of entries of the probed bucket. CASES spans that space; tests/
test_probe_geometry_cases.py proves with the oracle alone that the table is what it claims and
that its probes reach every decode branch, tests/test_gpu_probe_geometry.py runs every lookup
entry point over it.

Everything here is derived from the oracle's image: `decode_image` reads buckets and entries out
of the pages (the layout written at src/routing_filter.c:622-633), `lookup` answers probes from
them, `classify` names the branch of line_decode_w a probe takes, `expected_probe_lines` cuts the
device-only probe lines and `line_lookup` answers probes from those lines.
"""
import math
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from splinterdb_amd import keys as K

DEFAULT_SIGMA = 3.5  # PlanKnobs::line_sigma
WAVE = 64
RUN_WAVES = 48            # "k of a few dozen": a run set is 64 k probes, a tail set 64 k + 37
TAIL = 37
CLASSES = ("overflow", "empty", "rvs0", "swar", "loop", "window_walk", "multi")


def value_size(value):
    return int(value).bit_length()


def log_buckets(n, lis):
    """log_num_buckets of a filter of n fingerprints (src/routing_filter.c:374-379)"""
    return max(int(n).bit_length() - 1, lis)


def line_log_group(lis, rvs, lam, sigma):
    """rf_batch_plan.h's line_log_group, restated: g + 1 of the largest group G = 2^g <= min(IS, 64)
    whose line holds mean + sigma sd + 2 entries, 0 = no lines"""
    if rvs > 32:
        return 0
    for g in range(min(lis, 6), -1, -1):
        G = float(1 << g)
        mean = lam * G
        cap = min(128.0 - G, 384.0 / rvs) if rvs else 128.0 - G
        if mean + sigma * math.sqrt(mean) + 2.0 <= cap:
            return g + 1
    return 0


def lg_line_of(fp, lis, n, value, sigma=DEFAULT_SIGMA):
    lnb = log_buckets(n, lis)
    return line_log_group(lis, fp - lnb + value_size(value), n / (1 << lnb), float(sigma))


def group_of(fp, lis, n, value, sigma=DEFAULT_SIGMA):
    """buckets per probe line, 0 = the filter has no lines"""
    lg = lg_line_of(fp, lis, n, value, sigma)
    return 1 << (lg - 1) if lg else 0


@dataclass(frozen=True)
class Case:
    """one filter: n fingerprints (all adds together) whose last add carries `value`"""
    name: str
    fp: int
    lis: int
    n: int
    value: int
    recipe: str        # "random" (hashes of 24-byte keys), "clustered", "chain"
    adds: tuple = ()   # chain: ((count, value), ...), n = the sum of the counts

    @property
    def lnb(self):
        return log_buckets(self.n, self.lis)

    @property
    def rem(self):
        return self.fp - self.lnb

    @property
    def vs(self):
        return value_size(self.value)

    @property
    def rvs(self):
        return self.rem + self.vs

    @property
    def G(self):
        return group_of(self.fp, self.lis, self.n, self.value)

    def group(self, sigma=None):
        return group_of(self.fp, self.lis, self.n, self.value, DEFAULT_SIGMA if sigma is None else sigma)

    @property
    def cfg_kw(self):
        return dict(fingerprint_size=self.fp, log_index_size=self.lis)


# fp, lis, n, value, rem, rvs, G: the columns after `value` are claims, proven against the
# derivation above, the oracle's filter and rf_batch_plan.h by test_probe_geometry_cases.py
TABLE = [
    (12, 4, 5_000, 0, 0, 0, 16),
    (12, 4, 5_000, 3, 0, 2, 16),
    (13, 4, 5_000, 63, 1, 7, 16),
    (13, 4, 5_000, 0, 1, 1, 16),
    (32, 3, 9, 0, 29, 29, 2),
    (32, 3, 200, 0, 25, 25, 2),
    (26, 8, 100, 63, 18, 24, 8),
    (12, 8, 100, 1, 4, 5, 64),
    (26, 8, 1, 0, 18, 18, 64),
    (20, 11, 3_000, 0, 9, 9, 16),
    (26, 6, 40_000, 7, 11, 14, 8),
    (16, 6, 33_000, 31, 1, 6, 32),
    (22, 9, 140_000, 0, 5, 5, 32),
    (32, 8, 66_000, 0, 16, 16, 8),
    (28, 7, 20_000, 15, 14, 18, 4),
]
RANDOM = [Case(f"fp{fp}_lis{lis}_n{n}_v{v}", fp, lis, n, v, "random") for fp, lis, n, v, *_ in TABLE]
# test_probe_line_overflow_falls_back_to_image's recipe (clusters of 150 fingerprints in 4
# neighbouring buckets overflow their lines) at rvs <= 6, rvs >= 18 and log_index_size 3
CLUSTERED = [
    Case("clustered_fp20_lis6_rvs6", 20, 6, 20_000, 0, "clustered"),
    Case("clustered_fp28_lis7_rvs18", 28, 7, 20_000, 15, "clustered"),
    Case("clustered_fp32_lis3_rvs22", 32, 3, 2_000, 0, "clustered"),
]
# three adds, half of each repeating hashes of the one before: found words of two and three bits.
# Values 0, 2, then 63 where fp_size + value_size <= 32 allows, else the widest that fits (15)
CHAINED = [
    Case("chain_fp13_lis4", 13, 4, 4_500, 63, "chain", ((1_500, 0), (1_500, 2), (1_500, 63))),
    Case("chain_fp28_lis7", 28, 7, 18_000, 15, "chain", ((6_000, 0), (6_000, 2), (6_000, 15))),
]
CASES = RANDOM + CLUSTERED + CHAINED
BY_NAME = {c.name: c for c in CASES}
G1_CASE = BY_NAME["fp32_lis3_n200_v0"]


def batches():
    """the cases of one (fp, lis) share a batch, in table order; a chain is a batch of its own
    (its filter is the last of three batches, each built on the one before)"""
    out = {}
    for c in CASES:
        key = (c.name,) if c.recipe == "chain" else (c.fp, c.lis)
        out.setdefault(key, []).append(c)
    return list(out.values())


def knob_sigmas():
    """the two RF_AMD_LINE_SIGMA settings of the sweep, from the restatement: (g1, none) -- at g1
    G1_CASE has one bucket per line (G == 1), at `none` no case has lines (lg_line == 0)"""
    c = G1_CASE
    g1 = next(float(s) for s in range(4, 64) if lg_line_of(c.fp, c.lis, c.n, c.value, s) == 1)
    none = next(float(1 << k) for k in range(2, 24)
                if all(lg_line_of(x.fp, x.lis, x.n, x.value, 1 << k) == 0 for x in CASES))
    assert group_of(c.fp, c.lis, c.n, c.value, g1) == 1
    assert all(x.group(none) == 0 for x in CASES)
    return g1, none


# ---- inputs ------------------------------------------------------------------------------------
def _rng(case, *tag):
    return np.random.default_rng([case.fp, case.lis, case.n, case.value, len(case.name), *tag])


def _rand32(rng, n):
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


def clustered_hashes(rng, fp, lis, n, clusters=8, per=150):
    """tests/test_gpu_parity.py's recipe: `clusters` clusters of `per` fingerprints in 4
    neighbouring buckets, the rest uniform"""
    lnb = log_buckets(n, lis)
    rem, sh = fp - lnb, 32 - fp
    h = _rand32(rng, n)
    k = 0
    for _ in range(clusters):
        b0 = int(rng.integers(0, (1 << lnb) - 4))
        for j in range(per):
            f = ((b0 + j % 4) << rem) | (j * 7919 % (1 << rem))
            h[k] = np.uint32((f << sh) | (j & ((1 << sh) - 1)))
            k += 1
    return h


def inputs(case, oracle):
    """the case's hashes: .h (every add, concatenated), .adds [(hashes, value)], and for the
    random recipe .keys, the 24-byte keys whose oracle.hash_fixed the hashes are"""
    rng = _rng(case, 1)
    inp = SimpleNamespace(keys=None)
    if case.recipe == "random":
        inp.keys = K.random_keys(case.n, seed=int(rng.integers(1 << 30)))
        inp.adds = [(oracle.hash_fixed(inp.keys.reshape(-1), 24), case.value)]
    elif case.recipe == "clustered":
        inp.adds = [(clustered_hashes(rng, case.fp, case.lis, case.n), case.value)]
    else:
        inp.adds, prev = [], None
        for count, value in case.adds:
            h = _rand32(rng, count)
            if prev is not None:
                h[: count // 2] = prev[rng.integers(0, prev.size, size=count // 2)]
            inp.adds.append((h, value))
            prev = h
    inp.h = np.concatenate([h for h, _ in inp.adds])
    assert inp.h.size == case.n
    return inp


def oracle_filter(case, inp, oracle):
    cfg = oracle.make_config(**case.cfg_kw)
    of = None
    for h, value in inp.adds:
        of = oracle.filter_add(cfg, h, value=value, old=of)
    return of


def probes(case, h, rng, length):
    """`length` probes of the filter built from hashes h, shuffled: its own hashes; own hashes with
    the lowest and with the top remainder bit flipped (other remainder, same bucket); own hashes
    moved to the bucket before and after; own hashes with only the bits below the fingerprint
    changed (they must still hit); uniform hashes; and the hashes 0 and 0xffffffff"""
    fp, rem, sh = case.fp, case.rem, 32 - case.fp
    m = length // 7
    own = lambda: h[rng.integers(0, h.size, size=m)].astype(np.uint64)  # noqa: E731
    parts = [own()]
    if rem:
        parts += [own() ^ np.uint64(1 << sh), own() ^ np.uint64(1 << (sh + rem - 1))]
    else:  # no remainder bits to flip: two more sets of neighbouring buckets
        parts += [(own() + np.uint64(2 << sh)) & np.uint64(0xffffffff),
                  (own() - np.uint64(2 << sh)) & np.uint64(0xffffffff)]
    step = np.uint64(1 << (sh + rem))
    parts += [(own() + step) & np.uint64(0xffffffff), (own() - step) & np.uint64(0xffffffff)]
    low = rng.integers(0, 1 << sh, size=m, dtype=np.uint64)
    parts.append((own() >> np.uint64(sh) << np.uint64(sh)) | low)
    parts.append(np.array([0, 0xffffffff], dtype=np.uint64))
    have = sum(p.size for p in parts)
    parts.append(rng.integers(0, 1 << 32, size=length - have, dtype=np.uint64))
    out = np.concatenate(parts).astype(np.uint32)
    assert out.size == length
    return out[rng.permutation(length)]


def probe_sets(case, inp):
    """the case's two probe sets: `run` (64 k) and `tail` (64 k + 37)"""
    return SimpleNamespace(run=probes(case, inp.h, _rng(case, 2), WAVE * RUN_WAVES),
                           tail=probes(case, inp.h, _rng(case, 3), WAVE * RUN_WAVES + TAIL))


def run_counts(cases_of_batch, aligned):
    """the runs tests' probes per filter of a batch. aligned: every filter its run set (every wave
    full and inside one run). Else tail sets, so later runs start off a wave boundary; the last of
    two or more filters gets a run shorter than a wave, the middle one of three or more none."""
    F = len(cases_of_batch)
    if aligned:
        return [WAVE * RUN_WAVES] * F
    counts = [WAVE * RUN_WAVES + TAIL] * F
    if F >= 2:
        counts[-1] = 20
    if F >= 3:
        counts[F // 2] = 0
    return counts


def full_wave_mask(counts):
    """which of sum(counts) probes, laid out run after run, sit in a wave of 64 that lies inside
    one run: the waves the fast path may take"""
    n = int(sum(counts))
    run = np.repeat(np.arange(len(counts)), counts)
    full = np.zeros(n, dtype=bool)
    for w in range(n // WAVE):
        if run[w * WAVE] == run[w * WAVE + WAVE - 1]:
            full[w * WAVE:(w + 1) * WAVE] = True
    return full


# ---- the image, restated -----------------------------------------------------------------------
def image_of(of):
    """an oracle filter's image as (pages, slots, num_indices)"""
    return SimpleNamespace(pages=of.pages(), slots=of.slots()[: of.num_indices], num_indices=of.num_indices)


def decode_image(image, case):
    """buckets and entries of an image: count[b] entries of bucket b (index-major), start[b] the
    number of entries before it, entries[] the remainder|value words in image order"""
    IS, rvs = 1 << case.lis, case.rvs
    bits = np.unpackbits(image.pages, bitorder="little")
    count = np.zeros(image.num_indices * IS, dtype=np.int64)
    ents = []
    sh = np.arange(rvs, dtype=np.uint64)
    for i in range(image.num_indices):
        h = int(image.slots[i])
        c = int(image.pages[h]) | (int(image.pages[h + 1]) << 8)
        e0 = (h + 2) * 8
        ones = np.flatnonzero(bits[e0: e0 + c + IS])
        assert ones.size == IS and (c + IS == 0 or ones[-1] == c + IS - 1)
        count[i * IS:(i + 1) * IS] = np.diff(ones, prepend=-1) - 1
        r0 = (h + 2 + (c + IS - 1) // 8 + 4) * 8
        if c and rvs:
            ents.append((bits[r0: r0 + c * rvs].reshape(c, rvs).astype(np.uint64) << sh).sum(axis=1, dtype=np.uint64))
        else:
            ents.append(np.zeros(c, dtype=np.uint64))
    start = np.concatenate([[0], np.cumsum(count)])
    return SimpleNamespace(count=count, start=start, entries=np.concatenate(ents + [np.zeros(1, np.uint64)]))


def split(case, hashes):
    """bucket (index-major) and remainder of each hash (src/routing_filter.c:1004-1012)"""
    f = np.asarray(hashes, dtype=np.uint32).astype(np.uint64) >> np.uint64(32 - case.fp)
    return (f >> np.uint64(case.rem)).astype(np.int64), f & np.uint64((1 << case.rem) - 1)


def _scan(case, ent_at, c, r):
    """found words of probes whose bucket holds c entries, entry k given by ent_at(k, mask)"""
    found = np.zeros(c.size, dtype=np.uint64)
    vs = np.uint64(case.vs)
    for k in range(int(c.max()) if c.size else 0):
        m = k < c
        rv = ent_at(k, m)
        val = rv & np.uint64((1 << case.vs) - 1)
        hit = m & ((rv >> vs) == r) & (val < 64)
        found |= np.where(hit, np.uint64(1) << np.where(hit, val, np.uint64(0)), np.uint64(0))
    return found


def lookup(dec, case, hashes):
    """routing_filter_lookup's found_values from a decoded image"""
    B, r = split(case, hashes)
    c, s = dec.count[B], dec.start[B]
    return _scan(case, lambda k, m: dec.entries[np.where(m, s + k, 0)], c, r)


def classify(image, case, hashes, G=None, dec=None):
    """{class: mask over the probes}: the branch of line_decode_w each probe takes in a filter cut
    into lines of G buckets (default: the case's own group). The first six are disjoint and cover
    every probe, in the order the code tests them: `overflow` (the line holds the marker: n + G >
    128 encoding bits or n rvs > 384 remainder bits), `empty` bucket, `rvs0`, `window_walk` (off +
    c rvs > 96: the bucket does not fit the 96-bit window), `swar` (c rvs <= 64 and rem > 0), `loop`
    (the rest). `multi` lies across them: more than one found bit."""
    G = case.G if G is None else G
    assert G > 0, "a filter without lines has no line decode"
    dec = dec or decode_image(image, case)
    rvs = case.rvs
    B, _ = split(case, hashes)
    g0 = B // G * G
    n = dec.start[g0 + G] - dec.start[g0]
    s, c = dec.start[B] - dec.start[g0], dec.count[B]
    ovf = (n + G > 128) | (n * rvs > 384)
    off = (s * rvs) & 31
    out, rest = {}, np.ones(B.size, dtype=bool)
    for name, m in (("overflow", ovf), ("empty", c == 0), ("rvs0", np.full(B.size, rvs == 0)),
                    ("window_walk", off + c * rvs > 96), ("swar", (c * rvs <= 64) & (case.rem > 0)),
                    ("loop", np.ones(B.size, dtype=bool))):
        out[name] = rest & m
        rest = rest & ~m
    found = lookup(dec, case, hashes)
    out["multi"] = np.array([bin(int(x)).count("1") > 1 for x in found], dtype=bool)
    return out


# ---- the probe lines, restated -----------------------------------------------------------------
def expected_probe_lines(pages, slots, num_indices, IS, G, rvs):
    """numpy restatement of the device-only probe-line format (rf_kernels.hip, "probe
    lines"), cut from a filter image: per group of G buckets, bits [0,128) the group's slice
    of the unary encoding (zero padded; all ones = overflow), bits [128,512) its packed
    remainders."""
    bits = np.unpackbits(pages, bitorder="little")
    L = IS // G
    out = np.zeros((num_indices * L, 64), dtype=np.uint8)
    for i in range(num_indices):
        h = int(slots[i])
        c = int(pages[h]) | (int(pages[h + 1]) << 8)
        e0 = (h + 2) * 8
        enc = bits[e0: e0 + c + IS]
        ones = np.flatnonzero(enc)
        r0 = (h + 2 + (c + IS - 1) // 8 + 4) * 8
        for g in range(L):
            a = 0 if g == 0 else int(ones[g * G - 1]) + 1
            end = int(ones[g * G + G - 1]) + 1
            ne = end - a
            n, E = ne - G, a - g * G
            line = np.zeros(512, dtype=np.uint8)
            if ne > 128 or n * rvs > 384:
                line[:128] = 1
            else:
                line[:ne] = enc[a:end]
                line[128:128 + n * rvs] = bits[r0 + E * rvs: r0 + (E + n) * rvs]
            out[i * L + g] = np.packbits(line, bitorder="little")
    return out


def line_lookup(lines, case, G, hashes):
    """(found words, overflowed) of probes answered from probe lines alone: the line of the
    probe's group, the bucket's bounds from the encoding bits, its entries from the remainder area"""
    B, r = split(case, hashes)
    rows = np.unpackbits(lines, axis=1, bitorder="little")[B // G].astype(np.int64)
    j, rvs, at = B % G, case.rvs, np.arange(B.size)
    ovf = rows[:, :128].all(axis=1)
    cs = np.cumsum(rows[:, :128], axis=1)
    p1 = np.where(j == 0, 0, np.argmax(cs == j[:, None], axis=1) + 1)  # after terminator j - 1
    c = np.where(ovf, 0, np.argmax(cs == (j + 1)[:, None], axis=1) - p1)
    first = 128 + (p1 - j) * rvs
    sh = np.arange(rvs, dtype=np.uint64)

    def ent_at(k, m):
        col = np.where(m, first + k * rvs, 0)[:, None] + np.arange(rvs)
        return (rows[at[:, None], col].astype(np.uint64) << sh).sum(axis=1, dtype=np.uint64)
    return _scan(case, ent_at, c, r), ovf


# ---- the reference, computed once per process ----------------------------------------------------
POOL_SHARE = 150  # probes of each case's tail set in the filter-set pool
_REF = None


def runs_layout(ref, cases_of_batch, aligned):
    """(counts, probes, oracle's words) of a runs call over a batch"""
    counts = run_counts(cases_of_batch, aligned)
    part = [(ref[c.name].sets.run if aligned else ref[c.name].sets.tail)[:k] for c, k in zip(cases_of_batch, counts)]
    want = [(ref[c.name].want_run if aligned else ref[c.name].want_tail)[:k] for c, k in zip(cases_of_batch, counts)]
    return counts, np.concatenate(part), np.concatenate(want)


def reference(oracle):
    """{case name: inputs, oracle filter, image, decoded image, probe sets and the oracle's words},
    plus "pool": the filter-set probes (POOL_SHARE of every case's tail set) and words[m], every
    member's oracle lookup of the whole pool under its own config. Read-only."""
    global _REF
    if _REF is None:
        ref = {}
        for c in CASES:
            r = SimpleNamespace(case=c, inp=inputs(c, oracle))
            r.of = oracle_filter(c, r.inp, oracle)
            r.img = image_of(r.of)
            r.dec = decode_image(r.img, c)
            r.sets = probe_sets(c, r.inp)
            r.want_run, r.want_tail = r.of.lookup_hashes(r.sets.run), r.of.lookup_hashes(r.sets.tail)
            for a in (r.inp.h, r.sets.run, r.sets.tail, r.want_run, r.want_tail):
                a.setflags(write=False)
            ref[c.name] = r
        pool = np.concatenate([ref[c.name].sets.tail[:POOL_SHARE] for c in CASES])
        pool = pool[np.random.default_rng(99).permutation(pool.size)]
        words = np.stack([ref[c.name].of.lookup_hashes(pool) for c in CASES])
        pool.setflags(write=False)
        words.setflags(write=False)
        ref["pool"] = SimpleNamespace(hashes=pool, words=words)
        _REF = ref
    return _REF


def coverage(ref):
    """{path: {class: probes}}: the decode classes that the probes handed to each group of entry
    points take. `tail sets`: probe_hashes, probe_pairs, the host and server paths; `runs, full
    waves` / `runs, other waves`: both layouts of the runs tests, split by full_wave_mask; `filter
    set`: every (pool probe, member) pair."""
    cov = {p: dict.fromkeys(CLASSES, 0) for p in ("tail sets", "runs, full waves", "runs, other waves", "filter set")}

    def add(path, case, hashes, mask=None):
        r = ref[case.name]
        for k, m in classify(r.img, case, hashes, dec=r.dec).items():
            cov[path][k] += int((m if mask is None else m & mask).sum())
    for c in CASES:
        add("tail sets", c, ref[c.name].sets.tail)
        add("filter set", c, ref["pool"].hashes)
    for cs in batches():
        for aligned in (True, False):
            counts, ph, _ = runs_layout(ref, cs, aligned)
            full, at = full_wave_mask(counts), np.concatenate([[0], np.cumsum(counts)])
            for f, c in enumerate(cs):
                sl = slice(at[f], at[f + 1])
                add("runs, full waves", c, ph[sl], full[sl])
                add("runs, other waves", c, ph[sl], ~full[sl])
    return cov
