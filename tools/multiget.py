#!/usr/bin/env python3
"""Multi-get, two ways, in one process: the fan-out probe of a resident filter set
(FilterSet.probe_keys: each key read and hashed once, K members per key) against what a caller
could do before it existed -- hash the keys once (E.hash_keys), replicate every hash K times
(torch.repeat_interleave) and probe the replicas with per-probe filter ids (probe_hashes).

Shape: one batch of 64 filters x 2^20 keys (C3's per-filter size; one batch, so that the second
way is possible at all), n = 16M 24-byte keys, K = 4 random members per key; key i is a key of
filter i % 64. Each round runs both ways on the same inputs, alternating, after warm-up rounds;
times are HIP events on the launch stream. Reported: each way's minimum to maximum range and
whether the ranges touch, the compaction's time (rf_amd_found_compact at cap = count), the
bytes of the dense n K words against those of the candidate list, and the time of each one's
copy into pinned host memory. Both ways' words are compared before anything is reported.

--var: the same two ways on variable-length keys (keys.var_keys: 8-100 B, C5's distribution,
generated on the host): FilterSet.probe_var_keys against hash_var_keys + repeat_interleave +
probe_hashes. Key i is a member of filter i % 64: each filter is built (build_hashes) from the
hashes of its n / 64 probe keys and random hashes up to its 2^20. Default output:
profiles/multiget_var.json.

--ragged: per-key member lists of different lengths on the same filters and keys (with --var:
variable-length keys). Key i has min(16, 1 + Geometric(1/3)) random members (seeded, mean about
4). Timed with the same method: (a) the ragged probe (FilterSet.probe_keys_ragged) and the
compaction of its pairs, against (b) the same lists padded to K = 16 with the id num_members
through the fixed form (probe_keys) and the compaction of its n * 16 words; and (c) uniform
K = 4 lists through both kernels. The non-padded words of (a) and (b), and both outputs of (c),
are compared before anything is timed. Default output: profiles/multiget_ragged.json
(profiles/multiget_var_ragged.json).

--routed: the multi-get from raw device keys, on the --ragged shape (with --var:
variable-length keys). A range map (E.RangeMap) of R = 4,096 ranges, cut by boundaries drawn from
the key population (one per 8-byte prefix), each range with a list of min(16, 1 + Geometric(1/3))
random members. Timed with the same method: (a) the route call alone
(rf_amd_range_map_route_keys: keys to ranges and the CSR of their lists), (b) route + ragged probe
+ compaction, (c) ragged probe + compaction from a precomputed CSR (what a caller had before, re-
measured in the same run), and (d) the host alternative, by the wall clock: keys D2H into pinned
memory, routing by np.searchsorted over big-endian 8-byte prefixes (valid because the boundaries'
prefixes are unique and every key has 8 bytes), the CSR by numpy, and its H2D. (a)'s ranges are
compared with the host mirror (E.range_route_host) on a sample of 2^16 keys and, with its offsets,
ids and total, with (d)'s whole result before anything is timed. Default output:
profiles/multiget_routed.json (profiles/multiget_var_routed.json).

--update: what a compaction does to a resident set of --filters members (any number; each filter
of --keys hashes), two ways: (a) rf_amd_filter_set_update of u = 1, 16 and 256 members (clamped to
the set's size) and (b) rf_amd_filter_set_destroy plus rf_amd_filter_set_create of the whole set.
After each way one small probe runs (n = 4,096, K = 4); both ways' words after the same change are
compared before anything is timed. Reported per way and u, minimum to maximum over the
alternating rounds: the host wall time of the call or calls (the C calls alone: both ways'
argument arrays are built beforehand), and the HIP-event time from before the call to after the
probe (the stream is idle at the first event, so this interval contains the host time). Default output: profiles/multiget_update.json (measured with
--filters 1024 --keys 4096).

--segments: what the most frequent trunk event does to a resident range map, two ways. The table is
trunk-shaped: R = 4,096 leaves, fan-out 16 per level, so a leaf's path has 4 segments (the root's
pivot, two inner pivots, the leaf's own), each with 1 to 8 ids and room for 8. One root segment
changes. (a) rf_amd_range_map_update_segments of that segment on a map made from segments
(E.RangeMap.from_segments): one scatter launch and the three of the flatten. (b) what a flat map
needs: rf_amd_range_map_create of the rebuilt flat table and rf_amd_range_map_destroy_on of the old
map. Reported per way, minimum to maximum over the alternating rounds: the host wall time of the C
calls (arrays built beforehand) and the HIP-event time around them on the idle stream; (b) also
through E.RangeMap(...) + close_on. A route call of 2^20 24-byte keys is timed on the segmented map
before and after every update and on the flat map. Both ways' route output after the same change
is compared over all keys before anything is timed. Default output: profiles/range_segments.json.

--split: what a leaf split does to a resident range map, two ways, on the table of --segments with
16 spare segments: one leaf splits into 2 and into 8. (split) on a map created with room
(E.RangeMap.from_segments(..., room=...)): rf_amd_range_map_update_segments of the new leaves'
spare segments, then rf_amd_range_map_split -- one splice launch and the three of the flatten.
(rebuild) what the parent commit must do: rf_amd_range_map_create_segments of the new table and
rf_amd_range_map_destroy_on of the old map. Reported per way, median, minimum and maximum over the
rounds, a fresh pair of maps each: the host wall time until the calls return (arrays built
beforehand) and the wall time until the stream has drained. A route call of 2^20 24-byte keys is
timed on both maps after the event: the same table, with and without room. Both ways' route
output is compared over all keys before anything is timed. Conditions: the split's median to a
drained stream below the rebuild's by more than the rebuild's round-to-round spread; the roomy
map's route median not above the roomless map's by more than that one's spread. Default output:
profiles/range_split.json.

--per-key: the step behind the probe, two ways, on the --ragged lists and on the CSR that a route
call writes for a map of R = 4,096 ranges with such lists (with --var: variable-length keys). What a
consumer of the candidates needs is each record's member id and key. (parent_path) what a caller had:
rf_amd_found_compact, torch.searchsorted of the records' pairs over the n + 1 offsets, the gather
d_member[pair]. (per_key) one rf_amd_found_per_key_ragged, which writes the CSR of the records over
the keys as well. Both ways' records, keys, offsets and totals are compared before anything is
timed; then alternating rounds with the same method. Reported per workload: each way's rounds,
minimum, maximum and median, the parent path's round-to-round spread, and whether the new call's
median is within that spread of the parent path's. Default output: profiles/multiget_per_key.json
(profiles/multiget_var_per_key.json).

--by-branch: the per-key records grouped by branch, two ways, on the CSR of the --per-key route call
and on lists that hold every key's own filter. (parent_path) torch.sort(stable=True) of the sort
keys, the gather of the records' keys and torch.unique_consecutive(return_counts=True), with their
synchronisation and allocations. (by_branch) one rf_amd_found_by_branch. Same rounds and condition
as --per-key; the results are compared before timing. Default output: profiles/multiget_by_branch.json.

--advance: one step of the multi-get with early exit, two ways, on the two --by-branch workloads
and on lists of eight that name each key's own filter four times. (parent_path) torch masks, cumsum,
repeat_interleave and the gather, with their synchronisation and allocations. (advance) one
rf_amd_found_advance at width 1. Same rounds and condition as --per-key; the results are compared
before timing. Then whole multi-gets at width 1, 2 and 4, a key being done at its own filter's
record: the records handed out against all records. Default output: profiles/multiget_advance.json.

--exists: the existence multi-get (SPLINTERDB_LOOKUP_MIGHT_EXIST), on the same two workloads (with
--var: variable-length keys). (exists) one rf_amd_filter_set_exists_*_ragged: one byte per key.
(ragged_probe) the parent path's cheapest possible start: the ragged probe alone on the same
inputs, which writes 8 bytes per pair that a second pass would still have to reduce -- a lower bound
of any way to get the answer from the calls there were. Every byte is compared with "some word of
the key's pairs is not zero" before anything is timed; then alternating rounds with the same
method and the same condition as --per-key. Default output: profiles/multiget_exists.json
(profiles/multiget_var_exists.json).

    timeout -k 10 600 python tools/multiget.py [--var] [--ragged | --routed | --per-key | --by-branch | --advance | --exists] [--filters 64] [--keys 1048576]
                                               [--n 16777216] [--k 4] [--rounds 7] [--warmup 2]
                                               [--out profiles/multiget.json]
    timeout -k 10 300 python tools/multiget.py --update --filters 1024 --keys 4096
    timeout -k 10 300 python tools/multiget.py --segments
    timeout -k 10 300 python tools/multiget.py --split
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from splinterdb_amd import engine as E  # noqa: E402
from splinterdb_amd import keys as K  # noqa: E402


KPAD = 16  # --ragged: the longest list, and the K that the padded form needs


def ragged(args, fset, eng, stream, kin, own, mean_len, timed, rng):
    """--ragged: (a) ragged probe + compaction against (b) the lists padded to KPAD through the
    fixed form + compaction, and (c) uniform K = 4 through both kernels; kin: the keys'
    arguments, own[i]: the filter that holds key i"""
    import numpy as np
    F, n = args.filters, args.n
    dev, st = own.device, stream.cuda_stream
    probe_r = fset.probe_var_keys_ragged if args.var else fset.probe_keys_ragged
    probe_f = fset.probe_var_keys if args.var else fset.probe_keys
    counts = np.minimum(KPAD, 1 + np.random.default_rng(7).geometric(1.0 / 3.0, size=n)).astype(np.int64)
    off_h = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=off_h[1:])
    m = int(off_h[-1])
    with torch.cuda.stream(stream):
        g = torch.Generator(device=dev)
        g.manual_seed(8)
        off = torch.from_numpy(off_h).to(dev)
        d_counts = torch.from_numpy(counts).to(dev)
        key = torch.repeat_interleave(torch.arange(n, device=dev), d_counts)       # the pair's key
        at = key * KPAD + (torch.arange(m, device=dev) - off[key])                  # its place in the padded form
        member_r = torch.randint(0, F, (m,), device=dev, generator=g).to(torch.int32)
        member_p = torch.full((n * KPAD,), F, dtype=torch.int32, device=dev)       # id num_members: finds nothing
        member_p[at] = member_r
        member_u = torch.randint(0, F, (n * 4,), device=dev, generator=g).to(torch.int32)
        off_u = torch.arange(n + 1, device=dev, dtype=torch.int64) * 4
        found_r = torch.zeros(m, dtype=torch.int64, device=dev)
        found_p = torch.zeros(n * KPAD, dtype=torch.int64, device=dev)
        found_ur = torch.zeros(n * 4, dtype=torch.int64, device=dev)
        found_uf = torch.zeros(n * 4, dtype=torch.int64, device=dev)
        d_count = torch.zeros(1, dtype=torch.int64, device=dev)
        # every output once, compared before anything is timed
        probe_r(*kin, member_r, off, n, found_r, stream=st)
        probe_f(*kin, member_p, KPAD, n, found_p, stream=st)
        probe_r(*kin, member_u, off_u, n, found_ur, stream=st)
        probe_f(*kin, member_u, 4, n, found_uf, stream=st)
    stream.synchronize()
    with torch.cuda.stream(stream):
        assert torch.equal(found_r, found_p[at]), "ragged and padded words disagree"
        assert int(torch.count_nonzero(found_p)) == int(torch.count_nonzero(found_r)), "a padded slot found something"
        assert torch.equal(found_ur, found_uf), "uniform K = 4: the two kernels disagree"
        mine = member_r.to(torch.int64) == own[key]
        hits = int(((found_r >> member_r.to(torch.int64)) & 1)[mine].sum())
        assert hits == int(mine.sum()) and hits > 0, "false negative"
        del mine, key, at
        E.found_compact(found_r, m, None, d_count, stream=st, engine=eng)
    stream.synchronize()
    count = int(d_count.item())
    with torch.cuda.stream(stream):
        E.found_compact(found_p, n * KPAD, None, d_count, stream=st, engine=eng)
    stream.synchronize()
    assert int(d_count.item()) == count, "the padded form's candidates differ in number"
    with torch.cuda.stream(stream):
        d_cand = torch.zeros(max(count, 1), dtype=torch.int64, device=dev)
    stream.synchronize()

    ways = {
        "ragged_probe": lambda: probe_r(*kin, member_r, off, n, found_r, stream=st),
        "padded_probe": lambda: probe_f(*kin, member_p, KPAD, n, found_p, stream=st),
        "ragged_compact": lambda: E.found_compact(found_r, m, d_cand, d_count, stream=st, engine=eng),
        "padded_compact": lambda: E.found_compact(found_p, n * KPAD, d_cand, d_count, stream=st, engine=eng),
        "uniform4_ragged_probe": lambda: probe_r(*kin, member_u, off_u, n, found_ur, stream=st),
        "uniform4_fixed_probe": lambda: probe_f(*kin, member_u, 4, n, found_uf, stream=st),
    }
    t = {w: [] for w in ways}
    for r in range(args.warmup + args.rounds):
        for w, fn in ways.items():  # alternating: one of each per round
            ms = timed(fn)
            if r >= args.warmup:
                t[w].append(ms)
    assert int(d_count.item()) == count
    t["ragged_total"] = [a + b for a, b in zip(t["ragged_probe"], t["ragged_compact"])]
    t["padded_total"] = [a + b for a, b in zip(t["padded_probe"], t["padded_compact"])]

    def versus(a, b):
        return {"ranges_touch": not (max(a) < min(b) or max(b) < min(a)),
                "ragged_faster_beyond_ranges": bool(max(a) < min(b)),
                "ragged_slower_beyond_ranges": bool(max(b) < min(a))}

    mean_list = m / n
    key_bytes = round(mean_len + 8, 3) if args.var else 24
    out = {
        "what": ("ragged multi-get of n %s, key i against min(16, 1 + Geometric(1/3)) random members of one "
                 "batch of F filters: (a) FilterSet.probe_%skeys_ragged + found_compact of the pairs against (b) the "
                 "same lists padded to K = 16 with id num_members through probe_%skeys + found_compact of the n * 16 "
                 "words, and (c) uniform K = 4 lists through both kernels; alternating rounds in one process, HIP "
                 "events on the launch stream" % (("variable-length keys (keys.var_keys, 8-100 B)", "var_", "var_")
                                                  if args.var else ("24-byte keys", "", ""))),
        "config": {"filters": F, "keys_per_filter": args.keys, "n": n, "pairs": m, "mean_list": round(mean_list, 4),
                   "max_list": int(counts.max()), "K_padded": KPAD, "rounds": args.rounds, "warmup": args.warmup,
                   "fingerprint_size": 26, "log_index_size": 8},
        "ms": {w: rng(v) for w, v in t.items()},
        "probe": versus(t["ragged_probe"], t["padded_probe"]),
        "compact": versus(t["ragged_compact"], t["padded_compact"]),
        "probe_plus_compact": versus(t["ragged_total"], t["padded_total"]),
        "uniform4_probe": versus(t["uniform4_ragged_probe"], t["uniform4_fixed_probe"]),
        # per pair an id, a line and a word, and the pair's share of its key (--var: mean length + 8 of offset)
        # and of the key's 8-byte list offset
        "ragged_algorithmic_bytes_per_pair": round(4 + 64 + 8 + (key_bytes + 8) / mean_list, 3),
        "candidates": count,
        "ragged_found_bytes": m * 8,
        "padded_found_bytes": n * KPAD * 8,
        "verified": "the non-padded words of (a) and (b) equal, no padded slot found anything, both outputs of (c) "
                    "equal; every (key, own filter) pair found",
        "device": torch.cuda.get_device_name(0),
    }
    if args.var:
        out["config"]["mean_key_len"] = round(mean_len, 3)
    return out


ROUTED_R = 4096  # --routed: ranges of the map


def routed(args, fset, eng, stream, kin, timed, rng):
    """--routed: (a) route, (b) route + ragged probe + compaction, (c) ragged probe + compaction
    from a precomputed CSR, (d) the host alternative to (a); kin: the keys' arguments"""
    import time

    import numpy as np
    F, n, R = args.filters, args.n, ROUTED_R
    st = stream.cuda_stream
    dev = kin[0].device
    L = E.load_library()
    hr = np.random.default_rng(11)
    probe_r = fset.probe_var_keys_ragged if args.var else fset.probe_keys_ragged

    # keys to the host once (pinned), as (d) does every round
    def keys_to_host(pins):
        with torch.cuda.stream(stream):
            for p, d in zip(pins, kin if args.var else kin[:1]):
                p.copy_(d.reshape(-1), non_blocking=True)
        stream.synchronize()

    pins = [torch.empty(x.numel(), dtype=x.dtype, pin_memory=True) for x in (kin if args.var else kin[:1])]
    keys_to_host(pins)

    def prefixes(pins):
        """every key's first 8 bytes as a big-endian uint64 (a strided view of the pinned bytes)"""
        b = pins[0].numpy()
        if args.var:
            return np.ndarray((b.size - 7,), dtype=">u8", buffer=b.data, strides=(1,))[pins[1].numpy()[:-1]]
        return np.ndarray((n,), dtype=">u8", buffer=b.data, strides=(24,))

    def key_bytes(i):
        if args.var:
            o = pins[1].numpy()
            return bytes(pins[0].numpy()[int(o[i]):int(o[i + 1])])
        return bytes(pins[0].numpy()[24 * i:24 * i + 24])

    # R - 1 boundaries from the key population, one per 8-byte prefix
    pre = prefixes(pins)
    cand = hr.choice(n, size=2 * R, replace=False)
    _, first = np.unique(pre[cand], return_index=True)
    cand = cand[np.sort(first)][:R - 1]
    assert cand.size == R - 1, "too few keys with distinct prefixes"
    bounds = sorted(key_bytes(int(i)) for i in cand)
    bpre = np.array([int.from_bytes(b[:8], "big") for b in bounds], dtype=np.uint64)
    assert (bpre[1:] > bpre[:-1]).all()
    llen = np.minimum(KPAD, 1 + hr.geometric(1.0 / 3.0, size=R)).astype(np.int64)
    loff = np.zeros(R + 1, dtype=np.int64)
    np.cumsum(llen, out=loff[1:])
    flat = hr.integers(0, F, size=int(loff[-1])).astype(np.uint32)
    lists = [flat[loff[r]:loff[r + 1]].tolist() for r in range(R)]
    rmap = E.RangeMap(bounds, lists, engine=eng)
    assert rmap.max_list <= KPAD
    pair_cap = n * rmap.max_list

    def host_route(pins):
        """(d)'s compute: ranges by searchsorted over the prefixes, then the CSR"""
        rg = np.searchsorted(bpre, prefixes(pins), side="right").astype(np.uint32)
        cnt = llen[rg]
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(cnt, out=off[1:])
        key = np.repeat(np.arange(n, dtype=np.int64), cnt)
        src = loff[rg][key] + (np.arange(int(off[-1]), dtype=np.int64) - off[:-1][key])
        return rg, off, flat[src]

    with torch.cuda.stream(stream):
        d_range = torch.zeros(n, dtype=torch.int32, device=dev)
        d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_member = torch.zeros(pair_cap, dtype=torch.int32, device=dev)
        d_total = torch.zeros(1, dtype=torch.int64, device=dev)
        scratch = torch.zeros(E.range_route_scratch_bytes(n) // 8, dtype=torch.int64, device=dev)
        d_count = torch.zeros(1, dtype=torch.int64, device=dev)
    stream.synchronize()

    def route():
        out = (d_range.data_ptr(), d_off.data_ptr(), d_member.data_ptr(), pair_cap, d_total.data_ptr(),
               scratch.data_ptr(), st)
        if args.var:
            E._check(L.rf_amd_range_map_route_var_keys(rmap.h, kin[0].data_ptr(), kin[1].data_ptr(), n, *out))
        else:
            E._check(L.rf_amd_range_map_route_keys(rmap.h, kin[0].data_ptr(), 24, n, *out))

    # (a)'s output against the host mirror and against (d)'s result, before anything is timed
    route()
    stream.synchronize()
    m = int(d_total.item())
    rg_h, off_h, mem_h = host_route(pins)
    assert m == int(off_h[-1]), "total differs from the host's"
    assert np.array_equal(d_range.cpu().numpy().view(np.uint32), rg_h), "ranges differ from the host's"
    assert np.array_equal(d_off.cpu().numpy(), off_h), "offsets differ from the host's"
    assert np.array_equal(d_member[:m].cpu().numpy().view(np.uint32), mem_h), "ids differ from the host's"
    sample = hr.choice(n, size=1 << 16, replace=False)
    sample[:R - 1] = cand  # the boundaries themselves among them
    mirror = E.range_route_host(bounds, lists, [key_bytes(int(i)) for i in sample])[0]
    assert np.array_equal(mirror, rg_h[sample]), "ranges differ from E.range_route_host"
    del rg_h, mem_h, mirror
    with torch.cuda.stream(stream):
        off_pre, member_pre = d_off.clone(), d_member[:m].clone()  # (c)'s precomputed CSR
        found = torch.zeros(m, dtype=torch.int64, device=dev)
        probe_r(*kin, member_pre, off_pre, n, found, stream=st)
        E.found_compact(found, m, None, d_count, stream=st, engine=eng)
    stream.synchronize()
    count = int(d_count.item())
    with torch.cuda.stream(stream):
        d_cand = torch.zeros(max(count, 1), dtype=torch.int64, device=dev)
        found_b = torch.zeros(m, dtype=torch.int64, device=dev)
        h_off = torch.empty(n + 1, dtype=torch.int64, pin_memory=True)
        h_mem = torch.empty(m, dtype=torch.int32, pin_memory=True)
        up_off, up_mem = torch.zeros_like(off_pre), torch.zeros_like(member_pre)
    stream.synchronize()

    def routed_multiget():  # found_b is sized by the pair count read once above; the route call
        route()             # itself needs no read: pair_cap = n * max_list
        probe_r(*kin, d_member, d_off, n, found_b, stream=st)
        E.found_compact(found_b, m, d_cand, d_count, stream=st, engine=eng)

    def csr_multiget():
        probe_r(*kin, member_pre, off_pre, n, found, stream=st)
        E.found_compact(found, m, d_cand, d_count, stream=st, engine=eng)

    def host_alternative():
        stream.synchronize()
        t0 = time.perf_counter()
        keys_to_host(pins)
        t1 = time.perf_counter()
        _, off, mem = host_route(pins)
        t2 = time.perf_counter()
        h_off.numpy()[:] = off
        h_mem.numpy()[:] = mem.view(np.int32)
        with torch.cuda.stream(stream):
            up_off.copy_(h_off, non_blocking=True)
            up_mem.copy_(h_mem, non_blocking=True)
        stream.synchronize()
        t3 = time.perf_counter()
        return [(t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3]

    t = {"route": [], "routed_multiget": [], "csr_multiget": [], "host_total": [], "host_d2h": [],
         "host_compute": [], "host_h2d": []}
    for r in range(args.warmup + args.rounds):
        a, b, c = timed(route), timed(routed_multiget), timed(csr_multiget)
        d = host_alternative()
        if r >= args.warmup:
            for w, ms in zip(t, [a, b, c] + d):
                t[w].append(ms)
    assert int(d_count.item()) == count and torch.equal(found, found_b) and torch.equal(up_mem, member_pre)
    t["csr_plus_host"] = [x + y for x, y in zip(t["csr_multiget"], t["host_total"])]
    ms = {w: rng(v) for w, v in t.items()}
    a, b, c, cd = t["route"], t["routed_multiget"], t["csr_multiget"], t["csr_plus_host"]
    out = {
        "what": ("multi-get of n %s from raw device keys through a range map of R ranges (boundaries drawn from the "
                 "keys, lists of min(16, 1 + Geometric(1/3)) random members of one batch of F filters): (a) the route "
                 "call alone, (b) route + ragged probe + found_compact, (c) ragged probe + found_compact from a "
                 "precomputed CSR, (d) the host alternative to (a) by the wall clock: keys D2H into pinned memory, "
                 "np.searchsorted over big-endian 8-byte prefixes, the CSR by numpy, its H2D; alternating rounds in "
                 "one process, HIP events on the launch stream for (a)-(c)"
                 % ("variable-length keys (keys.var_keys, 8-100 B)" if args.var else "24-byte keys")),
        "config": {"filters": F, "keys_per_filter": args.keys, "n": n, "ranges": R, "pairs": m,
                   "mean_list": round(m / n, 4), "max_list": rmap.max_list, "rounds": args.rounds,
                   "warmup": args.warmup, "fingerprint_size": 26, "log_index_size": 8},
        "ms": ms,
        "route_share_of_csr_multiget": {"min": round(min(a) / max(c), 4), "max": round(max(a) / min(c), 4)},
        "routed_vs_csr_plus_host": {"ranges_touch": not (max(b) < min(cd) or max(cd) < min(b)),
                                    "routed_faster_beyond_ranges": bool(max(b) < min(cd))},
        "routed_minus_csr_ms": {"min": round(min(x - y for x, y in zip(b, c)), 4),
                                "max": round(max(x - y for x, y in zip(b, c)), 4)},
        "candidates": count,
        "csr_bytes": 8 * (n + 1) + 4 * m,
        "candidate_bytes": 8 * count,
        "verified": "ranges, offsets, ids and total of (a) equal to (d)'s for all n keys; ranges equal to "
                    "E.range_route_host for 2^16 sampled keys, every boundary key among them; found words of (b) "
                    "and (c) equal",
        "device": torch.cuda.get_device_name(0),
    }
    rmap.close()
    return out


def csr_workloads(args, eng, stream, kin, hr):
    """the two member-list workloads of --per-key and --exists as (name, make) pairs, make()
    returning (d_member_off, d_member, pairs): the --ragged lists and the CSR of a route call
    through a map of ROUTED_R such lists; hr: the host generator both draw from, in this order"""
    import numpy as np
    F, n, R = args.filters, args.n, ROUTED_R
    st = stream.cuda_stream
    dev = kin[0].device

    def geometric(size):
        return np.minimum(KPAD, 1 + hr.geometric(1.0 / 3.0, size=size)).astype(np.int64)

    def ragged_csr():
        """the --ragged lists: key i has min(16, 1 + Geometric(1/3)) random members"""
        off_h = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(geometric(n), out=off_h[1:])
        with torch.cuda.stream(stream):
            g = torch.Generator(device=dev)
            g.manual_seed(9)
            off = torch.from_numpy(off_h).to(dev)
            member = torch.randint(0, F, (int(off_h[-1]),), device=dev, generator=g).to(torch.int32)
        stream.synchronize()
        return off, member, int(off_h[-1])

    def routed_csr():
        """the --routed lists: the CSR a route call writes for a map of R ranges cut by keys of the
        population, each range with such a list"""
        pick = torch.from_numpy(hr.choice(n, size=2 * R, replace=False)).to(dev)
        with torch.cuda.stream(stream):
            if args.var:
                lo, hi = kin[1][pick].tolist(), kin[1][pick + 1].tolist()
                keys = {bytes(kin[0][a:b].cpu().numpy()) for a, b in zip(lo, hi)}
            else:
                keys = {bytes(row) for row in kin[0].reshape(n, 24)[pick].cpu().numpy()}
        bounds = sorted(keys)[:R - 1]
        assert len(bounds) == R - 1, "too few distinct keys"
        llen = geometric(R)
        lists = [hr.integers(0, F, size=int(k)).tolist() for k in llen]
        rmap = E.RangeMap(bounds, lists, engine=eng)
        with torch.cuda.stream(stream):
            route = rmap.route_var_keys if args.var else rmap.route_keys
            _, d_off, d_member, d_total = route(*kin, n, stream=st)
        stream.synchronize()
        m = int(d_total.item())
        with torch.cuda.stream(stream):
            off, member = d_off.clone(), d_member[:m].clone()
        stream.synchronize()
        del d_off, d_member
        rmap.close()
        return off, member, m

    return (("ragged", ragged_csr), ("routed", routed_csr))


def by_branch(args, fset, eng, stream, kin, own, timed, rng):
    """--by-branch: the per-key records grouped by branch, two ways, on the CSR of a route call
    (the --per-key shape) and on lists that hold every key's own filter, so that every key has at
    least one record; kin: the keys' arguments, own: the filter that holds key i"""
    import statistics

    import numpy as np
    F, n = args.filters, args.n
    st = stream.cuda_stream
    dev = kin[0].device
    hr = np.random.default_rng(13)
    probe_r = fset.probe_var_keys_ragged if args.var else fset.probe_keys_ragged
    nm = fset.num_members
    mask = (1 << (nm - 1).bit_length()) - 1
    passes = E.diag_by_branch_passes(nm)

    def present_csr():
        """key i against its own filter and three random ones"""
        with torch.cuda.stream(stream):
            g = torch.Generator(device=dev)
            g.manual_seed(11)
            member = torch.randint(0, F, (n, 4), device=dev, generator=g).to(torch.int32)
            member[:, 0] = own.to(torch.int32)
            off = torch.arange(n + 1, device=dev, dtype=torch.int64) * 4
        stream.synchronize()
        return off, member.reshape(-1).contiguous(), 4 * n

    def measure(off, member, m):
        with torch.cuda.stream(stream):
            found = torch.zeros(m, dtype=torch.int64, device=dev)
            d_count = torch.zeros(1, dtype=torch.int64, device=dev)
            d_key_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            probe_r(*kin, member, off, n, found, stream=st)
            E.found_per_key_ragged(found, member, off, n, d_key_off, None, None, d_count, stream=st, engine=eng)
        stream.synchronize()
        count = int(d_count.item())
        bcap = 64 * nm
        with torch.cuda.stream(stream):
            d_cand = torch.zeros(max(count, 1), dtype=torch.int64, device=dev)
            d_cand_key = torch.zeros_like(d_cand)
            E.found_per_key_ragged(found, member, off, n, d_key_off, d_cand, d_cand_key, d_count, stream=st,
                                   engine=eng)
            d_order = torch.zeros(max(count, 1), dtype=torch.int32, device=dev)
            d_okey = torch.zeros_like(d_cand)
            d_branch = torch.zeros(bcap, dtype=torch.int64, device=dev)
            d_boff = torch.zeros(bcap + 1, dtype=torch.int64, device=dev)
            d_runs = torch.zeros(1, dtype=torch.int64, device=dev)
        stream.synchronize()
        del found, d_key_off
        got = {}

        def sort_key(c):
            return (((c >> 8) & mask) << 6) | (c & 63)

        def parent_path():  # what a caller had on the device: a stable sort, the gather, the runs
            skey, order = torch.sort(sort_key(d_cand[:count]), stable=True)
            got["order"] = order
            got["order_key"] = d_cand_key[:count][order]
            got["u"], got["counts"] = torch.unique_consecutive(skey, return_counts=True)

        def by_branch_call():
            E.found_by_branch(d_cand, d_cand_key, d_count, count, nm, d_order, d_okey, d_branch, d_boff, bcap,
                              d_runs, stream=st, engine=eng)

        # both ways once, compared before anything is timed
        with torch.cuda.stream(stream):
            parent_path()
            by_branch_call()
        stream.synchronize()
        with torch.cuda.stream(stream):
            runs = int(d_runs.item())
            assert runs == got["u"].numel() <= bcap, "the numbers of runs differ"
            assert torch.equal(d_order[:count].to(torch.int64), got["order"]), "order differs from torch.sort"
            assert torch.equal(d_okey[:count], got["order_key"]), "keys differ from the gather"
            starts = torch.cumsum(got["counts"], 0) - got["counts"]
            assert torch.equal(d_boff[:runs], starts) and int(d_boff[runs].item()) == count, "run starts differ"
            assert torch.equal(sort_key(d_branch[:runs]), got["u"]), "branches differ from unique_consecutive"
            del starts
        stream.synchronize()
        ways = {"parent_path": parent_path, "by_branch": by_branch_call}
        t = {w: [] for w in ways}
        for r in range(args.warmup + args.rounds):
            for w, fn in ways.items():  # alternating: one of each per round
                ms = timed(fn)
                if r >= args.warmup:
                    t[w].append(ms)
        a, b = t["parent_path"], t["by_branch"]
        spread = max(a) - min(a)
        return {
            "pairs": m, "records": count, "records_per_key": round(count / n, 4), "branches": runs,
            "num_members": nm, "passes": passes,
            "ms": {w: dict(rng(v), median=round(statistics.median(v), 4)) for w, v in t.items()},
            "parent_spread_ms": round(spread, 4),
            # the condition: the new call's median is not above the parent path's by more than that
            # path's own round-to-round spread
            "by_branch_within_parent_spread": bool(statistics.median(b) <= statistics.median(a) + spread),
            "ranges_touch": not (max(a) < min(b) or max(b) < min(a)),
            "by_branch_faster_beyond_ranges": bool(max(b) < min(a)),
            "by_branch_slower_beyond_ranges": bool(max(a) < min(b)),
            # the new call, per record: each pass reads it twice (8 + 8) and all but the last write the
            # pair (8); the last writes order and sort key (4 + 4) and gathers the key (8 + 8); the run
            # table reads the sort keys twice (4 + 4)
            "by_branch_algorithmic_bytes": count * (24 * passes + 24),
        }

    out = {
        "what": ("the records of a per-key multi-get of n %s grouped by branch, two ways: (parent_path) "
                 "torch.sort(stable=True) of the sort keys, the gather of the records' keys, "
                 "torch.unique_consecutive(return_counts=True), its synchronisation and allocations included; "
                 "(by_branch) one rf_amd_found_by_branch; on the CSR of a route call through a map of R lists of "
                 "min(16, 1 + Geometric(1/3)) random members (3 %% non-zero words) and on lists of each key's own "
                 "filter and three random ones (every key present); alternating rounds in one process, HIP events "
                 "on the launch stream" % ("variable-length keys (keys.var_keys, 8-100 B)" if args.var
                                           else "24-byte keys")),
        "config": {"filters": F, "keys_per_filter": args.keys, "n": n, "ranges": ROUTED_R, "rounds": args.rounds,
                   "warmup": args.warmup, "fingerprint_size": 26, "log_index_size": 8},
    }
    for name, csr in csr_workloads(args, eng, stream, kin, hr) + (("present", present_csr),):
        off, member, m = csr()  # the --ragged lists are drawn too, so that the route call's are --per-key's
        if name != "ragged":
            out[name] = measure(off, member, m)
        del off, member
    out["verified"] = ("before timing, on both workloads: the numbers of runs equal; d_order equal to torch.sort's "
                       "indices; d_order_key equal to the gather; the run starts equal to the exclusive sums of "
                       "unique_consecutive's counts; the sort keys of d_branch equal to its values")
    return out


def advance(args, fset, eng, stream, kin, own, timed, rng):
    """--advance: one step of the early-exit multi-get, two ways, on the CSR of a route call (the
    --per-key shape), on lists that hold every key's own filter and three random ones, and on
    lists of eight that name the own filter four times (a key that lives in four bundles of its
    path); then the records a whole multi-get hands to the consumer at width 1, 2 and 4 against all
    the records, which is what found_by_branch groups without the exit. kin: the keys' arguments,
    own: the filter that holds key i"""
    import statistics

    import numpy as np
    F, n = args.filters, args.n
    st = stream.cuda_stream
    dev = kin[0].device
    hr = np.random.default_rng(13)
    probe_r = fset.probe_var_keys_ragged if args.var else fset.probe_keys_ragged

    def present_csr(k, own_at):
        """key i against k members, its own filter at the places own_at and random ones elsewhere"""
        def make():
            with torch.cuda.stream(stream):
                g = torch.Generator(device=dev)
                g.manual_seed(11)
                member = torch.randint(0, F, (n, k), device=dev, generator=g).to(torch.int32)
                for j in own_at:
                    member[:, j] = own.to(torch.int32)
                off = torch.arange(n + 1, device=dev, dtype=torch.int64) * k
            stream.synchronize()
            return off, member.reshape(-1).contiguous(), k * n
        return make

    def measure(off, member, m):
        with torch.cuda.stream(stream):
            found = torch.zeros(m, dtype=torch.int64, device=dev)
            d_count = torch.zeros(1, dtype=torch.int64, device=dev)
            d_key_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            probe_r(*kin, member, off, n, found, stream=st)
            E.found_per_key_ragged(found, member, off, n, d_key_off, None, None, d_count, stream=st, engine=eng)
        stream.synchronize()
        count = int(d_count.item())
        with torch.cuda.stream(stream):
            d_cand = torch.zeros(max(count, 1), dtype=torch.int64, device=dev)
            E.found_per_key_ragged(found, member, off, n, d_key_off, d_cand, None, d_count, stream=st, engine=eng)
            d_done = torch.zeros(n, dtype=torch.uint8, device=dev)
            d_cursor = torch.zeros(n, dtype=torch.int32, device=dev)
            zero_cursor = torch.zeros(n, dtype=torch.int32, device=dev)
            out_cap = max(1, min(count, 4 * n))  # the widest step below
            d_out = torch.zeros(out_cap, dtype=torch.int64, device=dev)
            d_out_key = torch.zeros(out_cap, dtype=torch.int64, device=dev)
            d_out_count = torch.zeros(1, dtype=torch.int64, device=dev)
            ar = torch.arange(n, device=dev, dtype=torch.int64)
        stream.synchronize()
        del found
        got = {}

        def parent_path(width=1, cursor=zero_cursor, done=d_done):
            # what a caller had on the device: masks, a cumsum, repeat_interleave (which waits for the
            # total) and the gather, every step into fresh tensors
            a = d_key_off[:-1] + cursor
            e = torch.clamp(d_key_off[1:], max=count)
            take = torch.clamp(torch.clamp(e - a, max=width), min=0) * (done == 0)
            pos = torch.cumsum(take, 0) - take
            key = torch.repeat_interleave(ar, take)
            src = torch.arange(key.numel(), device=dev, dtype=torch.int64) - pos[key] + a[key]
            got["cand"], got["key"], got["cursor"] = d_cand[src], key, (cursor + take).to(torch.int32)

        def advance_call(width=1, flags=E.ADVANCE_FIRST, done=d_done):
            E.found_advance(d_key_off, d_cand, count, n, width, flags, done, d_cursor, d_out, d_out_key, out_cap,
                            d_out_count, stream=st, engine=eng)

        # both ways once, on the first step and on a later one, compared before anything is timed
        with torch.cuda.stream(stream):
            g = torch.Generator(device=dev)
            g.manual_seed(5)
            some_done = (torch.rand(n, device=dev, generator=g) < 0.5).to(torch.uint8)
            one = torch.ones(n, dtype=torch.int32, device=dev)
        for width, flags, cursor, done in ((1, E.ADVANCE_FIRST, zero_cursor, d_done), (2, 0, one, some_done)):
            with torch.cuda.stream(stream):
                d_cursor.copy_(cursor)
                parent_path(width, cursor, done)
                advance_call(width, flags, done)
            stream.synchronize()
            with torch.cuda.stream(stream):
                k = int(d_out_count.item())
                assert k == got["key"].numel() <= out_cap, "the totals differ"
                assert torch.equal(d_out[:k], got["cand"]), "records differ from the gather"
                assert torch.equal(d_out_key[:k], got["key"]), "keys differ from repeat_interleave"
                assert torch.equal(d_cursor, got["cursor"]), "cursors differ"
            stream.synchronize()
        del some_done, one
        first_step = int((d_key_off[1:] > d_key_off[:-1]).sum().item())
        ways = {"parent_path": parent_path, "advance": advance_call}
        t = {w: [] for w in ways}
        for r in range(args.warmup + args.rounds):
            for w, fn in ways.items():  # alternating: one of each per round
                ms = timed(fn)
                if r >= args.warmup:
                    t[w].append(ms)
        got.clear()

        def whole_multiget(width):
            """advance, mark the keys whose step held their own filter, until nothing is handed out"""
            handed, steps = 0, 0
            with torch.cuda.stream(stream):
                d_done.zero_()
            while True:
                with torch.cuda.stream(stream):
                    advance_call(width, 0 if steps else E.ADVANCE_FIRST)
                stream.synchronize()
                k = int(d_out_count.item())
                if k == 0:
                    break
                with torch.cuda.stream(stream):
                    keys_out = d_out_key[:k]
                    hit = (d_out[:k] >> 8) == own[keys_out]
                    d_done[keys_out[hit]] = 1
                stream.synchronize()
                handed, steps = handed + k, steps + 1
            return {"records_handed_out": handed, "steps": steps,
                    "of_all_records": round(handed / max(count, 1), 4)}

        exits = {"width_%d" % w: whole_multiget(w) for w in (1, 2, 4)}
        a, b = t["parent_path"], t["advance"]
        spread = max(a) - min(a)
        return {
            "pairs": m, "records": count, "records_per_key": round(count / n, 4),
            "records_in_the_timed_step": first_step,
            "ms": {w: dict(rng(v), median=round(statistics.median(v), 4)) for w, v in t.items()},
            "parent_spread_ms": round(spread, 4),
            # the condition: the new call's median is not above the parent path's by more than that
            # path's own round-to-round spread
            "advance_within_parent_spread": bool(statistics.median(b) <= statistics.median(a) + spread),
            "ranges_touch": not (max(a) < min(b) or max(b) < min(a)),
            "advance_faster_beyond_ranges": bool(max(b) < min(a)),
            "advance_slower_beyond_ranges": bool(max(a) < min(b)),
            # the new call under FIRST: both kernels read two offsets and the done byte per key (the
            # neighbour's offset comes from the same lines: 8 + 1, twice), the emit writes the cursor (4)
            # and per record reads it and writes it and its key (8 + 8 + 8)
            "advance_algorithmic_bytes": n * (2 * 9 + 4) + first_step * 24,
            # found_by_branch without the exit groups all `records`; with it, what the steps hand out
            "whole_multiget_with_early_exit": exits,
        }

    out = {
        "what": ("one step of a per-key multi-get of n %s with early exit, two ways: (parent_path) torch masks, "
                 "cumsum, repeat_interleave and the gather, its synchronisation and allocations included; (advance) "
                 "one rf_amd_found_advance at width 1 under RF_AMD_ADVANCE_FIRST with a done buffer of zeros, so "
                 "that every round starts from the same cursors; on the CSR of a route call through a map of R "
                 "lists of min(16, 1 + Geometric(1/3)) random members (3 %% non-zero words), on lists of each "
                 "key's own filter and three random ones (every key present), and on lists of eight that name "
                 "the own filter at the places 0, 2, 4 and 6 (every key present in 4 of its members); "
                 "alternating rounds in one process, HIP events on the launch stream. Then whole multi-gets "
                 "at width 1, 2 and 4, a key being done when a step held a record of its own filter: the "
                 "records handed to the consumer against all records" % (
                     "variable-length keys (keys.var_keys, 8-100 B)" if args.var else "24-byte keys")),
        "config": {"filters": F, "keys_per_filter": args.keys, "n": n, "ranges": ROUTED_R, "rounds": args.rounds,
                   "warmup": args.warmup, "fingerprint_size": 26, "log_index_size": 8},
    }
    shapes = csr_workloads(args, eng, stream, kin, hr) + (("present", present_csr(4, (0,))),
                                                          ("present_in_4", present_csr(8, (0, 2, 4, 6))))
    for name, csr in shapes:
        off, member, m = csr()  # the --ragged lists are drawn too, so that the route call's are --per-key's
        if name != "ragged":
            out[name] = measure(off, member, m)
        del off, member
    out["verified"] = ("before timing, on every workload, for the first step at width 1 and for a later step at "
                       "width 2 with half the keys done: the totals equal; d_out_cand equal to the gather; d_out_key "
                       "equal to repeat_interleave's keys; the cursors equal")
    return out


def per_key(args, fset, eng, stream, kin, timed, rng):
    """--per-key: candidates with member ids, keys and a CSR over the keys, two ways, on the
    --ragged lists and on the CSR of a route call; kin: the keys' arguments"""
    import statistics

    import numpy as np
    F, n, R = args.filters, args.n, ROUTED_R
    st = stream.cuda_stream
    dev = kin[0].device
    hr = np.random.default_rng(13)
    probe_r = fset.probe_var_keys_ragged if args.var else fset.probe_keys_ragged

    def measure(off, member, m):
        with torch.cuda.stream(stream):
            found = torch.zeros(m, dtype=torch.int64, device=dev)
            d_count = torch.zeros(1, dtype=torch.int64, device=dev)
            probe_r(*kin, member, off, n, found, stream=st)
            E.found_compact(found, m, None, d_count, stream=st, engine=eng)
        stream.synchronize()
        count = int(d_count.item())
        with torch.cuda.stream(stream):
            d_cand = torch.zeros(max(count, 1), dtype=torch.int64, device=dev)
            d_cand2, d_cand_key = torch.zeros_like(d_cand), torch.zeros_like(d_cand)
            d_key_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            d_count2 = torch.zeros(1, dtype=torch.int64, device=dev)
        stream.synchronize()
        got = {}

        def parent_path():  # what a caller had: the records, then each record's key and member id
            E.found_compact(found, m, d_cand, d_count, stream=st, engine=eng)
            pair = d_cand[:count] >> 8
            got["key"] = torch.searchsorted(off, pair, right=True) - 1
            got["id"] = member[pair]

        def per_key_call():
            E.found_per_key_ragged(found, member, off, n, d_key_off, d_cand2, d_cand_key, d_count2, stream=st,
                                   engine=eng)

        # both ways once, compared before anything is timed
        with torch.cuda.stream(stream):
            parent_path()
            per_key_call()
        stream.synchronize()
        with torch.cuda.stream(stream):
            assert int(d_count2.item()) == count == int(d_key_off[n].item()), "the totals differ"
            want = (got["id"].to(torch.int64) & 0xFFFFFFFF) << 8 | (d_cand[:count] & 0xFF)
            assert torch.equal(d_cand2[:count], want), "records differ from found_compact + gather"
            assert torch.equal(d_cand_key[:count], got["key"]), "keys differ from found_compact + searchsorted"
            starts = torch.searchsorted(got["key"], torch.arange(n + 1, device=dev))
            assert torch.equal(d_key_off, starts), "offsets differ from the runs of the records' keys"
            del want, starts
        stream.synchronize()
        ways = {"parent_path": parent_path, "per_key": per_key_call,
                "found_compact_alone": lambda: E.found_compact(found, m, d_cand, d_count, stream=st, engine=eng)}
        t = {w: [] for w in ways}
        for r in range(args.warmup + args.rounds):
            for w, fn in ways.items():  # alternating: one of each per round
                ms = timed(fn)
                if r >= args.warmup:
                    t[w].append(ms)
        a, b = t["parent_path"], t["per_key"]
        spread = max(a) - min(a)
        return {
            "pairs": m, "mean_list": round(m / n, 4), "candidates": count,
            "ms": {w: dict(rng(v), median=round(statistics.median(v), 4)) for w, v in t.items()},
            "parent_spread_ms": round(spread, 4),
            # the condition: the new call's median is not above the parent path's by more than that
            # path's own round-to-round spread
            "per_key_within_parent_spread": bool(statistics.median(b) <= statistics.median(a) + spread),
            "ranges_touch": not (max(a) < min(b) or max(b) < min(a)),
            "per_key_faster_beyond_ranges": bool(max(b) < min(a)),
            "per_key_slower_beyond_ranges": bool(max(a) < min(b)),
            # the new call: every word at most twice; per key its pair offset read, its count written and
            # read and its record offset written; per record at most one id, the record and its key
            "per_key_algorithmic_bytes": 16 * m + 24 * n + 20 * count,
            # the parent path: every word twice and the record written; then per record the shift (8 + 8),
            # the search (8 + 8, the offsets it visits not counted), the - 1 (8 + 8), the gather (8 + 4 + 4)
            "parent_algorithmic_bytes": 16 * m + 72 * count,
        }

    out = {
        "what": ("the candidates of a ragged multi-get of n %s with each record's member id and key, two ways: "
                 "(parent_path) found_compact, torch.searchsorted of the records' pairs over the n + 1 offsets, the "
                 "gather member[pair]; (per_key) one rf_amd_found_per_key_ragged, which also writes the CSR of the "
                 "records over the keys; on the --ragged lists (min(16, 1 + Geometric(1/3)) random members of one "
                 "batch of F filters per key) and on the CSR of a route call through a map of R such lists; "
                 "alternating rounds in one process, HIP events on the launch stream"
                 % ("variable-length keys (keys.var_keys, 8-100 B)" if args.var else "24-byte keys")),
        "config": {"filters": F, "keys_per_filter": args.keys, "n": n, "ranges": R, "rounds": args.rounds,
                   "warmup": args.warmup, "fingerprint_size": 26, "log_index_size": 8},
    }
    for name, csr in csr_workloads(args, eng, stream, kin, hr):
        off, member, m = csr()
        out[name] = measure(off, member, m)
        del off, member
    out["verified"] = ("before timing, on both workloads: totals equal; every record equal to member[pair] << 8 | value "
                       "of found_compact's record; every record's key equal to searchsorted's; the offsets equal "
                       "to the starts of the keys' runs")
    out["device"] = torch.cuda.get_device_name(0)
    return out


def exists(args, fset, eng, stream, kin, timed, rng):
    """--exists: the existence multi-get against the ragged probe alone, on the --ragged lists and
    on the CSR of a route call; kin: the keys' arguments"""
    import statistics

    import numpy as np
    F, n, R = args.filters, args.n, ROUTED_R
    st = stream.cuda_stream
    dev = kin[0].device
    hr = np.random.default_rng(13)
    probe_r = fset.probe_var_keys_ragged if args.var else fset.probe_keys_ragged
    exists_r = fset.exists_var_keys_ragged if args.var else fset.exists_keys_ragged

    def measure(off, member, m):
        with torch.cuda.stream(stream):
            found = torch.zeros(m, dtype=torch.int64, device=dev)
            d_exists = torch.full((n,), 0xAB, dtype=torch.uint8, device=dev)
            # both once, compared before anything is timed: the set holds filters only, so the byte
            # is "some word of the key's pairs is not zero"
            probe_r(*kin, member, off, n, found, stream=st)
            exists_r(*kin, member, off, n, d_exists, stream=st)
        stream.synchronize()
        with torch.cuda.stream(stream):
            key = torch.repeat_interleave(torch.arange(n, device=dev), off[1:] - off[:-1])
            want = torch.zeros(n, dtype=torch.uint8, device=dev)
            want[key[found != 0]] = E.EXISTS_FILTER_HIT
            assert torch.equal(d_exists, want), "the bytes differ from the ragged probe's words"
            hits = int(want.sum())
            del key, want
        stream.synchronize()
        ways = {"ragged_probe": lambda: probe_r(*kin, member, off, n, found, stream=st),
                "exists": lambda: exists_r(*kin, member, off, n, d_exists, stream=st)}
        t = {w: [] for w in ways}
        for r in range(args.warmup + args.rounds):
            for w, fn in ways.items():  # alternating: one of each per round
                ms = timed(fn)
                if r >= args.warmup:
                    t[w].append(ms)
        a, b = t["ragged_probe"], t["exists"]
        spread = max(a) - min(a)
        return {
            "pairs": m, "mean_list": round(m / n, 4), "keys_that_might_exist": hits,
            "ms": {w: dict(rng(v), median=round(statistics.median(v), 4)) for w, v in t.items()},
            "parent_spread_ms": round(spread, 4),
            # the condition: the existence call's median is not above the ragged probe's by more than
            # that probe's own round-to-round spread
            "exists_within_parent_spread": bool(statistics.median(b) <= statistics.median(a) + spread),
            "ranges_touch": not (max(a) < min(b) or max(b) < min(a)),
            "exists_faster_beyond_ranges": bool(max(b) < min(a)),
            "exists_slower_beyond_ranges": bool(max(a) < min(b)),
            "ragged_probe_output_bytes": 8 * m,
            "exists_output_bytes": n,
        }

    out = {
        "what": ("existence multi-get of n %s (rf_amd_filter_set_exists_%skeys_ragged: one byte per key, no found "
                 "word) against the cheapest possible start of any way to get the answer from the parent commit, the "
                 "ragged probe alone on the same inputs (8 bytes per pair, still to be reduced); on the --ragged lists "
                 "(min(16, 1 + Geometric(1/3)) random members of one batch of F filters per key) and on the CSR of a "
                 "route call through a map of R such lists; alternating rounds in one process, HIP events on the "
                 "launch stream" % (("variable-length keys (keys.var_keys, 8-100 B)", "var_") if args.var
                                    else ("24-byte keys", ""))),
        "config": {"filters": F, "keys_per_filter": args.keys, "n": n, "ranges": R, "rounds": args.rounds,
                   "warmup": args.warmup, "fingerprint_size": 26, "log_index_size": 8},
    }
    for name, csr in csr_workloads(args, eng, stream, kin, hr):
        off, member, m = csr()
        out[name] = measure(off, member, m)
        del off, member
    out["exists_within_parent_spread"] = bool(out["ragged"]["exists_within_parent_spread"] and
                                              out["routed"]["exists_within_parent_spread"])
    out["verified"] = ("before timing, on both workloads: every key's byte equal to 'some found word of the key's "
                       "pairs, from the ragged probe of the same inputs, is not zero'")
    out["device"] = torch.cuda.get_device_name(0)
    return out


def update_mode(args):
    """--update: a compaction's change to a resident set, two ways; see the module docstring"""
    import ctypes
    import time

    import numpy as np
    F, nk, n, Kf = args.filters, args.keys, 4096, 4
    dev = torch.device("cuda:0")
    cfg = E.routing_config_init(fingerprint_size=26, log_index_size=8, seed=42)
    eng = E.Engine(0)
    L = E.load_library()
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    with torch.cuda.stream(stream):
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        # base: the set's members; alt: the filters compactions replace them with (other keys, other values)
        h_base = torch.randint(-(1 << 31), 1 << 31, (F, nk), device=dev, generator=g).to(torch.int32)
        h_alt = torch.randint(-(1 << 31), 1 << 31, (F, nk), device=dev, generator=g).to(torch.int32)
        base = E.FilterBatch(cfg, [nk] * F, [f % 32 for f in range(F)], engine=eng)
        alt = E.FilterBatch(cfg, [nk] * F, [32 + f % 32 for f in range(F)], engine=eng)
        base.build_hashes(h_base, stream=st)
        alt.build_hashes(h_alt, stream=st)
        assert not any(i.error for i in base.infos(stream=st)) and not any(i.error for i in alt.infos(stream=st))
        # probe i: a hash of base or alt filter i % F (so a replaced member answers differently), in Kf random members
        # of which the first is its own filter
        pick = torch.randint(0, nk, (n,), device=dev, generator=g)
        own = torch.arange(n, device=dev) % F
        ph = torch.where(torch.arange(n, device=dev) % 2 == 0, h_base[own, pick], h_alt[own, pick]).contiguous()
        member = torch.randint(0, F, (n, Kf), device=dev, generator=g)
        member[:, 0] = own
        member = member.to(torch.int32).contiguous()
        found = torch.zeros(n * Kf, dtype=torch.int64, device=dev)
    stream.synchronize()

    ptrs = {"base": (ctypes.c_void_p * F)(*[base.h.value] * F), "alt": (ctypes.c_void_p * F)(*[alt.h.value] * F)}
    index = np.arange(F, dtype=np.uint32)
    hset = ctypes.c_void_p()

    us = sorted({min(u, F) for u in (1, 16, 256)})
    # way (b)'s member arrays, built here like way (a)'s: the timed region holds the C calls only.
    # (first_u, name): the first first_u members from batch `name`, the others from base
    whole = {(u, name): (ctypes.c_void_p * F)(*([ptrs[name][0]] * u + [base.h.value] * (F - u)))
             for u in [0] + us for name in ("base", "alt")}
    whole_addr = {k: ctypes.addressof(v) for k, v in whole.items()}
    eng_h, index_addr, hset_ref = eng.h, index.ctypes.data, ctypes.byref(hset)
    ptrs_addr = {k: ctypes.addressof(v) for k, v in ptrs.items()}

    def create(first_u, name):
        E._check(L.rf_amd_filter_set_create(eng_h, whole_addr[first_u, name], index_addr, F, hset_ref))

    def way_update(u, name):
        E._check(L.rf_amd_filter_set_update(hset, index_addr, ptrs_addr[name], index_addr, u, st))

    def way_recreate(u, name):
        L.rf_amd_filter_set_destroy(hset)
        create(u, name)

    def probe():
        E._check(L.rf_amd_filter_set_probe_hashes(hset, ph.data_ptr(), member.data_ptr(), Kf, n, found.data_ptr(), st))

    def timed(way, u, name):
        """(host microseconds of the call or calls, HIP-event milliseconds from before them to after the probe)"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t0 = time.perf_counter()
        way(u, name)
        host = time.perf_counter() - t0
        probe()
        b.record(stream)
        stream.synchronize()
        return host * 1e6, a.elapsed_time(b)

    def rng(v):
        return {"min": round(min(v), 4), "max": round(max(v), 4), "rounds": [round(x, 4) for x in v]}

    def versus(a, b):
        return {"ranges_touch": not (max(a) < min(b) or max(b) < min(a)),
                "update_faster_beyond_ranges": bool(max(a) < min(b)),
                "update_slower_beyond_ranges": bool(max(b) < min(a))}

    create(0, "base")
    # both ways' words after the same change, compared before anything is timed
    for u in us:
        words = {}
        for wname, way in (("update", way_update), ("recreate", way_recreate)):
            way(u, "alt")
            probe()
            stream.synchronize()
            words[wname] = found.clone()
            way(u, "base")
        assert torch.equal(words["update"], words["recreate"]), ("the two ways disagree", u)
        hit = (words["update"].view(n, Kf)[:, 0] != 0)
        even = torch.arange(n, device=dev) % 2 == 0
        assert bool(hit[even & (own >= u)].all()) and bool(hit[~even & (own < u)].all()), "false negative"
    res = {}
    for u in us:
        t = {"update": ([], []), "recreate": ([], [])}
        for r in range(args.warmup + args.rounds):
            name = "alt" if r % 2 == 0 else "base"
            for wname, way in (("update", way_update), ("recreate", way_recreate)):  # alternating
                host, ev = timed(way, u, name)
                if r >= args.warmup:
                    t[wname][0].append(host)
                    t[wname][1].append(ev)
        res[str(u)] = {
            "update_host_us": rng(t["update"][0]), "recreate_host_us": rng(t["recreate"][0]),
            "update_event_ms": rng(t["update"][1]), "recreate_event_ms": rng(t["recreate"][1]),
            "host": versus(t["update"][0], t["recreate"][0]),
            "event": versus(t["update"][1], t["recreate"][1]),
        }
    L.rf_amd_filter_set_destroy(hset)
    out = {
        "what": ("a compaction's change to a resident set of F members, two ways: (a) rf_amd_filter_set_update of u "
                 "members, (b) rf_amd_filter_set_destroy + rf_amd_filter_set_create of the whole set; after each, one "
                 "probe_hashes of n hashes in K members. host_us: wall time of the call or calls; event_ms: HIP events "
                 "on the launch stream from before the call to after the probe; the stream is idle when the first "
                 "event is recorded, so this interval contains the host time of the call and is not a second, "
                 "independent figure. Both ways' argument arrays are built before the timed region: it holds the C "
                 "calls (through ctypes) only. Alternating rounds in one process"),
        "config": {"filters": F, "keys_per_filter": nk, "n": n, "K": Kf, "rounds": args.rounds, "warmup": args.warmup,
                   "fingerprint_size": 26, "log_index_size": 8},
        "u": res,
        "update_faster_beyond_ranges": all(r["host"]["update_faster_beyond_ranges"] and
                                           r["event"]["update_faster_beyond_ranges"] for r in res.values()),
        "update_slower_beyond_ranges": any(r["host"]["update_slower_beyond_ranges"] or
                                           r["event"]["update_slower_beyond_ranges"] for r in res.values()),
        "verified": "both ways' n K words equal after the same change, for every u; every probe of its own filter found",
        "device": torch.cuda.get_device_name(0),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    base.close()
    alt.close()
    eng.close()


SEG_R, SEG_FAN, SEG_N = 4096, 16, 1 << 20  # --segments: leaves, fan-out per level, keys of a route call


def segments_mode(args):
    """--segments: a trunk change to a resident range map, two ways; see the module docstring"""
    import ctypes
    import time

    import numpy as np
    R, fan, n = SEG_R, SEG_FAN, SEG_N
    dev = torch.device("cuda:0")
    eng = E.Engine(0)
    L = E.load_library()
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    hr = np.random.default_rng(17)
    # three levels of inner nodes above the leaves: leaf r's path is the root's pivot, the pivot of
    # each inner node below it, and the leaf's own segment
    widths = [fan, fan * fan, R, R]
    first = np.concatenate([[0], np.cumsum(widths)]).tolist()
    S = first[-1]
    paths = [[first[0] + r // (R // widths[0]), first[1] + r // (R // widths[1]), first[2] + r, first[3] + r]
             for r in range(R)]
    cap = 8
    seg_lists = [hr.integers(0, 1024, size=int(hr.integers(1, cap + 1))).tolist() for _ in range(S)]
    pool = sorted({bytes(b) for b in hr.integers(0, 256, size=(R + 64, 24), dtype=np.uint8)})
    bounds = [pool[i] for i in sorted(hr.choice(len(pool), size=R - 1, replace=False))]
    assert len(bounds) == R - 1
    smap = E.RangeMap.from_segments(bounds, paths, seg_lists, [cap] * S, engine=eng)
    assert smap.max_list == 4 * cap
    pair_cap = n * smap.max_list
    with torch.cuda.stream(stream):
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        keys = torch.randint(0, 256, (n, 24), device=dev, generator=g, dtype=torch.uint8).contiguous()
        outs = [(torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev),
                 torch.zeros(pair_cap, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
                for _ in range(2)]
        scratch = torch.zeros(E.range_route_scratch_bytes(n) // 8, dtype=torch.int64, device=dev)
    stream.synchronize()

    def route(h, out):
        E._check(L.rf_amd_range_map_route_keys(h, keys.data_ptr(), 24, n, out[0].data_ptr(), out[1].data_ptr(),
                                               out[2].data_ptr(), pair_cap, out[3].data_ptr(), scratch.data_ptr(), st))

    def flat_arrays(lists):
        """the rebuilt flat table in the C call's form: what the host holds before the timed region"""
        rows = E.range_segment_lists(paths, lists)
        loff = np.zeros(R + 1, dtype=np.uint64)
        np.cumsum(np.array([len(x) for x in rows], dtype=np.uint64), out=loff[1:])
        return rows, np.fromiter((i for x in rows for i in x), dtype=np.uint32, count=int(loff[-1])), loff

    boff = np.zeros(R, dtype=np.uint64)
    np.cumsum(np.array([len(b) for b in bounds], dtype=np.uint64), out=boff[1:])
    bbytes = np.frombuffer(b"".join(bounds) + b"\0", dtype=np.uint8)
    # the change: root segment 0 alternates between two lists of different lengths
    root = [seg_lists[0], hr.integers(0, 1024, size=cap if len(seg_lists[0]) < cap else 1).tolist()]
    tables = []
    for x in root:
        rows, flat, loff = flat_arrays([x] + seg_lists[1:])
        tables.append((rows, flat, loff))
    seg0 = np.zeros(1, dtype=np.uint32)
    upd = [(np.array(x, dtype=np.uint32), np.array([0, len(x)], dtype=np.uint64)) for x in root]
    hflat = ctypes.c_void_p()

    def way_update(k):
        E._check(L.rf_amd_range_map_update_segments(smap.h, seg0.ctypes.data, upd[k][0].ctypes.data,
                                                    upd[k][1].ctypes.data, 1, st))

    def create_flat(k):
        E._check(L.rf_amd_range_map_create(eng.h, R, bbytes.ctypes.data, boff.ctypes.data, tables[k][1].ctypes.data,
                                           tables[k][2].ctypes.data, ctypes.byref(hflat)))

    def way_rebuild(k):
        old = ctypes.c_void_p(hflat.value)
        create_flat(k)
        E._check(L.rf_amd_range_map_destroy_on(old, st))

    # both ways' route output after the same change, compared before anything is timed
    create_flat(0)
    for k in (1, 0):
        way_update(k)
        way_rebuild(k)
        route(smap.h, outs[0])
        route(hflat, outs[1])
        stream.synchronize()
        m = int(outs[0][3].item())
        assert m == int(outs[1][3].item()) and torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert torch.equal(outs[0][2][:m], outs[1][2][:m]), "the two ways' ids differ"
    sample = hr.choice(n, size=1 << 14, replace=False)
    hk = keys[torch.from_numpy(sample).to(dev)].cpu().numpy()
    mirror = E.range_route_host(bounds, tables[0][0], [bytes(x) for x in hk])[0]
    assert np.array_equal(mirror, outs[0][0].cpu().numpy().view(np.uint32)[sample]), "ranges differ from the host mirror"

    def timed_change(way, k):
        """(host microseconds of the C call or calls, HIP-event milliseconds around them on the stream)"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t0 = time.perf_counter()
        way(k)
        host = time.perf_counter() - t0
        b.record(stream)
        stream.synchronize()
        return host * 1e6, a.elapsed_time(b)

    def timed_route(h):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        route(h, outs[0])
        b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b)

    def timed_python_rebuild(k, old):
        """the same rebuild through the Python class, its flattening of the rows included"""
        stream.synchronize()
        t0 = time.perf_counter()
        new = E.RangeMap(bounds, tables[k][0], engine=eng)
        old.close_on(st)
        return (time.perf_counter() - t0) * 1e6, new

    def rng(v):
        return {"min": round(min(v), 4), "max": round(max(v), 4), "rounds": [round(x, 4) for x in v]}

    t = {k: [] for k in ("update_host_us", "update_event_ms", "rebuild_host_us", "rebuild_event_ms",
                         "rebuild_python_us", "route_segmented_before_ms", "route_segmented_after_ms", "route_flat_ms")}
    pymap = E.RangeMap(bounds, tables[0][0], engine=eng)
    for r in range(args.warmup + args.rounds):
        k = 1 - r % 2
        before = timed_route(smap.h)
        uh, ue = timed_change(way_update, k)
        after = timed_route(smap.h)
        rh, re = timed_change(way_rebuild, k)
        flat_ms = timed_route(hflat)
        pu, pymap = timed_python_rebuild(k, pymap)
        if r >= args.warmup:
            for name, v in (("update_host_us", uh), ("update_event_ms", ue), ("rebuild_host_us", rh),
                            ("rebuild_event_ms", re), ("rebuild_python_us", pu), ("route_segmented_before_ms", before),
                            ("route_segmented_after_ms", after), ("route_flat_ms", flat_ms)):
                t[name].append(v)
    uh, rh = t["update_host_us"], t["rebuild_host_us"]
    seg_route = t["route_segmented_before_ms"] + t["route_segmented_after_ms"]
    out = {
        "what": ("one root segment of a trunk-shaped range map changes (R leaves, paths of 4 segments, fan-out 16 per "
                 "level, lists of 1 to 8 ids, capacity 8), two ways on one stream: (a) "
                 "rf_amd_range_map_update_segments of that segment (scatter + flatten), (b) what a flat map needs: "
                 "rf_amd_range_map_create of the rebuilt flat table + rf_amd_range_map_destroy_on of the old map. "
                 "host_us: wall time of the C call or calls, their arrays built beforehand (the host's rebuild of the "
                 "flat table is not in it); event_ms: HIP events on the stream around the calls, the stream idle at "
                 "the first, so it contains the host time. rebuild_python_us: E.RangeMap(...) + close_on by the wall "
                 "clock, the class's flattening of the rows included. route_*: one rf_amd_range_map_route_keys of n "
                 "24-byte keys by events, on the segmented map before and after each update and on the flat map; "
                 "the route kernels and the flat map are the parent commit's, so route_flat_ms is the parent's route "
                 "call in this session. Alternating rounds in one process"),
        "config": {"ranges": R, "segments": S, "fan_out": fan, "path_segments": 4, "capacity": cap, "n": n,
                   "key_len": 24, "rounds": args.rounds, "warmup": args.warmup,
                   "update_launches": 4, "ids_per_update_launch": E.diag_range_seg_launch_ids()},
        **{k: rng(v) for k, v in t.items()},
        "update_vs_rebuild_host": {"ranges_touch": not (max(uh) < min(rh) or max(rh) < min(uh)),
                                   "update_faster_beyond_ranges": bool(max(uh) < min(rh))},
        "update_vs_rebuild_event": {"update_faster_beyond_ranges": bool(max(t["update_event_ms"]) <
                                                                        min(t["rebuild_event_ms"]))},
        "route_segmented_within_flat_range": bool(min(t["route_flat_ms"]) <= max(seg_route) and
                                                  min(seg_route) <= max(t["route_flat_ms"])),
        "verified": ("after each change both ways' route output equal (ranges, offsets, ids, total) over all n keys; "
                     "ranges equal E.range_route_host on 2^14 keys"),
        "device": torch.cuda.get_device_name(0),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    L.rf_amd_range_map_destroy(hflat)
    pymap.close()
    smap.close()
    eng.close()


def split_mode(args):
    """--split: a leaf split on a resident range map, two ways; see the module docstring"""
    import ctypes
    import statistics
    import time

    import numpy as np
    R, fan, n, cap = SEG_R, SEG_FAN, SEG_N, 8
    dev = torch.device("cuda:0")
    eng = E.Engine(0)
    L = E.load_library()
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    hr = np.random.default_rng(23)
    widths = [fan, fan * fan, R, R]
    first = np.concatenate([[0], np.cumsum(widths)]).tolist()
    spare = first[-1]          # 8 spare pivot segments of the parent, then 8 spare leaves
    S = spare + 16
    paths = [[first[0] + r // (R // widths[0]), first[1] + r // (R // widths[1]), first[2] + r, first[3] + r]
             for r in range(R)]
    seg_lists = [hr.integers(0, 1024, size=int(hr.integers(1, cap + 1))).tolist() for _ in range(spare)] + [[]] * 16
    caps = np.full(S + 1, cap, dtype=np.uint32)
    pool = sorted({bytes(b) for b in hr.integers(0, 256, size=(R + 64, 24), dtype=np.uint8)})
    bounds = [pool[i] for i in sorted(hr.choice(len(pool), size=R - 1, replace=False))]
    leaf = R // 2 + 5          # the leaf that splits
    room = E.RangeRoom(ranges=R + 64, bound_bytes=24 * (R + 64), path_entries=4 * (R + 64),
                       list_ids=4 * cap * (R + 64), max_list=4 * cap)
    pair_cap = n * 4 * cap
    with torch.cuda.stream(stream):
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        keys = torch.randint(0, 256, (n, 24), device=dev, generator=g, dtype=torch.uint8).contiguous()
        outs = [(torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev),
                 torch.zeros(pair_cap, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
                for _ in range(2)]
        scratch = torch.zeros(E.range_route_scratch_bytes(n) // 8, dtype=torch.int64, device=dev)
    stream.synchronize()

    def route(h, out):
        E._check(L.rf_amd_range_map_route_keys(h, keys.data_ptr(), 24, n, out[0].data_ptr(), out[1].data_ptr(),
                                               out[2].data_ptr(), pair_cap, out[3].data_ptr(), scratch.data_ptr(), st))

    def c_table(bounds, paths, lists):
        """a segmented table in the C create's form, built before anything is timed"""
        Rt = len(paths)
        boff = np.zeros(Rt, dtype=np.uint64)
        np.cumsum(np.array([len(b) for b in bounds], dtype=np.uint64), out=boff[1:])
        path, poff = E._csr(paths, np.uint32)
        ids, soff = E._csr(lists, np.uint32)
        return (Rt, np.frombuffer(b"".join(bounds) + b"\0", dtype=np.uint8), boff, path, poff, ids, soff)

    def create(t, with_room):
        h = ctypes.c_void_p()
        a = (eng.h, t[0], t[1].ctypes.data, t[2].ctypes.data, t[3].ctypes.data, t[4].ctypes.data, S, caps.ctypes.data,
             t[5].ctypes.data, t[6].ctypes.data)
        if with_room:
            E._check(L.rf_amd_range_map_create_segments_room(*a, ctypes.byref(room), ctypes.byref(h)))
        else:
            E._check(L.rf_amd_range_map_create_segments(*a, ctypes.byref(h)))
        return h

    base = c_table(bounds, paths, seg_lists)
    events = {}
    for m in (2, 8):  # the leaf splits into m: m - 1 new boundaries between its own
        lo, hi = bounds[leaf - 1], bounds[leaf]
        span = int.from_bytes(hi, "big") - int.from_bytes(lo, "big")
        nb = [(int.from_bytes(lo, "big") + span * (j + 1) // m).to_bytes(24, "big") for j in range(m - 1)]
        assert lo < nb[0] and nb[-1] < hi and nb == sorted(set(nb))
        new_paths = [paths[leaf][:2] + [spare + j, spare + 8 + j] for j in range(m)]
        lists = list(seg_lists)
        for j in range(m):  # the parent's new pivots start empty; each new leaf receives the old leaf's bundles
            lists[spare + 8 + j] = seg_lists[first[3] + leaf]
        nbounds, npaths = E.range_split_host(bounds, paths, leaf, nb, new_paths)
        sid = np.arange(spare + 8, spare + 8 + m, dtype=np.uint32)
        sids, sidoff = E._csr([lists[s] for s in sid], np.uint32)
        sb = np.frombuffer(b"".join(nb) + b"\0", dtype=np.uint8)
        sboff = (np.arange(m, dtype=np.uint64) * np.uint64(24))
        spath, spoff = E._csr(new_paths, np.uint32)
        events[m] = dict(new=c_table(nbounds, npaths, lists), nbounds=nbounds, npaths=npaths, lists=lists,
                         split=(sid, sids, sidoff, sb, sboff, spath, spoff))

    def way_split(h, m):
        sid, sids, sidoff, sb, sboff, spath, spoff = events[m]["split"]
        E._check(L.rf_amd_range_map_update_segments(h, sid.ctypes.data, sids.ctypes.data, sidoff.ctypes.data, m, st))
        E._check(L.rf_amd_range_map_split(h, leaf, m, sb.ctypes.data, sboff.ctypes.data, spath.ctypes.data,
                                          spoff.ctypes.data, st))

    def way_rebuild(old, m):
        h = create(events[m]["new"], False)
        E._check(L.rf_amd_range_map_destroy_on(old, st))
        return h

    # both ways' route output after the same event, compared before anything is timed
    for m in (2, 8):
        a = create(base, True)
        way_split(a, m)
        b = way_rebuild(create(base, False), m)
        route(a, outs[0])
        route(b, outs[1])
        stream.synchronize()
        tot = int(outs[0][3].item())
        assert L.rf_amd_range_map_num_ranges(a) == R + m - 1 == L.rf_amd_range_map_num_ranges(b)
        assert tot == int(outs[1][3].item()) and torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert torch.equal(outs[0][2][:tot], outs[1][2][:tot]), "the two ways' ids differ"
        sample = hr.choice(n, size=1 << 14, replace=False)
        hk = keys[torch.from_numpy(sample).to(dev)].cpu().numpy()
        flat = E.range_segment_lists(events[m]["npaths"], events[m]["lists"])
        mirror = E.range_route_host(events[m]["nbounds"], flat, [bytes(x) for x in hk])[0]
        assert np.array_equal(mirror, outs[0][0].cpu().numpy().view(np.uint32)[sample]), "ranges differ from the mirror"
        L.rf_amd_range_map_destroy(a)
        L.rf_amd_range_map_destroy(b)

    def timed(fn):
        """(host microseconds until the call returns, microseconds until the stream has drained)"""
        stream.synchronize()
        t0 = time.perf_counter()
        r = fn()
        t1 = time.perf_counter()
        stream.synchronize()
        return (t1 - t0) * 1e6, (time.perf_counter() - t0) * 1e6, r

    def timed_route(h):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        route(h, outs[0])
        b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b)

    def stats(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                "rounds": [round(x, 4) for x in v]}

    out_events = {}
    for m in (2, 8):
        t = {k: [] for k in ("split_host_us", "split_drained_us", "rebuild_host_us", "rebuild_drained_us",
                             "route_roomy_ms", "route_parent_ms")}
        for r in range(args.warmup + args.rounds):
            a = create(base, True)
            old = create(base, False)
            sh, sd, _ = timed(lambda: way_split(a, m))
            rh, rd, b = timed(lambda: way_rebuild(old, m))
            ra, rb = timed_route(a), timed_route(b)  # the same table: a roomy map, and the parent's map
            if r >= args.warmup:
                for name, v in (("split_host_us", sh), ("split_drained_us", sd), ("rebuild_host_us", rh),
                                ("rebuild_drained_us", rd), ("route_roomy_ms", ra), ("route_parent_ms", rb)):
                    t[name].append(v)
            L.rf_amd_range_map_destroy(a)
            L.rf_amd_range_map_destroy(b)
        s = {k: stats(v) for k, v in t.items()}
        spread = s["rebuild_drained_us"]["max"] - s["rebuild_drained_us"]["min"]
        rspread = s["route_parent_ms"]["max"] - s["route_parent_ms"]["min"]
        s["split_below_rebuild_by_more_than_its_spread"] = bool(
            s["split_drained_us"]["median"] < s["rebuild_drained_us"]["median"] - spread)
        s["route_roomy_within_parent_spread"] = bool(
            s["route_roomy_ms"]["median"] <= s["route_parent_ms"]["median"] + rspread)
        s["splice_launches"] = -(-E.range_splice_words([b"x" * 24] * (m - 1), [[0] * 4] * m) // E.diag_range_splice_words())
        out_events["pieces_%d" % m] = s
    out = {
        "what": ("one leaf of a trunk-shaped range map (R leaves, paths of 4 segments, fan-out 16 per level, lists of "
                 "1 to 8 ids, capacity 8) splits into 2 and into 8, two ways on one stream: (split) on a map created "
                 "with room, rf_amd_range_map_update_segments of the new leaves' spare segments, then "
                 "rf_amd_range_map_split; (rebuild) what a map without room needs: rf_amd_range_map_create_segments of "
                 "the new table + rf_amd_range_map_destroy_on of the old map. host_us: wall time until the C calls "
                 "return, their arrays built beforehand; drained_us: wall time from before the calls until the stream, "
                 "idle at the start, has drained. route_*: one rf_amd_range_map_route_keys of n 24-byte keys by HIP "
                 "events on the two maps after the event -- the same table; the route kernels and the roomless map "
                 "are the parent commit's. A fresh pair of maps per round; median, minimum and maximum over the rounds"),
        "config": {"ranges": R, "segments": S, "fan_out": fan, "path_segments": 4, "capacity": cap, "n": n,
                   "key_len": 24, "leaf": leaf, "rounds": args.rounds, "warmup": args.warmup,
                   "splice_words_per_launch": E.diag_range_splice_words()},
        **out_events,
        "verified": ("after each event both ways' route output equal (ranges, offsets, ids, total) over all n keys; "
                     "ranges equal E.range_route_host over the edited model on 2^14 keys"),
        "device": torch.cuda.get_device_name(0),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--filters", type=int, default=64)
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--var", action="store_true", help="variable-length keys (8-100 B)")
    ap.add_argument("--ragged", action="store_true", help="per-key member lists: ragged against padded to K = 16")
    ap.add_argument("--routed", action="store_true",
                    help="route + ragged probe + compaction from raw keys through a range map")
    ap.add_argument("--per-key", dest="per_key", action="store_true",
                    help="rf_amd_found_per_key_ragged against found_compact + searchsorted + gather")
    ap.add_argument("--by-branch", dest="by_branch", action="store_true",
                    help="rf_amd_found_by_branch against torch.sort + gather + unique_consecutive")
    ap.add_argument("--advance", action="store_true",
                    help="rf_amd_found_advance against torch masks + cumsum + repeat_interleave + gather")
    ap.add_argument("--exists", action="store_true",
                    help="rf_amd_filter_set_exists_*_ragged against the ragged probe alone")
    ap.add_argument("--update", action="store_true",
                    help="member updates of a resident set against destroy + create of the whole set")
    ap.add_argument("--segments", action="store_true",
                    help="a segment update of a range map against the rebuild of a flat one")
    ap.add_argument("--split", action="store_true",
                    help="a leaf split on a range map with room against the rebuild of a segmented one")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        name = "multiget" + ("_var" if args.var else "") + ("_ragged" if args.ragged else "") + \
            ("_routed" if args.routed else "") + ("_per_key" if args.per_key else "") + ("_by_branch" if args.by_branch else "") + \
            ("_advance" if args.advance else "") + ("_exists" if args.exists else "") + ".json"
        name = "multiget_update.json" if args.update else "range_segments.json" if args.segments else name
        name = "range_split.json" if args.split else name
        args.out = os.path.join(ROOT, "profiles", name)
    if not torch.cuda.is_available():
        sys.exit("multiget.py measures on the GPU: no HIP device")
    if args.update:
        return update_mode(args)
    if args.segments:
        return segments_mode(args)
    if args.split:
        return split_mode(args)
    F, nk, n, Kf = args.filters, args.keys, args.n, args.k
    assert 1 <= F <= 64, "one value per filter: at most 64 filters"
    dev = torch.device("cuda:0")
    cfg = E.routing_config_init(fingerprint_size=26, log_index_size=8, seed=42)
    eng = E.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    mean_len = 24.0
    if args.var:
        assert n % F == 0 and n // F <= nk, "--var: n a multiple of the filters, at most keys-per-filter each"
        vdata, voffs = K.var_keys(n)
        mean_len = float(voffs[-1]) / n
    with torch.cuda.stream(stream):
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        i = torch.arange(n, device=dev, dtype=torch.int64)
        own = i % F
        hashes = torch.zeros(n, dtype=torch.int32, device=dev)
        batch = E.FilterBatch(cfg, [nk] * F, list(range(F)), engine=eng)  # filter f tags its keys with value f
        if args.var:
            d_bytes = torch.from_numpy(vdata).to(dev)
            d_offs = torch.from_numpy(voffs.view("int64")).to(dev)
            del vdata, voffs
            E.hash_var_keys(cfg, d_bytes, d_offs, n, hashes, stream=st, engine=eng)
            fill = torch.randint(-(1 << 31), 1 << 31, (F, nk), device=dev, generator=g).to(torch.int32)
            fill[:, :n // F] = hashes.view(n // F, F).t()  # filter f: the keys with i % F == f
            batch.build_hashes(fill.contiguous(), stream=st)
            batch.infos(stream=st)
            del fill
        else:
            gid = torch.arange(F, device=dev, dtype=torch.int64)[:, None] << 32
            j = torch.arange(nk, device=dev, dtype=torch.int64)[None, :]
            batch.build_keys(K.ids_keys_torch((gid + j).reshape(-1), 24), 24, stream=st)
            batch.infos(stream=st)
            del gid, j
            ids = (own << 32) + torch.randint(0, nk, (n,), device=dev, generator=g)
            keys = K.ids_keys_torch(ids, 24)
            del ids
        member = torch.randint(0, F, (n, Kf), device=dev, generator=g).to(torch.int32).contiguous()
        del i
        fset = E.FilterSet([(batch, f) for f in range(F)], engine=eng)
        found_a = torch.zeros(n * Kf, dtype=torch.int64, device=dev)
        found_b = torch.zeros(n * Kf, dtype=torch.int64, device=dev)
        hashes.zero_()
        d_count = torch.zeros(1, dtype=torch.int64, device=dev)
    stream.synchronize()

    def fanout():
        if args.var:
            fset.probe_var_keys(d_bytes, d_offs, member, Kf, n, found_a, stream=st)
        else:
            fset.probe_keys(keys, 24, member, Kf, n, found_a, stream=st)

    def replicate():
        if args.var:
            E.hash_var_keys(cfg, d_bytes, d_offs, n, hashes, stream=st, engine=eng)
        else:
            E.hash_keys(cfg, keys, 24, n, hashes, stream=st, engine=eng)
        rep = torch.repeat_interleave(hashes, Kf)
        batch.probe_hashes(rep, member, n * Kf, found_b, stream=st)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            fn()
            b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b)

    def rng(v):
        return {"min": round(min(v), 4), "max": round(max(v), 4), "rounds": [round(x, 4) for x in v]}

    if args.ragged or args.routed or args.per_key or args.exists or args.by_branch or args.advance:
        del found_a, found_b, member
        kin = (d_bytes, d_offs) if args.var else (keys, 24)
        if args.advance:
            out = advance(args, fset, eng, stream, kin, own, timed, rng)
        elif args.by_branch:
            out = by_branch(args, fset, eng, stream, kin, own, timed, rng)
        elif args.exists:
            out = exists(args, fset, eng, stream, kin, timed, rng)
        elif args.per_key:
            out = per_key(args, fset, eng, stream, kin, timed, rng)
        elif args.routed:
            out = routed(args, fset, eng, stream, kin, timed, rng)
        else:
            out = ragged(args, fset, eng, stream, kin, own, mean_len, timed, rng)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
        print(json.dumps(out))
        fset.close()
        batch.close()
        eng.close()
        return

    t = {"fanout": [], "replicate": []}
    for r in range(args.warmup + args.rounds):
        for way, fn in (("fanout", fanout), ("replicate", replicate)):
            ms = timed(fn)
            if r >= args.warmup:
                t[way].append(ms)
    assert torch.equal(found_a, found_b), "the two ways disagree"
    hits = int(((found_a.view(n, Kf) >> member.to(torch.int64)) & 1)[member.to(torch.int64) == own[:, None]].sum())
    assert hits == int((member.to(torch.int64) == own[:, None]).sum()), "false negative"

    # compaction: count first, then the timed rounds at cap = count
    with torch.cuda.stream(stream):
        E.found_compact(found_a, n * Kf, None, d_count, stream=st, engine=eng)
    stream.synchronize()
    count = int(d_count.item())
    with torch.cuda.stream(stream):
        d_cand = torch.zeros(max(count, 1), dtype=torch.int64, device=dev)
    t_compact = []
    for r in range(args.warmup + args.rounds):
        ms = timed(lambda: E.found_compact(found_a, n * Kf, d_cand, d_count, stream=st, engine=eng))
        if r >= args.warmup:
            t_compact.append(ms)
    assert int(d_count.item()) == count

    # read-back into pinned memory: the dense words against the candidate list
    h_dense = torch.empty(n * Kf, dtype=torch.int64, pin_memory=True)
    h_cand = torch.empty(max(count, 1), dtype=torch.int64, pin_memory=True)
    t_dense, t_cand = [], []
    for r in range(args.warmup + args.rounds):
        a = timed(lambda: h_dense.copy_(found_a, non_blocking=True))
        b = timed(lambda: h_cand.copy_(d_cand, non_blocking=True))
        if r >= args.warmup:
            t_dense.append(a)
            t_cand.append(b)

    fa, rb = t["fanout"], t["replicate"]
    what = ("multi-get of n 24-byte keys, K random members per key, one batch of F filters: "
            "FilterSet.probe_keys against hash_keys + repeat_interleave + probe_hashes with per-probe "
            "filter ids; alternating rounds in one process, HIP events on the launch stream")
    config = {"filters": F, "keys_per_filter": nk, "n": n, "K": Kf, "rounds": args.rounds,
              "warmup": args.warmup, "fingerprint_size": 26, "log_index_size": 8}
    if args.var:
        what = ("multi-get of n variable-length keys (keys.var_keys, 8-100 B), K random members per key, one "
                "batch of F filters: FilterSet.probe_var_keys against hash_var_keys + repeat_interleave + "
                "probe_hashes with per-probe filter ids; alternating rounds in one process, HIP events on the "
                "launch stream")
        config["mean_key_len"] = round(mean_len, 3)
    out = {
        "what": what,
        "config": config,
        "fanout_ms": rng(fa),
        "replicate_ms": rng(rb),
        "ranges_touch": not (max(fa) < min(rb) or max(rb) < min(fa)),
        "fanout_faster_beyond_ranges": bool(max(fa) < min(rb)),
        "fanout_slower_beyond_ranges": bool(max(rb) < min(fa)),
        # the key (--var: its mean length and 8 bytes of offset), then per member an id, a line, a word
        "fanout_algorithmic_bytes_per_key": (round(mean_len + 8, 3) if args.var else 24) + Kf * (4 + 64 + 8),
        "compact_ms": rng(t_compact),
        "candidates": count,
        "dense_bytes": n * Kf * 8,
        "candidate_bytes": count * 8,
        "d2h_dense_ms": rng(t_dense),
        "d2h_candidates_ms": rng(t_cand),
        "verified": "both ways' n K words equal; every (key, own filter) pair found",
        "device": torch.cuda.get_device_name(0),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    fset.close()
    batch.close()
    eng.close()


if __name__ == "__main__":
    main()
