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

    timeout -k 10 600 python tools/multiget.py [--var] [--filters 64] [--keys 1048576]
                                               [--n 16777216] [--k 4] [--rounds 7] [--warmup 2]
                                               [--out profiles/multiget.json]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--filters", type=int, default=64)
    ap.add_argument("--keys", type=int, default=1 << 20)
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--var", action="store_true", help="variable-length keys (8-100 B)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "multiget_var.json" if args.var else "multiget.json")
    if not torch.cuda.is_available():
        sys.exit("multiget.py measures on the GPU: no HIP device")
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

    def rng(v):
        return {"min": round(min(v), 4), "max": round(max(v), 4), "rounds": [round(x, 4) for x in v]}

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
