#!/usr/bin/env python3
"""Compaction chain, two ways, in one process: the k incremental builds of today against one
fused build of the same keys (FilterBatch.chained).

Shape: bench.py's compaction workload -- 64 filters x 8 runs x (2^20-1) keys, run v of filter
f holding the ids (f << 32) + (v + 1) j under value v. A chain step is bench.py's: 8 rounds of
create + incremental build + stream-ordered release of the superseded batch + the round's
descriptors (rf_amd_batch_infos on the build stream, which is also what lets the pool hand
the released blocks to the next round); a fused step is one create + build + descriptors.
Both end in a stream synchronisation inside the host clock's window. Steps of
the two alternate, so drift of the machine hits both alike. Reported: the median of each over
the timed steps, every step's time, the spread (max - min), the ratio of the medians and the
per-stage event times of one fused build (outside the timed steps). The final filters of both
ways are compared byte for byte before anything is reported.

    python tools/fused_chain.py [--filters 64] [--rounds 8] [--keys 1048575] [--steps 7]
                                [--warmup 2] [--out profiles/fused_chain.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from splinterdb_amd import engine as E  # noqa: E402
from splinterdb_amd import keys as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--filters", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--keys", type=int, default=(1 << 20) - 1)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log-index-size", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_chain.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fused_chain.py measures on the GPU: no HIP device")
    F, V, n = args.filters, args.rounds, args.keys
    dev = torch.device("cuda:0")
    cfg = E.routing_config_init(fingerprint_size=26, log_index_size=args.log_index_size, seed=42)
    eng = E.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    with torch.cuda.stream(stream):
        gid = torch.arange(F, device=dev, dtype=torch.int64)[:, None] << 32
        j = torch.arange(n, device=dev, dtype=torch.int64)[None, :]
        # the chain's input: per round, filter-major; the fused build's: filter-major, run-minor
        keys_round = [K.ids_keys_torch((gid + (v + 1) * j).reshape(-1), 24) for v in range(V)]
        keys_fused = torch.stack([k.view(F, n, 24) for k in keys_round], dim=1).contiguous().view(-1, 24)
        del gid, j
    stream.synchronize()
    runs = [[(n, v) for v in range(V)]] * F

    def chain():
        prev = None
        for v in range(V):
            b = E.FilterBatch(cfg, [n] * F, [v] * F, old=[(prev, f) for f in range(F)] if prev else None,
                              engine=eng)
            b.build_keys(keys_round[v], 24, stream=st)
            if prev is not None:
                prev.close(stream=st)
            b.infos(stream=st)
            prev = b
        stream.synchronize()
        return prev

    def fused(timing=False):
        b = E.FilterBatch.chained(cfg, runs, engine=eng)
        if timing:
            b.set_timing(True)
        b.build_keys(keys_fused, 24, stream=st)
        b.infos(stream=st)
        stream.synchronize()
        return b

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b = fn()
        return b, (time.perf_counter() - t0) * 1e3

    t_chain, t_fused = [], []
    last_c = last_f = None
    for k in range(args.warmup + args.steps):
        for way in ("chain", "fused"):
            b, ms = timed(chain if way == "chain" else fused)
            if k >= args.warmup:
                (t_chain if way == "chain" else t_fused).append(ms)
            keep = k + 1 == args.warmup + args.steps
            if keep and way == "chain":
                last_c = b
            elif keep:
                last_f = b
            else:
                b.close(stream=st)

    # same filters both ways (descriptor fields and every image byte)
    ic, jf = last_c.infos(stream=st), last_f.infos(stream=st)
    for f in range(F):
        a, b = ic[f], jf[f]
        assert (a.num_fingerprints, a.num_unique, a.value_size, a.num_pages, a.error) == \
            (b.num_fingerprints, b.num_unique, b.value_size, b.num_pages, b.error), f
    for f in sorted({0, F // 2, F - 1}):
        x, y = last_c.image(f), last_f.image(f)
        assert (x.pages == y.pages).all() and (x.slots == y.slots).all(), f
    num_unique0 = int(ic[0].num_unique)
    last_c.close()
    last_f.close()

    bt = fused(timing=True)
    stages = bt.timings(0)
    bt.close()

    mc, mf = statistics.median(t_chain), statistics.median(t_fused)
    sc, sf = max(t_chain) - min(t_chain), max(t_fused) - min(t_fused)
    keys_total = F * V * n
    out = {
        "what": "compaction chain of k incremental builds vs one fused build of the same keys, one process, "
                "alternating steps; host clock around work ending in a stream synchronisation; the chain is "
                "bench.py --workload compaction's (create + incremental build + release + infos per round)",
        "config": {"filters": F, "rounds": V, "keys_per_round": n, "fingerprint_size": 26,
                   "log_index_size": args.log_index_size, "steps": args.steps, "warmup": args.warmup},
        "chain_ms": {"median": round(mc, 3), "min": round(min(t_chain), 3), "max": round(max(t_chain), 3),
                     "spread": round(sc, 3), "steps": [round(x, 3) for x in t_chain]},
        "fused_ms": {"median": round(mf, 3), "min": round(min(t_fused), 3), "max": round(max(t_fused), 3),
                     "spread": round(sf, 3), "steps": [round(x, 3) for x in t_fused]},
        "chain_mkeys_s": round(keys_total / mc / 1e3, 1),
        "fused_mkeys_s": round(keys_total / mf / 1e3, 1),
        "ratio_chain_over_fused": round(mc / mf, 3),
        "fused_faster_beyond_spread": bool(mc - mf > max(sc, sf)),
        "fused_stage_ms": {k: round(v, 4) for k, v in stages.items() if k != "probe"},
        "verified": "descriptors of all filters and images of filters 0, F/2, F-1 equal both ways",
        "num_unique_filter0": num_unique0,
        "device": torch.cuda.get_device_name(0),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
