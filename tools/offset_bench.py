"""Cost of the offset aggregates against MAX on the same stream (DESIGN.md (d) "Offset aggregates").

One process, device batches: the same seeded stream (BIGINT x, 1 % NULL, TUMBLING 5 s, grace 1 s,
2^24 records per push over ~1e6 keys, 10 s of event time per push with a 500 ms disorder: the
value pipeline's shape) through three handles, alternated push by push:
    MAX(x)                  the yardstick (the same engine path, no hidden column, no resolve)
    LATEST_BY_OFFSET(x)     + the sequence iota (8 B written, 8 B read per record) + the resolve
    EARLIEST_BY_OFFSET(x)
Prints the median wall time of the timed pushes, each ended by khip_agg_sync, one JSON line.
    python tools/offset_bench.py [--pushes 20] [--warmup 3] [--only latest]
--only runs one handle (for a rocprofv3 --kernel-trace --stats run of its kernels).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ksql_amd import abi  # noqa: E402

QUERIES = {"max": "MAX", "latest": "LATEST_BY_OFFSET", "earliest": "EARLIEST_BY_OFFSET"}


def batch(step, n, keys, span_ms=10_000, disorder_ms=500):
    g = torch.Generator(device="cuda")
    g.manual_seed(1234 + step)
    key = torch.randint(0, keys, (n,), generator=g, device="cuda", dtype=torch.int64)
    ts = step * span_ms + (torch.arange(n, device="cuda", dtype=torch.int64) * span_ms) // n + \
        torch.randint(0, disorder_ms, (n,), generator=g, device="cuda", dtype=torch.int64)
    x = torch.randint(-2**62, 2**62, (n,), generator=g, device="cuda", dtype=torch.int64)
    valid = abi.bitmap_torch(torch.rand(n, generator=g, device="cuda") >= 0.01)
    return abi.DeviceBatch(ts, keys=key, cols=[x], col_valid=[valid])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--records", type=int, default=1 << 24)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--only", choices=list(QUERIES))
    args = ap.parse_args()
    torch.cuda.init()
    lib = abi.load_product()
    names = [args.only] if args.only else list(QUERIES)
    handles = {q: abi.AggHandle(lib, abi.make_agg_desc(window_kind="TUMBLING", size_ms=5000, grace_ms=1000,
                                                        col_types=["INT64"], aggs=[(QUERIES[q], 0)],
                                                        capacity_hint=8_000_000, flags=abi.FLAG_PROFILE))
               for q in names}
    times = {q: [] for q in names}
    for step in range(args.warmup + args.pushes):
        b = batch(step, args.records, args.keys)
        torch.cuda.synchronize()
        order = names[step % len(names):] + names[:step % len(names)]  # alternate who goes first
        for q in order:
            h = handles[q]
            t0 = time.perf_counter()
            h.push(b, stats=False)
            lib.check(lib.agg_sync(h.h), "agg_sync")
            if step >= args.warmup:
                times[q].append(1e3 * (time.perf_counter() - t0))
    out = {"records_per_push": args.records, "keys": args.keys, "pushes": args.pushes}
    for q in names:
        kt = handles[q].kernel_times()
        out[q] = {"median_ms": round(statistics.median(times[q]), 3), "min_ms": round(min(times[q]), 3),
                  "max_ms": round(max(times[q]), 3), "pipeline_pushes": kt["c1_pushes"], "declined": kt["c1_declined"],
                  "groups": handles[q].snapshot_size()}
        handles[q].close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
