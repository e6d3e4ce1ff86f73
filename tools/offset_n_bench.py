"""Cost of the N forms of LATEST_BY_OFFSET / EARLIEST_BY_OFFSET (DESIGN.md (d) "Offset aggregates,
N forms") against TOPK, scalar LATEST and MAX on the same stream.

One process on the tuning build (KSQL_AMD_LIB_VARIANT=tune is set here when unset), device batches:
offset_bench.py's stream (BIGINT x, 1 % NULL, TUMBLING 5 s, grace 1 s, 2^24 records per push over
~1e6 keys, 10 s of event time per push with a 500 ms disorder) through eleven handles, alternated
push by push:
    latestN / earliestN     LATEST_BY_OFFSET(x, N) / EARLIEST_BY_OFFSET(x, N), N = 1, 3, 8: k_part_agg
                            with the TOPK chain over the hidden (complemented) sequence column, then
                            the resolve
    topkN                   TOPK(x, N), N = 1, 3, 8: the same chain on the same kernel without a
                            resolve: what the resolve (and the iota) costs is latestN - topkN
    latest                  the scalar LATEST_BY_OFFSET(x) on its default path (the value pipeline):
                            what the N forms lose by having no merge / pipeline form
    max_agg                 MAX(x) forced onto k_part_agg (KHIP_MERGE=0 around its pushes)
Prints the median wall time of the timed pushes, each ended by khip_agg_sync, one JSON line.
    python tools/offset_n_bench.py [--pushes 20] [--warmup 3] [--only latest3]
--only runs one handle (for a rocprofv3 --kernel-trace --stats run of its kernels).
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("KSQL_AMD_LIB_VARIANT", "tune")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ksql_amd import abi  # noqa: E402
from offset_bench import batch  # noqa: E402

QUERIES = {"max_agg": ("MAX", 0), "latest": ("LATEST_BY_OFFSET", 0)}
for _n in (1, 3, 8):
    QUERIES["topk%d" % _n] = ("TOPK", 0, _n)
    QUERIES["latest%d" % _n] = ("LATEST_BY_OFFSET", 0, _n)
    QUERIES["earliest%d" % _n] = ("EARLIEST_BY_OFFSET", 0, _n)


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
    assert lib.path.endswith("libksqldb_hip_tune.so"), lib.path  # (max_agg needs the KHIP_MERGE knob)
    names = [args.only] if args.only else list(QUERIES)
    handles = {q: abi.AggHandle(lib, abi.make_agg_desc(window_kind="TUMBLING", size_ms=5000, grace_ms=1000,
                                                        col_types=["INT64"], aggs=[QUERIES[q]],
                                                        capacity_hint=8_000_000, flags=abi.FLAG_PROFILE))
               for q in names}
    times = {q: [] for q in names}
    for step in range(args.warmup + args.pushes):
        b = batch(step, args.records, args.keys)
        torch.cuda.synchronize()
        order = names[step % len(names):] + names[:step % len(names)]  # alternate who goes first
        for q in order:
            h = handles[q]
            if q == "max_agg":
                os.environ["KHIP_MERGE"] = "0"
            t0 = time.perf_counter()
            h.push(b, stats=False)
            lib.check(lib.agg_sync(h.h), "agg_sync")
            if step >= args.warmup:
                times[q].append(1e3 * (time.perf_counter() - t0))
            os.environ.pop("KHIP_MERGE", None)
    out = {"records_per_push": args.records, "keys": args.keys, "pushes": args.pushes, "library": os.path.basename(lib.path)}
    for q in names:
        kt = handles[q].kernel_times()
        out[q] = {"median_ms": round(statistics.median(times[q]), 3), "min_ms": round(min(times[q]), 3),
                  "max_ms": round(max(times[q]), 3), "pipeline_pushes": kt["c1_pushes"], "declined": kt["c1_declined"],
                  "groups": handles[q].snapshot_size()}
        handles[q].close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
