"""Cost of CORRELATION(x, y) against STDDEV_SAMPLE(x) and AVG(x) on the same stream (DESIGN.md
"CORRELATION aggregate").

One process, device batches: the seeded stream of tools/stddev_bench.py with a second column (x and y
with 1 % NULL each, TUMBLING 5 s, grace 1 s, 2^24 records per push over ~1e6 keys, 10 s of event time
per push with a 500 ms disorder) through six handles, alternated push by push:
    avg64 / std64 / corr64      AVG(x) / STDDEV_SAMPLE(x) / CORRELATION(x, y), x and y BIGINT
    avg32 / std32 / corr32      the same, INT
Prints the median wall time of the timed pushes, each ended by khip_agg_sync, one JSON line.
    python tools/correlation_bench.py [--pushes 20] [--warmup 3] [--only corr64]
--only runs one handle (for a rocprofv3 --kernel-trace --stats run of its kernels).

    python tools/correlation_bench.py --ab parent --query topk3|sum|tsum [--atomic] [--repeats 6]
compares two builds of the library on a query both know: ksql_amd/libksqldb_hip_parent.so (a build
of the parent commit kept beside the library) against the library itself, alternated push by push
in this process, `repeats` rounds; per build the median of every round, and their min - max.
topk3: TOPK(x, 3) through k_part_agg; sum --atomic: SUM(x) through k_apply; tsum: SUM(x) of a table
source (khip_agg_push_table, host batches of 2^20 changes over 2^18 PRIMARY KEYs and 4096 groups)
through k_tagg_apply.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ksql_amd import abi  # noqa: E402

QUERIES = {"avg64": (("AVG", 0), "INT64"), "std64": (("STDDEV_SAMPLE", 0), "INT64"), "corr64": (("CORRELATION", 0, 1), "INT64"),
           "avg32": (("AVG", 0), "INT32"), "std32": (("STDDEV_SAMPLE", 0), "INT32"), "corr32": (("CORRELATION", 0, 1), "INT32")}
AB_QUERIES = {"topk3": [("TOPK", 0, 3)], "sum": [("SUM", 0)], "tsum": [("SUM", 0)]}


def column(g, n, typ):
    if typ == "INT64":
        return torch.randint(-2**62, 2**62, (n,), generator=g, device="cuda", dtype=torch.int64)
    return torch.randint(-2**31, 2**31, (n,), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)


def batch(step, n, keys, typ, span_ms=10_000, disorder_ms=500):
    g = torch.Generator(device="cuda")
    g.manual_seed(1234 + step)
    key = torch.randint(0, keys, (n,), generator=g, device="cuda", dtype=torch.int64)
    ts = step * span_ms + (torch.arange(n, device="cuda", dtype=torch.int64) * span_ms) // n + \
        torch.randint(0, disorder_ms, (n,), generator=g, device="cuda", dtype=torch.int64)
    cols = [column(g, n, typ), column(g, n, typ)]
    valid = [abi.bitmap_torch(torch.rand(n, generator=g, device="cuda") >= 0.01) for _ in cols]
    return abi.DeviceBatch(ts, keys=key, cols=cols, col_valid=valid)


def desc(typ, aggs, flags=0):
    return abi.make_agg_desc(window_kind="TUMBLING", size_ms=5000, grace_ms=1000, col_types=[typ, typ], aggs=aggs,
                             capacity_hint=8_000_000, flags=abi.FLAG_PROFILE | flags)


def timed_push(lib, h, b):
    t0 = time.perf_counter()
    h.push(b, stats=False)
    lib.check(lib.agg_sync(h.h), "agg_sync")
    return 1e3 * (time.perf_counter() - t0)


def table_batch(step, n):
    rng = np.random.default_rng(4321 + step)
    pk = rng.integers(0, 1 << 18, n)
    return (abi.HostBatch(np.arange(n, dtype=np.int64) + step * n, keys=pk % 4096, row_valid=rng.random(n) > 0.05,
                          cols=[rng.integers(-2**62, 2**62, n)], col_valid=[rng.random(n) > 0.01]), pk)


def timed_push_table(lib, h, b):
    t0 = time.perf_counter()
    h.push_table(b[0], src_keys=b[1], stats=False)
    lib.check(lib.agg_sync(h.h), "agg_sync")
    return 1e3 * (time.perf_counter() - t0)


def run_ab(args):
    libs = {"parent": abi.Lib(os.path.join(abi.REPO, "ksql_amd", "libksqldb_hip_%s.so" % args.ab), "khip_", True),
            "this": abi.load_product()}
    table = args.query == "tsum"
    flags = abi.FLAG_ENGINE_ATOMIC if args.atomic else 0
    names = list(libs)
    medians = {q: [] for q in names}
    step = 0
    for _ in range(args.repeats):
        if table:
            handles = {q: abi.AggHandle(libs[q], abi.make_agg_desc("NONE", "INT64", col_types=["INT64"], aggs=AB_QUERIES["tsum"],
                                                                   flags=abi.FLAG_TABLE_SOURCE)) for q in names}
        else:
            handles = {q: abi.AggHandle(libs[q], desc("INT64", AB_QUERIES[args.query], flags)) for q in names}
        times = {q: [] for q in names}
        for i in range(args.warmup + args.pushes):
            b = table_batch(step, 1 << 20) if table else batch(step, args.records, args.keys, "INT64")
            step += 1
            torch.cuda.synchronize()
            for q in names[i % 2:] + names[:i % 2]:
                t = timed_push_table(libs[q], handles[q], b) if table else timed_push(libs[q], handles[q], b)
                if i >= args.warmup:
                    times[q].append(t)
        for q in names:
            medians[q].append(round(statistics.median(times[q]), 3))
            handles[q].close()
    out = {"query": args.query, "engine": "table" if table else ("atomic" if args.atomic else "partitioned"),
           "records_per_push": 1 << 20 if table else args.records, "pushes": args.pushes, "repeats": args.repeats}
    for q in names:
        out[q] = {"round_medians_ms": medians[q], "min_ms": min(medians[q]), "max_ms": max(medians[q]),
                  "median_ms": statistics.median(medians[q])}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--records", type=int, default=1 << 24)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--only", choices=list(QUERIES))
    ap.add_argument("--ab")
    ap.add_argument("--query", choices=list(AB_QUERIES), default="topk3")
    ap.add_argument("--atomic", action="store_true")
    ap.add_argument("--repeats", type=int, default=6)
    args = ap.parse_args()
    torch.cuda.init()
    if args.ab:
        return run_ab(args)
    lib = abi.load_product()
    names = [args.only] if args.only else list(QUERIES)
    handles = {q: abi.AggHandle(lib, desc(QUERIES[q][1], [QUERIES[q][0]])) for q in names}
    times = {q: [] for q in names}
    for step in range(args.warmup + args.pushes):
        b = {t: batch(step, args.records, args.keys, t) for t in {QUERIES[q][1] for q in names}}
        torch.cuda.synchronize()
        for q in names[step % len(names):] + names[:step % len(names)]:  # alternate who goes first
            t = timed_push(lib, handles[q], b[QUERIES[q][1]])
            if step >= args.warmup:
                times[q].append(t)
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
