"""Throughput of the sink's AVRO value format against its JSON value format, on the same rows and the
same build (DESIGN.md (d) "Sink serializers", AVRO values).

One process, device rows to device record bytes (khip_sink_encode), bench.py's sink_json shape: a
KAFKA BIGINT key and the 8-byte TUMBLING window start, 22M rows by default.  Each case is encoded
as JSON and as AVRO:
    count     one BIGINT column, sink_json's count (1..30)          {"KSQL_COL_0":n}
    three     a BIGINT count, an INT and a DOUBLE column            {"KSQL_COL_0":n,"KSQL_COL_1":i,"KSQL_COL_2":d}
    arr10     one BIGINT list of L = 10, all full                   {"KSQL_COL_0":[n,...]}
The handles are alternated step by step; a step is one khip_sink_encode, which returns after the
device has finished.  Prints one JSON line: per handle the median / min / max ms per step, rows/s,
value bytes per row and output GB/s (key and value bytes written over the median), and per case the
AVRO median over the JSON median.
    python tools/sink_avro_bench.py [--steps 10] [--warmup 2] [--records 22000000] [--only avro_count]
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

from ksql_amd import abi, synth  # noqa: E402

CASES = ("count", "three", "arr10")
CONFIGS = ["%s_%s" % (f, c) for c in CASES for f in ("json", "avro")]
VALUE_CAP = {"count": 24, "three": 96, "arr10": 64}  # value bytes per row, at most (either format)


def columns(case, h0):
    """[(sink column, device values)] of a case; every element is drawn from the stream's hash."""
    count = lambda e: (((h0 >> (40 - 3 * e)) % 30) + 1).to(torch.int64)
    if case == "count":
        return [(("KSQL_COL_0", "INT64", 0), count(0))]
    if case == "three":
        return [(("KSQL_COL_0", "INT64", 0), count(0)),
                (("KSQL_COL_1", "INT32", 1), (((h0 >> 8) % 100_000) - 50_000).to(torch.int32)),
                (("KSQL_COL_2", "DOUBLE", 2), ((h0 >> 4) % 10_000_000).to(torch.float64) / 100.0)]
    return [(("KSQL_COL_0", "INT64", 0, 10), torch.stack([count(e) for e in range(10)], dim=1).contiguous())]


class Leg:
    def __init__(self, lib, fmt, case, n, cols, key, ws, we):
        C = abi.C
        self.vals = [v for _, v in cols]
        self.nuls = [torch.zeros(v.numel(), dtype=torch.uint8, device="cuda") for v in self.vals]
        self.sink = abi.SinkHandle(lib, "KAFKA", [("CARD_NUMBER", "INT64")], fmt.upper(), [c for c, _ in cols],
                                   window_kind="TUMBLING", avro_schema_id=1 if fmt == "avro" else None)
        self.rows = abi.SinkRows()
        self.rows.n_rows, self.rows.mem, self.rows.key_serialized = n, abi.MEM_DEVICE, 0
        self.rows.key_i64, self.rows.window_start, self.rows.window_end = key.data_ptr(), ws.data_ptr(), we.data_ptr()
        self._cd = (C.c_void_p * len(cols))(*[v.data_ptr() for v in self.vals])
        self._cn = (C.c_void_p * len(cols))(*[v.data_ptr() for v in self.nuls])
        self.rows.col_data, self.rows.col_null = self._cd, self._cn
        kcap, vcap = 16 * n, VALUE_CAP[case] * n
        self.bufs = [torch.empty(n + 1, dtype=torch.int64, device="cuda"), torch.empty(n + 1, dtype=torch.int64, device="cuda"),
                     torch.empty(kcap, dtype=torch.uint8, device="cuda"), torch.empty(vcap, dtype=torch.uint8, device="cuda"),
                     torch.empty(n, dtype=torch.uint8, device="cuda")]
        self.out = abi.SinkOut()
        self.out.mem, self.out.key_capacity, self.out.value_capacity = abi.MEM_DEVICE, kcap, vcap
        self.out.key_offsets, self.out.value_offsets = self.bufs[0].data_ptr(), self.bufs[1].data_ptr()
        self.out.key_bytes, self.out.value_bytes = self.bufs[2].data_ptr(), self.bufs[3].data_ptr()
        self.out.value_null = self.bufs[4].data_ptr()
        self.lib = lib
        self.times = []

    def step(self):
        self.lib.check(self.lib.sink_encode(self.sink.h, abi.C.byref(self.rows), abi.C.byref(self.out)), "sink_encode")
        return self.out.key_len, self.out.value_len

    def first_value(self):
        voff = self.bufs[1][:2].cpu().tolist()
        return bytes(self.bufs[3][voff[0]:voff[1]].cpu().tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--records", type=int, default=22_000_000)
    ap.add_argument("--only", choices=CONFIGS)
    args = ap.parse_args()
    torch.cuda.init()
    lib = abi.load_product()
    n = args.records
    h0 = synth._stream(synth.backend("torch"), 8, 0, n, "cuda")
    key = (h0 % 10_000_000).to(torch.int64)
    ws = ((h0 >> 24) % 3).to(torch.int64) * 5000
    we = ws + 5000
    names = [args.only] if args.only else CONFIGS
    cols = {c: columns(c, h0) for c in CASES if any(q.endswith("_" + c) for q in names)}
    legs = {q: Leg(lib, q.split("_")[0], q.split("_")[1], n, cols[q.split("_")[1]], key, ws, we) for q in names}
    torch.cuda.synchronize()
    lens = {}
    for step in range(args.warmup + args.steps):
        for q in names[step % len(names):] + names[:step % len(names)]:  # alternate who goes first
            t0 = time.perf_counter()
            lens[q] = legs[q].step()
            if step >= args.warmup:
                legs[q].times.append(1e3 * (time.perf_counter() - t0))
    out = {"rows": n, "steps": args.steps, "library": os.path.basename(lib.path)}
    for q in names:
        t, (kl, vl) = legs[q].times, lens[q]
        assert kl == 16 * n, kl
        med = statistics.median(t)
        first = legs[q].first_value()
        out[q] = {"median_ms": round(med, 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3),
                  "rows_per_s": round(n / med * 1e3), "value_bytes_per_row": round(vl / n, 3),
                  "output_GBps": round((kl + vl) / med / 1e6, 2),
                  "first_value": first.decode() if q.startswith("json") else first.hex()}
    for c in CASES:
        if "json_" + c in out and "avro_" + c in out:
            out["avro_over_json_" + c] = round(out["avro_" + c]["median_ms"] / out["json_" + c]["median_ms"], 3)
    for leg in legs.values():
        leg.sink.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
