"""Throughput of ARRAY value columns in the sink against the scalar row of bench.py's sink_json leg
(DESIGN.md (d) "Sink serializers", ARRAY columns).

One process, device rows to device record bytes (khip_sink_encode), sink_json's key (a KAFKA BIGINT
key and the 8-byte TUMBLING window start) and its row count (22M by default):
    scalar          {"KSQL_COL_0":n}             the yardstick: sink_json's own value, k_sink_write<TextEnc>
    arr1 / 3 / 8    {"KSQL_COL_0":[n,...]}       BIGINT lists of L = 1, 3 and 8, all full, k_sink_write_arr<TextEnc>
Every element is drawn as sink_json draws its count (1..30), so a list's bytes differ from the
scalar's by the brackets, the commas and the further elements only.  The handles are alternated
step by step; a step is one khip_sink_encode, which returns after the device has finished.  Prints
one JSON line: per handle the median / min / max ms per step, rows/s, output GB/s (key and value
bytes written over the median) and, for the lists, that figure as a fraction of the scalar's.
    python tools/sink_array_bench.py [--steps 10] [--warmup 2] [--records 22000000] [--only arr3]
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

CONFIGS = {"scalar": 0, "arr1": 1, "arr3": 3, "arr8": 8}


class Leg:
    def __init__(self, lib, L, n, h0, key, ws, we):
        C = abi.C
        self.n = n
        slots = max(L, 1)
        # element e of a row: sink_json's count with the hash rotated by e
        self.val = torch.stack([(((h0 >> (40 - 3 * e)) % 30) + 1).to(torch.int64) for e in range(slots)], dim=1).contiguous()
        self.nul = torch.zeros(n * slots, dtype=torch.uint8, device="cuda")
        col = ("KSQL_COL_0", "INT64", 0) + ((L,) if L else ())
        self.sink = abi.SinkHandle(lib, "KAFKA", [("CARD_NUMBER", "INT64")], "JSON", [col], window_kind="TUMBLING")
        self.rows = abi.SinkRows()
        self.rows.n_rows, self.rows.mem, self.rows.key_serialized = n, abi.MEM_DEVICE, 0
        self.rows.key_i64, self.rows.window_start, self.rows.window_end = key.data_ptr(), ws.data_ptr(), we.data_ptr()
        self._cd = (C.c_void_p * 1)(self.val.data_ptr())
        self._cn = (C.c_void_p * 1)(self.nul.data_ptr())
        self.rows.col_data, self.rows.col_null = self._cd, self._cn
        kcap, vcap = 16 * n, (20 + 3 * slots) * n
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
        return bytes(self.bufs[3][voff[0]:voff[1]].cpu().tolist()).decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--records", type=int, default=22_000_000)
    ap.add_argument("--only", choices=list(CONFIGS))
    args = ap.parse_args()
    torch.cuda.init()
    lib = abi.load_product()
    n = args.records
    h0 = synth._stream(synth.backend("torch"), 8, 0, n, "cuda")
    key = (h0 % 10_000_000).to(torch.int64)
    ws = ((h0 >> 24) % 3).to(torch.int64) * 5000
    we = ws + 5000
    names = [args.only] if args.only else list(CONFIGS)
    legs = {q: Leg(lib, CONFIGS[q], n, h0, key, ws, we) for q in names}
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
        out[q] = {"median_ms": round(med, 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3),
                  "rows_per_s": round(n / med * 1e3), "value_bytes_per_row": round(vl / n, 3),
                  "output_GBps": round((kl + vl) / med / 1e6, 2), "output_GBps_min": round((kl + vl) / max(t) / 1e6, 2),
                  "output_GBps_max": round((kl + vl) / min(t) / 1e6, 2), "first_value": legs[q].first_value()}
    if "scalar" in out:
        for q in names:
            if q != "scalar":
                out[q]["output_vs_scalar"] = round(out[q]["output_GBps"] / out["scalar"]["output_GBps"], 3)
    for leg in legs.values():
        leg.sink.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
