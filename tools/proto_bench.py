"""PROTOBUF against AVRO on the same records and rows, on one build (DESIGN.md "PROTOBUF values";
results in profiles/protobuf/README.md).

Four timings, device-resident inputs and outputs:
    decode_avro    bench.py's serde_avro records: KAFKA BIGINT key, {AMOUNT: long} in the Confluent AVRO
                   wire format (10 value bytes)
    decode_proto   the same amounts as PROTOBUF: framing (6 bytes), tag 0x08, a 5-byte varint (12 bytes)
    encode_avro    bench.py's sink_json rows (KAFKA BIGINT key, TUMBLING window start, one BIGINT count)
                   as AVRO values
    encode_proto   the same rows as PROTOBUF values (default representation)
The two handles of a pair are alternated step by step; a step is one khip_serde_decode /
khip_sink_encode, which returns after the device has finished, so a step is timed on the host
clock around the call (as tools/sink_avro_bench.py does).  Prints one JSON line: per timing the
median / min / max ms per step, records per second and value bytes per record.
    python tools/proto_bench.py [--steps 10] [--warmup 2] [--decode-records 100000000] [--encode-rows 22000000]
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


def varint_bytes(v, nbytes):
    """(n, nbytes) uint8: the base-128 varint of v, every value taking exactly nbytes."""
    return torch.stack([(((v >> (7 * i)) & 0x7F) | (0x80 if i < nbytes - 1 else 0)).to(torch.uint8) for i in range(nbytes)], dim=1)


def decode_legs(lib, n):
    card, ts = synth.possible_fraud(0, n, n, xp="torch", device="cuda", rank=0, world=1, keys=10_000_000)
    kb = torch.stack([((card >> (8 * (7 - i))) & 0xFF).to(torch.uint8) for i in range(8)], dim=1).reshape(-1)
    koff = torch.arange(0, 8 * (n + 1), 8, dtype=torch.int64, device="cuda")
    amount = 1_000_000_000 + card % 999_999_937  # 1e9..2e9: a 5-byte varint plain and zig-zagged
    legs = {}
    for name, head, body in (("decode_avro", [0, 0, 0, 0, 1], varint_bytes(amount * 2, 5)),
                             ("decode_proto", [0, 0, 0, 0, 1, 0, 0x08], varint_bytes(amount, 5))):
        w = len(head) + 5
        vb = torch.zeros((n, w), dtype=torch.uint8, device="cuda")
        for i, b in enumerate(head):
            vb[:, i] = b
        vb[:, len(head):] = body
        voff = torch.arange(0, w * (n + 1), w, dtype=torch.int64, device="cuda")
        if name == "decode_avro":
            sd = abi.SerdeHandle(lib, "AVRO", [("AMOUNT", "INT64", 0)], key_type="INT64", avro_schema=[("AMOUNT", "long", 0)],
                                 avro_schema_id=1)
        else:
            sd = abi.SerdeHandle(lib, "PROTOBUF", [("AMOUNT", "INT64", 0)], key_type="INT64",
                                 proto_schema=[("AMOUNT", "int64", 1, 0)], avro_schema_id=1)
        keep = (ts, koff, kb, voff, vb.reshape(-1))

        def step(sd=sd, keep=keep):
            d, nerr = sd.decode_device(*keep)
            assert nerr == 0, nerr
            return d
        legs[name] = {"step": step, "handle": sd, "bytes": w, "n": n, "amount": amount}
    return legs


def encode_legs(lib, n):
    h0 = synth._stream(synth.backend("torch"), 8, 0, n, "cuda")
    key = (h0 % 10_000_000).to(torch.int64)
    ws = ((h0 >> 24) % 3).to(torch.int64) * 5000
    we = ws + 5000
    cnt = ((h0 >> 40) % 30 + 1).to(torch.int64)
    nul = torch.zeros(n, dtype=torch.uint8, device="cuda")
    legs = {}
    for name, fmt in (("encode_avro", "AVRO"), ("encode_proto", "PROTOBUF")):
        s = abi.SinkHandle(lib, "KAFKA", [("CARD_NUMBER", "INT64")], fmt, [("KSQL_COL_0", "INT64", 0)], window_kind="TUMBLING",
                           schema_id=1)
        rows = abi.SinkRows()
        rows.n_rows, rows.mem, rows.key_serialized = n, abi.MEM_DEVICE, 0
        rows.key_i64, rows.window_start, rows.window_end = key.data_ptr(), ws.data_ptr(), we.data_ptr()
        cd = (abi.C.c_void_p * 1)(cnt.data_ptr())
        cn = (abi.C.c_void_p * 1)(nul.data_ptr())
        rows.col_data, rows.col_null = cd, cn
        kcap, vcap = 16 * n, 16 * n
        bufs = [torch.empty(n + 1, dtype=torch.int64, device="cuda"), torch.empty(n + 1, dtype=torch.int64, device="cuda"),
                torch.empty(kcap, dtype=torch.uint8, device="cuda"), torch.empty(vcap, dtype=torch.uint8, device="cuda"),
                torch.empty(n, dtype=torch.uint8, device="cuda")]
        out = abi.SinkOut()
        out.mem, out.key_capacity, out.value_capacity = abi.MEM_DEVICE, kcap, vcap
        out.key_offsets, out.value_offsets = bufs[0].data_ptr(), bufs[1].data_ptr()
        out.key_bytes, out.value_bytes, out.value_null = bufs[2].data_ptr(), bufs[3].data_ptr(), bufs[4].data_ptr()
        keep = (key, ws, we, cnt, nul, cd, cn, bufs)

        def step(s=s, rows=rows, out=out, keep=keep):
            lib.check(lib.sink_encode(s.h, abi.C.byref(rows), abi.C.byref(out)), "sink_encode")
            return out.value_len
        legs[name] = {"step": step, "handle": s, "n": n}
    return legs


def run_pair(legs, steps, warmup):
    names = list(legs)
    times = {q: [] for q in names}
    last = {}
    for k in range(warmup + steps):
        for q in names[k % 2:] + names[:k % 2]:  # alternate who goes first
            t0 = time.perf_counter()
            last[q] = legs[q]["step"]()
            if k >= warmup:
                times[q].append(1e3 * (time.perf_counter() - t0))
    return times, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--decode-records", type=int, default=100_000_000)
    ap.add_argument("--encode-rows", type=int, default=22_000_000)
    args = ap.parse_args()
    torch.cuda.init()
    lib = abi.load_product()
    out = {"steps": args.steps, "library": os.path.basename(lib.path)}
    legs = decode_legs(lib, args.decode_records)
    times, last = run_pair(legs, args.steps, args.warmup)
    cols = {q: legs[q]["handle"].columns(last[q], ["INT64"]) for q in legs}
    assert torch.equal(torch.from_numpy(cols["decode_avro"]["cols"][0]), torch.from_numpy(cols["decode_proto"]["cols"][0]))
    assert (cols["decode_proto"]["cols"][0][:1000] == legs["decode_proto"]["amount"][:1000].cpu().numpy()).all()
    for q in legs:
        med = statistics.median(times[q])
        out[q] = {"median_ms": round(med, 3), "min_ms": round(min(times[q]), 3), "max_ms": round(max(times[q]), 3),
                  "records_per_s": round(legs[q]["n"] / med * 1e3), "value_bytes_per_record": legs[q]["bytes"]}
        legs[q]["handle"].close()
    del legs, last, cols
    torch.cuda.empty_cache()
    legs = encode_legs(lib, args.encode_rows)
    times, last = run_pair(legs, args.steps, args.warmup)
    for q in legs:
        med = statistics.median(times[q])
        out[q] = {"median_ms": round(med, 3), "min_ms": round(min(times[q]), 3), "max_ms": round(max(times[q]), 3),
                  "records_per_s": round(legs[q]["n"] / med * 1e3), "value_bytes_per_record": round(last[q] / legs[q]["n"], 3)}
        legs[q]["handle"].close()
    out["proto_over_avro_decode"] = round(out["decode_proto"]["median_ms"] / out["decode_avro"]["median_ms"], 3)
    out["proto_over_avro_encode"] = round(out["encode_proto"]["median_ms"] / out["encode_avro"]["median_ms"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
