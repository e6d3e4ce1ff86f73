"""The expression step's time on device-resident batches (DESIGN.md "Expression step"; results in
profiles/expr/README.md).

Two programs over 2^26 rows (INT a, BIGINT b, DOUBLE c, BIGINT key, ts), with the WHERE keeping 0 %,
50 % and 100 % of the rows:
    shapes      WHERE a*b > c, OUT a+1 (INT), OUT b*2 (BIGINT), OUT c/2.0 (DOUBLE), KEY a % 7
    where_only  WHERE a*b > c: the rows' ts and key compacted, no computed column
A step is one khip_expr_apply, which returns after the device has finished, timed on
the host clock around the call; warm-up steps first, then the median / min / max of the timed ones.
Bytes are what the kernels must read and write, computed from the shapes below (bytes_needed), not
what they happen to move.  Prints one JSON line per (program, keep rate).
    python tools/expr_bench.py [--rows 67108864] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

A, B, C_ = ("COL", 0), ("COL", 1), ("COL", 2)
WHERE = ("WHERE", ("GT", ("MUL", A, B), C_))
PROGRAMS = {
    "shapes": [WHERE, ("OUT", ("ADD", A, ("I32", 1))), ("OUT", ("MUL", B, ("I32", 2))),
               ("OUT", ("DIV", C_, ("F64", 2.0))), ("KEY", ("MOD", A, ("I32", 7)))],
    "where_only": [WHERE],
}


def bytes_needed(program, n, kept):
    """Bytes the step cannot avoid: the keep pass reads a, b, c (20 B / row) and writes and re-reads a
    keep byte; the positions cost a scan's read and write of 8 B / row and the row list 8 B per kept
    row written and read; per kept row the output pass reads ts (8) and, for `shapes`, a, b, c again
    (20), or for `where_only` the key (8), and writes ts (8), the key (8) and, for `shapes`, the three
    columns (4 + 8 + 8); bitmaps are 1 bit per row and column (counted: 5 / 8 resp. 2 / 8 B per kept row)."""
    per_row = 20 + 2 + 16
    if program == "shapes":
        per_kept = 16 + 8 + 20 + 8 + 8 + 20 + 5 / 8
    else:
        per_kept = 16 + 8 + 8 + 8 + 8 + 2 / 8
    return n * per_row + kept * per_kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 26)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from ksql_amd import abi
    if not torch.cuda.is_available():
        sys.exit("expr_bench needs the GPU: there is no CPU path to time")
    torch.cuda.init()
    lib = abi.load_product()
    n = args.rows
    g = torch.Generator(device="cuda").manual_seed(1)
    a = torch.randint(-50, 50, (n,), dtype=torch.int32, device="cuda", generator=g)
    b = torch.randint(-1000, 1000, (n,), dtype=torch.int64, device="cuda", generator=g)
    ts = torch.arange(n, dtype=torch.int64, device="cuda")
    key = torch.randint(0, 1 << 40, (n,), dtype=torch.int64, device="cuda", generator=g)
    prod = (a.to(torch.int64) * b).to(torch.float64)
    for rate in (0.0, 0.5, 1.0):
        keep = torch.rand(n, device="cuda", generator=g) < rate
        c = prod + torch.where(keep, -0.5, 0.5).to(torch.float64)
        kept = int(keep.sum().item())
        batch = abi.DeviceBatch(ts, keys=key, cols=[a, b, c])
        for name, trees in PROGRAMS.items():
            e = abi.Expr(lib, ["INT32", "INT64", "DOUBLE"], abi.expr_words(*trees))
            times = []
            for i in range(args.warmup + args.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out, _ = e.apply(batch, count_errors=False)
                dt = time.perf_counter() - t0
                assert out.struct.n_rows == kept, (out.struct.n_rows, kept)
                if i >= args.warmup:
                    times.append(dt * 1e3)
            e.close()
            med = statistics.median(times)
            need = bytes_needed(name, n, kept)
            print(json.dumps({"program": name, "rows": n, "keep_rate": rate, "kept": kept, "steps": args.steps,
                              "ms_median": round(med, 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
                              "rows_per_s": round(n / (med * 1e-3)), "bytes_needed": int(need),
                              "bytes_per_s": round(need / (med * 1e-3))}), flush=True)
        del c, keep


if __name__ == "__main__":
    main()
