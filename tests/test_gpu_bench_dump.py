"""bench.py --dump-outputs, end to end on the GPU: a plain run of the default leg at a small size
writes the last step's results, and they equal a host GROUP BY of the same seeded records."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ksql_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_table(tmp_path):
    n, keys = 400_000, 40_000
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--records", str(n), "--keys", str(keys), "--dump-outputs", str(tmp_path / "out")],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["unit"] == "records/s" and d["higher_is_better"] is True
    assert abs(d["value"] - n / (d["ms_per_step"] / 1000.0)) <= 1e-9 * d["value"]
    assert d["cpu_baseline"] is None and d["pcie_inclusive_records_per_s"] is None and d["pull_query"] is None

    out = {f[:-4]: np.load(str(tmp_path / "out" / f)) for f in os.listdir(str(tmp_path / "out"))}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64_000_000

    # the host GROUP BY card_number, TUMBLING 5 s window of the same records (none is late: the
    # bench asserts windows_applied == n)
    card, ts = synth.possible_fraud(0, n, n, keys=keys)
    gid, inv, cnt = np.unique(card * 16 + ts // 5000, return_inverse=True, return_counts=True)
    rowtime = np.zeros(len(gid), np.int64)
    np.maximum.at(rowtime, inv, ts)
    stats = dict(zip(("rows_in", "rows_accepted"), out["stats"][:2]))
    assert stats == {"rows_in": n, "rows_accepted": n}
    assert out["having_rows"].tolist() == [int((cnt > 3).sum())]

    # the dumped rows: every group of the sampled card numbers, sorted by (key, window start)
    key, ws = out["table_key"].astype(np.int64), out["table_ws"].astype(np.int64)
    assert len(key) == out["table_rows"][0] > 1000
    dumped = key * 16 + ws // 5000
    want = np.isin(gid // 16, np.unique(key))
    assert np.array_equal(dumped, gid[want])
    assert np.array_equal(out["table_value0"], cnt[want]) and not out["table_null0"].any()
    assert np.array_equal(out["table_we"], ws + 5000) and np.array_equal(out["table_rowtime"], rowtime[want])
