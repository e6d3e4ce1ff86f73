"""The step runs' two-level positions and the push's bookkeeping around them (k_c1_scatter /
k_c1v_scatter's flush_run_counts, k_c1_runpos, k_c1_check, k_c1_chunks, chunk_map, k_part_commit;
ksql_amd/csrc/khip_agg_c1.hip) against the oracle, exact equality after every push.

A scatter step (4096 COUNT(*) records, 2048 value records) leaves as one run in bucket order; a
tile is 65,536 records (16 or 32 steps).  A run's place in its bucket = the tile's base in the
bucket (a per-bucket scan of the tiles' totals) + the run's place within the tile (u16).  The
refine's chunks (8192 records of a bucket) find their runs by two searches over those.  The shapes
are the smallest at which that arithmetic can go wrong:
- step and tile edges: n around one step, two steps, one tile and two tiles, with 50,000 keys
  (every bucket populated in every tile) and with one key (one bucket: the place within the tile
  reaches its maximum, every chunk starts in the middle of the bucket's tiles, the second tile's
  base is 65,536), for COUNT(*), SUM(BIGINT) TUMBLING and SUM HOPPING 60 s / 10 s (panes);
- empty runs and ties: one hot key and 3,000 keys of 1-3 records, so that most (bucket, step) runs
  are empty and consecutive runs share a position;
- sentinels: null keys, null rows and negative timestamps travel in the runs, are dropped by the
  refine, and are counted by k_c1_check's sums of the tiles' counters;
- three pushes on one handle, the last of which closes the first window AND is retried: its
  4,000 new keys share one partition (their hashes share the top 12 bits; hint 2^21 gives 2048
  partitions with an LDS table of 3072 groups, tests/test_gpu_c1.py::test_c1_evict_and_retry_release),
  so pass 0 overflows the table and evicts, and the closed rows' count of the later passes reaches
  the host with those passes' counters.  The release build has no pass trace: that the retry
  happens holds by construction;
- a declined push in between: push 2 of 3 ends with a record grace no longer allows, k_c1_check
  declines it and the general path computes that push's statistics itself.  The product then
  skips the pipeline for the next pushes, so push 3 takes the general path too: c1_pushes is 1;
- keys spread over 2^53: the wide records go through the same runs with the parallel ts array.
Every other case asserts that each push went through the pipeline (c1_pushes), so a case that
falls back to the general path fails.
"""
import numpy as np
import pytest

from ksql_amd import abi
from test_gpu_c1 import _desc, _fraud, _run  # noqa: F401  (_desc: _run's descriptor)
from test_gpu_c1v import _batches
from test_gpu_c1v import _run as _run_v

pytestmark = pytest.mark.gpu

EDGE_N = [1, 4095, 4096, 4097, 8191, 8193, 65535, 65536, 65537, 131073, 200001]
KEYS = [50_000, 1]
HINT = 1 << 22
V_HINT = 3_000_000


@pytest.fixture(scope="module")
def prod():
    return abi.load_product()


@pytest.fixture(scope="module")
def orc():
    return abi.load_oracle()


# ---- input generators (no GPU needed: checked against the oracle alone)

def edge_count(n, keys):
    rng = np.random.default_rng(1000 * keys + n)
    k, ts = _fraud(rng, n, keys)
    return [abi.HostBatch(ts, keys=k)]


def edge_value(n, keys, span):
    rng = np.random.default_rng(7000 * keys + n)
    return _batches(rng, "sum_i64", 1, n, keys, span)


def hot_and_cold():
    rng = np.random.default_rng(31)
    n = 300_000
    cold = np.repeat(rng.choice(1 << 20, 3000, replace=False) + 1, rng.integers(1, 4, 3000))
    k = rng.permutation(np.concatenate([np.zeros(n - len(cold), dtype=np.int64), cold]))
    assert len(k) == n and (k == 0).mean() > 0.95
    _, ts = _fraud(rng, n, 1)
    return [abi.HostBatch(ts, keys=k)]


def sentinels():
    rng = np.random.default_rng(32)
    n = 150_000
    k, ts = _fraud(rng, n, 20_000, t0=10_000)
    ts[rng.random(n) < 0.01] = -1
    return [abi.HostBatch(ts, keys=k, key_valid=rng.random(n) > 0.03, row_valid=rng.random(n) > 0.03)]


def _key_hash(k):
    """The partitioner's hash of an int64 key (key_hash, ksql_amd/csrc/khip_part.hpp): the
    partition is its top bits."""
    with np.errstate(over="ignore"):
        h = k.astype(np.uint64) ^ np.uint64(0x6A09E667F3BCC908)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xFF51AFD7ED558CCD)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xC4CEB9FE1A85EC53)
        h ^= h >> np.uint64(33)
    return h


def three_pushes_retry():
    """Pushes of 70,000 records over [0, 5 s), [5 s, 10 s), [10 s, 15 s), grace 1 s: push 3 closes
    window 0.  Pushes 1 and 2: 20,000 keys.  Push 3: 4,000 keys of one partition (hashes sharing
    their top 12 bits), 8 records each, and 38,000 records of the 20,000 keys."""
    rng = np.random.default_rng(33)
    n = 70_000
    cand = np.arange(1 << 20, (1 << 20) + (1 << 24), dtype=np.int64)
    top = _key_hash(cand) >> np.uint64(52)
    one_part = cand[top == top[0]][:4000]
    assert len(one_part) == 4000
    out = []
    for p in range(3):
        k, ts = _fraud(rng, n, 20_000, span=5_000, disorder=100, t0=5_000 * p)
        if p == 2:
            k[: 8 * len(one_part)] = np.repeat(one_part, 8)
            k = rng.permutation(k)
        out.append(abi.HostBatch(ts, keys=k))
    return out


def declined_in_between():
    """Three pushes of 70,000 records over consecutive 5 s spans, grace 1 s; push 2's last record
    has ts 0, whose window [0, 5 s) closed at stream time 6 s."""
    rng = np.random.default_rng(34)
    out = []
    for p in range(3):
        k, ts = _fraud(rng, 70_000, 20_000, span=5_000, disorder=100, t0=5_000 * p)
        if p == 1:
            ts[-1] = 0
        out.append(abi.HostBatch(ts, keys=k))
    return out


def wide_keys():
    rng = np.random.default_rng(35)
    k, ts = _fraud(rng, 70_000, 20_000)
    return [abi.HostBatch(ts, keys=(k * 0x5DEECE66D) & ((1 << 53) - 1))]  # a bijection on [0, 2^53)


# ---- the cases

@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("n", EDGE_N)
def test_count_step_and_tile_edges(prod, orc, n, keys):
    kt = _run(prod, orc, edge_count(n, keys), hint=HINT)
    assert kt["c1_pushes"] == 1 and kt["c1_declined"] == 0, kt


@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("n", EDGE_N)
def test_sum_tumbling_step_and_tile_edges(prod, orc, n, keys):
    kt = _run_v(prod, orc, "sum_i64", "tumbling", edge_value(n, keys, 40_000), hint=V_HINT)
    assert kt["c1_pushes"] == 1 and kt["c1_declined"] == 0, kt


@pytest.mark.parametrize("keys", KEYS)
@pytest.mark.parametrize("n", [65537, 131073])
def test_sum_hopping_tile_edges(prod, orc, n, keys):
    kt = _run_v(prod, orc, "sum_i64", "hop6", edge_value(n, keys, 200_000), hint=V_HINT)
    assert kt["c1_pushes"] == 1 and kt["c1_declined"] == 0, kt


def test_empty_runs_and_ties(prod, orc):
    kt = _run(prod, orc, hot_and_cold(), hint=HINT)
    assert kt["c1_pushes"] == 1 and kt["c1_declined"] == 0, kt


def test_sentinels_and_summed_statistics(prod, orc):
    kt = _run(prod, orc, sentinels(), hint=HINT)
    assert kt["c1_pushes"] == 1 and kt["c1_declined"] == 0, kt


def test_three_pushes_close_and_retry(prod, orc):
    kt = _run(prod, orc, three_pushes_retry(), changes=True, grace=1000, hint=1 << 21)
    assert kt["c1_pushes"] == 3 and kt["c1_declined"] == 0, kt


def test_declined_push_in_between(prod, orc):
    kt = _run(prod, orc, declined_in_between(), changes=True, grace=1000, hint=HINT)
    assert kt["c1_declined"] == 1 and kt["c1_pushes"] == 1, kt


def test_wide_records(prod, orc):
    kt = _run(prod, orc, wide_keys(), hint=HINT)
    assert kt["c1_pushes"] == 1 and kt["c1_declined"] == 0, kt
