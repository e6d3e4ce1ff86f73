"""Boundary shapes of the COUNT(*) merge's record loop (k_c1_merge, ksql_amd/csrc/khip_agg_c1.hip)
against the oracle, exact equality.

The merge reads a work item's records through a segment table in LDS: a record index is looked up
in a block → segment table (items up to C1_SEGOF << segb records, segb = 5, 6 or 7) or by binary
search (larger items), AU x NT = 2048 records per chunk, indices past the item's end clamped to its
last record.  The cases put an item's record count on every boundary of that code:
- one key (one partition, whole 8192-record segments) with n records around the wave, chunk,
  lookup-block and table/binary-search switches;
- one hot key and thousands of keys with 1-3 records: the hot key's bucket has items whose
  segments are mostly empty (the lookup steps over runs of empty segments), the others 0-3 records;
- many short segments (the bench shape), in one push and in three pushes with windows closing
  (resident rows merged, closed rows evicted, changelog flags);
- the 32-bit and the 64-bit group identity, one key apart;
- keys spread over 2^53 (the wide records' instantiation).
Inputs are TUMBLING 5 s over a 10 s span with at most 500 ms disorder.  Every push must go through
the pipeline (c1_pushes), so a case that falls to the general path fails.
"""
import numpy as np
import pytest

from ksql_amd import abi
from test_gpu_c1 import _desc, _fraud, _run  # noqa: F401  (_desc: _run's descriptor)

pytestmark = pytest.mark.gpu

ONE_KEY_N = [1, 63, 64, 65,
             2047, 2048, 2049, 4096, 4097, 6143, 6144, 6145,  # chunks of AU x NT = 2048, clamped tails
             16384, 16385, 32768, 32769,                      # lookup blocks of 32 / 64 / 128 records
             65536, 65537, 200000]                            # table lookup → binary search


@pytest.fixture(scope="module")
def prod():
    return abi.load_product()


@pytest.fixture(scope="module")
def orc():
    return abi.load_oracle()


@pytest.mark.parametrize("n", ONE_KEY_N)
def test_one_key(prod, orc, n):
    rng = np.random.default_rng(100 + n)
    _, ts = _fraud(rng, n, 1)
    k = np.full(n, 123_456, dtype=np.int64)
    kt = _run(prod, orc, [abi.HostBatch(ts, keys=k)], hint=1 << 22)
    assert kt["c1_pushes"] == 1, kt


def test_hot_key_and_sparse_items(prod, orc):
    rng = np.random.default_rng(21)
    cold = rng.choice(1 << 20, 5000, replace=False) + 1
    k = np.concatenate([np.zeros(200_000, dtype=np.int64), np.repeat(cold, rng.integers(1, 4, len(cold)))])
    k = rng.permutation(k)
    _, ts = _fraud(rng, len(k), 1)
    kt = _run(prod, orc, [abi.HostBatch(ts, keys=k)], hint=1 << 22)
    assert kt["c1_pushes"] == 1, kt


@pytest.fixture(scope="module")
def short_segments():
    rng = np.random.default_rng(22)
    return _fraud(rng, 2_000_000, 200_000)


def test_short_segments_one_push(prod, orc, short_segments):
    k, ts = short_segments
    kt = _run(prod, orc, [abi.HostBatch(ts, keys=k)], hint=400_000 * 8)
    assert kt["c1_pushes"] == 1, kt


def test_short_segments_three_pushes(prod, orc, short_segments):
    """The same records in three pushes, grace 1 s: the later pushes merge resident rows, the last
    one's stream time closes the first window (evicted), and every push's changelog is compared."""
    k, ts = short_segments
    cut = [0, len(k) // 3, 2 * len(k) // 3, len(k)]
    batches = [abi.HostBatch(ts[a:b], keys=k[a:b]) for a, b in zip(cut[:-1], cut[1:])]
    kt = _run(prod, orc, batches, changes=True, grace=1000, hint=400_000 * 8)
    assert kt["c1_pushes"] == 3, kt


@pytest.mark.parametrize("top,width", [((1 << 30) - 1, 32), (1 << 30, 64)])
def test_identity_width_switch(prod, orc, top, width):
    """Two windows (1 window bit) and keys 0 .. top: a key range of 30 bits gives the 32-bit
    identity (30 + 1 = 31), one key further the 64-bit one."""
    rng = np.random.default_rng(23)
    n = 300_000
    pool = np.concatenate([[0, top], rng.integers(0, top, 30_000)])
    k = pool[rng.integers(0, len(pool), n)]
    k[:2] = [0, top]
    _, ts = _fraud(rng, n, 1, span=9_500)  # ts < 10 000: windows 0 and 5000 only
    assert ts.max() < 10_000 and ts.min() < 5_000
    kt = _run(prod, orc, [abi.HostBatch(ts, keys=k)], hint=1 << 22)
    assert kt["c1_pushes"] == 1, kt


def test_sparse_keys_wide_records(prod, orc):
    rng = np.random.default_rng(24)
    batches = []
    for p in range(2):
        k, ts = _fraud(rng, 400_000, 40_000, t0=p * 10_000)
        k = (k * 0x5DEECE66D) & ((1 << 53) - 1)  # a bijection on [0, 2^53) (odd multiplier)
        k[rng.random(len(k)) < 0.2] = 7 * 0x5DEECE66D & ((1 << 53) - 1)  # and one hot key
        batches.append(abi.HostBatch(ts, keys=k))
    kt = _run(prod, orc, batches, changes=True, grace=2000, hint=1 << 22)
    assert kt["c1_pushes"] == 2, kt
