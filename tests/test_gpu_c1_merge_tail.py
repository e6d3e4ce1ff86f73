"""The COUNT(*) merge's sized last chunk and its shortcut for items without resident rows
(k_c1_merge, ksql_amd/csrc/khip_agg_c1.hip) against the oracle, exact equality, TUMBLING 5 s.

A chunk is AU x NT = 4 x 512 records (3 x 512 for the wide records); an item's last chunk with
nu = ceil(r / 512) live slot rows of 1 or 2 runs a variant that issues nothing for the other rows,
in the prefetch (load, load01) and in apply.  An item whose partition has no resident rows forms
its row counts without the count pass.  The cases:
- one key with n on every slot-row boundary of the last chunk, items of one to four chunks;
- one partition (keys picked on the host with the library's partition function) with the bench's
  ~1300 keys in its first three chunks and a tail of 1, 300 and 700 records, half of them to keys
  first seen in the tail (claims, list appends and collisions in the tail variant);
- one partition whose groups pass the table's 3072 only in the tail: the item fails and is retried
  with sub-passes (a work list and no resident rows: the shortcut's shared-region reservation);
- three pushes with a changelog: the second touches partitions with resident rows (count pass) and
  partitions first seen in it (shortcut), the third evicts the first window;
- the wide-record and the 64-bit-identity instantiations with a last chunk of one slot row.
hint 2^22 gives 2^12 partitions of 4096-row regions and a table of 4096 entries (hmax 3072).  Every
push must go through the pipeline (c1_pushes); a case's record count per item is checked from the
oracle's counts.
"""
import numpy as np
import pytest

from ksql_amd import abi
from test_gpu_c1 import HAVING, _desc, _fraud, _run  # noqa: F401  (_desc: _run's descriptor)
from test_gpu_parity import assert_snap_equal

pytestmark = pytest.mark.gpu

HINT = 1 << 22
LOG2P = 12  # part_init: ceil(log2(2 hint / 3072)) partitions
NT, CR = 512, 2048
ONE_KEY_N = [c * CR + d for c in range(4)
             for d in (1, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048)]


@pytest.fixture(scope="module")
def prod():
    return abi.load_product()


@pytest.fixture(scope="module")
def orc():
    return abi.load_oracle()


def _mix64(h):
    h = h ^ (h >> np.uint64(33))
    h = h * np.uint64(0xff51afd7ed558ccd)
    h = h ^ (h >> np.uint64(33))
    h = h * np.uint64(0xc4ceb9fe1a85ec53)
    return h ^ (h >> np.uint64(33))


def part_of(keys, log2p=LOG2P):
    """The library's partition of a key: the top log2P bits of mix64(key ^ C) (khip_part.hpp)."""
    with np.errstate(over="ignore"):
        h = _mix64(np.asarray(keys, dtype=np.int64).astype(np.uint64) ^ np.uint64(0x6A09E667F3BCC908))
    return (h >> np.uint64(64 - log2p)).astype(np.int64)


@pytest.fixture(scope="module")
def one_partition_keys():
    """Keys of one partition (the one key 1 falls in), ascending, from [1, 2^24): ~4096 of them."""
    cand = np.arange(1, 1 << 24, dtype=np.int64)
    p = part_of(cand)
    keys = cand[p == p[0]]
    assert len(keys) > 3600 and len(np.unique(part_of(keys))) == 1
    return keys


def _run_snap(prod, orc, batches, changes=False, **kw):
    """_run that also returns the oracle's final table."""
    flags = abi.FLAG_CHANGELOG if changes else 0
    gd, od = _desc(flags=flags | abi.FLAG_PROFILE, **kw), _desc(flags=flags, **kw)
    g, o = abi.AggHandle(prod, gd), abi.AggHandle(orc, od)
    for b in batches:
        gs, os_ = g.push(b), o.push(b)
        assert gs == os_, (gs, os_)
        if changes:
            gc, oc = g.changes(), o.changes()
            assert_snap_equal(gc, oc, gd)
            assert np.array_equal(gc["tombstone"], oc["tombstone"])
    gsnap, osnap = g.snapshot(), o.snapshot()
    assert_snap_equal(gsnap, osnap, gd)
    assert g.count_rows(HAVING) == o.snapshot(HAVING)["n"]
    kt = g.kernel_times()
    g.close()
    o.close()
    return kt, osnap


def _records_of(osnap, keys):
    """Records the oracle counted for these keys (the COUNT(*) column summed over their rows)."""
    m = np.isin(osnap["key"], keys)
    return int(np.asarray(osnap["values"][0])[m].sum())


@pytest.mark.parametrize("n", ONE_KEY_N)
def test_one_key_tail_rows(prod, orc, n):
    rng = np.random.default_rng(500 + n)
    _, ts = _fraud(rng, n, 1)
    k = np.full(n, 123_456, dtype=np.int64)
    kt, osnap = _run_snap(prod, orc, [abi.HostBatch(ts, keys=k)], hint=HINT)
    assert kt["c1_pushes"] == 1, kt
    assert _records_of(osnap, [123_456]) == n


@pytest.mark.parametrize("tail", [1, 300, 700])
def test_many_groups_in_the_tail(prod, orc, one_partition_keys, tail):
    rng = np.random.default_rng(600 + tail)
    old, fresh = one_partition_keys[:1300], one_partition_keys[1300:1300 + (tail + 1) // 2]
    head = old[rng.integers(0, len(old), 3 * CR)]
    t = np.where(np.arange(tail) % 2 == 0, fresh[np.arange(tail) // 2], old[rng.integers(0, len(old), tail)])
    k = np.concatenate([head, t])
    _, ts = _fraud(rng, len(k), 1)
    kt, osnap = _run_snap(prod, orc, [abi.HostBatch(ts, keys=k)], hint=HINT)
    assert kt["c1_pushes"] == 1, kt
    assert _records_of(osnap, one_partition_keys) == 3 * CR + tail == osnap["values"][0].sum()
    assert osnap["n"] < 3072  # the item stays under hmax: no retry


def test_table_overflow_first_seen_in_the_tail(prod, orc, one_partition_keys):
    """One window: 2900 groups in the item's first 6144 records, 400 more in its last 400."""
    rng = np.random.default_rng(700)
    old, fresh = one_partition_keys[:2900], one_partition_keys[2900:3300]
    head = rng.permutation(np.concatenate([old, old[rng.integers(0, len(old), 3 * CR - len(old))]]))
    k = np.concatenate([head, fresh])
    _, ts = _fraud(rng, len(k), 1, span=4_000)  # ts < 4500: one window, a group per key
    kt, osnap = _run_snap(prod, orc, [abi.HostBatch(ts, keys=k)], hint=HINT)
    assert kt["c1_pushes"] == 1 and kt["c1_declined"] == 0, kt
    assert _records_of(osnap, one_partition_keys) == 3 * CR + 400
    assert 3072 < osnap["n"] == 3300 < 4096  # over the table, inside the region


def test_resident_and_first_seen_partitions_in_one_launch(prod, orc):
    """Push 1: 1500 keys (at most 1500 of the 4096 partitions get rows).  Push 2: those keys and
    30000 more, still partly in the first window.  Push 3: later records; the stream time before
    it has closed the first window (grace 1 s), which it evicts."""
    rng = np.random.default_rng(800)
    ka = rng.choice(1 << 22, 1500, replace=False)
    kb = np.concatenate([ka, rng.choice(1 << 22, 30_000, replace=False)])
    pa, pb = np.unique(part_of(ka)), np.unique(part_of(kb))
    assert len(np.setdiff1d(pb, pa)) > 1000 and len(np.intersect1d(pb, pa)) > 1000
    batches = []
    for pool, n, t0 in ((ka, 20_000, 0), (kb, 300_000, 4_000), (kb, 100_000, 9_000)):
        _, ts = _fraud(rng, n, 1, span=4_900, disorder=100, t0=t0)
        batches.append(abi.HostBatch(ts, keys=pool[rng.integers(0, len(pool), n)]))
    kt = _run(prod, orc, batches, changes=True, grace=1000, hint=HINT)
    assert kt["c1_pushes"] == 3, kt


def test_wide_records_tail_of_one_row(prod, orc):
    """Two keys 2^53 apart (the wide records, chunks of 3 x 512): items of 3072 + 100 and
    1536 + 1 records."""
    rng = np.random.default_rng(900)
    a, b = 7, (1 << 53) - 5
    k = rng.permutation(np.concatenate([np.full(3072 + 100, a, dtype=np.int64), np.full(1536 + 1, b, dtype=np.int64)]))
    _, ts = _fraud(rng, len(k), 1)
    kt, osnap = _run_snap(prod, orc, [abi.HostBatch(ts, keys=k)], hint=HINT)
    assert kt["c1_pushes"] == 1 and kt["c1_declined"] == 0, kt
    assert part_of([a])[0] != part_of([b])[0]
    assert _records_of(osnap, [a]) == 3072 + 100 and _records_of(osnap, [b]) == 1536 + 1


def test_id64_tail_of_one_row(prod, orc):
    """Keys 0 and 2^30, two windows: a key range of 31 bits and a window bit need the 64-bit
    identity (as test_gpu_c1_merge_shapes.test_identity_width_switch).  Items of 4096 + 100 and
    2048 + 512 records."""
    rng = np.random.default_rng(901)
    a, b = 0, 1 << 30
    k = rng.permutation(np.concatenate([np.full(4096 + 100, a, dtype=np.int64), np.full(2048 + 512, b, dtype=np.int64)]))
    _, ts = _fraud(rng, len(k), 1, span=9_500)
    assert ts.max() < 10_000 and ts.min() < 5_000
    kt, osnap = _run_snap(prod, orc, [abi.HostBatch(ts, keys=k)], hint=HINT)
    assert kt["c1_pushes"] == 1, kt
    assert part_of([a])[0] != part_of([b])[0]
    assert _records_of(osnap, [a]) == 4096 + 100 and _records_of(osnap, [b]) == 2048 + 512
