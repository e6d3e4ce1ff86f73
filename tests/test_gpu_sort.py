"""The device primitives of ksql_amd/csrc/khip_sort.hpp, called directly through the test-only
helper library (tools/sort_check.hip, tests/sortcheck.py) and compared with numpy on the host.
Every comparison is exact.

- sort_pairs / sort_run: both tile shapes (1024 x 8 through sort_pairs, 512 x 16 through sort_run)
  and both value widths, sizes on and around the wave and tile edges, every pass count 1..8 (both
  parities of the third-buffer path), one tile to 301 tiles (more than can be resident at once, so
  late tiles look back over finished ones).  4-byte values are the row index, so equality with
  numpy's stable argsort is the stability check; 8-byte values carry the row index in their low
  half below a random payload.
- scan_excl: the three instantiated type pairs, sizes around one round (1024), one block (8192) and
  k_sc_top's second round (8192 * 1024 blocks' worth), in == out or not, with_total, total_host.
- rle_sorted: sizes around the same edges; segment heads on, before and after the round and block
  edges; the key extremes.

The helper guards every buffer a primitive writes and fails a call whose guard bytes changed."""
import itertools

import numpy as np
import pytest

import sortcheck

pytestmark = pytest.mark.gpu

TILE = sortcheck.TILE
U64 = np.uint64
FILL64 = int.from_bytes(bytes([sortcheck.FILL]) * 8, "little")

# ------------------------------------------------------------------ sort

SORT_PARAMS = [(0, 4), (0, 8), (1, 4), (1, 8)]  # (tile config, value bytes)
SORT_SIZES = [1, 2, 63, 64, 65, 8191, 8192, 8193, 16384, 3 * 8192 + 1, 40 * 8192 + 4097]
SORT_SIZE_RESIDENT = 300 * 8192 + 5  # more tiles than 256 CUs hold at one tile per CU
END_BITS = [1, 8, 9, 16, 17, 24, 32, 33, 40, 48, 56, 57, 64]
ALL_DISTS_UP_TO = 3 * 8192 + 1  # above it two distributions per end_bit, rotating through all


def _passes(end_bit):
    return min(8, max(1, (end_bit + 7) // 8))


def _mask(end_bit):
    return U64((1 << end_bit) - 1)


def _u64(rng, n):
    return rng.integers(0, 2 ** 64 - 1, n, dtype=U64, endpoint=True)


def _bytes_key(n, f):
    """Keys whose digit of pass p is f(i, p) & 255."""
    i = np.arange(n, dtype=U64)
    k = np.zeros(n, U64)
    for p in range(8):
        k |= (f(i, U64(p)) & U64(255)) << U64(8 * p)
    return k


def d_uniform(rng, n, eb):
    return _u64(rng, n) & _mask(eb)


def d_all_equal(rng, n, eb):  # one digit owns whole tiles
    return np.full(n, _u64(rng, 1)[0] & _mask(eb), U64)


def d_top_bit(rng, n, eb):  # two values that differ only in the top bit of the range
    base = _u64(rng, 1)[0] & (_mask(eb) >> U64(1))
    return base | (rng.integers(0, 2, n, dtype=U64) << U64(eb - 1))


def d_sorted(rng, n, eb):
    return np.sort(d_uniform(rng, n, eb))


def d_reversed(rng, n, eb):
    return np.sort(d_uniform(rng, n, eb))[::-1].copy()


def d_one_live_digit(rng, n, eb):  # every pass but one sees a constant digit
    p = int(rng.integers(0, _passes(eb)))
    live = U64(255) << U64(8 * p)
    return ((_u64(rng, 1)[0] & ~live) | (_u64(rng, n) & live)) & _mask(eb)


def d_wave_shares_digit(rng, n, eb):  # the 64 lanes of a wave's round hold one digit, in every pass
    return _bytes_key(n, lambda i, p: (i >> U64(6)) * U64(37) + p * U64(11)) & _mask(eb)


def d_wave_distinct_digits(rng, n, eb):  # 64 distinct digits per round (odd multiplier: a bijection mod 256)
    return _bytes_key(n, lambda i, p: i * (U64(2) * p + U64(1)) + p) & _mask(eb)


def d_long_runs(rng, n, eb):  # runs of one key that cross tile boundaries, keys in no order
    lens = rng.integers(3000, 20000, n // 3000 + 1)
    return np.repeat(_u64(rng, len(lens)) & _mask(eb), lens)[:n].copy()


DISTS = [d_uniform, d_all_equal, d_top_bit, d_sorted, d_reversed, d_one_live_digit, d_wave_shares_digit,
         d_wave_distinct_digits, d_long_runs]


def _sort_cases():
    """(n, end_bit, distribution) of the main matrix: every size at every end_bit; every distribution
    up to three tiles, two per end_bit (rotating through all nine) at the 41-tile size."""
    cases = []
    for n in SORT_SIZES:
        for j, eb in enumerate(END_BITS):
            ds = DISTS if n <= ALL_DISTS_UP_TO else [DISTS[(2 * j) % len(DISTS)], DISTS[(2 * j + 1) % len(DISTS)]]
            cases += [(n, eb, d) for d in ds]
    return cases


def _values(rng, n, vbytes):
    idx = np.arange(n, dtype=np.uint32)
    if vbytes == 4:
        return idx
    return (rng.integers(0, 2 ** 32, n, dtype=U64) << U64(32)) | idx.astype(U64)


def _check_sort(rng, cfg, vbytes, n, eb, dist):
    keys = dist(rng, n, eb)
    assert keys.dtype == U64 and len(keys) == n and int(keys.max()) < 2 ** eb  # the callers' contract
    vals = _values(rng, n, vbytes)
    ko, vo, passes, third = sortcheck.sort(cfg, keys, vals, eb)
    what = "cfg=%d V=%d n=%d end_bit=%d %s" % (cfg, vbytes, n, eb, dist.__name__)
    assert passes == _passes(eb), what
    assert third == (passes % 2 == 0), what  # the third buffer takes the first pass of an even count
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(ko, keys[order]), what
    assert np.array_equal(vo, vals[order]), what + " (values: order within equal keys)"
    return passes


def _assert_matrix(cases):
    """A later edit must not thin the matrix: both tile shapes and value widths, every listed size
    and end_bit, every pass count on many tiles, every distribution."""
    assert sorted(SORT_PARAMS) == sorted(itertools.product((0, 1), (4, 8)))
    assert {n for n, _, _ in cases} >= {1, 2, 63, 64, 65, 8191, 8192, 8193, 16384, 3 * 8192 + 1, 40 * 8192 + 4097}
    assert {eb for _, eb, _ in cases} == {1, 8, 9, 16, 17, 24, 32, 33, 40, 48, 56, 57, 64}
    for n in {n for n, _, _ in cases}:
        assert {_passes(eb) for m, eb, _ in cases if m == n} == set(range(1, 9)), n
    assert {_passes(eb) for n, eb, _ in cases if n > 2 * TILE} == set(range(1, 9))  # look-back at every pass count
    assert {d for n, _, d in cases if n > 2 * TILE} == set(DISTS) and len(DISTS) == 9


@pytest.mark.parametrize("cfg,vbytes", SORT_PARAMS)
def test_sort_matrix(cfg, vbytes):
    sortcheck.load()
    cases = _sort_cases()
    _assert_matrix(cases)
    rng = np.random.default_rng(1000 + 10 * cfg + vbytes)
    ran = set()
    for n, eb, dist in cases:
        ran.add((n > TILE, _check_sort(rng, cfg, vbytes, n, eb, dist)))
    assert ran == set(itertools.product((False, True), range(1, 9)))  # one tile and many, 1..8 passes reached


@pytest.mark.parametrize("cfg,vbytes", SORT_PARAMS)
def test_sort_more_tiles_than_resident(cfg, vbytes):
    """301 tiles at 8 passes: tiles with late tickets start after early ones have left, and look
    back over inclusive prefixes only."""
    sortcheck.load()
    assert sorted(SORT_PARAMS) == sorted(itertools.product((0, 1), (4, 8)))
    n = SORT_SIZE_RESIDENT
    assert n == 300 * 8192 + 5 and -(-n // TILE) > 256
    rng = np.random.default_rng(2000 + 10 * cfg + vbytes)
    for dist in (d_uniform, d_long_runs, d_top_bit):
        assert _check_sort(rng, cfg, vbytes, n, 64, dist) == 8


# ------------------------------------------------------------------ scan

SCAN_SIZES = [0, 1, 1023, 1024, 1025, 8191, 8192, 8193, 5 * 8192 + 17]
SCAN_SIZES_TOP = [8192 * 1024 - 1, 8192 * 1024, 8192 * 1024 + 1]  # the last: k_sc_top's second round
MODES = list(itertools.product((False, True), repeat=3))  # (with_total, alias, want_host)


def _check_scan(kind, x, with_total, alias, want_host):
    n = len(x)
    dt = sortcheck.SCAN_TYPES[kind][1]
    inc = np.cumsum(x.astype(np.int64), dtype=np.int64)
    total = int(inc[-1]) if n else 0
    assert np.iinfo(dt).min <= (int(inc.min()) if n else 0) and (int(inc.max()) if n else 0) <= np.iinfo(dt).max
    want = np.concatenate([np.zeros(1, np.int64), inc])[:n + (1 if with_total else 0)].astype(dt)
    out, host = sortcheck.scan(kind, x, with_total, alias, want_host)
    what = "%s n=%d with_total=%d alias=%d host=%d" % (kind, n, with_total, alias, want_host)
    assert out.dtype == want.dtype and np.array_equal(out, want), what
    if want_host:
        assert host == total, what


def _scan_input(rng, kind, n):
    dt = sortcheck.SCAN_TYPES[kind][1]
    return rng.integers(0 if kind == "uint32" else -7, 8, n).astype(dt)


@pytest.mark.parametrize("kind", ["int64", "int32", "uint32"])
def test_scan_sizes_and_modes(kind):
    sortcheck.load()
    assert len(MODES) == 8
    rng = np.random.default_rng(31)
    for n in SCAN_SIZES:
        x = _scan_input(rng, kind, n)
        for with_total, alias, want_host in MODES:
            _check_scan(kind, x, with_total, alias, want_host)


def test_scan_int64_carries_past_32_bits():
    sortcheck.load()
    rng = np.random.default_rng(32)
    x = 2 ** 40 + rng.integers(-1000, 1000, 5 * 8192 + 17)
    for with_total, alias, want_host in MODES:
        _check_scan("int64", x, with_total, alias, want_host)


@pytest.mark.parametrize("kind", ["int64", "uint32"])
def test_scan_top_level_rounds(kind):
    """1023.99.., 1024 and 1024.00.. blocks of 8192: k_sc_top scans the block sums in one round of
    1024, and in two with a carry between them at the last size."""
    sortcheck.load()
    rng = np.random.default_rng(33)
    big = _scan_input(rng, kind, SCAN_SIZES_TOP[-1])
    assert [-(-n // 8192) for n in SCAN_SIZES_TOP] == [1024, 1024, 1025]
    for n in SCAN_SIZES_TOP:
        for with_total, alias, want_host in ((True, False, True), (False, True, False)):
            _check_scan(kind, big[:n], with_total, alias, want_host)


# ------------------------------------------------------------------ run-length

RLE_SIZES = [1, 1023, 1024, 1025, 8191, 8192, 8193, 3 * 8192 + 1]


def _from_heads(n, heads):
    h = np.zeros(n, np.int64)
    h[np.array([i for i in heads if 0 < i < n], np.int64)] = 1
    return np.cumsum(h).astype(U64)


def r_distinct(rng, n):
    return np.arange(n, dtype=U64) * U64(3) + U64(5)


def r_one_segment(rng, n):
    return np.full(n, 77, U64)


def r_heads_at_edges(rng, n):  # heads on the round (1024) and block (8192) edges and one either side
    return _from_heads(n, [m + d for m in range(1024, n + 2, 1024) for d in (-1, 0, 1)])


def r_heads_on_edges_only(rng, n):
    return _from_heads(n, range(1024, n, 1024))


def r_long_run(rng, n):  # one run over several blocks between singletons
    return _from_heads(n, [1, 2, 3, n - 2, n - 1])


def r_singleton_ends(rng, n):
    return _from_heads(n, [1, n - 1])


def r_extreme_keys(rng, n):  # key 0 first, 2^64 - 1 last
    k = np.sort(rng.integers(1, 2 ** 64 - 1, n, dtype=U64) >> U64(int(rng.integers(0, 60))))
    k[0] = 0
    k[-1] = 2 ** 64 - 1
    return k


def r_random_runs(rng, n):
    return np.sort(rng.integers(0, max(2, n // 5), n).astype(U64))


RLE_PATTERNS = [r_distinct, r_one_segment, r_heads_at_edges, r_heads_on_edges_only, r_long_run, r_singleton_ends,
                r_extreme_keys, r_random_runs]


@pytest.mark.parametrize("pattern", RLE_PATTERNS, ids=[p.__name__ for p in RLE_PATTERNS])
def test_rle_sorted(pattern):
    sortcheck.load()
    rng = np.random.default_rng(41)
    for n in RLE_SIZES:
        keys = pattern(rng, n)
        assert len(keys) == n and keys.dtype == U64 and np.all(keys[1:] >= keys[:-1])
        uk, first, counts = np.unique(keys, return_index=True, return_counts=True)
        ns = len(uk)
        r = sortcheck.rle(keys)
        what = "%s n=%d" % (pattern.__name__, n)
        assert r["nseg_dev"] == ns and r["nseg_host"] == ns, what
        assert np.array_equal(r["ukeys"][:ns], uk), what
        assert np.array_equal(r["cnt"][:ns], counts.astype(np.int32)), what
        assert np.array_equal(r["start"][:ns], first.astype(np.int64)), what
        assert r["start"][ns] == n, what
        # nothing written past the segments
        assert np.all(r["ukeys"][ns:] == U64(FILL64)), what
        assert np.all(r["cnt"][ns:].view(np.uint32) == np.uint32(FILL64 & 0xFFFFFFFF)), what
        assert np.all(r["start"][ns + 1:].view(U64) == U64(FILL64)), what
    if pattern is r_distinct:
        assert ns == n
    if pattern is r_one_segment:
        assert ns == 1
