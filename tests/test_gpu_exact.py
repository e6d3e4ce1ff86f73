"""DOUBLE aggregates of the HIP path bit for bit, special values on every engine.

The streams of tests/exact_ref.py leave SUM / AVG one possible bit pattern (addends m * 2^e, so
every partial sum in every order is exact) and plant groups of NaNs (quiet, signalling, negative,
with a payload), +Inf / -Inf, signed zeros, an overflow to +Inf, subnormals, all-NULL arguments
and the BIGINT / INTEGER extremes.  Every engine selection must agree with the oracle under
exact_ref.assert_exact (values through their int64 view; NaN equals NaN, nothing else is left
out) on each push's batch statistics, the snapshot after each push, each push's changes where the
selection keeps them, count_rows of a descriptor HAVING SUM(x) > 0.0 (the maintained count across
finite -> NaN -> NaN) and, after every push, a pull query of the special keys; unwindowed and TUMBLING cases also
against exact_ref.model, so an error shared with the oracle does not pass.  tests/test_exact_ref.py
pins model == oracle without a GPU.

The special groups' rows arrive in pushes 1, 2 and 3 (in-push atomics and the resident merge both
see them); the last push moves stream time far ahead and closes / evicts the early windows.  The
shapes are those at which the existing tests reach each path (named in each test); the paths with
a witness (khip_agg_kernel_times c1_pushes / c1_declined) assert it.
"""
import numpy as np
import pytest

import exact_ref
from exact_ref import assert_exact
from ksql_amd import abi
from test_gpu_parity import ALL_AGGS, WINDOWS

pytestmark = pytest.mark.gpu

COLS4 = ["i32", "i64", "x", "x"]
SUM_X4 = 4  # ALL_AGGS[4] = SUM of the DOUBLE column
JUMP = 400_000
SCALES = exact_ref.SCALES


@pytest.fixture(scope="module")
def prod():
    return abi.load_product()


@pytest.fixture(scope="module")
def orc():
    return abi.load_oracle()


def _step(win):
    """The special groups' three pushes inside one window: 2 * step + 128 < size."""
    return 2000 if win.get("size_ms", 5000) < 60_000 else 20_000


def _check(prod, orc, stream, cols, aggs, win, sum_agg, flags=0, changes=True, model=False, hint=0, emit="CHANGES"):
    """Product against oracle (and model) after every push; returns the product's kernel times.
    sum_agg: the index of SUM over the DOUBLE column (the descriptor's HAVING SUM(x) > 0.0), or
    None.  changes: the selection keeps each push's changes."""
    types = [exact_ref.COL_TYPE[c] for c in cols]
    having = None if sum_agg is None else {"agg": sum_agg, "op": "GT", "value": 0.0}
    kw = dict(win, key_type="INT64", col_types=types, aggs=aggs, having=having, capacity_hint=hint, emit=emit)
    gflags = flags | abi.FLAG_PROFILE | (abi.FLAG_CHANGELOG if changes and emit == "CHANGES" else 0)
    g = abi.AggHandle(prod, abi.make_agg_desc(**dict(kw, flags=gflags)))
    o = abi.AggHandle(orc, abi.make_agg_desc(**kw))
    exp = exact_ref.model(stream, win.get("size_ms", 0), cols, aggs, win.get("grace_ms", -1)) if model else None
    keys, last = stream.special_keys(), len(stream.pushes) - 1
    for p in range(last + 1):
        b = stream.batch(p, cols)
        gs, os_ = g.push(b), o.push(b)
        assert gs == os_, (p, gs, os_)
        snap, osnap = g.snapshot(), o.snapshot()
        assert_exact(snap, osnap, "snapshot after push %d" % p)
        if changes:
            assert_exact(g.changes(), o.changes(), "changes of push %d" % p)
        if having is not None:
            assert g.count_rows(having) == o.snapshot(having)["n"], "HAVING count after push %d" % p
        if exp is not None:
            assert_exact(snap, exp[p]["snapshot"], "snapshot after push %d against the model" % p)
        if p == 1 and sum_agg is not None:
            # the classes are there: +Inf (P1) and -Inf (P2) met in one group, a NaN (P2) in four more
            rows = exact_ref.rows_of_keys(osnap, [stream.special["inf_cancel"]])
            assert np.isnan(rows["values"][sum_agg]).any(), "the special groups' pushes share no window"
            assert np.isnan(osnap["values"][sum_agg]).sum() >= 5
        # the pull query of the special keys, after every push: the jump of the last push expires
        # their windows, so the rows are there to pull only before it
        want = exact_ref.rows_of_keys(osnap, keys)
        assert want["n"] > 0 or p == last, "no special group left to pull after push %d" % p
        assert_exact(g.get(keys=keys), want, "pull query of the special keys after push %d" % p)
    kt = g.kernel_times()
    g.close()
    o.close()
    return kt


# ------------------------------------------------------------------ the general engines

ENGINES = {"part": 0, "part_claim": abi.FLAG_PART_CLAIM, "atomic": abi.FLAG_ENGINE_ATOMIC}


@pytest.mark.parametrize("e", SCALES)
@pytest.mark.parametrize("win", range(len(WINDOWS)))
@pytest.mark.parametrize("engine", list(ENGINES))
def test_general_engines(prod, orc, engine, win, e):
    """test_gpu_parity.py::test_random_vs_oracle's query (four columns, ALL_AGGS: the value pipeline
    is not eligible) and shape, 4 pushes x 4,000 rows over 300 keys, on the partitioned merge in
    both claim modes and on the global-atomic engine (no EMIT CHANGES changelog there).  Windows 2
    and 4 drop late records (disorder past the grace period): oracle only."""
    w = WINDOWS[win]
    late = win in (2, 4)
    stream = exact_ref.make_stream(np.random.default_rng(100 * win + e + 2000), 4, 4000, 300, e, _step(w),
                                   1500 if late else 500, jump=JUMP)
    _check(prod, orc, stream, COLS4, ALL_AGGS, w, SUM_X4, flags=ENGINES[engine], changes=engine != "atomic",
           model=win in (0, 1))


@pytest.mark.parametrize("e", SCALES)
@pytest.mark.parametrize("win", [dict(size_ms=60_000, advance_ms=10_000, grace_ms=30_000),
                                 dict(size_ms=30_000, advance_ms=5_000, grace_ms=0)])
def test_panes(prod, orc, win, e):
    """test_gpu_panes.py's shape (3 x 600,000 rows, 24 keys: partitions with full chunks, so a
    record whose windows are all open updates its pane and the pane is folded into its windows).
    The merge uses panes only for a partition with thousands of records (k_part_merge: rn >= AU * NT),
    which the special keys' few rows alone would not reach: three special groups (a negative NaN,
    +Inf then -Inf, -Inf among finite rows) therefore also take 5 % of every push's rows each, as
    hot as the hot key, and go through the pane -> window fold; the other special groups take
    the per-window path of the same merge.  The rows left behind the stream-time jump inside the
    last push are late under both grace periods."""
    w = dict(win, window_kind="HOPPING")
    stream = exact_ref.make_stream(np.random.default_rng(e + 3000 + win["grace_ms"]), 3, 600_000, 24, e,
                                   win["size_ms"] // 3 - 1000, 5000, jump=JUMP, jump_half=True,
                                   crowd=("nan_negative", "inf_cancel", "inf_neg"))
    _check(prod, orc, stream, COLS4, ALL_AGGS, w, SUM_X4)


# ------------------------------------------------------------------ the value pipeline

QUERIES = {
    # the specialised merges: PM_C3 (exactly these four of one DOUBLE), PM_C5 (SUM of one BIGINT)
    "c3_f64": (["x"], [("SUM", 0), ("AVG", 0), ("MIN", 0), ("MAX", 0)], 0),
    "sum_i64": (["i64"], [("SUM", 0)], None),
    # the generic planes
    "all_f64": (["x"], [("COUNT_STAR", -1), ("COUNT", 0), ("SUM", 0), ("MIN", 0), ("MAX", 0), ("AVG", 0)], 2),
    "all_i64": (["i64"], [("COUNT_STAR", -1), ("COUNT", 0), ("SUM", 0), ("MIN", 0), ("MAX", 0), ("AVG", 0)], None),
    "sumavg_i32": (["i32"], [("SUM", 0), ("AVG", 0)], None),
}
PIPE_WINDOWS = {"tumbling": dict(window_kind="TUMBLING", size_ms=5000, grace_ms=2000),
                "hop3": dict(window_kind="HOPPING", size_ms=6000, advance_ms=2000, grace_ms=2000)}
PIPE_CASES = [(q, e) for q in ("c3_f64", "all_f64") for e in SCALES] + \
             [(q, 0) for q in ("sum_i64", "all_i64", "sumavg_i32")]


@pytest.mark.parametrize("win", list(PIPE_WINDOWS))
@pytest.mark.parametrize("query,e", PIPE_CASES)
def test_value_pipeline(prod, orc, query, e, win):
    """test_gpu_offset.py::test_value_pipeline's shape (100,000 rows a push, 20,000 keys, capacity
    hint 3,000,000, in order within the 2 s grace): the three pushes of the special groups and a
    fourth after the stream-time jump, all of which must take the pipeline.  HOPPING 6 s / 2 s
    goes through panes and their fold."""
    cols, aggs, sum_agg = QUERIES[query]
    w = PIPE_WINDOWS[win]
    stream = exact_ref.make_stream(np.random.default_rng(4000 + e + len(query) + len(win)), 4, 100_000, 20_000, e,
                                   2000, 500, jump=JUMP)
    kt = _check(prod, orc, stream, cols, aggs, w, sum_agg, model=win == "tumbling", hint=3_000_000)
    assert kt["c1_pushes"] == 4 and kt["c1_declined"] == 0, kt


WIDE_WINDOW = dict(window_kind="TUMBLING", size_ms=5000, grace_ms=60_000)


@pytest.mark.parametrize("query,e", [("c3_f64", e) for e in SCALES] + [("sum_i64", 0)])
def test_value_pipeline_wide_identity(prod, orc, query, e):
    """test_gpu_c1v.py::test_c1v_wide_identity's shape: keys spread over 2^30 with 400,000 rows a
    push and several windows per push, so (key - kmin) << window bits needs the 64-bit identities
    in every push.  k_c1_check takes the 32-bit identities while kbits + wbits (+ the pane flag)
    <= 31, kbits = bits of the push's key range, wbits = bits of (last - first window index) of
    the push's records and the live resident rows.  Here kbits = 30 and every push's exact-class
    rows lie over 40 s + 2 s = 9 windows of 5 s (all within the 60 s grace, so the pipeline takes
    them in any order), wbits = 4: 34 > 31, asserted below from the stream itself for the three
    pushes that carry the special groups; the fourth, after the jump, spans more.  The special
    groups stay in the window [40 s, 45 s).  Pushes P1 .. P3 and the jump make four where
    test_c1v_wide_identity has two."""
    cols, aggs, sum_agg = QUERIES[query]
    rng = np.random.default_rng(5000 + e)
    pool = np.unique(rng.integers(0, 1 << 30, 21_000))[:20_000 + 64]
    rng.shuffle(pool)
    stream = exact_ref.make_stream(rng, 4, 400_000, 20_000, e, 2000, 0, jump=JUMP, key_pool=pool, t0=40_000,
                                   spread=40_000)
    for d in stream.pushes[:3]:
        kbits = int(d["keys"].max() - d["keys"].min()).bit_length()
        wbits = int(d["ts"].max() // 5000 - d["ts"].min() // 5000).bit_length()
        assert kbits + wbits > 31, (kbits, wbits)
    kt = _check(prod, orc, stream, cols, aggs, WIDE_WINDOW, sum_agg, model=True, hint=3_000_000)
    assert kt["c1_pushes"] == 4 and kt["c1_declined"] == 0, kt


@pytest.mark.parametrize("e", SCALES)
def test_pipeline_declined_one_column_path(prod, orc, e):
    """test_gpu_c1v.py::test_c1v_declines' shape (200,000 rows a push, 20,000 keys, HOPPING 6 s / 2 s
    with grace 0 and disorder across window ends): the pipeline declines the first push and the
    general merge's one-column update path runs C3's aggregate list."""
    cols, aggs, sum_agg = QUERIES["c3_f64"]
    w = dict(window_kind="HOPPING", size_ms=6000, advance_ms=2000, grace_ms=0)
    stream = exact_ref.make_stream(np.random.default_rng(6000 + e), 3, 200_000, 20_000, e, 2000, 1500, jump=JUMP,
                                   jump_half=True, t0=101_000)
    kt = _check(prod, orc, stream, cols, aggs, w, sum_agg, hint=2_000_000)
    assert kt["c1_declined"] >= 1 and kt["c1_pushes"] == 0, kt


# ------------------------------------------------------------------ SESSION windows

@pytest.mark.parametrize("e", SCALES)
@pytest.mark.parametrize("emit,win", [("CHANGES", dict(size_ms=5_000, grace_ms=10_000)),
                                      ("CHANGES", dict(size_ms=20_000, grace_ms=-1)),
                                      ("FINAL", dict(size_ms=5_000, grace_ms=10_000)),
                                      ("FINAL", dict(size_ms=20_000, grace_ms=0))])
def test_sessions(prod, orc, emit, win, e):
    """The SESSION engine (gaps and grace periods of test_gpu_emit.py), ALL_AGGS: a key's session
    grows over the pushes (each push merges the resident session into the new one), the jump
    starts new sessions and, with EMIT FINAL, emits the closed ones."""
    w = dict(win, window_kind="SESSION")
    stream = exact_ref.make_stream(np.random.default_rng(7000 + e + win["size_ms"]), 3, 20_000, 300, e, 2000, 500,
                                   jump=JUMP, jump_half=True)
    _check(prod, orc, stream, COLS4, ALL_AGGS, w, SUM_X4, emit=emit)


# ------------------------------------------------------------------ table source

TAGG_AGGS = [("COUNT_STAR", -1), ("COUNT", 0), ("SUM", 0), ("AVG", 0)]


def _table_results(orc_snap, gkey):
    return {name: [orc_snap["values"][a][np.flatnonzero(orc_snap["key"] == k)[0]] for a in range(len(TAGG_AGGS))]
            for name, k in gkey.items() if (orc_snap["key"] == k).any()}


@pytest.mark.parametrize("e", SCALES)
def test_table_source(prod, orc, e):
    """khip_agg_push_table at test_tagg.py's shape (5 pushes of 20,000 - 60,000 changes, 8,000
    PRIMARY KEYs, 300 groups): keys move between groups, are deleted and repeat inside one push; a
    key's intermediate row inside one push holds +Inf, another's a NaN (the reference adds and
    undoes them one by one: a sticky NaN), a stored +Inf / -Inf is replaced or moved away, -0.0
    rows, subnormal rows, an overflow to +Inf.  The table after every push and the HAVING count
    against the oracle; the random groups also against the closed form."""
    log, gkey = exact_ref.table_changelog(np.random.default_rng(8000 + e), 5, 8000, 300, e)
    having = {"agg": 2, "op": "GT", "value": 0.0}
    kw = dict(window_kind="NONE", key_type="INT64", col_types=["DOUBLE"], aggs=TAGG_AGGS, having=having)
    g = abi.AggHandle(prod, abi.make_agg_desc(flags=abi.FLAG_TABLE_SOURCE, **kw))
    o = abi.AggHandle(orc, abi.make_agg_desc(flags=abi.FLAG_TABLE_SOURCE, **kw))
    for p, push in enumerate(log):
        gs, os_ = g.push_table(push["batch"], **push["src"]), o.push_table(push["batch"], **push["src"])
        assert gs == os_, (p, gs, os_)
        snap, osnap = g.snapshot(), o.snapshot()
        # the oracle gives what the changelog was built for (the test's own check of its input)
        r = _table_results(osnap, gkey)
        if p >= 1:
            assert np.isnan(r["inf_mid"][2]) and np.isnan(r["nan_mid"][2]) and np.isnan(r["inf_move_from"][2])
            assert r["finite_mid"][2] == np.ldexp(12.0, e) and r["inf_move_to"][2] == np.ldexp(8.0, e)
        assert r["overflow"][2] == np.inf and np.isnan(r["inf_stored"][2]) == (p >= 2)
        assert r["neg_zero"][2] == 0 and not np.signbit(r["neg_zero"][2])
        assert 0 < abs(r["subnormal_a"][2]) < 2.3e-308
        assert_exact(snap, osnap, "table after push %d" % p)
        assert g.count_rows(having) == o.snapshot(having)["n"], "HAVING count after push %d" % p
        star, cnt, s, avg = exact_ref.table_model(log, 300, p)
        rows = np.flatnonzero(snap["key"] < 300)
        k = snap["key"][rows]
        for a, want in enumerate((star, cnt, s, avg)):
            got = snap["values"][a][rows]
            assert np.array_equal(exact_ref.bits(got), exact_ref.bits(want[k].astype(got.dtype))), (p, TAGG_AGGS[a])
    keys = np.array(sorted(gkey.values()), np.int64)
    assert_exact(g.get(keys=keys), exact_ref.rows_of_keys(o.snapshot(), keys), "pull query of the planted groups")
    g.close()
    o.close()
