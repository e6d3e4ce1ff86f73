"""The CORRELATION decode (ksql_amd/csrc/khip_correlation.hpp, compiled here for the host with g++
through tools/correlation_check.cpp, once plainly and once with -fsanitize=undefined,address) against
the exact Python model of tests/correlation_ref.py, bit for bit: the state words rebuilt into Σx, Σy,
Σx², Σy², Σxy with carries and signed top parts, N, DX, DY as exact integers, each rounded once half
to even.  CPU only."""
import os
import random
import subprocess

import pytest

import correlation_ref as cr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64, M32 = (1 << 64) - 1, (1 << 32) - 1
I32_MIN, I32_MAX = -2**31, 2**31 - 1
I64_MIN, I64_MAX = -2**63, 2**63 - 1
EXT = {"INT32": (I32_MIN, I32_MAX), "INT64": (I64_MIN, I64_MAX)}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("corr") / ("corrcheck_" + request.param))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-o", exe, os.path.join(REPO, "tools", "correlation_check.cpp")])

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        return [int(x) for x in p.stdout.split()]
    return run


def pieces(typ, x, y):
    """What one pair adds to each of the 17 word positions of a checker line (pair_addend of
    csrc/khip_agg_internal.hpp restated): signed where the engines add a signed quantity."""
    big = typ == "INT64"
    p = x * y

    def sq(v):
        return [(v * v >> (32 * j)) & M32 for j in range(4 if big else 2)] + ([] if big else [0, 0])
    if big:
        sx, sy = [x & M32, x >> 32], [y & M32, y >> 32]
        sxy = [p & M32, (p >> 32) & M32, (p >> 64) & M32, p >> 96]
    else:
        sx, sy = [x, 0], [y, 0]
        sxy = [p & M32, p >> 32, 0, 0]
    out = [1] + sx + sy + sq(x) + sq(y) + sxy
    assert all(-(1 << 31) <= v <= M32 for v in out)
    return out


def words(typ, multiset):
    """multiset: (count, x, y).  The 17 words: wrapped u64 sums of the per-record pieces."""
    w = [0] * 17
    for c, x, y in multiset:
        for i, v in enumerate(pieces(typ, x, y)):
            w[i] = (w[i] + c * v) & M64
    return w


def state(multiset):
    n = sum(c for c, _, _ in multiset)
    return (n, sum(c * x for c, x, _ in multiset), sum(c * y for c, _, y in multiset), sum(c * x * x for c, x, _ in multiset),
            sum(c * y * y for c, _, y in multiset), sum(c * x * y for c, x, y in multiset))


def line(typ, w):
    return " ".join(str(v) for v in [int(typ == "INT64")] + list(w))


def check(checker, cases):
    """cases: (typ, multiset) with at most 2^32 - 1 pairs."""
    lines = [line(typ, words(typ, ms)) for typ, ms in cases]
    want = [cr.bits(cr.model_state(*state(ms))) for _, ms in cases]
    got = checker(lines)
    assert len(got) == len(want)
    for (typ, ms), g, e in zip(cases, got, want):
        assert g == e, (typ, ms[:6], len(ms), hex(g), hex(e))
    return got


def ones(pairs):
    return [(1, x, y) for x, y in pairs]


def test_random_states(checker):
    rng = random.Random(4)
    cases = []
    for g in range(3000):
        typ = cr.TYPES[g % 2]
        lo, hi = EXT[typ]
        b = rng.randint(1, 31 if typ == "INT32" else 63)
        n = rng.choice([2, 3, 4, 7, 31, 200])

        def val():
            if rng.random() < 0.15:
                return rng.choice([lo, hi, 0, -1, 1])
            return max(lo, min(hi, rng.randint(-(1 << b), (1 << b) - 1)))
        slope = rng.choice([0, 1, -1, 3, -2])
        pairs = []
        for _ in range(n):
            x = val()
            y = max(lo, min(hi, slope * x + rng.randint(-(1 << (b // 2)), 1 << (b // 2)))) if slope else val()
            pairs.append((x, y))
        cases.append((typ, ones(pairs)))
    got = check(checker, cases)
    assert sum(g != cr.NAN_BITS for g in got) > 2500 and len({g >> 63 for g in got}) == 2  # finite, both signs


def test_small_counts_and_constant_arguments(checker):
    cases = []
    for typ in cr.TYPES:
        lo, hi = EXT[typ]
        ext = [lo, hi, 0, -1, 12345]
        cases.append((typ, []))
        for x in ext:
            for y in ext:
                cases.append((typ, [(1, x, y)]))                          # n = 1
                cases.append((typ, [(1000, x, y)]))                       # all equal
                cases.append((typ, [(1, x, y), (1, y, x)]))               # n = 2
                cases.append((typ, [(3, x, 7), (2, y, 7), (1, 5, 7)]))    # constant y
                cases.append((typ, [(3, 7, x), (2, 7, y), (1, 7, 5)]))    # constant x
    got = check(checker, cases)
    assert got.count(cr.NAN_BITS) > 200 and any(g != cr.NAN_BITS for g in got)


def test_words_near_the_limit(checker):
    """2^32 - 1 pairs of the extremes, as multiplicities (no list that long): every limb word near
    2^64, the signed words near -2^63 and back."""
    n = 2**32 - 1
    cases = []
    for typ in cr.TYPES:
        lo, hi = EXT[typ]
        for k in (1, 2, n // 2, n - 1):
            cases.append((typ, [(k, lo, lo), (n - k, hi, hi)]))
            cases.append((typ, [(k, lo, hi), (n - k, hi, lo)]))
            cases.append((typ, [(k, hi, hi), (n - k, hi - 1, lo)]))
            cases.append((typ, [(k, lo, hi), (n - k - 1, lo + 1, hi - 1), (1, 0, 0)]))
        cases.append((typ, [(n // 3, lo, lo), (n // 3, hi, lo), (n - 2 * (n // 3), lo, hi)]))
    for typ, ms in cases:
        assert sum(c for c, _, _ in ms) == n
    got = check(checker, cases)
    assert all(g != cr.NAN_BITS for g in got)


def test_negative_cross_term_with_carries(checker):
    """Σxy negative: every pair's low limb is near 2^32 (p = -15: 0xFFFFFFF1), so the low-limb sums
    carry many times while the signed top word goes negative."""
    cases = []
    for typ in cr.TYPES:
        for c in (3, 70_000, 2**31):
            cases.append((typ, [(c, -3, 5), (c, 3, -5), (1, 1, 1)]))
            cases.append((typ, [(c, -3, 5), (c + 1, 4, -6), (2, 0, 1)]))
            cases.append((typ, [(c, -1, 1), (5, 2, -7)]))
    for typ, ms in cases:
        assert state(ms)[5] < 0
    got = check(checker, cases)
    assert all(g >> 63 for g in got)  # r < 0


def test_extreme_products(checker):
    """Long.MIN_VALUE x Long.MIN_VALUE = 2^126 (the one product whose top limb is 2^30), MIN x MAX, and
    the INT counterparts."""
    cases = []
    for typ in cr.TYPES:
        lo, hi = EXT[typ]
        cases += [(typ, ones([(lo, lo), (0, 0)])), (typ, ones([(lo, hi), (hi, lo)])), (typ, ones([(lo, lo), (hi, lo), (0, 5)])),
                  (typ, ones([(lo, lo), (lo, hi), (hi, lo), (hi, hi)])), (typ, ones([(lo, lo), (hi, hi)])),
                  (typ, ones([(lo, hi), (lo + 1, hi - 1), (hi, lo)])), (typ, [(70_000, lo, lo), (70_000, hi, hi), (1, lo, hi)])]
    got = check(checker, cases)
    assert got[0] == cr.bits(1.0) and got[1] == cr.bits(-1.0)


def test_halfway_values_tie_to_even(checker):
    """Two pairs (0, 0), (a, b): N = a b, DX = a², DY = b².  a and b odd with a 54-bit product and
    54-bit squares: every one of the three integers is odd with 54 bits, exactly halfway between two
    doubles.  An odd square is 1 mod 8, so those ties round down; x = [0, 0, 2u, 2], u even, gives
    DX = 4 (3u² - 2u + 3), a tie that rounds up (the 54-bit factor is 3 mod 4).  Both parities of the
    kept 53 bits occur for N and for a denominator."""
    def tie(v):  # None, or the parity of the 53 kept bits when v is halfway between two doubles
        k = v.bit_length() - 53
        return (v >> k) & 1 if k > 0 and v & ((1 << k) - 1) == 1 << (k - 1) else None

    cases, parities = [], set()
    for i in range(1, 201):
        a, b = (1 << 27) - 1 - 2 * i, (1 << 27) - 3 - 6 * i
        for x, y in ((a, b), (-a, b), (a, a)):
            N, DX, DY = cr.exact_terms(*state(ones([(0, 0), (x, y)])))
            assert None not in (tie(abs(N)), tie(DX), tie(DY))
            parities |= {("N", tie(abs(N))), ("D", tie(DX)), ("D", tie(DY))}
            cases.append(("INT64", ones([(0, 0), (x, y)])))
        u = (1 << 26) - 2 * i
        ms = ones([(0, 0), (0, 1), (2 * u, 2), (2, 3)])
        N, DX, DY = cr.exact_terms(*state(ms))
        assert tie(DX) == 1
        parities.add(("D", tie(DX)))
        cases += [("INT64", ms), ("INT64", [(c, y, x) for c, x, y in ms])]
    assert parities == {("N", 0), ("N", 1), ("D", 0), ("D", 1)}
    check(checker, cases)
    # wider: the values scaled by 2^8 keep the ties (N, DX, DY gain 16 zero bits)
    check(checker, [("INT64", ones([(0, 0), (((1 << 27) - 1 - 2 * i) << 8, ((1 << 27) - 3 - 6 * i) << 8)])) for i in range(1, 100)])


def test_beyond_the_limit_does_not_fault(checker):
    """n >= 2^32 and arbitrary wrapped words: the result is unspecified, the sanitizers stay silent."""
    rng = random.Random(9)
    lines = []
    for typ in cr.TYPES:
        for n in (2**32, 2**40 + 1, 2**63 - 1, 2**64 - 5, 0, 1, 2, 3):
            for _ in range(20):
                lines.append(line(typ, [n] + [rng.getrandbits(64) for _ in range(16)]))
            lines.append(line(typ, [n] + [M64] * 16))
            lines.append(line(typ, [n] + [1 << 63] * 16))
    assert len(checker(lines)) == len(lines)
