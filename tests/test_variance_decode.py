"""The STDDEV decode (ksql_amd/csrc/khip_variance.hpp, compiled here for the host with g++ through
tools/variance_check.cpp, once plainly and once with -fsanitize=undefined,address) against the
exact Python model of tests/stddev_ref.py, bit for bit: the state words rebuilt into T and Q with
carries, n Q - T² in 192 bits, the division by n rounded once half to even.  CPU only."""
import os
import random
import subprocess

import pytest

import stddev_ref as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
I64_MIN, I64_MAX = -2**63, 2**63 - 1


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("var") / ("varcheck_" + request.param))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-o", exe, os.path.join(REPO, "tools", "variance_check.cpp")])

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        return [int(x) for x in p.stdout.split()]
    return run


def words(typ, xs):
    """The state words the engines keep for the non-null arguments xs: every word the wrapped u64
    sum of its per-record pieces (khip_variance.hpp)."""
    big = typ == "INT64"
    s = sum(xs) & M64
    hi = sum(x >> 32 for x in xs) & M64 if big else 0
    sq = [0, 0, 0, 0]
    for x in xs:
        q = x * x
        for j in range(4 if big else 2):
            sq[j] = (sq[j] + ((q >> (32 * j)) & 0xFFFFFFFF)) & M64
    return len(xs), s, hi, sq


def state_words(typ, n, T, Q_limbs):
    """Words of a synthetic state: n records, true sum T, limb sums Q_limbs (each < 2^64)."""
    big = typ == "INT64"
    if not big:
        return n, T & M64, 0, list(Q_limbs) + [0, 0]
    # T = hi * 2^32 + low with 0 <= low < 2^64: any split does, as the engines' sums are one
    hi = T >> 32
    return n, T & M64, hi & M64, list(Q_limbs)


def line(sample, typ, n, s, hi, sq):
    return "%d %d %d %d %d %d %d %d %d" % (sample, typ == "INT64", n, s, hi, sq[0], sq[1], sq[2], sq[3])


def check(checker, cases):
    """cases: (typ, xs).  Both kinds of every case against the model."""
    lines, want = [], []
    for typ, xs in cases:
        w = words(typ, xs)
        for sample, kind in enumerate(sr.KINDS):
            lines.append(line(sample, typ, *w))
            want.append(sr.bits(sr.model(kind, xs)) & M64)
    got = checker(lines)
    assert len(got) == len(want)
    for i, (g, e) in enumerate(zip(got, want)):
        assert g == e, (cases[i // 2][0], cases[i // 2][1][:6], len(cases[i // 2][1]), sr.KINDS[i % 2], g, e)


def test_random_states(checker):
    rng = random.Random(3)
    cases = []
    for g in range(3000):
        typ = sr.TYPES[g % 2]
        lim = 31 if typ == "INT32" else 63
        b = rng.randint(1, lim)
        n = rng.choice([2, 3, 4, 7, 31, 200])
        base = rng.randint(-(1 << b), (1 << b) - 1)
        spread = 1 << rng.randint(0, b)
        clamp = lambda v: max(-(1 << lim), min((1 << lim) - 1, v))  # noqa: E731
        cases.append((typ, [clamp(base + rng.randrange(spread)) if rng.random() < 0.7 else rng.randint(-(1 << b), (1 << b) - 1)
                            for _ in range(n)]))
    check(checker, cases)


def test_small_counts_and_equal_values(checker):
    cases = []
    for typ, ext in (("INT32", [-2**31, 2**31 - 1, 0, -1, 12345]), ("INT64", [I64_MIN, I64_MAX, 0, -1, 2**40, -2**62])):
        cases.append((typ, []))
        for x in ext:
            cases.append((typ, [x]))
            cases.append((typ, [x] * 1000))  # all equal: M2 = 0
            for y in ext:
                cases.append((typ, [x, y]))
    check(checker, cases)


def test_words_near_the_limit(checker):
    """2^32 - 1 records of an extreme value, as words (no list that long): every limb word near
    2^64 - 1, T at ±2^63 (2^32 - 1) and its neighbours, mixtures of the two extremes."""
    n = 2**32 - 1
    lines, want = [], []
    for typ, lo, hi in (("INT32", -2**31, 2**31 - 1), ("INT64", I64_MIN, I64_MAX)):
        for k in (0, 1, 2, n // 2, n - 1, n):  # k records at lo, n - k at hi
            T, Q = k * lo + (n - k) * hi, k * lo * lo + (n - k) * hi * hi
            limbs = []
            for j in range(4 if typ == "INT64" else 2):
                limbs.append((k * ((lo * lo >> (32 * j)) & 0xFFFFFFFF) + (n - k) * ((hi * hi >> (32 * j)) & 0xFFFFFFFF)))
            assert all(v <= M64 for v in limbs) and sum(v << (32 * j) for j, v in enumerate(limbs)) == Q
            w = state_words(typ, n, T, limbs)
            for sample, kind in enumerate(sr.KINDS):
                lines.append(line(sample, typ, *w))
                want.append(sr.bits(sr.model_state(kind, n, T, Q)) & M64)
        # 0xFFFFFFFF limbs: x = 2^32 - 1 (BIGINT) squares to 0xFFFFFFFE_00000001; x with x² limbs all high
        if typ == "INT64":
            x = 0xFFFFFFFFFFFFFFFF >> 1
            w = words(typ, [x, -x, x])
            Tn, Qn = x, 3 * x * x
            assert w[0] == 3
            lines.append(line(0, typ, *w))
            want.append(sr.bits(sr.model_state("STDDEV_SAMP", 3, Tn, Qn)) & M64)
    got = checker(lines)
    assert got == want


def test_halfway_quotients_tie_to_even(checker):
    """States whose exact (n Q - T²) / n lies halfway between two doubles, in both directions.
    [0, y], y odd with a 54-bit square: D / 2 = y² / 2 = m + 1/2, and m = (y² - 1) / 2 is even (an odd
    square is 1 mod 8): the tie rounds down.  [0, 0, 2u, 2], u even: D / 4 = 3u² - 2u + 3, a 54-bit
    integer that is 3 mod 4, i.e. 2m + 1 with m odd: the tie rounds up."""
    from fractions import Fraction

    def tie(xs):  # None, or the parity of m when (n Q - T²) / n = (m + 1/2) 2^s with 53-bit m
        n, T, Q = len(xs), sum(xs), sum(x * x for x in xs)
        v = Fraction(n * Q - T * T, n)
        e = (v.numerator.bit_length() - v.denominator.bit_length()) - 54
        while v / Fraction(2) ** e >= 2 ** 53:
            e += 1
        while v / Fraction(2) ** e < 2 ** 52:
            e -= 1
        m2 = v / Fraction(2) ** e
        return int(m2) & 1 if m2 - int(m2) == Fraction(1, 2) else None

    cases, ties = [], []
    for i in range(1, 201):
        cases.append(("INT64", [0, (1 << 27) - 1 - 2 * i]))
        cases.append(("INT64", [0, 0, 2 * ((1 << 26) - 2 * i), 2]))
    ties = [tie(xs) for _, xs in cases]
    assert ties == [0, 1] * 200
    check(checker, cases)
    # wider: D = y² * 2^k stays a tie after scaling the values by 2^j
    check(checker, [("INT64", [0, ((1 << 27) - 1 - 2 * i) << 8]) for i in range(1, 200)])


def test_beyond_the_limit_does_not_fault(checker):
    """n >= 2^32 and wrapped words: the result is unspecified, the sanitizers stay silent."""
    rng = random.Random(9)
    lines = [line(s, typ, n, rng.getrandbits(64), rng.getrandbits(64), [rng.getrandbits(64) for _ in range(4)])
             for s in (0, 1) for typ in sr.TYPES for n in (2**32, 2**40 + 1, 2**63 - 1, -5, 0, 1, 2, 3) for _ in range(20)]
    assert len(checker(lines)) == len(lines)
