"""ksql_amd/csrc/khip_expr.hpp on the CPU: the scalar helpers, the program checker and the host
interpreter (the same lowered instructions and x_exec the kernels run), compiled through
tools/expr_check.cpp with g++, once plainly and once with -fsanitize=address,undefined.  Its built-in
table of edge vectors must pass, and random well-typed programs over edge rows must agree with
tests/expr_ref.py value for value, state for state and error count for error count.  CPU only."""
import os
import random
import subprocess

import numpy as np
import pytest

import expr_cases as xc
import expr_ref as xr
from ksql_amd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
TYPES = ["INT32", "INT64", "DOUBLE", "STRING", "INT64", "DOUBLE", "INT32"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("expr") / ("exprcheck_" + request.param))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-o", exe,
                           os.path.join(REPO, "tools", "expr_check.cpp")])
    return exe


def test_edge_table(checker):
    p = subprocess.run([checker, "selftest"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert p.stdout.strip() == "selftest ok"


def _signed(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def _bits(t, v):
    return _signed(xr.f64_bits(float(v))) if t == "DOUBLE" else int(v)


def test_random_programs_against_the_restatement(checker):
    rng = random.Random(11)
    n = 60
    lines, want = [], []
    for _ in range(150):
        trees = xc.random_program(rng, TYPES)
        words = abi.expr_words(*trees)
        steps, outs, has_where, has_key = xr.check(TYPES, words)
        lines.append("P %d %s %d %s" % (len(TYPES), " ".join(str(xr.TYPE[t]) for t in TYPES), len(words),
                                        " ".join(map(str, words))))
        want.append("P 0 %d %d %d" % (len(outs), has_where, has_key))
        cols, valid = xc.edge_rows(rng, TYPES, n)
        for r in range(n):
            nulls = sum(1 << c for c in range(len(TYPES)) if not valid[c][r])
            lines.append("R %d %s" % (nulls, " ".join(str(_bits(t, cols[c][r])) for c, t in enumerate(TYPES))))
            row = [(cols[c][r].item(), not valid[c][r]) for c in range(len(TYPES))]
            keep, o, key, errs = xr.eval_row(steps, row)
            exp = ["R", str(int(keep)), str(errs)]
            for c, t in enumerate(outs):
                s, v = o.get(c, (xr.VALUE, 0)) if keep else (xr.VALUE, 0)
                exp += [str(s), "0" if s != xr.VALUE else str(_bits("DOUBLE" if t == xr.DOUBLE else "INT64", v) & M64)]
            s, v = key if (keep and key is not None) else (xr.VALUE, 0)
            exp += [str(s), "0" if s != xr.VALUE else str(int(v) & M64)]
            want.append((" ".join(exp), [c for c, tr in enumerate(t for t in trees if t[0] == "OUT") if tr[1][0] != "COL"]))
    p = subprocess.run([checker], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    got = p.stdout.strip().split("\n")
    assert len(got) == len(want)
    prog = None
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, str):
            assert g.startswith(w), (lines[i], g, w)
            prog = lines[i]
            continue
        w, produced = w
        if g != w:  # a NaN that arithmetic produced: the sign and payload are the platform's
            gt, wt = g.split(), w.split()
            assert len(gt) == len(wt), (prog, lines[i], g, w)
            for j, (a, b) in enumerate(zip(gt, wt)):
                c = (j - 3) // 2
                if a != b:
                    assert j >= 3 and (j - 3) % 2 == 1 and c in produced, (prog, lines[i], g, w)
                    fa, fb = xr.bits_f64(int(a)), xr.bits_f64(int(b))
                    assert fa != fa and fb != fb, (prog, lines[i], g, w)


def test_create_time_statuses(checker):
    """The checker's status for each malformed program, against the restatement's exception."""
    C = ("COL", 0)
    w = abi.expr_words
    X = abi.X
    types = ["INT64", "STRING", "DOUBLE"]
    deep = C
    for _ in range(8):
        deep = ("ADD", C, deep)
    progs = [[], [99], [X["COL"] | (3 << 32), X["OUT"]], [X["ADD"]], w(C), w(("OUT", ("GT", C, C))), w(("WHERE", C)),
             w(("OUT", ("COL", 1))), w(("WHERE", ("IS_NULL", C)), ("WHERE", ("IS_NULL", C))),
             w(("OUT", C), ("WHERE", ("IS_NULL", C))), w(("KEY", C), ("KEY", C)), [X["CONST_I64"]],
             w(("KEY", ("COL", 2))), w(("OUT", deep)), w(*[("OUT", ("ADD", C, C))] * 22), w(("OUT", ("NEG", ("COL", 1)))),
             w(("WHERE", ("IS_NULL", ("COL", 1)))), w(("OUT", C))]
    lines, want = [], []
    for words in progs:
        lines.append("P %d %s %d %s" % (len(types), " ".join(str(xr.TYPE[t]) for t in types), len(words),
                                        " ".join(map(str, words))))
        try:
            xr.check(types, words)
            want.append(0)
        except xr.Invalid:
            want.append(-1)
        except xr.Unsupported:
            want.append(-4)
    assert sorted(set(want)) == [-4, -1, 0]
    p = subprocess.run([checker], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    got = [ln.split(" ", 5) for ln in p.stdout.strip().split("\n")]
    assert [int(g[1]) for g in got] == want, (got, want)
    assert all(len(g) == 6 and g[5] for g, s in zip(got, want) if s != 0)  # every refusal carries a message
