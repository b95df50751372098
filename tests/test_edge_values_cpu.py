"""The references of the edge-value tests, checked without a GPU.

1. A hand-written truth table pins the oracle (oracle/refcpu.cpp `cmp`, `arith`) to
   Java: binary numeric promotion (JLS 5.6.2), integer division and remainder
   (15.17.2, 15.17.3: truncation, the dividend's sign, MIN / -1 wraps, MIN % -1 is 0),
   the floating remainder (15.17.3, C's fmod), the numerical comparison and equality
   operators (15.20.1, 15.21.1: NaN is unordered, -0.0 == 0.0), and the reference's
   executors where they depart from the plain operators:
     executor/condition/compare/equal/EqualCompareConditionExpressionExecutorFloatLong.java,
     .../LongFloat.java and notequal/NotEqual...FloatLong / LongFloat.java compare as
       double, while Equal...IntFloat.java and every ordering executor (e.g.
       greaterthan/GreaterThanCompareConditionExpressionExecutorLongFloat.java) use the
       promoted float;
     executor/math/divide/DivideExpressionExecutor{Int,Long,Float,Double}.java and
       executor/math/mod/ModExpressionExecutor*.java return null for a zero divisor,
       floating ones included (`right == 0.0f` holds for -0.0f too);
     executor/condition/compare/CompareConditionExpressionExecutor.java: a null operand
       makes the comparison false; executor/condition/NotConditionExpressionExecutor.java
       negates the Boolean it gets, so not (NaN > 20) is true.
   The expected values are derived by hand from those rules, never from an engine.
2. The NumPy restatements c2_check / c3_check / c5_check agree with the oracle on the
   edge streams the GPU tests use.
3. Every query of the shared lists gives rows on its edge stream, and other rows than
   on the same stream without the edge values."""
import numpy as np
import pytest

import edge_values as ev
from c2_check import c2_expected
from c3_check import c3_expected
from c5_check import c5_expected
from oracle_engine import OracleEngine, run_columns_oracle, run_stock_oracle
from rules_cases import card_strings
from siddhi_amd import compiler, synth

NAN, INF = float("nan"), float("inf")
FMAX, FMIN, FD, FDM = ev.FLT_MAX, ev.FLT_MIN, ev.F32_DENORM_MIN, ev.F32_DENORM_MAX
IMIN, IMAX, LMIN, LMAX = ev.INT_MIN, ev.INT_MAX, ev.LONG_MIN, ev.LONG_MAX
N20 = float(np.nextafter(np.float32(20), np.float32(np.inf)))
P20 = float(np.nextafter(np.float32(20), np.float32(-np.inf)))
F1234 = float(np.float32(12.34))     # 12.340000152587890625: above the double 12.34

TYPES = {"i": ("int", np.int32), "l": ("long", np.int64), "f": ("float", np.float32), "d": ("double", np.float64)}

# (op, left type, left value, right type, right value) -> bool
COMPARE = [
    # float, float (JLS 15.20.1 / 15.21.1)
    (">", "f", NAN, "f", 1.0, False), ("<", "f", NAN, "f", 1.0, False), ("<=", "f", 1.0, "f", NAN, False),
    (">=", "f", NAN, "f", NAN, False), ("==", "f", NAN, "f", NAN, False), ("!=", "f", NAN, "f", NAN, True),
    ("!=", "f", 1.0, "f", NAN, True),
    ("==", "f", 0.0, "f", -0.0, True), ("<", "f", -0.0, "f", 0.0, False), (">=", "f", -0.0, "f", 0.0, True),
    ("!=", "f", 0.0, "f", -0.0, False),
    (">", "f", FD, "f", 0.0, True), ("<", "f", -FD, "f", -0.0, True), (">", "f", FDM, "f", FD, True),
    ("<", "f", FDM, "f", FMIN, True), ("==", "f", FD, "f", 0.0, False), ("<=", "f", FD, "f", 0.0, False),
    (">", "f", INF, "f", FMAX, True), ("<", "f", -INF, "f", -FMAX, True), ("==", "f", INF, "f", INF, True),
    (">", "f", INF, "f", INF, False), (">=", "f", INF, "f", INF, True), ("<=", "f", -INF, "f", -INF, True),
    (">", "f", N20, "f", 20.0, True), ("<", "f", P20, "f", 20.0, True), (">=", "f", P20, "f", 20.0, False),
    ("==", "f", 16777216.0, "f", 16777218.0, False), ("<", "f", 16777216.0, "f", 16777218.0, True),
    # int, float: the int is promoted to float (5.6.2), rounding to nearest even
    ("==", "i", 16777217, "f", 16777216.0, True), (">", "i", 16777217, "f", 16777216.0, False),
    ("==", "i", IMAX, "f", 2147483648.0, True), ("<", "i", IMAX, "f", 2147483648.0, False),
    ("<", "i", IMAX - 4, "f", 2147483648.0, False),       # 2^31 - 5 rounds to 2^31 too
    (">", "i", 0, "f", -0.0, False), ("==", "i", 0, "f", -0.0, True), (">", "i", 1, "f", NAN, False),
    ("!=", "i", 1, "f", NAN, True), (">", "i", IMIN, "f", -INF, True), ("<", "i", IMIN, "f", -INF, False),
    (">", "i", 1, "f", FDM, True), ("<", "f", FD, "i", 1, True), (">", "f", FD, "i", 0, True),
    # long, float: orderings in float; == and != as double (the FloatLong / LongFloat executors)
    (">", "l", 2 ** 24 + 1, "f", 16777216.0, False), (">=", "l", 2 ** 24 + 1, "f", 16777216.0, True),
    ("==", "l", 2 ** 24 + 1, "f", 16777216.0, False), ("!=", "l", 2 ** 24 + 1, "f", 16777216.0, True),
    ("==", "f", 16777216.0, "l", 2 ** 24 + 1, False), ("!=", "f", 16777216.0, "l", 2 ** 24 + 1, True),
    ("<", "f", 16777216.0, "l", 2 ** 24 + 1, False),
    ("==", "l", 2 ** 53 + 1, "f", 9007199254740992.0, True),   # (double)(2^53 + 1) is 2^53
    (">=", "l", LMAX, "f", 9223372036854775808.0, True), (">", "l", LMAX, "f", 9223372036854775808.0, False),
    ("==", "l", LMAX, "f", 9223372036854775808.0, True), ("<", "l", LMIN, "f", -INF, False),
    ("==", "l", LMIN, "f", -9223372036854775808.0, True), ("!=", "l", 0, "f", -0.0, False),
    ("!=", "l", -1, "f", NAN, True), ("==", "l", -1, "f", NAN, False),
    # long, double and int, double
    ("==", "l", 2 ** 53 + 1, "d", 9007199254740992.0, True), (">", "l", 2 ** 53 + 1, "d", 9007199254740992.0, False),
    ("<", "l", -(2 ** 53 + 1), "d", -9007199254740992.0, False),
    ("<", "l", LMAX, "d", 9223372036854775808.0, False), ("==", "l", LMAX, "d", 9223372036854775808.0, True),
    ("<", "l", 2 ** 62, "d", 1e300, True),
    ("==", "i", 16777217, "d", 16777217.0, True), (">", "i", 16777217, "d", 16777216.0, True),
    ("<", "i", IMIN, "d", -1e300, False),
    # float, double: the float widens exactly
    ("==", "f", F1234, "d", 12.34, False), (">", "f", F1234, "d", 12.34, True), ("==", "f", FD, "d", FD, True),
    ("<", "f", FMAX, "d", 1e300, True), ("==", "f", INF, "d", INF, True), (">", "d", 1e300, "f", INF, False),
    ("==", "f", NAN, "d", NAN, False), ("==", "d", 0.0, "f", -0.0, True), (">", "d", 5e-324, "f", 0.0, True),
    ("<", "d", 5e-324, "f", FD, True),
    # double, double
    ("==", "d", 2.0 ** 53, "d", 2.0 ** 53 + 2, False), ("<", "d", 2.0 ** 53, "d", 2.0 ** 53 + 2, True),
    (">", "d", 5e-324, "d", 0.0, True), ("!=", "d", NAN, "d", NAN, True), ("<=", "d", NAN, "d", INF, False),
    (">", "d", 2.0 ** -25, "d", 0.0, True), ("<", "d", -ev.DBL_MAX, "d", -INF, False),
    ("==", "d", -0.0, "d", 0.0, True), (">", "d", ev.F64_DENORM_MAX, "d", ev.DBL_MIN, False),
    # integers
    (">", "i", IMAX, "i", IMIN, True), ("<", "i", IMIN, "i", -1, True), ("==", "i", -1, "i", -1, True),
    ("<", "i", IMIN, "i", IMIN + 1, True), (">=", "i", IMAX - 4, "i", IMAX, False),
    ("==", "i", -1, "l", -1, True), (">", "i", IMIN, "l", LMIN, True), ("<", "i", IMAX, "l", 2 ** 62, True),
    ("==", "i", 0, "l", 2 ** 32, False), ("!=", "i", -1, "l", 2 ** 32 - 1, True),
    (">", "l", LMAX, "l", LMIN, True), (">=", "l", LMIN, "l", LMIN, True), ("<", "l", 2 ** 53 + 1, "l", 2 ** 62, True),
    ("<", "l", -1, "l", 0, True),
]

# (op, left type, left value, right type, right value) -> (result type, value) | None (null)
ARITH = [
    # int: two's-complement wrap-around (15.17.1, 15.18.2), truncating division, the dividend's sign
    ("+", "i", IMAX, "i", 1, ("i", IMIN)), ("-", "i", IMIN, "i", 1, ("i", IMAX)),
    ("*", "i", IMIN, "i", -1, ("i", IMIN)), ("*", "i", IMAX, "i", 2, ("i", -2)),
    ("/", "i", IMIN, "i", -1, ("i", IMIN)), ("%", "i", IMIN, "i", -1, ("i", 0)),
    ("/", "i", -5, "i", 2, ("i", -2)), ("%", "i", -5, "i", 3, ("i", -2)), ("%", "i", 5, "i", -3, ("i", 2)),
    ("/", "i", -1, "i", 2, ("i", 0)), ("%", "i", -2, "i", 3, ("i", -2)), ("/", "i", IMAX, "i", -1, ("i", -IMAX)),
    ("/", "i", 1, "i", 0, None), ("%", "i", 1, "i", 0, None), ("/", "i", 0, "i", 0, None),
    ("+", "i", IMAX - 4, "i", 5, ("i", IMIN)),
    # long
    ("+", "l", LMAX, "l", 1, ("l", LMIN)), ("-", "l", LMIN, "l", 1, ("l", LMAX)),
    ("*", "l", 2 ** 62, "l", 2, ("l", LMIN)), ("*", "l", LMAX, "l", 2, ("l", -2)),
    ("/", "l", LMIN, "l", -1, ("l", LMIN)), ("%", "l", LMIN, "l", -1, ("l", 0)),
    ("%", "l", -5, "l", 3, ("l", -2)), ("/", "l", 5, "l", 0, None), ("%", "l", 5, "l", 0, None),
    ("*", "l", 2 ** 53 + 1, "l", 2 ** 53 + 1, ("l", ((2 ** 53 + 1) ** 2 + 2 ** 63) % 2 ** 64 - 2 ** 63)),
    # int with long: promoted to long, no int wrap
    ("+", "i", IMAX, "l", 1, ("l", 2 ** 31)), ("*", "i", IMIN, "l", -1, ("l", 2 ** 31)),
    ("/", "i", IMIN, "l", -1, ("l", 2 ** 31)),
    # float (15.17, IEEE 754 round to nearest even, gradual underflow)
    ("*", "f", FMAX, "f", 2.0, ("f", INF)), ("+", "f", FMAX, "f", FMAX, ("f", INF)),
    ("-", "f", INF, "f", INF, ("f", NAN)), ("*", "f", INF, "f", 0.0, ("f", NAN)),
    ("+", "f", 16777216.0, "f", 1.0, ("f", 16777216.0)), ("+", "f", 16777218.0, "f", 1.0, ("f", 16777220.0)),
    ("*", "f", FD, "f", 0.5, ("f", 0.0)), ("*", "f", -FD, "f", 0.5, ("f", -0.0)),
    ("/", "f", FMIN, "f", 2.0, ("f", 2.0 ** -127)), ("-", "f", FMIN, "f", FDM, ("f", FD)),
    ("+", "f", -0.0, "f", 0.0, ("f", 0.0)), ("+", "f", -0.0, "f", -0.0, ("f", -0.0)),
    ("/", "f", 0.0, "f", -INF, ("f", -0.0)), ("/", "f", 1.0, "f", INF, ("f", 0.0)),
    ("/", "f", 1.0, "f", 0.0, None), ("/", "f", 1.0, "f", -0.0, None), ("%", "f", 5.5, "f", 0.0, None),
    ("/", "f", NAN, "f", 0.0, None),
    ("%", "f", -5.5, "f", 2.0, ("f", -1.5)), ("%", "f", 5.5, "f", -2.0, ("f", 1.5)),
    ("%", "f", 5.5, "f", INF, ("f", 5.5)), ("%", "f", INF, "f", 2.0, ("f", NAN)),
    ("%", "f", -4.0, "f", 2.0, ("f", -0.0)), ("%", "f", FD, "f", 1.0, ("f", FD)),
    ("+", "i", 16777217, "f", 0.0, ("f", 16777216.0)), ("*", "l", LMAX, "f", 1.0, ("f", 9223372036854775808.0)),
    ("-", "i", 0, "f", 0.0, ("f", 0.0)),
    # double
    ("*", "f", FMAX, "d", 1e30, ("d", FMAX * 1e30)),    # finite: the product is a double product
    ("*", "d", 1e300, "d", 1e300, ("d", INF)), ("+", "d", 2.0 ** 53, "d", 1.0, ("d", 2.0 ** 53)),
    ("+", "d", 2.0 ** 53 + 2, "d", 1.0, ("d", 2.0 ** 53 + 4)),
    ("/", "d", 1.0, "d", 0.0, None), ("%", "d", 1.0, "d", -0.0, None),
    ("%", "d", -12.5, "d", 5.0, ("d", -2.5)), ("+", "l", 2 ** 53 + 1, "d", 0.0, ("d", 2.0 ** 53)),
    ("*", "d", 5e-324, "d", 0.5, ("d", 0.0)), ("-", "d", INF, "d", INF, ("d", NAN)),
    ("*", "f", F1234, "d", 1.0, ("d", F1234)), ("/", "d", ev.DBL_MIN, "d", 2.0, ("d", 2.0 ** -1023)),
    ("+", "d", 2.0 ** -25, "d", 1.0, ("d", 1.0 + 2.0 ** -25)),
]


def test_constants_match_the_compiler():
    assert (ev.FLOAT, ev.DOUBLE) == (compiler.FLOAT, compiler.DOUBLE)
    assert ev.F32_POOL.dtype == np.float32 and np.isnan(ev.F32_POOL[0]) and np.signbit(ev.F32_POOL[4])
    assert float(ev.F32_POOL[5]) == 2.0 ** -149 and float(ev.F32_POOL[7]) + 2.0 ** -149 == ev.FLT_MIN
    assert int(ev.I64_POOL[0]) == ev.LONG_MIN and int(ev.I32_POOL[0]) == ev.INT_MIN


def test_canon_maps_only_nans():
    f = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000], np.int64)
    d = np.array([0x7FF8000000000000, -0x8000000000000, 0x7FF0000000000001, 0, -2 ** 63, 0x7FF0000000000000], np.int64)
    i = np.array([0x7FC00000, -1, 0x7F800001, 0, ev.LONG_MIN, 5], np.int64)
    c = ev.canon(np.stack([f, d, i], axis=1), [compiler.FLOAT, compiler.DOUBLE, compiler.LONG])
    assert c[:, 0].tolist() == [ev.QNAN32] * 3 + [0, 0x80000000, 0x7F800000]
    assert c[:, 1].tolist() == [ev.QNAN64] * 3 + [0, -2 ** 63, 0x7FF0000000000000]
    assert c[:, 2].tolist() == i.tolist()
    assert ev.canon_obj(0.0) != ev.canon_obj(-0.0) and ev.canon_obj(NAN) == ev.canon_obj(-NAN)


def test_salt_replaces_its_share_and_keeps_the_rest():
    col = np.arange(10_000, dtype=np.float32) + 100
    s = ev.salt(col, share=0.25, rng=np.random.default_rng(1))
    hit = s != col
    assert 0.2 < hit.mean() < 0.3 and col[0] == 100
    bits = set(s[hit].view(np.uint32).tolist())
    assert bits == set(ev.F32_POOL.view(np.uint32).tolist())   # every pool value is drawn, -0.0 and NaN too


def _run_pairs(text, lt, lvals, rt, rvals):
    eng = OracleEngine(compiler.compile_app(text))
    eng.start()
    n = len(lvals)
    cols = [np.array(lvals, dtype=TYPES[lt][1]), np.array(rvals, dtype=TYPES[rt][1])]
    eng.send(0, np.arange(n, dtype=np.int64) + 1000, cols, [None, None], None, 0)
    out = eng.drain()
    types = compiler.compile_app(text).queries[0].out_types
    eng.close()
    return out, types


def _groups(table):
    g = {}
    for row in table:
        g.setdefault((row[0], row[1], row[3]), []).append(row)
    return sorted(g.items())


@pytest.mark.parametrize("key,rows", _groups(COMPARE), ids=["".join(k) for k, _ in _groups(COMPARE)])
def test_compare_truth_table(key, rows):
    """one one-state pattern per (operator, left type, right type); event i passes iff row i says true"""
    op, lt, rt = key
    text = (f"define stream S (a {TYPES[lt][0]}, b {TYPES[rt][0]}); "
            f"@info(name = 'query1') from every e1=S[a {op} b] select e1.a as a insert into Out;")
    out, _ = _run_pairs(text, lt, [r[2] for r in rows], rt, [r[4] for r in rows])
    passed = set(int(s) for s in out["seq"])
    for i, r in enumerate(rows):
        assert (i in passed) == r[5], r
    # and negated: not (a op b) is the Boolean's complement (NotConditionExpressionExecutor)
    text = text.replace(f"S[a {op} b]", f"S[not (a {op} b)]")
    out, _ = _run_pairs(text, lt, [r[2] for r in rows], rt, [r[4] for r in rows])
    passed = set(int(s) for s in out["seq"])
    for i, r in enumerate(rows):
        assert (i in passed) == (not r[5]), ("not", r)


def _bits(t, v):
    if t == "f":
        return int(np.array([v], np.float32).view(np.uint32)[0])
    if t == "d":
        return int(np.array([v], np.float64).view(np.int64)[0])
    return int(v)


@pytest.mark.parametrize("key,rows", _groups(ARITH), ids=["".join(k).replace("/", "div").replace("%", "mod")
                                                          .replace("*", "mul") for k, _ in _groups(ARITH)])
def test_arith_truth_table(key, rows):
    """one projection per (operator, left type, right type): the result's type, null flag and bits"""
    op, lt, rt = key
    text = (f"define stream S (a {TYPES[lt][0]}, b {TYPES[rt][0]}); "
            f"@info(name = 'query1') from every e1=S select e1.a {op} e1.b as r insert into Out;")
    out, types = _run_pairs(text, lt, [r[2] for r in rows], rt, [r[4] for r in rows])
    assert len(out["seq"]) == len(rows)
    want_t = {"i": compiler.INT, "l": compiler.LONG, "f": compiler.FLOAT, "d": compiler.DOUBLE}
    got = ev.canon(out["values"][:, :1], types[:1])
    for i, r in enumerate(rows):
        if r[5] is None:
            assert out["nulls"][i, 0], r
            continue
        t, v = r[5]
        assert types[0] == want_t[t], r
        assert not out["nulls"][i, 0], r
        want = ev.canon(np.array([[_bits(t, v)]], np.int64), types[:1])[0, 0]
        assert int(got[i, 0]) == int(want), (r, hex(int(got[i, 0])), hex(int(want)))
    # a null operand makes every comparison false (CompareConditionExpressionExecutor)
    nulls = [i for i, r in enumerate(rows) if r[5] is None]
    if nulls:
        zero = "0" if lt in "il" and rt in "il" else "0.0"
        for cmp_op in (">", "<=", "==", "!="):
            f = text.replace("e1=S select", f"e1=S[a {op} b {cmp_op} {zero}] select")
            out, _ = _run_pairs(f, lt, [r[2] for r in rows], rt, [r[4] for r in rows])
            assert not (set(int(s) for s in out["seq"]) & set(nulls)), (cmp_op, rows)


# ------------------------------------------------------------------ restatements
def _strings(nk):
    s = compiler.StringDict()
    for i in range(nk):
        s.id(f"K{i}")
    return s


@pytest.mark.parametrize("thr,text", [(20, synth.C2_QUERY), (-1, synth.C2_QUERY.replace("price>20", "price>-1"))],
                         ids=["thr20", "thr-1"])
@pytest.mark.parametrize("shape", ["short", "kb2"])
def test_c2_restatement_on_the_edge_stream(thr, text, shape):
    """the streams of the GPU file's bucket cases `c2` and `c2_free`"""
    import test_gpu_edge_values as G
    assert f"price>{thr}]" in text
    ts, k, p, v = ev.agg_stream(*G.BUCKET_SHAPES[shape])
    seq, _, vals, _ = run_stock_oracle(compiler.compile_app(text), ts, k, p, v)
    eseq, evals = c2_expected(ts, k, p, v, thr=thr)
    assert len(seq) == len(eseq) > 0
    assert np.array_equal(seq.astype(np.int64), eseq) and np.array_equal(vals, evals)


@pytest.mark.parametrize("nk", [600, 1200])
def test_c3_restatement_on_the_edge_stream(nk):
    ts, k, p, v = ev.c3_stream(60_000, nk, "c3")
    seq, _, vals, _ = run_stock_oracle(compiler.compile_app(synth.C3_QUERY), ts, k, p, v)
    eseq, evals = c3_expected(ts, k, p)
    assert len(seq) == len(eseq) > 0
    assert np.array_equal(seq.astype(np.int64), eseq) and np.array_equal(vals, evals)


def rules_oracle(text, cards, ts, card, amount, merchant, batch=4096):
    eng = OracleEngine(compiler.compile_app(text, card_strings(cards)))
    eng.start()
    for b0 in range(0, len(ts), batch):
        b1 = min(len(ts), b0 + batch)
        eng.send(0, ts[b0:b1].copy(), [card[b0:b1].copy(), amount[b0:b1].copy(), merchant[b0:b1].copy()],
                 [None] * 3, card[b0:b1].copy(), b0)
    out = eng.drain()
    eng.close()
    return out


@pytest.mark.parametrize("variant", ["base", "int", "long"])
def test_c5_restatement_on_the_edge_streams(variant):
    """(the float-conjunct variant has no restatement: c5_check finds a rule's merchant by
    sorted search, which is equality of keys, not of float values)"""
    text, rules, (ts, card, amount, merchant) = ev.rule_set(variant)
    ref = rules_oracle(text, 400, ts, card, amount, merchant)
    eseq, erule, evals = c5_expected(ts, card, amount, merchant, rules, within_ms=1)
    assert len(ref["seq"]) == len(eseq) > 0
    assert np.array_equal(ref["seq"].astype(np.int64), eseq)
    assert np.array_equal(ref["query"], erule)
    assert np.array_equal(ref["values"][:, :2], evals)


# ------------------------------------------------------------------ row counts
def _differs(a, b):
    """rows (seq, values) of the edge stream against the ordinary one"""
    return len(a[0]) != len(b[0]) or not np.array_equal(a[0], b[0]) or not np.array_equal(a[1], b[1])


@pytest.mark.parametrize("nk", [1, 50])
@pytest.mark.parametrize("name", [q[0] for q in ev.WINDOW_QUERIES])
def test_window_queries_give_rows_that_depend_on_the_edge_values(name, nk):
    app = ev.window_query(name)
    r = {}
    for edge in (True, False):
        ts, keys, cols = ev.window_stream(20_000, nk, edge=edge)
        seq, _, vals, _ = run_columns_oracle(compiler.compile_app(app, _strings(nk)), ts, [keys] + list(cols), keys)
        r[edge] = (seq, vals)
    assert len(r[True][0]) > 0
    assert _differs(r[True], r[False])


@pytest.fixture(scope="module")
def product():
    import ctypes as C
    from siddhi_amd import abi, build
    return abi.bind_product(C.CDLL(build.build()))


@pytest.mark.parametrize("name", [q[0] for q in ev.WINDOW_QUERIES])
def test_bucket_list_is_what_the_engine_accepts(name, product):
    """BUCKET_QUERIES is every (a) query the bucketed engine generates a matcher for
    (shx_bucket_compile), and it refuses every other one as unsupported"""
    import ctypes as C
    from siddhi_amd import abi
    app = ev.window_query(name, within_ms=1000)
    d = compiler.compile_app(app, _strings(2000)).descriptor()
    h = C.c_void_p()
    assert product.sh_compile(C.byref(d), C.byref(h)) == abi.SH_OK
    rc = product.shx_bucket_compile(h, None, 0)
    err = product.sh_last_error(h)
    product.sh_destroy(h)
    assert rc == (abi.SH_OK if name in ev.BUCKET_QUERIES else abi.SH_E_UNSUPPORTED), err


@pytest.mark.parametrize("name", ev.BUCKET_QUERIES)
def test_bucket_queries_give_rows_that_depend_on_the_edge_values(name):
    """on the short bucket stream (the kb2 stream is the same generator at 200,077 events)"""
    app = ev.window_query(name, within_ms=1000)
    r = {}
    for edge in (True, False):
        ts, keys, cols = ev.bucket_stream(3 * 8192 + 17, 2000, edge=edge)
        seq, _, vals, _ = run_columns_oracle(compiler.compile_app(app, _strings(2000)), ts, [keys] + list(cols), keys)
        r[edge] = (seq, vals)
    assert len(r[True][0]) > 0
    assert _differs(r[True], r[False])


@pytest.mark.parametrize("nk", [600, 1200])
@pytest.mark.parametrize("name", list(ev.C3_QUERIES))
def test_c3_queries_give_rows_that_depend_on_the_edge_values(name, nk):
    r = {}
    for edge in (True, False):
        ts, k, p, v = ev.c3_stream(60_000, nk, name, edge=edge)
        seq, _, vals, _ = run_columns_oracle(compiler.compile_app(ev.C3_QUERIES[name]), ts, [k, p, v], k)
        r[edge] = (seq, vals)
    assert len(r[True][0]) > 0
    assert _differs(r[True], r[False])


@pytest.mark.parametrize("variant", ev.RULE_VARIANTS)
def test_rule_sets_give_rows_that_depend_on_the_edge_values(variant):
    r = {}
    for edge in (True, False):
        text, rules, (ts, card, amount, merchant) = ev.rule_set(variant, edge=edge)
        out = rules_oracle(text, 400, ts, card, amount, merchant)
        r[edge] = (out["seq"], out["values"])
        if edge:
            fired = set(out["query"].tolist())
            assert {0, 1} <= fired, fired     # the 1e30 and the 0.0 factor rules fire
    assert len(r[True][0]) > 0
    assert _differs(r[True], r[False])


@pytest.mark.parametrize("name", list(ev.GENERAL_APPS))
def test_general_apps_give_rows_that_depend_on_the_edge_values(name):
    from test_gpu_parity import _run_engine
    r = {}
    for edge in (True, False):
        rows = _run_engine(OracleEngine, ev.GENERAL_APPS[name], ev.general_sends(edge=edge))
        r[edge] = [(t, [ev.canon_obj(x) for x in d]) for t, d in rows]
    assert len(r[True]) > 0
    assert r[True] != r[False]
    if name != "and":
        assert any(None in d for _, d in r[True])   # null select values (x / 0, an absent e2[1]) occur


@pytest.mark.parametrize("text,double", [("C2_AGG", False), ("C2_AGG", True), ("free", False), ("open", False),
                                         ("open", True)])
def test_aggregate_streams_reach_the_special_sums(text, double):
    """the salted volume wraps sum(long) past LONG_MAX and the price sums overflow to
    +inf; without the threshold -inf opens partials and inf + -inf makes the avg NaN"""
    from test_gpu_agg import C2_AGG
    app = {"C2_AGG": C2_AGG, "free": ev.C2_AGG_FREE, "open": ev.C2_AGG_OPEN}[text]
    if double:
        app = app.replace("price float", "price double")
    ts, k, p, v = ev.agg_stream(*ev.AGG_SHAPE, double=double, share=ev.AGG_SHARE)
    seq, _, vals, _ = run_columns_oracle(compiler.compile_app(app), ts, [k, p, v], k)
    assert len(seq) > 0
    total = vals[:, 1].view(np.float64)
    a1 = vals[:, 2].view(np.float64)
    assert np.isinf(total).any() and np.isfinite(total).sum() > len(seq) // 2
    # sum(e2.volume) wrapped: no single volume lies in (2^62, LONG_MAX) or (LONG_MIN, -2^62)
    vol = vals[:, 4]
    assert ((vol < -(2 ** 62)) & (vol != ev.LONG_MIN)).any() and ((vol > 2 ** 62) & (vol != ev.LONG_MAX)).any()
    if text == "open":
        assert (np.isinf(a1) & (a1 < 0)).any() and np.isnan(a1).any()


def _agg_cases():
    import test_gpu_edge_values as G
    cases = {}
    for w in G.AGG_APPS:
        cases[w] = (lambda edge, w=w: G.agg_case(w, edge=edge), True)
    for w in G.AGG_EXACT_APPS:
        cases[w + "-exact"] = (lambda edge, w=w: G.agg_case(w, edge=edge, exact=True), True)
    for nm, (case, partitioned, _) in G.AGG_OTHER.items():
        cases[nm] = (lambda edge, case=case: case(edge=edge), partitioned)
        cases[nm + "-exact"] = (lambda edge, case=case: case(edge=edge, exact=True), partitioned)
    return cases


@pytest.mark.parametrize("name", list(_agg_cases()))
def test_aggregate_cases_give_rows_that_depend_on_the_edge_values(name):
    """every aggregate stream of the GPU file, the ones salted from the accepted classes
    included, against the same stream left ordinary"""
    import test_gpu_edge_values as G
    case, partitioned = _agg_cases()[name]
    r = {}
    for edge in (True, False):
        app, strings, ts, keys, cols, nk = case(edge)
        out = G._oracle(app, strings, ts, keys, cols, partitioned=partitioned)
        r[edge] = (out["seq"], out["values"])
    assert len(r[True][0]) > 0
    assert _differs(r[True], r[False])
