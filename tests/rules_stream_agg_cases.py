"""Streaming rule sets of more than 16 queries whose selects aggregate (sum / avg /
count per (rule, card)): the cases of tests/rules_stream_cases.py with the select
rewritten. Shared by the CPU test of the cases and of the sequential walk, and by
the GPU parity tests of the carried aggregate pass."""
from fractions import Fraction

import numpy as np

from rules_stream_cases import S1, S2, S3, S5, assert_rows_equal, calls_of, compiled, oracle_rows, stream_data

PLAIN = "e2.amount as amount"
SEL_SUM_AVG = "sum(e2.amount) as total, avg(e1.amount) as a1"
SEL_COUNT_SUM = "count() as n, sum(e2.merchant) as ms"
# the same rows with the aggregators' arguments in their columns
ARGS_SUM_AVG = "e2.amount as total, e1.amount as a1"
ARGS_COUNT_SUM = "e2.merchant as n, e2.merchant as ms"

# (name, base case, select, arguments select, amounts scaled)
A1 = ("A1", S2, SEL_SUM_AVG, ARGS_SUM_AVG, False)
A2 = ("A2", S1, SEL_COUNT_SUM, ARGS_COUNT_SUM, False)
A3 = ("A3", S3, SEL_SUM_AVG, ARGS_SUM_AVG, False)   # unpartitioned: one key
A4 = ("A4", S2, SEL_SUM_AVG, ARGS_SUM_AVG, True)
A5 = ("A5", S5, SEL_SUM_AVG, ARGS_SUM_AVG, True)    # one card
AGG_CASES = [A1, A2, A3, A4, A5]
# oracle rows, (query, key) segments, rows of the longest segment
EXPECTED = {"A1": (5252, 51, 261), "A2": (1675, 797, 11), "A3": (2208, 19, 1089), "A4": (7646, 51, 194),
            "A5": (10578, 18, 620)}
N_VALUES = 3  # card, and two aggregates

# aggregate layout of the two selects, as the C-ABI numbers them (include/sh_query.h)
SH_T_INT, SH_T_FLOAT = 1, 3
SH_AGG_SUM, SH_AGG_AVG, SH_AGG_COUNT = 1, 2, 3
LAYOUT = {SEL_SUM_AVG: [(1, SH_AGG_SUM, SH_T_FLOAT), (2, SH_AGG_AVG, SH_T_FLOAT)],
          SEL_COUNT_SUM: [(1, SH_AGG_COUNT, SH_T_INT), (2, SH_AGG_SUM, SH_T_INT)]}


def agg_data(ac):
    """(aggregating text, arguments text, data) of a case"""
    name, base, select, args, scaled = ac
    text, rules, data = stream_data(base)
    assert text.count(PLAIN) == base[2]
    ts, card, amount, merchant = data
    if scaled:
        k = np.random.default_rng(700).integers(-40, 41, len(amount))
        amount = (amount * np.exp2(k).astype(np.float32)).astype(np.float32)
    return text.replace(PLAIN, select), text.replace(PLAIN, args), (ts, card, amount, merchant)


_cache = {}


def agg_ref(ac):
    """a case's text, data, calls and oracle rows at its drain cadence, computed once"""
    name, base = ac[0], ac[1]
    if name not in _cache:
        text, args_text, data = agg_data(ac)
        calls = calls_of(base, data)
        _cache[name] = (text, data, calls, oracle_rows(base, text, calls, base[5]))
    return _cache[name]


def args_rows(ac):
    """the oracle's rows of the arguments text: the same matches, projection only"""
    name, base = ac[0], ac[1]
    if (name, "args") not in _cache:
        text, args_text, data = agg_data(ac)
        calls = calls_of(base, data)
        _cache[(name, "args")] = oracle_rows(base, args_text, calls, base[5])
    return _cache[(name, "args")]


def row_keys(ac, rows):
    """the partition key of every row's trigger event (0 when unpartitioned)"""
    base = ac[1]
    card = agg_ref(ac)[1][1]
    if not base[7]:
        return np.zeros(len(rows["seq"]), np.int32)
    return card[rows["seq"].astype(np.int64)].astype(np.int32)


def row_groups(ac, rows):
    """the drain group every row came out in"""
    base = ac[1]
    return (rows["seq"].astype(np.int64) // base[4]) // base[5]


def segments(ac, rows):
    """{(query, key): row indices in output order}"""
    key = row_keys(ac, rows)
    segs = {}
    for i, (q, k) in enumerate(zip(rows["query"].tolist(), key.tolist())):
        segs.setdefault((q, k), []).append(i)
    return segs


def as_double(bits):
    return np.asarray(bits, np.int64).view(np.float64)


def is_float32(x):
    """x (a Fraction) is a float32 value"""
    try:
        f = np.float32(float(x))
    except OverflowError:
        return False
    return bool(np.isfinite(f)) and Fraction(float(f)) == x


def rounded_additions(ac, rows, col=1):
    """additions of the running float sum in `col` that rounded: the exact difference
    of consecutive running values of a segment is not the float32 that was added"""
    tot = as_double(rows["values"][:, col])
    n = 0
    for idx in segments(ac, rows).values():
        prev = Fraction(0)
        for i in idx:
            if not np.isfinite(tot[i]):
                break
            cur = Fraction(float(tot[i]))
            if not is_float32(cur - prev):
                n += 1
            prev = cur
    return n


def assert_agg_rows_equal(got, ref):
    """exact, every value column: this path has no tolerance"""
    assert_rows_equal(got, ref)
    for c in range(N_VALUES):
        assert np.array_equal(got["values"][:, c], ref["values"][:, c]), ("values", c)
