"""max(x) / min(x) in the select: the cases shared by the CPU tests
(tests/test_agg_minmax_cases.py) and the GPU parity tests (tests/test_gpu_agg_minmax.py).

Streaming rule sets: the cases of tests/rules_stream_cases.py with the select
rewritten (as tests/rules_stream_agg_cases.py does for sum / avg / count).

Post-pass with edge values: one window-shaped partitioned query over a stream
whose filters read only `a`, so planted NaN / signed zeros / infinities in `y` and
`d` reach the aggregators (in the C5 rule shape every rule filters on the amount it
aggregates, and a NaN never passes a filter).

The rule (MaxAttributeAggregatorExecutor / MinAttributeAggregatorExecutor
processAdd): an empty state takes the argument; otherwise the argument replaces
the state iff state < arg (max) or state > arg (min), compared in the argument's
type; the row carries the state's bits."""
import numpy as np

from rules_stream_agg_cases import PLAIN
from rules_stream_cases import S1, S2, S3, S5

SH_T_INT, SH_T_LONG, SH_T_FLOAT, SH_T_DOUBLE = 1, 2, 3, 4
SH_AGG_COUNT, SH_AGG_MAX, SH_AGG_MIN = 3, 4, 5

SEL_HI_LO = "max(e2.amount) as hi, min(e1.amount) as lo"
ARGS_HI_LO = "e2.amount as hi, e1.amount as lo"
SEL_HI_N = "max(e2.merchant) as hi, count() as n"
ARGS_HI_N = "e2.merchant as hi, e2.merchant as n"
SEL_LO_LO = "min(e2.amount) as hi, min(e1.amount) as lo"   # SEL_HI_LO with max -> min: another fingerprint

# (name, base case, select, arguments select, amounts scaled): the tuple of rules_stream_agg_cases
M1 = ("M1", S2, SEL_HI_LO, ARGS_HI_LO, False)
M2 = ("M2", S1, SEL_HI_N, ARGS_HI_N, False)
M3 = ("M3", S3, SEL_HI_LO, ARGS_HI_LO, False)   # unpartitioned: one key
M5 = ("M5", S5, SEL_HI_LO, ARGS_HI_LO, False)   # one card
MINMAX_CASES = [M1, M2, M3, M5]
LAYOUT = {SEL_HI_LO: [(1, SH_AGG_MAX, SH_T_FLOAT), (2, SH_AGG_MIN, SH_T_FLOAT)],
          SEL_HI_N: [(1, SH_AGG_MAX, SH_T_INT), (2, SH_AGG_COUNT, SH_T_INT)]}
assert PLAIN == "e2.amount as amount"

# ---- the post-pass's tiling (sh_agg.hip): rows per tile, tiles per carry iteration
SHA_TILE = 2048
SHA_CARRY_TPB = 1024

EDGE_HEAD = ("define stream S (symbol string, a float, y float, z long, w int, d double); "
             "partition with (symbol of S) begin @info(name = 'query1') "
             "from every e1=S[a>20] -> e2=S[a>e1.a] within 1 sec select e1.symbol as symbol, ")
EDGE_TAIL = " insert into Out; end;"
EDGE_TEXT = EDGE_HEAD + "max(e2.y) as hy, min(e1.y) as ly, max(e2.z) as hz, min(e2.w) as lw, max(e1.d) as hd" + EDGE_TAIL
EDGE_ARGS = EDGE_HEAD + "e2.y as hy, e1.y as ly, e2.z as hz, e2.w as lw, e1.d as hd" + EDGE_TAIL
# (row column, kind, argument type) of the five aggregates
EDGE_LAYOUT = [(1, SH_AGG_MAX, SH_T_FLOAT), (2, SH_AGG_MIN, SH_T_FLOAT), (3, SH_AGG_MAX, SH_T_LONG),
               (4, SH_AGG_MIN, SH_T_INT), (5, SH_AGG_MAX, SH_T_DOUBLE)]

MIXED_HEAD = ("define stream S (symbol string, a float, y double); "
              "partition with (symbol of S) begin @info(name = 'query1') "
              "from every e1=S[a>20] -> e2=S[a>e1.a] within 1 sec select e1.symbol as symbol, ")
MIXED_TEXT = MIXED_HEAD + "sum(e2.y) as total, max(e2.y) as hy" + EDGE_TAIL

C3_MINMAX = ("define stream S (symbol string, price float, volume long); "
             "partition with (symbol of S) begin @info(name = 'query1') "
             "from every e1=S, e2=S[price>e1.price]+, e3=S[price<e2[last].price] "
             "select e1.price as p1, max(e3.price) as hi, min(e2[last].price) as lo insert into Out; end;")


def _plant(rng, x):
    """NaN, both zeros and both infinities over about a third of x"""
    r = rng.random(len(x))
    x = x.copy()
    x[r < 0.12] = np.nan
    x[(r >= 0.12) & (r < 0.18)] = -0.0
    x[(r >= 0.18) & (r < 0.24)] = 0.0
    x[(r >= 0.24) & (r < 0.26)] = np.inf
    x[(r >= 0.26) & (r < 0.28)] = -np.inf
    return x


def edge_stream(n, K, hot, per_ms, seed):
    """(ts, key ids, a, y, z, w, d): `hot` of the events on key 0, the rest uniform"""
    rng = np.random.default_rng(seed)
    ts = (np.arange(n) // per_ms).astype(np.int64)
    k = rng.integers(1, K, n) if K > 1 else np.zeros(n, np.int64)
    k = np.where(rng.random(n) < hot, 0, k).astype(np.int32)
    a = rng.uniform(0.0, 100.0, n).astype(np.float32)
    y = _plant(rng, rng.normal(0.0, 50.0, n).astype(np.float32))
    d = _plant(rng, rng.normal(0.0, 50.0, n))
    # longs that differ only below 2^53's reach, of both signs
    big = np.int64(1) << np.int64(60)
    z = (np.where(rng.random(n) < 0.5, big, -big) + rng.integers(0, 4, n)).astype(np.int64)
    w = rng.integers(-1000, 1000, n).astype(np.int32)
    r = rng.random(n)
    w[r < 0.02] = np.iinfo(np.int32).min
    w[r > 0.98] = np.iinfo(np.int32).max
    return ts, k, a, y, z, w, d


def one_row_stream():
    """64 events over 4 keys with exactly one match (events 5 and 9 of key 1)"""
    n = 64
    ts = np.arange(n, dtype=np.int64)
    k = (np.arange(n) % 4).astype(np.int32)
    a = np.full(n, 10.0, np.float32)
    a[5], a[9] = 30.0, 40.0
    y = np.full(n, 1.0, np.float32)
    y[9], y[5] = np.nan, -0.0
    z = np.arange(n, dtype=np.int64) - 7
    w = (np.arange(n) - 30).astype(np.int32)
    d = np.linspace(-1.0, 1.0, n)
    return ts, k, a, y, z, w, d


# name -> (stream, key ids); E_BIG (a second iteration of the carry kernel) is GPU-only
E_ONE = ("E_ONE", one_row_stream, 4)
E_MAIN = ("E_MAIN", lambda: edge_stream(80_000, 4000, 0.12, 8, 5), 4000)
# (1,000 keys: under the bucketed engine's 1,024, so the projection-only arguments
# select of the GPU test runs on the window engine like the max / min select)
E_BIG = ("E_BIG", lambda: edge_stream(3_200_000, 1000, 0.0, 32, 6), 1000)

_cache = {}


def edge_data(case):
    if case[0] not in _cache:
        _cache[case[0]] = case[1]()
    return _cache[case[0]]


def edge_oracle(case, text):
    """the oracle's rows of an edge case (computed once per text)"""
    from oracle_engine import OracleEngine
    from siddhi_amd import compiler
    key = (case[0], text)
    if key not in _cache:
        ts, k, *cols = edge_data(case)
        cols = [k] + cols
        eng = OracleEngine(compiler.compile_app(text))
        eng.start()
        for b0 in range(0, len(ts), 4096):
            b1 = min(len(ts), b0 + 4096)
            eng.send(0, ts[b0:b1], [np.ascontiguousarray(c[b0:b1]) for c in cols], [None] * len(cols),
                     np.ascontiguousarray(k[b0:b1]), b0)
        _cache[key] = eng.drain()
        eng.close()
    return _cache[key]


# ---- the rule restated
def typed(raw, arg_type):
    """raw 8-byte row values -> the argument's values (float64 holds float32 exactly)"""
    raw = np.asarray(raw, np.int64)
    if arg_type == SH_T_FLOAT:
        return raw.astype(np.uint32).view(np.float32).astype(np.float64)
    if arg_type == SH_T_DOUBLE:
        return raw.view(np.float64)
    if arg_type == SH_T_INT:
        return raw.astype(np.int32).astype(np.int64)
    return raw


def extreme_sequential(values, kind):
    """index of the argument the state holds after each add: the rule itself, one
    argument at a time (Python's comparisons are IEEE on floats, exact on ints)"""
    state, out = None, []
    for i, a in enumerate(values):
        if state is None:
            state = i
        elif (values[state] < a) if kind == SH_AGG_MAX else (values[state] > a):
            state = i
        out.append(state)
    return out


def running_extreme(group, raw, kind, arg_type):
    """vectorised closed form per group, rows in output order: if the group's first
    argument is NaN every row is that NaN; otherwise row i is the earliest non-NaN
    argument up to i that attains the extreme (a later equal value, the other zero
    included, does not replace it). Returns the raw bits per row."""
    raw = np.asarray(raw, np.int64)
    n = len(raw)
    if n == 0:
        return raw.copy()
    x = typed(raw, arg_type)
    order = np.argsort(group, kind="stable")
    g = np.asarray(group)[order]
    starts = np.flatnonzero(np.r_[True, g[1:] != g[:-1]])
    lens = np.diff(np.r_[starts, n])
    gi = np.repeat(np.arange(len(starts)), lens)
    col = np.arange(n) - np.repeat(starts, lens)
    L = int(lens.max())
    fp = x.dtype == np.float64
    if kind == SH_AGG_MAX:
        pad = -np.inf if fp else np.iinfo(np.int64).min
    else:
        pad = np.inf if fp else np.iinfo(np.int64).max
    grid = np.full((len(starts), L), pad, x.dtype)
    grid[gi, col] = x[order]
    valid = np.zeros(grid.shape, bool)
    valid[gi, col] = ~np.isnan(x[order]) if fp else True
    v = np.where(valid, grid, pad)
    acc = (np.maximum if kind == SH_AGG_MAX else np.minimum).accumulate(v, axis=1)
    prev = np.c_[np.full(len(starts), pad, x.dtype), acc[:, :-1]]
    seen = np.c_[np.zeros(len(starts), bool), np.logical_or.accumulate(valid, axis=1)[:, :-1]]
    better = (v > prev) if kind == SH_AGG_MAX else (v < prev)
    record = valid & (~seen | better)   # the first value, then every strict improvement
    win = np.maximum.accumulate(np.where(record, np.arange(L)[None, :], -1), axis=1)
    head_nan = ~valid[:, 0]
    win = np.where(head_nan[:, None], 0, win)
    assert np.all(win[gi, col] >= 0)
    rgrid = np.zeros(grid.shape, np.int64)
    rgrid[gi, col] = raw[order]
    out = np.empty(n, np.int64)
    out[order] = rgrid[gi, win[gi, col]]
    return out


def tile_classes(group):
    """what the sorted layout of the rows (stable by group, as the post-pass sorts
    them) holds: (rows, longest span of one segment in tiles, most segment heads in
    one tile, segments lying inside one tile)"""
    g = np.sort(np.asarray(group), kind="stable")
    n = len(g)
    starts = np.flatnonzero(np.r_[True, g[1:] != g[:-1]])
    ends = np.r_[starts[1:], n] - 1
    span = ends // SHA_TILE - starts // SHA_TILE + 1
    heads = np.bincount(starts // SHA_TILE)
    return n, int(span.max()), int(heads.max()), int(np.sum(span == 1))
