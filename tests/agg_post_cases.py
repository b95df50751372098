"""Shared pieces of the aggregate post-pass tests (tests/test_agg_post_cases.py,
tests/test_gpu_agg_post.py): sha_running and shc_running of
siddhi_amd/csrc/sh_agg.hip called on their own, on small planted rows, and compared
bit for bit with a plain reference that shares nothing with the kernels.

Held fixed here:
  * the reference (`reference`): per (query, key) segment in row order the reference's
    own arithmetic -- np.add.accumulate from +0.0 over the `(double) x` addends (a
    left-to-right chain of IEEE additions, tests/agg_check.py), value / count for avg,
    wrap-around int64 for sum(int | long), the ordinal for count(), the first extreme
    for max / min;
  * beside it the exact running values as Python integers in units of 2^-1074
    (`exact_running`), and from those the verdict class of every case (`classify`),
    derived from the header comment of sh_agg.hip, not from its code:
      accept  every fp addend finite, per column at most 96 bits between the lowest set
              bit and the highest bit of all non-zero addends, every exact running value
              of at most 53 significant bits and below 2^1024 in magnitude: the pass
              must answer 0;
      refuse  a NaN or infinite addend in an fp column, or a sequential result that is
              not the exact running value (a rounding, or an overflow to infinity that
              the exact sum later leaves): the pass must answer 1;
      either  everything the reference computes is the exact value (an infinity where
              the exact value is at or beyond 2^1024 included), but the range is over 96
              bits or an exact value leaves the double range: 0 and 1 are both right,
              and on 0 the rows must still be the reference's;
  * the case list, as data (test_agg_post_cases.py asserts its premises).

Nothing here imports torch or touches the GPU at import time."""
import functools
import math

import numpy as np

SH_T_INT, SH_T_LONG, SH_T_FLOAT, SH_T_DOUBLE = 1, 2, 3, 4
SH_AGG_SUM, SH_AGG_AVG, SH_AGG_COUNT, SH_AGG_MAX, SH_AGG_MIN = 1, 2, 3, 4, 5
INT, LONG, FLOAT, DOUBLE = SH_T_INT, SH_T_LONG, SH_T_FLOAT, SH_T_DOUBLE
SUM, AVG, COUNT, MAX, MIN = SH_AGG_SUM, SH_AGG_AVG, SH_AGG_COUNT, SH_AGG_MAX, SH_AGG_MIN

TILE = 2048                # SHA_TILE: rows per scan tile
CARRY_THREADS = 1024       # SHA_CARRY_TPB: beyond that many tiles a carry thread walks two
MAX_COLS = 16              # SHA_MAX_COLS
QNAN64 = 0x7FF8000000000000
SCALE = 1074               # the exact values are integers in units of 2^-1074

DBL_MAX = float(np.finfo(np.float64).max)
DBL_MIN = float(np.finfo(np.float64).tiny)
DENORM = 5e-324
F32_DENORM = 2.0 ** -149
F32_DENORM_MAX = 2.0 ** -126 - F32_DENORM
INT_MIN, LONG_MAX, LONG_MIN = -2 ** 31, 2 ** 63 - 1, -2 ** 63


def is_fp(kind, arg_type):
    """a column the reference adds in doubles"""
    return kind == AVG or (kind == SUM and arg_type in (FLOAT, DOUBLE))


# ------------------------------------------------------------------ raw values
def encode(values, arg_type):
    """argument values -> the raw 8-byte row words (float bits zero-extended, double
    bits, integers sign-extended)"""
    if arg_type == FLOAT:
        return np.asarray(values, np.float32).view(np.uint32).astype(np.int64)
    if arg_type == DOUBLE:
        return np.asarray(values, np.float64).view(np.int64).copy()
    if arg_type == INT:
        return np.asarray(values, np.int32).astype(np.int64)
    return np.asarray(values, np.int64).copy()


def as_double(raw, arg_type):
    """the double the reference adds for a raw word: Float / Integer / Long unboxed"""
    raw = np.asarray(raw, np.int64)
    if arg_type == FLOAT:
        return (raw & 0xFFFFFFFF).astype(np.uint32).view(np.float32).astype(np.float64)
    if arg_type == DOUBLE:
        return raw.view(np.float64)
    if arg_type == INT:
        return raw.astype(np.int32).astype(np.float64)
    return raw.astype(np.float64)           # round to nearest even, as (double) of a long


def as_long(raw, arg_type):
    raw = np.asarray(raw, np.int64)
    return raw.astype(np.int32).astype(np.int64) if arg_type == INT else raw


# ------------------------------------------------------------------ cases
class Case:
    """rows in output order. vals [m, n_out] raw words with the aggregators' arguments in
    the columns of desc [(col, kind, arg_type)]; query [m] or None; key [m] the row's
    partition key, reached on the device as keys_table[seq - seq_base] (None: one key)"""

    def __init__(self, name, vals, desc, query, n_query, key, n_keys, seq, seq_base, keys_table, small_ints=False):
        self.name, self.vals, self.desc = name, vals, list(desc)
        self.query, self.n_query, self.key, self.n_keys = query, n_query, key, n_keys
        self.seq, self.seq_base, self.keys_table = seq, seq_base, keys_table
        self.small_ints = small_ints
        self.m, self.n_out = vals.shape

    def group(self):
        q = self.query.astype(np.int64) if self.query is not None else np.zeros(self.m, np.int64)
        return q * max(self.n_keys, 1) + self.key.astype(np.int64)

    def __repr__(self):
        return self.name


def build(name, segs, desc, n_out=None, n_keys=None, n_query=1, with_query=None, with_keys=True, seq_base=0,
          gaps=False, seed=0, small_ints=False):
    """segs: [(query, key, args)] with args [rows, len(desc)] raw words of the segment's
    rows in their order. The segments' rows are interleaved at random (each segment's own
    order kept: the pass sorts stably); the other columns hold arbitrary words."""
    rng = np.random.default_rng(seed + 12345)
    n_out = n_out or max(c for c, _, _ in desc) + 2
    lens = np.array([len(a) for _, _, a in segs])
    m = int(lens.sum())
    labels = np.repeat(np.arange(len(segs)), lens)
    rng.shuffle(labels)
    pos = np.argsort(labels, kind="stable")      # row positions: segment 0's rows in order, then segment 1's ...
    vals = rng.integers(-2 ** 62, 2 ** 62, (m, n_out)).astype(np.int64)
    args = np.concatenate([np.asarray(a, np.int64).reshape(len(a), len(desc)) for _, _, a in segs])
    for j, (c, _, _) in enumerate(desc):
        vals[pos, c] = args[:, j]
    query = np.zeros(m, np.int32)
    key = np.zeros(m, np.int32)
    query[pos] = np.repeat(np.array([q for q, _, _ in segs], np.int32), lens)
    key[pos] = np.repeat(np.array([k for _, k, _ in segs], np.int32), lens)
    n_keys = n_keys or int(key.max()) + 1
    assert int(key.max()) < n_keys and int(query.max()) < n_query
    with_query = (n_query > 1) if with_query is None else with_query
    if not with_query:
        assert not query.any()
    off = (np.cumsum(rng.integers(1, 4, m)) if gaps else np.arange(m)).astype(np.int64)
    seq = (np.uint64(seq_base) + off.astype(np.uint64)).astype(np.uint64)
    table = None
    if with_keys:
        table = rng.integers(0, n_keys, int(off[-1]) + 1).astype(np.int32)   # (the gaps: other events' keys)
        table[off] = key
    else:
        assert not key.any()
    return Case(name, vals, desc, query if with_query else None, n_query, key, n_keys, seq, seq_base, table,
                small_ints)


def single(name, seglists, arg_type=DOUBLE, kind=SUM, lead=0, unit=1.0, **kw):
    """one aggregate column (position 1 of 3); every list one segment (keys 1, 2, ... in
    that order, so in that sorted order), after `lead` rows of `unit` on key 0"""
    segs = []
    if lead:
        segs.append((0, 0, encode([unit] * lead, arg_type).reshape(-1, 1)))
    for i, s in enumerate(seglists):
        segs.append((0, i + 1, encode(s, arg_type).reshape(-1, 1)))
    return build(name, segs, [(1, kind, arg_type)], n_out=3, **kw)


def _typed_draw(rng, n, arg_type):
    """ordinary values whose sums stay exact: quarters, small ints, longs of any size
    for the wrapping sum (an avg over longs takes small ones)"""
    if arg_type in (FLOAT, DOUBLE):
        return rng.integers(-200, 200, n) * 0.25
    if arg_type == INT:
        return rng.integers(-1000, 1000, n)
    return rng.integers(-2 ** 40, 2 ** 40, n)


def mixed(name, m, n_keys, desc, n_query=1, n_out=None, seed=0, **kw):
    """m rows over random (query, key) segments, every column ordinary values"""
    rng = np.random.default_rng(seed + 999)
    q = rng.integers(0, n_query, m) if kw.get("with_query", n_query > 1) else np.zeros(m, np.int64)
    k = rng.integers(0, n_keys, m) if kw.get("with_keys", True) else np.zeros(m, np.int64)
    cols = [encode(_typed_draw(rng, m, t), t) for _, _, t in desc]
    args = np.stack(cols, axis=1)
    g = q * n_keys + k
    segs = [(int(gg // n_keys), int(gg % n_keys), args[g == gg]) for gg in np.unique(g)]
    return build(name, segs, desc, n_out=n_out, n_keys=n_keys, n_query=n_query, seed=seed, **kw)


ALL_KINDS = [(SUM, DOUBLE), (AVG, FLOAT), (SUM, LONG), (AVG, LONG), (SUM, FLOAT), (AVG, DOUBLE), (SUM, INT),
             (AVG, INT), (COUNT, INT)]


def _desc(n, stride=2, first=1):
    """n aggregate columns of mixed kinds at every `stride`-th row position"""
    return [(first + stride * i, *ALL_KINDS[i % len(ALL_KINDS)]) for i in range(n)]


P = lambda e: math.ldexp(1.0, e)        # noqa: E731  (2^e as a double)
FAR = TILE + 53                         # rows after which a segment's row lies in the next tile


def _cases():
    c = []
    neg = lambda s: [-x for x in s]     # noqa: E731
    # ---- the 53-bit gate
    g = {"g53_accept": [P(53) - 2, 1.0, 1.0],            # ... 2^53 - 1, 2^53
         "g53_refuse": [P(53), 1.0],                     # 2^53 + 1
         "g53_middle": [P(53), 1.0, 1.0]}                # 2^53 + 1 on the way to 2^53 + 2
    far = {"g53_accept": [P(53) - FAR] + [1.0] * FAR,
           "g53_refuse": [P(53) - FAR] + [1.0] * (FAR + 1),
           "g53_middle": [P(53) - FAR] + [1.0] * (FAR + 2)}
    for n, s in g.items():
        c.append(single(n, [s, [1.0, 2.0]]))
        c.append(single(n + "_neg", [neg(s), [1.0, 2.0]]))
        c.append(single(n + "_far", [far[n], [1.0]]))
        c.append(single(n + "_far_neg", [neg(far[n]), [1.0]], lead=7))
    # ---- the range gate
    c.append(single("range96", [[P(95)], [1.0]]))
    c.append(single("range97", [[P(96)], [1.0]]))
    c.append(single("range96_straddle", [[(P(53) - 1) * P(43)], [1.0], [-(P(53) - 1) * P(43), P(43)]]))
    c.append(single("shifts", [[1.0], [6.0], [3 * P(63)], [3 * P(64)], [3 * P(65)], [-3 * P(63), 3 * P(64)],
                               [-3.0, -6.0, 1.0]]))
    # ---- signs
    c.append(single("cancel_to_zero", [[1.5, -1.5, -0.0, P(-30)], [-0.0, 0.0, -0.0]]))
    c.append(single("only_negative_zero", [[-0.0] * 5]))
    c.append(single("negative_carry", [[-1.0] * (TILE + 900), [2.0] * 10], lead=300))
    c.append(single("alternating", [[x for i in range(1500) for x in (P(90) + P(40), -P(90))]], lead=11))
    # ---- small and large
    c.append(single("subnormal_sums", [[DENORM] * 5, [DBL_MIN - DENORM, DENORM], [-DENORM, -DENORM]], unit=DENORM,
                    lead=3))
    c.append(single("float_subnormals", [[F32_DENORM] * 3, [F32_DENORM_MAX, F32_DENORM], [-F32_DENORM] * 2],
                    arg_type=FLOAT, unit=F32_DENORM, lead=2))
    c.append(single("dbl_max", [[P(1023), DBL_MAX - P(1023)], [-P(1023), -(DBL_MAX - P(1023))]]))
    c.append(single("overflow_and_back", [[P(1023), P(1023), -P(1023)]]))
    c.append(single("overflow_and_back_neg", [[P(1000)], [-P(1023), -P(1023), P(1023)]]))
    c.append(single("overflow_and_back_far", [[P(1023), P(1023)] + [0.0] * FAR + [-P(1023)]], unit=0.0, lead=5))
    c.append(single("overflow_at_the_end", [[P(1023), P(1023)]]))
    # ---- types
    c.append(mixed("every_kind", 700, 5, _desc(9), seed=1))
    c.append(single("avg_long_rounded_addends", [[2 ** 53 + 1, 2 ** 53 + 3], [-(2 ** 53 + 1), 5]], arg_type=LONG,
                    kind=AVG))
    c.append(single("avg_long_rounding_sum", [[2 ** 60 + 1, 3]], arg_type=LONG, kind=AVG))
    c.append(single("sum_long_wraps", [[LONG_MAX] * (TILE + 5), [LONG_MIN, -1, LONG_MIN]], arg_type=LONG, unit=1,
                    lead=TILE - 3))
    c.append(single("sum_int_min", [[INT_MIN] * (TILE + 5)], arg_type=INT, unit=1, lead=TILE - 3))
    c.append(single("count_only", [[0] * 3, [0] * (TILE + 1), [0]], arg_type=INT, kind=COUNT, unit=0, lead=1))
    # ---- layout: heads at tile offsets 0, 1, 2047 and 2048; a segment over three tiles
    c.append(single("heads_at_seams", [[1.0], [0.5] * (TILE - 2), [4.0], [0.25] * 9]))
    c.append(single("three_tiles", [[1.0] * (2 * TILE + 500), [3.0]], lead=100))
    for m in (1, TILE - 1, TILE, TILE + 1, 3 * TILE + 1):
        c.append(mixed(f"rows_{m}", m, 3, _desc(2), seed=m))
    for nk in (1, 3, 255, 256, 257):
        c.append(mixed(f"keys_{nk}", 3000, nk, _desc(2), seed=nk, with_keys=nk > 1))
    c.append(mixed("queries_5", 3000, 7, _desc(2), n_query=5, seed=5))
    c.append(mixed("queries_5_no_keys", 2500, 1, _desc(2), n_query=5, seed=6, with_keys=False))
    c.append(mixed("query_array_absent", 2500, 7, _desc(2), n_query=5, seed=7, with_query=False))
    c.append(mixed("query_array_of_one", 900, 3, _desc(2), n_query=1, seed=8, with_query=True))
    c.append(mixed("seq_base_and_gaps", 2600, 9, _desc(2), n_query=2, seed=9, seq_base=(1 << 33) + 17, gaps=True))
    c.append(mixed("one_column", 2100, 4, [(0, SUM, DOUBLE)], n_out=1, seed=10))
    c.append(mixed("sixteen_columns", 2 * TILE + 77, 6, _desc(MAX_COLS), n_query=2, seed=11))
    # a max and a min column beside a sum that must refuse: nothing may move
    rng = np.random.default_rng(77)
    segs = []
    for k in range(4):
        n = 40
        x = rng.integers(-50, 50, n) * 0.5
        s = x.copy()
        if k == 2:
            s[7], s[8] = P(53), 1.0
        segs.append((0, k, np.stack([encode(x, DOUBLE), encode(s, DOUBLE), encode(x, FLOAT)], axis=1)))
    c.append(build("extremes_beside_refusal", segs, [(0, MAX, DOUBLE), (2, SUM, DOUBLE), (3, MIN, FLOAT)], n_out=5))
    c.append(build("extremes_beside_exact", [(q, k, a[:7]) for q, k, a in segs],
                   [(0, MAX, DOUBLE), (2, SUM, DOUBLE), (3, MIN, FLOAT)], n_out=5))
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

BIG_M = CARRY_THREADS * TILE + TILE + 1      # 1,026 tiles: two per thread of the carry workgroup


@functools.lru_cache(maxsize=None)
def big_case():
    """small integer addends over 3 keys, 2 columns; its reference is an int64 cumsum"""
    rng = np.random.default_rng(4242)
    key = rng.integers(0, 3, BIG_M)
    x = rng.integers(-3, 9, BIG_M)
    args = np.stack([encode(x.astype(np.float64), DOUBLE), encode(x, INT)], axis=1)
    segs = [(0, k, args[key == k]) for k in range(3)]
    return build("two_tiles_per_carry_thread", segs, [(0, SUM, DOUBLE), (2, AVG, INT)], n_out=3, small_ints=True)


def salted_case(arg_type):
    """shc_running alone: NaN, the infinities, DBL_MAX / FLT_MAX among ordinary values"""
    import edge_values as ev
    rng = np.random.default_rng(31 + arg_type)
    m, nk = 3000, 6
    pool = ev.F64_POOL if arg_type == DOUBLE else ev.F32_POOL
    x = (rng.integers(-200, 200, m) * 0.25).astype(pool.dtype)
    x = ev.salt(x, pool, share=0.1, rng=rng)
    key = rng.integers(0, nk, m)
    args = np.stack([encode(x, arg_type)] * 3, axis=1)
    segs = [(0, k, args[key == k]) for k in range(nk)]
    return build(f"salted_{arg_type}", segs, [(0, SUM, arg_type), (1, AVG, arg_type), (3, MAX, arg_type)], n_out=4,
                 seed=arg_type)


SPLIT_DESC = [(0, SUM, DOUBLE), (1, AVG, FLOAT), (3, COUNT, INT), (4, SUM, LONG), (5, MAX, DOUBLE), (6, AVG, LONG)]


@functools.lru_cache(maxsize=None)
def split_case():
    """(the whole case, the row where its second call starts): tenths, whose additions
    round, so the order and the carried state both show. Keys 0 - 3 only have rows before
    the cut, keys 4 - 7 only after it, keys 8 - 15 on both sides, under 3 queries"""
    rng = np.random.default_rng(2024)
    halves = []
    for lo, hi, m in ((0, 4, 1900), (4, 8, 2300)):
        key = np.where(rng.random(m) < 0.4, rng.integers(lo, hi, m), rng.integers(8, 16, m))
        q = rng.integers(0, 3, m)
        x = rng.integers(-999, 999, m) * 0.1
        args = np.stack([encode(x, DOUBLE), encode(x, FLOAT), encode(np.zeros(m), INT),
                         encode(rng.integers(-2 ** 62, 2 ** 62, m), LONG), encode(x * 3.0, DOUBLE),
                         encode(rng.integers(-2 ** 55, 2 ** 55, m), LONG)], axis=1)
        g = q * 16 + key
        segs = [(int(gg // 16), int(gg % 16), args[g == gg]) for gg in np.unique(g)]
        halves.append(build(f"half_{lo}", segs, SPLIT_DESC, n_out=8, n_keys=16, n_query=3, seed=lo))
    a, b = halves
    key = np.concatenate([a.key, b.key])
    whole = Case("split", np.concatenate([a.vals, b.vals]), SPLIT_DESC, np.concatenate([a.query, b.query]), 3, key, 16,
                 np.arange(a.m + b.m, dtype=np.uint64) + np.uint64(5), 5, key.copy())
    return whole, a.m


# ------------------------------------------------------------------ end to end: planted streams
# The bucketed carry's own gate (k_bk_aggp: every running value below 2^53 units of
# 2^-24). C2_AGG itself never reaches it with a double price: its avg(e1.price) would need
# an 8-byte e1 column and its two e2 sums two 8-byte staged columns, which the carry plan
# (sh_bucket_plan.h shb_plan_carry) leaves to the post-pass. This is C2_AGG with the
# select cut to what the plan carries over a double: the sum under test and count().
BK_GATE_APP = ("define stream StockStream (symbol string, price double, volume long); "
               "partition with (symbol of StockStream) begin @info(name = 'query1') "
               "from every e1=StockStream[price>20] -> e2=StockStream[symbol==e1.symbol and price>e1.price] "
               "within 1 sec select e1.symbol as symbol, sum(e2.price) as total, count() as n insert into Out; end;")
BK_SHAPE = (8192 + 5, 1024)      # the bucketed engine's gate: 1,024 keys and one 8,192-event tile
U = 2.0 ** -24                   # k_bk_aggp's unit
# the planted key's events: (21.0, P) pairs, P falling, so that each P consumes exactly
# the 21.0 before it and no P is consumed; the key's other events cannot open or consume
BK_PLANTS = {"below": [21.0, 2.0 ** 28, 21.0, 2.0 ** 28 - U],                          # 2^53 - 1 units
             "above": [21.0, 2.0 ** 28 + U, 21.0, 2.0 ** 28, 21.0, 21.0 + U]}         # 2^53 + 1 units, and on
BK_TOTALS = {"below": [2.0 ** 28, 2.0 ** 29 - U],
             # 2^29 + 2^-24 and 2^29 + 21 + 2^-23 need 54 bits: the reference rounds both (to even)
             "above": [2.0 ** 28 + U, 2.0 ** 29, 2.0 ** 29 + 21.0]}
BK_EXACT_UNITS = {"below": [2 ** 52, 2 ** 53 - 1], "above": [2 ** 52 + 1, 2 ** 53 + 1, 2 ** 53 + 21 * 2 ** 24 + 2]}


def _planted_key(k, need):
    """the first key with at least `need` events"""
    counts = np.bincount(k)
    return int(np.flatnonzero(counts >= need)[0])


@functools.lru_cache(maxsize=None)
def bk_gate_stream(which):
    """(ts, keys, price, volume, planted key) of one boundary stream"""
    from siddhi_amd import synth
    ts, k, p, v = synth.stock_stream(*BK_SHAPE, 100)
    p = p.astype(np.float64)
    kk = _planted_key(k, 6)
    at = np.flatnonzero(k == kk)
    p[at] = 1.0
    plant = BK_PLANTS[which]
    p[at[:len(plant)]] = plant
    return ts, k, p, v, kk


# The overflow through the whole engine ladder: the C2_AGG_OPEN form of
# tests/edge_values.py over a double price (every event opens, `>=` consumes), every
# price scaled by 2^1000 so that the column's range stays narrow, and one key planted
# with 2^1023, 2^1023, 2^1023, -2^1023, -2^1023: its total is 2^1023, then infinity, and
# the next row adds -2^1023 to an exact sum of 2^1024
OVF_PLANT = [2.0 ** 1023, 2.0 ** 1023, 2.0 ** 1023, -2.0 ** 1023, -2.0 ** 1023]


def overflow_app():
    import edge_values as ev
    return ev.C2_AGG_OPEN.replace("price float", "price double")


@functools.lru_cache(maxsize=None)
def overflow_stream():
    from siddhi_amd import synth
    ts, k, p, v = synth.stock_stream(*BK_SHAPE, 100)
    p = p.astype(np.float64) * 2.0 ** 1000
    kk = _planted_key(k, len(OVF_PLANT))
    at = np.flatnonzero(k == kk)
    p[at[:len(OVF_PLANT)]] = OVF_PLANT
    return ts, k, p, v, kk


def oracle_rows(app, ts, k, cols):
    from oracle_engine import OracleEngine
    from siddhi_amd import compiler
    eng = OracleEngine(compiler.compile_app(app))
    eng.start()
    for b0 in range(0, len(ts), 4096):
        b1 = min(len(ts), b0 + 4096)
        eng.send(0, np.ascontiguousarray(ts[b0:b1]), [np.ascontiguousarray(c[b0:b1]) for c in cols],
                 [None] * len(cols), np.ascontiguousarray(k[b0:b1]), b0)
    out = eng.drain()
    eng.close()
    return out


_oracle_cache = {}


def bk_gate_ref(which):
    if which not in _oracle_cache:
        ts, k, p, v, kk = bk_gate_stream(which)
        _oracle_cache[which] = oracle_rows(BK_GATE_APP, ts, k, [k, p, v])
    return _oracle_cache[which]


def overflow_ref():
    if "ovf" not in _oracle_cache:
        ts, k, p, v, kk = overflow_stream()
        _oracle_cache["ovf"] = oracle_rows(overflow_app(), ts, k, [k, p, v])
    return _oracle_cache["ovf"]


# ------------------------------------------------------------------ the reference
def _segments(case):
    """row indices of every (query, key) segment, in row order"""
    g = case.group()
    order = np.argsort(g, kind="stable")
    gs = g[order]
    cuts = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1], True])
    return [order[cuts[i]:cuts[i + 1]] for i in range(len(cuts) - 1)]


def _extreme(raw, kind, arg_type):
    """max / min: an empty state takes the argument, then the argument replaces the
    state iff state < arg (max) / state > arg (min); the row carries the state's bits"""
    x = as_double(raw, arg_type) if arg_type in (FLOAT, DOUBLE) else as_long(raw, arg_type)
    out, state = np.empty(len(raw), np.int64), 0
    for i in range(len(raw)):
        if i and ((x[state] < x[i]) if kind == MAX else (x[state] > x[i])):
            state = i
        out[i] = raw[state]
    return out


def reference(case):
    """the rows after the reference's sequential aggregation (raw words)"""
    out = case.vals.copy()
    with np.errstate(all="ignore"):
        for ix in _segments(case):
            n = np.arange(1, len(ix) + 1, dtype=np.int64)
            for col, kind, t in case.desc:
                raw = case.vals[ix, col]
                if kind == COUNT:
                    out[ix, col] = n
                elif kind in (MAX, MIN):
                    out[ix, col] = _extreme(raw, kind, t)
                elif is_fp(kind, t):
                    s = np.add.accumulate(np.concatenate(([0.0], as_double(raw, t))))[1:]
                    out[ix, col] = (s / n.astype(np.float64) if kind == AVG else s).view(np.int64)
                else:
                    out[ix, col] = np.cumsum(as_long(raw, t), dtype=np.int64)      # wraps
    return out


def fp_columns(case):
    return [(col, kind, t) for col, kind, t in case.desc if is_fp(kind, t)]


def agg_columns(case):
    return [col for col, _, _ in case.desc]


def canon(case, vals):
    """the comparison form: exact bits, all NaNs of a double-valued column as one"""
    v = np.array(vals, np.int64, copy=True)
    for col, kind, t in fp_columns(case):
        v[np.isnan(v[:, col].view(np.float64)), col] = QNAN64
    for col, kind, t in case.desc:
        if kind in (MAX, MIN) and t == DOUBLE:
            v[np.isnan(v[:, col].view(np.float64)), col] = QNAN64
        if kind in (MAX, MIN) and t == FLOAT:
            f = (v[:, col] & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
            v[np.isnan(f), col] = 0x7FC00000
    return v


# ------------------------------------------------------------------ exact values and the verdict class
def units(x):
    """a finite double as an integer number of 2^-1074"""
    n, d = float(x).as_integer_ratio()
    return n * ((1 << SCALE) // d)


def sig_bits(e):
    a = abs(e)
    return (a >> ((a & -a).bit_length() - 1)).bit_length() if a else 0


def exact_to_double(e):
    """the double equal to e * 2^-1074; +-inf when e is at or beyond 2^1024 in
    magnitude; None when e is not representable (more than 53 significant bits)"""
    if e == 0:
        return 0.0
    a = abs(e)
    if a.bit_length() > 1024 + SCALE:
        return -math.inf if e < 0 else math.inf
    if sig_bits(e) > 53:
        return None
    tz = (a & -a).bit_length() - 1
    d = math.ldexp(float(a >> tz), tz - SCALE)
    return -d if e < 0 else d


def exact_running(case, col, arg_type):
    """[(row indices, exact running sums as integers)] of one fp column with finite addends"""
    out = []
    for ix in _segments(case):
        acc, run = 0, []
        for x in as_double(case.vals[ix, col], arg_type).tolist():
            acc += units(x)
            run.append(acc)
        out.append((ix, run))
    return out


def addend_range(x):
    """(lowest set bit, highest bit) over the non-zero addends as powers of two, or None"""
    lo, hi = None, None
    for v in np.unique(x[x != 0]).tolist():
        u = abs(units(v))
        l, h = (u & -u).bit_length() - 1 - SCALE, u.bit_length() - 1 - SCALE
        lo, hi = (l if lo is None else min(lo, l)), (h if hi is None else max(hi, h))
    return None if lo is None else (lo, hi)


@functools.lru_cache(maxsize=None)
def _stats(name, big):
    case = big_case() if big else BY_NAME[name]
    ref = reference(case)
    st = dict(nonfinite=False, mismatch=None, range=0, sig=0, out_of_range=False, shifts=set(), subnormal_out=False)
    for col, kind, t in fp_columns(case):
        x = as_double(case.vals[:, col], t)
        if not np.isfinite(x).all():
            st["nonfinite"] = True
            continue
        rg = addend_range(x)
        if rg:
            st["range"] = max(st["range"], rg[1] - rg[0] + 1)
        if case.small_ints:
            # integers far below 2^53: the exact sums are an int64 cumsum
            for ix in _segments(case):
                e = np.cumsum(x[ix].astype(np.int64))
                assert np.abs(e).max() < 2 ** 53
                st["sig"] = max(st["sig"], int(np.abs(e).max()).bit_length())
                s = np.add.accumulate(np.concatenate(([0.0], x[ix])))[1:]
                if not np.array_equal(s, e.astype(np.float64)):
                    st["mismatch"] = (col, int(ix[0]))
            continue
        for v in np.unique(x[x != 0]).tolist():
            u = abs(units(v))
            st["shifts"].add((u & -u).bit_length() - 1 - SCALE - rg[0])
        with np.errstate(all="ignore"):
            for ix, run in exact_running(case, col, t):
                seq = np.add.accumulate(np.concatenate(([0.0], x[ix])))[1:]
                for r, e, s in zip(ix.tolist(), run, seq.tolist()):
                    st["sig"] = max(st["sig"], sig_bits(e))
                    d = exact_to_double(e)
                    if d is None or d != s or (d == 0.0 and math.copysign(1.0, s) < 0):
                        st["mismatch"] = st["mismatch"] or (col, r)
                    elif math.isinf(d):
                        st["out_of_range"] = True
                    elif d != 0.0 and abs(d) < DBL_MIN:
                        st["subnormal_out"] = True
    if st["nonfinite"] or st["mismatch"]:
        st["cls"] = "refuse"
    elif st["range"] > 96 or st["out_of_range"]:
        st["cls"] = "either"
    else:
        assert st["sig"] <= 53
        st["cls"] = "accept"
    st["ref"] = ref
    return st


def stats(case):
    return _stats(case.name, case.small_ints)


def classify(case):
    return stats(case)["cls"]


def layout(case):
    """(tiles, sorted positions of the segment heads) of the pass's sorted order"""
    lens = np.array([len(ix) for ix in _segments(case)])
    heads = np.concatenate(([0], np.cumsum(lens)[:-1]))
    return (case.m + TILE - 1) // TILE, heads
