"""IEEE-754 and Java edge values for the filter, arithmetic and aggregate paths:
value pools, a column salter, the query lists the CPU and GPU edge tests share, and
the one comparison rule (`canon`).

The device has many hand-written forms of "compare two attribute values the way
Java does" (the window kernels and their hipRTC-specialised source, the bucketed
matcher's float walks, k_s3b / k_seq3s, the rule engine's term loops, the VM of the
general engine, the aggregate carries). The oracle evaluates all of it with one plain
C++ switch (oracle/refcpu.cpp `cmp`, `arith`), which tests/test_edge_values_cpu.py
pins to Java with a hand-written truth table; the GPU tests then compare every
device form with the oracle on streams salted from the pools below.

No GPU is needed to import this module."""
import numpy as np

from siddhi_amd import compiler, synth

FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)          # smallest normal, 2^-126
F32_DENORM_MIN = 2.0 ** -149
F32_DENORM_MAX = FLT_MIN - F32_DENORM_MIN           # largest subnormal
DBL_MAX = float(np.finfo(np.float64).max)
DBL_MIN = float(np.finfo(np.float64).tiny)
F64_DENORM_MIN = 5e-324
F64_DENORM_MAX = DBL_MIN - F64_DENORM_MIN
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
LONG_MIN, LONG_MAX = -2 ** 63, 2 ** 63 - 1

_f32 = np.float32
F32_ABOVE_20 = float(np.nextafter(_f32(20), _f32(np.inf)))      # 20 + 2^-19
F32_BELOW_20 = float(np.nextafter(_f32(20), _f32(-np.inf)))     # 20 - 2^-19
F32_POOL = np.array(
    [np.nan, np.inf, -np.inf, 0.0, -0.0, F32_DENORM_MIN, -F32_DENORM_MIN, F32_DENORM_MAX, FLT_MIN,
     FLT_MAX, -FLT_MAX, 20.0, F32_ABOVE_20, F32_BELOW_20, 16777216.0, 16777218.0], dtype=np.float32)
F64_POOL = np.array(
    [np.nan, np.inf, -np.inf, 0.0, -0.0, F64_DENORM_MIN, -F64_DENORM_MIN, F64_DENORM_MAX, DBL_MIN,
     DBL_MAX, -DBL_MAX, 20.0, np.nextafter(20.0, np.inf), np.nextafter(20.0, -np.inf),
     2.0 ** 53, 2.0 ** 53 + 2, 12.34, 2.0 ** -25, 1e300], dtype=np.float64)
I32_POOL = np.array([INT_MIN, INT_MIN + 1, -1, 0, 1, INT_MAX, INT_MAX - 4, 16777217, -2, -5], dtype=np.int32)
I64_POOL = np.array([LONG_MIN, LONG_MAX, 2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 62, -1, 0, 2 ** 24 + 1], dtype=np.int64)
POOLS = {np.dtype(np.float32): F32_POOL, np.dtype(np.float64): F64_POOL,
         np.dtype(np.int32): I32_POOL, np.dtype(np.int64): I64_POOL}


def salt(col, pool=None, share=0.25, rng=None):
    """A copy of `col` with `share` of its positions (chosen by `rng`) replaced by
    uniform draws from `pool` (default: the pool of the column's type). The rest
    stays ordinary, so partials still open and get consumed."""
    rng = np.random.default_rng(0) if rng is None else rng
    pool = POOLS[col.dtype] if pool is None else np.asarray(pool, dtype=col.dtype)
    out = col.copy()
    hit = rng.random(len(col)) < share
    out[hit] = pool[rng.integers(0, len(pool), int(hit.sum()))]
    return out


# ---------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------
FLOAT, DOUBLE = compiler.FLOAT, compiler.DOUBLE
QNAN32 = 0x7FC00000
QNAN64 = 0x7FF8000000000000


def canon(vals, types):
    """Raw 8-byte row values (int64 [n, n_out]: float bits zero-extended, double bits,
    integers sign-extended) -> the form two engines are compared in. Bit patterns are
    compared exactly, with ONE exception: every NaN of a float / double column is
    mapped to the canonical quiet NaN of its width (0x7FC00000 / 0x7FF8000000000000), on
    both sides. Java cannot tell NaNs apart (Float.floatToIntBits, doubleToLongBits
    and toString collapse them), and the host FPU and the GPU give different default-NaN
    sign bits for `inf + -inf`. This is the only tolerance of the edge tests; +0.0 and
    -0.0 stay distinct, and so does every other bit."""
    v = np.array(vals, dtype=np.int64, copy=True)
    if v.ndim == 1:
        v = v.reshape(-1, 1)
    for o, t in enumerate(types):
        if o >= v.shape[1]:
            break
        c = v[:, o]
        if t == FLOAT:
            f = (c & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
            c[np.isnan(f)] = QNAN32
        elif t == DOUBLE:
            c[np.isnan(c.view(np.float64))] = QNAN64
    return v


def canon_obj(x):
    """A select value of the event API (None, bool, int, float, str) in comparable
    form: floats by their double bit pattern (a float attribute arrives widened, which
    is exact and keeps the sign of zero), NaN as one value."""
    if isinstance(x, float):
        return ("f", QNAN64 if x != x else int(np.float64(x).view(np.int64)))
    return x


def assert_rows_equal(got, ref, types, what=""):
    """`got` / `ref`: dicts with seq, values, optional nulls / query (the oracle's
    drain() form). Equal seq, equal query where both carry it, canon(values) equal
    where the reference is not null."""
    assert len(got["seq"]) == len(ref["seq"]), (what, len(got["seq"]), len(ref["seq"]))
    assert np.array_equal(np.asarray(got["seq"]).astype(np.int64), np.asarray(ref["seq"]).astype(np.int64)), what
    if got.get("query") is not None and ref.get("query") is not None:
        assert np.array_equal(got["query"], ref["query"]), what
    w = len(types)
    g, r = canon(got["values"][:, :w], types), canon(ref["values"][:, :w], types)
    if ref.get("nulls") is not None:
        nn = ~np.asarray(ref["nulls"])[:, :w].astype(bool)
        if got.get("nulls") is not None:
            assert np.array_equal(np.asarray(got["nulls"])[:, :w].astype(bool), ~nn), what
    else:
        nn = np.ones(r.shape, bool)
    bad = np.nonzero((g != r) & nn)
    assert len(bad[0]) == 0, (what, "first differing row", int(bad[0][0]), g[bad[0][0]].tolist(),
                              r[bad[0][0]].tolist())


# ---------------------------------------------------------------------------------
# (a) window-shaped queries
# ---------------------------------------------------------------------------------
S_DEF = "define stream S (sym string, price float, volume long, x int, d double); "
S_SELECT = "e1.sym as a, e1.price as b, e2.price as c, e2.volume as v, e1.x as x1, e2.d as d2"

F1 = {"thr": "price > 20", "neg": "price > -1.0f", "not": "not (price > 20)", "nan": "price != price"}

# (name, f1 key, f2): one promotion domain or arithmetic rule each
WINDOW_QUERIES = [
    # float against float, all four orderings and both operand orders
    ("f32_gt", "thr", "price > e1.price"),
    ("f32_gt_free", "neg", "price > e1.price"),
    ("f32_le", "neg", "price <= e1.price"),
    ("f32_le_not", "not", "price <= e1.price"),
    ("f32_lt_rev", "thr", "e1.price < price"),
    ("f32_ge_rev", "neg", "e1.price >= price"),
    ("f32_ge_rev_not", "not", "e1.price >= price"),
    ("f32_ge", "neg", "price >= e1.price"),
    ("f32_lt", "thr", "price < e1.price"),
    # NaN partials: no ordering comparison ever consumes them (`price != price` with
    # `price <= e1.price` gives no row on any stream, so that pair is not listed); != does
    ("f32_nan_ne", "nan", "price != e1.price"),
    # double
    ("f64_gt", "neg", "d > e1.d"),
    ("f32_x_f64lit", "thr", "price > e1.price * 1.05"),
    ("f64_lt_f32", "not", "d < e1.price"),
    # float arithmetic that overflows
    ("f32_mul_ovf", "neg", "price * 2.0f > e1.price"),
    ("f32_add", "thr", "price + 1.0f > e1.price"),
    # integer against float
    ("i64_gt_f32", "neg", "volume > e1.price"),
    ("i32_ge_f32", "not", "x >= e1.price"),
    ("i32_eq_f32", "neg", "x == e1.price"),
    ("i64_eq_f32", "neg", "volume == e1.price"),    # ==/!= of (Long, Float) compare as double
    ("i64_ne_f32", "thr", "volume != e1.price"),
    # integers
    ("i32_add_wrap", "thr", "x < e1.x + 5"),
    ("i32_div2", "neg", "(x / 2) > e1.x"),
    ("i32_mod3", "not", "x % 3 == 1"),
    ("i32_mod_m1", "thr", "x % -1 == 0"),
    ("i32_div_m1", "neg", "x / -1 > e1.x"),
    ("i64_ge", "thr", "volume >= e1.volume"),
    ("i64_mul_wrap", "neg", "volume * 2 > e1.volume"),
    # null -> false: no row at all, see NULL_QUERIES
    ("i32_div0", "neg", "x / 0 > 1 or price > e1.price"),
    ("f32_mod0", "thr", "price % 0.0f > 1.0f or volume >= e1.volume"),
]
# the issue's bare null forms: `x / 0 > 1` and `price % 0.0f > 1.0f` are null -> false for
# every event, so on their own they give no row; here they stand beside a term that can
# be true, so a kernel that evaluated the null comparison as true would add rows
WINDOW_BY_NAME = {q[0]: q for q in WINDOW_QUERIES}


def window_app(f1, f2, within_ms, partitioned=True, stream_def=S_DEF, select=S_SELECT):
    q = (f"@info(name = 'query1') from every e1=S[{f1}] -> e2=S[{f2}] within {within_ms} milliseconds "
         f"select {select} insert into Out;")
    return stream_def + (f"partition with (sym of S) begin {q} end;" if partitioned else q)


def window_query(name, within_ms=40, partitioned=True):
    _, k1, f2 = WINDOW_BY_NAME[name]
    return window_app(F1[k1], f2, within_ms, partitioned)


def ordinary_columns(n, rng):
    """price, volume, x, d the way the stock generators draw them (tests/test_gpu_parity.py)"""
    price = (rng.integers(0, 40, n) + rng.choice([0.0, 0.5, 0.25], n)).astype(np.float32)
    vol = rng.integers(0, 30, n).astype(np.int64)
    x = rng.integers(-3, 25, n).astype(np.int32)
    d = (rng.integers(0, 40, n) + rng.choice([0.0, 0.5, 0.125], n)).astype(np.float64)
    return price, vol, x, d


def salt_columns(cols, rng, share=0.25):
    return tuple(salt(c, share=share, rng=rng) for c in cols)


def window_stream(n, nk, seed=0, edge=True):
    """ts, keys, (price, volume, x, d) of stream S; `edge=False`: the same stream with
    the salted positions left ordinary"""
    rng = np.random.default_rng(100 + seed)
    keys = rng.integers(0, nk, n).astype(np.int32)
    ts = (1000 + np.cumsum(rng.choice([0, 0, 1, 2, 3], n))).astype(np.int64)
    cols = ordinary_columns(n, rng)
    if edge:
        cols = salt_columns(cols, np.random.default_rng(200 + seed))
    return ts, keys, cols


def bucket_stream(n, nk, seed=0, edge=True):
    """the stock generator's arrival pattern (100 events / ms, uniform keys) with the
    columns of stream S"""
    ts, keys, p, v = synth.stock_stream(n, nk, 100)
    rng = np.random.default_rng(300 + seed)
    _, _, x, d = ordinary_columns(n, rng)
    cols = (p, v, x, d)
    if edge:
        cols = salt_columns(cols, np.random.default_rng(400 + seed))
    return ts, keys, cols


# every partitioned (a) query the bucketed engine accepts. The CPU test asserts through
# shx_bucket_compile that these are accepted and every other (a) query refused. The float
# and double cross terms take the float walks (walk_count_f / walk_count_f_dyn; a long or
# int against a float compares in the float domain too), the integer ones the generic
# walk_count
BUCKET_FLOAT = ["f32_gt", "f32_gt_free", "f32_le", "f32_lt_rev", "f32_ge_rev", "f32_ge", "f32_lt", "f64_gt",
                "f32_x_f64lit", "f32_mul_ovf", "f32_add", "i64_gt_f32"]
BUCKET_INT = ["i32_add_wrap", "i64_ge", "i64_mul_wrap"]
BUCKET_QUERIES = BUCKET_FLOAT + BUCKET_INT

# ---------------------------------------------------------------------------------
# (b) C3-shaped
# ---------------------------------------------------------------------------------
C3_MIRROR = ("define stream S (symbol string, price float, volume long); "
             "partition with (symbol of S) begin @info(name = 'query1') "
             "from every e1=S, e2=S[price<e1.price]+, e3=S[price>e2[last].price] "
             "select e1.price as p1, e2[last].price as trough, e3.price as p3 insert into Out; end;")
C3_MIXED = ("define stream S (symbol string, price float, volume long); partition with (symbol of S) begin "
            "@info(name = 'query1') "
            "from every e1=S, e2=S[volume >= e1.volume]+, e3=S[e2[last].price > price] "
            "select e3.volume as v3, e1.symbol as s, e2[last].volume as lv, e1.price as p1 insert into Out; end;")
# the rise-and-fall shape over an int attribute: at 1,024 keys or more k_s3b's generic
# nf_cmp branch (the float form takes its float-as-float fast path)
C3_INT = ("define stream S (symbol string, price int, volume long); "
          "partition with (symbol of S) begin @info(name = 'query1') "
          "from every e1=S, e2=S[price>e1.price]+, e3=S[price<e2[last].price] "
          "select e1.price as p1, e2[last].price as peak, e3.price as p3 insert into Out; end;")
C3_QUERIES = {"c3": synth.C3_QUERY, "c3_mirror": C3_MIRROR, "c3_mixed": C3_MIXED, "c3_int": C3_INT}


def c3_stream(n, nk, name, edge=True):
    """the C3 generator's stream; the price column salted (for the int form the prices
    truncated to int, then salted from the int pool), for the mixed form the long column too"""
    ts, k, p, v = synth.stock_stream(n, nk, 1000, config_index=3)
    if name == "c3_mixed":
        v = np.random.default_rng(9).integers(0, 4, n).astype(np.int64)
    if name == "c3_int":
        p = p.astype(np.int32)
    if edge:
        rng = np.random.default_rng(500)
        p = salt(p, rng=rng)
        if name == "c3_mixed":
            v = salt(v, rng=rng)
    return ts, k, p, v


# ---------------------------------------------------------------------------------
# (c) C5-shaped rule sets (12 rules: they also fit the general engine's 16)
# ---------------------------------------------------------------------------------
def _rules_text(rules, mtype, mlit):
    qs = []
    for r, (a, m, f, w) in enumerate(rules):
        f1 = f"amount > {a!r} and merchant == {mlit(m)}"
        qs.append(f"@info(name = 'rule{r}') from every e1=Txn[{f1}] -> "
                  f"e2=Txn[card == e1.card and amount > e1.amount * {f!r}] within {w} milliseconds "
                  f"select e1.card as card, e2.amount as amount insert into Alerts;")
    return (f"define stream Txn (card string, amount float, merchant {mtype}); "
            "partition with (card of Txn) begin " + " ".join(qs) + " end;")


def rule_set(variant, n=24_000, cards=400, edge=True):
    """(app text, rules, (ts, card, amount, merchant)) of one 12-rule set.

    base     synth.c5_query over 4 merchants; rule 0 has the threshold -1.0 and the
             factor 1e30 (`e1.amount * 1e30` is a double product: FLT_MAX * 1e30 is
             finite, and a kernel that multiplied in float would see +inf), rule 1 the
             factor 0.0 (-x * 0.0 is -0.0; NaN * 0.0 is NaN)
    int      the indexed conjunct `merchant == M` with M and the merchant column from
             the int pool
    long     the conjunct on a long attribute (`merchant == ML`), values from the long pool
    float    the conjunct on a float attribute. `ix_term_ok` (sh_rules / the host's
             ix_const_key) must refuse to index it: 0.0f == -0.0f is true for two bit
             patterns and NaN == NaN is false for one, so equal keys are not equal
             values; the rows must still be the oracle's."""
    nr, seed = 12, 35
    ts, card, amount, merchant = synth.txn_stream(n, cards, 4, n_merchants=4, seed=seed)
    base = synth.c5_rules(nr, seed=seed, amount=(60.0, 400.0), merchants=4, factor=(0.5, 1.6), within=(5, 60))
    rules = [list(r) for r in base]
    rules[0][0], rules[0][2] = -1.0, 1e30
    rules[1][2] = 0.0
    rng = np.random.default_rng(600)
    if variant == "base":
        pass
    elif variant == "int":
        for r in rules:
            r[1] = int(I32_POOL[rng.integers(0, len(I32_POOL))])
    elif variant == "long":
        merchant = merchant.astype(np.int64)
        for r in rules:
            r[1] = int(I64_POOL[rng.integers(0, len(I64_POOL))])
    elif variant == "float":
        fpool = np.array([0.0, -0.0, 1.0, 2.0, 3.0, 16777216.0], np.float32)
        merchant = merchant.astype(np.float32)
        for r in rules:
            r[1] = float(fpool[rng.integers(0, len(fpool))])
    else:
        raise KeyError(variant)
    rules = [tuple(r) for r in rules]
    if variant == "base":
        text = synth.c5_query(rules, unit="milliseconds")
    elif variant == "int":
        text = _rules_text(rules, "int", lambda m: str(m))
    elif variant == "long":
        text = _rules_text(rules, "long", lambda m: f"{m}L")
    else:
        text = _rules_text(rules, "float", lambda m: ("-" if np.signbit(m) else "") + f"{abs(m)!r}f")
    if edge:
        srng = np.random.default_rng(700)
        amount = salt(amount, rng=srng)
        if variant != "base":
            merchant = salt(merchant, share=0.5, rng=srng)
    return text, rules, (ts, card, amount, merchant)


RULE_VARIANTS = ["base", "int", "long", "float"]

# ---------------------------------------------------------------------------------
# (d) general engine: chains, a count state, a logical `and`, computing selects
# ---------------------------------------------------------------------------------
G_SELECT = ("e1.x / e2.x as q, e1.x % e2.x as r, e1.price / e2.price as fq, e1.volume * e2.volume as vm, "
            "e1.price as p1, e2.d as d2")
GENERAL_APPS = {
    "chain3": S_DEF + "partition with (sym of S) begin @info(name = 'query1') "
              "from every e1=S[price > -1.0f] -> e2=S[price <= e1.price] -> e3=S[volume >= e2.volume and "
              "x % 3 == 1] within 30 milliseconds "
              f"select {G_SELECT}, e3.x as x3 insert into Out; end;",
    "chain3_int": S_DEF + "@info(name = 'query1') "
                  "from every e1=S[not (price > 20)] -> e2=S[x / -1 > e1.x] -> e3=S[d > e1.d or x == e2.price] "
                  "within 10 milliseconds "
                  f"select {G_SELECT}, e3.volume as v3 insert into Out;",
    "count": S_DEF + "partition with (sym of S) begin @info(name = 'query1') "
             "from every e1=S[price > 20] -> e2=S[price >= e1.price]<1:2> -> e3=S[volume != e1.price] "
             "within 30 milliseconds "
             "select e1.price as p1, e2[0].price as p20, e2[1].price as p21, e2[1].x / e1.x as q, "
             "e2[1].volume * e3.volume as vm, e3.d as d3 insert into Out; end;",
    "and": S_DEF + "partition with (sym of S) begin @info(name = 'query1') "
           "from every (e1=S[price != price] and e2=S[x < 3]) -> e3=S[price * 2.0f > e2.price] "
           "within 30 milliseconds "
           f"select {G_SELECT}, e3.price as p3 insert into Out; end;",
}


def general_sends(n=1500, nk=3, seed=0, edge=True, batch=37):
    """[(stream, [(ts, [sym, price, volume, x, d]), ...]), ...] for the event API"""
    ts, keys, (p, v, x, d) = window_stream(n, nk, seed=50 + seed, edge=edge)
    rows = [(int(ts[i]), [f"K{int(keys[i])}", float(p[i]), int(v[i]), int(x[i]), float(d[i])]) for i in range(n)]
    return [("S", rows[a:a + batch]) for a in range(0, n, batch)]


# ---------------------------------------------------------------------------------
# aggregates
# ---------------------------------------------------------------------------------
AGG_SELECT = ("select e1.symbol as symbol, sum(e2.price) as total, avg(e1.price) as a1, "
              "count() as n, sum(e2.volume) as vol insert into Out; end;")
C2_AGG_FREE = ("define stream StockStream (symbol string, price float, volume long); "
               "partition with (symbol of StockStream) begin @info(name = 'query1') "
               "from every e1=StockStream[price > -1.0f] -> e2=StockStream[symbol==e1.symbol and price>e1.price] "
               "within 1 sec " + AGG_SELECT)
# no threshold at all and `>=`: every event but NaN opens and -inf / +inf are consumed by
# their equals, so -inf, -FLT_MAX and -0.0 reach both sums, and inf + -inf makes them NaN
C2_AGG_OPEN = (C2_AGG_FREE.replace("[price > -1.0f]", "[price <= price]")
               .replace("price>e1.price", "price>=e1.price"))


AGG_SHAPE = (100_003, 2048)      # the bucketed engine's gate is 1,024 keys and one 8,192-event tile
AGG_SHARE = 0.1
# the classes the exact parallel carries accept (finite whole units of 2^-24 below 2^53,
# see DESIGN.md "Values"): signed zeros, the neighbours of the threshold, 2^24 and 2^24 + 2
AGG_EXACT_SMALL = [0.0, -0.0, 20.0, F32_ABOVE_20, F32_BELOW_20]
AGG_EXACT_F32 = np.array(AGG_EXACT_SMALL + [16777216.0, 16777218.0], dtype=np.float32)


def agg_stream(n, nk, double=False, edge=True, share=0.25, exact=False):
    """the stock stream with salted prices (as float or double) and volumes; a smaller
    `share` keeps a key's running sums finite for longer. `exact`: prices salted from
    AGG_EXACT_F32 only (the volumes still from the whole long pool: they wrap)"""
    ts, k, p, v = synth.stock_stream(n, nk, 100)
    if double:
        p = p.astype(np.float64)
    if edge:
        rng = np.random.default_rng(800)
        p = salt(p, AGG_EXACT_F32 if exact else None, share=share, rng=rng)
        v = salt(v, share=share, rng=rng)
    return ts, k, p, v
