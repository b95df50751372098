"""Shared pieces of the `group by` post-pass tests (tests/test_group_post_cases.py,
tests/test_gpu_group_post.py): the segment pass of siddhi_amd/csrc/sh_group.hip
(shg_segments) and sha_running_grouped of sh_agg.hip, called on their own on small
planted rows and compared with a numpy restatement that shares nothing with them.

Held fixed here:
  * the group word rule (`words_ref`), restated from DESIGN.md's `group by` section:
    every NaN of a type one group, -0.0 and +0.0 two, int / long / bool / string ids by
    value, a float column as the 4-byte float it is;
  * the contract of the pass (`segments_ref`): sidx the stable order by (query, key,
    word_0, word_1, ...), words compared as unsigned 64-bit numbers, and sseg a dense id
    per sorted position, non-decreasing from 0;
  * the ctypes mirrors of sha_group_q / sha_groups (tests/group_host --layout prints the
    header's sizes, test_group_post_cases.py compares);
  * the shapes and sizes, as data;
  * the running values: agg_post_cases.reference, the per-segment left-to-right
    restatement, over the grouped segments; and the 0 / 1 class of a case from exact
    integer arithmetic (`classify`).

Nothing here imports torch or touches the GPU at import time."""
import ctypes as C
import functools
import subprocess

import numpy as np

import agg_post_cases as ap

STRING, INT, LONG, FLOAT, DOUBLE, BOOL = 0, 1, 2, 3, 4, 5
SH_MAX_GROUP = 4
SHG_MAX_QUERIES = 16
SHG_TILE = 1024            # rows per head-flag tile
SCAN_TILE = 1024           # shd_exclusive_scan: beyond that many counts a second level


class sha_group_q(C.Structure):
    _fields_ = [("n", C.c_int32), ("col", C.c_int32 * SH_MAX_GROUP), ("type", C.c_int32 * SH_MAX_GROUP),
                ("pad", C.c_int32 * 3)]


class sha_groups(C.Structure):
    _fields_ = [("n_query", C.c_int32), ("pad", C.c_int32), ("q", sha_group_q * SHG_MAX_QUERIES)]


def descriptor(groups):
    """groups: per query [(col, type)]"""
    G = sha_groups(n_query=len(groups))
    for q, g in enumerate(groups):
        G.q[q].n = len(g)
        for i, (col, t) in enumerate(g):
            G.q[q].col[i], G.q[q].type[i] = col, t
    return G


def bind(L):
    """the prototypes of the grouped entry points on the product library"""
    import device_prims as dp
    vp, pvp = C.c_void_p, C.POINTER(C.c_void_p)
    L.shg_scratch_bytes.argtypes = [C.c_int64]
    L.shg_scratch_bytes.restype = C.c_int64
    L.shg_segments.argtypes = [vp, vp, C.c_int32, C.c_int64, vp, C.c_int32, vp, C.c_int32, C.c_uint64,
                               C.POINTER(sha_groups), vp, vp, pvp, pvp]
    L.shg_segments.restype = C.c_int
    L.sha_grouped_scratch_bytes.argtypes = [C.c_int64, C.c_int]
    L.sha_grouped_scratch_bytes.restype = C.c_int64
    L.sha_running_grouped.argtypes = [vp, vp, C.c_int32, C.c_int64, vp, C.c_int32, vp, C.c_int32, C.c_uint64,
                                      C.POINTER(dp.sha_desc), C.POINTER(sha_groups), vp, vp]
    L.sha_running_grouped.restype = C.c_int
    return L


# ------------------------------------------------------------------ the rule, restated
def words_ref(raw, t):
    """raw 8-byte row words of one column -> group words (uint64)"""
    raw = np.asarray(raw, np.int64)
    if t == FLOAT:
        b = (raw & 0xFFFFFFFF).astype(np.uint32)
        b = np.where(np.isnan(b.view(np.float32)), np.uint32(0x7FC00000), b)
        return b.astype(np.uint64)
    if t == DOUBLE:
        b = raw.view(np.uint64).copy()
        b[np.isnan(raw.view(np.float64))] = np.uint64(0x7FF8000000000000)
        return b
    if t == LONG:
        return raw.view(np.uint64).copy()
    if t == BOOL:
        return (raw != 0).astype(np.uint64)
    return (raw & 0xFFFFFFFF).astype(np.uint64)       # int, string id


def row_words(vals, query, groups):
    """[m, SH_MAX_GROUP] group words; a query with fewer attributes has zeros"""
    m = len(vals)
    q = np.zeros(m, np.int64) if query is None else np.asarray(query, np.int64)
    W = np.zeros((m, SH_MAX_GROUP), np.uint64)
    for qi, g in enumerate(groups):
        rows = q == qi
        for i, (col, t) in enumerate(g):
            W[rows, i] = words_ref(vals[rows, col], t)
    return W


def segments_ref(vals, query, key, n_keys, groups):
    """(sidx, sseg) of the contract"""
    m = len(vals)
    q = np.zeros(m, np.int64) if query is None else np.asarray(query, np.int64)
    k = np.zeros(m, np.int64) if key is None else np.asarray(key, np.int64)
    W = row_words(vals, query, groups)
    cols = [W[:, i] for i in range(SH_MAX_GROUP - 1, -1, -1)] + [k, q]      # lexsort: the last key first
    order = np.lexsort(cols) if m else np.zeros(0, np.int64)
    full = np.concatenate([q[:, None].astype(np.uint64), k[:, None].astype(np.uint64), W], axis=1)[order]
    head = np.ones(m, bool)
    head[1:] = (full[1:] != full[:-1]).any(axis=1)
    sseg = np.cumsum(head) - 1
    return order.astype(np.uint32), sseg.astype(np.uint32)


# ------------------------------------------------------------------ the stand-alone program
def write_job(path, vals, query, key, groups):
    m, n_out = vals.shape
    G = descriptor(groups)
    q = np.zeros(m, np.int32) if query is None else np.asarray(query, np.int32)
    k = np.zeros(m, np.int32) if key is None else np.asarray(key, np.int32)
    with open(path, "wb") as f:
        f.write(np.array([len(groups), n_out], np.int32).tobytes())
        f.write(np.array([m], np.int64).tobytes())
        f.write(bytes(G)[8:8 + len(groups) * C.sizeof(sha_group_q)])
        f.write(q.tobytes())
        f.write(k.tobytes())
        f.write(np.ascontiguousarray(vals, np.int64).tobytes())


def run_host(prog, vals, query, key, groups, path):
    write_job(path, vals, query, key, groups)
    out = subprocess.run([prog, path], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0].split()[0] == "order" and out[1].split()[0] == "seg"
    return (np.array(out[0].split()[1:], np.int64).astype(np.uint32),
            np.array(out[1].split()[1:], np.int64).astype(np.uint32))


# ------------------------------------------------------------------ cases
# row layout of every shape: 0 a long, 1 a float, 2 sum(long)'s argument, 3 count(),
# 4 max(float)'s argument, 5 an untouched word
N_OUT = 6
DESC = [(2, ap.SUM, ap.LONG), (3, ap.COUNT, ap.INT), (4, ap.MAX, ap.FLOAT)]
SHAPES = ("one_group", "own_group", "interleave", "high_half", "low_half", "four_and_eight", "two_queries",
          "one_query_ungrouped")
BIG_M = SCAN_TILE * SHG_TILE + 1          # 1,025 head-flag tiles: the scan's second level
SIZES = (0, 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 17, BIG_M)
RUN_SIZES = (1, 65, 2049, 3 * 2048 + 17)  # sha_running_grouped: the restatement walks every segment in Python


class GCase(ap.Case):
    """an agg_post_cases.Case whose segments are (query, key, group words)"""

    def __init__(self, name, vals, desc, query, n_query, key, n_keys, groups, seq_base=0):
        m = len(vals)
        seq = (np.uint64(seq_base) + np.arange(m, dtype=np.uint64)).astype(np.uint64)
        table = None if key is None else np.asarray(key, np.int32).copy()
        super().__init__(name, vals, desc, query, n_query, np.zeros(m, np.int32) if key is None else key, n_keys, seq,
                         seq_base, table)
        self.groups = groups
        self.m, self.n_out = vals.shape

    def group(self):
        order, sseg = segments_ref(self.vals, self.query, self.key, self.n_keys, self.groups)
        g = np.empty(self.m, np.int64)
        g[order.astype(np.int64)] = sseg
        return g


@functools.lru_cache(maxsize=8)
def shape_case(shape, m):
    rng = np.random.default_rng(SHAPES.index(shape) * 7919 + m)
    vals = rng.integers(-2 ** 62, 2 ** 62, (m, N_OUT)).astype(np.int64)
    vals[:, 2] = rng.integers(-2 ** 40, 2 ** 40, m)
    vals[:, 4] = ap.encode(rng.integers(-50, 50, m) * 0.5, ap.FLOAT)
    n_keys, n_query, query = 5, 1, None
    key = rng.integers(0, n_keys, m).astype(np.int32)
    groups = [[(0, LONG)]]
    if shape == "one_group":
        vals[:, 0] = 7
        key[:] = 3
    elif shape == "own_group":
        vals[:, 0] = rng.permutation(m).astype(np.int64) * 0x100000001 - 2 ** 40
    elif shape == "interleave":
        # three groups that every key has: a pass that ignores the key, or the group, differs
        vals[:, 0] = rng.integers(0, 3, m) - 1
    elif shape == "high_half":
        vals[:, 0] = (rng.integers(0, 4, m) << 32) + 5
    elif shape == "low_half":
        vals[:, 0] = (9 << 40) + rng.integers(0, 4, m)
    elif shape == "four_and_eight":
        f = np.array([0.0, -0.0, 1.5, np.nan], np.float32).view(np.uint32).astype(np.int64)
        f = np.concatenate([f, [0x7FA00001, 0xFFC00000]])           # NaNs of other payloads and sign
        # (the float's upper row half holds arbitrary bits: the column is 4 bytes wide)
        vals[:, 1] = f[rng.integers(0, len(f), m)] | (rng.integers(0, 2 ** 31, m) << 32)
        vals[:, 0] = rng.integers(0, 2, m) << 33
        groups = [[(1, FLOAT), (0, LONG)]]
    elif shape == "two_queries":
        # equal values under both queries; query 1 does not group
        n_query = 2
        query = rng.integers(0, 2, m).astype(np.int32)
        vals[:, 0] = rng.integers(0, 3, m)
        groups = [[(0, LONG)], []]
    elif shape == "one_query_ungrouped":
        groups = [[]]
    else:
        raise ValueError(shape)
    return GCase(f"{shape}_{m}", vals, DESC, query, n_query, key, n_keys, groups, seq_base=11)


def planted(split):
    """sum(double) over one key: 2^53 and then 1.0 in one group (split False: 2^53 + 1 is no
    double, the pass must answer 1) or in two groups of that key (split True: every
    running value is exact, it must answer 0; a pass that ignores the groups would refuse)"""
    m = 40
    rng = np.random.default_rng(5 + split)
    vals = rng.integers(-2 ** 62, 2 ** 62, (m, 3)).astype(np.int64)
    x = rng.integers(-8, 8, m) * 0.25
    g = rng.integers(0, 2, m)
    x[7], x[8], g[7] = 2.0 ** 53, 1.0, 0
    g[8] = 1 if split else 0
    rest = g == 0                       # nothing else on the large group: its total is 2^53 (+ 1)
    rest[[7, 8]] = False
    x[rest] = 0.0
    vals[:, 1] = ap.encode(x, ap.DOUBLE)
    vals[:, 0] = g
    return GCase(f"planted_{'split' if split else 'joined'}", vals, [(1, ap.SUM, ap.DOUBLE)], None, 1,
                 np.zeros(m, np.int32), 1, [[(0, INT)]])


# ------------------------------------------------------------------ end to end: the apps
INSERT_OUT = " insert into Out;"
N_BULK, NK_BULK = 200_000, 2_000      # the stream of tests/test_gpu_rate_fast.py (bulk_stream)


def _c2_select(select, clause):
    from siddhi_amd import synth
    head = synth.C2_QUERY[:synth.C2_QUERY.index("select ")]
    return head + "select " + select + " " + clause + INSERT_OUT + " end;"


SELECT_LONG = "e1.symbol as symbol, e2.volume as v2, sum(e2.volume) as tv, count() as n"
SELECT_FLOAT = "e1.symbol as symbol, e2.volume as v2, sum(e2.price) as total, count() as n"
GROUP = "group by e2.volume"
HAVING_N = 3                              # `having n > 3`: the oracle keeps some rows and drops some
C2_GROUP = _c2_select(SELECT_LONG, GROUP)
C2_UNGROUPED = _c2_select(SELECT_LONG, "").replace("  insert", " insert")
C2_GROUP_HAVING = _c2_select(SELECT_LONG, GROUP + f" having n > {HAVING_N}")
C2_GROUP_EVERY3 = _c2_select(SELECT_LONG, GROUP + " output every 3 events")
C2_GROUP_FLOAT = _c2_select(SELECT_FLOAT, GROUP)
# the oracle's rows on the bulk stream (test_group_post_cases.py asserts them)
C2_ROWS = {C2_GROUP: 147_118, C2_UNGROUPED: 147_118, C2_GROUP_FLOAT: 147_118, C2_GROUP_HAVING: 9_621,
           C2_GROUP_EVERY3: 145_332}
C2_GROUPS = (81_950, 1_766, 81)           # (key, group) pairs, keys with rows, most groups under one key
# what stays on the general engine / what the fast engines take (sh_compile accepts all:
# test_group_post_cases.py reads which engine from the chain engine's refusal)
C2_NOT_SELECTED = _c2_select("e1.symbol as symbol, sum(e2.volume) as tv, count() as n", GROUP)
C2_OTHER_EVENT = _c2_select(SELECT_LONG, "group by e1.volume")
C2_ARITHMETIC = _c2_select("e1.symbol as symbol, e2.volume + 1 as v2, sum(e2.volume) as tv", GROUP)
C2_ORDERED = _c2_select(SELECT_LONG, GROUP + " order by n")
C2_NO_AGGREGATOR = _c2_select("e1.symbol as symbol, e2.volume as v2", GROUP)
C2_ROWS[C2_NO_AGGREGATOR] = 147_118        # the clause has no effect on the rows
C2_TWO_ATTRS = _c2_select("e1.symbol as symbol, e2.volume as v2, e1.price as p1, sum(e2.volume) as tv",
                          "group by e2.volume, e1.price")

RULE_SELECT = "e2.merchant as merchant, sum(e2.merchant) as tm, count() as n"
RULE_CASES = (1, 3, 7, 8)                 # tests/rules_cases.CASES of 2..16 rules
RULE_ROWS = {1: 12_513, 3: 6_052, 7: 490, 8: 6_430}      # the oracle's rows


# a set whose start filters open few partials per card (24,767 over 600 cards: below the
# sparse path's 64 per key and 65,536 in all), so the sparse-partial path takes it;
# built by rules_cases.case_data like the others
RULE_SPARSE_CASE = (30000, 600, 6, 20, 4096, 3, True, (), 23)
RULE_SPARSE_ROWS = 3_566
RULE_SPARSE_PARTIALS = 24_767


def rule_case(ci):
    from rules_cases import CASES
    return RULE_SPARSE_CASE if ci == "sparse" else CASES[ci]


def rule_text(plain, select=RULE_SELECT, clause="group by e2.merchant"):
    """a rules_cases text with the grouped select in every rule"""
    from having_fast_cases import PLAIN
    ins = " insert into Alerts;"
    return plain.replace(PLAIN, select).replace(ins, " " + clause + ins)


_bulk = {}


def bulk_stream():
    from siddhi_amd import synth
    if "s" not in _bulk:
        _bulk["s"] = synth.stock_stream(N_BULK, NK_BULK, 100)
    return _bulk["s"]


def bulk_oracle(text):
    """(seq, ts, values, nulls) of the oracle on the bulk stream"""
    from oracle_engine import run_columns_oracle
    from siddhi_amd import compiler
    if text not in _bulk:
        ts, k, p, v = bulk_stream()
        _bulk[text] = run_columns_oracle(compiler.compile_app(text), ts, [k, p, v], k)
    return _bulk[text]


def classify(case):
    """accept / refuse from the exact running sums as Python integers (units of 2^-1074):
    refuse when some sequential double sum is not the exact one. The cases here keep
    inside the 96-bit range and the double range, so there is no third class."""
    for col, kind, t in ap.fp_columns(case):
        x = ap.as_double(case.vals[:, col], t)
        assert np.isfinite(x).all()
        rg = ap.addend_range(x)
        assert rg is None or rg[1] - rg[0] + 1 <= 96
        for ix, run in ap.exact_running(case, col, t):
            seq = np.add.accumulate(np.concatenate(([0.0], x[ix])))[1:]
            for e, s in zip(run, seq.tolist()):
                d = ap.exact_to_double(e)
                assert d is None or abs(d) != float("inf")
                if d is None or d != s:
                    return "refuse"
    return "accept"
