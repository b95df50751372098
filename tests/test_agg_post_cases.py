"""CPU side of the aggregate post-pass tests (tests/agg_post_cases.py): the plain
reference against the product's own sequential walk (sh_agg_seq.h shq_walk, built with
g++ as tests/agg_seq_host), the theorem the parallel pass relies on (exact running
values of at most 53 bits are the sequential results), and the premises of the case
list, computed from the data, so that a later edit cannot empty a class silently."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import agg_post_cases as ap

HERE = os.path.dirname(os.path.abspath(__file__))
ALL = ap.CASES


@pytest.fixture(scope="module")
def walk():
    d = os.path.join(HERE, "agg_seq_host")
    subprocess.run(["make", "-s", "-C", d], check=True)
    lib = C.CDLL(os.path.join(d, "libaggseqhost.so"))
    lib.agq_create.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.agq_create.restype = C.c_void_p
    lib.agq_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
    lib.agq_step.restype = C.c_int
    lib.agq_destroy.argtypes = [C.c_void_p]
    lib.agq_destroy.restype = None
    return lib


def _walked(walk, case):
    cols = np.array([c for c, k, t in case.desc], np.int32)
    kinds = np.array([k for c, k, t in case.desc], np.int32)
    types = np.array([t for c, k, t in case.desc], np.int32)
    h = walk.agq_create(len(case.desc), cols.ctypes.data, kinds.ctypes.data, types.ctypes.data)
    assert h
    vals = np.ascontiguousarray(case.vals).copy()
    q = np.ascontiguousarray(case.query if case.query is not None else np.zeros(case.m, np.int32))
    key = np.ascontiguousarray(case.key)
    assert walk.agq_step(h, vals.ctypes.data, case.n_out, case.m, q.ctypes.data, key.ctypes.data, 0) == 0
    walk.agq_destroy(h)
    return vals


def _same(case, got, want):
    g, w = ap.canon(case, got), ap.canon(case, want)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, (case.name, "first differing (row, column)", bad[0].tolist(), hex(int(g[tuple(bad[0])])),
                           hex(int(w[tuple(bad[0])])))


@pytest.mark.parametrize("case", ALL + [ap.salted_case(ap.DOUBLE), ap.salted_case(ap.FLOAT)], ids=repr)
def test_reference_is_the_products_sequential_walk(walk, case):
    """bit for bit (all NaNs of a column as one value), the other columns untouched"""
    _same(case, _walked(walk, case), ap.reference(case))
    other = [c for c in range(case.n_out) if c not in ap.agg_columns(case)]
    assert np.array_equal(ap.reference(case)[:, other], case.vals[:, other])


def test_reference_of_the_large_case(walk):
    case = ap.big_case()
    assert case.m == 1024 * 2048 + 2049 and len(case.desc) == 2
    assert (case.m + ap.TILE - 1) // ap.TILE > ap.CARRY_THREADS            # two tiles on a carry thread
    _same(case, _walked(walk, case), ap.reference(case))
    assert ap.classify(case) == "accept"


@pytest.mark.parametrize("case", [c for c in ALL if ap.classify(c) == "accept"], ids=repr)
def test_exact_running_values_are_the_sequential_results(case):
    """the theorem the pass relies on: where every exact running value has at most 53
    significant bits and lies inside the double range, the exact values converted to
    doubles are the reference's left-to-right results"""
    ref = ap.reference(case)
    for col, kind, t in ap.fp_columns(case):
        for ix, run in ap.exact_running(case, col, t):
            d = [ap.exact_to_double(e) for e in run]
            assert None not in d
            d = np.array(d, np.float64)
            if kind == ap.AVG:
                d = d / np.arange(1, len(ix) + 1, dtype=np.float64)
            assert np.array_equal(d.view(np.int64), ref[ix, col]), (case.name, col)


def _cls(name):
    return ap.classify(ap.BY_NAME[name])


def test_every_verdict_class_is_there():
    cls = [ap.classify(c) for c in ALL]
    assert cls.count("accept") >= 30 and cls.count("refuse") >= 10 and cls.count("either") >= 2
    # the refusals for each reason, and the two "either" reasons
    assert any(ap.stats(c)["sig"] > 53 and ap.stats(c)["range"] <= 96 for c in ALL if ap.classify(c) == "refuse")
    assert any(ap.stats(c)["sig"] <= 53 and ap.stats(c)["mismatch"] for c in ALL)      # the overflow that comes back
    assert any(ap.stats(c)["range"] > 96 for c in ALL if ap.classify(c) == "either")
    assert any(ap.stats(c)["out_of_range"] for c in ALL if ap.classify(c) == "either")
    for arg_type in (ap.DOUBLE, ap.FLOAT):
        c = ap.salted_case(arg_type)
        x = ap.as_double(c.vals[:, c.desc[0][0]], arg_type)
        assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
        assert (np.abs(x) == (ap.DBL_MAX if arg_type == ap.DOUBLE else float(np.finfo(np.float32).max))).any()


def test_the_53_bit_gate_cases():
    for sfx in ("", "_neg", "_far", "_far_neg"):
        sign = -1.0 if "neg" in sfx else 1.0
        acc, ref_, mid = (ap.BY_NAME[n + sfx] for n in ("g53_accept", "g53_refuse", "g53_middle"))
        assert [ap.classify(c) for c in (acc, ref_, mid)] == ["accept", "refuse", "refuse"]
        # the running values pass through exactly 2^53 - 1 and 2^53 / reach 2^53 + 1 / pass it on to 2^53 + 2
        run = {c.name: [e for ix, r in ap.exact_running(c, 1, ap.DOUBLE) for e in r] for c in (acc, ref_, mid)}
        u = lambda v: int(sign) * v << ap.SCALE     # noqa: E731
        assert u(2 ** 53 - 1) in run[acc.name] and u(2 ** 53) in run[acc.name]
        assert max(abs(e) for e in run[acc.name]) == 2 ** 53 << ap.SCALE
        assert u(2 ** 53 + 1) in run[ref_.name] and u(2 ** 53 + 2) not in run[ref_.name]
        assert u(2 ** 53 + 1) in run[mid.name]
        # ... whose segment ends on a representable value: its tail alone would pass
        segs = ap.exact_running(mid, 1, ap.DOUBLE)
        assert all(ap.exact_to_double(r[-1]) is not None for ix, r in segs)
        assert any(abs(r[-1]) == 2 ** 53 + 2 << ap.SCALE for ix, r in segs)
        if "far" in sfx:
            # the offending row lies in another tile than its segment's head
            for c in (ref_, mid):
                tiles, heads = ap.layout(c)
                row = ap.stats(c)["mismatch"][1]
                g = c.group()
                order = np.argsort(g, kind="stable")
                p = int(np.flatnonzero(order == row)[0])
                head = int(heads[heads <= p].max())
                assert p // ap.TILE > head // ap.TILE, (c.name, p, head)


def test_the_range_gate_cases():
    s = {n: ap.stats(ap.BY_NAME[n]) for n in ("range96", "range97", "range96_straddle", "shifts")}
    assert s["range96"]["range"] == 96 and s["range96"]["cls"] == "accept" and 95 in s["range96"]["shifts"]
    assert s["range97"]["range"] == 97 and s["range97"]["cls"] == "either" and s["range97"]["sig"] == 1
    # a 53-bit mantissa whose top bit is bit 95: shifted by 43 it straddles the two 64-bit words
    assert s["range96_straddle"]["range"] == 96 and s["range96_straddle"]["sig"] == 53
    assert 43 in s["range96_straddle"]["shifts"] and s["range96_straddle"]["cls"] == "accept"
    assert {0, 1, 63, 64, 65} <= s["shifts"]["shifts"] and s["shifts"]["cls"] == "accept"


def test_sign_and_magnitude_cases():
    c = ap.BY_NAME["cancel_to_zero"]
    ref = ap.reference(c)
    rows = ap._segments(c)[0]
    assert ap.as_double(c.vals[rows, 1], ap.DOUBLE).tolist() == [1.5, -1.5, -0.0, 2.0 ** -30]
    assert ref[rows, 1].tolist() == ap.encode([1.5, 0.0, 0.0, 2.0 ** -30], ap.DOUBLE).tolist()     # +0.0
    c = ap.BY_NAME["only_negative_zero"]
    assert (c.vals[:, 1] == np.int64(-2 ** 63)).all() and (ap.reference(c)[:, 1] == 0).all()
    # a negative carry into a tile without a head of that segment
    c = ap.BY_NAME["negative_carry"]
    tiles, heads = ap.layout(c)
    assert tiles == 2 and heads.tolist()[:2] == [0, 300] and heads[2] > ap.TILE + 300
    assert ap.as_double(ap.reference(c)[:, 1], ap.DOUBLE).min() == -(ap.TILE + 900.0)
    # large addends of both signs, a small sum
    c = ap.BY_NAME["alternating"]
    x = ap.as_double(c.vals[:, 1], ap.DOUBLE)
    assert (x > 2.0 ** 89).sum() == 1500 and (x < -2.0 ** 89).sum() == 1500 and ap.classify(c) == "accept"
    assert np.abs(ap.as_double(ap.reference(c)[c.key == 1, 1], ap.DOUBLE)).min() == 2.0 ** 40
    # subnormal outputs with q = -1074; the largest double; the overflow
    assert ap.stats(ap.BY_NAME["subnormal_sums"])["subnormal_out"] and _cls("subnormal_sums") == "accept"
    assert ap.addend_range(ap.as_double(ap.BY_NAME["subnormal_sums"].vals[:, 1], ap.DOUBLE))[0] == -1074
    assert ap.encode([ap.DBL_MIN], ap.DOUBLE)[0] in ap.reference(ap.BY_NAME["subnormal_sums"])[:, 1]
    assert _cls("float_subnormals") == "accept"
    assert ap.addend_range(ap.as_double(ap.BY_NAME["float_subnormals"].vals[:, 1], ap.FLOAT))[0] == -149
    c = ap.BY_NAME["dbl_max"]
    assert ap.classify(c) == "accept"
    assert {ap.DBL_MAX, -ap.DBL_MAX} <= set(ap.as_double(ap.reference(c)[:, 1], ap.DOUBLE).tolist())
    for n in ("overflow_and_back", "overflow_and_back_neg", "overflow_and_back_far"):
        c = ap.BY_NAME[n]
        st = ap.stats(c)
        # every exact value is one significant bit and the range is narrow: only the magnitude tells
        assert st["cls"] == "refuse" and st["sig"] == 1 and st["range"] <= 96 and not st["nonfinite"]
        seg = [ix for ix in ap._segments(c) if np.isinf(ap.as_double(ap.reference(c)[ix, 1], ap.DOUBLE)).any()][0]
        out = ap.as_double(ap.reference(c)[seg, 1], ap.DOUBLE)
        exact = ap.exact_running(c, 1, ap.DOUBLE)
        run = [r for ix, r in exact if ix[0] == seg[0]][0]
        assert np.isinf(out[-1]) and abs(run[-1]) == 2 ** 1023 << ap.SCALE       # the reference stays at infinity
    c = ap.BY_NAME["overflow_at_the_end"]
    assert ap.classify(c) == "either" and np.isinf(ap.as_double(ap.reference(c)[:, 1], ap.DOUBLE)).sum() == 1


def test_type_cases():
    c = ap.BY_NAME["every_kind"]
    assert {(k, t) for _, k, t in c.desc} >= {(k, t) for k in (ap.SUM, ap.AVG)
                                              for t in (ap.INT, ap.LONG, ap.FLOAT, ap.DOUBLE)} | {(ap.COUNT, ap.INT)}
    assert ap.classify(c) == "accept"
    c = ap.BY_NAME["avg_long_rounded_addends"]
    assert (np.abs(c.vals[:, 1]) > 2 ** 53).sum() == 3 and ap.classify(c) == "accept"
    assert (ap.as_double(c.vals[:, 1], ap.LONG).astype(np.int64) != c.vals[:, 1]).sum() == 3      # the addend is rounded
    assert _cls("avg_long_rounding_sum") == "refuse"
    c = ap.BY_NAME["sum_long_wraps"]
    ref = ap.reference(c)
    seg = ap._segments(c)[1]
    assert (c.vals[seg, 1] == ap.LONG_MAX).all() and (ref[seg[1:], 1] < ref[seg[:-1], 1]).any()   # wrapped
    for n in ("sum_long_wraps", "sum_int_min"):
        c = ap.BY_NAME[n]
        tiles, heads = ap.layout(c)
        assert ap.classify(c) == "accept" and not ap.fp_columns(c)
        assert heads[1] < ap.TILE < heads[1] + ap.TILE                       # the segment crosses the seam
    assert (ap.BY_NAME["sum_int_min"].vals[:, 1] == ap.INT_MIN).sum() == ap.TILE + 5
    assert [k for _, k, _ in ap.BY_NAME["count_only"].desc] == [ap.COUNT]


def test_layout_cases():
    tiles, heads = ap.layout(ap.BY_NAME["heads_at_seams"])
    assert heads.tolist() == [0, 1, ap.TILE - 1, ap.TILE] and tiles == 2
    tiles, heads = ap.layout(ap.BY_NAME["three_tiles"])
    assert tiles == 3 and not any(ap.TILE <= h < 2 * ap.TILE for h in heads)          # the middle tile has no head
    assert {ap.BY_NAME[f"rows_{m}"].m for m in (1, 2047, 2048, 2049, 3 * 2048 + 1)} == {1, 2047, 2048, 2049, 6145}
    for nk in (1, 3, 255, 256, 257):
        c = ap.BY_NAME[f"keys_{nk}"]
        assert c.n_keys == nk and len(np.unique(c.key)) == nk and (c.keys_table is None) == (nk == 1)
    assert ap.BY_NAME["keys_1"].query is None                                         # no sort at all
    c = ap.BY_NAME["queries_5"]
    assert c.n_query == 5 and len(np.unique(c.query)) == 5 and c.keys_table is not None
    c = ap.BY_NAME["queries_5_no_keys"]
    assert c.n_query == 5 and len(np.unique(c.query)) == 5 and c.keys_table is None
    c = ap.BY_NAME["query_array_absent"]
    assert c.n_query == 5 and c.query is None
    c = ap.BY_NAME["query_array_of_one"]
    assert c.n_query == 1 and c.query is not None
    c = ap.BY_NAME["seq_base_and_gaps"]
    off = (c.seq - np.uint64(c.seq_base)).astype(np.int64)
    assert c.seq_base > 2 ** 32 and (np.diff(off) > 1).any() and np.array_equal(c.keys_table[off], c.key)
    assert len(c.keys_table) > c.m
    assert [len(ap.BY_NAME[n].desc) for n in ("one_column", "rows_2049", "sixteen_columns")] == [1, 2, ap.MAX_COLS]
    for n in ("rows_2049", "sixteen_columns", "every_kind"):
        c = ap.BY_NAME[n]
        assert c.n_out > len(c.desc)                                                  # among other columns
    assert len({(k, t) for _, k, t in ap.BY_NAME["sixteen_columns"].desc}) == len(ap.ALL_KINDS)
    c = ap.BY_NAME["extremes_beside_refusal"]
    assert {k for _, k, _ in c.desc} == {ap.MAX, ap.SUM, ap.MIN} and ap.classify(c) == "refuse"
    ref = ap.reference(c)
    assert not np.array_equal(ref[:, 0], c.vals[:, 0]) and not np.array_equal(ref[:, 3], c.vals[:, 3])
    assert _cls("extremes_beside_exact") == "accept"
    # no case but the large one is beyond a few thousand rows
    assert max(c.m for c in ALL) <= 3 * ap.TILE + 1


# ---- the planted streams, from the oracle alone
def _planted_rows(ref, k, kk):
    mine = k[ref["seq"].astype(np.int64)] == kk
    return ref["seq"].astype(np.int64)[mine], ref["values"][mine]


@pytest.mark.parametrize("which", ["below", "above"])
def test_bucketed_gate_streams_pass_through_the_boundary(which):
    """the planted key's running total in the oracle, and the exact sums in k_bk_aggp's
    units: 2^53 - 1 at most on one stream, 2^53 + 1 (which the oracle rounds) on the other"""
    from fractions import Fraction
    from siddhi_amd import compiler
    ts, k, p, v, kk = ap.bk_gate_stream(which)
    assert (len(ts), int(k.max()) + 1) == ap.BK_SHAPE and ap.BK_SHAPE[0] >= 8192 and ap.BK_SHAPE[1] == 1024
    assert compiler.compile_app(ap.BK_GATE_APP) is not None
    ref = ap.bk_gate_ref(which)
    seq, rows = _planted_rows(ref, k, kk)
    assert rows[:, 1].view(np.float64).tolist() == ap.BK_TOTALS[which]
    assert rows[:, 2].tolist() == list(range(1, len(rows) + 1))
    exact = np.cumsum([Fraction(x) / Fraction(ap.U) for x in p[seq].tolist()]).tolist()
    assert exact == ap.BK_EXACT_UNITS[which] and all(e.denominator == 1 for e in exact)
    assert (max(exact) == 2 ** 53 - 1) if which == "below" else (2 ** 53 + 1 in exact)
    if which == "above":
        assert float(2 ** 53 + 1) == 2.0 ** 53            # why `>` in place of `>=` would keep it
    # every other key's sums are whole units far below the gate
    other = k[ref["seq"].astype(np.int64)] != kk
    tot = ref["values"][other, 1].view(np.float64) / ap.U
    assert np.array_equal(tot, np.trunc(tot)) and np.abs(tot).max() < 2.0 ** 40
    assert len(ref["seq"]) > 1000


def test_overflow_stream_goes_to_infinity_and_takes_a_negative_addend():
    ts, k, p, v, kk = ap.overflow_stream()
    ref = ap.overflow_ref()
    seq, rows = _planted_rows(ref, k, kk)
    total, addend = rows[:, 1].view(np.float64), p[seq]
    assert total[0] == 2.0 ** 1023 and np.isposinf(total[1:]).all() and len(total) >= 3
    assert addend[:3].tolist() == [2.0 ** 1023, 2.0 ** 1023, -2.0 ** 1023]
    # the exact sum after the third row is 2^1023 again: one significant bit, inside the range
    assert sum(ap.units(x) for x in addend[:3].tolist()) == 2 ** 1023 << ap.SCALE
    # the column's addends lie within the pass's 96 bits, so only the magnitude can refuse
    lo, hi = ap.addend_range(p[ref["seq"].astype(np.int64)])
    assert hi == 1023 and hi - lo + 1 <= 96
    a1 = ref["values"][:, 2].view(np.float64)
    assert np.isfinite(a1[k[ref["seq"].astype(np.int64)] != kk]).all()
