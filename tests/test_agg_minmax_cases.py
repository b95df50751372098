"""max(x) / min(x) on the fast engines, the CPU side: rule sets of more than 16
queries with such a select lower through sh_compile; the product's sequential walk
(siddhi_amd/csrc/sh_agg_seq.h) compiled for the CPU reproduces the oracle's rows bit
for bit, carried across drain groups, and follows the rule on hand-planted edge
values; and the cases of tests/agg_minmax_cases.py hold what the GPU tests rely on
(checked from the oracle alone)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from agg_minmax_cases import (E_MAIN, E_ONE, EDGE_ARGS, EDGE_LAYOUT, EDGE_TEXT, LAYOUT, M1, M2, M3, M5, MINMAX_CASES,
                              SH_AGG_MAX, SH_AGG_MIN, SH_T_DOUBLE, SH_T_FLOAT, SH_T_INT, SH_T_LONG, edge_data,
                              edge_oracle, extreme_sequential, running_extreme, tile_classes, typed)
from rules_stream_agg_cases import PLAIN, agg_data, agg_ref, args_rows, row_groups, row_keys, segments
from rules_stream_cases import compiled, stream_data
from siddhi_amd import abi, build

HERE = os.path.dirname(os.path.abspath(__file__))
BY_NAME = {ac[0]: ac for ac in MINMAX_CASES}


@pytest.fixture(scope="module")
def lib():
    return abi.bind_product(C.CDLL(build.build()))


# ---- lowering
@pytest.mark.parametrize("name", ["M1", "M2", "M3"])
def test_max_min_rule_sets_beyond_the_general_engine_lower(lib, name):
    """the 17-rule S2 set, the 40-rule S1 set and the unpartitioned S3 set"""
    ac = BY_NAME[name]
    assert ac[1][2] > 16  # the general engine's query table holds 16
    text, args_text, data = agg_data(ac)
    for t in (text, args_text):
        d = compiled(ac[1], t).descriptor()
        h = C.c_void_p()
        rc = lib.sh_compile(C.byref(d), C.byref(h))
        assert rc == abi.SH_OK, lib.sh_last_error(h)
        lib.sh_destroy(h)


def test_rules_aggregating_different_positions_are_still_refused(lib):
    text, rules, data = stream_data(M1[1])
    mixed = text.replace(PLAIN, "max(e2.amount) as hi, e1.amount as lo", 1).replace(
        PLAIN, "e2.amount as hi, min(e1.amount) as lo")
    d = compiled(M1[1], mixed).descriptor()
    h = C.c_void_p()
    rc = lib.sh_compile(C.byref(d), C.byref(h))
    assert rc == abi.SH_E_UNSUPPORTED
    if h:
        assert b"different select positions" in lib.sh_last_error(h)
        lib.sh_destroy(h)


# ---- the walk on the CPU
@pytest.fixture(scope="module")
def walk():
    d = os.path.join(HERE, "agg_seq_host")
    subprocess.run(["make", "-s", "-C", d], check=True)
    lib = C.CDLL(os.path.join(d, "libaggseqhost.so"))
    lib.agq_create.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.agq_create.restype = C.c_void_p
    lib.agq_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
    lib.agq_step.restype = C.c_int
    lib.agq_entries.argtypes = [C.c_void_p]
    lib.agq_entries.restype = C.c_int64
    lib.agq_destroy.argtypes = [C.c_void_p]
    lib.agq_destroy.restype = None
    return lib


def _create(walk, lay):
    cols = np.array([c for c, k, t in lay], np.int32)
    kinds = np.array([k for c, k, t in lay], np.int32)
    types = np.array([t for c, k, t in lay], np.int32)
    h = walk.agq_create(len(lay), cols.ctypes.data, kinds.ctypes.data, types.ctypes.data)
    assert h
    return h


def _walk_case(walk, ac, carry=True, one_step=False):
    """the oracle's rows with the arguments put back, walked drain group by drain
    group with the table carried; returns (values, table entries)"""
    rows, args = agg_ref(ac)[3], args_rows(ac)
    assert np.array_equal(rows["seq"], args["seq"]) and np.array_equal(rows["query"], args["query"])
    h = _create(walk, LAYOUT[ac[2]])
    n_out = args["values"].shape[1]
    vals = np.ascontiguousarray(args["values"], np.int64).copy()
    q = np.ascontiguousarray(rows["query"], np.int32)
    key = np.ascontiguousarray(row_keys(ac, rows), np.int32)
    grp = np.zeros(len(q), np.int64) if one_step else row_groups(ac, rows)
    assert np.all(np.diff(grp) >= 0)
    for g in np.unique(grp):
        ix = np.nonzero(grp == g)[0]
        lo, hi = int(ix[0]), int(ix[-1]) + 1
        assert hi - lo == len(ix)
        part = np.ascontiguousarray(vals[lo:hi])
        assert walk.agq_step(h, part.ctypes.data, n_out, hi - lo, q[lo:hi].ctypes.data, key[lo:hi].ctypes.data,
                             1 if carry else 0) == 0
        vals[lo:hi] = part
    entries = walk.agq_entries(h)
    walk.agq_destroy(h)
    return vals, entries


@pytest.mark.parametrize("name", list(BY_NAME))
def test_cpu_walk_reproduces_the_oracle(walk, name):
    ac = BY_NAME[name]
    rows = agg_ref(ac)[3]
    assert len(rows["seq"]) > 0
    vals, entries = _walk_case(walk, ac)
    for c in range(3):
        assert np.array_equal(vals[:, c], rows["values"][:, c]), c
    assert entries == len(segments(ac, rows))


@pytest.mark.parametrize("name", ["M1", "M5"])
def test_cpu_walk_split_invariance_and_no_carry(walk, name):
    """walked in one step: the same values; without the carried table: others (a
    segment's extreme lies in an earlier drain group)"""
    ac = BY_NAME[name]
    rows = agg_ref(ac)[3]
    once = _walk_case(walk, ac, one_step=True)[0]
    assert np.array_equal(once[:, :3], rows["values"][:, :3])
    fresh = _walk_case(walk, ac, carry=False)[0]
    assert not np.array_equal(fresh[:, 1], rows["values"][:, 1])


# ---- edge values, straight into the walk (no filter screens them)
def _f32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _f64(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


NAN, INF = float("nan"), float("inf")
NAN2_F32 = 0x7FC00123  # a NaN with a payload: the bits must come through unchanged
IMIN, IMAX = -2 ** 31, 2 ** 31 - 1
# segments of arguments (each walked under max and under min)
FLOAT_SEGMENTS = [
    [NAN, 1.0, 2.0, -INF],                 # NaN first: every row is that NaN
    [1.0, NAN, 2.0, NAN, 0.5],             # NaN in the middle never replaces
    [-0.0, 0.0, -0.0],                     # the first zero stays
    [0.0, -0.0, 0.0],
    [-1.0, -0.0, 0.0, 1.0, INF, INF, -INF],
    [INF, 1.0, -INF, NAN],
    [-INF, -INF, NAN, -0.0, 0.0],
    [3.5],
]
INT_SEGMENTS = [[IMIN, -5, IMAX, 0], [IMAX, IMIN], [-3, -2, -7, -2], [0, IMIN, IMIN, -1], [7]]
LONG_SEGMENTS = [[2 ** 60, 2 ** 60 + 1, 2 ** 60], [2 ** 60 + 1, 2 ** 60, 2 ** 60 + 2], [-2 ** 60, -2 ** 60 - 1, -2 ** 60 + 1],
                 [-2 ** 63, 2 ** 63 - 1, 0], [2 ** 53, 2 ** 53 + 1, 2 ** 53 - 1], [-4, -9, IMIN - 1]]


def _edge_walk(walk, segs, arg_type, encode):
    """every segment as one key of query 0, rows interleaved round-robin; columns 0 / 1:
    max / min of the same arguments. Returns per segment (values, max bits, min bits)."""
    order = []
    for i in range(max(len(s) for s in segs)):
        order += [(k, i) for k, s in enumerate(segs) if i < len(s)]
    raw = np.array([encode(segs[k][i]) for k, i in order], np.int64)
    key = np.array([k for k, i in order], np.int32)
    vals = np.ascontiguousarray(np.stack([raw, raw], axis=1))
    h = _create(walk, [(0, SH_AGG_MAX, arg_type), (1, SH_AGG_MIN, arg_type)])
    q = np.zeros(len(key), np.int32)
    # two steps with the table carried: the second continues the first's states
    half = len(key) // 2
    for lo, hi in ((0, half), (half, len(key))):
        part = np.ascontiguousarray(vals[lo:hi])
        assert walk.agq_step(h, part.ctypes.data, 2, hi - lo, q[lo:hi].ctypes.data, key[lo:hi].ctypes.data, 1) == 0
        vals[lo:hi] = part
    walk.agq_destroy(h)
    out = []
    for k, s in enumerate(segs):
        ix = np.nonzero(key == k)[0]
        out.append((s, raw[ix], vals[ix, 0], vals[ix, 1]))
    return out


@pytest.mark.parametrize("what", ["float", "double", "int", "long"])
def test_cpu_walk_follows_the_rule_on_edge_values(walk, what):
    segs, arg_type, encode = {
        "float": (FLOAT_SEGMENTS, SH_T_FLOAT, _f32), "double": (FLOAT_SEGMENTS, SH_T_DOUBLE, _f64),
        "int": (INT_SEGMENTS, SH_T_INT, lambda v: v),
        "long": (LONG_SEGMENTS, SH_T_LONG, lambda v: v)}[what]
    for s, raw, hi, lo in _edge_walk(walk, segs, arg_type, encode):
        for kind, got in ((SH_AGG_MAX, hi), (SH_AGG_MIN, lo)):
            want = raw[extreme_sequential(s, kind)]
            assert np.array_equal(got, want), (what, s, kind, got.tolist(), want.tolist())


def test_cpu_walk_keeps_a_nan_payload_and_narrow_raw_bits(walk):
    """a head NaN with a payload comes through bit for bit; a float column's raw word
    is the float's bits zero-extended, whichever argument wins"""
    enc = lambda v: NAN2_F32 if isinstance(v, str) else _f32(v)
    (s, raw, hi, lo), (s2, raw2, hi2, lo2) = _edge_walk(walk, [["nan*", 1.0, 2.0], [-1.5, "nan*", -2.5]],
                                                       SH_T_FLOAT, enc)
    assert hi.tolist() == [NAN2_F32] * 3 and lo.tolist() == [NAN2_F32] * 3
    assert hi2.tolist() == [_f32(-1.5)] * 3 and lo2.tolist() == [_f32(-1.5), _f32(-1.5), _f32(-2.5)]


def test_the_vectorised_restatement_is_the_rule():
    """running_extreme (what the largest GPU case is checked against) against the
    one-at-a-time rule on the planted segments"""
    for segs, arg_type, encode in ((FLOAT_SEGMENTS, SH_T_FLOAT, _f32), (FLOAT_SEGMENTS, SH_T_DOUBLE, _f64),
                                   (INT_SEGMENTS, SH_T_INT, lambda v: v), (LONG_SEGMENTS, SH_T_LONG, lambda v: v)):
        # the groups' rows interleaved round-robin, each group's in order
        order = []
        for i in range(max(len(s) for s in segs)):
            order += [(k, i) for k, s in enumerate(segs) if i < len(s)]
        group = np.array([k for k, i in order])
        raw = np.array([encode(segs[k][i]) for k, i in order], np.int64)
        for kind in (SH_AGG_MAX, SH_AGG_MIN):
            got = running_extreme(group, raw, kind, arg_type)
            for k, s in enumerate(segs):
                want = raw[group == k][extreme_sequential(s, kind)]
                assert np.array_equal(got[group == k], want), (arg_type, kind, s)


# ---- the cases, from the oracle alone
def _edge_segments(case):
    """{key: row indices in output order} and the rows of both texts"""
    rows, args = edge_oracle(case, EDGE_TEXT), edge_oracle(case, EDGE_ARGS)
    assert np.array_equal(rows["seq"], args["seq"])
    k = edge_data(case)[1]
    key = k[rows["seq"].astype(np.int64)]
    segs = {}
    for i, kk in enumerate(key.tolist()):
        segs.setdefault(kk, []).append(i)
    return rows, args, key, segs


def test_one_row_case_has_one_row():
    rows, args, key, segs = _edge_segments(E_ONE)
    assert len(rows["seq"]) == 1 and rows["seq"][0] == 9
    assert np.array_equal(rows["values"][0], args["values"][0])


def test_main_edge_case_holds_what_it_claims():
    rows, args, key, segs = _edge_segments(E_MAIN)
    n, span, heads, inside = tile_classes(key)
    print("rows", n, "longest span in tiles", span, "most heads in a tile", heads, "segments inside a tile", inside)
    assert n > 0 and span >= 3 and heads >= 100 and inside >= 1
    for col, kind, t in EDGE_LAYOUT:
        if t not in (SH_T_FLOAT, SH_T_DOUBLE):
            continue
        x = typed(args["values"][:, col], t)
        head_nan = mid_nan = neg_pos = pos_neg = kept_left = 0
        for ix in segs.values():
            v = x[ix]
            nan = np.isnan(v)
            head_nan += bool(nan[0])
            num = np.flatnonzero(~nan)
            mid_nan += bool(len(num) and np.any(nan[num[0]:]))
            nz = np.flatnonzero((v == 0) & np.signbit(v))
            pz = np.flatnonzero((v == 0) & ~np.signbit(v))
            neg_pos += bool(len(nz) and len(pz) and nz[0] < pz[-1])
            pos_neg += bool(len(nz) and len(pz) and pz[0] < nz[-1])
            # rows where a zero is the state while the argument is the other zero
            out = typed(rows["values"][ix, col], t)
            kept_left += int(np.sum((out == 0) & (v == 0) & (np.signbit(out) != np.signbit(v))))
        print("column", col, dict(head_nan=head_nan, mid_nan=mid_nan, neg_pos=neg_pos, pos_neg=pos_neg,
                                  kept_left=kept_left))
        assert head_nan >= 5 and mid_nan >= 5 and neg_pos >= 5 and pos_neg >= 5 and kept_left >= 5
    # edge ints and longs reach the rows
    assert np.any(args["values"][:, 4] == IMIN) and np.any(args["values"][:, 4] == IMAX)
    z = args["values"][:, 3]
    assert np.any(z == 2 ** 60) and np.any(z == 2 ** 60 + 1) and np.any(z < 0)


def test_the_restatement_reproduces_the_oracle_on_the_main_edge_case():
    rows, args, key, segs = _edge_segments(E_MAIN)
    for col, kind, t in EDGE_LAYOUT:
        got = running_extreme(key, args["values"][:, col], kind, t)
        assert np.array_equal(got, rows["values"][:, col]), col


def test_streaming_cases_have_rows_and_segments_spanning_groups():
    for ac in MINMAX_CASES:
        rows = agg_ref(ac)[3]
        assert len(rows["seq"]) > 0
        grp = row_groups(ac, rows)
        later = sum(int(np.sum(grp[ix] > grp[ix[0]])) for ix in segments(ac, rows).values())
        assert later >= 50, (ac[0], later)
