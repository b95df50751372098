"""The aggregating streaming rule-set cases (tests/rules_stream_agg_cases.py) on the
CPU: the oracle's row and segment counts, that only a carried and sequential
aggregate pass can pass the GPU parity tests (segments span drain groups; additions
round), that every app is beyond the general engine's table and lowers, and the
product's sequential walk (siddhi_amd/csrc/sh_agg_seq.h) compiled for the CPU
against the oracle, bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rules_stream_agg_cases import (A1, A2, A4, AGG_CASES, EXPECTED, LAYOUT, SH_T_INT, agg_data, agg_ref, args_rows,
                                    as_double, rounded_additions, row_groups, row_keys, segments)
from rules_stream_cases import compiled
from siddhi_amd import abi, build

HERE = os.path.dirname(os.path.abspath(__file__))
BY_NAME = {ac[0]: ac for ac in AGG_CASES}


@pytest.mark.parametrize("name", list(BY_NAME))
def test_rows_and_segments(name):
    ac = BY_NAME[name]
    rows = agg_ref(ac)[3]
    segs = segments(ac, rows)
    got = (len(rows["seq"]), len(segs), max(len(v) for v in segs.values()))
    print(name, got)
    assert got == EXPECTED[name]


@pytest.fixture(scope="module")
def lib():
    return abi.bind_product(C.CDLL(build.build()))


@pytest.mark.parametrize("name", list(BY_NAME))
def test_apps_are_beyond_the_general_engine_and_lower(lib, name):
    ac = BY_NAME[name]
    assert ac[1][2] > 16  # the general engine's query table holds 16
    text, args_text, data = agg_data(ac)
    for t in (text, args_text):
        d = compiled(ac[1], t).descriptor()
        h = C.c_void_p()
        rc = lib.sh_compile(C.byref(d), C.byref(h))
        assert rc == abi.SH_OK, lib.sh_last_error(h)
        lib.sh_destroy(h)


@pytest.mark.parametrize("name,least", [("A4", 50), ("A5", 20)])
def test_scaled_cases_round(name, least):
    """an aggregate pass that is exact only where the parallel sums are cannot pass"""
    ac = BY_NAME[name]
    n = rounded_additions(ac, agg_ref(ac)[3])
    print(name, "rounded additions", n)
    assert n >= least


@pytest.mark.parametrize("name", ["A1", "A3"])
def test_plain_cases_are_exact_and_finite(name):
    ac = BY_NAME[name]
    rows = agg_ref(ac)[3]
    assert rounded_additions(ac, rows) == 0
    assert np.all(np.isfinite(as_double(rows["values"][:, 1])))
    assert np.all(np.isfinite(as_double(rows["values"][:, 2])))


def test_a2_is_long_arithmetic():
    """A2 (count and a sum of ints) has no double column: its values are the long
    running count and the long running sum of e2.merchant per (query, card)"""
    assert all(t == SH_T_INT for c, k, t in LAYOUT[A2[2]])
    rows = agg_ref(A2)[3]
    merchant = agg_ref(A2)[1][3]
    arg = merchant[rows["seq"].astype(np.int64)].astype(np.int64)
    for idx in segments(A2, rows).values():
        assert np.array_equal(rows["values"][idx, 1], np.arange(1, len(idx) + 1))
        assert np.array_equal(rows["values"][idx, 2], np.cumsum(arg[idx]))


def test_a1_segments_span_drain_groups():
    """a matcher that resets its aggregates per step cannot pass"""
    rows = agg_ref(A1)[3]
    grp = row_groups(A1, rows)
    later = 0
    for idx in segments(A1, rows).values():
        later += int(np.sum(grp[idx] > grp[idx[0]]))
    print("rows behind an earlier group's row of their segment", later)
    assert later >= 50


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
    lib.agq_capacity.argtypes = [C.c_void_p]
    lib.agq_capacity.restype = C.c_int64
    lib.agq_destroy.argtypes = [C.c_void_p]
    lib.agq_destroy.restype = None
    return lib


def _walk_case(walk, ac, carry=True, one_step=False):
    """the oracle's rows with the arguments put back, walked drain group by drain
    group with the table carried; returns (values, table entries, capacity)"""
    rows, args = agg_ref(ac)[3], args_rows(ac)
    assert np.array_equal(rows["seq"], args["seq"]) and np.array_equal(rows["query"], args["query"])
    lay = LAYOUT[ac[2]]
    cols = np.array([c for c, k, t in lay], np.int32)
    kinds = np.array([k for c, k, t in lay], np.int32)
    types = np.array([t for c, k, t in lay], np.int32)
    h = walk.agq_create(len(lay), cols.ctypes.data, kinds.ctypes.data, types.ctypes.data)
    assert h
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
    out = (vals, walk.agq_entries(h), walk.agq_capacity(h))
    walk.agq_destroy(h)
    return out


@pytest.mark.parametrize("name", list(BY_NAME))
def test_cpu_walk_reproduces_the_oracle(walk, name):
    ac = BY_NAME[name]
    rows = agg_ref(ac)[3]
    vals, entries, cap = _walk_case(walk, ac)
    for c in range(3):
        assert np.array_equal(vals[:, c], rows["values"][:, c]), c
    assert entries == EXPECTED[name][1] and cap >= 2 * entries


def test_cpu_walk_split_invariance_and_no_carry(walk):
    """A4 walked in one step gives the same values; without the carried table it does not"""
    rows = agg_ref(A4)[3]
    once = _walk_case(walk, A4, one_step=True)[0]
    assert np.array_equal(once[:, :3], rows["values"][:, :3])
    fresh = _walk_case(walk, A4, carry=False)[0]
    assert not np.array_equal(fresh[:, 1], rows["values"][:, 1])
