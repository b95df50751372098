"""`output all every N events` behind the fast engines, on the CPU: the product's
placement rule (siddhi_amd/csrc/sh_rate.h shl_place) compiled for the CPU
(tests/rate_all_host) against the oracle's rows, the pinned row counts of the cases the
GPU tests share, and what libsiddhi_hip.so lowers and refuses (compiling needs no
device)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle_engine import run_columns_oracle
from rate_all_cases import (BIG, SET_ROWS, SETS, SH_RATE_ALL_EVENTS, SH_RATE_FIRST_EVENTS, SH_RATE_LAST_EVENTS, c2,
                            mix_all, run_place, set_ref)
from rate_fast_cases import R_F3, rate_texts, with_rate
from rules_cases import CASES, card_strings
from rules_stream_cases import S2, compiled
from siddhi_amd import abi, build, compiler, synth

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def place_host():
    d = os.path.join(HERE, "rate_all_host")
    subprocess.run(["make", "-s", "-C", d], check=True)
    return os.path.join(d, "rate_all_host")


# ---- one window-shaped query: C2 on a small stream
N_SMALL, NK_SMALL = 20_000, 200
HAVING = "having p2 - p1 > 0.19 and v2 != 3"
# clause -> (N, text whose rows reach the limiter, the oracle's rows reaching / leaving it)
C2_SMALL = {
    "output all every 1 events": (1, synth.C2_QUERY, (14_003, 14_003)),
    "output all every 2 events": (2, synth.C2_QUERY, (14_003, 13_906)),
    "output all every 3 events": (3, synth.C2_QUERY, (14_003, 13_833)),
    "output every 4 events": (4, synth.C2_QUERY, (14_003, 13_744)),
    "output all every 100000 events": (100_000, synth.C2_QUERY, (14_003, 0)),  # beyond every key's rows
    HAVING + " output all every 2 events": (2, c2(HAVING), (6_855, 6_770)),
}

_small = {}


def small_rows(text):
    if "s" not in _small:
        _small["s"] = synth.stock_stream(N_SMALL, NK_SMALL, 100)
    if text not in _small:
        ts, k, p, v = _small["s"]
        seq, ots, vals, nulls = run_columns_oracle(compiler.compile_app(text), ts, [k, p, v], k)
        _small[text] = dict(seq=seq, ts=ots, values=vals, nulls=nulls)
    return _small[text]


def not_ascending(seq):
    return bool(np.any(np.diff(np.asarray(seq).astype(np.int64)) < 0))


def assert_placed(rows0, order, rows1, fields):
    assert len(order) == len(rows1["seq"]), (len(order), len(rows1["seq"]))
    for f in fields:
        assert np.array_equal(np.asarray(rows0[f])[order], rows1[f]), f


@pytest.mark.parametrize("clause", list(C2_SMALL))
def test_cpu_placement_reproduces_the_oracle_one_query(place_host, tmp_path, clause):
    """the oracle's rows without the clause, placed by the stand-alone program by their
    key and order, are the oracle's rows with it: full rows, in order"""
    n, before, counts = C2_SMALL[clause]
    rows0, rows1 = small_rows(before), small_rows(c2(clause))
    assert (len(rows0["seq"]), len(rows1["seq"])) == counts
    key = _small["s"][1][rows0["seq"].astype(np.int64)].astype(np.int32)
    assert np.bincount(key).max() < 100_000
    order = run_place(place_host, [(SH_RATE_ALL_EVENTS, n)], np.zeros(len(key), np.int32), key,
                      str(tmp_path / "job.bin"))
    assert_placed(rows0, order, rows1, ("seq", "ts", "values", "nulls"))
    if n == 1:  # the identity
        assert np.array_equal(order, np.arange(len(key)))
    elif counts[1]:
        assert 0 < counts[1] < counts[0]
        assert not_ascending(rows1["seq"])  # rows moved back to their chunk's N-th


@pytest.mark.parametrize("ci,select", SETS)
def test_cpu_placement_reproduces_the_oracle_mixed_set(place_host, tmp_path, ci, select):
    """a set of at most 16 rules that mixes `all`, `first`, `last` and no limiter"""
    text, rules, data, rows0, rows1, key = set_ref(ci, select)
    assert {k for k, n in rules} == {0, SH_RATE_FIRST_EVENTS, SH_RATE_LAST_EVENTS, SH_RATE_ALL_EVENTS}
    assert (len(rows0["seq"]), len(rows1["seq"])) == SET_ROWS[(ci, select)]
    assert 0 < len(rows1["seq"]) < len(rows0["seq"])
    assert not_ascending(rows1["seq"])
    order = run_place(place_host, rules, rows0["query"], key, str(tmp_path / "job.bin"))
    assert_placed(rows0, order, rows1, ("seq", "query", "ts", "nulls", "values"))


def test_cpu_placement_edges(place_host, tmp_path):
    """N = 1, N = 2^31 - 1, runs of N - 1, N and N + 1 rows, and the other kinds beside
    `all` on one key: rows 0..6 of each query interleaved"""
    rules = [(3, 1), (3, BIG), (3, 3), (1, 2), (2, 3), (0, 0), (3, 7), (3, 6), (3, 8)]
    m = 7
    query = np.tile(np.arange(len(rules), dtype=np.int32), m)  # row r: query r % 9, its ordinal r // 9 + 1
    order = run_place(place_host, rules, query, np.zeros(len(query), np.int32), str(tmp_path / "job.bin"))
    nq = len(rules)
    want = []
    for j in range(1, m + 1):  # the rows of ordinal j, in query order
        want.append((j - 1) * nq + 0)                                  # all every 1
        if j % 3 == 0:
            want += [(i - 1) * nq + 2 for i in range(j - 2, j + 1)]    # all every 3: the chunk with its 3rd
        if j % 2 == 1:
            want.append((j - 1) * nq + 3)                              # first every 2
        if j % 3 == 0:
            want.append((j - 1) * nq + 4)                              # last every 3
        want.append((j - 1) * nq + 5)                                  # no limiter
        if j == 7:
            want += [i * nq + 6 for i in range(7)]                     # all every 7: a run of exactly N
        if j == 6:
            want += [i * nq + 7 for i in range(6)]                     # all every 6: N + 1 rows, the last held
    assert order.tolist() == want                                      # (all every 8: N - 1 rows, none leaves)


# ---- compile through libsiddhi_hip.so
@pytest.fixture(scope="module")
def lib():
    return abi.bind_product(C.CDLL(build.build()))


def _compile(lib, ca):
    d = ca.descriptor()
    h = C.c_void_p()
    rc = lib.sh_compile(C.byref(d), C.byref(h))
    err = (lib.sh_last_error(h) or b"").decode()
    fp = lib.shx_fingerprint(h) if rc == abi.SH_OK else 0
    lib.sh_destroy(h)
    return rc, err, fp


def test_one_query_and_small_sets_compile_and_stream_as_before(lib, monkeypatch):
    """they stream on the general engine: the image's fingerprint is what the switch
    SH_NO_RATE_FILTER=1 (the parent's behaviour) gives"""
    text, rules, data, rows0, rows1, key = set_ref(1, SETS[0][1])
    apps = [compiler.compile_app(c2("output all every 3 events")),
            compiler.compile_app(text, card_strings(CASES[1][1]))]
    now = [_compile(lib, ca) for ca in apps]
    monkeypatch.setenv("SH_NO_RATE_FILTER", "1")
    parent = [_compile(lib, ca) for ca in apps]
    for (rc, err, fp), (prc, perr, pfp) in zip(now, parent):
        assert rc == prc == abi.SH_OK, (err, perr)
        assert fp == pfp != 0


def test_a_set_beyond_the_table_is_refused_for_its_held_rows(lib, monkeypatch):
    before, text, data = rate_texts(R_F3)
    assert S2[2] == 17
    held = with_rate(before, mix_all)
    rc, err, fp = _compile(lib, compiled(S2, held))
    assert rc == abi.SH_E_UNSUPPORTED and "held rows" in err
    # without an `all` rule the same set lowers
    rc, err, fp = _compile(lib, compiled(S2, held.replace("output all", "output last")))
    assert rc == abi.SH_OK, err
    # the switch: the limiters are the general engine's again, for every kind
    monkeypatch.setenv("SH_NO_RATE_FILTER", "1")
    rc, err, fp = _compile(lib, compiled(S2, held))
    assert rc == abi.SH_E_UNSUPPORTED and "held rows" not in err and "run on the general engine" in err


def test_the_clause_beside_order_by_is_still_unsupported(lib):
    before, text, data = rate_texts(R_F3)
    ordered = with_rate(before, lambda r: ("all", 2)).replace(" output all", " order by amount output all")
    assert ordered.count("order by") == S2[2]
    rc, err, fp = _compile(lib, compiled(S2, ordered))
    assert rc == abi.SH_E_UNSUPPORTED
    assert "rule engine: order by" in err and "held rows" not in err
    one = c2("order by p2 output all every 3 events")
    rc, err, fp = _compile(lib, compiler.compile_app(one))
    assert rc == abi.SH_OK, err  # (one query: the chain engine refuses it too, and the general engine takes it)
