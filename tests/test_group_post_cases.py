"""`group by` behind the aggregate post-pass, on the CPU: the product's group word rule
(siddhi_amd/csrc/sh_group.h) compiled for the CPU (tests/group_host) against the numpy
restatement of tests/group_post_cases.py on planted values, the premises of the shapes
the GPU tests share, and the ctypes mirrors against the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import agg_post_cases as ap
import group_post_cases as gp

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def group_host():
    d = os.path.join(HERE, "group_host")
    subprocess.run(["make", "-s", "-C", d], check=True)
    return os.path.join(d, "group_host")


def test_mirrors_match_the_header(group_host):
    w = subprocess.run([group_host, "--layout"], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(w[0::2], map(int, w[1::2])))
    assert got == dict(sha_group_q=C.sizeof(gp.sha_group_q), sha_groups=C.sizeof(gp.sha_groups),
                       q=gp.sha_groups.q.offset, col=gp.sha_group_q.col.offset, type=gp.sha_group_q.type.offset,
                       max_group=gp.SH_MAX_GROUP, max_queries=gp.SHG_MAX_QUERIES, tile=gp.SHG_TILE)


def _f32(bits):
    return np.array(bits, np.uint32).astype(np.int64)


def _f64(bits):
    return np.array(bits, np.uint64).view(np.int64)


def _rows(cols, m=None):
    m = m or len(cols[0])
    vals = np.arange(m * 4, dtype=np.int64).reshape(m, 4) * 1000003
    for c, a in enumerate(cols):
        vals[:, c] = a
    return vals


def _both(group_host, tmp_path, vals, query, key, groups):
    """(host program's, restatement's) (order, segment ids): equal, and returned"""
    got = gp.run_host(group_host, vals, query, key, groups, str(tmp_path / "job.bin"))
    want = gp.segments_ref(vals, query, key, 1 << 20, groups)
    assert np.array_equal(got[0], want[0]), "order"
    assert np.array_equal(got[1], want[1]), "segment ids"
    return want


def _labels(order, sseg):
    g = np.empty(len(order), np.int64)
    g[order.astype(np.int64)] = sseg
    return g


def test_nans_of_any_payload_are_one_group(group_host, tmp_path):
    f = _f32([0x7FC00000, 0x7F800001, 0xFFC00000, 0x7FFFFFFF, 0x7F800000, 0xFF800000, 0x3F800000])
    d = _f64([0x7FF8000000000000, 0x7FF0000000000001, 0xFFF8000000000000, 0x7FFFFFFFFFFFFFFF, 0x7FF0000000000000,
              0xFFF0000000000000, 0x3FF0000000000000])
    for col, t in ((f, gp.FLOAT), (d, gp.DOUBLE)):
        g = _labels(*_both(group_host, tmp_path, _rows([col]), None, None, [[(0, t)]]))
        assert len(set(g[:4])) == 1                      # four NaNs
        assert len(set(g)) == 4                          # ... +inf, -inf, 1.0


def test_negative_zero_is_its_own_group(group_host, tmp_path):
    f = _f32([0x00000000, 0x80000000, 0x00000000])
    d = _f64([0x0000000000000000, 0x8000000000000000, 0x8000000000000000])
    g = _labels(*_both(group_host, tmp_path, _rows([f]), None, None, [[(0, gp.FLOAT)]]))
    assert g[0] == g[2] != g[1]
    g = _labels(*_both(group_host, tmp_path, _rows([d]), None, None, [[(0, gp.DOUBLE)]]))
    assert g[1] == g[2] != g[0]


def test_longs_that_differ_in_one_half_only(group_host, tmp_path):
    hi = np.array([5, 5 + (1 << 32), 5 + (1 << 63) - (1 << 64), 5, 5 + (1 << 32)], np.int64)
    lo = np.array([(7 << 32) + 1, (7 << 32) + 2, (7 << 32) + 1, (7 << 32) + 0xFFFFFFFF, (7 << 32)], np.int64)
    g = _labels(*_both(group_host, tmp_path, _rows([hi]), None, None, [[(0, gp.LONG)]]))
    assert g[0] == g[3] and g[1] == g[4] and len(set(g)) == 3
    g = _labels(*_both(group_host, tmp_path, _rows([lo]), None, None, [[(0, gp.LONG)]]))
    assert g[0] == g[2] and len(set(g)) == 4
    # an int column is its low half: the sign extension of the row word does not matter
    i = np.array([-1, 0xFFFFFFFF, 1, 1 + (1 << 32)], np.int64)
    g = _labels(*_both(group_host, tmp_path, _rows([i]), None, None, [[(0, gp.INT)]]))
    assert g[0] == g[1] and g[2] == g[3] and g[0] != g[2]
    b = np.array([0, 1, 2, -1], np.int64)
    g = _labels(*_both(group_host, tmp_path, _rows([b]), None, None, [[(0, gp.BOOL)]]))
    assert g[1] == g[2] == g[3] != g[0]


def test_two_attributes_two_queries_and_keys(group_host, tmp_path):
    rng = np.random.default_rng(3)
    m = 500
    a = rng.integers(0, 3, m)
    f = _f32([0x00000000, 0x80000000, 0x7FC00000, 0x7F800001])[rng.integers(0, 4, m)]
    vals = _rows([a, f], m)
    key = rng.integers(0, 4, m).astype(np.int32)
    query = rng.integers(0, 2, m).astype(np.int32)
    groups = [[(0, gp.LONG), (1, gp.FLOAT)], [(1, gp.FLOAT), (0, gp.LONG)]]
    order, sseg = _both(group_host, tmp_path, vals, query, key, groups)
    g = _labels(order, sseg)
    # equal values under two queries, or two keys, are different groups
    nan = np.isnan((f & 0xFFFFFFFF).astype(np.uint32).view(np.float32))
    fk = np.where(nan, 0x7FC00000, f)
    full = {}
    for r in range(m):
        full.setdefault((int(query[r]), int(key[r]), int(a[r]), int(fk[r])), set()).add(int(g[r]))
    assert all(len(s) == 1 for s in full.values())
    assert len({next(iter(s)) for s in full.values()}) == len(full) == int(sseg[-1]) + 1
    assert len(full) > 2 * 4 * 3          # more than the (query, key, a) classes: the float splits them
    # stable: inside a segment the rows keep their order; the order is by (query, key, words)
    assert all(np.all(np.diff(order[sseg == s].astype(np.int64)) > 0) for s in range(int(sseg[-1]) + 1))
    assert np.all(np.diff(query[order.astype(np.int64)]) >= 0)
    # a query without attributes keeps (query, key)
    order, sseg = _both(group_host, tmp_path, vals, query, key, [[(0, gp.LONG)], []])
    g = _labels(order, sseg)
    for k in range(4):
        assert len(set(g[(query == 1) & (key == k)])) == 1
        assert len(set(g[(query == 0) & (key == k)])) == 3


@pytest.mark.parametrize("shape", gp.SHAPES)
def test_host_program_on_the_shared_shapes(group_host, tmp_path, shape):
    for m in (0, 1, 65, 2049):
        c = gp.shape_case(shape, m)
        _both(group_host, tmp_path, c.vals, c.query, c.key, c.groups)


def test_premises_of_the_shared_shapes():
    m = 3 * 2048 + 17
    assert m in gp.SIZES and (gp.BIG_M + gp.SHG_TILE - 1) // gp.SHG_TILE == gp.SCAN_TILE + 1
    seg = {s: gp.segments_ref(*(lambda c: (c.vals, c.query, c.key, c.n_keys, c.groups))(gp.shape_case(s, m)))[1]
           for s in gp.SHAPES}
    assert int(seg["one_group"][-1]) == 0
    assert int(seg["own_group"][-1]) == m - 1
    c = gp.shape_case("interleave", m)
    assert int(seg["interleave"][-1]) + 1 == 15                    # 5 keys x 3 groups, each under every key
    by_key = len(np.unique(c.key))
    by_group = len(np.unique(c.vals[:, 0]))
    assert by_key == 5 and by_group == 3
    for s, col in (("high_half", 0), ("low_half", 0)):
        v = gp.shape_case(s, m).vals[:, col]
        half = (v >> 32) if s == "low_half" else (v & 0xFFFFFFFF)
        assert len(np.unique(half)) == 1 and len(np.unique(v)) == 4
        assert int(seg[s][-1]) + 1 == 20
    c = gp.shape_case("four_and_eight", m)
    assert [t for _, t in c.groups[0]] == [gp.FLOAT, gp.LONG]
    assert int(seg["four_and_eight"][-1]) + 1 == 5 * 4 * 2         # floats: 0.0, -0.0, 1.5, NaN
    c = gp.shape_case("two_queries", m)
    assert int(seg["two_queries"][-1]) + 1 == 5 * 3 + 5
    assert int(seg["one_query_ungrouped"][-1]) + 1 == 5


def test_planted_classes():
    """what the GPU test expects of the planted streams, from exact integers"""
    joined, split = gp.planted(False), gp.planted(True)
    assert gp.classify(joined) == "refuse" and gp.classify(split) == "accept"
    # the same rows without the groups would refuse either way
    for c in (joined, split):
        flat = gp.GCase(c.name + "_flat", c.vals, c.desc, None, 1, c.key, 1, [[]])
        assert gp.classify(flat) == "refuse"
    for shape in gp.SHAPES:
        assert not ap.fp_columns(gp.shape_case(shape, 65))          # sum(long), count(), max(float): always 0


# ---- the apps of tests/test_gpu_group_fast.py: the oracle alone
@pytest.mark.parametrize("name", ["C2_GROUP", "C2_UNGROUPED", "C2_GROUP_HAVING", "C2_GROUP_EVERY3", "C2_GROUP_FLOAT",
                                  "C2_NO_AGGREGATOR"])
def test_oracle_row_counts(name):
    text = getattr(gp, name)
    assert len(gp.bulk_oracle(text)[0]) == gp.C2_ROWS[text]


def test_the_stream_makes_key_and_group_both_matter():
    """more than one group under a key, and groups that span several keys: a pass that
    ignores the key, or ignores the group, gives other rows; `having` keeps some rows and
    drops some, and so does the limiter"""
    ts, k, p, v = gp.bulk_stream()
    seq, _, vals, _ = gp.bulk_oracle(gp.C2_GROUP)
    key = k[seq.astype(np.int64)].astype(np.int64)
    pairs = np.unique(np.stack([key, vals[:, 1]], axis=1), axis=0)
    assert (len(pairs), len(np.unique(key)), int(np.bincount(pairs[:, 0]).max())) == gp.C2_GROUPS
    values, keys_of = np.unique(pairs[:, 1], return_counts=True)
    assert int((keys_of > 1).sum()) > len(values) // 2
    flat = gp.bulk_oracle(gp.C2_UNGROUPED)[2]
    assert np.array_equal(flat[:, :2], vals[:, :2])
    differ = (flat[:, 2:] != vals[:, 2:]).any(axis=1)
    assert int(differ.sum()) > len(vals) // 2
    # ... and grouping by the value alone (no key) differs from the oracle's count() as well
    order = np.argsort(vals[:, 1], kind="stable")
    by_value = np.empty(len(vals), np.int64)
    sv = vals[order, 1]
    head = np.r_[True, sv[1:] != sv[:-1]]
    pos = np.arange(len(sv))
    by_value[order] = pos - np.maximum.accumulate(np.where(head, pos, 0)) + 1
    assert int((by_value != vals[:, 3]).sum()) > len(vals) // 2
    assert 0 < gp.C2_ROWS[gp.C2_GROUP_HAVING] < gp.C2_ROWS[gp.C2_GROUP]
    assert 0 < gp.C2_ROWS[gp.C2_GROUP_EVERY3] < gp.C2_ROWS[gp.C2_GROUP]
    assert int((vals[:, 3] > gp.HAVING_N).sum()) == gp.C2_ROWS[gp.C2_GROUP_HAVING]


@pytest.mark.parametrize("ci", gp.RULE_CASES + ("sparse",))
def test_oracle_rule_sets(ci):
    from rules_cases import case_data, oracle_run
    case = gp.rule_case(ci)
    n, cards, nr, rate, batch, merchants, partitioned, free, seed = case
    assert 2 <= nr <= 16
    plain, rules, (ts, card, amount, merchant) = case_data(case)
    if ci == "sparse":
        # what the sparse-partial path asks: the (event, rule) pairs the start filters open
        # stay below 64 per card and 65,536 in all
        opened = sum(int(((amount > np.float32(a)) & (merchant == m)).sum()) for a, m, f, w in rules)
        assert opened == gp.RULE_SPARSE_PARTIALS < min(64 * cards, 65536) and not free
    ref = oracle_run(gp.rule_text(plain), cards, ts, card, amount, merchant, batch, partitioned)
    flat = oracle_run(gp.rule_text(plain, clause=""), cards, ts, card, amount, merchant, batch, partitioned)
    assert len(ref["seq"]) == len(flat["seq"]) == (gp.RULE_SPARSE_ROWS if ci == "sparse" else gp.RULE_ROWS[ci])
    assert int((ref["values"] != flat["values"]).any(axis=1).sum()) > len(ref["seq"]) // 3


# ---- what compiles (needs no device)
@pytest.fixture(scope="module")
def lib():
    from siddhi_amd import abi, build
    return abi.bind_product(C.CDLL(build.build()))


def _compile(lib, ca):
    """(return code, 1 when bulk runs take the grouped post-pass, fingerprint)"""
    from siddhi_amd import abi
    d = ca.descriptor()
    h = C.c_void_p()
    rc = lib.sh_compile(C.byref(d), C.byref(h))
    g = lib.shx_group_compiled(h)
    fp = lib.shx_fingerprint(h) if rc == abi.SH_OK else 0
    lib.sh_destroy(h)
    return rc, g, fp


TAKEN = ["C2_GROUP", "C2_GROUP_HAVING", "C2_GROUP_EVERY3", "C2_GROUP_FLOAT", "C2_TWO_ATTRS"]
GENERAL = ["C2_NOT_SELECTED",    # group by e2.volume, which the select does not output
           "C2_OTHER_EVENT",     # group by e1.volume: the select outputs e2's
           "C2_ARITHMETIC",      # the select outputs e2.volume + 1
           "C2_ORDERED",         # order by beside it
           "C2_NO_AGGREGATOR",   # the clause has no effect: no group layout, the fast engines as without it
           "C2_UNGROUPED"]


def test_scope_rule(lib, monkeypatch):
    from siddhi_amd import abi, compiler
    apps = {n: compiler.compile_app(getattr(gp, n)) for n in TAKEN + GENERAL}
    now = {n: _compile(lib, ca) for n, ca in apps.items()}
    for n in TAKEN:
        assert now[n][:2] == (abi.SH_OK, 1), n
    for n in GENERAL:
        assert now[n][:2] == (abi.SH_OK, 0), n
    # the switch: every app as the parent compiled it; streaming images do not change
    monkeypatch.setenv("SH_NO_GROUP_POST", "1")
    for n, ca in apps.items():
        rc, g, fp = _compile(lib, ca)
        assert (rc, g) == (abi.SH_OK, 0), n
        assert fp == now[n][2] != 0, n


def test_scope_rule_on_rule_sets(lib):
    from rules_cases import CASES, card_strings, case_data
    from siddhi_amd import abi, compiler
    case = CASES[3]
    plain, rules, data = case_data(case)
    strings = card_strings(case[1])
    assert _compile(lib, compiler.compile_app(gp.rule_text(plain), strings))[:2] == (abi.SH_OK, 1)
    # one rule groups by another select position than the others: the general engine
    text = gp.rule_text(plain, select="e2.merchant as merchant, e1.merchant as m1, sum(e2.merchant) as tm")
    mixed = text.replace("group by e2.merchant", "group by e1.merchant", 1)
    assert mixed != text
    assert _compile(lib, compiler.compile_app(text, strings))[:2] == (abi.SH_OK, 1)
    assert _compile(lib, compiler.compile_app(mixed, strings))[:2] == (abi.SH_OK, 0)
    # one rule does not group at all
    some = gp.rule_text(plain).replace(" group by e2.merchant", "", 1)
    assert _compile(lib, compiler.compile_app(some, strings))[:2] == (abi.SH_OK, 0)
    # more than 16 rules: refused, as before
    big = CASES[4]
    assert big[2] > 16
    plain, rules, data = case_data(big)
    assert _compile(lib, compiler.compile_app(gp.rule_text(plain), card_strings(big[1])))[0] == abi.SH_E_UNSUPPORTED


def _handle_facts(lib, ca):
    """(return code, fingerprint, 1 when a rise-and-fall rung is staged for bulk runs)"""
    from siddhi_amd import abi
    d = ca.descriptor()
    h = C.c_void_p()
    rc = lib.sh_compile(C.byref(d), C.byref(h))
    out = (rc, lib.shx_fingerprint(h) if rc == abi.SH_OK else 0, lib.shx_seq3_shape(h) if rc == abi.SH_OK else 0)
    lib.sh_destroy(h)
    return out


def test_a_grouped_select_without_an_aggregator_streams_as_before(lib, monkeypatch):
    """the clause is a no-op only for bulk runs: the handle streams on the general engine
    with the fingerprint the switch (the earlier behaviour) gives, not the chain engine's
    of the clause-free app; sets of more than 16 queries stay refused and the
    rise-and-fall rungs are not staged for it"""
    from rules_cases import CASES, card_strings, case_data
    from siddhi_amd import abi, compiler, synth
    grouped = compiler.compile_app(gp.C2_NO_AGGREGATOR)
    plain = compiler.compile_app(gp.C2_NO_AGGREGATOR.replace(" " + gp.GROUP, ""))
    big = CASES[4]
    assert big[2] > 16
    text, rules, data = case_data(big)
    ins = " insert into Alerts;"
    big_grouped = compiler.compile_app(text.replace(ins, " group by e2.amount" + ins), card_strings(big[1]))
    c3 = synth.C3_QUERY.replace(" insert into Out;", " having p1 > 25.0 insert into Out;")
    c3_grouped = compiler.compile_app(c3.replace(" having", " group by e1.price having"))
    now = [_handle_facts(lib, ca) for ca in (grouped, plain, big_grouped, c3_grouped, compiler.compile_app(c3))]
    assert now[0][0] == now[1][0] == abi.SH_OK and now[0][1] != now[1][1]
    assert now[2][0] == abi.SH_E_UNSUPPORTED
    assert now[3][0] == now[4][0] == abi.SH_OK and (now[3][2], now[4][2]) == (0, 1)
    monkeypatch.setenv("SH_NO_GROUP_POST", "1")
    assert [_handle_facts(lib, ca) for ca in (grouped, big_grouped, c3_grouped)] == [now[0], now[2], now[3]]
