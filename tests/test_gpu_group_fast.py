"""`group by` selects behind the fast engines in bulk runs (sh_run_device), exact against
the CPU oracle: the C2-shaped app of tests/group_post_cases.py on the 200,000-event,
2,000-key stream (the bucketed engine writes the aggregators' arguments, the grouped
post-pass of sh_group.hip + sh_agg.hip forms the running values per (key, group)), in
every row layout, with `having` and `output every N events` behind it, with a float sum
that may leave the post-pass for the general engine, under the switch SH_NO_GROUP_POST=1,
and rule sets of 2..16 queries on both rule paths."""
import numpy as np
import pytest

import group_post_cases as gp
from rules_cases import card_strings, case_data, oracle_run
from siddhi_amd import compiler

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _run(text, layout=None):
    """(m, seq, raw rows), statuses"""
    import torch
    from siddhi_amd.device_run import DeviceRunner, columns_to_raw, packed_to_raw
    ts, k, p, v = gp.bulk_stream()
    runner = DeviceRunner(compiler.compile_app(text))
    dev = torch.device("cuda:0")
    tc = [torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in (k, p, v)]
    tts, tk = torch.from_numpy(ts).to(dev), tc[0]
    if layout == "packed":
        offs, rb = runner.packed_layout()
        m, rows = runner.run(tts, tk, tc, gp.NK_BULK, packed=True)
        torch.cuda.synchronize()
        seq, vals = packed_to_raw(rows.cpu().numpy(), runner.out_types, offs, rb)
        seq = seq.astype(np.int64)
    elif layout == "columns":
        m, seq, ocols = runner.run(tts, tk, tc, gp.NK_BULK, columns=True)
        torch.cuda.synchronize()
        seq, vals = seq.cpu().numpy(), columns_to_raw([c.cpu().numpy() for c in ocols], runner.out_types)
    else:
        m, seq, vals = runner.run(tts, tk, tc, gp.NK_BULK)
        torch.cuda.synchronize()
        seq, vals = seq.cpu().numpy(), vals.cpu().numpy()
    st = dict(bucket=runner.bucket_status(), group=runner.group_status(), agg=runner.agg_status(),
              having=runner.having_status(), rate=runner.rate_status(), having_rows=runner.having_rows(),
              rate_rows=runner.rate_rows(), post_ms=runner.agg_post_ms(), err=runner.last_error())
    runner.close()
    return (m, seq, vals), st


def _check(text, layout=None):
    seq, _, vals, _ = gp.bulk_oracle(text)
    assert len(seq) == gp.C2_ROWS[text]
    (m, oseq, ovals), st = _run(text, layout)
    print(text[-70:], layout, st)
    assert m == len(seq) > 0, (m, len(seq), st)
    assert np.array_equal(oseq, seq.astype(np.int64))
    assert np.array_equal(ovals, vals)
    return st


@pytest.mark.parametrize("layout", [None, "columns", "packed"])
def test_c2_grouped_bucketed_vs_oracle(layout):
    st = _check(gp.C2_GROUP, layout)
    assert (st["bucket"], st["group"], st["agg"]) == (1, 1, 1), st
    assert st["post_ms"] > 0.0


def test_c2_grouped_then_having_vs_oracle():
    st = _check(gp.C2_GROUP_HAVING)
    assert (st["bucket"], st["group"], st["agg"], st["having"]) == (1, 1, 1, 1), st
    assert st["having_rows"] == (gp.C2_ROWS[gp.C2_GROUP], gp.C2_ROWS[gp.C2_GROUP_HAVING])


def test_c2_grouped_then_every_3_vs_oracle():
    st = _check(gp.C2_GROUP_EVERY3)
    assert (st["bucket"], st["group"], st["agg"], st["rate"]) == (1, 1, 1, 1), st
    assert st["rate_rows"] == (gp.C2_ROWS[gp.C2_GROUP], gp.C2_ROWS[gp.C2_GROUP_EVERY3])


def test_c2_grouped_float_sum_vs_oracle():
    """sum(e2.price) in doubles: the grouped post-pass when its additions are exact
    (agg_status 1), else the general engine's selector (2, group_status 0); the oracle's
    rows either way"""
    st = _check(gp.C2_GROUP_FLOAT)
    assert st["agg"] in (1, 2), st
    assert st["group"] == (1 if st["agg"] == 1 else 0), st


def test_c2_grouped_not_exact_goes_to_the_general_engine():
    """one key planted with 21, 2^40, 21, 21 + 2^-19 and one volume on both consumers: the
    group's total 2^40 + 21 + 2^-19 needs 60 bits, so the grouped post-pass answers "not
    exact" (agg_status 2) and k_nfa_run, whose selector groups, produces the rows"""
    from fractions import Fraction
    import torch
    from oracle_engine import run_columns_oracle
    from siddhi_amd.device_run import DeviceRunner
    ts, k, p, v = (a.copy() for a in gp.bulk_stream())
    kk = int(np.flatnonzero(np.bincount(k) >= 6)[0])
    at = np.flatnonzero(k == kk)
    p[at] = 1.0
    plant = np.array([21.0, 2.0 ** 40, 21.0, 21.0 + 2.0 ** -19], np.float32)
    assert [float(x) for x in plant] == [21.0, 2.0 ** 40, 21.0, 21.0 + 2.0 ** -19]
    p[at[:4]] = plant
    v[at[:4]] = 7
    assert ts[at[3]] - ts[at[0]] < 1000
    exact = Fraction(2 ** 40) + Fraction(21) + Fraction(1, 2 ** 19)
    assert Fraction(float(exact)) != exact
    ca = compiler.compile_app(gp.C2_GROUP_FLOAT)
    seq, _, vals, _ = run_columns_oracle(ca, ts, [k, p, v], k)
    runner = DeviceRunner(ca)
    dev = torch.device("cuda:0")
    tc = [torch.from_numpy(c).to(dev) for c in (k, p, v)]
    m, oseq, ovals = runner.run(torch.from_numpy(ts).to(dev), tc[0], tc, gp.NK_BULK)
    torch.cuda.synchronize()
    st = dict(bucket=runner.bucket_status(), group=runner.group_status(), agg=runner.agg_status(),
              err=runner.last_error())
    oseq, ovals = oseq.cpu().numpy(), ovals.cpu().numpy()
    runner.close()
    print(st)
    mine = vals[k[seq.astype(np.int64)] == kk]
    assert len(mine) == 2 and mine[1, 2] == np.float64(2.0 ** 40 + 21.0 + 2.0 ** -19).view(np.int64), mine
    assert m == len(seq) > 0
    assert np.array_equal(oseq, seq.astype(np.int64))
    assert np.array_equal(ovals, vals)
    assert (st["agg"], st["group"], st["bucket"]) == (2, 0, 0), st


def test_c2_switch_runs_the_general_engine(monkeypatch):
    monkeypatch.setenv("SH_NO_GROUP_POST", "1")
    st = _check(gp.C2_GROUP)
    assert st["group"] == 0 and st["bucket"] == 0 and st["post_ms"] == 0.0, st


def test_c2_grouped_without_an_aggregator_takes_the_fast_engines():
    """the clause has no effect: the bucketed engine, no post-pass"""
    st = _check(gp.C2_NO_AGGREGATOR)
    assert (st["bucket"], st["group"], st["agg"]) == (1, 0, 0), st


def test_c2_ungrouped_select_is_untouched():
    st = _check(gp.C2_UNGROUPED)
    assert st["group"] == 0 and st["bucket"] == 1, st


# ------------------------------------------------------------------ rule sets of 2..16 queries
@pytest.mark.parametrize("sparse", [True, False])
@pytest.mark.parametrize("ci", gp.RULE_CASES + ("sparse",))
def test_bulk_rule_sets_grouped_vs_oracle(ci, sparse, monkeypatch):
    """the sets of rules_cases (few cards: the key-segment path takes them, allowed or not)
    and one whose start filters open few partials per card: the sparse-partial path takes
    it when allowed (rules_status 1)"""
    import torch
    from siddhi_amd.device_run import DeviceRunner
    case = gp.rule_case(ci)
    n, cards, nr, rate, batch, merchants, partitioned, free, seed = case
    if not sparse:
        monkeypatch.setenv("SH_RULES_SPARSE", "0")
    plain, rules, (ts, card, amount, merchant) = case_data(case)
    text = gp.rule_text(plain)
    assert text.count("group by e2.merchant") == nr
    ref = oracle_run(text, cards, ts, card, amount, merchant, batch, partitioned)
    assert len(ref["seq"]) == (gp.RULE_SPARSE_ROWS if ci == "sparse" else gp.RULE_ROWS[ci])
    runner = DeviceRunner(compiler.compile_app(text, card_strings(cards)))
    dev = torch.device("cuda:0")
    cols = [torch.from_numpy(c).to(dev) for c in (card, amount, merchant)]
    m, seq, vals, q = runner.run(torch.from_numpy(ts).to(dev), cols[0], cols, cards, batch_events=batch,
                                 with_query=True)
    torch.cuda.synchronize()
    st = dict(group=runner.group_status(), agg=runner.agg_status(), rules=runner.rules_status(),
              err=runner.last_error())
    seq, vals, q = seq.cpu().numpy(), vals.cpu().numpy(), q.cpu().numpy()
    runner.close()
    print(ci, sparse, st)
    assert m == len(ref["seq"])
    assert np.array_equal(seq, ref["seq"].astype(np.int64))
    assert np.array_equal(q, ref["query"])
    nv = ref["values"].shape[1]
    assert np.array_equal(vals[:, :nv], ref["values"])
    # sum(int) and count(): long arithmetic, the post-pass never refuses
    assert (st["group"], st["agg"]) == (1, 1), st
    assert st["rules"] == (1 if sparse and ci == "sparse" else 0), st
