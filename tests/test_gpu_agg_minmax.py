"""max(x) / min(x) in the select on the fast engines, exact against the CPU oracle
in every value column: streamed rule sets of more than 16 queries (the carried
sequential pass, agg_status 6), the parallel post-pass (sh_agg.hip k_shm_tile /
k_shm_carry / k_shm_out, agg_status 1) behind the window engine with planted NaN, signed zeros, infinities and extreme integers, behind bulk rule sets on
both paths and behind the rise-and-fall engine, and a select that mixes max with a
sum whose additions round (the sequential engine, agg_status 2)."""
import numpy as np
import pytest

from agg_minmax_cases import (C3_MINMAX, E_BIG, E_MAIN, E_ONE, EDGE_ARGS, EDGE_LAYOUT, EDGE_TEXT, M1, MINMAX_CASES,
                              MIXED_TEXT, SEL_HI_LO, SEL_LO_LO, SHA_CARRY_TPB, SHA_TILE, edge_data, edge_oracle,
                              running_extreme)
from oracle_engine import OracleEngine
from rules_cases import CASES, card_strings, case_data, oracle_run
from rules_stream_agg_cases import PLAIN, agg_ref, assert_agg_rows_equal
from rules_stream_cases import compiled, run_calls
from siddhi_amd import InMemoryPersistenceStore, SiddhiManager, abi, compiler

pytestmark = pytest.mark.gpu

BY_NAME = {ac[0]: ac for ac in MINMAX_CASES}
POST_PASS, SEQUENTIAL_ENGINE, CARRIED_SEQUENTIAL = 1, 2, 6  # shx_agg_status


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ streamed rule sets
def hip_engine(case, text):
    from siddhi_amd._native import HipEngine
    eng = HipEngine(compiled(case, text))
    eng.start()
    return eng


def agg_status(eng):
    from siddhi_amd._native import lib
    return lib().shx_agg_status(eng.h)


@pytest.mark.parametrize("name", list(BY_NAME))
def test_streamed_max_min_sets_vs_oracle(name):
    ac = BY_NAME[name]
    base = ac[1]
    text, data, calls, ref = agg_ref(ac)
    eng = hip_engine(base, text)
    got = run_calls(eng, calls, base[5])
    status = agg_status(eng)
    eng.close()
    assert len(ref["seq"]) > 0
    assert_agg_rows_equal(got, ref)
    assert status == CARRIED_SEQUENTIAL


def test_snapshot_restore_continues_and_max_image_is_refused_by_min():
    from siddhi_amd._native import HipError
    base = M1[1]
    text, data, calls, ref = agg_ref(M1)
    every = base[5]
    eng = hip_engine(base, text)
    head = run_calls(eng, calls[:40], every)
    image = eng.snapshot()
    eng.close()
    # the same set with min where max stood: another aggregate layout
    other = hip_engine(base, text.replace(SEL_HI_LO, SEL_LO_LO))
    with pytest.raises(HipError) as ei:
        other.restore(image)
    assert ei.value.code == abi.SH_E_INVALID_ARG
    other.close()
    eng2 = hip_engine(base, text)
    eng2.restore(image)
    assert eng2.snapshot() == image
    tail = run_calls(eng2, calls[40:], every)
    assert agg_status(eng2) == CARRIED_SEQUENTIAL
    eng2.close()
    assert_agg_rows_equal(abi.concat_drains([head, tail]), ref)


def _public_api_run(factory, text, data, call, persist_at=None):
    from siddhi_amd import Event
    ts, card, amount, merchant = data
    store = InMemoryPersistenceStore()
    mgr = SiddhiManager(engine_factory=factory)
    mgr.setPersistenceStore(store)
    got = []

    def open_rt():
        rt = mgr.createSiddhiAppRuntime(text)
        rt.addCallback("Alerts", lambda evs: got.extend((e.timestamp, tuple(e.data)) for e in evs))
        rt.start()
        return rt, rt.getInputHandler("Txn")

    rt, ih = open_rt()
    for ci, b0 in enumerate(range(0, len(ts), call)):
        if persist_at is not None and ci == persist_at:
            rt.persist()
            rt.shutdown()
            rt, ih = open_rt()
            assert rt.restoreLastRevision() is not None
        b1 = min(len(ts), b0 + call)
        ih.send([Event(int(ts[i]), [f"C{int(card[i])}", float(amount[i]), int(merchant[i])])
                 for i in range(b0, b1)])
    rt.shutdown()
    return got


def test_public_api_streams_a_max_min_rule_set():
    """SiddhiManager / InputHandler.send(Event[]) in calls of 37 with persist() and
    restoreLastRevision() in the middle, against the same calls on the oracle"""
    from siddhi_amd._native import HipEngine
    text, data, calls, ref = agg_ref(M1)
    want = _public_api_run(OracleEngine, text, data, 37)
    got = _public_api_run(HipEngine, text, data, 37, persist_at=80)
    assert len(want) == len(ref["seq"]) > 0
    assert got == want


# ------------------------------------------------------------------ the post-pass, edge values
def _run(text, ts, k, cols, nkeys, layout="raw", with_query=False, batch=4096, cards=None):
    import torch
    from siddhi_amd.device_run import DeviceRunner, columns_to_raw, packed_to_raw
    r = DeviceRunner(compiler.compile_app(text) if cards is None else compiler.compile_app(text, card_strings(cards)))
    dev = torch.device("cuda:0")
    tk = torch.from_numpy(k).to(dev)
    res = r.run(torch.from_numpy(ts).to(dev), tk, [torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in cols],
                nkeys, with_query=with_query, packed=layout == "packed", columns=layout == "columns",
                batch_events=batch)
    torch.cuda.synchronize()
    if layout == "packed":
        offs, rb = r.packed_layout()
        oseq, ovals = packed_to_raw(res[1].cpu().numpy(), r.out_types, offs, rb)
        out = [res[0], oseq.view(np.int64), ovals] + [x.cpu().numpy() for x in res[2:]]
    elif layout == "columns":
        typed_cols = [c.cpu().numpy() for c in res[2]]
        # a max / min column has its argument's natural width
        assert [c.dtype.itemsize for c in typed_cols] == [
            {compiler.LONG: 8, compiler.DOUBLE: 8}.get(t, 4) for t in r.out_types]
        out = [res[0], res[1].cpu().numpy(), columns_to_raw(typed_cols, r.out_types)] + [x.cpu().numpy() for x in res[3:]]
    else:
        out = [res[0]] + [x.cpu().numpy() for x in res[1:]]
    st = dict(agg=r.agg_status(), bucket=r.bucket_status(), seq3=r.seq3_status(), rules=r.rules_status(),
              err=r.last_error())
    r.close()
    return out, st


@pytest.mark.parametrize("layout", ["raw", "columns", "packed"])
@pytest.mark.parametrize("case", [E_ONE, E_MAIN], ids=lambda c: c[0])
def test_post_pass_edge_values_vs_oracle(case, layout):
    """E_ONE: one matching row in the whole run. E_MAIN (asserted from the oracle in
    tests/test_agg_minmax_cases.py): a segment over 4 tiles of 2,048 rows, a tile
    holding over 300 segment heads, thousands of segments inside one tile; hundreds of
    segments whose first argument is NaN, with a NaN after a number, with both zeros
    in each order; int extremes; longs that differ only in their lowest bits"""
    ts, k, *cols = edge_data(case)
    ref = edge_oracle(case, EDGE_TEXT)
    (m, seq, vals), st = _run(EDGE_TEXT, ts, k, [k] + cols, case[2], layout=layout)
    assert st["agg"] == POST_PASS, st
    assert st["bucket"] == 0, st  # a max / min select is not offered to the bucketed engine
    assert m == len(ref["seq"]) > 0
    assert np.array_equal(seq, ref["seq"].astype(np.int64))
    for c in range(ref["values"].shape[1]):
        assert np.array_equal(vals[:, c], ref["values"][:, c]), c


def test_post_pass_second_carry_iteration_vs_restatement():
    """more rows than one iteration of the carry kernel covers (1,024 tiles of 2,048):
    its threads each walk two tiles. Too large for the oracle: the same matches'
    arguments (the projection-only select, on the device) under the vectorised
    restatement of the rule per key (checked against the oracle and against the
    one-at-a-time rule in tests/test_agg_minmax_cases.py)"""
    ts, k, *cols = edge_data(E_BIG)
    (m, seq, vals), st = _run(EDGE_TEXT, ts, k, [k] + cols, E_BIG[2])
    assert st["agg"] == POST_PASS, st
    assert m > SHA_TILE * SHA_CARRY_TPB, m
    (ma, aseq, avals), sta = _run(EDGE_ARGS, ts, k, [k] + cols, E_BIG[2])
    assert ma == m and np.array_equal(aseq, seq)
    assert np.array_equal(vals[:, 0], avals[:, 0])
    group = k[seq]
    for col, kind, t in EDGE_LAYOUT:
        assert np.array_equal(vals[:, col], running_extreme(group, avals[:, col], kind, t)), col


# ------------------------------------------------------------------ bulk rule sets
RULES_SELECT = "max(e2.amount) as hi, min(e2.merchant) as lo, count() as n"


@pytest.mark.parametrize("engine", ["sparse", "segment"])
@pytest.mark.parametrize("ci", [1, 0], ids=["12-rules", "40-rules"])
def test_bulk_rule_sets_max_min_count(ci, engine, monkeypatch):
    """sh_run_device on a rule set of up to 16 queries and of more than 16, on the
    sparse-partial path and on the key-segment path (SH_RULES_SPARSE=0)"""
    if engine == "segment":
        monkeypatch.setenv("SH_RULES_SPARSE", "0")
    case = CASES[ci]
    n, cards, nr, rate, batch, merchants, partitioned, free, seed = case
    text, rules, (ts, card, amount, merchant) = case_data(case)
    assert text.count(PLAIN) == nr
    text = text.replace(PLAIN, RULES_SELECT)
    ref = oracle_run(text, cards, ts, card, amount, merchant, batch, partitioned)
    (m, seq, vals, q), st = _run(text, ts, card, [card, amount, merchant], cards, with_query=True, batch=batch,
                                 cards=cards)
    assert st["agg"] == POST_PASS, st
    if engine == "segment":
        assert st["rules"] == 0, st
    assert m == len(ref["seq"]) > 0
    assert np.array_equal(seq, ref["seq"].astype(np.int64))
    assert np.array_equal(q, ref["query"])
    assert np.array_equal(vals[:, :4], ref["values"][:, :4])


# ------------------------------------------------------------------ rise-and-fall
def test_rise_and_fall_max_min_vs_oracle():
    """the C3 shape at 3,000 keys: k_seq3s writes the arguments, the post-pass forms
    max(e3.price) and min(e2[last].price) (agg_status 1; its lanes keep sum / avg / count only)"""
    from siddhi_amd import synth
    ts, k, p, v = synth.stock_stream(100_000, 3_000, 1000, config_index=3)
    (m, seq, vals), st = _run(C3_MINMAX, ts, k, [k, p, v], 3_000)
    eng = OracleEngine(compiler.compile_app(C3_MINMAX))
    eng.start()
    for b0 in range(0, len(ts), 4096):
        b1 = min(len(ts), b0 + 4096)
        eng.send(0, ts[b0:b1], [np.ascontiguousarray(c[b0:b1]) for c in (k, p, v)], [None] * 3,
                 np.ascontiguousarray(k[b0:b1]), b0)
    ref = eng.drain()
    eng.close()
    assert st["seq3"] == 1 and st["agg"] == POST_PASS, st
    assert m == len(ref["seq"]) > 0
    assert np.array_equal(seq, ref["seq"].astype(np.int64))
    assert np.array_equal(vals, ref["values"])


# ------------------------------------------------------------------ mixed with a sum that rounds
def test_sum_whose_proof_fails_takes_max_along_to_the_sequential_engine():
    """sum(e2.y), max(e2.y) over two-decimal doubles (12.34: not dyadic, the running
    sums round): the post-pass answers "not exact" for the sum, the whole select
    reruns on the sequential engine, and both columns are the oracle's"""
    from siddhi_amd import synth
    ts, k, p, v = synth.stock_stream(60_000, 256, 100)
    y = np.round(p.astype(np.float64) + 0.003, 2)
    (m, seq, vals), st = _run(MIXED_TEXT, ts, k, [k, p, y], 256)
    eng = OracleEngine(compiler.compile_app(MIXED_TEXT))
    eng.start()
    for b0 in range(0, len(ts), 4096):
        b1 = min(len(ts), b0 + 4096)
        eng.send(0, ts[b0:b1], [np.ascontiguousarray(c[b0:b1]) for c in (k, p, y)], [None] * 3,
                 np.ascontiguousarray(k[b0:b1]), b0)
    ref = eng.drain()
    eng.close()
    assert st["agg"] == SEQUENTIAL_ENGINE, st
    assert m == len(ref["seq"]) > 0
    assert np.array_equal(seq, ref["seq"].astype(np.int64))
    assert np.array_equal(vals, ref["values"])
