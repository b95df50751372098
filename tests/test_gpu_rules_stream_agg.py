"""Aggregating rule sets of more than 16 queries streamed through sh_push_batch /
sh_drain / sh_snapshot and run through sh_run_device: the carried, sequential
aggregate pass (sh_agg.hip k_shc_walk / k_shc_put behind rules_step), exact against
the CPU oracle fed the same send() calls -- rows, order, and every value column bit
for bit (running sums whose additions round included)."""
import ctypes as C

import numpy as np
import pytest

from oracle_engine import OracleEngine
from rules_stream_agg_cases import A1, A2, A4, AGG_CASES, EXPECTED, agg_ref, assert_agg_rows_equal
from rules_stream_cases import S2, assert_rows_equal, calls_of, compiled, oracle_rows, run_calls, stream_data
from siddhi_amd import InMemoryPersistenceStore, SiddhiManager, abi

pytestmark = pytest.mark.gpu

BY_NAME = {ac[0]: ac for ac in AGG_CASES}
CARRIED_SEQUENTIAL = 6  # shx_agg_status


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def hip_engine(case, text):
    from siddhi_amd._native import HipEngine
    eng = HipEngine(compiled(case, text))
    eng.start()
    return eng


def carry(eng):
    """(partials, rows) carried after the last step"""
    from siddhi_amd._native import lib
    p, r = C.c_int64(-1), C.c_int64(-1)
    lib().shx_rules_carry(eng.h, C.byref(p), C.byref(r))
    return p.value, r.value


def agg_carry(eng):
    """carried (query, key) aggregate entries"""
    from siddhi_amd._native import lib
    e = C.c_int64(-1)
    lib().shx_rules_agg_carry(eng.h, C.byref(e))
    return e.value


def agg_status(eng):
    from siddhi_amd._native import lib
    return lib().shx_agg_status(eng.h)


_hip = {}


def hip_rows(ac):
    """a case streamed at its drain cadence, once: (rows, entries after every drain, status)"""
    name, base = ac[0], ac[1]
    if name not in _hip:
        text, data, calls, ref = agg_ref(ac)
        eng = hip_engine(base, text)
        seen = []
        got = run_calls(eng, calls, base[5], after_drain=lambda: seen.append(agg_carry(eng)))
        _hip[name] = (got, seen, agg_status(eng))
        eng.close()
    return _hip[name]


@pytest.mark.parametrize("name", list(BY_NAME))
def test_agg_cases_vs_oracle(name):
    ac = BY_NAME[name]
    ref = agg_ref(ac)[3]
    got, seen, status = hip_rows(ac)
    assert len(ref["seq"]) == EXPECTED[name][0]
    assert_agg_rows_equal(got, ref)
    assert seen[-1] == EXPECTED[name][1], (seen[-1], EXPECTED[name][1])
    assert all(b >= a for a, b in zip(seen, seen[1:])), seen[:16]
    assert status == CARRIED_SEQUENTIAL


def test_split_invariance():
    """A4 drained per call, every 7 calls and once at the end: identical rows"""
    text, data, calls, ref = agg_ref(A4)
    outs = []
    for every in (1, 7, len(calls)):
        eng = hip_engine(A4[1], text)
        outs.append(run_calls(eng, calls, every))
        assert agg_carry(eng) == EXPECTED["A4"][1]
        eng.close()
    for o in outs:
        assert_agg_rows_equal(o, ref)


@pytest.mark.parametrize("name,status", [("A1", 1), ("A4", CARRIED_SEQUENTIAL)])
def test_bulk_path(name, status):
    """sh_run_device on a fresh handle, batch_events = 37: the streamed rows; the
    parallel post-pass where every addition is exact (A1), the sequential pass where
    additions round (A4)"""
    import torch
    from siddhi_amd.device_run import DeviceRunner
    ac = BY_NAME[name]
    base = ac[1]
    text, data, calls, ref = agg_ref(ac)
    streamed = hip_rows(ac)[0]
    ts, card, amount, merchant = data
    runner = DeviceRunner(compiled(base, text))
    dev = torch.device("cuda:0")
    cols = [torch.from_numpy(c).to(dev) for c in (card, amount, merchant)]
    m, seq, vals, q = runner.run(torch.from_numpy(ts).to(dev), cols[0], cols, base[1], batch_events=37,
                                 with_query=True)
    torch.cuda.synchronize()
    assert base[4] == 37
    assert m == len(streamed["seq"])
    assert np.array_equal(seq.cpu().numpy(), streamed["seq"].astype(np.int64))
    assert np.array_equal(q.cpu().numpy(), streamed["query"])
    assert np.array_equal(vals.cpu().numpy()[:, :3], streamed["values"][:, :3])
    assert runner.agg_status() == status
    runner.close()


def test_refused_step_leaves_the_aggregates_alone():
    """A2: after 20 calls a call whose first timestamp is below that card's previous
    event fails the drain; the carried partials and aggregates stay, and the
    remaining calls give the uninterrupted run's rows"""
    from siddhi_amd._native import HipError
    text, data, calls, ref = agg_ref(A2)
    ts, card, amount, merchant = data
    eng = hip_engine(A2[1], text)
    head = run_calls(eng, calls[:20], 1)
    before, agg_before = carry(eng), agg_carry(eng)
    assert before[0] > 0 and agg_before > 0
    b0, cts, cols, keys = calls[20]
    cts, cols = cts.copy(), [c.copy() for c in cols]
    prev = np.nonzero(card[:b0] == keys[0])[0]
    assert len(prev) and ts[prev[-1]] > 0
    cts[0] = ts[prev[-1]] - 1
    eng.send(0, cts, cols, [None] * 3, keys, b0)
    with pytest.raises(HipError) as ei:
        eng.drain()
    assert ei.value.code == abi.SH_E_UNSUPPORTED
    assert carry(eng) == before
    assert agg_carry(eng) == agg_before
    tail = run_calls(eng, calls[20:], 1)
    eng.close()
    assert_agg_rows_equal(abi.concat_drains([head, tail]), ref)


@pytest.mark.parametrize("name", ["A2", "A4"])
def test_snapshot_restore_continues_exactly(name):
    ac = BY_NAME[name]
    base = ac[1]
    text, data, calls, ref = agg_ref(ac)
    every = base[5]
    eng = hip_engine(base, text)
    head = run_calls(eng, calls[:40], every)
    entries = agg_carry(eng)
    assert entries > 0
    image = eng.snapshot()
    eng.close()
    eng2 = hip_engine(base, text)
    eng2.restore(image)
    assert agg_carry(eng2) == entries
    # snapshot -> restore -> snapshot: equal bytes
    assert eng2.snapshot() == image
    tail = run_calls(eng2, calls[40:], every)
    assert agg_carry(eng2) == EXPECTED[name][1]
    eng2.close()
    assert_agg_rows_equal(abi.concat_drains([head, tail]), ref)


@pytest.mark.parametrize("name", ["A2", "A4"])
def test_refused_restore_leaves_the_handle_as_it_was(name):
    """a good image with a trailing byte is refused after its aggregate section was
    loaded: the handle then streams the whole case like an untouched one -- rows,
    carried entries after every drain, and the final snapshot"""
    from siddhi_amd._native import HipError
    ac = BY_NAME[name]
    base = ac[1]
    text, data, calls, ref = agg_ref(ac)
    every = base[5]
    eng = hip_engine(base, text)
    run_calls(eng, calls[:40], every)
    image = eng.snapshot()
    assert agg_carry(eng) > 0
    eng.close()

    def whole_run(e):
        seen = []
        rows = run_calls(e, calls, every, after_drain=lambda: seen.append(agg_carry(e)))
        return rows, seen, e.snapshot()

    clean = hip_engine(base, text)
    want_rows, want_seen, want_image = whole_run(clean)
    clean.close()
    eng2 = hip_engine(base, text)
    with pytest.raises(HipError) as ei:
        eng2.restore(image + b"\0")
    assert ei.value.code == abi.SH_E_INVALID_ARG
    assert agg_carry(eng2) == 0
    got_rows, got_seen, got_image = whole_run(eng2)
    eng2.close()
    assert_agg_rows_equal(got_rows, ref)
    assert_agg_rows_equal(got_rows, want_rows)
    assert got_seen == want_seen and got_seen[-1] == EXPECTED[name][1]
    assert got_image == want_image


def test_snapshot_of_another_layout_is_refused():
    """the non-aggregating S2 set's image is refused by the A1 handle and the other
    way round, and both handles stay usable"""
    from siddhi_amd._native import HipError
    text, data, calls, ref = agg_ref(A1)
    ptext, prules, pdata = stream_data(S2)
    pcalls = calls_of(S2, pdata)
    a = hip_engine(S2, text)
    run_calls(a, calls[:6], 3)
    image_a = a.snapshot()
    a.close()
    p = hip_engine(S2, ptext)
    run_calls(p, pcalls[:6], 3)
    image_p = p.snapshot()
    p.close()
    fresh_a, fresh_p = hip_engine(S2, text), hip_engine(S2, ptext)
    for eng, image in ((fresh_a, image_p), (fresh_p, image_a)):
        with pytest.raises(HipError) as ei:
            eng.restore(image)
        assert ei.value.code == abi.SH_E_INVALID_ARG
    got = run_calls(fresh_a, calls, S2[5])
    assert agg_carry(fresh_a) == EXPECTED["A1"][1]
    fresh_a.close()
    assert_agg_rows_equal(got, ref)
    gotp = run_calls(fresh_p, pcalls[:12], S2[5])
    fresh_p.close()
    assert_rows_equal(gotp, oracle_rows(S2, ptext, pcalls[:12], S2[5]))


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


def test_public_api_streams_an_aggregating_rule_set():
    """SiddhiManager / InputHandler.send(Event[]) in calls of 37 / StreamCallback on
    the device engine with A1's text, persist() and restoreLastRevision() in the
    middle, against the same calls on the oracle"""
    from siddhi_amd._native import HipEngine
    text, data, calls, ref = agg_ref(A1)
    want = _public_api_run(OracleEngine, text, data, 37)
    got = _public_api_run(HipEngine, text, data, 37, persist_at=80)
    assert len(want) == len(ref["seq"]) > 0
    assert got == want
