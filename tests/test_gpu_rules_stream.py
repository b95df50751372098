"""Rule sets of more than 16 queries streamed through sh_push_batch / sh_drain /
sh_snapshot (the rule engine's carried state, sh_rules.hip + rules_step), exact
against the CPU oracle fed the same send() calls: rows, order, trigger sequence
numbers, query ids, timestamps, values, null flags."""
import ctypes as C

import numpy as np
import pytest

from oracle_engine import OracleEngine
from rules_stream_cases import (S1, S2, S4, STREAM_CASES, assert_rows_equal, calls_of, compiled, oracle_rows,
                                run_calls, send_call, stream_data)
from siddhi_amd import InMemoryPersistenceStore, SiddhiManager, abi

pytestmark = pytest.mark.gpu


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


_cache = {}


def case_ref(ci):
    """a case's text, calls and oracle rows, computed once"""
    if ci not in _cache:
        case = STREAM_CASES[ci]
        text, rules, data = stream_data(case)
        calls = calls_of(case, data)
        _cache[ci] = (text, data, calls, oracle_rows(case, text, calls, case[5]))
    return _cache[ci]


def s1_hip_rows():
    if "s1_hip" not in _cache:
        text, data, calls, ref = case_ref(0)
        eng = hip_engine(S1, text)
        _cache["s1_hip"] = run_calls(eng, calls, S1[5])
        eng.close()
    return _cache["s1_hip"]


@pytest.mark.parametrize("ci", range(len(STREAM_CASES)))
def test_stream_cases_vs_oracle(ci):
    case = STREAM_CASES[ci]
    text, data, calls, ref = case_ref(ci)
    eng = hip_engine(case, text)
    seen = []
    got = run_calls(eng, calls, case[5], after_drain=lambda: seen.append(carry(eng)))
    eng.close()
    assert len(ref["seq"]) > 0
    assert_rows_equal(got, ref)
    assert max(p for p, r in seen) > 0 and max(r for p, r in seen) > 0, seen[:8]
    assert all(0 <= r <= p for p, r in seen)


def test_split_invariance_one_drain_and_bulk_path():
    """S1 drained once at the end, and sh_run_device over the same events with
    batch_events = 64 on a fresh handle, give the rows of the per-call drains"""
    import torch
    from siddhi_amd.device_run import DeviceRunner
    text, data, calls, ref = case_ref(0)
    per_call = s1_hip_rows()
    assert_rows_equal(per_call, ref)
    eng = hip_engine(S1, text)
    once = run_calls(eng, calls, len(calls))
    eng.close()
    assert_rows_equal(once, per_call)
    ts, card, amount, merchant = data
    runner = DeviceRunner(compiled(S1, text))
    dev = torch.device("cuda:0")
    cols = [torch.from_numpy(c).to(dev) for c in (card, amount, merchant)]
    m, seq, vals, q = runner.run(torch.from_numpy(ts).to(dev), cols[0], cols, S1[1], batch_events=S1[4],
                                 with_query=True)
    torch.cuda.synchronize()
    assert m == len(per_call["seq"])
    assert np.array_equal(seq.cpu().numpy(), per_call["seq"].astype(np.int64))
    assert np.array_equal(q.cpu().numpy(), per_call["query"])
    assert np.array_equal(vals.cpu().numpy()[:, :2], per_call["values"][:, :2])
    runner.close()


def _closing_call(case, data, skip_card=None):
    """one event per card, 41 ms after the stream's last event, amount 0: opens
    nothing (every rule wants amount > A >= 10) and is past every window (W <= 40)"""
    n, cards = case[0], case[1]
    ts = data[0]
    ids = np.array([c for c in range(cards) if c != skip_card], np.int32)
    k = len(ids)
    t = np.full(k, int(ts[-1]) + 41, np.int64)
    cols = [ids.copy(), np.zeros(k, np.float32), np.zeros(k, np.int32)]
    return (n, t, cols, ids.copy())


def _card_with_a_live_partial(case, data):
    """a card whose last event opens a partial that an event 1 ms after the stream's
    end can still consume (f1 holds for a rule whose window reaches that far)"""
    ts, card, amount, merchant = data
    free = set(case[8])
    rules = stream_data(case)[1]
    for i in range(len(ts) - 1, -1, -1):
        if np.any(card[i + 1:] == card[i]):
            continue  # not its card's last event
        for r, (a, m, f, w) in enumerate(rules):
            if amount[i] > np.float64(a) and (r in free or merchant[i] == m) and ts[-1] + 1 - ts[i] <= w:
                return int(card[i])
    raise AssertionError("no card ends the stream with a live partial")


@pytest.mark.parametrize("quiet", [False, True], ids=["all-cards", "one-card-quiet"])
def test_carry_is_bounded_by_the_live_partials(quiet):
    """after S4, an event per card beyond every window empties the carried state;
    a card left out keeps its partials, and a later event of it inside the window
    still consumes them"""
    text, data, calls, ref = case_ref(3)
    ts, card, amount, merchant = data
    skip = None
    extra = []
    if quiet:
        skip = _card_with_a_live_partial(S4, data)
        extra.append(_closing_call(S4, data, skip))
        n1 = S4[0] + len(extra[0][1])
        one = np.array([skip], np.int32)
        extra.append((n1, np.array([int(ts[-1]) + 1], np.int64),
                      [one.copy(), np.array([1.0e9], np.float32), np.zeros(1, np.int32)], one.copy()))
    else:
        extra.append(_closing_call(S4, data))
    oeng = OracleEngine(compiled(S4, text))
    oeng.start()
    for c in calls:
        send_call(oeng, c)
    oeng.drain()
    eng = hip_engine(S4, text)
    got = run_calls(eng, calls, S4[5])
    assert_rows_equal(got, ref)
    assert carry(eng)[0] > 0
    send_call(oeng, extra[0])
    send_call(eng, extra[0])
    assert_rows_equal(eng.drain(), oeng.drain())
    if not quiet:
        assert carry(eng) == (0, 0)
    else:
        # only the quiet card's partials are left
        p, r = carry(eng)
        last = ts[np.nonzero(card == skip)[0][-1]]
        live = int(np.sum((card == skip) & (ts >= last - 40)))
        assert 0 < r <= live and p >= r, (p, r, live)
        send_call(oeng, extra[1])
        send_call(eng, extra[1])
        a, b = eng.drain(), oeng.drain()
        assert len(b["seq"]) > 0
        assert_rows_equal(a, b)
    eng.close()
    oeng.close()


def _null_key_calls(calls):
    out = []
    for b0, ts, cols, keys in calls:
        keys = keys.copy()
        keys[(np.arange(b0, b0 + len(keys)) % 7) == 6] = -1
        out.append((b0, ts, cols, keys))
    return out


def test_null_keys_vs_oracle():
    """S2 with every 7th event's key -1: rows and trigger_seq equal the oracle's. A
    null-key event is dropped, still takes its sequence number, and ends the
    same-card run around it (as the oracle and the general engine's streaming path
    end it: 68 of the 4397 rows would come at another position otherwise)"""
    text, data, calls, ref = case_ref(1)
    nk = _null_key_calls(calls)
    ref = oracle_rows(S2, text, nk, S2[5])
    eng = hip_engine(S2, text)
    got = run_calls(eng, nk, S2[5])
    eng.close()
    assert len(ref["seq"]) > 0
    assert_rows_equal(got, ref)


@pytest.mark.parametrize("bad", ["timestamp", "null"])
def test_refused_step_leaves_the_state_alone(bad):
    """after 20 calls a call is refused (a card's timestamp below that card's
    previous event, in an earlier step; a set null-mask bit): the drain fails with
    SH_E_UNSUPPORTED, and the remaining calls give the uninterrupted run's rows"""
    from siddhi_amd._native import HipError
    text, data, calls, ref = case_ref(0)
    ts, card, amount, merchant = data
    eng = hip_engine(S1, text)
    head = run_calls(eng, calls[:20], 1)
    before = carry(eng)
    assert before[0] > 0
    b0, cts, cols, keys = calls[20]
    cts, cols = cts.copy(), [c.copy() for c in cols]
    nulls = [None] * 3
    if bad == "timestamp":
        prev = np.nonzero(card[:b0] == keys[0])[0]
        assert len(prev) and ts[prev[-1]] > 0
        cts[0] = ts[prev[-1]] - 1
    else:
        nm = np.zeros(len(cts), np.uint8)
        nm[3] = 1
        nulls[1] = nm
    eng.send(0, cts, cols, nulls, keys, b0)
    with pytest.raises(HipError) as ei:
        eng.drain()
    assert ei.value.code == abi.SH_E_UNSUPPORTED
    assert carry(eng) == before
    tail = run_calls(eng, calls[20:], 1)
    eng.close()
    assert_rows_equal(abi.concat_drains([head, tail]), ref)


def test_snapshot_restore_continues_exactly():
    from siddhi_amd._native import HipError
    text, data, calls, ref = case_ref(0)
    eng = hip_engine(S1, text)
    head = run_calls(eng, calls[:40], 1)
    assert carry(eng)[0] > 0
    image = eng.snapshot()
    eng.close()
    eng2 = hip_engine(S1, text)
    eng2.restore(image)
    assert carry(eng2)[0] > 0
    tail = run_calls(eng2, calls[40:], 1)
    assert_rows_equal(abi.concat_drains([head, tail]), ref)
    # a handle that has processed events refuses an image
    with pytest.raises(HipError):
        eng2.restore(image)
    eng2.close()
    # another rule set's image is refused
    text2, data2, calls2, ref2 = case_ref(1)
    e2 = hip_engine(S2, text2)
    run_calls(e2, calls2[:6], 3)
    image2 = e2.snapshot()
    e2.close()
    fresh = hip_engine(S1, text)
    with pytest.raises(HipError) as ei:
        fresh.restore(image2)
    assert ei.value.code == abi.SH_E_INVALID_ARG
    # ... and the handle is still usable: the whole run from the start
    got = run_calls(fresh, calls, 1)
    fresh.close()
    assert_rows_equal(got, ref)


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


def test_public_api_streams_a_rule_set():
    """SiddhiManager / SiddhiAppRuntime / InputHandler.send(Event[]) / StreamCallback
    on the device engine, with persist() and restoreLastRevision() in the middle,
    against the same calls on the oracle"""
    from siddhi_amd._native import HipEngine
    text, data, calls, ref = case_ref(0)
    want = _public_api_run(OracleEngine, text, data, S1[4])
    got = _public_api_run(HipEngine, text, data, S1[4], persist_at=47)
    assert len(want) == len(ref["seq"]) > 0
    assert got == want
