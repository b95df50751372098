"""`output first|last every N events` on the fast engines, exact against the CPU
oracle: rule sets of more than 16 queries streamed through sh_push_batch / sh_drain /
sh_snapshot (the limiter pass of sh_rate.hip behind the carried aggregates and the
`having` filter, its counters carried in a table of their own), the public API,
sh_run_device on a window-shaped query (bucketed engine, every row layout, with
`having` and aggregating selects) and on bulk rule sets, and the pass itself through
ctypes against numpy."""
import ctypes as C

import numpy as np
import pytest

from device_prims import shq_table, shw_rows, shw_rows_out
from having_fast_cases import PLAIN, assert_all_rows_equal
from oracle_engine import OracleEngine, run_columns_oracle
from rate_fast_cases import AGGREGATING, BY_NAME, R_F3, mix, rate_ref, with_rate
from rules_cases import CASES, card_strings, case_data, oracle_run
from rules_stream_cases import compiled, run_calls
from siddhi_amd import InMemoryPersistenceStore, SiddhiManager, abi, compiler, synth

pytestmark = pytest.mark.gpu

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


def rate_status(eng):
    from siddhi_amd._native import lib
    a, b = C.c_int64(-1), C.c_int64(-1)
    lib().shx_rate_rows(eng.h, C.byref(a), C.byref(b))
    return lib().shx_rate_status(eng.h), a.value, b.value


# ------------------------------------------------------------------ streamed rule sets
@pytest.mark.parametrize("name", list(BY_NAME))
def test_streamed_limiters_vs_oracle(name):
    from siddhi_amd._native import lib
    rc = BY_NAME[name]
    base = rc[1]
    before, text, data, calls, rows0, ref = rate_ref(rc)
    eng = hip_engine(base, text)
    seen = []
    got = run_calls(eng, calls, base[5], after_drain=lambda: seen.append(rate_status(eng)))
    agg = lib().shx_agg_status(eng.h)
    eng.close()
    assert len(ref["seq"]) == rc[5][1]
    assert_all_rows_equal(got, ref)
    assert all(s[0] == 1 for s in seen)
    # every step limited what reached it: rows in (after any `having`) and rows kept add
    # up (a drain group of several calls is one step)
    assert sum(s[1] for s in seen) == len(rows0["seq"]) and sum(s[2] for s in seen) == rc[5][1]
    if name in AGGREGATING:
        assert agg == CARRIED_SEQUENTIAL


def test_snapshot_restore_continues_and_another_n_is_refused():
    from siddhi_amd._native import HipError
    base = R_F3[1]
    before, text, data, calls, rows0, ref = rate_ref(R_F3)
    every = base[5]
    eng = hip_engine(base, text)
    head = run_calls(eng, calls[:40], every)
    image = eng.snapshot()
    eng.close()
    eng2 = hip_engine(base, text)
    eng2.restore(image)
    assert eng2.snapshot() == image
    tail = run_calls(eng2, calls[40:], every)
    eng2.close()
    assert_all_rows_equal(abi.concat_drains([head, tail]), ref)
    # the same set compiled with `every 4`
    other = text.replace("every 3 events", "every 4 events")
    assert other != text
    eng3 = hip_engine(base, other)
    with pytest.raises(HipError) as ei:
        eng3.restore(image)
    assert ei.value.code == abi.SH_E_INVALID_ARG
    eng3.close()


def test_a_damaged_counter_section_leaves_the_handle_as_it_was():
    from siddhi_amd._native import HipError
    base = R_F3[1]
    before, text, data, calls, rows0, ref = rate_ref(R_F3)
    eng = hip_engine(base, text)
    run_calls(eng, calls[:6], base[5])
    image = bytearray(eng.snapshot())
    eng.close()
    image[-1] = 0x7F  # the last run's counter: first every 3 holds 0..2
    eng2 = hip_engine(base, text)
    fresh = eng2.snapshot()
    with pytest.raises(HipError) as ei:
        eng2.restore(bytes(image))
    assert ei.value.code == abi.SH_E_INVALID_ARG
    assert eng2.snapshot() == fresh
    got = run_calls(eng2, calls, base[5])
    eng2.close()
    assert_all_rows_equal(got, ref)


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


def test_public_api_streams_a_rule_set_with_limiters():
    from siddhi_amd._native import HipEngine
    before, text, data, calls, rows0, ref = rate_ref(R_F3)
    want = _public_api_run(OracleEngine, text, data, 37)
    got = _public_api_run(HipEngine, text, data, 37, persist_at=80)
    assert len(want) == len(ref["seq"]) > 0
    assert got == want


# ------------------------------------------------------------------ bulk, one window-shaped query
INSERT_OUT = " insert into Out;"
C2_HEAD = synth.C2_QUERY[:synth.C2_QUERY.index("select ")]
C2_AGG_HAVING = (C2_HEAD + "select e1.symbol as symbol, sum(e2.volume) as tv, count() as n, e2.price as p2 "
                 "having n > 20 and tv > 100000 insert into Out; end;")


def _c2(clause, text=synth.C2_QUERY):
    assert text.count(INSERT_OUT) == 1
    return text.replace(INSERT_OUT, " " + clause + INSERT_OUT)


C2_F3 = _c2("output first every 3 events")
C2_L4 = _c2("output last every 4 events")
C2_F1 = _c2("output first every 1 events")
C2_HAV_L2 = _c2("having p2 - p1 > 0.19 and v2 != 3 output last every 2 events")
C2_AGG_F5 = _c2("output first every 5 events", C2_AGG_HAVING)
# (text, the oracle's rows, the rows that reach the limiter)
C2_ROWS = {C2_F3: 49_655, C2_L4: 36_097, C2_F1: 1_766, C2_HAV_L2: 36_032, C2_AGG_F5: 22_649}
C2_BEFORE = {C2_F3: synth.C2_QUERY, C2_L4: synth.C2_QUERY, C2_F1: synth.C2_QUERY,
             C2_HAV_L2: _c2("having p2 - p1 > 0.19 and v2 != 3"), C2_AGG_F5: C2_AGG_HAVING}
N_BULK, NK_BULK = 200_000, 2_000   # (the stream of tests/test_gpu_having_fast.py: the bucketed engine takes it)

_bulk = {}


def bulk_stream():
    if "s" not in _bulk:
        _bulk["s"] = synth.stock_stream(N_BULK, NK_BULK, 100)
    return _bulk["s"]


def bulk_oracle(text):
    if text not in _bulk:
        ts, k, p, v = bulk_stream()
        _bulk[text] = run_columns_oracle(compiler.compile_app(text), ts, [k, p, v], k)
    return _bulk[text]


def _run(text, ts, keys, cols, nk, layout=None):
    """(m, seq, raw rows), statuses"""
    import torch
    from siddhi_amd.device_run import DeviceRunner, columns_to_raw, packed_to_raw
    runner = DeviceRunner(compiler.compile_app(text))
    dev = torch.device("cuda:0")
    tc = [torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in cols]
    tts, tk = torch.from_numpy(ts).to(dev), torch.from_numpy(keys).to(dev)
    if layout == "packed":
        offs, rb = runner.packed_layout()
        m, rows = runner.run(tts, tk, tc, nk, packed=True)
        torch.cuda.synchronize()
        seq, vals = packed_to_raw(rows.cpu().numpy(), runner.out_types, offs, rb)
        seq = seq.astype(np.int64)
    elif layout == "columns":
        m, seq, ocols = runner.run(tts, tk, tc, nk, columns=True)
        torch.cuda.synchronize()
        seq, vals = seq.cpu().numpy(), columns_to_raw([c.cpu().numpy() for c in ocols], runner.out_types)
    else:
        m, seq, vals = runner.run(tts, tk, tc, nk)
        torch.cuda.synchronize()
        seq, vals = seq.cpu().numpy(), vals.cpu().numpy()
    st = dict(bucket=runner.bucket_status(), rate=runner.rate_status(), having=runner.having_status(),
              agg=runner.agg_status(), rows=runner.rate_rows(), ms=runner.rate_ms(), err=runner.last_error())
    runner.close()
    return (m, seq, vals), st


def test_c2_plain_rows():
    assert len(bulk_oracle(synth.C2_QUERY)[0]) == 147_118


def _check_c2(text, layout=None):
    ts, k, p, v = bulk_stream()
    seq, _, vals, _ = bulk_oracle(text)
    before = len(bulk_oracle(C2_BEFORE[text])[0])
    assert len(seq) == C2_ROWS[text]
    (m, oseq, ovals), st = _run(text, ts, k, [k, p, v], NK_BULK, layout)
    print(text[-60:], st)
    assert st["bucket"] == 1 and st["rate"] == 1, st
    assert st["rows"] == (before, len(seq)) and st["ms"] > 0.0
    assert m == len(seq) > 0
    assert np.array_equal(oseq, seq.astype(np.int64))
    assert np.array_equal(ovals, vals)
    return st


@pytest.mark.parametrize("layout", [None, "columns", "packed"])
def test_c2_first_every_3_bucketed_vs_oracle(layout):
    _check_c2(C2_F3, layout)


@pytest.mark.parametrize("text", [C2_L4, C2_F1], ids=["last4", "first1"])
def test_c2_other_limiters_vs_oracle(text):
    _check_c2(text)


def test_c2_having_then_limiter_vs_oracle():
    st = _check_c2(C2_HAV_L2)
    assert st["having"] == 1


def test_c2_aggregates_having_and_limiter_vs_oracle():
    st = _check_c2(C2_AGG_F5)
    assert st["having"] == 1 and st["agg"] in (1, 2, 4, 5), st


def test_c2_switch_runs_the_general_engine(monkeypatch):
    monkeypatch.setenv("SH_NO_RATE_FILTER", "1")
    ts, k, p, v = bulk_stream()
    seq, _, vals, _ = bulk_oracle(C2_F3)
    (m, oseq, ovals), st = _run(C2_F3, ts, k, [k, p, v], NK_BULK)
    assert st["rate"] == 0 and st["rows"] == (0, 0), st
    assert m == len(seq)
    assert np.array_equal(oseq, seq.astype(np.int64))
    assert np.array_equal(ovals, vals)


# ------------------------------------------------------------------ bulk rule sets
@pytest.mark.parametrize("sparse", [True, False])
@pytest.mark.parametrize("select", [PLAIN, "max(e2.amount) as hi, count() as n"])
@pytest.mark.parametrize("ci", [1, 0])
def test_bulk_rule_sets_with_limiters_vs_oracle(ci, select, sparse, monkeypatch):
    import torch
    from siddhi_amd.device_run import DeviceRunner
    case = CASES[ci]
    n, cards, nr, rate, batch, merchants, partitioned, free, seed = case
    if not sparse:
        monkeypatch.setenv("SH_RULES_SPARSE", "0")
    plain, rules, (ts, card, amount, merchant) = case_data(case)
    assert plain.count(PLAIN) == nr
    plain = plain.replace(PLAIN, select)
    text = with_rate(plain, mix)
    ref = oracle_run(text, cards, ts, card, amount, merchant, batch, partitioned)
    plain_rows = len(oracle_run(plain, cards, ts, card, amount, merchant, batch, partitioned)["seq"])
    runner = DeviceRunner(compiler.compile_app(text, card_strings(cards)))
    dev = torch.device("cuda:0")
    cols = [torch.from_numpy(c).to(dev) for c in (card, amount, merchant)]
    m, seq, vals, q = runner.run(torch.from_numpy(ts).to(dev), cols[0], cols, cards, batch_events=batch,
                                 with_query=True)
    torch.cuda.synchronize()
    rs, rows = runner.rate_status(), runner.rate_rows()
    seq, vals, q = seq.cpu().numpy(), vals.cpu().numpy(), q.cpu().numpy()
    runner.close()
    assert 0 < len(ref["seq"]) < plain_rows
    assert m == len(ref["seq"])
    assert np.array_equal(seq, ref["seq"].astype(np.int64))
    assert np.array_equal(q, ref["query"])
    nv = ref["values"].shape[1]
    assert np.array_equal(vals[:, :nv], ref["values"])
    if nr > 16:  # beyond the general engine's table: the rule rung and the pass, always
        assert rs == 1 and rows == (plain_rows, len(ref["seq"]))
    else:        # the rule rung and the pass, or the general engine's selector
        assert rs in (0, 1)


# ------------------------------------------------------------------ the pass itself
T = 2048             # SHL_TILE, the pass's scan tile
GUARD = 64
FILL = 0xA5
EMPTY = 0xFFFFFFFFFFFFFFFF
NONE, FIRST, LAST = 0, 1, 2
BIG = 2**31 - 1


def _prim_lib():
    import torch  # noqa: F401  (first: the library shares torch's HIP runtime)
    from device_prims import LIB_PATH
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.shl_limit_ws_words.argtypes = [C.c_int64]
    L.shl_limit_ws_words.restype = C.c_int64
    L.shl_limit.argtypes = [vp, C.c_int32, C.c_int64, C.c_int32, C.POINTER(shw_rows), vp, C.c_int32, C.c_uint64, vp,
                            C.POINTER(shw_rows_out), vp, vp, vp, C.POINTER(vp), C.POINTER(vp)]
    L.shl_limit.restype = C.c_int
    L.shc_put.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp]
    L.shc_put.restype = C.c_int
    return L


def numpy_limit(rules, query, key, carried):
    """the keep mask in row order and {run key: next counter} of the limited queries'
    runs, restated: a stable sort by (query, key), the ordinal inside each run from its
    head, the rule on carried counter + ordinal"""
    m = len(query)
    seg = (query.astype(np.uint64) << np.uint64(32)) | key.astype(np.uint32).astype(np.uint64)
    order = np.argsort(seg, kind="stable")
    ss = seg[order]
    head = np.ones(m, bool)
    head[1:] = ss[1:] != ss[:-1]
    pos = np.arange(m, dtype=np.int64)
    j = pos - np.maximum.accumulate(np.where(head, pos, 0)) + 1
    useg, inv = np.unique(ss, return_inverse=True)
    c0 = np.array([carried.get(int(s), 0) for s in useg], np.int64)[inv]
    r = np.asarray(rules, np.int64)[(ss >> np.uint64(32)).astype(np.int64)]
    kind, n = r[:, 0], np.maximum(r[:, 1], 1)
    first = np.where(n == 1, (c0 == 0) & (j == 1), (c0 + j - 1) % n == 0)
    keep_sorted = np.where(kind == FIRST, first, np.where(kind == LAST, (c0 + j) % n == 0, True))
    keep = np.zeros(m, bool)
    keep[order] = keep_sorted
    tail = np.ones(m, bool)
    tail[:-1] = ss[1:] != ss[:-1]
    nxt = np.where((kind == FIRST) & (n == 1), 1, (c0 + j) % n)
    pairs = {int(s): int(c) for s, c, t, kd in zip(ss[tail], nxt[tail], tail[tail], kind[tail]) if kd != NONE}
    return keep, pairs


def _shape(name, m, n, rng):
    """(query, key, n_keys) of a run shape; n: the first rule's N (small)"""
    q = np.zeros(m, np.int32)
    if name == "one":
        return q, np.zeros(m, np.int32), 1
    if name == "own":
        return q, rng.permutation(m).astype(np.int32), max(m, 1)
    if name == "lengths":  # runs of exactly n, n - 1 and n + 1 rows, one after the other
        lens = [x for x in (n, n - 1, n + 1) if x > 0]
        reps = np.resize(np.array(lens), max(1, m))
        key = np.repeat(np.arange(len(reps)), reps)[:m].astype(np.int32)
        return q, key, int(key.max()) + 1 if m else 1
    if name == "cross":    # a run that crosses a tile boundary by one row
        key = (np.arange(m) > T).astype(np.int32)
        return q, key, 2
    if name == "two_queries":  # two queries with different N on the same key
        return rng.integers(0, 2, m).astype(np.int32), np.full(m, 3, np.int32), 4
    if name == "no_limiter":
        return rng.integers(0, 3, m).astype(np.int32), rng.integers(0, 5, m).astype(np.int32), 5
    if name == "wide_keys":    # key bits + query bits beyond 32: the pass's two-sort form
        return rng.integers(0, 3, m).astype(np.int32), rng.choice(np.array([0, 5, BIG - 1, 1 << 20], np.int32), m), BIG
    assert name == "interleaved"
    return rng.integers(0, 3, m).astype(np.int32), rng.integers(0, 37, m).astype(np.int32), 37


SHAPES = ["one", "own", "lengths", "cross", "two_queries", "no_limiter", "interleaved", "wide_keys"]
LIMITERS = [(kind, n) for kind in (FIRST, LAST) for n in (1, 2, 3, 64, BIG)]
# every multi-level scan and carry at its second level: the carry launch's threads walk
# two tiles each beyond 1024 scan tiles, which is beyond the 1024 compaction tiles and
# the 1024 radix histogram words one scan block covers
M_LEVEL2 = 1025 * T + 5
M_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17, M_LEVEL2]


def _run_pass(L, dev, rules, query, key, n_keys, n_out, carried, table, via_seq, rng):
    import torch
    m = len(query)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def guarded(nbytes):
        return torch.full((nbytes + 4 * GUARD,), FILL, dtype=torch.uint8, device=dev)

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def out(t, nbytes, dtype):
        a = t.cpu().numpy()
        assert np.all(a[nbytes:] == FILL), "guard"
        return a[:nbytes].view(dtype)

    seq_base = 1 << 33
    seq = (seq_base + np.arange(m)).astype(np.uint64) if via_seq else rng.integers(0, 1 << 40, m).astype(np.uint64)
    vals = rng.integers(-(1 << 60), 1 << 60, (m, n_out)).astype(np.int64)
    ts = rng.integers(0, 1 << 40, m).astype(np.int64)
    nulls = (rng.random((m, n_out)) < 0.2).astype(np.uint8)
    d_rules = to_dev(np.asarray(rules, np.int32).reshape(-1, 2))
    d_seq, d_vals, d_q, d_ts, d_nulls = to_dev(seq.view(np.int64)), to_dev(vals), to_dev(query), to_dev(ts), to_dev(nulls)
    d_key = to_dev(key)
    ws_words = L.shl_limit_ws_words(m)
    o_seq, o_vals = guarded(m * 8), guarded(m * n_out * 8)
    o_q, o_ts, o_nulls = guarded(m * 4), guarded(m * 8), guarded(m * n_out)
    ws, kept = guarded(ws_words * 4), guarded(8)
    assert ws.data_ptr() % 8 == 0
    tab, keep_alive = None, []
    if table == "zero":
        tab = shq_table(None, None, 0, 1, 0)
    elif table == "filled":
        n_ent = max(1, len(carried))
        cap = 16
        while cap < 2 * n_ent:
            cap *= 2
        tk = torch.full((cap,), -1, dtype=torch.int64, device=dev)  # SHQ_EMPTY
        tst = torch.zeros((cap * 2,), dtype=torch.int64, device=dev)
        ctl = torch.zeros((4,), dtype=torch.int64, device=dev)
        tab = shq_table(tk.data_ptr(), tst.data_ptr(), cap, 1, 0)
        pk = np.array(list(carried.keys()) or [EMPTY], np.uint64)
        fin = np.zeros((len(pk), 2), np.int64)
        fin[:, 0] = list(carried.values()) or [0]
        d_pk, d_fin = to_dev(pk.view(np.int64)), to_dev(fin)
        assert L.shc_put(C.byref(tab), d_pk.data_ptr(), d_fin.data_ptr(), len(pk), ctl.data_ptr(),
                         ctl.data_ptr() + 8, stream) == 0
        keep_alive += [tk, tst, ctl, d_pk, d_fin]
    put_k, put_s = C.c_void_p(), C.c_void_p()
    src = shw_rows(d_seq.data_ptr(), d_vals.data_ptr(), d_q.data_ptr(), d_ts.data_ptr(), d_nulls.data_ptr(),
                   None if via_seq else d_key.data_ptr())
    dst = shw_rows_out(o_seq.data_ptr(), o_vals.data_ptr(), o_q.data_ptr(), o_ts.data_ptr(), o_nulls.data_ptr(), None)
    rc = L.shl_limit(d_rules.data_ptr(), len(rules), m, n_out, C.byref(src), d_key.data_ptr() if via_seq else None,
                     n_keys, seq_base if via_seq else 0, C.byref(tab) if tab is not None else None, C.byref(dst),
                     ws.data_ptr(), kept.data_ptr(), stream, C.byref(put_k), C.byref(put_s))
    assert rc == 0
    torch.cuda.synchronize()
    if table == "filled":
        assert int(keep_alive[2].cpu()[0]) == len(carried) and int(keep_alive[2].cpu()[1]) == 0
    keep, pairs = numpy_limit(rules, query, key, carried if table == "filled" else {})
    k = int(keep.sum())
    assert out(kept, 8, np.uint64)[0] == k
    wsb = out(ws, ws_words * 4, np.uint8)
    assert np.array_equal(out(o_seq, m * 8, np.uint64)[:k], seq[keep])
    assert np.array_equal(out(o_vals, m * n_out * 8, np.int64).reshape(m, n_out)[:k], vals[keep])
    assert np.array_equal(out(o_q, m * 4, np.int32)[:k], query[keep])
    assert np.array_equal(out(o_ts, m * 8, np.int64)[:k], ts[keep])
    assert np.array_equal(out(o_nulls, m * n_out, np.uint8).reshape(m, n_out)[:k], nulls[keep])
    # nothing behind the kept rows is written
    for t, w in ((o_seq, 8), (o_vals, n_out * 8), (o_q, 4), (o_ts, 8), (o_nulls, n_out)):
        assert np.all(out(t, m * w, np.uint8)[k * w:] == FILL)
    if m == 0:
        assert put_k.value is None and put_s.value is None
        return
    # the (run key, counter) pairs shc_put takes, inside the workspace
    ko, so = put_k.value - ws.data_ptr(), put_s.value - ws.data_ptr()
    assert 0 <= ko and ko + m * 8 <= ws_words * 4 and 0 <= so and so + m * 16 <= ws_words * 4
    pk = wsb[ko:ko + m * 8].view(np.uint64)
    fin = wsb[so:so + m * 16].view(np.int64).reshape(m, 2)
    live = pk != np.uint64(EMPTY)
    got = dict(zip(pk[live].tolist(), fin[live, 0].tolist()))
    assert int(live.sum()) == len(got), "a run wrote two pairs"
    assert got == pairs


def _carried_for(rules, query, key, rng, rows=None):
    """a counter != 0 for about half of the limited runs (those of the first `rows`
    rows) whose rule can hold one: first every N holds 0 .. max(N, 2) - 1, last every N
    0 .. N - 1"""
    seg = np.unique((query[:rows].astype(np.uint64) << np.uint64(32)) |
                    key[:rows].astype(np.uint32).astype(np.uint64))
    out = {}
    for s in seg.tolist():
        kind, n = rules[s >> 32]
        hi = 0 if kind == NONE else max(n, 2) if kind == FIRST else n
        if hi > 1 and rng.random() < 0.5:
            out[s] = int(rng.integers(1, hi))
    return out


@pytest.mark.parametrize("m", M_SIZES)
def test_limit_pass_vs_numpy(m):
    """every run shape and limiter at one size, the tables in turn: none, capacity 0,
    filled beforehand through shc_put so that runs start at c0 != 0; the keys come from
    the row-key array, every fourth time through the sequence numbers"""
    import torch
    L = _prim_lib()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1000 + m % 9973)
    big = m == M_LEVEL2
    if big:  # (one run over all rows: ordinals beyond two million; 70,000 keys: three radix passes)
        combos = [("interleaved", (FIRST, 3)), ("one", (LAST, 2))]
    else:
        combos = [(s, lim) for s in SHAPES if s != "cross" or m > T + 1 for lim in LIMITERS]
    for i, (shape, (kind, n)) in enumerate(combos):
        query, key, n_keys = _shape(shape, m, n if n <= 64 else 3, rng)
        if big and shape == "interleaved":
            n_keys = 70_000
            key = rng.integers(0, n_keys, m).astype(np.int32)
        other = (LAST if kind == FIRST else FIRST, n + 1 if n < BIG else 5)
        rules = [(kind, n), other, (NONE, 0)]
        table = "filled" if big else ("none", "zero", "filled")[i % 3]
        carried = _carried_for(rules, query, key, rng, 64 if big else None) if table == "filled" else {}
        _run_pass(L, dev, rules, query, key, n_keys, 1 if big else (1, 7)[i % 2], carried, table, i % 4 == 3, rng)
