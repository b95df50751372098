"""An output-only `having` on the fast engines, exact against the CPU oracle: rule
sets of more than 16 queries streamed through sh_push_batch / sh_drain / sh_snapshot
(the device row filter of sh_having.hip between the carried aggregate pass and the
host queue), the public API, sh_run_device on a window-shaped query (bucketed
engine, every row layout, aggregating selects) and on bulk rule sets, and the filter
primitive itself through ctypes against numpy."""
import ctypes as C

import numpy as np
import pytest

from device_prims import shw_rows, shw_rows_out
from having_fast_cases import (AGGREGATING, BY_NAME, H1, H2, INSERT, PLAIN, assert_all_rows_equal, having_ref,
                               with_having)
from oracle_engine import OracleEngine, run_columns_oracle
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


def having_status(eng):
    from siddhi_amd._native import lib
    a, b = C.c_int64(-1), C.c_int64(-1)
    lib().shx_having_rows(eng.h, C.byref(a), C.byref(b))
    return lib().shx_having_status(eng.h), a.value, b.value


# ------------------------------------------------------------------ streamed rule sets
@pytest.mark.parametrize("name", list(BY_NAME))
def test_streamed_having_vs_oracle(name):
    from siddhi_amd._native import lib
    hc = BY_NAME[name]
    base = hc[1]
    plain, text, data, calls, rows0, ref = having_ref(hc)
    eng = hip_engine(base, text)
    seen = []
    got = run_calls(eng, calls, base[5], after_drain=lambda: seen.append(having_status(eng)))
    status = having_status(eng)[0]
    agg = lib().shx_agg_status(eng.h)
    eng.close()
    assert len(ref["seq"]) == hc[4][1]
    assert_all_rows_equal(got, ref)
    assert status == 1 and all(s[0] == 1 for s in seen)
    # every step filtered what it matched: the unfiltered and the kept rows add up
    # (a drain group of several calls is one step)
    assert sum(s[1] for s in seen) == hc[4][0] and sum(s[2] for s in seen) == hc[4][1]
    if name in AGGREGATING:
        assert agg == CARRIED_SEQUENTIAL


def test_snapshot_restore_continues_and_other_thresholds_are_refused():
    from siddhi_amd._native import HipError
    base = H2[1]
    plain, text, data, calls, rows0, ref = having_ref(H2)
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
    # the same set with one threshold changed
    other = text.replace("total > 250.0", "total > 251.0")
    assert other != text and text.count("total > 250.0") == 1
    eng3 = hip_engine(base, other)
    with pytest.raises(HipError) as ei:
        eng3.restore(image)
    assert ei.value.code == abi.SH_E_INVALID_ARG
    eng3.close()


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


def test_public_api_streams_a_rule_set_with_having():
    from siddhi_amd._native import HipEngine
    plain, text, data, calls, rows0, ref = having_ref(H1)
    want = _public_api_run(OracleEngine, text, data, 37)
    got = _public_api_run(HipEngine, text, data, 37, persist_at=80)
    assert len(want) == len(ref["seq"]) > 0
    assert got == want


# ------------------------------------------------------------------ bulk, one window-shaped query
C2_HEAD = synth.C2_QUERY[:synth.C2_QUERY.index("select ")]
C2_HAVING = synth.C2_QUERY.replace(" insert into Out;", " having p2 - p1 > 0.19 and v2 != 3 insert into Out;")
C2_AGG_HAVING = (C2_HEAD + "select e1.symbol as symbol, sum(e2.volume) as tv, count() as n, e2.price as p2 "
                 "having n > 20 and tv > 100000 insert into Out; end;")
N_BULK, NK_BULK = 200_000, 2_000   # (the key count of tests/test_gpu_bucket.py)

_bulk = {}


def bulk_stream():
    if "s" not in _bulk:
        _bulk["s"] = synth.stock_stream(N_BULK, NK_BULK, 100)
    return _bulk["s"]


def bulk_oracle(text, cols=None):
    if text not in _bulk:
        ts, k, p, v = bulk_stream()
        _bulk[text] = run_columns_oracle(compiler.compile_app(text), ts, cols or [k, p, v], k)
    return _bulk[text]


def _run(text, ts, keys, cols, nk, layout=None):
    """(m, seq or None, raw rows), statuses"""
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
    st = dict(bucket=runner.bucket_status(), having=runner.having_status(), agg=runner.agg_status(),
              rows=runner.having_rows(), err=runner.last_error())
    runner.close()
    return (m, seq, vals), st


def test_c2_having_keeps_some_and_drops_some():
    seq0 = bulk_oracle(synth.C2_QUERY)[0]
    seq1 = bulk_oracle(C2_HAVING)[0]
    assert 0 < len(seq1) < len(seq0)


@pytest.mark.parametrize("layout", [None, "columns", "packed"])
def test_c2_having_bucketed_vs_oracle(layout):
    ts, k, p, v = bulk_stream()
    seq, _, vals, _ = bulk_oracle(C2_HAVING)
    unfiltered = len(bulk_oracle(synth.C2_QUERY)[0])
    (m, oseq, ovals), st = _run(C2_HAVING, ts, k, [k, p, v], NK_BULK, layout)
    assert st["bucket"] == 1 and st["having"] == 1, st
    assert st["rows"] == (unfiltered, len(seq))
    assert m == len(seq) > 0
    assert np.array_equal(oseq, seq.astype(np.int64))
    assert np.array_equal(ovals, vals)


def test_c2_having_over_aggregates_vs_oracle():
    ts, k, p, v = bulk_stream()
    seq, _, vals, _ = bulk_oracle(C2_AGG_HAVING)
    (m, oseq, ovals), st = _run(C2_AGG_HAVING, ts, k, [k, p, v], NK_BULK)
    assert st["having"] == 1 and st["agg"] in (1, 2, 4, 5), st
    assert 0 < len(seq) < st["rows"][0]
    assert m == len(seq)
    assert np.array_equal(oseq, seq.astype(np.int64))
    assert np.array_equal(ovals, vals)


def test_sum_that_rounds_with_having_vs_oracle():
    """the MIXED_TEXT shape of tests/agg_minmax_cases.py (the post-pass answers "not
    exact", the sequential engine reruns: status 2) with a `having` on the sum"""
    from agg_minmax_cases import MIXED_TEXT
    text = MIXED_TEXT.replace(" insert into Out;", " having total > 100.0 insert into Out;")
    ts, k, p, v = synth.stock_stream(60_000, 256, 100)
    y = np.round(p.astype(np.float64) + 0.003, 2)
    seq, _, vals, _ = run_columns_oracle(compiler.compile_app(text), ts, [k, p, y], k)
    (m, oseq, ovals), st = _run(text, ts, k, [k, p, y], 256)
    assert st["having"] == 1 and st["agg"] == 2, st
    assert 0 < len(seq) < st["rows"][0]
    assert m == len(seq)
    assert np.array_equal(oseq, seq.astype(np.int64))
    assert np.array_equal(ovals, vals)


# ------------------------------------------------------------------ bulk rule sets
def _rules_text(case, select):
    text, rules, data = case_data(case)
    assert text.count(PLAIN) == case[2]
    text = text.replace(PLAIN, select)
    if select == PLAIN:
        return with_having(text, lambda r: f"amount > {40.0 + 3 * r}"), data
    return with_having(text, lambda r: "n > 1"), data


@pytest.mark.parametrize("sparse", [True, False])
@pytest.mark.parametrize("select", [PLAIN, "max(e2.amount) as hi, count() as n"])
@pytest.mark.parametrize("ci", [1, 0])
def test_bulk_rule_sets_with_having_vs_oracle(ci, select, sparse, monkeypatch):
    import torch
    from siddhi_amd.device_run import DeviceRunner
    case = CASES[ci]
    n, cards, nr, rate, batch, merchants, partitioned, free, seed = case
    if not sparse:
        monkeypatch.setenv("SH_RULES_SPARSE", "0")
    text, (ts, card, amount, merchant) = _rules_text(case, select)
    ref = oracle_run(text, cards, ts, card, amount, merchant, batch, partitioned)
    plain_rows = len(oracle_run(_strip_having(text), cards, ts, card, amount, merchant, batch, partitioned)["seq"])
    runner = DeviceRunner(compiler.compile_app(text, card_strings(cards)))
    dev = torch.device("cuda:0")
    cols = [torch.from_numpy(c).to(dev) for c in (card, amount, merchant)]
    m, seq, vals, q = runner.run(torch.from_numpy(ts).to(dev), cols[0], cols, cards, batch_events=batch,
                                 with_query=True)
    torch.cuda.synchronize()
    hs, rows = runner.having_status(), runner.having_rows()
    seq, vals, q = seq.cpu().numpy(), vals.cpu().numpy(), q.cpu().numpy()
    runner.close()
    assert 0 < len(ref["seq"]) < plain_rows
    assert m == len(ref["seq"])
    assert np.array_equal(seq, ref["seq"].astype(np.int64))
    assert np.array_equal(q, ref["query"])
    nv = ref["values"].shape[1]
    assert np.array_equal(vals[:, :nv], ref["values"])
    if nr > 16:  # beyond the general engine's table: the rule rung and the filter, always
        assert hs == 1 and rows == (plain_rows, len(ref["seq"]))
    else:        # the rule rung and the filter, or the general engine's selector
        assert hs in (0, 1)


def _strip_having(text):
    import re
    return re.sub(r" having [^;]*? insert into", " insert into", text)


# ------------------------------------------------------------------ the filter primitive
SH_T_LONG, SH_OP_GT, DOM_I64 = 2, 7, 1
OPC_CONST, OPC_CMP, OPC_OUTPUT = 0, 6, 12
TILE = 256           # SHV_TILE
SCAN_TILE = 1024     # tiles one scan block covers
GUARD = 64
FILL = 0xA5


class shv_instr(C.Structure):
    _fields_ = [("op", C.c_uint8), ("a", C.c_uint8), ("b", C.c_uint8), ("lt", C.c_uint8), ("rt", C.c_uint8),
                ("x", C.c_uint8), ("pad", C.c_uint8 * 2)]


class shv_prog(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_const", C.c_int32), ("code", shv_instr * 32), ("consts", C.c_int64 * 16)]


def _greater_than(c):
    """col0 > c, both long"""
    P = shv_prog()
    P.n, P.n_const = 3, 1
    P.consts[0] = c
    P.code[0] = shv_instr(OPC_OUTPUT, 0, 0, SH_T_LONG, 0, 0)
    P.code[1] = shv_instr(OPC_CONST, 0, 0, SH_T_LONG, 0, 0)
    P.code[2] = shv_instr(OPC_CMP, SH_OP_GT, DOM_I64, SH_T_LONG, SH_T_LONG, 0)
    return P


def _prim_lib():
    import torch  # noqa: F401  (first: the library shares torch's HIP runtime)
    from device_prims import LIB_PATH
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.shv_filter_ws_words.argtypes = [C.c_int64]
    L.shv_filter_ws_words.restype = C.c_int64
    L.shv_filter.argtypes = [vp, C.c_int32, C.c_int64, C.c_int32, C.POINTER(shw_rows), C.POINTER(shw_rows_out),
                             vp, vp, vp]
    L.shv_filter.restype = C.c_int
    return L


def _ptrs(cls, **cols):
    """a row set from device tensors (a column left out, or None, is NULL)"""
    return cls(**{k: t.data_ptr() for k, t in cols.items() if t is not None})


M_TILES = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, (SCAN_TILE + 2) * TILE + 5]
PATTERNS = ["all", "none", "alternating", "last", "first", "last_tile"]


def _pattern(m, pattern):
    keep = np.zeros(m, bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "alternating":
        keep[::2] = True
    elif pattern == "last":
        keep[-1] = True
    elif pattern == "first":
        keep[0] = True
    elif pattern == "last_tile":
        keep[(m - 1) // TILE * TILE:] = True
    return keep


@pytest.mark.parametrize("extras", [True, False])
@pytest.mark.parametrize("n_out", [1, 7])
@pytest.mark.parametrize("m", M_TILES)
def test_filter_primitive_vs_numpy(m, n_out, extras):
    """every keep pattern at one size; with the query / ts / nulls arrays, a null flag
    on the compared column of every 5th kept row drops it"""
    import torch
    L = _prim_lib()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(m * 31 + n_out)
    P = (shv_prog * 2)(_greater_than(1000), _greater_than(1000))
    d_prog = torch.from_numpy(np.frombuffer(bytes(P), np.uint8).copy()).to(dev)
    ws_words = L.shv_filter_ws_words(m)
    for pattern in PATTERNS:
        keep = _pattern(m, pattern)
        vals = rng.integers(-500, 500, (m, n_out)).astype(np.int64)
        vals[keep, 0] += 2000
        seq = rng.integers(0, 1 << 40, m).astype(np.uint64)
        query = rng.integers(0, 2, m).astype(np.int32)
        ts = rng.integers(0, 1 << 40, m).astype(np.int64)
        nulls = np.zeros((m, n_out), np.uint8)
        if extras:
            nulls[np.flatnonzero(keep)[::5], 0] = 1
            nulls[:, n_out - 1] |= (rng.random(m) < 0.3).astype(np.uint8) if n_out > 1 else 0
            keep = keep & (nulls[:, 0] == 0)
        k = int(keep.sum())

        def guarded(nbytes):
            return torch.full((nbytes + 4 * GUARD,), FILL, dtype=torch.uint8, device=dev)

        def to_dev(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

        key = rng.integers(-(1 << 31), 1 << 31, m).astype(np.int32)
        d_seq, d_vals = to_dev(seq.view(np.int64)), to_dev(vals)
        d_q, d_ts, d_nulls, d_key = to_dev(query), to_dev(ts), to_dev(nulls), to_dev(key)
        o_seq, o_vals = guarded(m * 8), guarded(m * n_out * 8)
        o_q, o_ts, o_nulls, o_key = guarded(m * 4), guarded(m * 8), guarded(m * n_out), guarded(m * 4)
        ws, kept = guarded(ws_words * 4), guarded(8)
        # (without the extras the optional columns are NULL on both sides: a NULL
        # destination never asks for its source)
        src = _ptrs(shw_rows, seq=d_seq, vals=d_vals, **(dict(query=d_q, ts=d_ts, nulls=d_nulls, key=d_key)
                                                          if extras else {}))
        dst = _ptrs(shw_rows_out, seq=o_seq, vals=o_vals, **(dict(query=o_q, ts=o_ts, nulls=o_nulls, key=o_key)
                                                              if extras else {}))
        rc = L.shv_filter(d_prog.data_ptr(), 2, m, n_out, C.byref(src), C.byref(dst), ws.data_ptr(), kept.data_ptr(),
                          torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()

        def out(t, nbytes, dtype):
            a = t.cpu().numpy()
            assert np.all(a[nbytes:] == FILL), "guard"
            return a[:nbytes].view(dtype)

        assert out(kept, 8, np.uint64)[0] == k, pattern
        out(ws, ws_words * 4, np.uint8)
        got_seq, got_vals = out(o_seq, m * 8, np.uint64), out(o_vals, m * n_out * 8, np.int64).reshape(m, n_out)
        assert np.array_equal(got_seq[:k], seq[keep]), pattern
        assert np.array_equal(got_vals[:k], vals[keep]), pattern
        # nothing behind the kept rows is written
        assert np.all(out(o_seq, m * 8, np.uint8)[k * 8:] == FILL)
        assert np.all(out(o_vals, m * n_out * 8, np.uint8)[k * n_out * 8:] == FILL)
        got_q, got_ts = out(o_q, m * 4, np.int32), out(o_ts, m * 8, np.int64)
        got_nulls = out(o_nulls, m * n_out, np.uint8).reshape(m, n_out)
        got_key = out(o_key, m * 4, np.int32)
        if extras:
            assert np.array_equal(got_q[:k], query[keep]) and np.array_equal(got_ts[:k], ts[keep])
            assert np.array_equal(got_nulls[:k], nulls[keep])
            assert np.array_equal(got_key[:k], key[keep]), pattern
            assert np.all(out(o_key, m * 4, np.uint8)[k * 4:] == FILL)
        else:
            assert np.all(out(o_q, m * 4, np.uint8) == FILL) and np.all(out(o_ts, m * 8, np.uint8) == FILL)
            assert np.all(out(o_nulls, m * n_out, np.uint8) == FILL)
            assert np.all(out(o_key, m * 4, np.uint8) == FILL)


@pytest.mark.parametrize("col", ["key", "ts"])
def test_filter_primitive_refuses_a_destination_without_its_source(col):
    """dst.key (dst.ts) set while src.key (src.ts) is NULL: -1, nothing launched --
    every output, the workspace and the kept word stay as filled"""
    import torch
    L = _prim_lib()
    dev = torch.device("cuda:0")
    m, n_out = TILE + 1, 2
    P = (shv_prog * 1)(_greater_than(-1))   # (would keep every row)
    d_prog = torch.from_numpy(np.frombuffer(bytes(P), np.uint8).copy()).to(dev)
    ws_words = L.shv_filter_ws_words(m)

    def guarded(nbytes):
        return torch.full((nbytes + 4 * GUARD,), FILL, dtype=torch.uint8, device=dev)

    d_vals = torch.arange(m * n_out, dtype=torch.int64, device=dev)
    o_vals, o_col, ws, kept = guarded(m * n_out * 8), guarded(m * 8), guarded(ws_words * 4), guarded(8)
    src = _ptrs(shw_rows, vals=d_vals)
    dst = _ptrs(shw_rows_out, vals=o_vals, **{col: o_col})
    rc = L.shv_filter(d_prog.data_ptr(), 1, m, n_out, C.byref(src), C.byref(dst), ws.data_ptr(), kept.data_ptr(),
                      torch.cuda.current_stream(dev).cuda_stream)
    assert rc == -1
    torch.cuda.synchronize()
    for t in (o_vals, o_col, ws, kept):
        assert bool((t == FILL).all()), col


def test_filter_primitive_zero_rows():
    import torch
    L = _prim_lib()
    dev = torch.device("cuda:0")
    P = (shv_prog * 1)(_greater_than(0))
    d_prog = torch.from_numpy(np.frombuffer(bytes(P), np.uint8).copy()).to(dev)
    kept = torch.full((8 + 4 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    rc = L.shv_filter(d_prog.data_ptr(), 1, 0, 1, None, None, None, kept.data_ptr(),
                      torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    a = kept.cpu().numpy()
    assert a[:8].view(np.uint64)[0] == 0 and np.all(a[8:] == FILL)
