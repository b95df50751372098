"""`output all every N events` behind the fast engines on the GPU: one window-shaped
query in bulk (the bucketed engine with the placement pass behind it) and rule sets of
at most 16 queries against the oracle, and the pass itself (sh_rate.hip, through
shl_limit) against a numpy restatement of the placement rule."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_rate_fast as base
from device_prims import shw_rows, shw_rows_out
from rate_all_cases import BIG, SET_ROWS, SETS, c2, set_ref
from rules_cases import CASES, card_strings
from siddhi_amd import compiler, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ bulk, one window-shaped query
HAVING = "having p2 - p1 > 0.19 and v2 != 3"
C2_A3 = c2("output all every 3 events")
C2_E4 = c2("output every 4 events")
C2_A1 = c2("output all every 1 events")
C2_ABOVE = c2("output all every 100000 events")  # beyond every key's rows: nothing leaves
C2_HAV_A2 = c2(HAVING + " output all every 2 events")
C2_AGG_E5 = c2("output every 5 events", base.C2_AGG_HAVING)
# text -> (the text whose rows reach the limiter, the oracle's rows reaching / leaving it)
C2_ROWS = {C2_A3: (synth.C2_QUERY, 147_118, 145_332), C2_E4: (synth.C2_QUERY, 147_118, 144_388),
           C2_A1: (synth.C2_QUERY, 147_118, 147_118), C2_ABOVE: (synth.C2_QUERY, 147_118, 0),
           C2_HAV_A2: (c2(HAVING), 72_940, 72_064), C2_AGG_E5: (base.C2_AGG_HAVING, 109_774, 106_410)}


def moved(seq):
    return bool(np.any(np.diff(np.asarray(seq).astype(np.int64)) < 0))


def _check_c2(text, layout=None):
    ts, k, p, v = base.bulk_stream()
    before, reach, leave = C2_ROWS[text]
    seq, _, vals, _ = base.bulk_oracle(text)
    assert (len(base.bulk_oracle(before)[0]), len(seq)) == (reach, leave)
    (m, oseq, ovals), st = base._run(text, ts, k, [k, p, v], base.NK_BULK, layout)
    print(text[-60:], st)
    assert st["bucket"] == 1 and st["rate"] == 1, st
    assert st["rows"] == (reach, leave) and st["ms"] > 0.0
    assert m == leave
    assert np.array_equal(oseq[:m], seq.astype(np.int64))
    assert np.array_equal(ovals[:m], vals)
    return st, seq


@pytest.mark.parametrize("layout", [None, "columns", "packed"])
def test_c2_all_every_3_bucketed_vs_oracle(layout):
    st, seq = _check_c2(C2_A3, layout)
    assert moved(seq)


def test_c2_every_4_is_all_every_4():
    st, seq = _check_c2(C2_E4)
    assert moved(seq)


def test_c2_all_every_1_is_the_plain_rows():
    st, seq = _check_c2(C2_A1)
    plain = base.bulk_oracle(synth.C2_QUERY)
    assert np.array_equal(seq, plain[0]) and np.array_equal(base.bulk_oracle(C2_A1)[2], plain[2])


def test_c2_n_above_every_run_releases_nothing():
    _check_c2(C2_ABOVE)


def test_c2_having_then_all_every_2_vs_oracle():
    st, seq = _check_c2(C2_HAV_A2)
    assert st["having"] == 1 and moved(seq)


def test_c2_aggregates_having_and_every_5_vs_oracle():
    st, seq = _check_c2(C2_AGG_E5)
    assert st["having"] == 1 and st["agg"] in (1, 2, 4, 5), st
    assert moved(seq)


def test_c2_switch_runs_the_general_engine(monkeypatch):
    monkeypatch.setenv("SH_NO_RATE_FILTER", "1")
    ts, k, p, v = base.bulk_stream()
    seq, _, vals, _ = base.bulk_oracle(C2_A3)
    (m, oseq, ovals), st = base._run(C2_A3, ts, k, [k, p, v], base.NK_BULK)
    assert st["rate"] == 0 and st["rows"] == (0, 0), st
    assert m == len(seq) == C2_ROWS[C2_A3][2]
    assert np.array_equal(oseq[:m], seq.astype(np.int64))
    assert np.array_equal(ovals[:m], vals)


# ------------------------------------------------------------------ bulk rule sets of at most 16 queries
@pytest.mark.parametrize("sparse", [True, False])
@pytest.mark.parametrize("ci,select", SETS)
def test_bulk_mixed_sets_vs_oracle(ci, select, sparse, monkeypatch):
    import torch
    from siddhi_amd.device_run import DeviceRunner
    n, cards, nr, rate, batch, merchants, partitioned, free, seed = CASES[ci]
    if not sparse:
        monkeypatch.setenv("SH_RULES_SPARSE", "0")
    text, rules, (ts, card, amount, merchant), rows0, ref, key = set_ref(ci, select)
    assert (len(rows0["seq"]), len(ref["seq"])) == SET_ROWS[(ci, select)] and moved(ref["seq"])
    runner = DeviceRunner(compiler.compile_app(text, card_strings(cards)))
    dev = torch.device("cuda:0")
    cols = [torch.from_numpy(c).to(dev) for c in (card, amount, merchant)]
    m, seq, vals, q = runner.run(torch.from_numpy(ts).to(dev), cols[0], cols, cards, batch_events=batch,
                                 with_query=True)
    torch.cuda.synchronize()
    rs, rows = runner.rate_status(), runner.rate_rows()
    seq, vals, q = seq.cpu().numpy(), vals.cpu().numpy(), q.cpu().numpy()
    runner.close()
    print(ci, select, sparse, rs, rows)
    assert m == len(ref["seq"])
    assert np.array_equal(seq[:m], ref["seq"].astype(np.int64))
    assert np.array_equal(q[:m], ref["query"])
    nv = ref["values"].shape[1]
    assert np.array_equal(vals[:m, :nv], ref["values"])
    # the rule rung and the pass, or the general engine's selector
    assert rs in (0, 1)
    if rs == 1:
        assert rows == SET_ROWS[(ci, select)]


# ------------------------------------------------------------------ the pass itself
T = base.T           # SHL_TILE, the pass's scan tile
GUARD, FILL = base.GUARD, base.FILL
NONE, FIRST, LAST, ALL = 0, 1, 2, 3
# the weights' scan (shd_exclusive_scan: tiles of 1,024 entries) takes its second level
# from two tiles on
M_SCAN2 = 1025
M_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17, M_SCAN2]
SHAPES = ["one", "own", "lengths", "cross", "two_queries", "no_limiter", "interleaved", "wide_keys"]
NS = (1, 2, 3, 64, BIG)


def numpy_place(rules, query, key):
    """the source row of every output row, restated: a stable sort by (query, key), the
    ordinal j in each run; an `all every N` row leaves with the row (N - j mod N) mod N
    places on if that is still its run, as number (j - 1) mod N of the N rows the N-th
    releases; the other kinds' kept rows release themselves; a row's place is the
    exclusive scan of the released counts, in row order, at its release row plus its
    number"""
    m = len(query)
    if m == 0:
        return np.zeros(0, np.int64)
    seg = (query.astype(np.uint64) << np.uint64(32)) | key.astype(np.uint32).astype(np.uint64)
    order = np.argsort(seg, kind="stable")
    ss = seg[order]
    head = np.ones(m, bool)
    head[1:] = ss[1:] != ss[:-1]
    pos = np.arange(m, dtype=np.int64)
    j = pos - np.maximum.accumulate(np.where(head, pos, 0)) + 1
    r = np.asarray(rules, np.int64)[(ss >> np.uint64(32)).astype(np.int64)]
    kind, n = r[:, 0], np.maximum(r[:, 1], 1)
    held = kind == ALL
    first = np.where(n == 1, j == 1, (j - 1) % n == 0)
    kept = np.where(kind == FIRST, first, np.where(kind == LAST, j % n == 0, True))
    ahead = np.where(held, (n - j % n) % n, 0)
    number = np.where(held, (j - 1) % n, 0)
    released = np.where(held, np.where(j % n == 0, n, 0), kept.astype(np.int64))
    to = np.minimum(pos + ahead, m - 1)
    leaves = kept & (pos + ahead < m) & (ss[to] == ss)
    w = np.zeros(m, np.int64)
    w[order] = released
    start = np.cumsum(w) - w
    src_of = np.full(int(w.sum()), -1, np.int64)
    src_of[start[order[to[leaves]]] + number[leaves]] = order[leaves]
    assert np.all(src_of >= 0) and len(np.unique(src_of)) == len(src_of)
    return src_of


def _run_place(L, dev, rules, query, key, n_keys, n_out, optional, via_seq, rng, refused=None):
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
    o_q, o_ts, o_nulls, o_key = guarded(m * 4), guarded(m * 8), guarded(m * n_out), guarded(m * 4)
    ws, kept = guarded(ws_words * 4), guarded(8)
    assert ws.data_ptr() % 8 == 0
    src = shw_rows(d_seq.data_ptr(), d_vals.data_ptr(), d_q.data_ptr(), d_ts.data_ptr(), d_nulls.data_ptr(),
                   None if via_seq else d_key.data_ptr())
    with_key = optional and not via_seq
    dst = shw_rows_out(o_seq.data_ptr() if optional else None, o_vals.data_ptr(), o_q.data_ptr() if optional else None,
                       o_ts.data_ptr() if optional else None, o_nulls.data_ptr() if optional else None,
                       o_key.data_ptr() if with_key else None)
    put_k, put_s = C.c_void_p(), C.c_void_p()
    tab = None
    if refused == "table":  # a table with room: the pass would have to start runs from it
        tk = torch.full((16,), -1, dtype=torch.int64, device=dev)
        tst = torch.zeros((32,), dtype=torch.int64, device=dev)
        tab = base.shq_table(tk.data_ptr(), tst.data_ptr(), 16, 1, 0)
    elif refused is None and m % 2:
        tab = base.shq_table(None, None, 0, 1, 0)
    rc = L.shl_limit(d_rules.data_ptr(), len(rules), m, n_out, C.byref(src), d_key.data_ptr() if via_seq else None,
                     n_keys, seq_base if via_seq else 0, C.byref(tab) if tab is not None else None, C.byref(dst),
                     ws.data_ptr(), kept.data_ptr(), stream, C.byref(put_k) if refused == "put" else None,
                     C.byref(put_s) if refused == "put" else None)
    torch.cuda.synchronize()
    outs = ((o_seq, 8, seq), (o_vals, n_out * 8, vals), (o_q, 4, query), (o_ts, 8, ts), (o_nulls, n_out, nulls),
            (o_key, 4, key))
    if refused:
        assert rc == -1 and put_k.value is None and put_s.value is None
        for t, w, a in outs + ((ws, 0, None), (kept, 0, None)):
            assert np.all(t.cpu().numpy() == FILL), "a refused call wrote"
        return
    assert rc == 0
    src_of = numpy_place(rules, query, key)
    k = len(src_of)
    assert out(kept, 8, np.uint64)[0] == k
    out(ws, ws_words * 4, np.uint8)
    written = {id(o_vals)} | ({id(o_seq), id(o_q), id(o_ts), id(o_nulls)} if optional else set()) | (
        {id(o_key)} if with_key else set())
    for t, w, a in outs:
        got = out(t, m * w, np.uint8)
        if id(t) not in written:
            assert np.all(got == FILL), "a NULL destination's neighbour was written"
            continue
        want = np.ascontiguousarray(a[src_of]).view(np.uint8).reshape(-1)
        assert np.array_equal(got[:k * w], want)
        assert np.all(got[k * w:] == FILL), "written behind the released rows"


def _rules_for(shape, n, i):
    """the first query holds rows back; the second one does too, with another N, or
    keeps `first` / `last` rows; the third has no limiter"""
    other = [(ALL, n + 1 if n < BIG else 5), (FIRST, 2), (LAST, 3)][0 if shape == "two_queries" else i % 3]
    return [(ALL, n), other, (NONE, 0)]


@pytest.mark.parametrize("m", M_SIZES)
def test_place_pass_vs_numpy(m):
    """every run shape and N at one size; 1 and 7 value columns, with and without the
    optional columns, the keys from the row-key array or through the sequence numbers"""
    import torch
    L = base._prim_lib()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2000 + m)
    combos = [(s, n) for s in SHAPES if s != "cross" or m > T + 1 for n in NS]
    released = 0
    for i, (shape, n) in enumerate(combos):
        query, key, n_keys = base._shape(shape, m, n if n <= 64 else 3, rng)
        rules = _rules_for(shape, n, i)
        released += len(numpy_place(rules, query, key))
        _run_place(L, dev, rules, query, key, n_keys, (1, 7)[i % 2], i % 3 != 2, i % 4 == 3, rng)
    assert released > 0 or m == 0


@pytest.mark.parametrize("refused", ["put", "table"])
def test_held_rows_are_not_carried(refused):
    """an `all` rule with put_keys / put_state, or with a table that has room: -1, and
    nothing is written"""
    import torch
    L = base._prim_lib()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    query, key, n_keys = base._shape("interleaved", 300, 3, rng)
    _run_place(L, dev, [(FIRST, 2), (ALL, 3), (NONE, 0)], query, key, n_keys, 2, True, False, rng, refused=refused)
