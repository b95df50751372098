"""GPU parity of the bucketed matcher's count walk (shb_match, the per-lane hand-out
walk of a float ordering term and its neighbours) against the CPU oracle, on small
streams built around the walk's edges: walk lengths around the block of SHB_D = 4
predecessors, the 15-step consumed mask and its overflow, the 255-partial count
limit, the window's edges, the first and last local key of a bucket, the first
element of a span, NaN / signed zero / filter-constant prices, the packed
timestamp range and timestamps that go back inside a key. Rows are compared
exactly (trigger sequence numbers and raw select values); every case also checks
its property on the oracle's own output, so none can pass empty.

The streams have 1,024 keys (the engine's minimum: 256 buckets of 4 local keys,
kb = 2, so a packed timestamp has 30 bits) unless a case says otherwise, one event
per millisecond, and fit one matcher chunk. The packed time is centred on the
first event (dt = 2^(31-kb) there), so the cases that need dt near 0 put one event
of a key of its own first, 2^(31-kb) ms after the rest of the stream."""
import numpy as np
import pytest

from oracle_engine import run_columns_oracle, run_stock_oracle
from siddhi_amd import compiler, synth

pytestmark = pytest.mark.gpu

NK = 1024
KB = 2                      # bits of the local key at 1,024 keys
N = 16_384                  # two 8,192-event tiles
BASE = 1_700_000_000_000
W = 1000                    # C2's `within 1 sec`
K = 5                       # the crafted key (bucket 5, local key 0)
FIRST = 6                   # the key of the early-stream cases' first event
RESERVED = (0, 768, 7, 775, K, FIRST)


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _background(n=N, nk=NK, seed=1, early=False):
    """one event per ms over the unreserved keys, prices on both sides of the filter
    constant; early: event 0 (key FIRST) lies 2^(31-kb) ms after the others, so that
    event i >= 1 has the packed time dt = i"""
    rng = np.random.default_rng(seed)
    free = np.setdiff1d(np.arange(nk), RESERVED).astype(np.int32)
    keys = free[rng.integers(0, len(free), n)]
    ts = BASE + np.arange(n, dtype=np.int64)
    price = (rng.integers(5, 40, n) + rng.choice([0.0, 0.5, 0.25], n)).astype(np.float32)
    vol = rng.integers(0, 6, n).astype(np.int64)
    if early:
        keys[0] = FIRST
        ts[0] = BASE + (1 << (31 - KB))
    return ts, keys, price, vol


def _put(stream, pos, key, prices):
    """events pos, pos + 1, ... become events of `key` with the given prices"""
    _, keys, price, _ = stream
    keys[pos:pos + len(prices)] = key
    price[pos:pos + len(prices)] = np.asarray(prices, np.float32)
    return pos + len(prices)


def _runs(stream, pos, lengths):
    """per length L: a stopper (price 1000), L strictly descending prices, a trigger
    above them: the trigger takes the L partials and walks L + 1 steps; the next
    stopper takes the trigger and walks back over the whole run"""
    trig = []
    for L in lengths:
        pos = _put(stream, pos, K, [1000.0] + [500.0 - j for j in range(L)] + [600.0])
        trig.append(pos - 1)
    return pos, trig


def _run_device(app, strings, ts, cols, keys, nk):
    import torch
    from siddhi_amd.device_run import DeviceRunner
    runner = DeviceRunner(compiler.compile_app(app, strings))
    dev = torch.device("cuda:0")
    m, oseq, ovals = runner.run(torch.from_numpy(ts).to(dev), torch.from_numpy(keys).to(dev),
                                [torch.from_numpy(c).to(dev) for c in cols], nk)
    torch.cuda.synchronize()
    status, err = runner.bucket_status(), runner.last_error()
    res = (m, oseq.cpu().numpy(), ovals.cpu().numpy())
    runner.close()
    return res, status, err


def _per_trigger(seq):
    """rows per trigger event of the oracle's output: {trigger seq: rows}"""
    u, c = np.unique(seq.astype(np.int64), return_counts=True)
    return dict(zip(u.tolist(), c.tolist()))


def _c2(stream, nk=NK):
    """the C2 query over the stream on the oracle and on the device"""
    ts, k, p, v = stream
    ca = compiler.compile_app(synth.C2_QUERY)
    seq, _, vals, _ = run_stock_oracle(ca, ts, k, p, v)
    assert len(seq) > 0
    (m, oseq, ovals), status, err = _run_device(synth.C2_QUERY, None, ts, [k, p, v], k, nk)
    assert m == len(seq), (m, len(seq), status, err)
    assert np.array_equal(oseq, seq.astype(np.int64))
    assert np.array_equal(ovals, vals)
    return _per_trigger(seq), status, err


def test_walk_lengths_around_block_edges():
    lengths = [0, 1, 3, 4, 5, 7, 8, 9, 14, 15]
    stream = _background()
    _, trig = _runs(stream, 100, lengths)
    rows, status, err = _c2(stream)
    for L, t in zip(lengths, trig):
        assert rows.get(t, 0) == L, (L, rows.get(t, 0))
    assert status == 1, err


def test_mask_overflow_takes_the_slow_walk():
    lengths = [16, 17, 40, 200]
    stream = _background()
    _, trig = _runs(stream, 100, lengths)
    rows, status, err = _c2(stream)
    for L, t in zip(lengths, trig):
        assert rows[t] == L
    assert 16 <= max(rows.values()) <= 255
    assert status == 1, err


def test_count_overflow_falls_back_exactly():
    stream = _background()
    _, trig = _runs(stream, 100, [300])
    rows, status, err = _c2(stream)
    assert rows[trig[0]] == 300 and max(rows.values()) > 255
    assert status == 0, "a consumer of more than 255 partials must leave the bucketed engine"


def test_window_edge():
    """same-key pairs exactly W, W - 1 and W + 1 ms apart; the first pair's consumer has
    a packed time below W (the window's lower bound clamps to 0)"""
    stream = _background(early=True)
    ts = stream[0]
    pairs = [(10, 500), (3000, W), (6000, W - 1), (9000, W + 1), (12000, W)]
    for p0, d in pairs:
        _put(stream, p0, K, [30.0])
        _put(stream, p0 + d, K, [40.0])
        assert ts[p0 + d] - ts[p0] == d
    assert ts[10 + 500] - (ts[0] - (1 << (31 - KB))) < W
    rows, status, err = _c2(stream)
    got = [rows.get(p0 + d, 0) for p0, d in pairs]
    assert got[0] == 1 and got[2] == 1 and got[3] == 0, got   # inside the window; one past it
    assert got[1] == got[4], got                              # exactly W: whatever the oracle says, both alike
    assert status == 1, err


def test_key_and_position_edges():
    """local key 0 and the largest local key of a bucket (keys b and b + 256 k_max, in
    bucket 0 and bucket 7); a consumer that is its span's first element; a key whose only
    predecessor is that element; the all-zero packed word (key 0 at dt == 0: event 1, as
    the packed time is centred on event 0)"""
    stream = _background(early=True)
    ts, keys = stream[0], stream[1]
    ts[1] = BASE                                # dt == 0
    _put(stream, 1, 0, [30.0])                  # word 0: bucket 0's span starts with it
    _put(stream, 50, 0, [40.0])                 # its only predecessor is the span's first element
    _put(stream, 60, 768, [30.0, 25.0, 50.0])   # bucket 0's largest local key: the span's last elements
    _put(stream, 2, 7, [30.0])                  # bucket 7: sp == 0
    _put(stream, 70, 7, [31.0])
    _put(stream, 80, 775, [22.0, 21.0, 23.0])
    _put(stream, 9000, 775, [30.0])             # the second tile
    assert ts[1] - (ts[0] - (1 << (31 - KB))) == 0 and keys[1] == 0
    rows, status, err = _c2(stream)
    assert rows.get(50) == 1 and rows.get(62) == 2 and rows.get(70) == 1 and rows.get(82) == 2, rows
    assert status == 1, err


def test_value_edges():
    nan = float("nan")
    up = float(np.nextafter(np.float32(20.0), np.float32(np.inf)))
    stream = _background()
    pos = 100
    pos = _put(stream, pos, K, [1000.0, 30.0, 30.0, 30.0, 31.0])       # equal prices: nothing until 31 takes all three
    t_eq = pos - 1
    pos = _put(stream, pos, K, [1000.0, nan, 30.0, 40.0])               # a NaN partial is never taken
    t_nan1 = pos - 1
    pos = _put(stream, pos, K, [1000.0, 30.0, nan, 40.0])               # a NaN consumer takes nothing, hides nothing
    t_nan2 = pos - 1
    pos = _put(stream, pos, K, [1000.0, 0.0, -0.0, 0.0, 25.0])          # zeros are below the filter
    t_zero = pos - 1
    pos = _put(stream, pos, K, [1000.0, 20.0, up, 20.5, 21.0])          # 20 is not > 20, the next float is
    t_flt = pos - 1
    rows, status, err = _c2(stream)
    assert rows.get(t_eq) == 3 and rows.get(t_nan1) == 1 and rows.get(t_nan2) == 1, rows
    assert rows.get(t_zero, 0) == 0 and rows.get(t_flt - 1) == 1 and rows.get(t_flt) == 1, rows
    assert status == 1, err


@pytest.mark.parametrize("past", [0, 1])
def test_timestamp_range(past):
    """the last two events of key K at the top of the packed range (dt = 2^(32-kb) - 1),
    and one past it: the partition then refuses the stream and the general path runs"""
    stream = _background()
    ts = stream[0]
    top = ts[0] + (1 << (31 - KB)) - 1 + past
    _put(stream, N - 2, K, [30.0, 40.0])
    ts[N - 2] = top - 500
    ts[N - 1] = top
    assert ts[N - 1] - (ts[0] - (1 << (31 - KB))) == (1 << (32 - KB)) - 1 + past
    rows, status, err = _c2(stream)
    assert rows.get(N - 1) == 1
    assert status == (0 if past else 1), err


@pytest.mark.parametrize("back", [1, 2])
def test_decreasing_timestamps_inside_a_key(back):
    """a timestamp of key K goes back: at the last consumer's immediate predecessor
    (back = 1) or one event earlier, two steps back from the last consumer (back = 2)"""
    stream = _background()
    ts = stream[0]
    _put(stream, 100, K, [30.0, 31.0, 32.0, 33.0])
    ts[103 - back] -= 50          # now earlier than the event before it, which no longer precedes in time
    assert ts[103 - back] < ts[102 - back]
    rows, status, err = _c2(stream)
    assert max(rows.values()) >= 1
    assert status == 0, "the bucketed engine must not accept decreasing timestamps"


def test_sparse_keys_run_off_the_halo():
    """2,048 keys at one event per ms: a key's previous event is usually more than a
    window back, so most walks leave their key's run while still in the window"""
    n, nk = 60_000, 2048
    ts, k, p, v = synth.stock_stream(n, nk, 1)
    rows, status, err = _c2((ts, k, p, v), nk)
    assert max(rows.values()) >= 1
    assert status >= 0, err


S4 = "define stream S (sym string, price float, volume long, x int); partition with (sym of S) begin "


@pytest.mark.parametrize("query", [
    # an int ordering term (walk_count)
    "from every e1=S[x > 2] -> e2=S[x > e1.x] within 1 sec "
    "select e1.sym as a, e1.x as b, e2.x as c, e2.volume as d insert into Out; end;",
    # no cross term: the first later event that passes its own filter takes every partial
    "from every e1=S[price > 20.0f] -> e2=S[price > 30.0f] within 1 sec "
    "select e1.sym as a, e1.price as b, e2.price as c insert into Out; end;"])
def test_other_walks_stay_bucketed(query):
    app = S4 + query
    ts, keys, price, vol = _background()
    x = np.random.default_rng(3).integers(-3, 25, N).astype(np.int32)
    strings = compiler.StringDict()
    for i in range(NK):
        strings.id(f"K{i}")
    ca = compiler.compile_app(app, strings)
    seq, _, vals, nulls = run_columns_oracle(ca, ts, [keys, price, vol, x], keys)
    assert len(seq) > 0 and max(_per_trigger(seq).values()) >= 2
    (m, oseq, ovals), status, err = _run_device(app, strings, ts, [keys, price, vol, x], keys, NK)
    assert status == 1, err
    assert m == len(seq)
    assert np.array_equal(oseq, seq.astype(np.int64))
    nn = ~nulls.astype(bool)
    assert np.array_equal(ovals[nn], vals[nn])
