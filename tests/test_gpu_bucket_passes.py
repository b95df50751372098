"""GPU parity of the bucketed matcher's pass structure (shb_match: the segment
table a workgroup loads once from the partition's segment prefixes, the passes
cut from it, the halo) through the public DeviceRunner path: trigger sequence
numbers and raw values bit-exact against the CPU oracle (up to ~300k events) or
the C2 restatement (c2_check, larger C2-shaped streams).

Shapes: the smallest that reach each path of the table code. A tile is 8,192
events, a prefix block 64 tiles, a matcher chunk 60 tiles, a pass at most 2,048
consumer events inside a 2,560-event span, the halo at most 64 tiles.

`bucket_status()` 1: the bucketed engine produced the rows; 0: a device premise
failed (or the engine does not apply) and another engine did. BUCKETED lists the
status the engine had on each stream before the segment prefixes existed; the
prefixes change no decision, so the status must stay what it was."""
import numpy as np
import pytest

from c2_check import c2_expected
from oracle_engine import run_stock_oracle
from siddhi_amd import compiler, synth

pytestmark = pytest.mark.gpu

TILE = 8192
T0 = 1_700_000_000_000

# bucket_status() of each stream on the commit before the segment prefixes
BUCKETED = {
    "short": 1, "seams": 1, "kb2": 1, "kb3": 1, "kb8": 1, "dense_40ms": 1, "dense_1s": 0,
    "empty_segments": 0, "sparse_bucket": 1, "big_segment": 0, "equal_ts": 1,
}


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _query(within="1 sec"):
    assert "within 1 sec " in synth.C2_QUERY
    return synth.C2_QUERY.replace("within 1 sec ", "within " + within + " ")


def _run(app, ts, k, p, v, nk, layout=False):
    """layout: False raw rows, "packed" packed rows, True typed columns; all
    returned as (m, seq, raw values), with the engine's status"""
    import torch
    from siddhi_amd.device_run import DeviceRunner, columns_to_raw, packed_to_raw
    runner = DeviceRunner(compiler.compile_app(app))
    dev = torch.device("cuda:0")
    tk = torch.from_numpy(k).to(dev)
    cols = [tk, torch.from_numpy(p).to(dev), torch.from_numpy(v).to(dev)]
    tts = torch.from_numpy(ts).to(dev)
    if layout == "packed":
        offs, rb = runner.packed_layout()
        m, rows = runner.run(tts, tk, cols, nk, packed=True)
        torch.cuda.synchronize()
        status, err = runner.bucket_status(), runner.last_error()
        oseq, ovals = packed_to_raw(rows.cpu().numpy(), runner.out_types, offs, rb)
        oseq = oseq.astype(np.int64)
    else:
        m, oseq, ovals = runner.run(tts, tk, cols, nk, columns=bool(layout))
        torch.cuda.synchronize()
        status, err = runner.bucket_status(), runner.last_error()
        oseq = oseq.cpu().numpy()
        ovals = (columns_to_raw([c.cpu().numpy() for c in ovals], runner.out_types) if layout
                 else ovals.cpu().numpy())
    runner.close()
    return (m, oseq, ovals), status, err


def _check(name, app, ts, k, p, v, nk, expected, layout=False):
    eseq, evals = expected
    (m, oseq, ovals), status, err = _run(app, ts, k, p, v, nk, layout)
    print(f"{name} layout={layout}: n={len(ts)} rows={m} expected={len(eseq)} bucket_status={status}")
    assert len(eseq) > 0
    assert status >= 0, err
    assert status == BUCKETED[name], (status, err)
    assert m == len(eseq)
    assert np.array_equal(oseq, np.asarray(eseq).astype(np.int64))
    assert np.array_equal(ovals, evals)


def _oracle(app, ts, k, p, v):
    seq, _, vals, _ = run_stock_oracle(compiler.compile_app(app), ts, k, p, v)
    return seq, vals


def _prices(rng, n):
    # mostly above the query's threshold of 20, few distinct values: many partials and ties
    return (rng.integers(15, 40, n) + rng.choice([0.0, 0.5, 0.25], n)).astype(np.float32)


def test_short_stream():
    """nt = 4 with a partial last tile: one prefix block, the halo clipped at tile 0"""
    n, nk = 3 * TILE + 17, 2000
    ts, k, p, v = synth.stock_stream(n, nk, 100)
    _check("short", synth.C2_QUERY, ts, k, p, v, nk, _oracle(synth.C2_QUERY, ts, k, p, v))


_seams = {}


def _seam_stream():
    if not _seams:
        n, nk = 130 * TILE + 5, 2000
        ts, k, p, v = synth.stock_stream(n, nk, 100)
        _seams["s"] = (ts, k, p, v, nk, c2_expected(ts, k, p, v))
    return _seams["s"]


@pytest.mark.parametrize("layout", [False, "packed", True])
def test_block_and_chunk_seams(layout):
    """131 tiles: every bucket crosses two 64-tile prefix-block seams and two
    60-tile chunk seams; raw rows, packed rows and typed columns give the same rows"""
    ts, k, p, v, nk, exp = _seam_stream()
    _check("seams", synth.C2_QUERY, ts, k, p, v, nk, exp, layout)


@pytest.mark.parametrize("nk,name", [(1024, "kb2"), (1500, "kb3"), (65536, "kb8")])
def test_local_key_bits(nk, name):
    """2, 3 and 8 (the engine's cap) local key bits"""
    n = 200_000 + 77
    ts, k, p, v = synth.stock_stream(n, nk, 100)
    _check(name, synth.C2_QUERY, ts, k, p, v, nk, _oracle(synth.C2_QUERY, ts, k, p, v))


@pytest.mark.parametrize("within,name", [("40 milliseconds", "dense_40ms"), ("1 sec", "dense_1s")])
def test_dense_bucket_one_tile_per_pass(within, name):
    """12 % of the events on the four keys of one bucket: ~1,000 of its events per
    tile, so its passes take one tile each and the halo tile just fits the span.
    At 40 ms (4,000 events) the halo is one tile; at 1 s it would be 13 tiles and is
    trimmed at the front (sb > 0): walks may leave the span, and the rows are
    exact whichever engine then produces them"""
    n, nk = 300_000 + 11, 1024
    rng = np.random.default_rng(41)
    k = rng.integers(0, nk, n).astype(np.int32)
    hot = rng.random(n) < 0.12
    k[hot] = (7 + 256 * rng.integers(0, 4, n))[hot].astype(np.int32)
    ts = (T0 + np.arange(n) // 100).astype(np.int64)
    p = _prices(rng, n)
    v = rng.integers(1, 1000, n).astype(np.int64)
    app = _query(within)
    _check(name, app, ts, k, p, v, nk, _oracle(app, ts, k, p, v))


def test_mostly_empty_segments():
    """keys of buckets 0, 1 and 255 only, and one key of bucket 77 that first
    appears after tile 5: every other bucket's prefixes are runs of equal values"""
    n, nk = 200_000 + 3, 4096
    rng = np.random.default_rng(42)
    k = (rng.choice([0, 1, 255], n) + 256 * rng.integers(0, 16, n)).astype(np.int32)
    late = np.nonzero(rng.random(n) < 0.01)[0]
    late = late[late > 5 * TILE + 100]
    k[late] = 77 + 256 * 3
    ts = (T0 + np.arange(n) // 100).astype(np.int64)
    p = _prices(rng, n)
    v = rng.integers(1, 1000, n).astype(np.int64)
    _check("empty_segments", synth.C2_QUERY, ts, k, p, v, nk, _oracle(synth.C2_QUERY, ts, k, p, v))


def test_sparse_bucket_between_full_ones():
    """buckets 0..127 uniformly filled (the run stays bucketed) and one key of
    bucket 200 in bursts a few tiles apart: its segment table is mostly empty
    segments between non-empty ones, so seg_of must name the last segment that
    starts at or before each 32-event block"""
    n, nk = 200_000 + 5, 4096
    rng = np.random.default_rng(43)
    k = (rng.integers(0, 128, n) + 256 * rng.integers(0, 16, n)).astype(np.int32)
    i = np.arange(n)
    burst = ((i // TILE) % 3 == 1) & (i % TILE > 4000) & (i % TILE < 4400) & (rng.random(n) < 0.5)
    k[burst] = 200 + 256 * 5
    ts = (T0 + i // 100).astype(np.int64)
    p = _prices(rng, n)
    v = rng.integers(1, 1000, n).astype(np.int64)
    _check("sparse_bucket", synth.C2_QUERY, ts, k, p, v, nk, _oracle(synth.C2_QUERY, ts, k, p, v))


def test_segment_larger_than_a_chunk():
    """one key takes 30 % of a tile: its segment exceeds a pass (SHB_F_SPAN), the
    run falls back and the rows stay exact"""
    n, nk = 100_000 + 9, 2048
    rng = np.random.default_rng(44)
    k = rng.integers(0, nk, n).astype(np.int32)
    tile3 = np.arange(3 * TILE, 4 * TILE)
    k[tile3[rng.random(TILE) < 0.30]] = 5
    ts = (T0 + np.arange(n) // 100).astype(np.int64)
    p = _prices(rng, n)
    v = rng.integers(1, 1000, n).astype(np.int64)
    _check("big_segment", synth.C2_QUERY, ts, k, p, v, nk, _oracle(synth.C2_QUERY, ts, k, p, v))


def test_equal_timestamps_over_70_tiles():
    """every event at one timestamp: the window reaches the start of the stream,
    so the halo runs into its cap of 64 tiles"""
    n, nk = 70 * TILE + 100, 2000
    _, k, p, v = synth.stock_stream(n, nk, 100)
    ts = np.full(n, T0, np.int64)
    _check("equal_ts", synth.C2_QUERY, ts, k, p, v, nk, c2_expected(ts, k, p, v))
