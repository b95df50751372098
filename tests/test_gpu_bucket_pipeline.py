"""GPU parity of the bucketed engine's pipeline over time segments (run_bucket:
the matchers of segment 0, 1, ... on the caller's stream, each segment's carry
scan and emitter behind an event on the handle's side stream) through the public
DeviceRunner path: trigger sequence numbers and raw values bit-exact against the
C2 restatement (c2_check) or the CPU oracle, and equal to the single-launch form
(`SH_BK_SEG=0`) on the same arrays.

`SH_BK_SEG` is the number of matcher chunks per segment, read on every call. A
tile is 8,192 events, a matcher chunk 60 tiles, so the 131-tile stream has three
chunks: `SH_BK_SEG=1` gives three segments, `SH_BK_SEG=2` an uneven last one."""
import numpy as np
import pytest

from c2_check import c2_expected
from oracle_engine import run_stock_oracle
from siddhi_amd import compiler, synth

pytestmark = pytest.mark.gpu

TILE = 8192
T0 = 1_700_000_000_000

# bucket_status() of the dense 70-tile stream on the commit before the pipeline
# (the single-launch form)
DENSE_70_STATUS = 1


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _query(within):
    assert "within 1 sec " in synth.C2_QUERY
    return synth.C2_QUERY.replace("within 1 sec ", "within " + within + " ")


def _once(runner, ts, k, p, v, nk, layout=False):
    """one run of an open runner. layout: False raw rows, "packed" packed rows,
    True typed columns; all returned as (m, seq, raw values), with the status"""
    import torch
    from siddhi_amd.device_run import columns_to_raw, packed_to_raw
    dev = torch.device("cuda:0")
    tk = torch.from_numpy(k).to(dev)
    cols = [tk, torch.from_numpy(p).to(dev), torch.from_numpy(v).to(dev)]
    tts = torch.from_numpy(ts).to(dev)
    torch.cuda.synchronize()
    if layout == "packed":
        offs, rb = runner.packed_layout()
        m, rows = runner.run(tts, tk, cols, nk, packed=True)
        torch.cuda.current_stream().synchronize()
        status, err = runner.bucket_status(), runner.last_error()
        oseq, ovals = packed_to_raw(rows.cpu().numpy(), runner.out_types, offs, rb)
        oseq = oseq.astype(np.int64)
    else:
        m, oseq, ovals = runner.run(tts, tk, cols, nk, columns=bool(layout))
        torch.cuda.current_stream().synchronize()
        status, err = runner.bucket_status(), runner.last_error()
        oseq = oseq.cpu().numpy()
        ovals = (columns_to_raw([c.cpu().numpy() for c in ovals], runner.out_types) if layout
                 else ovals.cpu().numpy())
    return (m, oseq, ovals), status, err


def _run(app, ts, k, p, v, nk, layout=False):
    from siddhi_amd.device_run import DeviceRunner
    runner = DeviceRunner(compiler.compile_app(app))
    try:
        return _once(runner, ts, k, p, v, nk, layout)
    finally:
        runner.close()


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _exact(out, expected):
    eseq, evals = expected
    m, oseq, ovals = out
    assert len(eseq) > 0
    assert m == len(eseq)
    assert np.array_equal(oseq, np.asarray(eseq).astype(np.int64))
    assert np.array_equal(ovals, evals)


def _prices(rng, n):
    # mostly above the query's threshold of 20, few distinct values: many partials and ties
    return (rng.integers(15, 40, n) + rng.choice([0.0, 0.5, 0.25], n)).astype(np.float32)


_cache = {}


def _seam_stream():
    if "seams" not in _cache:
        n, nk = 130 * TILE + 5, 2000
        ts, k, p, v = synth.stock_stream(n, nk, 100)
        _cache["seams"] = (ts, k, p, v, nk, c2_expected(ts, k, p, v))
    return _cache["seams"]


def _short_stream():
    if "short" not in _cache:
        n, nk = 3 * TILE + 17, 2000
        ts, k, p, v = synth.stock_stream(n, nk, 100)
        seq, _, vals, _ = run_stock_oracle(compiler.compile_app(synth.C2_QUERY), ts, k, p, v)
        _cache["short"] = (ts, k, p, v, nk, (seq, vals))
    return _cache["short"]


def _single_launch(monkeypatch, layout):
    """the seam stream's rows in the single-launch form, once per layout"""
    key = ("seams0", layout)
    if key not in _cache:
        ts, k, p, v, nk, _ = _seam_stream()
        monkeypatch.setenv("SH_BK_SEG", "0")
        out, status, err = _run(synth.C2_QUERY, ts, k, p, v, nk, layout)
        assert status == 1, (status, err)
        _cache[key] = out
    return _cache[key]


@pytest.mark.parametrize("layout", [False, "packed", True])
@pytest.mark.parametrize("seg", [1, 2])
def test_several_segments(monkeypatch, seg, layout):
    """131 tiles, three chunks: three segments of one chunk, or one of two chunks
    and an uneven last one; each segment's first row comes from the carry the scan
    of the segment before left, and both 64-tile prefix seams are crossed"""
    ts, k, p, v, nk, exp = _seam_stream()
    ref = _single_launch(monkeypatch, layout)
    monkeypatch.setenv("SH_BK_SEG", str(seg))
    out, status, err = _run(synth.C2_QUERY, ts, k, p, v, nk, layout)
    print(f"seg={seg} layout={layout}: rows={out[0]} expected={len(exp[0])} bucket_status={status}")
    assert status == 1, (status, err)
    _exact(out, exp)
    assert _same(out, ref)


def test_one_chunk(monkeypatch):
    """nt = 4 with a partial last tile, a single segment: the rows' first positions
    and the step's total (ttot[nt]) come from the carry scan"""
    ts, k, p, v, nk, exp = _short_stream()
    monkeypatch.setenv("SH_BK_SEG", "1")
    out, status, err = _run(synth.C2_QUERY, ts, k, p, v, nk)
    assert status == 1, (status, err)
    _exact(out, exp)


def test_multi_pass_workgroups_in_a_later_segment(monkeypatch):
    """12 % of the events on the four keys of one bucket over 70 tiles (two chunks):
    the dense bucket's workgroup of the second chunk, launched alone with a grid of
    one chunk, takes several passes, whose match-stream regions come from the shared
    tail: the tail must start behind the regions of every chunk of the step, not
    behind those of the launch"""
    n, nk = 70 * TILE + 11, 1024
    rng = np.random.default_rng(41)
    k = rng.integers(0, nk, n).astype(np.int32)
    hot = rng.random(n) < 0.12
    k[hot] = (7 + 256 * rng.integers(0, 4, n))[hot].astype(np.int32)
    ts = (T0 + np.arange(n) // 100).astype(np.int64)
    p = _prices(rng, n)
    v = rng.integers(1, 1000, n).astype(np.int64)
    app = _query("40 milliseconds")
    exp = c2_expected(ts, k, p, v, within=40)
    monkeypatch.setenv("SH_BK_SEG", "0")
    ref, status0, err0 = _run(app, ts, k, p, v, nk)
    monkeypatch.setenv("SH_BK_SEG", "1")
    out, status, err = _run(app, ts, k, p, v, nk)
    print(f"dense 70 tiles: rows={out[0]} expected={len(exp[0])} bucket_status={status} single launch {status0}")
    assert status0 == DENSE_70_STATUS, (status0, err0)
    assert status == DENSE_70_STATUS, (status, err)
    _exact(ref, exp)
    _exact(out, exp)


def test_device_flag_raised_in_the_last_segment(monkeypatch):
    """one key takes 30 % of tile 125: its segment exceeds a pass (SHB_F_SPAN) in
    the third segment's matcher, after the emitters of the first two segments were
    issued (and may have written rows); the run falls back and the rows are exact"""
    n, nk = 130 * TILE + 5, 2048
    rng = np.random.default_rng(44)
    k = rng.integers(0, nk, n).astype(np.int32)
    t125 = np.arange(125 * TILE, 126 * TILE)
    k[t125[rng.random(TILE) < 0.30]] = 5
    ts = (T0 + np.arange(n) // 100).astype(np.int64)
    p = _prices(rng, n)
    v = rng.integers(1, 1000, n).astype(np.int64)
    exp = c2_expected(ts, k, p, v)
    monkeypatch.setenv("SH_BK_SEG", "1")
    out, status, err = _run(synth.C2_QUERY, ts, k, p, v, nk)
    print(f"late flag: rows={out[0]} expected={len(exp[0])} bucket_status={status}")
    assert status == 0, (status, err)
    _exact(out, exp)


def test_handle_reuse(monkeypatch):
    """one runner: the 131-tile stream, the 4-tile stream, the 131-tile stream again
    (the side stream, the events and the carry word are reused)"""
    from siddhi_amd.device_run import DeviceRunner
    ts, k, p, v, nk, exp = _seam_stream()
    sts, sk, sp, sv, snk, sexp = _short_stream()
    monkeypatch.setenv("SH_BK_SEG", "1")
    runner = DeviceRunner(compiler.compile_app(synth.C2_QUERY))
    try:
        first, s1, e1 = _once(runner, ts, k, p, v, nk)
        short, s2, e2 = _once(runner, sts, sk, sp, sv, snk)
        third, s3, e3 = _once(runner, ts, k, p, v, nk)
    finally:
        runner.close()
    assert (s1, s2, s3) == (1, 1, 1), (e1, e2, e3)
    _exact(first, exp)
    _exact(short, sexp)
    assert _same(first, third)


def test_caller_on_a_side_stream(monkeypatch):
    """the caller's stream is not the default one: the pipeline's events order its
    own stream against the caller's"""
    import torch
    ts, k, p, v, nk, exp = _seam_stream()
    monkeypatch.setenv("SH_BK_SEG", "1")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out, status, err = _run(synth.C2_QUERY, ts, k, p, v, nk)
    assert status == 1, (status, err)
    _exact(out, exp)
