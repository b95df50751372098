"""The bucketed emitter compiled per (select list, output layout) on the GPU, against
the oracle's rows of the burst stream at 1,024 keys (tests/emit_cases.py), with the
runner, the guard rows and the bit-for-bit asserts of tests/test_gpu_emit.py.

By default every list of at most 8 values runs the kernel hipRTC compiled for it
(shx_bucket_emit_status 1, bucket status 1: a silent fallback to the generic k_bk_emit
fails here); `SH_BK_EMIT_SPEC=0`, read per call, runs the generic kernel; lists of 9
and 16 values always do. Capacity cuts inside a dense and inside a row-parallel half,
and a step cut into three pipelined segments, run under the specialised kernel."""
import numpy as np
import pytest

import emit_cases as ec
from siddhi_amd import abi
from test_gpu_emit import Runner, _cut_rows, _device, assert_guard, assert_rows  # noqa: F401 (_device: autouse)

pytestmark = pytest.mark.gpu

NK = 1024
SPEC = [n for n, v in ec.CASES.items() if len(v) <= 8]
GENERIC_ONLY = [n for n, v in ec.CASES.items() if len(v) > 8]


def _emit_status(r):
    return r.lib.shx_bucket_emit_status(r.handle.h)


def _check(name, layout, want_emit):
    values = ec.CASES[name]
    seq, raw = ec.expected_raw(NK, values)
    types = ec.types_of(values)
    what = f"{name} {layout} emitter {want_emit}"
    r = Runner(values, NK)
    try:
        rc, count, out = r.run(layout, len(seq))
        st, es = r.bucket_status(), _emit_status(r)
        print(f"{what}: rc={rc} rows={count} bucket_status={st} emit_status={es} err={r.error()!r}")
        assert rc == abi.SH_OK, r.error()
        assert st == 1, (what, st, r.error())
        assert es == want_emit, (what, es, r.error())
        assert count == len(seq) > 0
        assert_rows(out, layout, types, seq, raw, what)
        assert_guard(out, layout, types, len(seq), what)
    finally:
        r.close()


@pytest.mark.parametrize("layout", ec.LAYOUTS)
@pytest.mark.parametrize("name", SPEC)
def test_specialised_emitter_rows(monkeypatch, name, layout):
    monkeypatch.delenv("SH_BK_EMIT_SPEC", raising=False)
    _check(name, layout, 1)


@pytest.mark.parametrize("layout", ec.LAYOUTS)
@pytest.mark.parametrize("name", SPEC)
def test_generic_emitter_on_request(monkeypatch, name, layout):
    monkeypatch.setenv("SH_BK_EMIT_SPEC", "0")
    _check(name, layout, 0)


@pytest.mark.parametrize("layout", ec.LAYOUTS)
@pytest.mark.parametrize("name", GENERIC_ONLY)
def test_longer_lists_run_the_generic_emitter(monkeypatch, name, layout):
    monkeypatch.delenv("SH_BK_EMIT_SPEC", raising=False)
    _check(name, layout, 0)


@pytest.mark.parametrize("where", ["dense", "row_parallel"])
@pytest.mark.parametrize("layout", ec.LAYOUTS)
@pytest.mark.parametrize("name", ["w2_int_long", "w8_all_wide"])      # 6 waves / 4 waves in every layout
def test_capacity_cut_under_the_specialised_emitter(monkeypatch, name, layout, where):
    """out_capacity inside a half the emitter writes event-parallel (dense) or
    row-parallel: SH_E_MORE, the whole total in out_count, no byte past the capacity"""
    monkeypatch.delenv("SH_BK_EMIT_SPEC", raising=False)
    values = ec.CASES[name]
    seq, raw = ec.expected_raw(NK, values)
    types = ec.types_of(values)
    cap = _cut_rows(NK)[where]
    what = f"spec capacity {name} {layout} {where} cut at row {cap} of {len(seq)}"
    r = Runner(values, NK)
    try:
        guard = len(seq) - cap + 64
        rc, count, out = r.run(layout, cap, guard=guard)
        es = _emit_status(r)
        print(f"{what}: rc={rc} out_count={count} emit_status={es}")
        assert rc == abi.SH_E_MORE, (what, rc, r.error())
        assert es == 1, (what, es, r.error())
        assert count == len(seq)
        assert_guard(out, layout, types, cap, what, guard=guard)
        rc, count, out = r.run(layout, len(seq))
        assert rc == abi.SH_OK, r.error()
        assert r.bucket_status() == 1 and _emit_status(r) == 1
        assert_rows(out, layout, types, seq, raw, what)
        assert_guard(out, layout, types, len(seq), what)
    finally:
        r.close()


@pytest.mark.parametrize("layout", [False, "packed", True])
def test_three_pipelined_segments(monkeypatch, layout):
    """the burst stream is one matcher chunk, so a step of three segments needs the
    131-tile stream of tests/test_gpu_bucket_pipeline.py (three chunks, SH_BK_SEG=1):
    every segment's emitter is the specialised kernel on the side stream, and the rows
    equal the C2 restatement's and the generic kernel's on the same arrays"""
    import test_gpu_bucket_pipeline as bp
    from siddhi_amd import compiler, synth
    from siddhi_amd.device_run import DeviceRunner
    ts, k, p, v, nk, exp = bp._seam_stream()
    assert (len(ts) + bp.TILE - 1) // bp.TILE > 2 * 60          # three chunks of 60 tiles
    monkeypatch.setenv("SH_BK_SEG", "1")
    runner = DeviceRunner(compiler.compile_app(synth.C2_QUERY))
    try:
        monkeypatch.delenv("SH_BK_EMIT_SPEC", raising=False)
        out, status, err = bp._once(runner, ts, k, p, v, nk, layout)
        assert status == 1 and runner.bucket_emit_status() == 1, (status, runner.bucket_emit_status(), err)
        bp._exact(out, exp)
        monkeypatch.setenv("SH_BK_EMIT_SPEC", "0")
        ref, status, err = bp._once(runner, ts, k, p, v, nk, layout)
        assert status == 1 and runner.bucket_emit_status() == 0, (status, runner.bucket_emit_status(), err)
        assert bp._same(out, ref)
    finally:
        runner.close()
