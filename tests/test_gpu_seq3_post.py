"""`having` and `output first|last|all every N events` on the rise-and-fall sequence
through sh_run_device, exact against the oracle: the bucket-carry engine (k_s3b, seq3
status 2) and the key-segment engine (k_seq3s, status 1) with the row post-filter stage
behind them in every row layout, the general engine's selector under SH_NO_SEQ3 (the
rows copied as they are: a clause applied twice would leave too few), aggregating selects
whose `having` reads the finished running value (in the kernel's lanes, by the post-pass,
and by the general engine's second pass when the additions round), and the capacity rule.
The cases, streams and oracle rows are tests/seq3_post_cases.py's."""
import ctypes as C

import numpy as np
import pytest

import seq3_post_cases as sc
from siddhi_amd import abi, compiler

pytestmark = pytest.mark.gpu

LAYOUTS = ("raw", "packed", "columns")


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_dev = {}


def device_stream(which):
    """a stream's columns on the device, uploaded once"""
    import torch
    if which not in _dev:
        dev = torch.device("cuda:0")
        ts, k, p, v = sc.data_of(which)
        tk = torch.from_numpy(np.ascontiguousarray(k)).to(dev)
        _dev[which] = (torch.from_numpy(np.ascontiguousarray(ts)).to(dev), tk,
                       [tk, torch.from_numpy(np.ascontiguousarray(p)).to(dev),
                        torch.from_numpy(np.ascontiguousarray(v)).to(dev)])
    return _dev[which]


def n_keys(which):
    return which[1] if isinstance(which, tuple) else sc.K_S3B if which == "tie" else which


def run(runner, which, layout="raw"):
    """(m, seq, raw rows) of one sh_run_device call, and the statuses"""
    import torch
    from siddhi_amd.device_run import columns_to_raw, packed_to_raw
    ts, tk, cols = device_stream(which)
    res = runner.run(ts, tk, cols, n_keys(which), packed=layout == "packed", columns=layout == "columns")
    torch.cuda.synchronize()
    if layout == "packed":
        offs, rb = runner.packed_layout()
        seq, vals = packed_to_raw(res[1].cpu().numpy(), runner.out_types, offs, rb)
        seq = seq.astype(np.int64)
    elif layout == "columns":
        seq, vals = res[1].cpu().numpy(), columns_to_raw([c.cpu().numpy() for c in res[2]], runner.out_types)
    else:
        seq, vals = res[1].cpu().numpy(), res[2].cpu().numpy()
    st = dict(seq3=runner.seq3_status(), agg=runner.agg_status(), having=runner.having_status(),
              rate=runner.rate_status(), having_rows=runner.having_rows(), rate_rows=runner.rate_rows())
    return (res[0], seq, vals), st


def runner_of(text):
    from siddhi_amd.device_run import DeviceRunner
    return DeviceRunner(compiler.compile_app(text))


def assert_rows(got, ref, what):
    m, seq, vals = got
    assert m == len(ref["seq"]) > 0, (what, m, len(ref["seq"]))
    assert np.array_equal(seq[:m], ref["seq"].astype(np.int64)), what
    assert np.array_equal(vals[:m], ref["values"]), what


def assert_stage(st, case, which, what):
    """the stage's passes ran, on the oracle's counts"""
    n0, n1, n2 = sc.counts(case, which)
    assert st["having"] == (1 if case[1] else 0), (what, st)
    assert st["rate"] == (1 if case[2] else 0), (what, st)
    assert st["having_rows"] == ((n0, n1) if case[1] else (0, 0)), (what, st)
    assert st["rate_rows"] == ((n1, n2) if case[2] else (0, 0)), (what, st)


def fast_status(case, which):
    return 2 if n_keys(which) >= 1024 and sc.one_attribute(case) else 1


@pytest.mark.parametrize("name", list(sc.CASES))
def test_fast_engines_every_layout_vs_oracle(name):
    case = sc.CASES[name]
    r = runner_of(sc.text_of(case))
    try:
        for K in sc.KS:
            ref = sc.oracle_rows(sc.text_of(case), K)
            for layout in LAYOUTS:
                what = (name, K, layout)
                got, st = run(r, K, layout)
                print(what, st)
                assert_rows(got, ref, what)
                assert st["seq3"] == fast_status(case, K), (what, st)
                assert_stage(st, case, K, what)
                if name in sc.AGGREGATING:
                    assert st["agg"] == {"sum": 3, "max": 1}[sc.AGGREGATING[name]], (what, st)
    finally:
        r.close()


@pytest.mark.parametrize("name", list(sc.CASES))
def test_key_segment_engine_at_bucket_sizes_vs_oracle(name, monkeypatch):
    """SH_DISABLE_S3B=1: k_seq3s at the key count the bucket-carry engine would take"""
    monkeypatch.setenv("SH_DISABLE_S3B", "1")
    case = sc.CASES[name]
    r = runner_of(sc.text_of(case))
    try:
        for layout in LAYOUTS:
            got, st = run(r, sc.K_S3B, layout)
            assert_rows(got, sc.oracle_rows(sc.text_of(case), sc.K_S3B), (name, layout))
            assert st["seq3"] == 1, (layout, st)
            assert_stage(st, case, sc.K_S3B, (name, layout))
            if name in sc.AGGREGATING:
                assert st["agg"] == {"sum": 3, "max": 1}[sc.AGGREGATING[name]], (layout, st)
    finally:
        r.close()


@pytest.mark.parametrize("name,which", [(n, K) for n in sc.CASES for K in sc.KS] + [(n, "tie") for n in sc.TIE_CASES])
def test_general_engine_rows_are_copied_as_they_are(name, which, monkeypatch):
    """SH_NO_SEQ3=1 on the handle that has the stage: k_nfa_run's selector applies the
    clause, and the stage must not apply it again (status 0, the passes did not run)"""
    monkeypatch.setenv("SH_NO_SEQ3", "1")
    case = sc.CASES.get(name) or sc.TIE_CASES[name]
    r = runner_of(sc.text_of(case))
    try:
        got, st = run(r, which)
        assert_rows(got, sc.oracle_rows(sc.text_of(case), which), (name, which))
        assert st["seq3"] == 0 and st["having"] == 0 and st["rate"] == 0, st
        assert st["having_rows"] == (0, 0) and st["rate_rows"] == (0, 0), st
    finally:
        r.close()


@pytest.mark.parametrize("name", list(sc.TIE_CASES))
def test_equal_prices_vs_oracle(name):
    """the stream with five distinct prices: the fast engines keep it (as
    tests/test_gpu_c3.py pins for the clause-free app), the stage behind them"""
    case = sc.TIE_CASES[name]
    r = runner_of(sc.text_of(case))
    try:
        for layout in ("raw", "packed"):
            got, st = run(r, "tie", layout)
            print(name, layout, st)
            assert_rows(got, sc.oracle_rows(sc.text_of(case), "tie"), (name, layout))
            assert st["seq3"] == 2, st
            assert_stage(st, case, "tie", (name, layout))
    finally:
        r.close()


@pytest.mark.parametrize("K", sc.KS)
def test_rounding_sums_take_the_general_engine_second_pass(K, monkeypatch):
    """sums of the rounding prices formed by the post-pass are not exact: the second pass
    runs on k_nfa_run, whose selector filters (agg status 2; those rows are not filtered
    again). In the kernel's lanes (status 3) the additions are the reference's own"""
    case = sc.CASES["sum_having"]
    which = ("r", K)
    ref = sc.oracle_rows(sc.text_of(case), which)
    n0 = len(sc.oracle_rows(case[0], which)["seq"])
    assert 0 < len(ref["seq"]) < n0
    r = runner_of(sc.text_of(case))
    try:
        got, st = run(r, which)
        assert_rows(got, ref, ("lanes", K))
        assert (st["seq3"], st["agg"], st["having"]) == (1, 3, 1), st
        assert st["having_rows"] == (n0, len(ref["seq"])), st
        monkeypatch.setenv("SH_S3_AGG_POST", "1")
        got, st = run(r, which)
        assert_rows(got, ref, ("post", K))
        assert (st["seq3"], st["agg"], st["having"]) == (0, 2, 0), st
    finally:
        r.close()


def _raw_call(runner, which, capacity):
    """one sh_run_device_v2 call with raw rows of `capacity`: (rc, out_count, seq, rows)"""
    import torch
    from siddhi_amd._native import lib
    dev = torch.device("cuda:0")
    ts, tk, cols = device_stream(which)
    seq = torch.zeros(capacity, dtype=torch.int64, device=dev)
    vals = torch.zeros(capacity * runner.n_out, dtype=torch.int64, device=dev)
    r = abi.sh_device_run()
    r.version = abi.SH_DEVICE_RUN_V2
    r.n = ts.numel()
    r.d_ts = ts.data_ptr()
    r.d_keys = tk.data_ptr()
    r.n_keys = n_keys(which)
    r.batch_events = 4096
    r.d_cols = (C.c_void_p * len(cols))(*[c.data_ptr() for c in cols])
    r.out_capacity = capacity
    r.d_out_seq = seq.data_ptr()
    r.d_out_values = vals.data_ptr()
    r.stream = torch.cuda.current_stream(dev).cuda_stream
    torch.cuda.synchronize()
    rc = lib().sh_run_device_v2(runner.handle.h, C.byref(r))
    torch.cuda.synchronize()
    return rc, int(r.out_count), seq.cpu().numpy(), vals.cpu().numpy().reshape(capacity, runner.n_out)


@pytest.mark.parametrize("name", ["having_p3", "first3", "all3"])
@pytest.mark.parametrize("K", sc.KS)
def test_capacity_is_the_unfiltered_count(name, K):
    """the engine's rows must fit: one row short of the unfiltered count is refused as
    without the clause, a capacity that fits only the kept rows too; and two runs on one
    handle give the same rows (every call starts every counter at zero)"""
    case = sc.CASES[name]
    n0, n1, n2 = sc.counts(case, K)
    assert n2 < n0 - 1
    ref = sc.oracle_rows(sc.text_of(case), K)
    plain = runner_of(case[0])
    r = runner_of(sc.text_of(case))
    try:
        want = _raw_call(plain, K, n0 - 1)[:2]
        assert want == (abi.SH_E_MORE, n0)
        assert _raw_call(r, K, n0 - 1)[:2] == want
        assert _raw_call(r, K, n2)[:2] == want
        for again in range(2):
            rc, m, seq, vals = _raw_call(r, K, n0)
            assert (rc, m) == (abi.SH_OK, n2), r.last_error()
            assert_rows((m, seq, vals), ref, (name, K, again))
            assert r.seq3_status() == fast_status(case, K)
    finally:
        plain.close()
        r.close()
