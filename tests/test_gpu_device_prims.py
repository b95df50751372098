"""The scan, the radix segment, the pair sort and the tile directory
(siddhi_amd/csrc/sh_kernels.hip, sh_window.hip: shd_exclusive_scan, shd_segment,
shd_segment_payload, shd_sort_pairs, shd_tile_dir) on their own, against the numpy
contracts of tests/device_prims.py, by exact equality, on the null stream, with
every buffer at its stated size plus a guard that must stay untouched:
  * the scan at one, two and three levels, in place and out of place;
  * the segment at 1, 2, 3 and 4 passes, with the null-key sentinel at key counts
    2^k - 1, 2^k and 2^k + 1, on both sides of the 4,096-event seam between the
    one-workgroup kernel and the radix path, with 34 tiles (no multiple of the 8 XCDs);
  * carried payloads of 1, 3 and 8 columns at every pass count (the ping-pong);
  * the arrival-tile-major form the window engine calls, and its tile directory;
  * the pair sort at 0..4 passes, at 16 and 17 tiles (the no-scan form's limit);
  * the environment forms that ship, each in a child process of its own;
  * the window engine on both segment paths with key counts around 2^8 and null keys.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import device_prims as dp
from oracle_engine import run_columns_oracle
from siddhi_amd import compiler, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ scan
@pytest.mark.parametrize("inplace", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("n", dp.SCAN_NS)
def test_exclusive_scan(n, inplace):
    for kind in dp.SCAN_INPUTS:
        dp.check_scan(n, kind, inplace)


# ------------------------------------------------------------------ segment, global order
@pytest.mark.parametrize("nkeys,n", dp.SEG_CASES)
def test_segment(nkeys, n):
    dp.check_segment(nkeys, n)


@pytest.mark.parametrize("nkeys", dp.SEAM_NKEYS)
def test_segment_small_and_radix_paths_agree(nkeys):
    dp.check_seam(nkeys)


@pytest.mark.parametrize("n", [5, dp.SMALL_MAX + 1])
def test_segment_without_keys(n):
    dp.check_no_keys(n)


# ------------------------------------------------------------------ payload
@pytest.mark.parametrize("nkeys,n,widths", dp.PAYLOAD_CASES,
                         ids=[f"{nk}-{n}-{len(w)}cols" for nk, n, w in dp.PAYLOAD_CASES])
def test_segment_payload(nkeys, n, widths):
    dp.check_payload(nkeys, n, widths)


# ------------------------------------------------------------------ tile-major
@pytest.mark.parametrize("shift,nkeys,n", dp.TILED_CASES)
def test_segment_tile_major_and_directory(shift, nkeys, n):
    dp.check_tiled(shift, nkeys, n)


# ------------------------------------------------------------------ pair sort
@pytest.mark.parametrize("bits,n", dp.SORT_CASES)
def test_sort_pairs(bits, n):
    dp.check_sort_pairs(bits, n)


# ------------------------------------------------------------------ environment forms
_child_died = []


@pytest.mark.parametrize("var", sorted(dp.ENV_FORMS))
def test_environment_form_in_a_child(var):
    """each form is read once per process: a fresh child runs its subsets"""
    assert not _child_died, f"an earlier child ended abnormally ({_child_died[0]}): nothing more is started"
    value, subsets = dp.ENV_FORMS[var]
    env = dict(os.environ)
    for v in dp.ENV_FORMS:
        env.pop(v, None)
    env[var] = value
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "device_prims_child.py"), *subsets], env=env,
                           capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _child_died.append(f"{var}={value}: timeout")
        raise
    if r.returncode < 0 or r.returncode > 1:
        _child_died.append(f"{var}={value}: exit status {r.returncode}")
    assert r.returncode == 0, f"{var}={value}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert r.stdout.strip().endswith(f"ok: {len(subsets)} subsets ({' '.join(subsets)})"), r.stdout[-500:]


# ------------------------------------------------------------------ product level
def _null_key_stream(n, nkeys):
    ts, k, p, v = synth.stock_stream(n, nkeys, 100)
    k = k.copy()
    k[np.random.default_rng(nkeys).random(n) < 0.1] = -1
    k[:2] = (nkeys - 1, -1)
    return ts, k, p, v


@pytest.mark.parametrize("nkeys", [255, 256, 257])
def test_window_engine_null_keys_radix_path(nkeys):
    """the window engine over the radix segment: the null-key sentinel needs a bit
    more than the largest key at 256 keys"""
    import torch
    from siddhi_amd.device_run import DeviceRunner
    n = 20_000
    ts, k, p, v = _null_key_stream(n, nkeys)
    seq, _, vals, _ = run_columns_oracle(compiler.compile_app(synth.C2_QUERY), ts, [k, p, v], k)
    runner = DeviceRunner(compiler.compile_app(synth.C2_QUERY))
    dev = torch.device("cuda:0")
    tk = torch.from_numpy(k).to(dev)
    m, oseq, ovals = runner.run(torch.from_numpy(ts).to(dev), tk,
                                [tk, torch.from_numpy(p).to(dev), torch.from_numpy(v).to(dev)], nkeys)
    torch.cuda.synchronize()
    assert runner.bucket_status() == 0
    oseq, ovals = oseq.cpu().numpy(), ovals.cpu().numpy()
    runner.close()
    assert m == len(seq) > 0
    assert np.array_equal(oseq, seq.astype(np.int64))
    assert np.array_equal(ovals, vals)


@pytest.mark.parametrize("nkeys", [255, 256, 257])
def test_push_api_null_keys_small_path(nkeys):
    """send() calls of 1,000 events: the one-workgroup segment under the engine"""
    from siddhi_amd._native import HipEngine
    n, call = 3_000, 1_000
    ts, k, p, v = _null_key_stream(n, nkeys)
    seq, ots, vals, _ = run_columns_oracle(compiler.compile_app(synth.C2_QUERY), ts, [k, p, v], k, batch=call)
    eng = HipEngine(compiler.compile_app(synth.C2_QUERY))
    for b0 in range(0, n, call):
        b1 = b0 + call
        eng.send(0, ts[b0:b1], [k[b0:b1].copy(), p[b0:b1].copy(), v[b0:b1].copy()], [None] * 3, k[b0:b1].copy(), b0)
    got = eng.drain()
    eng.close()
    assert len(got["seq"]) == len(seq) > 0
    assert np.array_equal(got["seq"], seq)
    assert np.array_equal(got["ts"], ots)
    assert np.array_equal(got["values"], vals)
