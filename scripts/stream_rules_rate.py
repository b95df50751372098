"""Rate of the streaming rule engine (rule sets beyond the general engine's query
table through sh_push_batch / sh_drain): the C5 distributions, 2M card
transactions over 20k cards and 1,000 rules, pushed from host memory as
send(Event[]) calls of 4,096 and drained every 64 calls; the rows checked against
the vectorised C5 restatement on the same calls; the bulk sh_run_device time for
the same events beside it. One record, no gate.

    python scripts/stream_rules_rate.py [--events N] [--cards K] [--repeats R]

Each timed pass runs on a fresh handle (the state starts empty) after one untimed
warm-up pass over the whole stream; a pass ends in the last drain's stream
synchronise, the bulk run in torch.cuda.synchronize()."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=2_000_000)
    ap.add_argument("--cards", type=int, default=20_000)
    ap.add_argument("--call", type=int, default=4096)
    ap.add_argument("--drain-every", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()

    import torch
    from c5_check import c5_expected
    from rules_cases import card_strings
    from siddhi_amd import abi, compiler, synth
    from siddhi_amd._native import HipEngine, lib
    from siddhi_amd.device_run import DeviceRunner

    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no rate"
    n = a.events
    ts, card, amount, merchant = synth.txn_stream(n, a.cards, 100)
    rules = synth.c5_rules()
    ca = compiler.compile_app(synth.c5_query(rules), card_strings(a.cards))
    eseq, erule, evals = c5_expected(ts, card, amount, merchant, rules, batch=a.call)
    calls = [(b0, min(n, b0 + a.call)) for b0 in range(0, n, a.call)]

    def one_pass(check):
        eng = HipEngine(ca)
        eng.start()
        parts, paths, dev_ms = [], [], 0.0
        peak_p = peak_r = 0
        p, r = C.c_int64(0), C.c_int64(0)
        kt = abi.sh_kernel_times()
        t0 = time.perf_counter()
        for i, (b0, b1) in enumerate(calls):
            eng.send(0, ts[b0:b1], [card[b0:b1], amount[b0:b1], merchant[b0:b1]], [None] * 3, card[b0:b1], b0)
            if (i + 1) % a.drain_every == 0 or i + 1 == len(calls):
                parts.append(eng.drain())  # (ends in the step's stream synchronise)
                lib().shx_rules_carry(eng.h, C.byref(p), C.byref(r))
                lib().sh_last_kernel_times(eng.h, C.byref(kt))
                paths.append("sparse" if lib().shx_rules_status(eng.h) else "key-segment")
                dev_ms += kt.total_ms
                peak_p, peak_r = max(peak_p, p.value), max(peak_r, r.value)
        dt = time.perf_counter() - t0
        eng.close()
        if check:
            out = abi.concat_drains(parts)
            assert len(out["seq"]) == len(eseq) > 0, (len(out["seq"]), len(eseq))
            assert np.array_equal(out["seq"].astype(np.int64), eseq)
            assert np.array_equal(out["query"], erule)
            assert np.array_equal(out["values"][:, :2], evals)
        return dt, dev_ms, paths, peak_p, peak_r

    one_pass(check=True)  # warm-up: code objects, buffers' first growth; the rows checked
    runs = [one_pass(check=False) for _ in range(a.repeats)]
    dts = [r[0] for r in runs]
    med = statistics.median(dts)
    dev = statistics.median(r[1] for r in runs)
    _, _, paths, peak_p, peak_r = runs[-1]

    # the bulk path over the same events, already in HBM
    dvc = torch.device("cuda:0")
    tts = torch.from_numpy(ts).to(dvc)
    cols = [torch.from_numpy(c).to(dvc) for c in (card, amount, merchant)]
    runner = DeviceRunner(ca)
    bulk = []
    for i in range(a.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m, seq, vals, q = runner.run(tts, cols[0], cols, a.cards, batch_events=a.call, with_query=True)
        torch.cuda.synchronize()
        if i:
            bulk.append(time.perf_counter() - t0)
    assert m == len(eseq) and np.array_equal(seq.cpu().numpy(), eseq)
    bulk_path = "sparse" if runner.rules_status() else "key-segment"
    bulk_dev = runner.kernel_times()["total_ms"]
    runner.close()

    print(f"stream_rules_rate: {n} events, {a.cards} cards, {len(rules)} rules, calls of {a.call}, "
          f"drain every {a.drain_every} calls, {len(eseq)} rows (checked against c5_expected)")
    print(f"  streamed, host memory -> rows on the host: median {med * 1e3:.1f} ms of {a.repeats} passes "
          f"(min {min(dts) * 1e3:.1f}, max {max(dts) * 1e3:.1f}) = {n / med / 1e6:.2f} M events/s")
    print(f"  steps {len(paths)}, paths {','.join(paths)}")
    print(f"  device part (HIP events around each step, summed): median {dev:.1f} ms; "
          f"host staging, PCIe and read-backs: {med * 1e3 - dev:.1f} ms")
    print(f"  peak carried rows {peak_r}, peak carried partials {peak_p}")
    print(f"  bulk sh_run_device, events in HBM ({bulk_path}): median {statistics.median(bulk) * 1e3:.1f} ms "
          f"host clock, {bulk_dev:.1f} ms device")


if __name__ == "__main__":
    main()
