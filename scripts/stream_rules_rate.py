"""Rate of the streaming rule engine (rule sets beyond the general engine's query
table through sh_push_batch / sh_drain): the C5 distributions, 2M card
transactions over 20k cards and 1,000 rules, pushed from host memory as
send(Event[]) calls of 4,096 and drained every 64 calls; the rows checked against
the vectorised C5 restatement on the same calls; the bulk sh_run_device time for
the same events beside it. One record, no gate.

    python scripts/stream_rules_rate.py [--events N] [--cards K] [--repeats R] [--agg]

--agg: the same rules selecting `sum(e2.amount) as total, avg(e1.amount) as a1`
(running values per (rule, card): the carried, sequential aggregate pass behind
every step). Its rows are checked against the arguments -- the same rules
projecting `e2.amount, e1.amount` through the same calls -- added one at a time
per (rule, card) in doubles on the host. No bulk run beside it: sh_run_device
keeps no state between calls, so it measures another thing.

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
    ap.add_argument("--agg", action="store_true")
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
    plain = "e2.amount as amount"
    text = synth.c5_query(rules)
    assert text.count(plain) == len(rules)
    if a.agg:
        ca_args = compiler.compile_app(text.replace(plain, "e2.amount as total, e1.amount as a1"),
                                       card_strings(a.cards))
        text = text.replace(plain, "sum(e2.amount) as total, avg(e1.amount) as a1")
    ca = compiler.compile_app(text, card_strings(a.cards))
    eseq, erule, evals = c5_expected(ts, card, amount, merchant, rules, batch=a.call)
    calls = [(b0, min(n, b0 + a.call)) for b0 in range(0, n, a.call)]

    def running(args):
        """sum / avg of the arguments' rows, one double addition per row and (rule, card)"""
        tot = np.zeros(len(eseq), np.float64)
        avg = np.zeros(len(eseq), np.float64)
        x2 = (args["values"][:, 1] & 0xFFFFFFFF).astype(np.uint32).view(np.float32).astype(np.float64)
        x1 = (args["values"][:, 2] & 0xFFFFFFFF).astype(np.uint32).view(np.float32).astype(np.float64)
        state = {}
        for i, k in enumerate(zip(erule.tolist(), card[eseq].tolist())):
            s2, s1, c = state.get(k, (0.0, 0.0, 0))
            s2, s1, c = s2 + float(x2[i]), s1 + float(x1[i]), c + 1
            state[k] = (s2, s1, c)
            tot[i], avg[i] = s2, s1 / c
        return tot.view(np.int64), avg.view(np.int64), len(state)

    def one_pass(check, app=None):
        eng = HipEngine(app or ca)
        eng.start()
        parts, paths, dev_ms = [], [], 0.0
        steps_ms = []
        ent = C.c_int64(0)
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
                steps_ms.append(kt.total_ms)
                peak_p, peak_r = max(peak_p, p.value), max(peak_r, r.value)
        dt = time.perf_counter() - t0
        lib().shx_rules_agg_carry(eng.h, C.byref(ent))
        table = (ent.value, lib().shx_rules_agg_capacity(eng.h), lib().shx_agg_status(eng.h))
        out = None
        if check:
            out = abi.concat_drains(parts)
            assert len(out["seq"]) == len(eseq) > 0, (len(out["seq"]), len(eseq))
            assert np.array_equal(out["seq"].astype(np.int64), eseq)
            assert np.array_equal(out["query"], erule)
            if not a.agg:
                assert np.array_equal(out["values"][:, :2], evals)
        eng.close()
        return dt, dev_ms, paths, peak_p, peak_r, steps_ms, table, out

    if a.agg:
        # the arguments through the same calls (projection only), then the aggregating app
        args = one_pass(check=True, app=ca_args)[7]
        assert np.array_equal(args["values"][:, :2], evals)
        tot, avg, nseg = running(args)
        got = one_pass(check=True)
        assert np.array_equal(got[7]["values"][:, 0], evals[:, 0])
        assert np.array_equal(got[7]["values"][:, 1], tot), "running sums"
        assert np.array_equal(got[7]["values"][:, 2], avg), "running averages"
        assert got[6][0] == nseg and got[6][2] == 6, (got[6], nseg)
    else:
        one_pass(check=True)  # warm-up: code objects, buffers' first growth; the rows checked
    runs = [one_pass(check=False) for _ in range(a.repeats)]
    dts = [r[0] for r in runs]
    med = statistics.median(dts)
    dev = statistics.median(r[1] for r in runs)
    _, _, paths, peak_p, peak_r, steps_ms, table, _ = runs[-1]
    head = (f"stream_rules_rate{' --agg' if a.agg else ''}: {n} events, {a.cards} cards, {len(rules)} rules, "
            f"calls of {a.call}, drain every {a.drain_every} calls, {len(eseq)} rows ")
    if a.agg:
        print(head + "(checked against the arguments added in sequence on the host)")
        print(f"  streamed, host memory -> rows on the host: median {med * 1e3:.1f} ms of {a.repeats} passes "
              f"(min {min(dts) * 1e3:.1f}, max {max(dts) * 1e3:.1f}) = {n / med / 1e6:.2f} M events/s")
        print(f"  steps {len(paths)}, device time per step (last pass, ms): "
              f"{' '.join(f'{x:.2f}' for x in steps_ms)}")
        print(f"  device part (HIP events around each step, summed): median {dev:.1f} ms; "
              f"host staging, PCIe and read-backs: {med * 1e3 - dev:.1f} ms")
        print(f"  peak carried rows {peak_r}, peak carried partials {peak_p}")
        print(f"  carried aggregates: {table[0]} (rule, card) entries in a table of {table[1]}, agg status {table[2]}")
        return

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
    print(f"  device time per step (last pass, ms): {' '.join(f'{x:.2f}' for x in steps_ms)}")
    print(f"  device part (HIP events around each step, summed): median {dev:.1f} ms; "
          f"host staging, PCIe and read-backs: {med * 1e3 - dev:.1f} ms")
    print(f"  peak carried rows {peak_r}, peak carried partials {peak_p}")
    print(f"  bulk sh_run_device, events in HBM ({bulk_path}): median {statistics.median(bulk) * 1e3:.1f} ms "
          f"host clock, {bulk_dev:.1f} ms device")


if __name__ == "__main__":
    main()
