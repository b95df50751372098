"""Rate of an output-only `having` and of `output first|all every N events` on the
rise-and-fall sequence (C3) in bulk runs: the row post-filter stage behind k_s3b, beside
the general engine whose selector applied them before.

    python scripts/seq3_post_rate.py [--events N] [--keys K] [--repeats R]

C3 over N stock events (K symbols, 1,000 events/ms) through sh_run_device with the events
in HBM, four variants: no clause, `having p3 < 30.0` (about half of the rows), `output
first every 3 events` and `output all every 3 events`. Each variant with a clause is
compiled twice in this process: as it lowers now (the rise-and-fall rungs with the stage
behind them) and under its switch SH_NO_HAVING_FILTER=1 / SH_NO_RATE_FILTER=1 (read at
compile time: the app lowers as before the stage took it, k_nfa_run and its selector).
All runners run in alternation in one job.

Every timed pass follows one untimed warm-up; medians with min and max of R passes.
Reported per variant: the general engine's time, the new path's time, and the new path's
overhead over the clause-free run. One record, no gate."""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from rate_limit_rate import spread  # noqa: E402  (sets the package's path up)

VARIANTS = [("having p3 < 30.0", "SH_NO_HAVING_FILTER"), ("output first every 3 events", "SH_NO_RATE_FILTER"),
            ("output all every 3 events", "SH_NO_RATE_FILTER")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10_000_000)
    ap.add_argument("--keys", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no rate"
    from siddhi_amd import compiler, synth
    from siddhi_amd.device_run import DeviceRunner
    ts, k, p, v = synth.stock_stream(a.events, a.keys, 1000, config_index=3)
    dev = torch.device("cuda:0")
    tts, tk = torch.from_numpy(ts).to(dev), torch.from_numpy(k).to(dev)
    cols = [tk, torch.from_numpy(p).to(dev), torch.from_numpy(v).to(dev)]
    runners = [("no clause", None, DeviceRunner(compiler.compile_app(synth.C3_QUERY)))]
    for clause, switch in VARIANTS:
        text = synth.C3_QUERY.replace(" insert into Out;", f" {clause} insert into Out;")
        runners.append((clause, None, DeviceRunner(compiler.compile_app(text))))
        os.environ[switch] = "1"
        try:
            runners.append((clause, switch, DeviceRunner(compiler.compile_app(text))))
        finally:
            del os.environ[switch]
    times = [[] for _ in runners]
    last = [None] * len(runners)
    for i in range(a.repeats + 1):
        for j, (clause, switch, r) in enumerate(runners):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = r.run(tts, tk, cols, a.keys)[0]
            torch.cuda.synchronize()
            if i:
                times[j].append(time.perf_counter() - t0)
            last[j] = dict(m=m, seq3=r.seq3_status(), having=r.having_status(), rate=r.rate_status(),
                           having_rows=r.having_rows(), rate_rows=r.rate_rows(), having_ms=r.having_ms(),
                           rate_ms=r.rate_ms())
    for _, _, r in runners:
        r.close()
    base = statistics.median(times[0])
    print(f"seq3_post_rate: C3, {a.events} events, {a.keys} keys: {last[0]['m']} rows without a clause "
          f"(seq3 status {last[0]['seq3']})")
    print(f"  sh_run_device without a clause: {spread(times[0])}")
    for j in range(1, len(runners), 2):
        clause = runners[j][0]
        new, old = last[j], last[j + 1]
        assert new["m"] == old["m"], (clause, new, old)
        assert new["seq3"] in (1, 2) and (new["having"] or new["rate"]) == 1, new
        assert old["seq3"] == 0 and old["having"] == 0 and old["rate"] == 0, old
        tn, to = statistics.median(times[j]), statistics.median(times[j + 1])
        pass_ms = new["having_ms"] + new["rate_ms"]
        print(f"  `{clause}`: {new['m']} rows kept")
        print(f"    general engine ({runners[j + 1][1]}=1, seq3 status {old['seq3']}): {spread(times[j + 1])}")
        print(f"    fast engine and the stage (seq3 status {new['seq3']}):            {spread(times[j])}")
        print(f"    overhead over the clause-free run: {(tn - base) * 1e3:.2f} ms (the stage's launches alone, HIP "
              f"events: {pass_ms:.3f} ms); new path vs general engine: {to / tn:.1f}x "
              + ("faster" if to > tn else "-- NOT faster"))


if __name__ == "__main__":
    main()
