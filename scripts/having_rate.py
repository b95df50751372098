"""Rate of an output-only `having` on the fast engines (the device row filter of
sh_having.hip behind them), beside the general engine that applied it before.

    python scripts/having_rate.py [--events N] [--keys K] [--repeats R] [--stream-events M]

1. C2 bulk: the C2 shape over N stock events (K symbols, 100 events/ms) with a
   `having` that keeps about half the rows, through sh_run_device with the events in
   HBM. Reported: the call's host-clock time, the filter's share (the same app
   without the clause, same job, alternating runs), and the bytes the filter moves by
   construction -- rows in (values, sequence numbers), rows out, ballot words and tile
   counts -- as a fraction of 8 TB/s over the filter's share.
2. The comparison: the same app with SH_NO_HAVING_FILTER=1, which compiles it as
   before this filter existed (the general engine's selector applies `having`), in a
   child process of the same job (the variable is read at compile time).
3. H6-shaped streaming: 64 rules, `amount / (m - c) > 20.0`, M card transactions in
   calls of 4,096 drained every 64 calls, in events per second, beside the same set
   without the clause.

Every timed pass follows one untimed warm-up; medians with min and max of R passes.
One record, no gate."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

CLAUSE = "p2 - p1 > 0.19"
HBM_BYTES_PER_S = 8e12


def c2_texts():
    from siddhi_amd import synth
    return synth.C2_QUERY, synth.C2_QUERY.replace(" insert into Out;", f" having {CLAUSE} insert into Out;")


def spread(x):
    return f"median {statistics.median(x) * 1e3:.2f} ms (min {min(x) * 1e3:.2f}, max {max(x) * 1e3:.2f}, n={len(x)})"


def bulk(a, texts):
    """alternating timed runs of each text on its own runner; [(times, m, statuses)]"""
    import torch
    from siddhi_amd import compiler, synth
    from siddhi_amd.device_run import DeviceRunner
    ts, k, p, v = synth.stock_stream(a.events, a.keys, 100)
    dev = torch.device("cuda:0")
    tts, tk = torch.from_numpy(ts).to(dev), torch.from_numpy(k).to(dev)
    cols = [tk, torch.from_numpy(p).to(dev), torch.from_numpy(v).to(dev)]
    runners = [DeviceRunner(compiler.compile_app(t)) for t in texts]
    times = [[] for _ in texts]
    ms = [0] * len(texts)
    for i in range(a.repeats + 1):
        for j, r in enumerate(runners):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ms[j] = r.run(tts, tk, cols, a.keys)[0]
            torch.cuda.synchronize()
            if i:
                times[j].append(time.perf_counter() - t0)
    out = [(times[j], ms[j], dict(bucket=r.bucket_status(), having=r.having_status(), rows=r.having_rows(),
                                  filter_ms=r.having_ms()))
           for j, r in enumerate(runners)]
    for r in runners:
        r.close()
    return out


def child(a):
    """the comparison arm: prints one line"""
    plain, having = c2_texts()
    (t, m, st), = bulk(a, [having])
    print(f"CHILD {m} {st['having']} {st['bucket']} " + " ".join(f"{x:.6f}" for x in t))


def stream(a, with_clause):
    from rules_cases import card_strings
    from siddhi_amd import compiler, synth
    from siddhi_amd._native import HipEngine
    n, cards, call, every = a.stream_events, 20_000, 4096, 64
    ts, card, amount, merchant = synth.txn_stream(n, cards, 100, n_merchants=12, seed=44)
    rules = synth.c5_rules(64, seed=44, amount=(10.0, 150.0), merchants=12, factor=(0.6, 1.6), within=(1, 40))
    text = synth.c5_query(rules, unit="milliseconds").replace("e2.amount as amount",
                                                              "e2.amount as amount, e2.merchant as m")
    if with_clause:
        parts = text.split(" insert into Alerts;")
        text = "".join(q + f" having amount / (m - {r % 12}) > 20.0 insert into Alerts;"
                       for r, q in enumerate(parts[:-1])) + parts[-1]
    ca = compiler.compile_app(text, card_strings(cards))
    times, rows = [], 0
    for i in range(a.repeats + 1):
        eng = HipEngine(ca)
        eng.start()
        rows = 0
        t0 = time.perf_counter()
        for c, b0 in enumerate(range(0, n, call)):
            b1 = min(n, b0 + call)
            eng.send(0, ts[b0:b1], [card[b0:b1], amount[b0:b1], merchant[b0:b1]], [None] * 3, card[b0:b1], b0)
            if (c + 1) % every == 0 or b1 == n:
                rows += len(eng.drain()["seq"])
        if i:
            times.append(time.perf_counter() - t0)
        eng.close()
    return times, rows, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10_000_000)
    ap.add_argument("--keys", type=int, default=10_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--stream-events", type=int, default=1_000_000)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no rate"
    if a.child:
        return child(a)
    plain, having = c2_texts()
    (tp, mp, sp), (th, mh, sh) = bulk(a, [plain, having])
    assert sh["having"] == 1 and sh["rows"] == (mp, mh), (sh, mp, mh)
    n_out = 4
    words_in = mp * (n_out + 1) * 8
    words_out = mh * (n_out + 1) * 8
    tiles = (mp + 255) // 256
    side = tiles * 4 * 8 * 2 + tiles * 4 * 4          # ballots written and read, counts and offsets
    moved = words_in + mp * 8 + words_out + side      # the mark reads the compared columns' lines again
    share = statistics.median(th) - statistics.median(tp)
    print(f"having_rate: C2, {a.events} events, {a.keys} keys, having `{CLAUSE}`: {mp} rows in, {mh} kept "
          f"({mh / max(1, mp):.2f}); bucketed engine {sh['bucket']}, device row filter {sh['having']}")
    print(f"  sh_run_device without the clause: {spread(tp)}")
    print(f"  sh_run_device with the clause:    {spread(th)}")
    print(f"  the clause's share of the call (difference of the medians: mark, scan, move, one 8-byte read-back and "
          f"its synchronise): {share * 1e3:.2f} ms; the filter's three launches alone (HIP events, last run): "
          f"{sh['filter_ms']:.3f} ms")
    share = sh["filter_ms"] / 1e3 if sh["filter_ms"] > 0 else share
    print(f"  bytes the filter moves by construction: {moved / 1e6:.1f} MB (rows in {words_in / 1e6:.1f}, mark "
          f"re-read {mp * 8 / 1e6:.1f}, rows out {words_out / 1e6:.1f}, ballots and tile counts {side / 1e6:.2f})"
          f" = {moved / max(share, 1e-9) / HBM_BYTES_PER_S * 100:.1f}% of 8 TB/s over the launches' time")
    env = dict(os.environ, SH_NO_HAVING_FILTER="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--events", str(a.events), "--keys",
                        str(a.keys), "--repeats", str(min(3, a.repeats))], env=env, capture_output=True, text=True)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
    if r.returncode or not line:
        print(f"  general engine (the selector applies having): failed rc={r.returncode}: {r.stderr[-400:]}")
    else:
        f = line[0].split()
        tg = [float(x) for x in f[4:]]
        assert int(f[1]) == mh and int(f[2]) == 0, f[:4]
        print(f"  the same app on the general engine (as before the filter; filter status {f[2]}): {spread(tg)}")
        ratio = statistics.median(tg) / statistics.median(th)
        print(f"  fast path vs general engine: {ratio:.1f}x " + ("faster" if ratio > 1 else "-- NOT faster"))
    for with_clause in (False, True):
        t, rows, n = stream(a, with_clause)
        med = statistics.median(t)
        print(f"  streamed, 64 rules {'with' if with_clause else 'without'} having, {n} events in calls of 4096, "
              f"{rows} rows: {spread(t)} = {n / med / 1e6:.2f} M events/s")


if __name__ == "__main__":
    main()
