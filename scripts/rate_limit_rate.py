"""Rate of `output first|last every N events` on the fast engines (the limiter pass of
sh_rate.hip behind them), beside the general engine that applied it before.

    python scripts/rate_limit_rate.py [--events N] [--keys K] [--repeats R] [--stream-events M]
    rocprofv3 --kernel-trace --stats ... -- python scripts/rate_limit_rate.py --bulk-only

1. C2 bulk: the C2 shape over N stock events (K symbols, 100 events/ms) with
   `output first every 3 events`, through sh_run_device with the events in HBM.
   Reported: the call's host-clock time, the clause's share (the same app without it,
   same job, alternating runs), the pass's own launches (HIP events) and the bytes it
   moves by construction -- sort words and indices, the radix passes over (word, index)
   pairs, the scan's pairs, keep bytes, the kept rows in and out (a bulk call writes no
   put pairs) -- as a fraction of 8 TB/s over the launches' time.
2. The comparison: the same app with SH_NO_RATE_FILTER=1, which compiles it as before
   this pass existed (the general engine's selector applies the limiter), in a child
   process of the same job (the variable is read at compile time).
3. Streaming: the 64-rule set of scripts/having_rate.py, M card transactions in calls
   of 4,096 drained every 64 calls, in events per second, without and with
   `output first every 3 events` on every rule.

--bulk-only runs part 1's app with the clause alone, for a kernel trace: the pass's kernels
are k_shl_*, the radix sort's k_digit_hist / k_digit_scatter (the bucketed engine launches
none) and k_shv_move.

Every timed pass follows one untimed warm-up; medians with min and max of R passes.
One record, no gate."""
import argparse
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

CLAUSE = "output first every 3 events"
HBM_BYTES_PER_S = 8e12


def c2_texts():
    from siddhi_amd import synth
    return synth.C2_QUERY, synth.C2_QUERY.replace(" insert into Out;", f" {CLAUSE} insert into Out;")


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
    pass_ms = [[] for _ in texts]
    ms = [0] * len(texts)
    for i in range(a.repeats + 1):
        for j, r in enumerate(runners):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ms[j] = r.run(tts, tk, cols, a.keys)[0]
            torch.cuda.synchronize()
            if i:
                times[j].append(time.perf_counter() - t0)
                pass_ms[j].append(r.rate_ms())
    out = [(times[j], ms[j], dict(bucket=r.bucket_status(), rate=r.rate_status(), rows=r.rate_rows(),
                                  pass_ms=statistics.median(pass_ms[j])))
           for j, r in enumerate(runners)]
    for r in runners:
        r.close()
    return out


def child(a):
    """the comparison arm: prints one line"""
    plain, limited = c2_texts()
    (t, m, st), = bulk(a, [limited])
    print(f"CHILD {m} {st['rate']} {st['bucket']} " + " ".join(f"{x:.6f}" for x in t))


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
        text = text.replace(" insert into Alerts;", f" {CLAUSE} insert into Alerts;")
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
    ap.add_argument("--bulk-only", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no rate"
    if a.child or a.bulk_only:
        return child(a)
    plain, limited = c2_texts()
    (tp, mp, sp), (tl, ml, sl) = bulk(a, [plain, limited])
    assert sl["rate"] == 1 and sl["rows"] == (mp, ml), (sl, mp, ml)
    n_out = 4
    radix_passes = (max(1, (a.keys - 1).bit_length()) + 7) // 8
    prep = mp * (8 + 4 + 8)                 # sequence number and key in; sort word and index out
    sort = radix_passes * mp * (4 + 8 + 8)  # histogram read; scatter read and write of (word, index)
    rank = mp * (4 + 8) + mp * (4 + 4 + 8 + 1)  # the scan: word in, pair out; ordinals: word, index, pair in, keep byte out
    rows = 2 * ml * (n_out + 1) * 8 + mp    # keep bytes to ballots; the kept rows in and out
    moved = prep + sort + rank + rows
    share = statistics.median(tl) - statistics.median(tp)
    print(f"rate_limit_rate: C2, {a.events} events, {a.keys} keys, `{CLAUSE}`: {mp} rows in, {ml} kept "
          f"({ml / max(1, mp):.2f}); bucketed engine {sl['bucket']}, device limiter pass {sl['rate']}")
    print(f"  sh_run_device without the clause: {spread(tp)}")
    print(f"  sh_run_device with the clause:    {spread(tl)}")
    print(f"  the clause's share of the call (difference of the medians: the pass, one 8-byte read-back and its "
          f"synchronise): {share * 1e3:.2f} ms; the pass's launches alone (HIP events, median): {sl['pass_ms']:.3f} ms")
    t_pass = sl["pass_ms"] / 1e3 if sl["pass_ms"] > 0 else share
    print(f"  bytes the pass moves by construction: {moved / 1e6:.1f} MB (sort words and indices {prep / 1e6:.1f}, "
          f"{radix_passes} radix passes over (word, index) {sort / 1e6:.1f}, scan pairs and keep bytes "
          f"{rank / 1e6:.1f}, ballots and kept rows {rows / 1e6:.1f}) = "
          f"{moved / max(t_pass, 1e-9) / HBM_BYTES_PER_S * 100:.1f}% of 8 TB/s over the launches' time; the sort is "
          f"{sort / moved * 100:.0f}% of the bytes")
    env = dict(os.environ, SH_NO_RATE_FILTER="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--events", str(a.events), "--keys",
                        str(a.keys), "--repeats", str(min(3, a.repeats))], env=env, capture_output=True, text=True)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
    if r.returncode or not line:
        print(f"  general engine (the selector applies the limiter): failed rc={r.returncode}: {r.stderr[-400:]}")
    else:
        f = line[0].split()
        tg = [float(x) for x in f[4:]]
        assert int(f[1]) == ml and int(f[2]) == 0, f[:4]
        print(f"  the same app on the general engine (as before the pass; pass status {f[2]}): {spread(tg)}")
        ratio = statistics.median(tg) / statistics.median(tl)
        print(f"  fast path vs general engine: {ratio:.1f}x " + ("faster" if ratio > 1 else "-- NOT faster"))
    for with_clause in (False, True):
        t, rows, n = stream(a, with_clause)
        med = statistics.median(t)
        print(f"  streamed, 64 rules {'with' if with_clause else 'without'} the clause, {n} events in calls of 4096, "
              f"{rows} rows: {spread(t)} = {n / med / 1e6:.2f} M events/s")


if __name__ == "__main__":
    main()
