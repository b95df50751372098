"""Rate of `output all every N events` on the fast engines (the placement pass of
sh_rate.hip behind them), beside the general engine that applied it before.

    python scripts/rate_all_rate.py [--events N] [--keys K] [--repeats R]

1. C2 bulk: the C2 shape over N stock events (K symbols, 100 events/ms) through
   sh_run_device with the events in HBM, three apps in alternating runs of one job: without
   a limiter, with `output all every 3 events`, and with `output first every 3 events`
   (the compaction, whose launches the placement leaves as they were: to hold against
   profiles/rate_limit_filter.txt). Reported: the calls' host-clock times, the pass's own
   launches (HIP events) and the bytes the placement moves by construction -- sort words
   and indices, the radix passes over (word, index) pairs, the scan's pairs, release row,
   offset and weight per row, the weights' scan, the source list, the released rows in and
   out -- as a fraction of 8 TB/s over the launches' time.
2. The comparison: the `all` app with SH_NO_RATE_FILTER=1, which compiles it as before
   this pass existed (the general engine's selector applies the limiter), in a child
   process of the same job (the variable is read at compile time).

Every timed pass follows one untimed warm-up; medians with min and max of R passes.
One record, no gate."""
import argparse
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from rate_limit_rate import HBM_BYTES_PER_S, bulk, spread  # noqa: E402  (sets the package's path up)

ALL, FIRST = "output all every 3 events", "output first every 3 events"


def texts():
    from siddhi_amd import synth
    with_clause = lambda c: synth.C2_QUERY.replace(" insert into Out;", f" {c} insert into Out;")  # noqa: E731
    return synth.C2_QUERY, with_clause(ALL), with_clause(FIRST)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10_000_000)
    ap.add_argument("--keys", type=int, default=10_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no rate"
    plain, held, first = texts()
    if a.child:
        (t, m, st), = bulk(a, [held])
        print(f"CHILD {m} {st['rate']} {st['bucket']} " + " ".join(f"{x:.6f}" for x in t))
        return
    (tp, mp, sp), (ta, ma, sa), (tf, mf, sf) = bulk(a, [plain, held, first])
    assert sa["rate"] == 1 and sa["rows"] == (mp, ma), (sa, mp, ma)
    assert sf["rate"] == 1 and sf["rows"] == (mp, mf), (sf, mp, mf)
    n_out = 4
    radix_passes = (max(1, (a.keys - 1).bit_length()) + 7) // 8
    prep = mp * (8 + 4 + 8)                 # sequence number and key in; sort word and index out
    sort = radix_passes * mp * (4 + 8 + 8)  # histogram read; scatter read and write of (word, index)
    rank = mp * (4 + 8) + mp * (4 + 4 + 8 + 4 + 12)  # the scan: word in, pair out; release rows: word, index, pair,
                                                     # the release row's index in; release row, offset, weight out
    place = mp * 16 + mp * 16 + ma * 4      # the weights' scan (two levels); release row, offset, weight and the
                                            # release row's start in, the source list out
    rows = ma * 4 + 2 * ma * (n_out + 1) * 8  # the source list in; the released rows in and out
    moved = prep + sort + rank + place + rows
    print(f"rate_all_rate: C2, {a.events} events, {a.keys} keys, `{ALL}`: {mp} rows in, {ma} released "
          f"({ma / max(1, mp):.3f}); bucketed engine {sa['bucket']}, device limiter pass {sa['rate']}")
    print(f"  sh_run_device without a limiter:   {spread(tp)}")
    print(f"  sh_run_device with `{ALL}`:   {spread(ta)}")
    print(f"  sh_run_device with `{FIRST}`: {spread(tf)} ({mf} rows kept)")
    share = statistics.median(ta) - statistics.median(tp)
    print(f"  the `all` clause's share of the call (difference of the medians: the pass, one 8-byte read-back and its "
          f"synchronise): {share * 1e3:.2f} ms; the pass's launches alone (HIP events, median): placement "
          f"{sa['pass_ms']:.3f} ms, compaction {sf['pass_ms']:.3f} ms")
    t_pass = sa["pass_ms"] / 1e3 if sa["pass_ms"] > 0 else share
    print(f"  bytes the placement moves by construction: {moved / 1e6:.1f} MB (sort words and indices {prep / 1e6:.1f}, "
          f"{radix_passes} radix passes over (word, index) {sort / 1e6:.1f}, scan pairs and release rows "
          f"{rank / 1e6:.1f}, weight scan and source list {place / 1e6:.1f}, released rows {rows / 1e6:.1f}) = "
          f"{moved / max(t_pass, 1e-9) / HBM_BYTES_PER_S * 100:.1f}% of 8 TB/s over the launches' time")
    env = dict(os.environ, SH_NO_RATE_FILTER="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--events", str(a.events), "--keys",
                        str(a.keys), "--repeats", str(min(3, a.repeats))], env=env, capture_output=True, text=True)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
    if r.returncode or not line:
        print(f"  general engine (the selector applies the limiter): failed rc={r.returncode}: {r.stderr[-400:]}")
        return
    f = line[0].split()
    tg = [float(x) for x in f[4:]]
    assert int(f[1]) == ma and int(f[2]) == 0, f[:4]
    print(f"  the same app on the general engine (as before the pass; pass status {f[2]}): {spread(tg)}")
    ratio = statistics.median(tg) / statistics.median(ta)
    print(f"  fast path vs general engine: {ratio:.1f}x " + ("faster" if ratio > 1 else "-- NOT faster"))


if __name__ == "__main__":
    main()
