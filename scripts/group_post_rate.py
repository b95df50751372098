"""Rate of a `group by` select behind the fast engines (the segment pass of sh_group.hip
and the aggregate post-pass of sh_agg.hip behind the bucketed engine), beside the general
engine that applied the clause before.

    python scripts/group_post_rate.py [--events N] [--keys K] [--repeats R] [--out FILE]

The C2 shape over N stock events (K symbols, 100 events/ms) through sh_run_device with
the events in HBM, four runners in alternating runs of one job:
  grouped   select e1.symbol, e2.volume, sum(e2.volume), count() group by e2.volume
  general   the same app compiled under SH_NO_GROUP_POST=1 (read at compile time): the
            general engine's selector applies the clause, as before the pass existed
  ungrouped the same select without the clause, as it runs by default (the bucketed
            engine's carry forms the running values)
  ungrouped_post the same, with SH_BK_AGG_POST=1 around its calls (read per call): the
            bucketed engine writes arguments and the post-pass over (query, key) forms
            the values, so the difference to `grouped` is the segment pass alone
Reported: the calls' host-clock times, the post-pass's own launches (HIP events,
shx_agg_post_ms), and the cost of the group sort passes as the difference to the
ungrouped select. Every timed pass follows one untimed warm-up; medians with min and
max of R passes. One record, no gate."""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SELECT = "e1.symbol as symbol, e2.volume as v2, sum(e2.volume) as tv, count() as n"
GROUP = "group by e2.volume"


def spread(x):
    return f"median {statistics.median(x) * 1e3:.2f} ms (min {min(x) * 1e3:.2f}, max {max(x) * 1e3:.2f}, n={len(x)})"


def texts():
    from siddhi_amd import synth
    head = synth.C2_QUERY[:synth.C2_QUERY.index("select ")]
    return (head + f"select {SELECT} {GROUP} insert into Out; end;", head + f"select {SELECT} insert into Out; end;")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10_000_000)
    ap.add_argument("--keys", type=int, default=10_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: a CPU run gives no rate"
    from siddhi_amd import compiler, synth
    from siddhi_amd.device_run import DeviceRunner
    grouped, plain = texts()
    ts, k, p, v = synth.stock_stream(a.events, a.keys, 100)
    dev = torch.device("cuda:0")
    tts, tk = torch.from_numpy(ts).to(dev), torch.from_numpy(k).to(dev)
    cols = [tk, torch.from_numpy(p).to(dev), torch.from_numpy(v).to(dev)]
    names = ("grouped", "general", "ungrouped", "ungrouped_post")
    runners = {"grouped": DeviceRunner(compiler.compile_app(grouped))}
    os.environ["SH_NO_GROUP_POST"] = "1"
    runners["general"] = DeviceRunner(compiler.compile_app(grouped))
    del os.environ["SH_NO_GROUP_POST"]
    runners["ungrouped"] = DeviceRunner(compiler.compile_app(plain))
    runners["ungrouped_post"] = DeviceRunner(compiler.compile_app(plain))
    times = {n: [] for n in names}
    post = {n: [] for n in names}
    rows, seqs = {}, {}
    for i in range(a.repeats + 1):
        for n in names:
            r = runners[n]
            if n == "ungrouped_post":
                os.environ["SH_BK_AGG_POST"] = "1"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = r.run(tts, tk, cols, a.keys)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            os.environ.pop("SH_BK_AGG_POST", None)
            rows[n] = res[0]
            if i == 0:
                seqs[n] = (res[1].clone(), res[2].clone())
                print(f"  warm-up {n}: {dt * 1e3:.1f} ms, {res[0]} rows", flush=True)
            else:
                times[n].append(dt)
                post[n].append(r.agg_post_ms())
    st = {n: dict(bucket=r.bucket_status(), group=r.group_status(), agg=r.agg_status()) for n, r in runners.items()}
    same = bool(torch.equal(seqs["grouped"][0], seqs["general"][0]) and torch.equal(seqs["grouped"][1], seqs["general"][1]))
    for r in runners.values():
        r.close()
    assert st["grouped"]["group"] == 1 and st["general"]["group"] == 0 and st["ungrouped"]["group"] == 0, st
    assert st["ungrouped_post"] == dict(bucket=1, group=0, agg=1), st
    key_passes = (max(1, (a.keys - 1).bit_length()) + 7) // 8
    word_passes = 64 // 8   # e2.volume is a long: low and high half of the group word, 8 bits a pass
    med = lambda x: statistics.median(x)  # noqa: E731
    lines = [
        f"group_post_rate: C2, {a.events} events, {a.keys} keys, `{GROUP}` over a long column: {rows['grouped']} rows; "
        f"grouped and general rows equal: {same}",
        f"  statuses (bucket, group, agg): " + ", ".join(f"{n} {tuple(st[n].values())}" for n in names),
        f"  sh_run_device, grouped select on the fast path:      {spread(times['grouped'])}",
        f"  sh_run_device, the same app on the general engine:   {spread(times['general'])}",
        f"  sh_run_device, the ungrouped sum / count select:     {spread(times['ungrouped'])}",
        f"  sh_run_device, ungrouped through the post-pass:      {spread(times['ungrouped_post'])}",
        f"  the post-pass's own launches (HIP events, median): grouped {med(post['grouped']):.3f} ms, "
        f"ungrouped through the post-pass {med(post['ungrouped_post']):.3f} ms",
        f"  cost of the group sort passes (grouped less ungrouped through the post-pass): "
        f"{med(post['grouped']) - med(post['ungrouped_post']):.3f} ms of launches, "
        f"{(med(times['grouped']) - med(times['ungrouped_post'])) * 1e3:.2f} ms of the call, for {word_passes} radix passes "
        f"over the group word on top of the {key_passes} over (query, key), with the words, the head flags and the ids",
    ]
    ratio = statistics.median(times["general"]) / statistics.median(times["grouped"])
    lines.append(f"  fast path vs general engine: {ratio:.1f}x " + ("faster" if ratio > 1 else "-- NOT faster"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
