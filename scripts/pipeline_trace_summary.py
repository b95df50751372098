"""Summarise a rocprofv3 --kernel-trace CSV of a C2 bench run of the bucketed
engine's segment pipeline: per segment of the last step the start and end of
shb_match and k_bk_emit (us from the step's scatter), and the share of the
emitters' time during which a matcher kernel was running.

usage: pipeline_trace_summary.py <..._kernel_trace.csv>"""
import csv
import sys


def main(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if "k_bk_scatter" in r[2]]
    if not starts:
        print("no k_bk_scatter dispatch in the trace")
        return 1
    step = rows[starts[-1]:]
    t0 = step[0][0]
    match = [(s, e) for s, e, n in step if "shb_match" in n]
    emit = [(s, e) for s, e, n in step if "k_bk_emit" in n]
    scan = [(s, e) for s, e, n in step if "k_bk_scan_seg" in n]
    us = lambda t: (t - t0) / 1000.0
    print(f"last step of {len(starts)}: {len(match)} shb_match, {len(scan)} k_bk_scan_seg, {len(emit)} k_bk_emit "
          f"dispatches; times in us from the start of k_bk_scatter")
    print(f"{'seg':>3} {'match start':>12} {'match end':>10} {'emit start':>11} {'emit end':>9} {'emit us':>8} "
          f"{'beside a matcher us':>20}")
    tot = both = 0.0
    for k in range(max(len(match), len(emit))):
        ms, me = match[k] if k < len(match) else (t0, t0)
        line = f"{k:>3} {us(ms):>12.1f} {us(me):>10.1f}"
        if k < len(emit):
            es, ee = emit[k]
            ov = sum(max(0, min(ee, b) - max(es, a)) for a, b in match) / 1000.0
            tot += (ee - es) / 1000.0
            both += ov
            line += f" {us(es):>11.1f} {us(ee):>9.1f} {(ee - es) / 1000.0:>8.1f} {ov:>20.1f}"
        print(line)
    end = max(e for _, e in emit) if emit else step[-1][1]
    print(f"step: {us(end):.1f} us from the scatter's start to the last emitter's end; matchers "
          f"{sum(e - s for s, e in match) / 1000.0:.1f} us, emitters {tot:.1f} us summed")
    if tot > 0:
        print(f"share of emitter time with a matcher kernel running: {100.0 * both / tot:.1f} %")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
