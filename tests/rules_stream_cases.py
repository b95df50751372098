"""Streaming rule sets of more than 16 queries (beyond the general engine's table):
the C5 distributions of tests/rules_cases.py pushed as send(Event[]) calls and
drained every k calls. Shared by the CPU test of the cases themselves and the GPU
parity tests of the streaming rule engine (push, drain, snapshot)."""
import numpy as np

from oracle_engine import OracleEngine
from rules_cases import card_strings
from siddhi_amd import abi, compiler, synth

# (events, cards, rules, rate ev/ms, call size, drain every k calls, merchants, partitioned, free rules, seed)
S1 = (6000, 50, 40, 2, 64, 1, 10, True, (0, 5), 41)          # a step per call, 94 steps
S2 = (6000, 3, 17, 5, 37, 3, 6, True, (), 42)                # smallest set beyond the table; long same-card runs
S3 = (4000, 30, 20, 2, 50, 2, 8, False, (2,), 43)            # unpartitioned: each call is one run
S4 = (8000, 400, 64, 4, 997, 1, 12, True, (3, 7, 9), 44)     # few large steps, many keys
S5 = (5000, 1, 18, 3, 100, 1, 4, True, (), 45)               # one card
STREAM_CASES = [S1, S2, S3, S4, S5]
# rows of the five cases: one oracle over all calls / a fresh oracle per drain group
EXPECTED_ROWS = [(1675, 1024), (5252, 4449), (2208, 1897), (1003, 940), (5374, 4848)]

ROW_FIELDS = ("seq", "query", "ts", "nulls")


def stream_data(case):
    n, cards, nr, rate, call, every, merchants, partitioned, free, seed = case
    ts, card, amount, merchant = synth.txn_stream(n, cards, rate, n_merchants=merchants, seed=seed)
    rules = synth.c5_rules(nr, seed=seed, amount=(10.0, 150.0), merchants=merchants, factor=(0.6, 1.6),
                           within=(1, 40))
    text = synth.c5_query(rules, unit="milliseconds", partitioned=partitioned, free=free)
    return text, rules, (ts, card, amount, merchant)


def compiled(case, text):
    return compiler.compile_app(text, card_strings(case[1]))


def calls_of(case, data, lo=0, hi=None):
    """the send() calls [lo, hi) of a case: (first sequence number, ts, cols, keys)"""
    n, call, partitioned = case[0], case[4], case[7]
    ts, card, amount, merchant = data
    out = []
    for b0 in range(0, n, call):
        b1 = min(n, b0 + call)
        cols = [card[b0:b1].copy(), amount[b0:b1].copy(), merchant[b0:b1].copy()]
        out.append((b0, ts[b0:b1].copy(), cols, card[b0:b1].copy() if partitioned else None))
    return out[lo:hi]


def send_call(eng, c):
    b0, ts, cols, keys = c
    eng.send(0, ts, cols, [None] * len(cols), keys, b0)


def run_calls(eng, calls, every, after_drain=None):
    """send per call, drain every `every` calls (and at the end): the drains as one"""
    parts = []
    for i, c in enumerate(calls):
        send_call(eng, c)
        if (i + 1) % every == 0 or i + 1 == len(calls):
            parts.append(eng.drain())
            if after_drain is not None:
                after_drain()
    return abi.concat_drains(parts) if parts else None


def oracle_rows(case, text, calls, every=1):
    eng = OracleEngine(compiled(case, text))
    eng.start()
    out = run_calls(eng, calls, every)
    eng.close()
    return out


def oracle_rows_fresh_groups(case, text, calls, every):
    """a fresh engine per drain group: what a matcher that carries nothing gives"""
    parts = []
    for g0 in range(0, len(calls), every):
        eng = OracleEngine(compiled(case, text))
        eng.start()
        for c in calls[g0:g0 + every]:
            send_call(eng, c)
        parts.append(eng.drain())
        eng.close()
    return abi.concat_drains(parts)


def assert_rows_equal(got, ref):
    """exact: this path has no tolerance"""
    assert len(got["seq"]) == len(ref["seq"]), (len(got["seq"]), len(ref["seq"]))
    for k in ROW_FIELDS:
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["values"][:, :2], ref["values"][:, :2]), "values"
