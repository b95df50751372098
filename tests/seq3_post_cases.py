"""An output-only `having` and `output first|last|all every N events` on the
rise-and-fall sequence (synth.C3_QUERY) in bulk runs: the apps, the streams and the
oracle's rows shared by the CPU test of the premises and the lowering
(tests/test_seq3_post_cases.py) and the GPU parity tests of sh_run_device with the row
post-filter stage behind k_s3b / k_seq3s (tests/test_gpu_seq3_post.py)."""
import numpy as np

from oracle_engine import OracleEngine
from rate_all_cases import KIND
from siddhi_amd import compiler, synth
from test_gpu_agg import C3_AGG

INSERT_OUT = " insert into Out;"
C3_MAX = C3_AGG.replace("sum(", "max(")

N = 16_384
K_S3B, K_SEQ3S = 1_200, 600  # keys: the bucket-carry engine takes 1,024 or more, k_seq3s the rest
KS = (K_S3B, K_SEQ3S)


def c3(clause, text=synth.C3_QUERY):
    assert text.count(INSERT_OUT) == 1
    return text.replace(INSERT_OUT, " " + clause + INSERT_OUT) if clause else text


# name -> (the clause-free text, `having` or None, limiter (kind, N) or None)
# thresholds: near the medians of the oracle's rows on both streams (prices 5..55, a
# key's sum of up to 13 of them); tests/test_seq3_post_cases.py asserts what they keep
CASES = {
    "having_p3": (synth.C3_QUERY, "p3 < 30.0", None),
    "having_and": (synth.C3_QUERY, "peak > 24.0 and p3 < 36.0", None),
    "first3": (synth.C3_QUERY, None, ("first", 3)),
    "last2": (synth.C3_QUERY, None, ("last", 2)),
    "all3": (synth.C3_QUERY, None, ("all", 3)),
    "having_first2": (synth.C3_QUERY, "p3 < 30.0", ("first", 2)),
    "sum_having": (C3_AGG, "s3 > 60.0", None),
    "max_having": (C3_MAX, "s3 > 30.0", None),
    "all1": (synth.C3_QUERY, None, ("all", 1)),
}
# the same shape on the stream with few distinct prices (tie_stream)
TIE_CASES = {
    "tie_having": (synth.C3_QUERY, "p3 < 2.0", None),
    "tie_first3": (synth.C3_QUERY, None, ("first", 3)),
    "tie_having_all2": (synth.C3_QUERY, "peak > 2.0", ("all", 2)),
}
AGGREGATING = {"sum_having": "sum", "max_having": "max"}


def clause(case):
    plain, having, lim = case
    parts = []
    if having:
        parts.append("having " + having)
    if lim:
        parts.append(f"output {lim[0]} every {lim[1]} events")
    return " ".join(parts)


def text_of(case):
    return c3(clause(case), case[0])


def having_text(case):
    """the app with the `having` alone: its rows reach the limiter"""
    return c3("having " + case[1], case[0]) if case[1] else case[0]


def rule_of(case):
    return (KIND[case[2][0]], case[2][1]) if case[2] else (0, 0)


def one_attribute(case):
    """every select value is the 4-byte price: the bucket-carry engine's premise"""
    return case[0] == synth.C3_QUERY


_streams = {}
_rows = {}


def stream(K):
    if K not in _streams:
        _streams[K] = synth.stock_stream(N, K, 1000, config_index=3)
    return _streams[K]


def tie_stream():
    """five distinct prices: equal neighbours in most keys (neither filter holds on a tie)"""
    if "tie" not in _streams:
        ts, k, p, v = stream(K_S3B)
        _streams["tie"] = (ts, k, np.random.default_rng(3).integers(0, 5, N).astype(np.float32), v)
    return _streams["tie"]


def rounding_stream(K):
    """the rounding prices of tests/test_gpu_run_ladder.py: sums of them are not exact in
    any order but the reference's"""
    if ("r", K) not in _streams:
        ts, k, p, v = stream(K)
        p = p.copy()
        p[::7] *= np.float32(2.0 ** 60)
        p[3::11] *= np.float32(2.0 ** -60)
        _streams[("r", K)] = (ts, k, p, v)
    return _streams[("r", K)]


def data_of(which):
    return tie_stream() if which == "tie" else rounding_stream(which[1]) if isinstance(which, tuple) else stream(which)


def oracle_rows(text, which):
    """the oracle's rows (a drain's arrays) of `text` over a stream, once; `which`: a key
    count, "tie", or ("r", key count)"""
    if (text, which) not in _rows:
        ts, k, p, v = data_of(which)
        eng = OracleEngine(compiler.compile_app(text))
        eng.start()
        for b0 in range(0, N, 4096):
            b1 = b0 + 4096
            eng.send(0, ts[b0:b1], [np.ascontiguousarray(c[b0:b1]) for c in (k, p, v)], [None] * 3,
                     np.ascontiguousarray(k[b0:b1]), b0)
        out = eng.drain()
        eng.close()
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _rows[(text, which)] = out
    return _rows[(text, which)]


def row_keys(rows, which):
    """the partition key of every row: its trigger event's symbol"""
    return np.asarray(data_of(which)[1])[rows["seq"].astype(np.int64)].astype(np.int32)


def counts(case, which):
    """the oracle's rows: unfiltered, after `having`, after the limiter"""
    return tuple(len(oracle_rows(t, which)["seq"]) for t in (case[0], having_text(case), text_of(case)))
