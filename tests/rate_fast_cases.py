"""Streaming rule sets of more than 16 queries whose rules carry an event limiter,
`output first|last every N events`: the sets of tests/rules_stream_cases.py with a
clause of its own per rule inserted before its `insert into Alerts;`. Shared by the
CPU test of the cases and of the keep rule (siddhi_amd/csrc/sh_rate.h), and by the GPU
parity tests of the device pass (sh_rate.hip)."""
import struct

import numpy as np

from having_fast_cases import INSERT, PLAIN, with_having
from rules_stream_cases import S1, S2, S3, S4, S5, calls_of, oracle_rows, stream_data
from siddhi_amd import abi

SH_RATE_NONE, SH_RATE_FIRST_EVENTS, SH_RATE_LAST_EVENTS = 0, 1, 2
KIND = {"first": SH_RATE_FIRST_EVENTS, "last": SH_RATE_LAST_EVENTS}


def uniform(kind, n):
    return lambda r: (kind, n)


def mix(r):
    """the S1 mix: `first` if r is odd else `last`, every 1 + r % 4 events"""
    return ("first" if r % 2 else "last", 1 + r % 4)


def every_third_free(r):
    return None if r % 3 == 0 else ("first", 3)


# (name, base case, select in place of PLAIN, having of rule r or None, limiter of rule r
#  -> (kind, N) or None, oracle rows without / with the limiter clause)
R_F3 = ("F3", S2, PLAIN, None, uniform("first", 3), (5252, 1769))
R_L2 = ("L2", S2, PLAIN, None, uniform("last", 2), (5252, 2615))
R_F1 = ("F1", S2, PLAIN, None, uniform("first", 1), (5252, 51))  # 17 rules x 3 cards
R_L1 = ("L1", S2, PLAIN, None, uniform("last", 1), (5252, 5252))
R_MIX1 = ("MIX_S1", S1, PLAIN, None, mix, (1675, 981))
R_S3 = ("F3_S3", S3, PLAIN, None, uniform("first", 3), (2208, 742))  # unpartitioned
R_S4 = ("L2_S4", S4, PLAIN, None, uniform("last", 2), (1003, 52))
R_MIX5 = ("MIX_S5", S5, PLAIN, None, mix, (5374, 3115))  # one card
R_HAV = ("HAV_F2", S2, PLAIN, lambda r: f"amount > {60.0 + 5 * r}", uniform("first", 2), (5252, 2307))
R_AGG = ("AGG_L3", S2, "sum(e2.amount) as total, count() as n", None, uniform("last", 3), (5252, 1734))
# every third rule has no limiter (pinned from the oracle)
R_FREE = ("FREE3", S2, PLAIN, None, every_third_free, (5252, 2972))
RATE_CASES = [R_F3, R_L2, R_F1, R_L1, R_MIX1, R_S3, R_S4, R_MIX5, R_HAV, R_AGG, R_FREE]
BY_NAME = {rc[0]: rc for rc in RATE_CASES}
AGGREGATING = ("AGG_L3",)


def clause_text(lim):
    return "" if lim is None else f" output {lim[0]} every {lim[1]} events"


def with_rate(text, limiter):
    """rule r's limiter clause inserted before its `insert into Alerts;`"""
    parts = text.split(INSERT)
    assert parts[-1].strip() in ("", "end;")
    return "".join(p + clause_text(limiter(r)) + INSERT for r, p in enumerate(parts[:-1])) + parts[-1]


def rate_texts(rc):
    """(text without the limiters -- with the case's select and `having` --, text with
    them, data) of a case"""
    name, base, select, having, limiter, counts = rc
    text, rules, data = stream_data(base)
    assert text.count(PLAIN) == base[2] and text.count(INSERT) == base[2]
    plain = text.replace(PLAIN, select)
    if having is not None:
        plain = with_having(plain, having)
    return plain, with_rate(plain, limiter), data


def plain_text(rc):
    """the case's text with its select, without `having` and without limiters"""
    text, rules, data = stream_data(rc[1])
    return text.replace(PLAIN, rc[2])


def rule_table(rc):
    """[(kind, N)] per rule, as shl_rule holds them"""
    out = []
    for r in range(rc[1][2]):
        lim = rc[4](r)
        out.append((SH_RATE_NONE, 0) if lim is None else (KIND[lim[0]], lim[1]))
    return out


_cache = {}


def rate_ref(rc):
    """a case's texts, data, calls and the oracle's rows without the limiters (the rows
    that reach them: after any `having`) and with them at its drain cadence, once"""
    name, base = rc[0], rc[1]
    if name not in _cache:
        before, text, data = rate_texts(rc)
        calls = calls_of(base, data)
        _cache[name] = (before, text, data, calls, oracle_rows(base, before, calls, base[5]),
                        oracle_rows(base, text, calls, base[5]))
    return _cache[name]


def row_keys(rc, data, rows):
    """the partition key of every row: its trigger event's card (0 when unpartitioned)"""
    if not rc[1][7]:
        return np.zeros(len(rows["seq"]), np.int32)
    return np.asarray(data[1])[rows["seq"].astype(np.int64)].astype(np.int32)


def keep_job(rules, query, key, cuts, path):
    """the job file of tests/rate_host"""
    with open(path, "wb") as f:
        f.write(struct.pack("<iiq", len(rules), len(cuts), len(query)))
        f.write(np.asarray(rules, np.int32).reshape(-1, 2).tobytes())
        f.write(np.asarray(cuts, np.int64).tobytes())
        f.write(np.ascontiguousarray(query, np.int32).tobytes())
        f.write(np.ascontiguousarray(key, np.int32).tobytes())


def take_rows(rows, mask):
    """the rows a keep mask leaves, as a drain's arrays"""
    return {k: np.asarray(v)[mask] for k, v in rows.items() if k in ("seq", "query", "ts", "nulls", "values")}


def concat(parts):
    return abi.concat_drains(parts)
