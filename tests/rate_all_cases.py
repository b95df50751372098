"""`output all every N events` (and its keyword-free form) behind the fast engines: the
apps, the rule table and the placement job shared by the CPU test of the rule
(siddhi_amd/csrc/sh_rate.h shl_place, tests/rate_all_host) and the GPU parity tests of
the device pass (sh_rate.hip). One window-shaped query (synth.C2_QUERY), and rule sets
of at most 16 queries (tests/rules_cases.py) whose rules mix `all`, `first`, `last` and
no limiter."""
import struct
import subprocess

import numpy as np

from having_fast_cases import PLAIN
from rate_fast_cases import with_rate
from rules_cases import CASES, case_data, oracle_run
from siddhi_amd import synth

SH_RATE_NONE, SH_RATE_FIRST_EVENTS, SH_RATE_LAST_EVENTS, SH_RATE_ALL_EVENTS = 0, 1, 2, 3
KIND = {"first": SH_RATE_FIRST_EVENTS, "last": SH_RATE_LAST_EVENTS, "all": SH_RATE_ALL_EVENTS}
INSERT_OUT = " insert into Out;"
BIG = 2**31 - 1


def c2(clause, text=synth.C2_QUERY):
    assert text.count(INSERT_OUT) == 1
    return text.replace(INSERT_OUT, " " + clause + INSERT_OUT)


MIX = (("all", 2), ("first", 3), ("all", 3), None, ("last", 2), ("all", 1))


def mix_all(r):
    """rule r's limiter: half of the rules hold rows back, every sixth has none"""
    return MIX[r % len(MIX)]


def rule_table(limiter, n_rules):
    """[(kind, N)] per rule, as shl_rule holds them"""
    out = []
    for r in range(n_rules):
        lim = limiter(r)
        out.append((SH_RATE_NONE, 0) if lim is None else (KIND[lim[0]], lim[1]))
    return out


# rule sets of at most 16 queries: (index into rules_cases.CASES, select in place of PLAIN)
AGG_SELECT = "max(e2.amount) as hi, count() as n"
SETS = [(1, PLAIN), (1, AGG_SELECT), (3, PLAIN)]
# the oracle's rows (reaching the limiters, leaving them) of SETS under mix_all
SET_ROWS = {(1, PLAIN): (12_513, 9_774), (1, AGG_SELECT): (12_513, 9_774), (3, PLAIN): (6_052, 4_285)}

_sets = {}


def set_ref(ci, select):
    """(text with mix_all, rule table, data, the oracle's rows without and with the
    limiters, the partition key of every row that reaches them) of a set, once"""
    if (ci, select) not in _sets:
        case = CASES[ci]
        n, cards, nr, rate, batch, merchants, partitioned, free, seed = case
        assert 2 <= nr <= 16
        plain, rules, data = case_data(case)
        assert plain.count(PLAIN) == nr
        plain = plain.replace(PLAIN, select)
        text = with_rate(plain, mix_all)
        ts, card, amount, merchant = data
        rows0 = oracle_run(plain, cards, ts, card, amount, merchant, batch, partitioned)
        rows1 = oracle_run(text, cards, ts, card, amount, merchant, batch, partitioned)
        key = (np.asarray(card)[rows0["seq"].astype(np.int64)].astype(np.int32) if partitioned
               else np.zeros(len(rows0["seq"]), np.int32))
        _sets[(ci, select)] = (text, rule_table(mix_all, nr), data, rows0, rows1, key)
    return _sets[(ci, select)]


def place_job(rules, query, key, path):
    """the job file of tests/rate_all_host"""
    with open(path, "wb") as f:
        f.write(struct.pack("<iiq", len(rules), 0, len(query)))
        f.write(np.asarray(rules, np.int32).reshape(-1, 2).tobytes())
        f.write(np.ascontiguousarray(query, np.int32).tobytes())
        f.write(np.ascontiguousarray(key, np.int32).tobytes())


def run_place(exe, rules, query, key, path):
    """the source row of every output row, by the stand-alone program"""
    place_job(rules, query, key, path)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    (line,) = r.stdout.splitlines()
    assert line.startswith("rows")
    return np.array(line.split()[1:], np.int64)
