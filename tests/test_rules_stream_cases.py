"""The streaming rule-set cases (tests/rules_stream_cases.py) on the CPU: every
case needs carried state -- the oracle fed all calls gives at least 50 more rows
than a fresh oracle per drain group, so a matcher without carry cannot pass the
GPU parity test -- and every case's app is beyond the general engine's query
table yet lowers through the C-ABI (no GPU needed)."""
import ctypes as C

import pytest

from rules_stream_cases import (EXPECTED_ROWS, STREAM_CASES, calls_of, compiled, oracle_rows,
                                oracle_rows_fresh_groups, stream_data)
from siddhi_amd import abi, build


@pytest.mark.parametrize("ci", range(len(STREAM_CASES)))
def test_cases_need_carried_state(ci):
    case = STREAM_CASES[ci]
    every = case[5]
    text, rules, data = stream_data(case)
    calls = calls_of(case, data)
    carried = oracle_rows(case, text, calls, every)
    fresh = oracle_rows_fresh_groups(case, text, calls, every)
    print(ci, len(carried["seq"]), len(fresh["seq"]))
    assert len(carried["seq"]) - len(fresh["seq"]) >= 50
    assert (len(carried["seq"]), len(fresh["seq"])) == EXPECTED_ROWS[ci]


@pytest.fixture(scope="module")
def lib():
    return abi.bind_product(C.CDLL(build.build()))


@pytest.mark.parametrize("ci", range(len(STREAM_CASES)))
def test_cases_are_beyond_the_general_engine_and_lower(lib, ci):
    case = STREAM_CASES[ci]
    assert case[2] > 16  # the general engine's query table holds 16
    text, rules, data = stream_data(case)
    d = compiled(case, text).descriptor()
    h = C.c_void_p()
    rc = lib.sh_compile(C.byref(d), C.byref(h))
    assert rc == abi.SH_OK, lib.sh_last_error(h)
    lib.sh_destroy(h)
