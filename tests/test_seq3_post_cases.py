"""`having` and the event limiters on the rise-and-fall sequence, on the CPU: the
premises of the shared cases against the oracle alone, the product's row predicate
(sh_having.h, tests/having_host), keep rule and placement rule (sh_rate.h,
tests/rate_host and tests/rate_all_host) applied to the oracle's clause-free rows
against the oracle's rows with the clause, and what libsiddhi_hip.so lowers: the shape
sh_run_device's rise-and-fall rungs read, and the streaming program it leaves alone
(compiling needs no device)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import seq3_post_cases as sc
from having_fast_cases import predicate_job
from rate_all_cases import SH_RATE_ALL_EVENTS, run_place
from rate_fast_cases import keep_job, take_rows
from siddhi_amd import abi, build, compiler, synth

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("seq", "query", "ts", "nulls", "values")
ALL = [(name, K) for name in sc.CASES for K in sc.KS] + [(name, "tie") for name in sc.TIE_CASES]
# `last every 2` at 600 keys: every key of that stream has two rows or more, so no key has
# fewer than N; a key with an odd count (its last row has no second) stands in
NO_SHORT_KEY = {("last2", sc.K_SEQ3S)}


def case_of(name):
    return sc.CASES.get(name) or sc.TIE_CASES[name]


def _make(name):
    d = os.path.join(HERE, name)
    subprocess.run(["make", "-s", "-C", d], check=True)
    return os.path.join(d, name)


@pytest.fixture(scope="module")
def hosts():
    return {n: _make(n) for n in ("having_host", "rate_host", "rate_all_host")}


def _having_mask(exe, case, rows, path):
    predicate_job(compiler.compile_app(sc.having_text(case)).descriptor(), rows, path)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[0].startswith("q 0 ") and int(lines[0].split()[2]) > 0  # it lowers
    return np.array([c == "1" for c in lines[-1].split()[1]], bool)


def _keep_mask(exe, rule, key, path):
    keep_job([rule], np.zeros(len(key), np.int32), key, [], path)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return np.array([c == "1" for c in r.stdout.splitlines()[0].split()[1]], bool)


@pytest.mark.parametrize("name,which", ALL)
def test_premises_and_host_rules_reproduce_the_oracle(hosts, tmp_path, name, which):
    case = case_of(name)
    plain, having, lim = case
    rows0 = sc.oracle_rows(plain, which)
    rows1 = sc.oracle_rows(sc.having_text(case), which)
    rows2 = sc.oracle_rows(sc.text_of(case), which)
    n0, n1, n2 = len(rows0["seq"]), len(rows1["seq"]), len(rows2["seq"])
    print(name, which, "rows: unfiltered, after having, after the limiter =", (n0, n1, n2))
    assert n0 > 1000
    # ---- `having`: the product's row predicate over the oracle's clause-free rows
    reach = rows0
    if having:
        assert 0.1 * n0 < n1 < 0.9 * n0
        mask = _having_mask(hosts["having_host"], case, rows0, str(tmp_path / "hv.bin"))
        reach = take_rows(rows0, mask)
        for f in FIELDS:
            assert np.array_equal(reach[f], rows1[f]), f
    else:
        assert n1 == n0
    # ---- the limiter: keep rule / placement rule over the rows that reach it
    if lim:
        kind, n = lim
        key = sc.row_keys(reach, which)
        bc = np.bincount(key)
        assert np.any(bc > n)
        if n > 1 and (name, which) in NO_SHORT_KEY:
            assert not np.any((bc > 0) & (bc < n)) and np.any(bc % n != 0)
        elif n > 1:
            assert np.any((bc > 0) & (bc < n))
        rule = sc.rule_of(case)
        if kind == "all":
            assert rule[0] == SH_RATE_ALL_EVENTS
            order = run_place(hosts["rate_all_host"], [rule], np.zeros(len(key), np.int32), key,
                              str(tmp_path / "place.bin"))
            if n == 1:
                assert np.array_equal(order, np.arange(len(key)))
            else:
                assert np.any(np.diff(rows2["seq"].astype(np.int64)) < 0)  # rows moved to their chunk's N-th
        else:
            order = np.nonzero(_keep_mask(hosts["rate_host"], rule, key, str(tmp_path / "keep.bin")))[0]
        assert len(order) == n2
        assert (n2 == n1) == (n == 1)
        for f in FIELDS:
            assert np.array_equal(np.asarray(reach[f])[order], rows2[f]), f
    else:
        assert n2 == n1


# ---- compile through libsiddhi_hip.so
@pytest.fixture(scope="module")
def lib():
    return abi.bind_product(C.CDLL(build.build()))


def _compile(lib, text):
    """(rc, error, shx_seq3_shape, shx_fingerprint)"""
    d = compiler.compile_app(text).descriptor()
    h = C.c_void_p()
    rc = lib.sh_compile(C.byref(d), C.byref(h))
    err = (lib.sh_last_error(h) or b"").decode()
    shape = lib.shx_seq3_shape(h) if rc == abi.SH_OK else -1
    fp = lib.shx_fingerprint(h) if rc == abi.SH_OK else 0
    lib.sh_destroy(h)
    return rc, err, shape, fp


def _switches(case):
    return [s for s, on in (("SH_NO_HAVING_FILTER", case[1]), ("SH_NO_RATE_FILTER", case[2])) if on]


@pytest.mark.parametrize("name", list(sc.CASES) + list(sc.TIE_CASES))
def test_cases_lower_to_the_rise_and_fall_shape_and_stream_as_before(lib, monkeypatch, name):
    """shape 1 (0 without this stage, and 0 again under either switch of the case's
    clauses); the fingerprint a snapshot image carries is the switch's: the streaming
    program does not know the stage"""
    case = case_of(name)
    text = sc.text_of(case)
    rc, err, shape, fp = _compile(lib, text)
    assert rc == abi.SH_OK, err
    assert shape == 1
    assert _compile(lib, case[0])[2] == 1  # the clause-free app, as ever
    for s in _switches(case):
        with monkeypatch.context() as m:
            m.setenv(s, "1")
            prc, perr, pshape, pfp = _compile(lib, text)
        assert prc == abi.SH_OK, perr
        assert pshape == 0, s
        assert pfp == fp != 0, s


@pytest.mark.parametrize("clause", [
    "having e1.volume > 5",                        # a state attribute that is not selected
    "having p3 < 30.0 order by p1",                # order by beside the clause
    "order by p1 output first every 3 events",
    "having p3 < 30.0 limit 5",
    "output first every 1 sec",                    # the time limiter (playback)
])
def test_other_selector_extras_stay_on_the_general_engine(lib, clause):
    text = sc.c3(clause)
    if "sec" in clause:
        text = "@app:playback " + text
    rc, err, shape, fp = _compile(lib, text)
    assert rc == abi.SH_OK, err
    assert shape == 0


def test_a_set_of_two_queries_is_not_the_shape(lib):
    q = synth.C3_QUERY
    begin, end = q.index("@info"), q.index(" end;")
    body = q[begin:end].replace(sc.INSERT_OUT, " having p3 < 30.0" + sc.INSERT_OUT)
    two = q[:begin] + body + " " + body.replace("query1", "query2") + q[end:]
    rc, err, shape, fp = _compile(lib, two)
    assert rc == abi.SH_OK, err
    assert shape == 0
