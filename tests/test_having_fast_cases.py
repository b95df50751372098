"""The output-only `having` cases (tests/having_fast_cases.py) on the CPU: the
oracle's row counts without and with the clause, the product's row predicate
(siddhi_amd/csrc/sh_having.h) compiled for the CPU against the oracle's rows, and
what libsiddhi_hip.so lowers and refuses (compiling needs no device)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from having_fast_cases import (AGGREGATING, BY_NAME, H1, INSERT, PLAIN, having_ref, having_texts, kept_in,
                               predicate_job, with_having)
from rules_stream_cases import S2, compiled, stream_data
from siddhi_amd import abi, build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("name", list(BY_NAME))
def test_row_counts(name):
    hc = BY_NAME[name]
    plain, text, data, calls, rows0, rows1 = having_ref(hc)
    got = (len(rows0["seq"]), len(rows1["seq"]))
    print(name, got)
    assert got == hc[4]
    assert hc[1][2] > 16  # beyond the general engine's query table
    if name in AGGREGATING:
        assert rows0["values"].shape[1] == 3


def test_some_rows_kept_and_some_dropped():
    """a filter that does nothing, or drops everything, passes none of H1..H6"""
    for name, hc in BY_NAME.items():
        without, with_ = hc[4]
        if name == "H_ALL":
            assert with_ == without
        elif name == "H_NONE":
            assert with_ == 0
        else:
            assert 0 < with_ < without


# ---- the predicate on the CPU
@pytest.fixture(scope="module")
def having_host():
    d = os.path.join(HERE, "having_host")
    subprocess.run(["make", "-s", "-C", d], check=True)
    return os.path.join(d, "having_host")


def run_predicate(exe, desc, rows, path):
    predicate_job(desc, rows, path)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    lines = r.stdout.splitlines()
    lowered = [int(ln.split()[2]) for ln in lines if ln.startswith("q ")]
    mask = None
    for ln in lines:
        if ln.startswith("mask"):
            mask = np.frombuffer(ln[5:].encode(), np.uint8) == ord("1")
    return r.returncode, lowered, mask


@pytest.mark.parametrize("name", list(BY_NAME))
def test_cpu_predicate_reproduces_the_oracle(having_host, tmp_path, name):
    """the keep mask of the stand-alone program over the oracle's no-`having` rows is
    membership in its with-`having` rows, by (seq, query) and in order"""
    hc = BY_NAME[name]
    plain, text, data, calls, rows0, rows1 = having_ref(hc)
    want = kept_in(rows0, rows1)
    assert int(want.sum()) == hc[4][1]
    # the kept rows carry the values the unfiltered rows carry
    assert np.array_equal(rows0["values"][want], rows1["values"])
    assert np.array_equal(rows0["ts"][want], rows1["ts"])
    desc = compiled(hc[1], text).descriptor()
    rc, lowered, mask = run_predicate(having_host, desc, rows0, str(tmp_path / "job.bin"))
    assert rc == 0 and len(lowered) == hc[1][2] and all(1 <= n <= 32 for n in lowered), (rc, lowered)
    assert len(mask) == len(want)
    assert np.array_equal(mask, want), np.nonzero(mask != want)[0][:10]


def test_cpu_predicate_reads_null_flags(having_host, tmp_path):
    """a null flag on a compared column drops the row"""
    plain, text, data, calls, rows0, rows1 = having_ref(BY_NAME["H_ALL"])
    rows = {k: np.array(v, copy=True) for k, v in rows0.items()}
    rows["nulls"][::3, 1] = 1
    desc = compiled(S2, text).descriptor()
    rc, lowered, mask = run_predicate(having_host, desc, rows, str(tmp_path / "job.bin"))
    assert rc == 0
    want = np.ones(len(mask), bool)
    want[::3] = False
    assert np.array_equal(mask, want)


def _state_attr_text():
    text, rules, data = stream_data(S2)
    return with_having(text, lambda r: "e1.amount > 50.0")


def test_cpu_predicate_refuses_a_state_event_attribute(having_host, tmp_path):
    plain, text, data, calls, rows0, rows1 = having_ref(H1)
    desc = compiled(S2, _state_attr_text()).descriptor()
    rc, lowered, mask = run_predicate(having_host, desc, rows0, str(tmp_path / "job.bin"))
    assert rc == 2 and mask is None and all(n == -1 for n in lowered)


# ---- compile through libsiddhi_hip.so
@pytest.fixture(scope="module")
def lib():
    return abi.bind_product(C.CDLL(build.build()))


def _compile(lib, case, text):
    d = compiled(case, text).descriptor()
    h = C.c_void_p()
    rc = lib.sh_compile(C.byref(d), C.byref(h))
    err = lib.sh_last_error(h)
    return rc, h, err


@pytest.mark.parametrize("name", list(BY_NAME))
def test_having_sets_beyond_the_table_lower(lib, name):
    hc = BY_NAME[name]
    plain, text, data = having_texts(hc)
    rc, h, err = _compile(lib, hc[1], text)
    assert rc == abi.SH_OK, err
    lib.sh_destroy(h)


def test_a_state_event_attribute_is_still_unsupported(lib):
    """17 rules whose `having` reads e1.amount without selecting it"""
    rc, h, err = _compile(lib, S2, _state_attr_text())
    assert rc == abi.SH_E_UNSUPPORTED
    lib.sh_destroy(h)


def test_having_with_order_by_is_still_unsupported(lib):
    plain, text, data = having_texts(H1)
    ordered = text.replace(INSERT, " order by amount" + INSERT)
    assert ordered.count("order by") == S2[2]
    rc, h, err = _compile(lib, S2, ordered)
    assert rc == abi.SH_E_UNSUPPORTED
    lib.sh_destroy(h)


def _image_header_fingerprints(lib, texts):
    """the compiled-program fingerprints, read through shx_fingerprint"""
    out = []
    for t in texts:
        rc, h, err = _compile(lib, S2, t)
        assert rc == abi.SH_OK, err
        out.append(lib.shx_fingerprint(h))
        lib.sh_destroy(h)
    return out


def test_one_threshold_changes_the_fingerprint(lib):
    """two 17-rule sets that differ in one threshold; a set without `having` and the
    same set compiled twice agree with themselves"""
    plain, text, data = having_texts(H1)
    other = text.replace("having amount > 100.0", "having amount > 100.5")
    assert other != text and text.count("having amount > 100.0") == 1
    a, b, a2, p, p2 = _image_header_fingerprints(lib, [text, other, text, plain, plain])
    assert a == a2 and p == p2
    assert a != b and a != p and b != p
