"""The aggregate post-passes of siddhi_amd/csrc/sh_agg.hip on their own: sha_running
(the parallel pass that proves its own additions exact, or answers "not exact") and
shc_running (the carried, sequential pass), called through ctypes on the small planted
cases of tests/agg_post_cases.py and compared bit for bit with its plain reference; all
NaNs of a column count as one value. Every device buffer has exactly its stated size
plus a 64-word guard, all pre-filled with 0xA5, and the guards are checked after every
call; the scratch buffers are exactly sha_scratch_bytes / shc_scratch_bytes long.

The rule every sha_running call must keep: answer 0 and every aggregate column is the
reference's, every other column untouched; or answer 1 and the rows are bit for bit as
they were; never an error. Cases whose class (agg_post_cases.classify, derived from the
exactness argument, not from the kernels) is "accept" must answer 0, "refuse" 1; for
"either" the answer is printed.

Then the two gates as the engines reach them: the bucketed carry's (k_bk_aggp) one unit
on either side of 2^53 units, and a sum that overflows and comes back through
sh_run_device's ladder (2^1023, 2^1023, -2^1023: one significant bit at every step, so
only a test of the magnitude keeps the pass from answering 2^1023, inf, 2^1023 where the
reference stays at inf)."""
import ctypes as C

import numpy as np
import pytest

import agg_post_cases as ap
import device_prims as dp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _words(nbytes):
    return (int(nbytes) + 3) // 4


def _inputs(case, lo=0, hi=None):
    """the device buffers of the rows [lo, hi) of a case"""
    hi = case.m if hi is None else hi
    m = hi - lo
    b = dict(vals=dp.Dev(m * case.n_out * 2, case.vals[lo:hi]), seq=dp.Dev(m * 2, case.seq[lo:hi]))
    if case.query is not None:
        b["query"] = dp.Dev(m, case.query[lo:hi])
    if case.keys_table is not None:
        b["keys"] = dp.Dev(len(case.keys_table), case.keys_table)
    return b, m


def _desc(case):
    D = dp.sha_desc(n_cols=len(case.desc))
    for i, (col, kind, t) in enumerate(case.desc):
        D.c[i] = dp.sha_col(col, kind, t, 0)
    return D


def _ptr(b, name):
    return b[name].ptr if name in b else None


def _check_guards(bufs, what):
    for name, b in bufs.items():
        assert b.guard_ok(), f"{what}: guard of {name} ({b.words} words) overwritten"


def _first_diff(case, got, want):
    g, w = ap.canon(case, got), ap.canon(case, want)
    bad = np.argwhere(g != w)
    if not len(bad):
        return None
    r, c = bad[0].tolist()
    return f"{len(bad)} words differ, first at row {r} column {c}: got {int(g[r, c]):#x} want {int(w[r, c]):#x}"


def run_sha(case):
    """(rc, rows after the call)"""
    import torch
    L = dp.lib()
    b, m = _inputs(case)
    nbytes = L.sha_scratch_bytes(m, len(case.desc))
    b["scratch"] = dp.Dev(_words(nbytes))
    D = _desc(case)
    rc = L.sha_running(b["seq"].ptr, b["vals"].ptr, case.n_out, m, _ptr(b, "query"), case.n_query, _ptr(b, "keys"),
                       case.n_keys, case.seq_base, C.byref(D), b["scratch"].ptr, None)
    torch.cuda.synchronize()
    _check_guards(b, f"sha_running {case.name}")
    assert np.array_equal(b["seq"].read(np.uint64), case.seq), "sequence numbers changed"
    return rc, b["vals"].read(np.int64).reshape(m, case.n_out)


def check_sha(case):
    rc, got = run_sha(case)
    cls = ap.classify(case)
    print(f"sha_running {case.name}: m={case.m} class={cls} rc={rc}")
    assert rc in (0, 1), (case.name, rc)
    if rc == 1:
        assert np.array_equal(got, case.vals), f"{case.name}: refused, but the rows moved: " + \
            str(np.argwhere(got != case.vals)[:3].tolist())
    else:
        assert _first_diff(case, got, ap.stats(case)["ref"]) is None, \
            f"{case.name}: answered exact: " + _first_diff(case, got, ap.stats(case)["ref"])
    if cls != "either":
        assert rc == (0 if cls == "accept" else 1), (case.name, cls, rc, ap.stats(case)["mismatch"])
    return rc


@pytest.mark.parametrize("case", ap.CASES, ids=repr)
def test_sha_running(case):
    check_sha(case)


def test_sha_running_two_tiles_per_carry_thread():
    """1,026 tiles: every thread of the one carry workgroup walks two"""
    assert check_sha(ap.big_case()) == 0


def run_shc(case, lo=0, hi=None, table=None):
    """one shc_running call over the rows [lo, hi); returns (rows, buffers, put pointers)"""
    import torch
    L = dp.lib()
    b, m = _inputs(case, lo, hi)
    nbytes = L.shc_scratch_bytes(m, len(case.desc))
    b["scratch"] = dp.Dev(_words(nbytes))
    D = _desc(case)
    pk, ps = C.c_void_p(), C.c_void_p()
    # the sequence numbers of the slice look their keys up from the same base
    rc = L.shc_running(b["seq"].ptr, b["vals"].ptr, case.n_out, m, _ptr(b, "query"), case.n_query, None,
                       _ptr(b, "keys"), case.n_keys, case.seq_base, C.byref(D),
                       C.byref(table) if table is not None else None, b["scratch"].ptr, None, C.byref(pk), C.byref(ps))
    torch.cuda.synchronize()
    assert rc == 0, (case.name, rc)
    _check_guards(b, f"shc_running {case.name}")
    s0 = b["scratch"].ptr
    assert s0 <= pk.value and pk.value + m * 8 <= s0 + nbytes, "put_keys outside the scratch"
    assert s0 <= ps.value and ps.value + m * len(case.desc) * 16 <= s0 + nbytes, "put_state outside the scratch"
    return b["vals"].read(np.int64).reshape(m, case.n_out), b, (pk, ps)


@pytest.mark.parametrize("case", ap.CASES, ids=repr)
def test_shc_running_without_a_table(case):
    """the sequential pass needs no proof: the refused cases included"""
    got, _, _ = run_shc(case)
    d = _first_diff(case, got, ap.stats(case)["ref"])
    assert d is None, f"{case.name}: {d}"


@pytest.mark.parametrize("arg_type", [ap.DOUBLE, ap.FLOAT], ids=["double", "float"])
def test_shc_running_on_salted_values(arg_type):
    """NaN, the infinities, DBL_MAX / FLT_MAX: carried the way the reference's additions carry them"""
    case = ap.salted_case(arg_type)
    got, _, _ = run_shc(case)
    d = _first_diff(case, got, ap.reference(case))
    assert d is None, d
    rc, rows = run_sha(case)                      # the parallel pass sees the NaN / infinite addends
    assert rc == 1 and np.array_equal(rows, case.vals)


def test_shc_running_carries_through_a_table():
    """two calls with shc_put between them are one sequential pass over all the rows"""
    import torch
    L = dp.lib()
    case, cut = ap.split_case()
    g = case.group()
    first, second = set(g[:cut].tolist()), set(g[cut:].tolist())
    assert first - second and second - first and first & second
    nc = len(case.desc)
    cap = 1
    while cap < 2 * case.m:
        cap *= 2
    keys = dp.Dev(cap * 2, np.full(cap, -1, np.int64))              # SHQ_EMPTY
    state = dp.Dev(cap * nc * 4, np.zeros(cap * nc * 2, np.int64))
    ctl = dp.Dev(4, np.zeros(2, np.int64))                          # entries, error
    T = dp.shq_table(keys.ptr, state.ptr, cap, nc, 0)
    got1, b1, (pk, ps) = run_shc(case, 0, cut, T)
    assert L.shc_put(C.byref(T), pk.value, ps.value, cut, ctl.ptr, ctl.ptr + 8, None) == 0
    torch.cuda.synchronize()
    _check_guards(dict(table_keys=keys, table_state=state, ctl=ctl, **b1), "shc_put")
    assert ctl.read(np.int64).tolist() == [len(first), 0]
    got2, b2, _ = run_shc(case, cut, case.m, T)
    _check_guards(dict(table_keys=keys, table_state=state, ctl=ctl), "second call")
    d = _first_diff(case, np.concatenate([got1, got2]), ap.reference(case))
    assert d is None, d
    # (without the table the second call starts every segment from zero: other values)
    fresh, _, _ = run_shc(case, cut, case.m, None)
    assert _first_diff(case, fresh, ap.reference(case)[cut:]) is not None


# ------------------------------------------------------------------ the gates as the engines reach them
def _device_rows(app, ts, k, cols, nk):
    import torch
    from siddhi_amd import compiler
    from siddhi_amd.device_run import DeviceRunner
    r = DeviceRunner(compiler.compile_app(app))
    dev = torch.device("cuda:0")
    tk = torch.from_numpy(k).to(dev)
    res = r.run(torch.from_numpy(ts).to(dev), tk, [tk] + [torch.from_numpy(c).to(dev) for c in cols[1:]], nk)
    torch.cuda.synchronize()
    st = dict(agg=r.agg_status(), bucket=r.bucket_status(), err=r.last_error())
    got = dict(seq=res[1].cpu().numpy(), values=res[2].cpu().numpy())
    types = list(r.out_types)
    assert res[0] == len(got["seq"])
    r.close()
    return got, st, types


@pytest.mark.parametrize("which", ["below", "above"])
def test_bucketed_carry_gate_at_two_to_the_53_units(which):
    """one key's sum(e2.price) reaches 2^29 - 2^-24 = 2^53 - 1 units (k_bk_aggp keeps the
    run, agg_status 5) or 2^29 + 2^-24 = 2^53 + 1 units, whose conversion to a double
    rounds to 2^53: a `>` in place of the gate's `>=` would keep it. The run must leave
    k_bk_aggp, and the rows are the oracle's either way"""
    import edge_values as ev
    ts, k, p, v, kk = ap.bk_gate_stream(which)
    ref = ap.bk_gate_ref(which)
    got, st, types = _device_rows(ap.BK_GATE_APP, ts, k, [k, p, v], ap.BK_SHAPE[1])
    print(f"k_bk_aggp gate {which}: rows={len(got['seq'])} status={st}")
    ev.assert_rows_equal(got, ref, types, which)
    assert (st["agg"] == 5) == (which == "below"), st
    if which == "below":
        assert st["bucket"] == 1, st


def test_overflow_and_back_through_the_ladder():
    """a key's total goes to infinity and then takes -2^1023: whichever pass forms the
    values (agg_status printed), they are the oracle's"""
    import edge_values as ev
    ts, k, p, v, kk = ap.overflow_stream()
    ref = ap.overflow_ref()
    got, st, types = _device_rows(ap.overflow_app(), ts, k, [k, p, v], ap.BK_SHAPE[1])
    print(f"overflow and back: rows={len(got['seq'])} status={st}")
    ev.assert_rows_equal(got, ref, types, "overflow")
