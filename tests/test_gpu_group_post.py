"""The `group by` segment pass of siddhi_amd/csrc/sh_group.hip (shg_segments) and
sha_running_grouped of sh_agg.hip on their own, called through ctypes on the shapes of
tests/group_post_cases.py. The pass's sidx / sseg are compared with the numpy contract
(group_post_cases.segments_ref), the running values bit for bit with the per-segment
left-to-right restatement of tests/agg_post_cases.py over the grouped segments. Every
device buffer has exactly its stated size plus a 64-word guard, all pre-filled with 0xA5,
and the guards are checked after every call; the scratch buffers are exactly
shg_scratch_bytes / sha_grouped_scratch_bytes long.

sha_running_grouped keeps sha_running's rule: answer 0 and every aggregate column is the
restatement's, every other column untouched; or answer 1 and the rows are bit for bit as
they were. The class of every case comes from exact integers (group_post_cases.classify).
It runs at the sizes RUN_SIZES: the restatement walks every segment in Python; the tail
beyond 1,024 scan tiles is tests/test_gpu_agg_post.py's."""
import ctypes as C

import numpy as np
import pytest

import agg_post_cases as ap
import device_prims as dp
import group_post_cases as gp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def L():
    return gp.bind(dp.lib())


def _words(nbytes):
    return (int(nbytes) + 3) // 4


def _inputs(case):
    m = case.m
    b = dict(vals=dp.Dev(m * case.n_out * 2, case.vals), seq=dp.Dev(m * 2, case.seq),
             keys=dp.Dev(len(case.keys_table), case.keys_table))
    if case.query is not None:
        b["query"] = dp.Dev(m, case.query)
    return b


def _ptr(b, name):
    return b[name].ptr if name in b else None


def _check_guards(bufs, what):
    for name, b in bufs.items():
        assert b.guard_ok(), f"{what}: guard of {name} ({b.words} words) overwritten"


def run_segments(L, case):
    """(sidx, sseg) as the device wrote them"""
    import torch
    m = case.m
    b = _inputs(case)
    nbytes = L.shg_scratch_bytes(m)
    b["scratch"] = dp.Dev(_words(nbytes))
    G = gp.descriptor(case.groups)
    sseg, sidx = C.c_void_p(1), C.c_void_p(1)
    rc = L.shg_segments(b["seq"].ptr, b["vals"].ptr, case.n_out, m, _ptr(b, "query"), case.n_query, b["keys"].ptr,
                        case.n_keys, case.seq_base, C.byref(G), b["scratch"].ptr, None, C.byref(sseg), C.byref(sidx))
    torch.cuda.synchronize()
    assert rc == 0, (case.name, rc)
    _check_guards(b, f"shg_segments {case.name}")
    assert np.array_equal(b["vals"].read(np.int64).reshape(m, case.n_out), case.vals), "the rows changed"
    if m == 0:
        assert sseg.value is None and sidx.value is None and b["scratch"].untouched(), "m = 0 wrote"
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    s0 = b["scratch"].ptr
    ws = b["scratch"].read()
    out = []
    for p in (sidx, sseg):
        assert s0 <= p.value and p.value + m * 4 <= s0 + nbytes and (p.value - s0) % 4 == 0, "outside the scratch"
        at = (p.value - s0) // 4
        out.append(ws[at:at + m].copy())
    return out


def _diff(got, want):
    d = np.flatnonzero(got != want)
    return f"{len(d)} differ, first at {d[:3]}: got {got[d[:3]]} want {want[d[:3]]}"


@pytest.mark.parametrize("m", gp.SIZES)
@pytest.mark.parametrize("shape", gp.SHAPES)
def test_segments(L, shape, m):
    case = gp.shape_case(shape, m)
    sidx, sseg = run_segments(L, case)
    want_idx, want_seg = gp.segments_ref(case.vals, case.query, case.key, case.n_keys, case.groups)
    assert np.array_equal(sidx, want_idx), f"{case.name}: sidx " + _diff(sidx, want_idx)
    assert np.array_equal(sseg, want_seg), f"{case.name}: sseg " + _diff(sseg, want_seg)


def run_grouped(L, case):
    """(rc, rows after the call)"""
    import torch
    m = case.m
    b = _inputs(case)
    b["scratch"] = dp.Dev(_words(L.sha_grouped_scratch_bytes(m, len(case.desc))))
    D = dp.sha_desc(n_cols=len(case.desc))
    for i, (col, kind, t) in enumerate(case.desc):
        D.c[i] = dp.sha_col(col, kind, t, 0)
    G = gp.descriptor(case.groups)
    rc = L.sha_running_grouped(b["seq"].ptr, b["vals"].ptr, case.n_out, m, _ptr(b, "query"), case.n_query,
                               b["keys"].ptr, case.n_keys, case.seq_base, C.byref(D), C.byref(G), b["scratch"].ptr,
                               None)
    torch.cuda.synchronize()
    _check_guards(b, f"sha_running_grouped {case.name}")
    assert np.array_equal(b["seq"].read(np.uint64), case.seq), "sequence numbers changed"
    return rc, b["vals"].read(np.int64).reshape(m, case.n_out)


def check_grouped(L, case):
    rc, got = run_grouped(L, case)
    cls = gp.classify(case)
    print(f"sha_running_grouped {case.name}: m={case.m} class={cls} rc={rc}")
    assert rc == (0 if cls == "accept" else 1), (case.name, cls, rc)
    if rc == 1:
        assert np.array_equal(got, case.vals), f"{case.name}: refused, but the rows moved: " + \
            str(np.argwhere(got != case.vals)[:3].tolist())
        return
    g, w = ap.canon(case, got), ap.canon(case, ap.reference(case))
    bad = np.argwhere(g != w)
    assert not len(bad), f"{case.name}: {len(bad)} words differ, first at {bad[0].tolist()}: " \
                         f"got {int(g[tuple(bad[0])]):#x} want {int(w[tuple(bad[0])]):#x}"


@pytest.mark.parametrize("m", gp.RUN_SIZES)
@pytest.mark.parametrize("shape", gp.SHAPES)
def test_running_grouped(L, shape, m):
    check_grouped(L, gp.shape_case(shape, m))


@pytest.mark.parametrize("split", [False, True], ids=["joined", "split"])
def test_running_grouped_planted(L, split):
    """2^53 and 1.0 in one group: answer 1, the rows as they were; in two groups of the
    same key: answer 0"""
    check_grouped(L, gp.planted(split))


def test_grouped_differs_from_ungrouped():
    """the restatement itself: on the interleaved shape the grouped running values are not
    the (query, key) ones, so a pass that ignored the groups could not pass above"""
    c = gp.shape_case("interleave", 2049)
    flat = gp.GCase("flat", c.vals, c.desc, None, 1, c.key, c.n_keys, [[]], seq_base=c.seq_base)
    assert not np.array_equal(ap.reference(c), ap.reference(flat))
