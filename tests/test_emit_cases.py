"""The premises of tests/test_gpu_emit.py, checked without a GPU.

1. The burst stream of tests/emit_cases.py reaches, by the oracle's per-event row counts,
   every row path of k_bk_emit in both of its occupancy forms: halves of 512 events with
   no row, with rows the 6-wave form's map holds (<= 512), with rows only the 4-wave
   form's map holds (513..1,024: row-parallel there, event-parallel in the 6-wave form)
   and with more (event-parallel in both); consumers inside the matcher's 15-step mask
   and beyond it; none above the 255 rows a count byte holds.
2. The packed layout restated from include/siddhi_hip.h is sh_packed_row_layout's.
3. The gfx950 matcher builds for every match-stream set of the select lists.
4. The lists reach each of {raw, packed, columns} x {6-wave, 4-wave}, every unrolled
   width and the generic path."""
import ctypes as C

import numpy as np
import pytest

import emit_cases as ec
from siddhi_amd import abi, build, compiler

NKS = [1024, 600]     # the bucketed engine's stream and the conversion kernels'


@pytest.fixture(scope="module")
def product():
    return abi.bind_product(C.CDLL(build.build()))


@pytest.mark.parametrize("nk", NKS)
def test_burst_stream_reaches_every_row_class(nk):
    R = ec.half_rows(nk)
    classes = {"none": R == 0, "map6": (R > 0) & (R <= ec.ROWS_6W),
               "map4_only": (R > ec.ROWS_6W) & (R <= ec.ROWS_4W), "dense": R > ec.ROWS_4W}
    got = {k: int(v.sum()) for k, v in classes.items()}
    print(f"nk={nk}: events={len(ec.burst_stream(nk)[0])} rows={int(R.sum())} halves={got}")
    assert all(v >= 2 for v in got.values()), got
    c = ec.event_counts(nk)
    assert (c > 15).any() and ((c > 0) & (c <= 15)).any()
    assert c.max() <= 255
    # the last tile is partial and there is more than one
    n = len(c)
    assert n > 8192 and n % 8192 != 0


def test_burst_stream_reaches_both_forms_of_the_match_stream_write():
    """The matcher marks a consumed partial met at walk step 15 or later (SHB_MSTEPS) with
    SHB_MOVF, and a pass with such a consumer writes its e1-side values by walking again;
    a pass without one writes a single 4-byte column in the coalesced staged form, any
    other set straight from the mask. A pass is one key bucket (key & 255) over a run of
    tiles; this stream has fewer events per bucket than a pass holds, so a bucket is one
    pass. Both kinds of bucket exist, and rows come from both"""
    nk = 1024
    _, keys, _ = ec.burst_stream(nk)
    seq, _ = ec.wide_rows(nk)
    step = ec.walk_steps(nk)
    assert step.min() == 0 and step.max() >= 15
    per_bucket = np.bincount(keys & 255, minlength=256)
    assert per_bucket.max() <= 512                     # well below SHB_CH, a pass's consumers
    slow = np.zeros(256, bool)
    slow[np.unique(keys[seq[step >= 15]] & 255)] = True
    rows = np.bincount(keys[seq] & 255, minlength=256)
    print(f"buckets with a consumer beyond the mask: {int(slow.sum())}, without: {int((~slow).sum())} "
          f"({int(rows[~slow].sum())} rows)")
    assert slow.sum() >= 4 and (~slow).sum() >= 4
    assert rows[~slow].min() > 0


def test_burst_stream_is_the_same_for_every_caller():
    a, b = ec.burst_stream(1024), ec.burst_stream(1024)
    assert all(x is y for x, y in zip(a[2], b[2]))
    assert not a[2][1].flags.writeable


def test_wide_rows_hold_what_the_events_hold():
    """the one oracle run the expectations are cut from: every e2-side value is the
    consuming event's attribute, every e1-side value an earlier event's of the same key
    with a lower price above 20"""
    nk = 1024
    ts, keys, cols = ec.burst_stream(nk)
    seq, vals = ec.wide_rows(nk)
    assert len(seq) > 0 and (np.diff(seq) >= 0).all()
    for a, name in enumerate(ec.ATTRS):
        t = ec.ATTR_TYPE[name]
        col = cols[a][seq]
        e2 = vals[:, ec.WIDE_POS[(2, name)]]
        if t == ec.FLOAT:
            want = col.view(np.uint32).astype(np.int64)
        elif t == ec.DOUBLE:
            want = col.view(np.int64)
        else:
            want = col.astype(np.int64)
        assert np.array_equal(e2, want), name
    assert np.array_equal(vals[:, ec.WIDE_POS[(1, "sym")]], vals[:, ec.WIDE_POS[(2, "sym")]])
    p1 = (vals[:, ec.WIDE_POS[(1, "price")]] & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
    p2 = cols[1][seq]
    assert (p1 > 20).all() and (p2 > p1).all()
    # the columns are random over their whole ranges: both halves of an 8-byte value and
    # every byte of a 4-byte one differ from each other somewhere
    v1 = vals[:, ec.WIDE_POS[(1, "volume")]]
    assert ((v1 >> 32) != (v1 & 0xFFFFFFFF)).any() and (v1 < 0).any() and (v1 > 2 ** 32).any()
    assert set(np.unique(vals[:, ec.WIDE_POS[(1, "flag")]]).tolist()) == {0, 1}


ALL_LISTS = dict(ec.CASES, five_ms=ec.FIVE_MS)


def _handle(product, values, nk=1024):
    d = compiler.compile_app(ec.app(values), ec.strings(nk)).descriptor()
    h = C.c_void_p()
    assert product.sh_compile(C.byref(d), C.byref(h)) == abi.SH_OK, product.sh_last_error(h)
    return h


@pytest.mark.parametrize("name", list(ALL_LISTS))
def test_packed_layout_restatement(name, product):
    values = ALL_LISTS[name]
    h = _handle(product, values)
    offs = (C.c_int32 * 16)()
    n, rb = C.c_int32(), C.c_int32()
    rc = product.sh_packed_row_layout(h, offs, 16, C.byref(n), C.byref(rb))
    product.sh_destroy(h)
    assert rc == abi.SH_OK
    want_offs, want_rb = ec.packed_layout(ec.types_of(values))
    assert n.value == len(values)
    assert [offs[i] for i in range(n.value)] == want_offs
    assert rb.value == want_rb


def test_packed_layout_by_hand():
    """worked from the header's sentence, not from any code"""
    T = ec.types_of
    assert ec.packed_layout(T(ec.CASES["w1_e2_price"])) == ([8], 16)
    assert ec.packed_layout(T(ec.CASES["w1_e1_volume"])) == ([8], 16)
    assert ec.packed_layout(T(ec.CASES["w1_e1_flag"])) == ([8], 16)
    assert ec.packed_layout(T(ec.CASES["w2_int_long"])) == ([8, 16], 32)               # a pad word at 12
    assert ec.packed_layout(T(ec.CASES["w3_bool_float_double"])) == ([8, 12, 16], 32)
    assert ec.packed_layout(T(ec.CASES["w4_two_wide_ms"])) == ([8, 16, 24, 32], 48)    # int at 16, pad at 20
    assert ec.packed_layout(T(ec.CASES["w8_all_wide"])) == ([8 * (1 + o) for o in range(8)], 80)


def test_encoders_by_hand():
    raw = np.array([[0x3F800000, -2, 1, np.float64(-1.5).view(np.int64), -(2 ** 40) + 3]], dtype=np.int64)
    types = [ec.FLOAT, ec.INT, ec.BOOL, ec.DOUBLE, ec.LONG]
    cols = ec.expected_columns(raw, types)
    assert [c.shape[1] for c in cols] == [4, 4, 1, 8, 8]
    assert cols[0].view(np.float32)[0, 0] == 1.0 and cols[1].view(np.int32)[0, 0] == -2
    assert cols[2][0, 0] == 1 and cols[3].view(np.float64)[0, 0] == -1.5
    assert cols[4].view(np.int64)[0, 0] == -(2 ** 40) + 3
    fields = ec.expected_packed_fields(np.array([77], np.int64), raw, types)
    assert [(off, b.shape[1]) for off, b in fields] == [(0, 8), (8, 4), (12, 4), (16, 4), (24, 8), (32, 8)]
    assert fields[0][1].view(np.int64)[0, 0] == 77
    assert fields[3][1].tolist() == [[1, 0, 0, 0]]


@pytest.mark.parametrize("name", ec.BUCKETED)
def test_matcher_builds(name, product):
    """shb_match for the list's match-stream set compiles for gfx950"""
    h = _handle(product, ec.CASES[name])
    rc = product.shx_bucket_compile(h, None, 0)
    err = product.sh_last_error(h)
    product.sh_destroy(h)
    assert rc == abi.SH_OK, err


def test_match_stream_sets():
    """the forms of the matcher's e1-side writes (sh_jit.cpp gen_bucket): no column, one
    column of 4 bytes (the staged form) as float and as int, one of 8 bytes, one of 1 byte,
    and 2, 3 and 4 columns; five for the refusal"""
    W = {a: ec.NATURAL[t] for a, t in ec.ATTR_TYPE.items()}
    sets = {name: [W[a] for a in ec.ms_attrs(v)] for name, v in ec.CASES.items()}
    have = {tuple(s) for s in sets.values()}
    assert () in have and (8,) in have and (1,) in have
    assert sets["w2_int_long"] == [4] and sets["w3_bool_float_double"] == [4]
    assert {len(s) for s in sets.values()} == {0, 1, 2, 3, 4}
    assert sorted(sets["w7_mixed_ms"]) == [1, 4, 4]
    assert max(len(s) for s in sets.values()) == 4        # SHB_MAX_MS
    assert len(ec.ms_attrs(ec.FIVE_MS)) == 5 and "sym" not in ec.ms_attrs(ec.FIVE_MS)
    assert (1, "sym") in ec.CASES["w5_sym"] and len(ec.ms_attrs(ec.CASES["w5_sym"])) == 2


def test_instantiation_coverage():
    widths = {len(v) for v in ec.CASES.values()}
    assert set(range(1, 9)) <= widths and 9 in widths and 16 in widths     # 1..8 unrolled, generic, SHB_MAX_OUT
    forms = {(lay, ec.six_waves(lay, len(v))) for lay in ec.LAYOUTS for v in ec.CASES.values()}
    assert forms == {(lay, six) for lay in ec.LAYOUTS for six in (True, False)}
    # the thresholds of bk_ru_lm (sh_bucket.hip), as data
    assert ec.six_waves("raw", 5) and not ec.six_waves("raw", 6)
    assert ec.six_waves("packed", 5) and not ec.six_waves("packed", 6)
    assert ec.six_waves("columns", 2) and not ec.six_waves("columns", 3)
    assert all(ec.six_waves(lay, 9) and ec.six_waves(lay, 16) for lay in ec.LAYOUTS)
    # a bool and an 8-byte value appear on both sides
    for side in (1, 2):
        assert any((side, "flag") in v for v in ec.CASES.values())
        assert any((side, "volume") in v for v in ec.CASES.values())
