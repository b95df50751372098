"""Every select width (1..8 unrolled, the generic 9..16 path), row layout (raw, packed,
typed columns), occupancy form and row path of k_bk_emit, the match-stream forms of the
hipRTC matcher that feed it, and the conversions k_pack_rows / k_narrow_rows of the
engines that write raw rows -- against the oracle's rows of the burst stream
(tests/emit_cases.py; its premises are checked in tests/test_emit_cases.py).

The runner below drives sh_run_device_v2 as DeviceRunner.run does, but owns the outputs:
each is one allocation of capacity rows plus a guard of 64 rows (64 elements per typed
column and for d_out_seq), filled with 0xA5 before every call. A row the device skips
shows as 0xA5 bytes instead of passing on what an earlier run left in recycled memory,
and a write past the capacity shows in the guard, inside the allocation.

Compared bit for bit: the sequence numbers and every value field (emit_cases restates the
packed layout from include/siddhi_hip.h; padding bytes are not compared)."""
import ctypes as C

import numpy as np
import pytest

import emit_cases as ec
from siddhi_amd import abi, compiler

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_dev_streams = {}


def device_stream(nk):
    """the burst stream's columns on the device, uploaded once per key count"""
    import torch
    if nk not in _dev_streams:
        dev = torch.device("cuda:0")
        ts, keys, cols = ec.burst_stream(nk)
        up = {id(keys): torch.from_numpy(np.array(keys)).to(dev)}
        dcols = [up.setdefault(id(c), torch.from_numpy(np.array(c)).to(dev)) for c in cols]
        _dev_streams[nk] = (torch.from_numpy(np.array(ts)).to(dev), up[id(keys)], dcols)
    return _dev_streams[nk]


class Runner:
    """one compiled select list on one stream; run() is one sh_run_device_v2 call"""

    def __init__(self, values, nk):
        from siddhi_amd._native import CompiledHandle, lib
        self.lib = lib()
        self.values, self.nk = values, nk
        self.types = ec.types_of(values)
        self.handle = CompiledHandle(compiler.compile_app(ec.app(values), ec.strings(nk)))

    def close(self):
        self.handle.close()

    def bucket_status(self):
        return self.lib.shx_bucket_status(self.handle.h)

    def run(self, layout, capacity, guard=GUARD):
        """(rc, out_count, {name: uint8 host array of the WHOLE allocation, guard included})"""
        import torch
        dev = torch.device("cuda:0")
        ts, keys, cols = device_stream(self.nk)
        no = len(self.values)
        rows = capacity + guard

        def alloc(nbytes):
            return torch.full((nbytes,), FILL, dtype=torch.uint8, device=dev)

        r = abi.sh_device_run()
        r.version = abi.SH_DEVICE_RUN_V2
        r.n = ts.numel()
        r.d_ts = ts.data_ptr()
        r.d_keys = keys.data_ptr()
        r.n_keys = self.nk
        r.batch_events = ec.BATCH
        r.d_cols = (C.c_void_p * len(cols))(*[c.data_ptr() for c in cols])
        r.out_capacity = capacity
        r.stream = torch.cuda.current_stream(dev).cuda_stream
        out = {}
        if layout == "packed":
            _, rb = ec.packed_layout(self.types)
            out["rows"] = alloc(rows * rb)
            r.out_layout = abi.SH_OUT_PACKED
            r.d_out_values = out["rows"].data_ptr()
        else:
            out["seq"] = alloc(rows * 8)
            r.d_out_seq = out["seq"].data_ptr()
            if layout == "raw":
                out["vals"] = alloc(rows * no * 8)
                r.d_out_values = out["vals"].data_ptr()
            else:
                for o, t in enumerate(self.types):
                    out[f"col{o}"] = alloc(rows * ec.NATURAL[t])
                keep = (C.c_void_p * no)(*[out[f"col{o}"].data_ptr() for o in range(no)])
                r.d_out_cols = keep
        torch.cuda.synchronize()
        rc = self.lib.sh_run_device_v2(self.handle.h, C.byref(r))
        torch.cuda.synchronize()
        return rc, int(r.out_count), {k: v.cpu().numpy() for k, v in out.items()}

    def error(self):
        return self.lib.sh_last_error(self.handle.h).decode()


def _widths(layout, types):
    """bytes per row of every output allocation of a layout"""
    if layout == "packed":
        return {"rows": ec.packed_layout(types)[1]}
    if layout == "raw":
        return {"seq": 8, "vals": 8 * len(types)}
    return dict({"seq": 8}, **{f"col{o}": ec.NATURAL[t] for o, t in enumerate(types)})


def assert_guard(out, layout, types, capacity, what, guard=GUARD):
    """no byte past `capacity` rows was written, in any output"""
    for name, w in _widths(layout, types).items():
        g = out[name][capacity * w:]
        assert len(g) == guard * w
        bad = np.nonzero(g != FILL)[0]
        assert len(bad) == 0, (what, name, "first written guard byte at row", capacity + int(bad[0]) // w)


def _same(got, want, what, field):
    assert got.shape == want.shape, (what, field, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (what, field, f"{len(bad)} rows differ, first {int(bad[0])}",
                           got[bad[0]].tolist(), want[bad[0]].tolist())


def assert_rows(out, layout, types, seq, raw, what):
    """the first len(seq) rows of every output are the expected ones, bit for bit"""
    m = len(seq)
    if layout == "packed":
        rb = ec.packed_layout(types)[1]
        rows = out["rows"][:m * rb].reshape(m, rb)
        for off, want in ec.expected_packed_fields(seq, raw, types):
            _same(rows[:, off:off + want.shape[1]], want, what, f"packed bytes {off}..{off + want.shape[1]}")
        return
    _same(out["seq"][:m * 8].reshape(m, 8), seq.astype("<i8").view(np.uint8).reshape(m, 8), what, "seq")
    if layout == "raw":
        no = len(types)
        _same(out["vals"][:m * no * 8].view("<i8").reshape(m, no), raw, what, "raw values")
    else:
        for o, want in enumerate(ec.expected_columns(raw, types)):
            w = want.shape[1]
            _same(out[f"col{o}"][:m * w].reshape(m, w), want, what, f"column {o}")


def check_run(values, nk, layout, status, what):
    seq, raw = ec.expected_raw(nk, values)
    types = ec.types_of(values)
    r = Runner(values, nk)
    try:
        rc, count, out = r.run(layout, len(seq))      # room for exactly the rows: the guard follows the last
        st = r.bucket_status()
        print(f"{what}: rc={rc} rows={count} bucket_status={st} err={r.error()!r}")
        assert rc == abi.SH_OK, r.error()
        assert st == status, (what, st, r.error())
        assert count == len(seq) > 0
        assert_rows(out, layout, types, seq, raw, what)
        assert_guard(out, layout, types, len(seq), what)
    finally:
        r.close()


@pytest.mark.parametrize("layout", ec.LAYOUTS)
@pytest.mark.parametrize("name", ec.BUCKETED)
def test_bucketed_rows(name, layout):
    """k_bk_emit<layout, width, form> on 1,024 keys: the halves of the burst stream take
    the row-parallel path, the event-parallel path of the 6-wave form alone (513..1,024
    rows) and of both forms; the matcher writes the list's e1-side values in its form for
    that match-stream set, through the 15-step mask and beyond it. Status 1: a fallback
    must not stand in for the emitter"""
    check_run(ec.CASES[name], 1024, layout, 1, f"bucketed {name} {layout}")


@pytest.mark.parametrize("layout", ["packed", "columns"])
@pytest.mark.parametrize("name", ec.BUCKETED)
def test_conversion_rows(name, layout):
    """below 1,024 keys the window engine writes raw rows into a workspace and
    k_pack_rows<width> / k_narrow_rows convert them into the caller's layout"""
    check_run(ec.CASES[name], 600, layout, 0, f"conversion {name} {layout}")


@pytest.mark.parametrize("layout", ec.LAYOUTS)
def test_five_match_stream_columns_fall_back(layout):
    """five e1-side attributes are more than SHB_MAX_MS: the bucketed engine refuses the
    list before building a matcher, and the rows are still exact"""
    assert len(ec.ms_attrs(ec.FIVE_MS)) == 5
    check_run(ec.FIVE_MS, 1024, layout, 0, f"five match-stream columns {layout}")


def _cut_rows(nk):
    """(a row inside a half both forms write event-parallel, a row inside a half both write
    row-parallel), from the oracle's counts: past the half's middle, inside an event's rows
    where the half has such an event, with rows of the stream left after it"""
    R = ec.half_rows(nk)
    c = ec.event_counts(nk)
    first = np.concatenate([[0], np.cumsum(R)])
    total = int(first[-1])

    def cut(h):
        ev = np.arange(h * ec.HALF, min(len(c), (h + 1) * ec.HALF))
        start = np.concatenate([[0], np.cumsum(c[ev])])[:-1] + first[h]       # first row of each event
        mid = first[h] + R[h] // 2
        multi = [int(start[i]) + 1 for i in range(len(ev)) if c[ev[i]] >= 3 and start[i] + 1 >= mid]
        row = multi[0] if multi else int(mid) + 1
        assert first[h] < row < first[h + 1] and row < total
        return row

    dense = [h for h in range(len(R)) if R[h] > ec.ROWS_4W]
    sparse = [h for h in range(len(R)) if 128 <= R[h] <= ec.ROWS_6W]
    assert dense and sparse
    return {"dense": cut(dense[len(dense) // 2]), "row_parallel": cut(sparse[len(sparse) // 2])}


@pytest.mark.parametrize("where", ["dense", "row_parallel"])
@pytest.mark.parametrize("layout", ec.LAYOUTS)
@pytest.mark.parametrize("name", ["w2_int_long", "w8_all_wide"])      # 6 waves / 4 waves in every layout
def test_capacity_is_a_hard_bound(name, layout, where):
    """out_capacity cut inside a half: SH_E_MORE, out_count is the whole total, and no byte
    past the capacity is written (the rows below the cut are not promised and not
    compared); the same handle then gives the exact rows with room for them"""
    values, nk = ec.CASES[name], 1024
    assert ec.six_waves(layout, len(values)) == (name == "w2_int_long")
    seq, raw = ec.expected_raw(nk, values)
    types = ec.types_of(values)
    cap = _cut_rows(nk)[where]
    what = f"capacity {name} {layout} {where} cut at row {cap} of {len(seq)}"
    r = Runner(values, nk)
    try:
        # the guard reaches past the last row of the stream: an emitter that ignored the
        # capacity altogether would still write inside the allocation, and show here
        guard = len(seq) - cap + GUARD
        rc, count, out = r.run(layout, cap, guard=guard)
        print(f"{what}: rc={rc} out_count={count}")
        assert rc == abi.SH_E_MORE, (what, rc, r.error())
        assert count == len(seq)
        assert_guard(out, layout, types, cap, what, guard=guard)
        rc, count, out = r.run(layout, len(seq))
        assert rc == abi.SH_OK, r.error()
        assert r.bucket_status() == 1
        assert count == len(seq)
        assert_rows(out, layout, types, seq, raw, what)
        assert_guard(out, layout, types, len(seq), what)
    finally:
        r.close()
