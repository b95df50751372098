"""Select widths, row layouts and match-stream forms of the bucketed emitter
(k_bk_emit, bk_pack, bk_store in siddhi_amd/csrc) and of the row conversions
(k_pack_rows, k_narrow_rows): a burst stream whose 512-event halves fall into
every row-count class of the emitter, twelve select lists, and the expected
rows in each of the three output layouts.

The expectation of every list is a column selection of ONE oracle run per
stream with all twelve e1.* / e2.* attributes selected: which events match does
not depend on the select list. The packed layout is restated here from the text
of include/siddhi_hip.h (sh_device_run.out_layout), never taken from
sh_packed_row_layout or siddhi_amd.device_run.packed_to_raw.

No GPU is needed to import this module."""
import numpy as np

from oracle_engine import OracleEngine
from siddhi_amd import compiler

STRING, INT, LONG, FLOAT, DOUBLE, BOOL = (compiler.STRING, compiler.INT, compiler.LONG, compiler.FLOAT,
                                          compiler.DOUBLE, compiler.BOOL)
ATTRS = ["sym", "price", "volume", "x", "d", "flag"]
ATTR_TYPE = {"sym": STRING, "price": FLOAT, "volume": LONG, "x": INT, "d": DOUBLE, "flag": BOOL}
S_DEF = "define stream S (sym string, price float, volume long, x int, d double, flag bool); "
HALF = 512          # events of one row-map pass of an emitter wave (BK_EHALF)
ROWS_6W = 512       # rows a half's row map holds in the 6-wave form, 1,024 in the 4-wave form
ROWS_4W = 1024
BATCH = 4096        # events per send(Event[]) call


def app(values):
    """values: [(side, attribute)], side 1 / 2 for e1 / e2"""
    sel = ", ".join(f"e{s}.{a} as v{o}" for o, (s, a) in enumerate(values))
    return (S_DEF + "partition with (sym of S) begin @info(name = 'query1') "
            "from every e1=S[price > 20] -> e2=S[price > e1.price] within 1 sec "
            f"select {sel} insert into Out; end;")


def types_of(values):
    return [ATTR_TYPE[a] for _, a in values]


WIDE = [(s, a) for s in (1, 2) for a in ATTRS]
WIDE_POS = {v: i for i, v in enumerate(WIDE)}

# name -> select list. The comment names what only this list reaches; "ms" is the set of
# match-stream columns (the e1-side attributes but sym, which the engine reads from e2)
CASES = {
    # width 1, no match-stream column
    "w1_e2_price": [(2, "price")],
    # one 8-byte column: the generic ms_put form (not stage1); an 8-byte value at word 2
    "w1_e1_volume": [(1, "volume")],
    # one 1-byte column written and read; a bool in its 4-byte packed slot
    "w1_e1_flag": [(1, "flag")],
    # stage1 with an int; int then long leaves a pad word; the widest 6-wave typed-columns form
    "w2_int_long": [(1, "x"), (2, "volume")],
    # odd raw store; bool, float, double alignment; ms = one float
    "w3_bool_float_double": [(2, "flag"), (1, "price"), (2, "d")],
    # width 4 with other types than C2's; ms = two 8-byte columns
    "w4_two_wide_ms": [(1, "d"), (2, "x"), (1, "volume"), (2, "flag")],
    # the folded partition attribute; the last 6-wave width of raw / packed rows; ms = {price, d}
    "w5_sym": [(1, "sym"), (1, "price"), (2, "volume"), (1, "d"), (2, "x")],
    # width 6 (the first 4-wave raw / packed width), a pad word after each 4-byte value
    "w6_alternating": [(1, "x"), (2, "d"), (2, "flag"), (1, "volume"), (2, "price"), (2, "volume")],
    # width 7, ms of 1, 4 and 4 bytes
    "w7_mixed_ms": [(1, "flag"), (2, "d"), (1, "x"), (2, "volume"), (1, "price"), (2, "flag"), (2, "x")],
    # width 8, all 8-byte: 80-byte packed rows, the largest unrolled bk_pack
    "w8_all_wide": [(1, "volume"), (2, "volume"), (1, "d"), (2, "d"), (2, "volume"), (1, "d"), (2, "d"),
                    (1, "volume")],
    # nine values, four match-stream columns (SHB_MAX_MS): the generic NO == 0 path
    "w9_four_ms": [(1, "price"), (1, "volume"), (1, "x"), (1, "d"), (1, "x"), (1, "volume"), (1, "d"),
                   (1, "price"), (1, "x")],
    # sixteen values (SHB_MAX_OUT), ms = {flag, volume, price, d}
    "w16": [(1, "flag"), (2, "volume"), (1, "sym"), (2, "x"), (1, "volume"), (2, "flag"), (1, "price"), (2, "d"),
            (2, "sym"), (1, "d"), (2, "price"), (1, "flag"), (2, "volume"), (1, "price"), (2, "x"), (1, "volume")],
}
BUCKETED = list(CASES)
# five distinct e1-side attributes: more match-stream columns than the bucketed engine has
FIVE_MS = [(1, "price"), (1, "volume"), (1, "x"), (1, "d"), (1, "flag"), (2, "price")]

LAYOUTS = ["raw", "packed", "columns"]


def ms_attrs(values):
    """the e1-side attributes that ride the match stream, in first-use order"""
    out = []
    for s, a in values:
        if s == 1 and a != "sym" and a not in out:
            out.append(a)
    return out


def six_waves(layout, width):
    """bk_emit_launch's choice of the occupancy form, restated: 6 waves per SIMD for raw /
    packed rows of at most 5 values, typed columns of at most 2 and every generic list
    (more than 8 values); 4 waves otherwise"""
    if width > 8:
        return True
    return width <= (2 if layout == "columns" else 5)


# ---------------------------------------------------------------------------------
# the burst stream
# ---------------------------------------------------------------------------------
_streams = {}


def burst_stream(nk, seed=7, cycles=3):
    """(ts, keys, [sym, price, volume, x, d, flag]) at 100 events per ms. Per cycle c:
    (A) for j in 0..19 one shuffled round of the keys with L_k > j, priced 30 + L_k - j
        (L_k uniform in 0..20 per key and cycle; a key's prices descend, so nothing is
        consumed and the key holds L_k partials);
    (B) one shuffled round of all keys at price 100: each consumes its L_k partials, so a
        half of 512 such events carries about 5,000 rows;
    (C) 3000 + 17c ordinary events (random keys, prices 15..40.5): sparse halves.
    The other columns are random over their whole ranges."""
    if (nk, seed, cycles) in _streams:
        return _streams[(nk, seed, cycles)]
    rng = np.random.default_rng(seed)
    keys, price = [], []
    for c in range(cycles):
        L = rng.integers(0, 21, nk)
        for j in range(20):
            ks = np.nonzero(L > j)[0]
            rng.shuffle(ks)
            keys.append(ks)
            price.append(30.0 + L[ks] - j)
        ks = rng.permutation(nk)
        keys.append(ks)
        price.append(np.full(nk, 100.0))
        m = 3000 + 17 * c
        keys.append(rng.integers(0, nk, m))
        price.append(rng.integers(15, 40, m) + rng.choice([0.0, 0.5, 0.25], m))
    keys = np.concatenate(keys).astype(np.int32)
    price = np.concatenate(price).astype(np.float32)
    n = len(keys)
    ts = (1000 + np.arange(n) // 100).astype(np.int64)
    volume = rng.integers(-2 ** 40, 2 ** 40, n).astype(np.int64)
    x = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    d = rng.standard_normal(n).astype(np.float64)
    flag = rng.integers(0, 2, n).astype(np.uint8)
    for a in (ts, keys, price, volume, x, d, flag):
        a.setflags(write=False)
    _streams[(nk, seed, cycles)] = (ts, keys, [keys, price, volume, x, d, flag])
    return _streams[(nk, seed, cycles)]


def strings(nk):
    s = compiler.StringDict()
    for i in range(nk):
        s.id(f"K{i}")
    return s


_wide = {}


def wide_rows(nk):
    """the oracle's rows of the burst stream at `nk` keys with all twelve attributes
    selected: (seq int64 [m], values int64 [m, 12]); computed once and read-only"""
    if nk not in _wide:
        ts, keys, cols = burst_stream(nk)
        eng = OracleEngine(compiler.compile_app(app(WIDE), strings(nk)))
        eng.start()
        for b0 in range(0, len(ts), BATCH):
            b1 = min(len(ts), b0 + BATCH)
            eng.send(0, np.ascontiguousarray(ts[b0:b1]), [np.ascontiguousarray(c[b0:b1]) for c in cols],
                     [None] * len(cols), np.ascontiguousarray(keys[b0:b1]), b0)
        out = eng.drain()
        eng.close()
        assert not out["nulls"].any()
        seq = out["seq"].astype(np.int64)
        vals = np.ascontiguousarray(out["values"][:, :len(WIDE)])
        seq.setflags(write=False)
        vals.setflags(write=False)
        _wide[nk] = (seq, vals)
    return _wide[nk]


def expected_raw(nk, values):
    """(seq, raw 8-byte values [m, len(values)]) of one select list"""
    seq, vals = wide_rows(nk)
    return seq, np.ascontiguousarray(vals[:, [WIDE_POS[v] for v in values]])


def event_counts(nk):
    """rows per consuming event (arrival index), from the oracle's trigger sequence numbers"""
    seq, _ = wide_rows(nk)
    return np.bincount(seq, minlength=len(burst_stream(nk)[0]))


def walk_steps(nk):
    """per row, how many events of its key lie between the opening and the consuming event
    (the matcher's walk step at which the partial is met: 0 is the key's previous event).
    The opening event is found by its volume, which the generator draws from 2^41 values
    (asserted unique)"""
    _, keys, cols = burst_stream(nk)
    seq, vals = wide_rows(nk)
    vol = cols[2]
    order = np.argsort(vol)
    assert (np.diff(vol[order]) > 0).all()
    e1 = order[np.searchsorted(vol[order], vals[:, WIDE_POS[(1, "volume")]])]
    assert (vol[e1] == vals[:, WIDE_POS[(1, "volume")]]).all() and (keys[e1] == keys[seq]).all() and (e1 < seq).all()
    by_key = np.argsort(keys, kind="stable")
    ks = keys[by_key]
    first = np.concatenate([[0], np.nonzero(np.diff(ks))[0] + 1])
    rank = np.empty(len(keys), np.int64)
    rank[by_key] = np.arange(len(ks)) - np.repeat(first, np.diff(np.concatenate([first, [len(ks)]])))
    return rank[seq] - rank[e1] - 1


def half_rows(nk):
    """rows of every arrival-aligned half of 512 events"""
    c = event_counts(nk)
    pad = (-len(c)) % HALF
    return np.concatenate([c, np.zeros(pad, c.dtype)]).reshape(-1, HALF).sum(axis=1)


# ---------------------------------------------------------------------------------
# the layouts, restated from include/siddhi_hip.h
# ---------------------------------------------------------------------------------
# natural width of a select value: long / double 8 B, int / float / string id 4 B, bool 1 B
NATURAL = {LONG: 8, DOUBLE: 8, INT: 4, FLOAT: 4, STRING: 4, BOOL: 1}
COLUMN_DTYPE = {LONG: np.int64, DOUBLE: np.float64, INT: np.int32, FLOAT: np.float32, STRING: np.int32,
                BOOL: np.uint8}


def packed_layout(types):
    """(byte offset of each value, row bytes): the trigger_seq in 8 bytes, then each value at
    its natural width aligned to that width, a bool in a 4-byte slot, the row padded to a
    multiple of 16 bytes"""
    pos, offs = 8, []
    for t in types:
        w = 4 if t == BOOL else NATURAL[t]
        pos = (pos + w - 1) // w * w
        offs.append(pos)
        pos += w
    return offs, (pos + 15) // 16 * 16


def column_bytes(raw, t):
    """one raw 8-byte column (int64 [m]) as the little-endian bytes [m, width] of the typed
    column element: the low `width` bytes (a float's bits are zero-extended in the raw form,
    an int or a string id sign-extended, a bool is 0 / 1)"""
    b = np.ascontiguousarray(raw.astype("<i8")).view(np.uint8).reshape(-1, 8)
    return np.ascontiguousarray(b[:, :NATURAL[t]])


def expected_columns(raw, types):
    """typed columns as byte arrays [m, width], one per select value"""
    return [column_bytes(raw[:, o], t) for o, t in enumerate(types)]


def expected_packed_fields(seq, raw, types):
    """[(byte offset, bytes [m, width])] of the contracted fields of the packed rows: the
    sequence number and every value. A bool's field is its whole 4-byte slot holding 0 / 1;
    the padding between fields and after the last one is left out"""
    offs, _ = packed_layout(types)
    fields = [(0, np.ascontiguousarray(seq.astype("<i8")).view(np.uint8).reshape(-1, 8))]
    for o, t in enumerate(types):
        b = column_bytes(raw[:, o], t)
        if t == BOOL:
            b = np.concatenate([b, np.zeros((len(b), 3), np.uint8)], axis=1)
        fields.append((offs[o], b))
    return fields
