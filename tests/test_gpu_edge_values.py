"""IEEE / Java edge values (tests/edge_values.py: NaN, +-inf, +-0.0, subnormals,
FLT_MAX, 2^24 + 1, INT_MIN, LONG_MAX, ...) through every device form of "compare two
attribute values the way Java does" and every sum path, against the CPU oracle (pinned
to Java and to the NumPy restatements in tests/test_edge_values_cpu.py).

Each case runs the device once and compares it with the oracle's rows of the same stream
(computed once per stream and shared): equal trigger sequence numbers, equal query ids
where the run carries them, and equal values under edge_values.canon (exact bits, all
NaNs as one) wherever the reference is not null.

No engine documents a premise about attribute values (the aggregate carries do, and
fall back inside the handle), so each case also expects the engine status the same shape
reports on ordinary values: STATUS below, measured on an MI355X. A case that left its
fast path because of a value class would fail here rather than test only the fallback."""
import os

import numpy as np
import pytest

import edge_values as ev
from oracle_engine import OracleEngine
from rules_cases import card_strings
from siddhi_amd import compiler, synth

pytestmark = pytest.mark.gpu

TILE = 8192
KB2 = (200_000 + 77, 1024)      # ~100 same-key events per 1 s window: walks pass SHB_MSTEPS (SHB_MOVF)
SHORT = (3 * TILE + 17, 2000)   # four tiles, the last one partial
BUCKET_SHAPES = {"kb2": KB2, "short": SHORT}

# engine status of each shape, as the same shape reports it on ordinary values
STATUS = {
    "bucket": {"kb2": 1, "short": 1},                       # bucket_status()
    # seq3_status(): 2 k_s3b (needs 1,024 keys and one 4-byte attribute throughout), 1 k_seq3s, 0 general
    "seq3": {("c3", "s3b", 600): 1, ("c3", "seq3", 600): 1, ("c3", "general", 600): 0,
             ("c3_mirror", "s3b", 600): 1, ("c3_mirror", "seq3", 600): 1, ("c3_mirror", "general", 600): 0,
             ("c3_mixed", "s3b", 600): 1, ("c3_mixed", "seq3", 600): 1, ("c3_mixed", "general", 600): 0,
             ("c3_int", "s3b", 600): 1, ("c3_int", "seq3", 600): 1, ("c3_int", "general", 600): 0,
             ("c3", "s3b", 1200): 2, ("c3_mirror", "s3b", 1200): 2, ("c3_mixed", "s3b", 1200): 1,
             ("c3_int", "s3b", 1200): 2},
    "rules": {"sparse": 1, "segment": 0, "img0": 1, "general": 0},   # rules_status()
    "agg_bucket": 1,                                        # bucket_status() of the C2 aggregate runs
    "agg_seq3": 1,                                          # seq3_status() of the C3 aggregate run (3 as agg_status)
    # agg_status() on the streams whose prices k_bk_aggp and the post-pass accept: 5 the
    # fixed-point carry, 1 the post-pass, 4 the sequential carry
    "agg_exact": {("float", "default"): 5, ("float", "aggp0"): 1, ("float", "aggc"): 4, ("float", "post"): 1,
                  ("double", "default"): 1, ("double", "aggp0"): 1, ("double", "aggc"): 1, ("double", "post"): 1,
                  "c1": 1, "c3": 3, "c5": 1},
}


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _strings(nk):
    s = compiler.StringDict()
    for i in range(nk):
        s.id(f"K{i}")
    return s


def device_rows(app, strings, ts, keys, cols, nk, with_query=False, packed=False, batch=4096):
    """one DeviceRunner run: (rows as the oracle's drain() gives them, statuses, out types)"""
    import torch
    from siddhi_amd.device_run import DeviceRunner, packed_to_raw
    r = DeviceRunner(compiler.compile_app(app, strings))
    dev = torch.device("cuda:0")
    dcols = [torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in cols]
    dkeys = torch.from_numpy(np.ascontiguousarray(keys)).to(dev)
    res = r.run(torch.from_numpy(ts).to(dev), dkeys, dcols, nk, with_query=with_query, packed=packed,
                batch_events=batch)
    torch.cuda.synchronize()
    st = dict(jit=r.jit_status(), bucket=r.bucket_status(), seq3=r.seq3_status(), rules=r.rules_status(),
              agg=r.agg_status(), err=r.last_error())
    if packed:
        offs, rb = r.packed_layout()
        seq, vals = packed_to_raw(res[1].cpu().numpy(), r.out_types, offs, rb)
        got = dict(seq=seq.view(np.int64), values=vals)
    else:
        got = dict(seq=res[1].cpu().numpy(), values=res[2].cpu().numpy())
    if with_query:
        got["query"] = res[-1].cpu().numpy()
    assert res[0] == len(got["seq"])
    types = list(r.out_types)
    r.close()
    return got, st, types


_refs = {}


def _ref(key, make):
    """the oracle's rows of one (query, stream), computed once and left unchanged"""
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def _oracle(app, strings, ts, keys, cols, batch=4096, partitioned=True):
    eng = OracleEngine(compiler.compile_app(app, strings))
    eng.start()
    for b0 in range(0, len(ts), batch):
        b1 = min(len(ts), b0 + batch)
        eng.send(0, np.ascontiguousarray(ts[b0:b1]), [np.ascontiguousarray(c[b0:b1]) for c in cols],
                 [None] * len(cols), np.ascontiguousarray(keys[b0:b1]) if partitioned else None, b0)
    out = eng.drain()
    eng.close()
    return out


# ------------------------------------------------------------------ window engine
def window_case(name, nk, edge=True):
    """(app, strings, ts, keys, cols) of one (a) query on the 20,000-event stream"""
    ts, keys, cols = ev.window_stream(20_000, nk, edge=edge)
    return ev.window_query(name), _strings(nk), ts, keys, [keys] + list(cols)


@pytest.mark.parametrize("tiles", [0, 12], ids=["untiled", "tiles4096"])
@pytest.mark.parametrize("jit", [True, False], ids=["jit", "aot"])
@pytest.mark.parametrize("nk", [1, 50])
@pytest.mark.parametrize("name", [q[0] for q in ev.WINDOW_QUERIES])
def test_window_engine(name, nk, jit, tiles, monkeypatch):
    """the hipRTC-specialised window kernels (their own flag list: denormals kept, no
    contraction) and the ahead-of-time ones, on one key segment and on arrival tiles"""
    if not jit:
        monkeypatch.setenv("SH_DISABLE_JIT", "1")
    monkeypatch.setenv("SH_TILE_SHIFT", str(tiles))
    app, strings, ts, keys, cols = window_case(name, nk)
    ref = _ref(("win", name, nk), lambda: _oracle(app, strings, ts, keys, cols))
    got, st, types = device_rows(app, strings, ts, keys, cols, nk)
    print(f"window {name} nk={nk} jit={jit} tiles={tiles}: rows={len(got['seq'])} status={st}")
    assert st["jit"] == (1 if jit else -1), st
    assert len(ref["seq"]) > 0
    ev.assert_rows_equal(got, ref, types, app)


# ------------------------------------------------------------------ bucketed engine
def bucket_case(name, shape, edge=True):
    n, nk = BUCKET_SHAPES[shape]
    if name in ("c2", "c2_free"):       # the StockStream form, which c2_check restates
        ts, keys, p, v = ev.agg_stream(n, nk, edge=edge)
        app = synth.C2_QUERY if name == "c2" else synth.C2_QUERY.replace("price>20", "price>-1")
        return app, None, ts, keys, [keys, p, v], nk
    ts, keys, cols = ev.bucket_stream(n, nk, edge=edge)
    return ev.window_query(name, within_ms=1000), _strings(nk), ts, keys, [keys] + list(cols), nk


def _bucket_check(name, shape, packed):
    app, strings, ts, keys, cols, nk = bucket_case(name, shape)
    ref = _ref(("bucket", name, shape), lambda: _oracle(app, strings, ts, keys, cols))
    got, st, types = device_rows(app, strings, ts, keys, cols, nk, packed=packed)
    print(f"bucket {name} {shape} packed={packed} dyn={os.environ.get('SH_BK_DYN', '1')}: "
          f"rows={len(got['seq'])} status={st}")
    assert st["bucket"] == STATUS["bucket"][shape], st
    assert len(ref["seq"]) > 0
    ev.assert_rows_equal(got, ref, types, app)


BUCKET_ALL = ev.BUCKET_QUERIES + ["c2", "c2_free"]
# every query the engine accepts, raw on both shapes and packed on the short one; a few
# packed on kb2 as well (the packed writer is the same code for every query: it differs by
# the select's types, which all share, so one shape per query covers it)
BUCKET_CASES = ([(q, "kb2", False) for q in BUCKET_ALL] + [(q, "short", False) for q in BUCKET_ALL] +
                [(q, "short", True) for q in BUCKET_ALL] +
                [(q, "kb2", True) for q in ("f32_gt", "f32_le", "f32_x_f64lit", "i64_gt_f32", "i64_ge")])


@pytest.mark.parametrize("name,shape,packed", BUCKET_CASES,
                         ids=[f"{q}-{s}-{'packed' if p else 'raw'}" for q, s, p in BUCKET_CASES])
def test_bucketed_engine(name, shape, packed):
    """shb_match: the float cross terms take walk_count_f_dyn (the running extremum starts
    as NaN, fmax / fmin skip a NaN operand, liveness is x == x), the integer ones the
    generic walk_count (a hasM flag)"""
    _bucket_check(name, shape, packed)


@pytest.mark.parametrize("shape,packed", [("kb2", False), ("short", True)], ids=["kb2-raw", "short-packed"])
@pytest.mark.parametrize("name", ev.BUCKET_FLOAT + ["c2", "c2_free"])
def test_bucketed_engine_wave_uniform_float_walk(name, shape, packed, monkeypatch):
    """SH_BK_DYN=0: walk_count_f (every lane of a wave walks to the wave's longest walk),
    for every float-domain query"""
    monkeypatch.setenv("SH_BK_DYN", "0")
    _bucket_check(name, shape, packed)


# ------------------------------------------------------------------ seq3
S3_ENV = {"s3b": None, "seq3": "SH_DISABLE_S3B", "general": "SH_NO_SEQ3"}


def seq3_case(name, nk=600, edge=True):
    ts, k, p, v = ev.c3_stream(60_000, nk, name, edge=edge)
    return ev.C3_QUERIES[name], None, ts, k, [k, p, v], nk


@pytest.mark.parametrize("engine,nk", [("s3b", 600), ("seq3", 600), ("general", 600), ("s3b", 1200)])
@pytest.mark.parametrize("name", list(ev.C3_QUERIES))
def test_seq3_engines(name, engine, nk, monkeypatch):
    """k_s3b (its float-as-float fast path beside the generic nf_cmp), k_seq3s and the
    general engine on the rise-and-fall shape, its mirror, the mixed long form and the int
    form (k_s3b's generic nf_cmp branch). The
    bucket-carry engine takes 1,024 keys or more, so at 600 keys the default run is
    k_seq3s on any values; the 1,200-key leg is the one that reaches k_s3b"""
    if S3_ENV[engine]:
        monkeypatch.setenv(S3_ENV[engine], "1")
    app, strings, ts, keys, cols, nk = seq3_case(name, nk)
    ref = _ref(("seq3", name, nk), lambda: _oracle(app, strings, ts, keys, cols))
    got, st, types = device_rows(app, strings, ts, keys, cols, nk)
    print(f"seq3 {name} {engine} nk={nk}: rows={len(got['seq'])} status={st}")
    assert st["seq3"] == STATUS["seq3"][(name, engine, nk)], st
    assert len(ref["seq"]) > 0
    ev.assert_rows_equal(got, ref, types, app)


# ------------------------------------------------------------------ rules
RULES_ENV = {"sparse": None, "segment": ("SH_RULES_SPARSE", "0"), "img0": ("SH_SPARSE_IMG", "0"),
             "general": ("SH_DISABLE_RULES", "1")}


def rules_case(variant, edge=True):
    text, rules, (ts, card, amount, merchant) = ev.rule_set(variant, edge=edge)
    return text, card_strings(400), ts, card, [card, amount, merchant], 400


@pytest.mark.parametrize("engine", list(RULES_ENV))
@pytest.mark.parametrize("variant", ev.RULE_VARIANTS)
def test_rule_engines(variant, engine, monkeypatch):
    """rule_terms_pre (its float-attribute-against-double-constant shortcut), rule_terms,
    rule_terms_img and the indexed equality conjunct (rule_ix_key / ix_const_key) on int,
    long and float attributes; the general engine's VM on the same sets"""
    if RULES_ENV[engine]:
        monkeypatch.setenv(*RULES_ENV[engine])
    app, strings, ts, keys, cols, nk = rules_case(variant)
    ref = _ref(("rules", variant), lambda: _oracle(app, strings, ts, keys, cols))
    got, st, types = device_rows(app, strings, ts, keys, cols, nk, with_query=True)
    print(f"rules {variant} {engine}: rows={len(got['seq'])} status={st}")
    assert st["rules"] == STATUS["rules"][engine], st
    assert len(ref["seq"]) > 0
    ev.assert_rows_equal(got, ref, types[:2], app)


# ------------------------------------------------------------------ general engine
@pytest.mark.parametrize("name", list(ev.GENERAL_APPS))
def test_general_engine(name):
    """vm_eval / vm_cmp / vm_arith and null select values through the event API"""
    from test_gpu_parity import _run_engine, hip_factory
    sends = ev.general_sends()
    ref = _run_engine(OracleEngine, ev.GENERAL_APPS[name], sends)
    got = _run_engine(hip_factory, ev.GENERAL_APPS[name], sends)
    print(f"general {name}: rows={len(got)}")
    assert len(got) == len(ref) > 0
    for g, r in zip(got, ref):
        assert g[0] == r[0]
        assert [ev.canon_obj(x) for x in g[1]] == [ev.canon_obj(x) for x in r[1]], (name, g, r)


# ------------------------------------------------------------------ aggregates
AGG_ENV = {"default": None, "aggp0": ("SH_BK_AGGP", "0"), "aggc": ("SH_BK_AGGC", "1"), "post": ("SH_BK_AGG_POST", "1")}
AGG_APPS = ["c2agg-float", "c2agg-double", "free-float", "open-float", "open-double"]
AGG_EXACT_APPS = ["c2agg-float", "open-float", "c2agg-double"]


def agg_case(which, edge=True, exact=False):
    from test_gpu_agg import C2_AGG
    text, kind = which.split("-")
    app = {"c2agg": C2_AGG, "free": ev.C2_AGG_FREE, "open": ev.C2_AGG_OPEN}[text]
    if kind == "double":
        app = app.replace("price float", "price double")
    ts, k, p, v = ev.agg_stream(*ev.AGG_SHAPE, double=kind == "double", edge=edge, share=ev.AGG_SHARE, exact=exact)
    return app, None, ts, k, [k, p, v], ev.AGG_SHAPE[1]


@pytest.mark.parametrize("carry", list(AGG_ENV))
@pytest.mark.parametrize("which", AGG_APPS)
def test_c2_aggregates(which, carry, monkeypatch):
    """k_bk_aggp / agp_units (values exact in 2^-24 fixed point or refused), the post-pass
    and its isfinite test, k_bk_aggc: whichever carry ends up producing them (any
    agg_status), sum and avg are the oracle's left-to-right double additions, sums that
    became inf or NaN included, and sum(long) wraps past LONG_MAX"""
    if AGG_ENV[carry]:
        monkeypatch.setenv(*AGG_ENV[carry])
    app, strings, ts, keys, cols, nk = agg_case(which)
    ref = _ref(("agg", which), lambda: _oracle(app, strings, ts, keys, cols))
    got, st, types = device_rows(app, strings, ts, keys, cols, nk)
    print(f"agg {which} {carry}: rows={len(got['seq'])} status={st}")
    assert st["bucket"] == STATUS["agg_bucket"], st
    assert len(ref["seq"]) > 0
    ev.assert_rows_equal(got, ref, types, app)


@pytest.mark.parametrize("carry", list(AGG_ENV))
@pytest.mark.parametrize("which", AGG_EXACT_APPS)
def test_c2_aggregates_exact_classes(which, carry, monkeypatch):
    """NaN, +-inf, subnormals, FLT_MAX and 2^-25 are not whole units of 2^-24 below 2^53, the
    documented premise of the parallel carries (DESIGN.md "Values"): the streams above leave
    k_bk_aggp and the post-pass for the sequential carry. So that the fast carries still
    meet the classes they accept (+-0.0, the threshold's neighbours, 2^24 and 2^24 + 2, and
    the wrapping long sum), this stream is salted from those alone and must keep the
    agg_status of ordinary values"""
    if AGG_ENV[carry]:
        monkeypatch.setenv(*AGG_ENV[carry])
    app, strings, ts, keys, cols, nk = agg_case(which, exact=True)
    ref = _ref(("agg-exact", which), lambda: _oracle(app, strings, ts, keys, cols))
    got, st, types = device_rows(app, strings, ts, keys, cols, nk)
    print(f"agg-exact {which} {carry}: rows={len(got['seq'])} status={st}")
    assert st["bucket"] == STATUS["agg_bucket"], st
    assert st["agg"] == STATUS["agg_exact"][(which.split("-")[1], carry)], st
    assert len(ref["seq"]) > 0
    ev.assert_rows_equal(got, ref, types, app)


def _salt_pv(p, v, exact, seed):
    rng = np.random.default_rng(seed)
    return (ev.salt(p, ev.AGG_EXACT_F32 if exact else None, share=ev.AGG_SHARE, rng=rng),
            ev.salt(v, share=ev.AGG_SHARE, rng=rng))


def c1_agg_case(edge=True, exact=False):
    """(one unpartitioned group of ~20,000 rows: with 2^24-sized addends beside 2^-19-unit
    ones its running sum needs more than 53 bits, the additions round and the post-pass
    rightly hands over; the exact stream of this shape leaves 2^24 and 2^24 + 2 out)"""
    from test_gpu_agg import C1_AGG
    ts, k, p, v = synth.stock_stream(30_000, 100, 1, config_index=1)
    if edge:
        rng = np.random.default_rng(810)
        p = ev.salt(p, ev.AGG_EXACT_SMALL if exact else None, share=ev.AGG_SHARE, rng=rng)
        v = ev.salt(v, share=ev.AGG_SHARE, rng=rng)
    return C1_AGG, None, ts, np.zeros(len(ts), np.int32), [k, p, v], 1


def c3_agg_case(edge=True, exact=False):
    from test_gpu_agg import C3_AGG
    ts, k, p, v = synth.stock_stream(60_000, 600, 1000, config_index=3)
    if edge:
        p, v = _salt_pv(p, v, exact, 820)
    return C3_AGG, None, ts, k, [k, p, v], 600


def c5_agg_case(edge=True, exact=False):
    text, strings, ts, card, (_, amount, merchant), nk = rules_case("base", edge=False)
    if edge:
        amount = ev.salt(amount, ev.AGG_EXACT_F32 if exact else None, rng=np.random.default_rng(700))
    assert "e2.amount as amount" in text
    return (text.replace("e2.amount as amount", "sum(e2.amount) as total, avg(e1.amount) as a1"), strings, ts, card,
            [card, amount, merchant], nk)


AGG_OTHER = {"c1": (c1_agg_case, False, False), "c3": (c3_agg_case, True, False), "c5": (c5_agg_case, True, True)}


@pytest.mark.parametrize("exact", [False, True], ids=["all", "exact"])
@pytest.mark.parametrize("shape", list(AGG_OTHER))
def test_other_aggregates(shape, exact):
    """the window engine's (C1), k_seq3s's (C3) and the rule set's (C5) aggregates, one case
    each on the whole pools (any agg_status) and one on the classes the post-pass accepts
    (the agg_status of ordinary values)"""
    case, partitioned, with_query = AGG_OTHER[shape]
    app, strings, ts, keys, cols, nk = case(exact=exact)
    ref = _oracle(app, strings, ts, keys, cols, partitioned=partitioned)
    got, st, types = device_rows(app, strings, ts, keys, cols, nk, with_query=with_query)
    print(f"agg {shape} exact={exact}: rows={len(got['seq'])} status={st}")
    if shape == "c3":
        assert st["seq3"] == STATUS["agg_seq3"], st
    if exact:
        assert st["agg"] == STATUS["agg_exact"][shape], st
    elif shape == "c5":
        # inf and NaN sums: the post-pass hands the set to the general engine, and says so
        assert (st["agg"], st["rules"]) == (2, 0), st
    assert len(ref["seq"]) > 0
    ev.assert_rows_equal(got, ref, types, app)
