"""Shared pieces of the device-primitive tests (tests/test_device_prims_cpu.py,
tests/test_gpu_device_prims.py, tests/device_prims_child.py): the scan, the radix
segment, the pair sort and the tile directory of siddhi_amd/csrc/sh_kernels.hip and
sh_window.hip, called through ctypes with torch device pointers and compared with
numpy restatements of what siddhi_amd/csrc/sh_device.h promises.

Held fixed here:
  * the ctypes mirrors of shd_batch / shd_segment_ws / shd_payload, of the row
    sets shw_rows / shw_rows_out of sh_having.h, and of sha_col / sha_desc /
    shq_table of the aggregate post-passes (tests/agg_post_cases.py), all checked
    against the headers by tests/prims_layout;
  * the numpy contracts (*_ref), written from the header comments, not the kernels;
  * the workspace sizes in 4-byte words as the header and the callers state them.
    Every device buffer has exactly that size plus a guard of GUARD words; outputs
    and guards are filled with 0xA5 bytes before every call and every check asserts
    the guards untouched;
  * the case lists, as data (test_device_prims_cpu.py asserts their premises).

Nothing here imports torch or touches the GPU at import time."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(HERE), "siddhi_amd", "libsiddhi_hip.so")

RADIX_TILE = 4096          # events per radix block
WAVES_PER_TILE = 4         # each wave of a block ranks a contiguous quarter
SCAN_TILE = 1024
SMALL_MAX = 4096           # the one-workgroup segment takes n <= 4,096
GUARD = 64                 # words
FILL = 0xA5
FILL32 = 0xA5A5A5A5


# ------------------------------------------------------------------ ctypes mirrors
class shd_batch(C.Structure):
    _fields_ = [("ts", C.c_void_p), ("stream", C.c_void_p), ("row", C.c_void_p), ("keys", C.c_void_p),
                ("row_base", C.c_uint32), ("pad", C.c_int32), ("seq_base", C.c_uint64), ("n", C.c_int64)]


class shd_segment_ws(C.Structure):
    _fields_ = [("keys_a", C.c_void_p), ("keys_b", C.c_void_p), ("idx_a", C.c_void_p), ("idx_b", C.c_void_p),
                ("hist", C.c_void_p), ("scan_tmp", C.c_void_p), ("seg_off", C.c_void_p), ("cap", C.c_int64)]


class shd_payload(C.Structure):
    _fields_ = [("n", C.c_int32), ("pad", C.c_int32), ("src", C.c_void_p * 8), ("dst", C.c_void_p * 8),
                ("width", C.c_uint8 * 8)]


class shw_rows(C.Structure):
    """a set of rows as parallel columns (sh_having.h); shw_rows_out is its writable twin"""
    _fields_ = [("seq", C.c_void_p), ("vals", C.c_void_p), ("query", C.c_void_p), ("ts", C.c_void_p),
                ("nulls", C.c_void_p), ("key", C.c_void_p)]


class shw_rows_out(C.Structure):
    _fields_ = list(shw_rows._fields_)


SHA_MAX_COLS = 16


class sha_col(C.Structure):
    """one aggregate output column of the raw rows (sh_agg.h)"""
    _fields_ = [("col", C.c_int32), ("kind", C.c_int32), ("arg_type", C.c_int32), ("pad", C.c_int32)]


class sha_desc(C.Structure):
    _fields_ = [("n_cols", C.c_int32), ("pad", C.c_int32), ("c", sha_col * SHA_MAX_COLS)]


class shq_table(C.Structure):
    """the carried aggregate states (sh_agg_seq.h): open addressing over the segment key"""
    _fields_ = [("keys", C.c_void_p), ("state", C.c_void_p), ("cap", C.c_int64), ("n_cols", C.c_int32),
                ("pad", C.c_int32)]


MIRRORS = {"shd_batch": shd_batch, "shd_segment_ws": shd_segment_ws, "shd_payload": shd_payload,
           "shw_rows": shw_rows, "shw_rows_out": shw_rows_out, "sha_col": sha_col, "sha_desc": sha_desc,
           "shq_table": shq_table}

_lib = None


def lib():
    """the product library with the shd_* prototypes bound (DEVICE_PRIMS_LIB names
    another build of it, e.g. a mutant of a mutation check)"""
    global _lib
    if _lib is None:
        import torch  # noqa: F401  (first: the library must share torch's HIP runtime, whose pointers it takes)
        L = C.CDLL(os.environ.get("DEVICE_PRIMS_LIB") or LIB_PATH)
        vp, pvp = C.c_void_p, C.POINTER(C.c_void_p)
        L.shd_scan_tmp_words.argtypes = [C.c_int64]
        L.shd_scan_tmp_words.restype = C.c_size_t
        L.shd_exclusive_scan.argtypes = [vp, vp, C.c_int64, vp, vp]
        L.shd_exclusive_scan.restype = C.c_int
        L.shd_segment.argtypes = [C.POINTER(shd_batch), C.c_int32, C.POINTER(shd_segment_ws), vp, pvp, pvp]
        L.shd_segment.restype = C.c_int
        L.shd_segment_payload.argtypes = [C.POINTER(shd_batch), C.c_int32, C.POINTER(shd_segment_ws), vp, pvp, pvp,
                                          C.POINTER(shd_payload), pvp, C.c_int, C.c_int]
        L.shd_segment_payload.restype = C.c_int
        L.shd_sort_pairs.argtypes = [vp, vp, C.c_int64, C.c_int, pvp, pvp, vp, vp, vp, pvp, pvp]
        L.shd_sort_pairs.restype = C.c_int
        L.shd_tile_dir.argtypes = [vp, C.c_int64, C.c_int, C.c_uint32, C.c_uint32, vp, vp, vp]
        L.shd_tile_dir.restype = C.c_int
        # the aggregate post-passes (sh_agg.h, sh_agg_seq.h)
        for f in (L.sha_scratch_bytes, L.shc_scratch_bytes):
            f.argtypes = [C.c_int64, C.c_int]
            f.restype = C.c_int64
        L.sha_running.argtypes = [vp, vp, C.c_int32, C.c_int64, vp, C.c_int32, vp, C.c_int32, C.c_uint64,
                                  C.POINTER(sha_desc), vp, vp]
        L.sha_running.restype = C.c_int
        L.shc_running.argtypes = [vp, vp, C.c_int32, C.c_int64, vp, C.c_int32, vp, vp, C.c_int32, C.c_uint64,
                                  C.POINTER(sha_desc), C.POINTER(shq_table), vp, vp, pvp, pvp]
        L.shc_running.restype = C.c_int
        L.shc_put.argtypes = [C.POINTER(shq_table), vp, vp, C.c_int64, vp, vp, vp]
        L.shc_put.restype = C.c_int
        _lib = L
    return _lib


# ------------------------------------------------------------------ numpy contracts
def scan_ref(a):
    """exclusive prefix sum in uint64, reduced mod 2^32"""
    a = np.asarray(a, dtype=np.uint64)
    out = np.zeros(len(a), dtype=np.uint64)
    if len(a) > 1:
        out[1:] = np.cumsum(a[:-1], dtype=np.uint64)
    return (out & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def segment_ref(keys, nkeys, tile_shift=0):
    """(perm, skeys, seg_list, nseg): null keys (< 0) become the sentinel nkeys;
    perm is the stable order by (key, arrival), inside each arrival tile of
    2^tile_shift events when tiled (global indices); the list holds the positions
    where the sorted key changes and is not the sentinel"""
    keys = np.asarray(keys, dtype=np.int64)
    n = len(keys)
    k = np.where(keys < 0, np.int64(nkeys), keys)
    if tile_shift:
        T = 1 << tile_shift
        perm = np.concatenate([b + np.argsort(k[b:b + T], kind="stable") for b in range(0, n, T)])
    else:
        perm = np.argsort(k, kind="stable")
    skeys = k[perm]
    start = np.ones(n, dtype=bool)
    start[1:] = skeys[1:] != skeys[:-1]
    seg = np.flatnonzero(start & (skeys != nkeys))
    return perm.astype(np.uint32), skeys.astype(np.uint32), seg.astype(np.uint32), len(seg)


def payload_ref(col, perm):
    return col[perm.astype(np.int64)]


def sort_pairs_ref(keys, vals, bits):
    """stable order by key (keys < 2^bits); vals NULL: the arrival index"""
    keys = np.asarray(keys, dtype=np.uint32)
    assert bits >= 32 or not len(keys) or int(keys.max()) < (1 << bits)
    v = np.arange(len(keys), dtype=np.uint32) if vals is None else np.asarray(vals, dtype=np.uint32)
    o = np.argsort(keys, kind="stable")
    return keys[o], v[o]


def tile_dir_ref(skeys, n, shift, K1):
    """ds / de [ntile][K1]: the run of key k in arrival tile a of a tile-major
    segment is [ds[a][k], de[a][k]); an absent (tile, key) pair is 0 / 0"""
    ntile = (n + (1 << shift) - 1) >> shift
    ds = np.zeros((ntile, K1), dtype=np.uint32)
    de = np.zeros((ntile, K1), dtype=np.uint32)
    for a in range(ntile):
        lo, hi = a << shift, min(n, (a + 1) << shift)
        t = np.asarray(skeys[lo:hi], dtype=np.int64)
        first = np.ones(len(t), dtype=bool)
        first[1:] = t[1:] != t[:-1]
        last = np.ones(len(t), dtype=bool)
        last[:-1] = t[1:] != t[:-1]
        ds[a, t[first]] = lo + np.flatnonzero(first)
        de[a, t[last]] = lo + np.flatnonzero(last) + 1
    return ds, de


# ------------------------------------------------------------------ sizes (4-byte words)
def bits_for(v):
    return int(v).bit_length()


def seg_passes(nkeys):
    """8-bit passes of a segment over nkeys keys: the null-key sentinel nkeys
    itself has to sort, so its bits count"""
    return (bits_for(nkeys) + 7) // 8


def radix10_env():
    return os.environ.get("SH_RADIX10", "")[:1] == "1"


def digit_bits(nkeys, tile_shift=0, radix10=None):
    """10-bit digits: opt-in, for 17..20 key bits, and only where the padded tile
    count of the tile-major form stays inside the callers' histogram (tiles of at
    most 2^20 events)"""
    r10 = radix10_env() if radix10 is None else radix10
    return 10 if (r10 and 16 < bits_for(nkeys) <= 20 and tile_shift <= 20) else 8


def padded_tiles(n, tile_shift=0):
    t = (n + RADIX_TILE - 1) // RADIX_TILE
    if tile_shift >= 12:
        per = 1 << (tile_shift - 12)
        t = (t + per - 1) // per * per
    return t


def scan_tmp_words_ref(n):
    """restated from the scan's recursion: 2 * tiles + 2 words per level + 4"""
    words, m = 0, (n + SCAN_TILE - 1) // SCAN_TILE
    while m > 1:
        words += 2 * m + 2
        m = (m + SCAN_TILE - 1) // SCAN_TILE
    return words + 4


def hist_words(n, nkeys, tile_shift=0, radix10=None):
    return (1 << digit_bits(nkeys, tile_shift, radix10)) * padded_tiles(n, tile_shift)


def host_hist_alloc_words(n):
    """what sh_host.cpp ensure_ws allocates for the histogram"""
    return 1024 * ((n + RADIX_TILE - 1) // RADIX_TILE + 256)


# ------------------------------------------------------------------ key patterns
PATTERNS = ("uniform", "one_key", "ascending", "descending", "top_digit", "low_digit", "nulls10", "all_null",
            "null_alt")
NULL_PATTERNS = ("nulls10", "all_null", "null_alt")
STABILITY_PATTERNS = ("one_key", "top_digit", "null_alt")


def patterns_for(n):
    """a one-event batch cannot hold a null and a non-null event"""
    return tuple(p for p in PATTERNS if n >= 2 or p not in ("nulls10", "null_alt"))


def make_keys(pattern, n, nkeys, seed=0):
    """int32 partition keys in [0, nkeys), -1 = null key"""
    rng = np.random.default_rng((n * 1000003 + nkeys * 7 + PATTERNS.index(pattern) * 131 + seed) & 0xFFFFFFFF)
    i = np.arange(n, dtype=np.int64)
    if pattern == "uniform":
        k = rng.integers(0, nkeys, n)
    elif pattern == "one_key":
        k = np.full(n, nkeys - 1)
    elif pattern in ("ascending", "descending"):
        k = i * (nkeys // n) if nkeys >= n else i * nkeys // n     # distinct where the range allows
        if pattern == "descending":
            k = k[::-1]
    elif pattern == "top_digit":
        # only the top 8-bit digit differs: every lower pass is pure stability
        shift = 8 * (max(bits_for(nkeys - 1), 1) - 1 >> 3)
        k = rng.integers(0, ((nkeys - 1) >> shift) + 1, n) << shift
    elif pattern == "low_digit":
        # only the low digit differs: every higher pass is pure stability
        k = (((nkeys >> 8) - 1) << 8) + rng.integers(0, 256, n) if nkeys > 512 else rng.integers(0, min(nkeys, 256), n)
    elif pattern == "nulls10":
        k = rng.integers(0, nkeys, n)
        k[rng.random(n) < 0.1] = -1
        k[0], k[-1] = -1, nkeys - 1
    elif pattern == "all_null":
        k = np.full(n, -1)
    elif pattern == "null_alt":
        k = np.where(i % 2 == 0, -1, 0)
    else:
        raise ValueError(pattern)
    k = np.ascontiguousarray(k, dtype=np.int64)
    assert k.min(initial=0) >= -1 and k.max(initial=0) < nkeys
    return k.astype(np.int32)


def payload_column(width, n, c):
    """column c of a carried payload: a function of the arrival index alone; the 8-
    and 4-byte columns are bijections of it (odd multipliers), so a misplaced or a
    duplicated row shows; one byte cannot be, it takes mixed bits of the index"""
    i = np.arange(n, dtype=np.uint64)
    if width == 8:
        return i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(c)
    if width == 4:
        return ((i * np.uint64(2654435761) + np.uint64(c)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return (((i * np.uint64(2654435761)) >> np.uint64(13)) + np.uint64(c)).astype(np.uint8)


# ------------------------------------------------------------------ case lists
SCAN_NS = (0, 1, 1023, 1024, 1025, 1024 ** 2 - 1, 1024 ** 2, 1024 ** 2 + 1, 1024 ** 2 + 1025)
SCAN_INPUTS = ("ones", "small", "last_one", "wrap")

SEG_NKEYS = (1, 2, 255, 256, 257, 65535, 65536, 65537, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 1)
SEG_NS = (1, 63, 64, 65, 4095, 4096, 4097, 8191, 16 * 4096, 34 * 4096 + 5)
SEG_CASES = tuple(sorted({(nk, n) for nk in SEG_NKEYS for n in (4096, 4097, 34 * 4096 + 5)} |
                         {(nk, n) for n in SEG_NS for nk in (256, 65536)}))
SEAM_NKEYS = SEG_NKEYS     # n = 4096 (one workgroup) against n = 4097 (radix path)

PAYLOAD_WIDTHS = ((8,), (1, 4, 8), (8, 4, 1, 8, 4, 1, 8, 4))
PAYLOAD_NKEYS = (200, 60_000, 1_000_000, 2 ** 24 + 1)       # 1, 2, 3 and 4 passes
PAYLOAD_NS = (4097, 34 * 4096 + 5)
PAYLOAD_PATTERNS = ("uniform", "top_digit", "nulls10")
PAYLOAD_CASES = tuple((nk, n, w) for nk in PAYLOAD_NKEYS for n in PAYLOAD_NS for w in PAYLOAD_WIDTHS)

TILED_SHIFTS = (12, 13, 14)
TILED_NKEYS = (1, 5, 300, 65536)
TILED_PATTERNS = ("uniform", "nulls10", "one_key", "null_alt")
TILED_WIDTHS = (8, 4, 1)


def tiled_ns(s):
    return ((1 << s) + 1, 3 * (1 << s) - 1, 3 * (1 << s), 3 * (1 << s) + 7)


TILED_CASES = tuple((s, nk, n) for s in TILED_SHIFTS for nk in TILED_NKEYS for n in tiled_ns(s))

SORT_BITS = (0, 1, 8, 9, 16, 17, 24, 25, 32)
SORT_NS = (0, 1, 4095, 4096, 4097, 16 * 4096, 16 * 4096 + 1, 33 * 4096 + 5)
SORT_CASES = tuple((b, n) for b in SORT_BITS for n in SORT_NS)

RADIX10_NKEYS = (65536, 200_000, 2 ** 20 - 1)
RADIX10_NS = (4097, 34 * 4096 + 5)

# what the children of the environment forms run (device_prims_child.py)
SUBSETS = ("scan", "segment", "seam", "payload", "tiled", "sort", "radix10", "small", "large")
ENV_FORMS = {
    "SH_RADIX_XCD": ("0", ("large", "payload", "tiled", "sort")),
    "SH_RADIX10": ("1", ("radix10",)),
    "SH_SEG_LASTCARRY": ("1", ("payload", "tiled")),
    "SH_SEG_SMALL": ("0", ("small", "seam")),
}


def stability_cases():
    """(pattern, nkeys, n) of the segment list that lean on stability alone"""
    return [(p, nk, n) for nk, n in SEG_CASES if n > RADIX_TILE for p in STABILITY_PATTERNS]


# ------------------------------------------------------------------ device side
class Dev:
    """one device buffer of exactly `words` 4-byte words plus the guard, all 0xA5"""

    def __init__(self, words, data=None):
        import torch
        self.words = int(words)
        self.t = torch.full((self.words + GUARD,), FILL32 - (1 << 32), dtype=torch.int32, device="cuda:0")
        if data is not None:
            a = np.ascontiguousarray(data)
            b = np.frombuffer(a.tobytes() + b"\xa5" * (-a.nbytes % 4), dtype=np.int32)
            assert len(b) <= self.words
            self.t[:len(b)].copy_(torch.from_numpy(b.copy()))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guard_ok(self):
        return bool((self.t[self.words:] == FILL32 - (1 << 32)).all())

    def untouched(self):
        return bool((self.t == FILL32 - (1 << 32)).all())

    def read(self, dtype=np.uint32, count=None):
        a = self.t[:self.words].cpu().numpy().view(dtype)
        return a if count is None else a[:count]


def _sync():
    import torch
    torch.cuda.synchronize()


def _guards(bufs, what):
    for name, b in bufs.items():
        assert b.guard_ok(), f"{what}: guard of {name} ({b.words} words) overwritten"


def scan_input(kind, n):
    rng = np.random.default_rng(n + 17)
    if kind == "ones":
        return np.ones(n, dtype=np.uint32)
    if kind == "small":
        return rng.integers(0, 4, n).astype(np.uint32)
    if kind == "last_one":
        a = np.zeros(n, dtype=np.uint32)
        a[-1:] = 1
        return a
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def check_scan(n, kind, inplace):
    L = lib()
    what = f"scan n={n} {kind} {'in place' if inplace else 'out of place'}"
    a = scan_input(kind, n)
    tw = L.shd_scan_tmp_words(n)
    assert tw == scan_tmp_words_ref(n), (what, tw)
    src = Dev(n, a)
    dst = src if inplace else Dev(n)
    tmp = Dev(tw)
    rc = L.shd_exclusive_scan(src.ptr, dst.ptr, n, tmp.ptr, None)
    _sync()
    assert rc == 0, (what, rc)
    _guards(dict(src=src, dst=dst, tmp=tmp), what)
    if n == 0:
        assert tmp.untouched() and dst.untouched(), what + ": n = 0 wrote"
        return
    got = dst.read()
    want = scan_ref(a)
    assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:4])
    if not inplace:
        assert np.array_equal(src.read(), a), what + ": input changed"


def _first_diff(got, want):
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    d = np.flatnonzero(got != want)
    return f"{len(d)} differ, first at {d[:3]}: got {got[d[:3]]} want {want[d[:3]]}"


def run_segment(keys, nkeys, api="segment", want_segments=1, tile_shift=0, widths=None, n=None):
    """one call on the null stream at the exact workspace sizes (keys None: an
    unpartitioned batch of n events). Returns dict(perm, skeys, seg, nseg, cols):
    numpy copies (None where not produced), and the buffers."""
    L = lib()
    n = n if keys is None else len(keys)
    what = f"{api} nkeys={nkeys} n={n} tile_shift={tile_shift} want_segments={want_segments} widths={widths}"
    hw = hist_words(n, nkeys, tile_shift)
    bufs = dict(keys_a=Dev(n), keys_b=Dev(n), idx_a=Dev(n), idx_b=Dev(n), hist=Dev(hw),
                scan_tmp=Dev(L.shd_scan_tmp_words(max(hw, n))), seg_off=Dev(3 * n + 2))
    if keys is not None:
        bufs["keys"] = Dev(n, keys)
    ws = shd_segment_ws(cap=n, **{k: bufs[k].ptr for k in ("keys_a", "keys_b", "idx_a", "idx_b", "hist", "scan_tmp",
                                                           "seg_off")})
    b = shd_batch(keys=bufs["keys"].ptr if keys is not None else None, n=n)
    perm_p, skeys_p = C.c_void_p(1), C.c_void_p(1)
    cols = None
    if api == "segment":
        rc = L.shd_segment(C.byref(b), nkeys, C.byref(ws), None, C.byref(perm_p), C.byref(skeys_p))
    else:
        carry, mid = None, None
        if widths:
            cols = [payload_column(w, n, c) for c, w in enumerate(widths)]
            carry = shd_payload(n=len(widths))
            mid = (C.c_void_p * 8)()
            for c, w in enumerate(widths):
                words = (n * w + 3) // 4
                bufs[f"src{c}"], bufs[f"dst{c}"], bufs[f"mid{c}"] = Dev(words, cols[c]), Dev(words), Dev(words)
                carry.src[c], carry.dst[c], carry.width[c] = bufs[f"src{c}"].ptr, bufs[f"dst{c}"].ptr, w
                mid[c] = bufs[f"mid{c}"].ptr
        rc = L.shd_segment_payload(C.byref(b), nkeys, C.byref(ws), None, C.byref(perm_p), C.byref(skeys_p),
                                   C.byref(carry) if carry else None, mid, tile_shift, want_segments)
    _sync()
    assert rc == 0, (what, rc)
    _guards(bufs, what)
    out = dict(what=what, perm=None, skeys=None, seg=None, nseg=None, cols=None, n=n, bufs=bufs)
    if keys is None:
        assert perm_p.value is None and skeys_p.value is None, what + ": outputs not NULL without keys"
    else:
        by_ptr = {bufs[k].ptr: bufs[k] for k in ("keys_a", "keys_b", "idx_a", "idx_b")}
        assert perm_p.value in by_ptr and skeys_p.value in by_ptr, what + ": outputs outside the workspace"
        out["perm"] = by_ptr[perm_p.value].read()
        out["skeys"] = by_ptr[skeys_p.value].read()
        assert np.array_equal(bufs["keys"].read(np.int32), keys), what + ": input keys changed"
    if want_segments:
        so = bufs["seg_off"].read()
        out["nseg"] = int(so[3 * n])
        assert 0 <= out["nseg"] <= n, (what, out["nseg"])
        out["seg"] = so[2 * n:2 * n + out["nseg"]]
    else:
        assert bufs["seg_off"].untouched(), what + ": segment list written with want_segments = 0"
    if widths:
        out["cols"] = [bufs[f"dst{c}"].read(cols[c].dtype, n) for c in range(len(widths))]
        for c in range(len(widths)):
            assert np.array_equal(bufs[f"src{c}"].read(cols[c].dtype, n), cols[c]), what + ": payload source changed"
        out["src_cols"] = cols
    return out


def compare_segment(out, keys, nkeys, tile_shift=0):
    what = out["what"]
    perm, skeys, seg, nseg = segment_ref(keys, nkeys, tile_shift)
    assert np.array_equal(out["perm"], perm), what + ": perm " + _first_diff(out["perm"], perm)
    assert np.array_equal(out["skeys"], skeys), what + ": skeys " + _first_diff(out["skeys"], skeys)
    if out["seg"] is not None:
        assert out["nseg"] == nseg, (what, "segment count", out["nseg"], nseg)
        assert np.array_equal(out["seg"], seg), what + ": segment list " + _first_diff(out["seg"], seg)
    if out["cols"] is not None:
        for c, got in enumerate(out["cols"]):
            want = payload_ref(out["src_cols"][c], perm)
            assert np.array_equal(got, want), what + f": payload column {c} " + _first_diff(got, want)


def check_segment(nkeys, n, patterns=None):
    """shd_segment, and shd_segment_payload with and without the segment list,
    over every key pattern"""
    for p in patterns or patterns_for(n):
        keys = make_keys(p, n, nkeys)
        for api, ws in (("segment", 1), ("payload", 1), ("payload", 0)):
            out = run_segment(keys, nkeys, api, ws)
            out["what"] += " " + p
            compare_segment(out, keys, nkeys)


def check_no_keys(n):
    """keys = NULL: no order (both outputs NULL), one segment, the sort's buffers untouched"""
    for api in ("segment", "payload"):
        out = run_segment(None, 7, api, 1, n=n)
        what = out["what"] + " keys=NULL"
        assert out["nseg"] == 1 and out["seg"].tolist() == [0], (what, out["nseg"], out["seg"][:4])
        for k in ("keys_a", "keys_b", "idx_a", "idx_b", "hist"):
            assert out["bufs"][k].untouched(), what + f": {k} written"


def check_seam(nkeys):
    """n = 4,096 (one workgroup) and n = 4,097 (radix path) over the same first
    4,096 events agree once the extra event is dropped"""
    for p in ("uniform", "nulls10", "top_digit"):
        keys = make_keys(p, SMALL_MAX + 1, nkeys)
        a = run_segment(keys[:-1], nkeys)
        b = run_segment(keys, nkeys)
        keep = b["perm"] != SMALL_MAX
        what = f"seam nkeys={nkeys} {p}"
        assert keep.sum() == SMALL_MAX, what
        assert np.array_equal(a["perm"], b["perm"][keep]), what + ": perm " + _first_diff(a["perm"], b["perm"][keep])
        assert np.array_equal(a["skeys"], b["skeys"][keep]), what + ": skeys"
        compare_segment(a, keys[:-1], nkeys)
        compare_segment(b, keys, nkeys)


def check_payload(nkeys, n, widths, patterns=PAYLOAD_PATTERNS):
    for p in patterns:
        keys = make_keys(p, n, nkeys)
        for ws in (1, 0):
            out = run_segment(keys, nkeys, "payload", ws, 0, widths)
            out["what"] += " " + p
            compare_segment(out, keys, nkeys)


def check_tiled(shift, nkeys, n, patterns=TILED_PATTERNS):
    """the tile-major form as the window engine calls it (no segment list), bare
    and with a payload, and its tile directory for small key counts"""
    L = lib()
    for p in patterns:
        keys = make_keys(p, n, nkeys)
        for widths in (None, TILED_WIDTHS):
            out = run_segment(keys, nkeys, "payload", 0, shift, widths)
            out["what"] += " " + p
            compare_segment(out, keys, nkeys, shift)
        if nkeys > 300:
            continue
        K1 = nkeys + 1
        ntile = (n + (1 << shift) - 1) >> shift
        sk = Dev(n, out["skeys"])
        ds, de = Dev(ntile * K1), Dev(ntile * K1)
        rc = L.shd_tile_dir(sk.ptr, n, shift, K1, ntile, ds.ptr, de.ptr, None)
        _sync()
        what = f"tile_dir shift={shift} nkeys={nkeys} n={n} {p}"
        assert rc == 0, (what, rc)
        _guards(dict(skeys=sk, ds=ds, de=de), what)
        wds, wde = tile_dir_ref(out["skeys"], n, shift, K1)
        assert np.array_equal(ds.read().reshape(ntile, K1), wds), what + ": ds " + _first_diff(ds.read(), wds.ravel())
        assert np.array_equal(de.read().reshape(ntile, K1), wde), what + ": de " + _first_diff(de.read(), wde.ravel())


def sort_keys(bits, n):
    rng = np.random.default_rng(bits * 1009 + n)
    k = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    if n > 8:
        k[rng.integers(0, n, n // 4)] = k[0]           # ties in every tile: stability
    return (k & np.uint64((1 << bits) - 1)).astype(np.uint32)


def check_sort_pairs(bits, n):
    L = lib()
    keys = sort_keys(bits, n)
    ntiles = (n + RADIX_TILE - 1) // RADIX_TILE
    passes = (bits + 7) // 8
    for with_vals in (True, False):
        what = f"sort_pairs bits={bits} n={n} vals={'given' if with_vals else 'NULL'}"
        vals = (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) if with_vals else None
        bufs = dict(keys=Dev(n, keys), k0=Dev(n), k1=Dev(n), v0=Dev(n), v1=Dev(n), hist=Dev(256 * ntiles),
                    scan_tmp=Dev(L.shd_scan_tmp_words(256 * ntiles)))
        if with_vals:
            bufs["vals"] = Dev(n, vals)
        kb = (C.c_void_p * 2)(bufs["k0"].ptr, bufs["k1"].ptr)
        vb = (C.c_void_p * 2)(bufs["v0"].ptr, bufs["v1"].ptr)
        ko, vo = C.c_void_p(1), C.c_void_p(1)
        vptr = bufs["vals"].ptr if with_vals else None
        rc = L.shd_sort_pairs(bufs["keys"].ptr, vptr, n, bits, kb, vb, bufs["hist"].ptr, bufs["scan_tmp"].ptr, None,
                              C.byref(ko), C.byref(vo))
        _sync()
        assert rc == 0, (what, rc)
        _guards(bufs, what)
        assert np.array_equal(bufs["keys"].read(), keys), what + ": input keys changed"
        if passes == 0 or n == 0:
            # nothing ran: the inputs come back and nothing is written
            assert ko.value == bufs["keys"].ptr and vo.value == vptr, what + ": returned pointers"
            for k in ("k0", "k1", "v0", "v1", "hist", "scan_tmp"):
                assert bufs[k].untouched(), what + f": {k} written"
            continue
        last = (passes - 1) & 1
        assert ko.value == kb[last] and vo.value == vb[last], what + ": returned pointers"
        wk, wv = sort_pairs_ref(keys, vals, bits)
        gk, gv = bufs[f"k{last}"].read(), bufs[f"v{last}"].read()
        assert np.array_equal(gk, wk), what + ": keys " + _first_diff(gk, wk)
        assert np.array_equal(gv, wv), what + ": vals " + _first_diff(gv, wv)


def check_radix10(nkeys, n):
    """global and tile-major, with a payload (meant for a process with SH_RADIX10=1;
    the sizes follow the process's setting either way)"""
    for p in ("uniform", "top_digit", "nulls10"):
        keys = make_keys(p, n, nkeys)
        for shift in (0, 12, 13):
            for ws in ((1, 0) if shift == 0 else (0,)):
                out = run_segment(keys, nkeys, "payload", ws, shift, (8, 4, 1))
                out["what"] += " " + p
                compare_segment(out, keys, nkeys, shift)
        out = run_segment(keys, nkeys, "segment")
        compare_segment(out, keys, nkeys)


def run_subset(name, report=lambda s: None):
    """the cases of one named subset, in order"""
    def each(fn, cases):
        for c in cases:
            report(f"{name} {fn.__name__} {c}")
            fn(*c)
    if name == "scan":
        each(check_scan, [(n, k, ip) for n in SCAN_NS for k in SCAN_INPUTS for ip in (False, True)])
    elif name == "segment":
        each(check_segment, SEG_CASES)
        each(check_no_keys, [(5,), (SMALL_MAX + 1,)])
    elif name == "small":
        each(check_segment, [c for c in SEG_CASES if c[1] <= SMALL_MAX])
    elif name == "large":
        each(check_segment, [c for c in SEG_CASES if c[1] > SMALL_MAX])
    elif name == "seam":
        each(check_seam, [(nk,) for nk in SEAM_NKEYS])
    elif name == "payload":
        each(check_payload, PAYLOAD_CASES)
    elif name == "tiled":
        each(check_tiled, TILED_CASES)
    elif name == "sort":
        each(check_sort_pairs, SORT_CASES)
    elif name == "radix10":
        each(check_radix10, [(nk, n) for nk in RADIX10_NKEYS for n in RADIX10_NS])
    else:
        raise ValueError(name)
