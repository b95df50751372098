"""CPU side of the device-primitive tests (tests/device_prims.py): the ctypes mirrors
against the header's real layout, the premises of the case lists (so that a later
edit cannot hollow them out), the numpy contracts against naive loops, and the
arithmetic of the callers' workspace sizes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import device_prims as dp

HERE = os.path.dirname(os.path.abspath(__file__))


def test_struct_layout_matches_header():
    d = os.path.join(HERE, "prims_layout")
    subprocess.run(["make", "-s", "-C", d], check=True)
    r = subprocess.run([os.path.join(d, "prims_layout")], capture_output=True, text=True, timeout=60, check=True)
    seen = {}
    for line in r.stdout.split("\n"):
        if line:
            s, m, v = line.split()
            seen.setdefault(s, {})[m] = int(v)
    assert set(seen) == set(dp.MIRRORS)
    for name, cls in dp.MIRRORS.items():
        want = {"sizeof": C.sizeof(cls)}
        want.update({f: getattr(cls, f).offset for f, _ in cls._fields_})
        assert seen[name] == want, name


def test_pass_counts_of_the_segment_list():
    assert [dp.seg_passes(nk) for nk in (255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24)] == [1, 2, 2, 3, 3, 4]
    assert {dp.seg_passes(nk) for nk in dp.SEG_NKEYS} == {1, 2, 3, 4}
    assert [dp.seg_passes(nk) for nk in dp.PAYLOAD_NKEYS] == [1, 2, 3, 4]
    # a count of keys that is a power of two needs one bit more than its largest key
    for nk in (2, 256, 65536, 2 ** 24):
        assert nk in dp.SEG_NKEYS and dp.bits_for(nk) == dp.bits_for(nk - 1) + 1
    # the 10-bit digit range
    assert all(16 < dp.bits_for(nk) <= 20 for nk in dp.RADIX10_NKEYS)


def test_segment_list_meets_what_it_must():
    cases = set(dp.SEG_CASES)
    for nk in dp.SEG_NKEYS:
        assert {(nk, 4096), (nk, 4097), (nk, 34 * 4096 + 5)} <= cases
    for n in dp.SEG_NS:
        assert {(256, n), (65536, n)} <= cases
    assert (34 * 4096 + 5 + 4095) // 4096 % 8 != 0          # a tile count the XCD mapping pads
    assert max(n for _, n in cases) == 139_269
    assert set(dp.PAYLOAD_NS) == {4097, 34 * 4096 + 5} and all(n > dp.SMALL_MAX for n in dp.PAYLOAD_NS)
    assert [len(w) for w in dp.PAYLOAD_WIDTHS] == [1, 3, 8]
    for s, nk, n in dp.TILED_CASES:
        assert n > (1 << s)                                  # at least two arrival tiles
    # the tile-major list has padding blocks (a block count no multiple of the tile's) and a short last tile
    assert any(dp.padded_tiles(n, s) > dp.padded_tiles(n) for s, _, n in dp.TILED_CASES)
    assert {n for b, n in dp.SORT_CASES} >= {16 * 4096, 16 * 4096 + 1}      # 16 against 17 tiles
    assert {(b + 7) // 8 for b, _ in dp.SORT_CASES} == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("pattern,nkeys,n", dp.stability_cases())
def test_stability_cases_have_a_key_over_two_waves_and_two_tiles(pattern, nkeys, n):
    keys = dp.make_keys(pattern, n, nkeys).astype(np.int64)
    i = np.arange(n)
    tile, wave = i // dp.RADIX_TILE, i % dp.RADIX_TILE // (dp.RADIX_TILE // dp.WAVES_PER_TILE)
    ok = False
    for k in np.unique(keys)[:300]:
        at = keys == k
        tiles = np.unique(tile[at])
        two_waves = any(len(np.unique(wave[at & (tile == t)])) >= 2 for t in tiles[:3])
        if len(tiles) >= 2 and two_waves:
            ok = True
            break
    assert ok


def test_null_cases_hold_null_and_other_events():
    for nk, n in dp.SEG_CASES:
        for p in dp.patterns_for(n):
            keys = dp.make_keys(p, n, nk)
            assert len(keys) == n and keys.dtype == np.int32
            if p == "all_null":
                assert (keys == -1).all()
            elif p in dp.NULL_PATTERNS:
                assert (keys == -1).any() and (keys >= 0).any(), (p, nk, n)
            else:
                assert (keys >= 0).all()
        assert set(dp.PATTERNS) - set(dp.patterns_for(n)) <= ({"nulls10", "null_alt"} if n < 2 else set())
    for nk in dp.TILED_NKEYS:
        for p in dp.TILED_PATTERNS:
            if p in dp.NULL_PATTERNS:
                keys = dp.make_keys(p, 4097, nk)
                assert (keys == -1).any() and (keys >= 0).any()


def test_patterns_are_what_their_names_say():
    for nk in dp.SEG_NKEYS:
        n = 4097
        top = dp.make_keys("top_digit", n, nk).astype(np.int64)
        low = dp.make_keys("low_digit", n, nk).astype(np.int64)
        shift = 8 * (dp.seg_passes(max(nk - 1, 1)) - 1) if nk > 1 else 0
        assert (top & ((1 << shift) - 1) == 0).all()
        assert len(np.unique(low >> 8)) == 1
        if nk >= n:
            for p in ("ascending", "descending"):
                assert len(np.unique(dp.make_keys(p, n, nk))) == n
        assert (np.diff(dp.make_keys("ascending", n, nk).astype(np.int64)) >= 0).all()
        assert (np.diff(dp.make_keys("descending", n, nk).astype(np.int64)) <= 0).all()
    for w in (8, 4):
        assert len(np.unique(dp.payload_column(w, 139_269, 3))) == 139_269


def test_references_agree_with_naive_loops():
    rng = np.random.default_rng(3)
    n = 200
    a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    acc, want = 0, []
    for v in a:
        want.append(acc & 0xFFFFFFFF)
        acc += int(v)
    assert dp.scan_ref(a).tolist() == want
    assert dp.scan_ref(a[:0]).tolist() == [] and dp.scan_ref(a[:1]).tolist() == [0]
    for nkeys, shift in ((5, 0), (5, 6), (64, 0)):
        keys = rng.integers(-1, nkeys, n)
        T = 1 << shift if shift else n
        perm = []
        for b in range(0, n, T):
            blk = list(range(b, min(n, b + T)))
            perm += sorted(blk, key=lambda i: (nkeys if keys[i] < 0 else keys[i], i))
        sk = [nkeys if keys[i] < 0 else int(keys[i]) for i in perm]
        seg = [p for p in range(n) if (p == 0 or sk[p - 1] != sk[p]) and sk[p] != nkeys]
        gp, gs, gl, gn = dp.segment_ref(keys, nkeys, shift)
        assert gp.tolist() == perm and gs.tolist() == sk and gl.tolist() == seg and gn == len(seg)
        col = dp.payload_column(8, n, 1)
        assert dp.payload_ref(col, gp).tolist() == [int(col[i]) for i in perm]
        if shift:
            K1 = nkeys + 1
            ds, de = dp.tile_dir_ref(gs, n, shift, K1)
            for t in range((n + T - 1) // T):
                for k in range(K1):
                    at = [p for p in range(t * T, min(n, t * T + T)) if sk[p] == k]
                    assert (ds[t, k], de[t, k]) == ((at[0], at[-1] + 1) if at else (0, 0))
    k = rng.integers(0, 8, n).astype(np.uint32)
    v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    order = sorted(range(n), key=lambda i: (k[i], i))
    gk, gv = dp.sort_pairs_ref(k, v, 3)
    assert gk.tolist() == [int(k[i]) for i in order] and gv.tolist() == [int(v[i]) for i in order]
    assert dp.sort_pairs_ref(k, None, 3)[1].tolist() == order


def test_scan_workspace_restatement():
    assert dp.scan_tmp_words_ref(0) == dp.scan_tmp_words_ref(1024) == 4
    assert dp.scan_tmp_words_ref(1025) == 2 * 2 + 2 + 4
    assert dp.scan_tmp_words_ref(1024 ** 2 + 1) == 2 * 1025 + 2 + 2 * 2 + 2 + 4
    # the three-level cases of the scan list and the two ways to get there
    assert sum(n > 1024 ** 2 for n in dp.SCAN_NS) >= 2 and 256 * 4097 > 1024 ** 2


@pytest.mark.parametrize("shift", range(12, 25))
def test_host_histogram_covers_every_tile_shift(shift):
    """sh_host.cpp ensure_ws sizes the histogram as 1024 x (blocks + 256) words; the
    tile-major form pads the block count to whole arrival tiles. At the smallest n
    that gives two tiles (the most padding per event) the allocation must hold
    2^db x padded blocks for both digit widths the segment can pick."""
    n = (1 << shift) + 1
    assert dp.padded_tiles(n, shift) == 2 << (shift - 12)
    for radix10 in (False, True):
        for nkeys in (300, 65536, 200_000, 2 ** 20 - 1, 2 ** 20):
            need = dp.hist_words(n, nkeys, shift, radix10)
            assert need <= dp.host_hist_alloc_words(n), (shift, nkeys, radix10, need)
    # 8-bit digits always fit; 10-bit digits fit up to tiles of 2^20 events and are
    # refused beyond (without the refusal: 1024 x 1024 words against 1024 x 769 at 2^21 + 1)
    assert dp.digit_bits(200_000, shift, True) == (10 if shift <= 20 else 8)
    if shift > 20:
        assert 1024 * dp.padded_tiles(n, shift) > dp.host_hist_alloc_words(n)
    assert dp.digit_bits(200_000, shift, False) == dp.digit_bits(65535, shift, True) == 8
    assert dp.digit_bits(2 ** 20, shift, True) == 8
