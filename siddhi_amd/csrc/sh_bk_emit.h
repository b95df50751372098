// sh_bk_emit.h — the bucketed engine's emitter (device side), one source for two
// compilers: sh_bucket.hip instantiates the generic k_bk_emit<layout, values, ...>,
// whose select descriptors are kernel arguments read at run time; sh_jit.cpp
// (hipRTC) compiles the same row loop per (select list, output layout) with the
// descriptors as constexpr tables defined before this text (BKS_NO and its
// companions, see sh_rows.h; BKS_NAME, BKS_RU and BKS_OCC: the kernel's name, its
// rows per lane and round and its waves per SIMD), so that the type switches, the
// widening to 8 bytes and the packed-word selects fold away.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sh_query.h"
#include "sh_device.h"
#include "sh_rows.h"
#include "sh_wave.h"

#define BK_TPB 512
#define BK_ITEMS (SHB_TILE / BK_TPB)

static_assert(BK_ITEMS == 16, "tile / threads");


// XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs, so
// block `bid` takes tile (bid % 8) * per + bid / 8 and each XCD walks a
// contiguous run of arrival tiles; the (bucket, tile) segments of neighbouring
// tiles share cache lines (partial-line writes of the scatter, count and
// match-stream gathers of the emitter) and now meet in the same L2. -1: none.
// (the grid: bk_grid, sh_bucket.hip)
__device__ __forceinline__ int bk_tile(int nt) {
    const int per = (nt + 7) >> 3;
    const int t = (int)(blockIdx.x & 7u) * per + (int)(blockIdx.x >> 3);
    return t < nt ? t : -1;
}
// the same order over the tiles [t0, t1) of one launch (grid: bk_grid(t1 - t0))
__device__ __forceinline__ int bk_tile(int t0, int t1) {
    const int t = bk_tile(t1 - t0);
    return t < 0 ? -1 : t0 + t;
}

// ---------------------------------------------------------------- emitter
// Per arrival tile, 8 waves of 1,024 consecutive events each:
//  1. the tile's counts in its bucket order (one 16-byte load per thread) ->
//     their exclusive prefix pfx[slot] (LDS): an event of bucket d at slot s has
//     count pfx[s+1] - pfx[s] and match-stream position mstart[T][d] + pfx[s] -
//     pfx[toff[d]] (the matcher wrote each (tile, bucket) segment's matches
//     contiguously, in arrival order)
//  2. per wave: the counts and positions of its events (registers), its total
//  3. per half-wave-block of 512 events: a DPP scan gives each event its first
//     row; the wave's row map (row -> event) is filled and lane t writes rows t,
//     t + 64, ... (consecutive lanes, consecutive rows: coalesced stores); the
//     consumer-side values are read by arrival index, the e1-side values from
//     the match stream
#define BK_EHALF 512   // events of one row-map pass of a wave
#define BK_PFX_BITS 24  // pfx words: prefix in the low bits, the slot's bucket above
#define BK_PFX_MASK ((1u << BK_PFX_BITS) - 1u)
#define BK_NOSLOT 0xFFFFFFFFu
#define BK_EROWS 1024  // rows the wave's map holds per pass (more: event-parallel writes)

// select value o of a row (raw 8-byte form; kind 0: by match-stream position, 1: by event)
#define BK_VAL(o, i, mp, row) bk_raw(O.src[o], BK_KIND(o) == 1 ? (i) : (mp), BK_TYPE(o))


// the select values of a row (NO > 0: unrolled, the descriptors in scalar registers
// or, in a specialised build, constants)
template <int NO>
__device__ __forceinline__ void bk_vals(const bk_out_t& O, int64_t i, int64_t mp, int64_t row, int64_t* v) {
#pragma unroll
    for (int o = 0; o < NO; o++) v[o] = BK_VAL(o, i, mp, row);
}


template <int MODE, int NO>
__device__ __forceinline__ void bk_row(const bk_out_t& O, const bk_cols_t& OC, const int32_t* o_kind,
                                       const int32_t* o_type, const void* const* o_src, int64_t row, int64_t i,
                                       int64_t mp, uint64_t seq, uint64_t* __restrict__ out_seq,
                                       int64_t* __restrict__ out_vals) {
    if (NO > 0) {
        int64_t v[NO > 0 ? NO : 1];
        bk_vals<NO>(O, i, mp, row, v);
        bk_store<MODE, NO>(OC, row, v, seq, out_seq, out_vals);
        return;
    }
#ifndef BKS_NO
    // any number of values: the descriptors from LDS, one value at a time
    const int no = O.n_out;
    if (MODE == SHB_OUT_PACKED) {
        uint32_t* r = (uint32_t*)OC.rows + row * OC.rw;
        r[0] = (uint32_t)seq;
        r[1] = (uint32_t)(seq >> 32);
        for (int k = 2; k < OC.rw; k++) r[k] = 0u;
    } else if (out_seq) {
        out_seq[row] = seq;
    }
    for (int o = 0; o < no; o++) {
        const int64_t v = bk_raw(o_src[o], o_kind[o] == 1 ? i : mp, o_type[o]);
        if (MODE == SHB_OUT_PACKED) {
            uint32_t* r = (uint32_t*)OC.rows + row * OC.rw + OC.woff[o];
            r[0] = OC.colw[o] == 1 ? (uint32_t)(uint8_t)v : (uint32_t)v;
            if (OC.colw[o] == 8) r[1] = (uint32_t)((uint64_t)v >> 32);
        } else if (MODE == SHB_OUT_COLS) {
            bk_put(OC.cols[o], OC.colw[o], row, v);
        } else if (out_vals) {
            out_vals[row * no + o] = v;
        }
    }
#endif
}

// one arrival tile per workgroup. BK_RU: rows per lane whose loads are issued before
// their stores (a half of 512 events has ~290 rows on C2). The generic emitter takes
// the select's descriptors as kernel arguments; a specialised one (BKS_NAME) takes the
// plan and the pointers, its template parameters are the constants of its build
// (One body behind two signatures, not a __device__ function that both kernels call:
// with the body in a function taking the arguments by reference the generic kernels
// compiled worse -- k_bk_emit<2, 4, 3, 6> went from 0 to 12 VGPR spills and from 60 to
// 173 SGPR spills -- and they have to stay what they were. o_kind / o_type / o_src
// serve the generic any-width path alone; unused, they take no LDS.)
#ifdef BKS_NO
extern "C" __global__ void __launch_bounds__(BK_TPB, BKS_OCC) BKS_NAME(shb_plan P, bks_ptrs Q, uint64_t seq_base,
                                                               uint64_t* __restrict__ out_seq,
                                                               int64_t* __restrict__ out_vals, int64_t out_cap) {
    constexpr int MODE = BKS_MODE, NO = BKS_NO, BK_RU = BKS_RU, BK_OCC = BKS_OCC;
    const bks_ptrs &O = Q, &OC = Q;
#else
template <int MODE, int NO, int BK_RU, int BK_OCC = 4>
__global__ void __launch_bounds__(BK_TPB, BK_OCC) k_bk_emit(shb_plan P, shb_out O, shb_cols OC, uint64_t seq_base,
                                                    uint64_t* __restrict__ out_seq, int64_t* __restrict__ out_vals,
                                                    int64_t out_cap) {
#endif
    // the slot prefix (phases 1-2) and the row maps (phase 3) share storage: phase 3
    // starts after the barrier that ends every wave's phase 2 (42 KB instead of 75:
    // three workgroups per CU when the registers allow)
    // LM (6 waves per SIMD, <= 80 VGPRs): the wave's 1,024 match-stream positions go
    // to LDS once (emp holds both halves) instead of living in registers through the
    // row loop, and a half's row map holds 512 rows (more: the event-parallel path)
    constexpr bool LM = BK_OCC >= 6;
    constexpr int EROWS = LM ? 512 : BK_EROWS;
    constexpr int EMPW = LM ? 2 * BK_EHALF : BK_EHALF;
    constexpr int BK_MAPW = (BK_TPB / 64) * (EROWS / 2 + EMPW + BK_EHALF / 2);
    __shared__ uint32_t pool[(SHB_TILE + 1) > BK_MAPW ? (SHB_TILE + 1) : BK_MAPW];
    uint32_t* const pfx = pool;
    uint16_t(*const rmap)[EROWS] = (uint16_t(*)[EROWS])pool;
    uint32_t(*const emp)[EMPW] = (uint32_t(*)[EMPW])(pool + (BK_TPB / 64) * (EROWS / 2));
    uint16_t(*const ero)[BK_EHALF] =
        (uint16_t(*)[BK_EHALF])(pool + (BK_TPB / 64) * (EROWS / 2 + EMPW));
    __shared__ uint32_t ms0[SHB_NB];
    __shared__ uint16_t to[SHB_NB + 1];
    __shared__ uint32_t wtot[BK_TPB / 64], ws[BK_TPB / 64];
    __shared__ int32_t o_kind[SHB_MAX_OUT], o_type[SHB_MAX_OUT];
    __shared__ const void* o_src[SHB_MAX_OUT];
    __shared__ uint32_t s_tb;
    constexpr int NV = NO > 0 ? NO : 1;
    const int T = bk_tile(P.et0, P.et1);
    if (T < 0) return;
    const int64_t b0 = (int64_t)T << SHB_TILE_SHIFT;
    const int tile_n = (int)((P.n - b0) < SHB_TILE ? (P.n - b0) : SHB_TILE);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x <= SHB_NB) to[threadIdx.x] = P.toff[(int64_t)T * SHB_TOFF + threadIdx.x];
    if (threadIdx.x < SHB_NB) ms0[threadIdx.x] = P.mstart[(int64_t)T * SHB_NB + threadIdx.x];
    if (threadIdx.x == 0) s_tb = P.ttot[T];
#ifndef BKS_NO
    if (NO == 0 && threadIdx.x < SHB_MAX_OUT) {
#pragma unroll
        for (int o = 0; o < SHB_MAX_OUT; o++)
            if (o == (int)threadIdx.x) {
                o_kind[o] = O.kind[o];
                o_type[o] = O.type[o];
                o_src[o] = O.src[o];
            }
    }
#endif
    // the events of this wave (arrival order): their slots, loaded up front (the
    // bucket of a slot follows from the tile's bucket starts: no key read)
    uint32_t sl[BK_ITEMS];
    {
        const int l0 = w * (64 * BK_ITEMS) + lane;
#pragma unroll
        for (int j = 0; j < BK_ITEMS; j++) {
            const int l = l0 + j * 64;
            sl[j] = l < tile_n ? (uint32_t)P.sp[b0 + l] : BK_NOSLOT;
        }
    }
    // 1. counts in the tile's bucket order -> pfx (loaded with the events; the
    // slots past the tile's valid events are masked below). Each word holds the
    // exclusive prefix (< 2^21: 8,192 counts of at most 255) and, in its top 8
    // bits, the slot's bucket: a thread's 16 consecutive slots find theirs by one
    // binary search over the bucket starts and a forward walk
    {
        const int s0 = threadIdx.x * 16;
        const uint4 q = *(const uint4*)(P.cnt + b0 + s0);
        __syncthreads();
        const int nv = to[SHB_NB];
        uint32_t c[16];
        const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            c[k] = (s0 + k < nv) ? (wd[k >> 2] >> (8 * (k & 3))) & 0xFFu : 0u;
            sum += c[k];
        }
        uint32_t tot;
        uint32_t off = shw_block_excl<BK_TPB>(sum, ws, &tot);
        int d = 0;  // the last bucket whose start is <= s0
        {
            int lo = 0, hi = SHB_NB - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if ((int)to[mid] <= s0) lo = mid;
                else hi = mid - 1;
            }
            d = lo;
        }
#pragma unroll
        for (int k = 0; k < 16; k++) {
            while (d < SHB_NB - 1 && (int)to[d + 1] <= s0 + k) d++;
            pfx[s0 + k] = off | ((uint32_t)d << BK_PFX_BITS);
            off += c[k];
        }
        if (threadIdx.x == 0) pfx[SHB_TILE] = tot;
        __syncthreads();
    }
    // 2. counts (4 packed per register) and match-stream positions of the wave's events
    uint32_t cp[BK_ITEMS / 4];
    uint32_t mp[BK_ITEMS];
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < BK_ITEMS; j++) {
        uint32_t c = 0;
        mp[j] = 0u;
        if (sl[j] != BK_NOSLOT) {
            const uint32_t s = sl[j];
            const uint32_t pw = pfx[s];
            const uint32_t d = pw >> BK_PFX_BITS;
            const uint32_t ps = pw & BK_PFX_MASK;
            c = (pfx[s + 1] & BK_PFX_MASK) - ps;
            mp[j] = ms0[d] + ps - (pfx[to[d]] & BK_PFX_MASK);
        }
        if ((j & 3) == 0) cp[j >> 2] = 0u;
        cp[j >> 2] |= c << (8 * (j & 3));
        mine += c;
    }
    {
        const uint32_t wsum = shw_last(shw_incl_scan(mine));
        if (lane == 0) wtot[w] = wsum;
    }
    __syncthreads();
    if (LM) {
#pragma unroll
        for (int j = 0; j < BK_ITEMS; j++) emp[w][j * 64 + lane] = mp[j];
    }
    uint64_t rb = s_tb;  // this wave's first row
    for (int q = 0; q < w; q++) rb += wtot[q];
    // 3. rows, one half (512 events) at a time
#pragma unroll
    for (int hf = 0; hf < BK_ITEMS / 8; hf++) {
        uint32_t carry = 0;
        uint32_t ro8[8];
#pragma unroll
        for (int jj = 0; jj < 8; jj++) {
            const int j = hf * 8 + jj;
            const uint32_t c = (cp[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            const uint32_t incl = shw_incl_scan(c);
            const uint32_t ro = carry + incl - c;
            if (!LM) ro8[jj] = ro;
            const int e = jj * 64 + lane;
            if (!LM) emp[w][e] = mp[j];
            ero[w][e] = (uint16_t)ro;
            for (uint32_t k = 0; k < c; k++)
                if (ro + k < EROWS) rmap[w][ro + k] = (uint16_t)e;
            carry += shw_last(incl);
        }
        const uint32_t R = carry;
        const int64_t ib = b0 + (int64_t)w * (64 * BK_ITEMS) + hf * BK_EHALF;  // arrival index of event 0 of the half
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int eo = LM ? hf * BK_EHALF : 0;  // the half's first entry of emp
        if (R <= EROWS) {
            // row-parallel: lane t writes rows t, t + 64, ... (consecutive lanes,
            // consecutive rows); BK_RU rows' loads go out before their stores
            if (NO > 0) {
                for (uint32_t t0 = 0; t0 < R; t0 += 64 * BK_RU) {
                    int64_t v[BK_RU][NV];
                    int64_t ii[BK_RU];
                    bool ok[BK_RU];
#pragma unroll
                    for (int u = 0; u < BK_RU; u++) {
                        const uint32_t t = t0 + u * 64 + lane;
                        ok[u] = t < R && (int64_t)rb + t < out_cap;  // (past out_cap: the host reports SH_E_MORE)
                        ii[u] = ib;
                        if (ok[u]) {
                            const int e = rmap[w][t];
                            const uint32_t k = t - ero[w][e];
                            ii[u] = ib + e;
                            bk_vals<NV>(O, ii[u], (int64_t)emp[w][eo + e] + k, (int64_t)rb + t, v[u]);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < BK_RU; u++)
                        if (ok[u])
                            bk_store<MODE, NV>(OC, (int64_t)rb + t0 + u * 64 + lane, v[u],
                                                           seq_base + (uint64_t)ii[u], out_seq, out_vals);
                }
            } else {
                for (uint32_t t = lane; t < R; t += 64) {
                    const int e = rmap[w][t];
                    const uint32_t k = t - ero[w][e];
                    const int64_t i = ib + e;
                    const int64_t row = (int64_t)rb + t;
                    if (row >= out_cap) continue;  // the host reports SH_E_MORE
                    bk_row<MODE, NO>(O, OC, o_kind, o_type, o_src, row, i, (int64_t)emp[w][eo + e] + k,
                                     seq_base + (uint64_t)i, out_seq, out_vals);
                }
            }
        } else {
            // a dense half (more rows than the map holds): each event writes its rows
            // (LM: its first row from the same scan again, not kept in registers)
            uint32_t carry2 = 0;
#pragma unroll
            for (int jj = 0; jj < 8; jj++) {
                const int j = hf * 8 + jj;
                const uint32_t c = (cp[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                const int64_t i = ib + jj * 64 + lane;
                uint32_t ro = 0;
                if (LM) {
                    const uint32_t incl = shw_incl_scan(c);
                    ro = carry2 + incl - c;
                    carry2 += shw_last(incl);
                } else {
                    ro = ro8[jj];
                }
                for (uint32_t k = 0; k < c; k++) {
                    const int64_t row = (int64_t)rb + ro + k;
                    if (row >= out_cap) break;
                    bk_row<MODE, NO>(O, OC, o_kind, o_type, o_src, row, i,
                                     (int64_t)(LM ? emp[w][j * 64 + lane] : mp[j]) + k,
                                     seq_base + (uint64_t)i, out_seq, out_vals);
                }
            }
        }
        rb += R;
        // the map is rewritten by the next half: this wave's reads come first
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

