// sh_agg.hip — select-clause aggregators (sum / avg / count / max / min) behind the
// fast engines.
//
// With aggregators a pattern query's selector keeps one running value per
// partition key and query (AttributeAggregatorExecutor state through the
// partitioned state holder, AttributeAggregatorExecutor.java:52) and emits it
// with every match in match order (a state query's selector sees one state
// event per chunk, QuerySelector.processInBatchNoGroupBy :271-313 keeps it):
//   sum(int|long) -> long  wrap-around long additions
//   sum(float|double), avg(*) -> double: value += (double) x, one double add per
//     match (SumAttributeAggregatorExecutor.java:167-185,
//     AvgAttributeAggregatorExecutor.java:145-155: value / count)
//   count() -> long
//   max(x), min(x) -> x's type: the winning argument's raw bits ("max / min" below;
//     these columns are never "not exact")
// The fast engines (bucketed / window / rise-and-fall / rule set) write the
// aggregator's argument in the aggregate's column; this pass turns the ordered
// rows into the running values.
//
// A chain of double additions is not associative, so the pass first proves it
// does not round: every addend x is an integer multiple of 2^q (q = the lowest
// set bit over all addends) and every running value the reference would form
// is then a multiple of 2^q as well. The sums are taken exactly in 128-bit
// fixed point (any order), and each running value is checked to be exactly
// representable as a double (at most 53 significant bits, and below 2^1024 in
// magnitude: the reference's sum that leaves the double range is an infinity and
// stays one, whatever the exact sum does next); when all are, every
// one of the reference's additions was exact and its results equal these bit
// for bit. Otherwise (or with NaN / infinite addends, or a fixed-point range
// over 96 bits) the pass reports "not exact" and the caller reruns the query on
// an engine that adds sequentially -- for a rule set beyond the general engine's
// query table, the carried sequential pass at the end of this file, which also
// keeps such a set's aggregates between streaming steps.
//
// Pipeline: k_sha_prep (segment id = query * nkeys + key of the trigger event,
// exponent range per column) -> stable radix sort of (segment, row) ->
// k_sha_gather (every aggregate column of a row into sorted order, one row read)
// -> per column: k_sha_tile (segmented inclusive scan of 2,048-row tiles in
// registers + LDS) -> k_sha_carry (one workgroup: segmented scan of the tile
// aggregates) -> k_sha_out (carry-in, exactness check, double conversion)
// -> k_sha_scatter (every column back into its row, one row write). A max / min
// column takes k_shm_tile -> k_shm_carry -> k_shm_out between the same gather and
// scatter. Under `group by` (sha_running_grouped) the segment ids and the sorted order
// come from sh_group.hip instead -- a segment is (query, key, group values) -- and
// everything from k_sha_gather on is the same.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "../../include/sh_query.h"
#include "sh_agg.h"
#include "sh_agg_seq.h"
#include "sh_device.h"
#include "sh_group.h"
#include "sh_wave.h"

#define SHA_TPB 256
#define SHA_ITEMS 8
#define SHA_TILE (SHA_TPB * SHA_ITEMS)
#define SHA_CARRY_TPB 1024

// 128-bit two's complement fixed point
struct sha_i128 {
    uint64_t lo, hi;
};
__device__ __forceinline__ sha_i128 sha_add(sha_i128 a, sha_i128 b) {
    sha_i128 r;
    r.lo = a.lo + b.lo;
    r.hi = a.hi + b.hi + (r.lo < a.lo ? 1ull : 0ull);
    return r;
}
__device__ __forceinline__ sha_i128 sha_zero() { return sha_i128{0ull, 0ull}; }

// the running value with its segment flag (segmented-scan element): flag = a
// segment starts inside the span, value = the sum since its last start
struct sha_el {
    sha_i128 v;
    int64_t c;
    uint32_t f;
};
__device__ __forceinline__ sha_el sha_comb(const sha_el& a, const sha_el& b) {
    sha_el r;
    r.f = a.f | b.f;
    r.v = b.f ? b.v : sha_add(a.v, b.v);
    r.c = b.f ? b.c : a.c + b.c;
    return r;
}

// decomposition of a double: value = m * 2^e with an odd (or zero) m
__device__ __forceinline__ void sha_split(double d, uint64_t* m, int* e, int* neg) {
    const uint64_t bits = (uint64_t)__double_as_longlong(d);
    const int ef = (int)((bits >> 52) & 0x7FF);
    uint64_t mant = bits & ((1ull << 52) - 1ull);
    int ex;
    if (ef == 0) {
        ex = -1074;
    } else {
        mant |= 1ull << 52;
        ex = ef - 1075;
    }
    if (mant) {
        const int tz = __builtin_ctzll(mant);
        mant >>= tz;
        ex += tz;
    }
    *m = mant;
    *e = ex;
    *neg = (int)(bits >> 63);
}

// the double the reference adds for a raw column value (Float/Integer/Long unboxed to double)
__device__ __forceinline__ double sha_as_double(int64_t raw, int type) {
    switch (type) {
        case SH_T_FLOAT: return (double)__uint_as_float((uint32_t)raw);
        case SH_T_DOUBLE: return __longlong_as_double(raw);
        case SH_T_INT: return (double)(int32_t)raw;
        case SH_T_LONG: return (double)raw;
        default: return 0.0;
    }
}

__device__ __forceinline__ bool sha_fp(const sha_col& c) {
    return c.kind == SH_AGG_AVG || (c.kind == SH_AGG_SUM && (c.arg_type == SH_T_FLOAT || c.arg_type == SH_T_DOUBLE));
}

// ---------------------------------------------------------------- prep
__global__ void __launch_bounds__(SHA_TPB) k_sha_prep(const uint64_t* __restrict__ seq, const int64_t* __restrict__ vals,
                                                      int n_out, int64_t m, const int32_t* __restrict__ query,
                                                      const int32_t* __restrict__ keys, int32_t nkeys,
                                                      uint64_t seq_base, sha_desc D, uint32_t* __restrict__ seg,
                                                      uint32_t* __restrict__ idx, int32_t* __restrict__ range) {
    // grid-stride over the rows with the exponent range per column in registers,
    // then one reduction per workgroup: the range words are a handful of
    // addresses, so per-wave atomics would serialise on them
    int lo[SHA_MAX_COLS], hi[SHA_MAX_COLS], bad[SHA_MAX_COLS];
#pragma unroll
    for (int k = 0; k < SHA_MAX_COLS; k++) {
        lo[k] = 1 << 30;
        hi[k] = -(1 << 30);
        bad[k] = 0;
    }
    for (int64_t r = (int64_t)blockIdx.x * SHA_TPB + threadIdx.x; r < m; r += (int64_t)gridDim.x * SHA_TPB) {
        const int64_t key = keys ? keys[seq[r] - seq_base] : 0;
        const int64_t q = query ? query[r] : 0;
        seg[r] = (uint32_t)(q * nkeys + key);
        idx[r] = (uint32_t)r;
#pragma unroll
        for (int k = 0; k < SHA_MAX_COLS; k++) {
            const sha_col c = D.c[k];
            if (k >= D.n_cols || !sha_fp(c)) continue;
            const double d = sha_as_double(vals[r * n_out + c.col], c.arg_type);
            if (!isfinite(d)) {
                bad[k] = 1;
            } else if (d != 0.0) {
                uint64_t mm;
                int e, ng;
                sha_split(d, &mm, &e, &ng);
                lo[k] = min(lo[k], e);
                hi[k] = max(hi[k], e + 63 - __builtin_clzll(mm));
            }
        }
    }
    __shared__ int s_r[SHA_TPB / 64][SHA_MAX_COLS][3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < SHA_MAX_COLS; k++) {
        if (k >= D.n_cols) continue;
        int l = lo[k], h = hi[k], b = bad[k];
        for (int o = 32; o > 0; o >>= 1) {
            l = min(l, __shfl_xor(l, o));
            h = max(h, __shfl_xor(h, o));
            b |= __shfl_xor(b, o);
        }
        if (lane == 0) {
            s_r[wave][k][0] = l;
            s_r[wave][k][1] = h;
            s_r[wave][k][2] = b;
        }
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < D.n_cols && sha_fp(D.c[k])) {
        int l = s_r[0][k][0], h = s_r[0][k][1], b = s_r[0][k][2];
        for (int w = 1; w < SHA_TPB / 64; w++) {
            l = min(l, s_r[w][k][0]);
            h = max(h, s_r[w][k][1]);
            b |= s_r[w][k][2];
        }
        atomicMin(&range[3 * k], l);
        atomicMax(&range[3 * k + 1], h);
        if (b) atomicOr(&range[3 * k + 2], 1);
    }
}

// ---------------------------------------------------------------- scans
// the addend of sorted position p for column c (fixed point at 2^q for doubles), from
// the column's copy in sorted order (sv[p])
__device__ __forceinline__ sha_el sha_load(const int64_t* __restrict__ sv, int64_t p, const sha_col& c, int q) {
    sha_el x;
    x.f = 0;
    x.c = 1;
    x.v = sha_zero();
    const int64_t raw = sv[p];
    if (c.kind == SH_AGG_COUNT) return x;
    if (!sha_fp(c)) {
        // long arithmetic (sum of int / long): the low 64 bits wrap like Java's long
        const int64_t v = c.arg_type == SH_T_INT ? (int64_t)(int32_t)raw : raw;
        x.v.lo = (uint64_t)v;
        x.v.hi = v < 0 ? ~0ull : 0ull;
        return x;
    }
    const double d = sha_as_double(raw, c.arg_type);
    if (d == 0.0) return x;
    uint64_t mm;
    int e, ng;
    sha_split(d, &mm, &e, &ng);
    const int sh = e - q;  // 0 <= sh, sh + bits(mm) <= 96 (checked on the host)
    sha_i128 v;
    if (sh >= 64) {
        v.lo = 0ull;
        v.hi = mm << (sh - 64);
    } else if (sh > 0) {
        v.lo = mm << sh;
        v.hi = mm >> (64 - sh);
    } else {
        v.lo = mm;
        v.hi = 0ull;
    }
    if (ng) {
        v.lo = ~v.lo;
        v.hi = ~v.hi;
        v = sha_add(v, sha_i128{1ull, 0ull});
    }
    x.v = v;
    return x;
}

__device__ __forceinline__ sha_el sha_shfl_up(const sha_el& a, int o) {
    sha_el r;
    r.v.lo = (uint64_t)__shfl_up((long long)a.v.lo, o, 64);
    r.v.hi = (uint64_t)__shfl_up((long long)a.v.hi, o, 64);
    r.c = (int64_t)__shfl_up((long long)a.c, o, 64);
    r.f = (uint32_t)__shfl_up((int)a.f, o, 64);
    return r;
}

// inclusive segmented scan of one element per thread over the workgroup; the
// LDS arrays hold one element per wave
template <int NT>
__device__ __forceinline__ sha_el sha_block_scan(sha_el x, sha_el* wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const sha_el y = sha_shfl_up(x, o);
        if (lane >= o) x = sha_comb(y, x);
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    if (w > 0) {
        sha_el pre = wsum[0];
        for (int i = 1; i < w; i++) pre = sha_comb(pre, wsum[i]);
        x = sha_comb(pre, x);
    }
    __syncthreads();
    return x;
}

// per tile: inclusive segmented scan (sorted order) into out[], the tile's
// aggregate and the tile offset of its first segment start (SHA_TILE: none)
__global__ void __launch_bounds__(SHA_TPB) k_sha_tile(const int64_t* __restrict__ scol,
                                                      const uint32_t* __restrict__ sseg, int64_t m, sha_col c, int q,
                                                      sha_i128* __restrict__ out_v, int64_t* __restrict__ out_c,
                                                      sha_el* __restrict__ tiles, uint32_t* __restrict__ first_head) {
    __shared__ sha_el wsum[SHA_TPB / 64];
    __shared__ uint32_t fh;
    const int64_t t0 = (int64_t)blockIdx.x * SHA_TILE;
    const int64_t p0 = t0 + (int64_t)threadIdx.x * SHA_ITEMS;
    if (threadIdx.x == 0) fh = SHA_TILE;
    __syncthreads();
    sha_el it[SHA_ITEMS];
    sha_el acc;
    acc.f = 0;
    acc.c = 0;
    acc.v = sha_zero();
    uint32_t myfh = SHA_TILE;
#pragma unroll
    for (int j = 0; j < SHA_ITEMS; j++) {
        const int64_t p = p0 + j;
        sha_el x;
        if (p < m) {
            x = sha_load(scol, p, c, q);
            x.f = (p == 0 || sseg[p] != sseg[p - 1]) ? 1u : 0u;
            if (x.f && myfh == SHA_TILE) myfh = (uint32_t)(p - t0);
        } else {
            x.f = 0;
            x.c = 0;
            x.v = sha_zero();
        }
        acc = j == 0 ? x : sha_comb(acc, x);
        it[j] = acc;
    }
    if (myfh != SHA_TILE) atomicMin(&fh, myfh);
    // exclusive prefix of the thread aggregates
    const sha_el inc = sha_block_scan<SHA_TPB>(acc, wsum);
    sha_el pre = sha_shfl_up(inc, 1);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        // the previous wave's last inclusive value
        pre.f = 0;
        pre.c = 0;
        pre.v = sha_zero();
        if (w > 0) {
            pre = wsum[0];
            for (int i = 1; i < w; i++) pre = sha_comb(pre, wsum[i]);
        }
    }
    const bool has_pre = threadIdx.x > 0;
#pragma unroll
    for (int j = 0; j < SHA_ITEMS; j++) {
        const int64_t p = p0 + j;
        if (p >= m) break;
        const sha_el y = has_pre ? sha_comb(pre, it[j]) : it[j];
        out_v[p] = y.v;
        out_c[p] = y.c;
    }
    __syncthreads();
    if (threadIdx.x == SHA_TPB - 1) {
        tiles[blockIdx.x] = inc;
        first_head[blockIdx.x] = fh;
    }
}

// exclusive segmented scan of the tile aggregates (one workgroup)
__global__ void __launch_bounds__(SHA_CARRY_TPB) k_sha_carry(sha_el* __restrict__ tiles, int64_t nt) {
    __shared__ sha_el wsum[SHA_CARRY_TPB / 64];
    const int64_t per = (nt + SHA_CARRY_TPB - 1) / SHA_CARRY_TPB;
    const int64_t b = (int64_t)threadIdx.x * per;
    sha_el acc;
    acc.f = 0;
    acc.c = 0;
    acc.v = sha_zero();
    for (int64_t t = b; t < b + per && t < nt; t++) acc = sha_comb(acc, tiles[t]);
    const sha_el inc = sha_block_scan<SHA_CARRY_TPB>(acc, wsum);
    // exclusive prefix of this thread's run
    sha_el run;
    {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        sha_el up = sha_shfl_up(inc, 1);
        if (lane == 0) {
            up.f = 0;
            up.c = 0;
            up.v = sha_zero();
            if (w > 0) {
                up = wsum[0];
                for (int i = 1; i < w; i++) up = sha_comb(up, wsum[i]);
            }
        }
        run = up;
        if (threadIdx.x == 0) {
            run.f = 0;
            run.c = 0;
            run.v = sha_zero();
        }
    }
    __syncthreads();
    for (int64_t t = b; t < b + per && t < nt; t++) {
        const sha_el x = tiles[t];
        tiles[t] = run;  // exclusive
        run = sha_comb(run, x);
    }
}

// carry-in, exactness, conversion, write into the row
__global__ void __launch_bounds__(SHA_TPB) k_sha_out(int64_t* __restrict__ scol, int64_t m, sha_col c, int q,
                                                     const sha_i128* __restrict__ in_v, const int64_t* __restrict__ in_c,
                                                     const sha_el* __restrict__ tiles,
                                                     const uint32_t* __restrict__ first_head, int32_t* __restrict__ flag) {
    const int64_t p = (int64_t)blockIdx.x * SHA_TPB + threadIdx.x;
    if (p >= m) return;
    const int64_t t = p / SHA_TILE;
    sha_i128 v = in_v[p];
    int64_t cnt = in_c[p];
    if ((uint32_t)(p - t * SHA_TILE) < first_head[t]) {
        // before the tile's first segment start: the running value carries in
        v = sha_add(tiles[t].v, v);
        cnt += tiles[t].c;
    }
    int64_t out;
    if (c.kind == SH_AGG_COUNT) {
        out = cnt;
    } else if (!sha_fp(c)) {
        out = (int64_t)v.lo;
    } else {
        // exactly representable: at most 53 significant bits
        const bool neg = (int64_t)v.hi < 0;
        sha_i128 a = v;
        if (neg) {
            a.lo = ~a.lo;
            a.hi = ~a.hi;
            a = sha_add(a, sha_i128{1ull, 0ull});
        }
        double d = 0.0;
        if (a.lo | a.hi) {
            int tz;
            uint64_t mlo = a.lo, mhi = a.hi;
            if (mlo) {
                tz = __builtin_ctzll(mlo);
                mlo = (mlo >> tz) | (tz ? (mhi << (64 - tz)) : 0ull);
                mhi = tz ? (mhi >> tz) : mhi;
            } else {
                tz = 64 + __builtin_ctzll(mhi);
                mlo = mhi >> (tz - 64);
                mhi = 0ull;
            }
            // ... and below 2^1024: a sum that leaves the double range is an infinity in
            // the reference, and stays one when the exact sum comes back
            if (mhi || mlo >= (1ull << 53) || q + tz + 64 - __builtin_clzll(mlo) > 1024) {
                atomicOr(flag, 1);
                return;
            }
            d = ldexp((double)mlo, q + tz);
            if (neg) d = -d;
        }
        out = c.kind == SH_AGG_AVG ? __double_as_longlong(d / (double)cnt) : __double_as_longlong(d);
    }
    scol[p] = out;
}

// the aggregate columns into sorted order, one row read for all of them (SoA: column k
// at sc + k * m), and back into the rows once every column is done
__global__ void __launch_bounds__(SHA_TPB) k_sha_gather(const int64_t* __restrict__ vals, int n_out,
                                                        const uint32_t* __restrict__ idx, int64_t m, sha_desc D,
                                                        int64_t* __restrict__ sc) {
    const int64_t p = (int64_t)blockIdx.x * SHA_TPB + threadIdx.x;
    if (p >= m) return;
    const int64_t* row = vals + (int64_t)idx[p] * n_out;
    for (int k = 0; k < D.n_cols; k++) sc[(int64_t)k * m + p] = row[D.c[k].col];
}

__global__ void __launch_bounds__(SHA_TPB) k_sha_scatter(int64_t* __restrict__ vals, int n_out,
                                                         const uint32_t* __restrict__ idx, int64_t m, sha_desc D,
                                                         const int64_t* __restrict__ sc) {
    const int64_t p = (int64_t)blockIdx.x * SHA_TPB + threadIdx.x;
    if (p >= m) return;
    int64_t* row = vals + (int64_t)idx[p] * n_out;
    for (int k = 0; k < D.n_cols; k++) row[D.c[k].col] = sc[(int64_t)k * m + p];
}

// ---------------------------------------------------------------- max / min
// max(x) / min(x) over the same sorted columns (sh_agg_seq.h shq_better restates the
// reference). In sequence the rule is not associative over raw floats (a NaN
// argument never replaces, a NaN state is never replaced), so the scan element
// encodes it: a NaN argument is the identity (no value), a NaN at a segment head is
// absorbing (the segment's first argument: every row of the segment is that NaN),
// and of two values that compare equal the left one stays (-0.0 / +0.0). That is
// "the earliest argument attaining the extreme", a segmented scan: one 64-bit
// value (the winning argument's raw bits) plus three flag bits.
#define SHM_HEAD 1u  // a segment starts inside the span
#define SHM_HAS 2u   // the span (since its last start) holds a value
#define SHM_ABS 4u   // ... started with a NaN: v is that NaN, nothing replaces it

struct shm_el {
    uint64_t v;
    uint32_t f;
};

__device__ __forceinline__ shm_el shm_comb(const shm_el& a, const shm_el& b, const sha_col& c) {
    if (b.f & SHM_HEAD) return b;
    shm_el r = a;
    if ((a.f & SHM_ABS) || !(b.f & SHM_HAS)) return r;
    if (!(a.f & SHM_HAS) || shq_better(c.kind, c.arg_type, (int64_t)b.v, (int64_t)a.v)) {
        r.v = b.v;
        r.f = a.f | SHM_HAS;
    }
    return r;
}

template <int CTRL>
__device__ __forceinline__ shm_el shm_move(const shm_el& a) {
    shm_el r;
    r.v = shw_move64<CTRL>(a.v);
    r.f = shw_move<CTRL>(a.f);
    return r;
}

// inclusive scan over the 64 lanes of a wave: the DPP row shifts and row
// broadcasts of sh_wave.h with shm_comb in place of the addition (a lane without a
// source is guarded, as there)
__device__ __forceinline__ shm_el shm_wave_scan(shm_el x, const sha_col& c) {
    const int lane = threadIdx.x & 63, rl = lane & 15;
    shm_el t;
    t = shm_move<SHW_ROW_SHR(1)>(x);
    if (rl >= 1) x = shm_comb(t, x, c);
    t = shm_move<SHW_ROW_SHR(2)>(x);
    if (rl >= 2) x = shm_comb(t, x, c);
    t = shm_move<SHW_ROW_SHR(4)>(x);
    if (rl >= 4) x = shm_comb(t, x, c);
    t = shm_move<SHW_ROW_SHR(8)>(x);
    if (rl >= 8) x = shm_comb(t, x, c);
    t = shm_move<SHW_ROW_BCAST15>(x);
    if ((lane & 31) >= 16) x = shm_comb(t, x, c);
    t = shm_move<SHW_ROW_BCAST31>(x);
    if (lane >= 32) x = shm_comb(t, x, c);
    return x;
}

// workgroup scan of one element per thread: *inc the inclusive value, the return
// value the exclusive one (the identity for thread 0); wsum: one element per wave
template <int NT>
__device__ __forceinline__ shm_el shm_block_scan(const shm_el& x, const sha_col& c, shm_el* wsum, shm_el* inc) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const shm_el wi = shm_wave_scan(x, c);
    if (lane == 63) wsum[w] = wi;
    __syncthreads();
    shm_el pre;  // the waves before this one
    pre.v = 0ull;
    pre.f = 0u;
    for (int i = 0; i < w; i++) pre = shm_comb(pre, wsum[i], c);
    // the lane below's inclusive value (lane 0: none)
    shm_el up;
    up.v = (uint64_t)__shfl_up((long long)wi.v, 1, 64);
    up.f = (uint32_t)__shfl_up((int)wi.f, 1, 64);
    if (lane == 0) {
        up.v = 0ull;
        up.f = 0u;
    }
    __syncthreads();
    *inc = shm_comb(pre, wi, c);
    return shm_comb(pre, up, c);
}

// per tile, in place: the column's arguments become the inclusive segmented scan's
// values (sorted order), has[p] whether the span from the tile's start to p holds
// a value; the tile's aggregate and the offset of its first segment start
__global__ void __launch_bounds__(SHA_TPB) k_shm_tile(int64_t* __restrict__ scol, const uint32_t* __restrict__ sseg,
                                                      int64_t m, sha_col c, uint8_t* __restrict__ has,
                                                      shm_el* __restrict__ tiles, uint32_t* __restrict__ first_head) {
    __shared__ shm_el wsum[SHA_TPB / 64];
    __shared__ uint32_t fh;
    const int64_t t0 = (int64_t)blockIdx.x * SHA_TILE;
    const int64_t p0 = t0 + (int64_t)threadIdx.x * SHA_ITEMS;
    if (threadIdx.x == 0) fh = SHA_TILE;
    __syncthreads();
    shm_el it[SHA_ITEMS];
    shm_el acc;
    acc.v = 0ull;
    acc.f = 0u;
    uint32_t myfh = SHA_TILE;
#pragma unroll
    for (int j = 0; j < SHA_ITEMS; j++) {
        const int64_t p = p0 + j;
        shm_el x;
        x.v = 0ull;
        x.f = 0u;
        if (p < m) {
            x.v = (uint64_t)scol[p];
            const bool head = p == 0 || sseg[p] != sseg[p - 1];
            const bool nan = shq_arg_nan((int64_t)x.v, c.arg_type);
            x.f = (head ? SHM_HEAD : 0u) | (nan ? (head ? SHM_ABS : 0u) : SHM_HAS);
            if (head && myfh == SHA_TILE) myfh = (uint32_t)(p - t0);
        }
        acc = j == 0 ? x : shm_comb(acc, x, c);
        it[j] = acc;
    }
    if (myfh != SHA_TILE) atomicMin(&fh, myfh);
    shm_el inc;
    const shm_el pre = shm_block_scan<SHA_TPB>(acc, c, wsum, &inc);
#pragma unroll
    for (int j = 0; j < SHA_ITEMS; j++) {
        const int64_t p = p0 + j;
        if (p >= m) break;
        const shm_el y = shm_comb(pre, it[j], c);
        scol[p] = (int64_t)y.v;
        has[p] = (uint8_t)(y.f & (SHM_HAS | SHM_ABS));
    }
    __syncthreads();
    if (threadIdx.x == SHA_TPB - 1) {
        tiles[blockIdx.x] = inc;
        first_head[blockIdx.x] = fh;
    }
}

// exclusive segmented scan of the tile aggregates (one workgroup; a thread walks
// its run of ceil(nt / SHA_CARRY_TPB) tiles)
__global__ void __launch_bounds__(SHA_CARRY_TPB) k_shm_carry(shm_el* __restrict__ tiles, int64_t nt, sha_col c) {
    __shared__ shm_el wsum[SHA_CARRY_TPB / 64];
    const int64_t per = (nt + SHA_CARRY_TPB - 1) / SHA_CARRY_TPB;
    const int64_t b = (int64_t)threadIdx.x * per;
    shm_el acc;
    acc.v = 0ull;
    acc.f = 0u;
    for (int64_t t = b; t < b + per && t < nt; t++) acc = shm_comb(acc, tiles[t], c);
    shm_el inc;
    shm_el run = shm_block_scan<SHA_CARRY_TPB>(acc, c, wsum, &inc);
    for (int64_t t = b; t < b + per && t < nt; t++) {
        const shm_el x = tiles[t];
        tiles[t] = run;  // exclusive
        run = shm_comb(run, x, c);
    }
}

// the rows before their tile's first segment start take the carry-in (the others
// are final as k_shm_tile left them)
__global__ void __launch_bounds__(SHA_TPB) k_shm_out(int64_t* __restrict__ scol, int64_t m, sha_col c,
                                                     const uint8_t* __restrict__ has, const shm_el* __restrict__ tiles,
                                                     const uint32_t* __restrict__ first_head) {
    const int64_t p = (int64_t)blockIdx.x * SHA_TPB + threadIdx.x;
    if (p >= m) return;
    const int64_t t = p / SHA_TILE;
    if ((uint32_t)(p - t * SHA_TILE) >= first_head[t]) return;
    shm_el x;
    x.v = (uint64_t)scol[p];
    x.f = has[p];
    scol[p] = (int64_t)shm_comb(tiles[t], x, c).v;
}

// ---------------------------------------------------------------- host
extern "C" int64_t sha_scratch_bytes(int64_t m, int n_cols) {
    const int64_t nt = (m + SHA_TILE - 1) / SHA_TILE;
    const int64_t rt = (m + 4095) / 4096;
    // seg, idx, 2 x 2 sort buffers, 128-bit values, counts, tiles, first heads,
    // sort histogram, scan temporaries, exponent ranges, the sorted column copies
    return m * 4 * 6 + m * 16 + m * 8 + nt * (int64_t)sizeof(sha_el) + nt * 4 + 256 * rt * 4 +
           (int64_t)shd_scan_tmp_words(256 * rt) * 4 + 4096 + (int64_t)(n_cols < 1 ? 1 : n_cols) * m * 8 + 256;
}

static int sha_ok() { return hipGetLastError() == hipSuccess ? 0 : -3; }

// the workspace of one sha_running call (sha_scratch_bytes)
struct sha_ws {
    uint32_t *seg, *idx, *kb0, *kb1, *vb0, *vb1;
    sha_i128* sv;
    int64_t* sc;
    sha_el* tiles;
    uint32_t *fh, *hist, *stmp;
    int32_t* range;
    int64_t* scol;
};

static uint8_t* sha_carve(void* d_scratch, int64_t m, int n_cols, sha_ws* W) {
    const int64_t nt = (m + SHA_TILE - 1) / SHA_TILE;
    const int64_t rt = (m + 4095) / 4096;
    uint8_t* p = (uint8_t*)d_scratch;
    auto take = [&](int64_t bytes) {
        uint8_t* r = p;
        p += (bytes + 255) & ~(int64_t)255;
        return (void*)r;
    };
    W->seg = (uint32_t*)take(m * 4);
    W->idx = (uint32_t*)take(m * 4);
    W->kb0 = (uint32_t*)take(m * 4);
    W->kb1 = (uint32_t*)take(m * 4);
    W->vb0 = (uint32_t*)take(m * 4);
    W->vb1 = (uint32_t*)take(m * 4);
    W->sv = (sha_i128*)take(m * 16);
    W->sc = (int64_t*)take(m * 8);
    W->tiles = (sha_el*)take(nt * (int64_t)sizeof(sha_el));
    W->fh = (uint32_t*)take(nt * 4);
    W->hist = (uint32_t*)take(256 * rt * 4);
    W->stmp = (uint32_t*)take((int64_t)shd_scan_tmp_words(256 * rt) * 4);
    W->range = (int32_t*)take(4 * 3 * SHA_MAX_COLS + 64);
    W->scol = (int64_t*)take((int64_t)n_cols * m * 8);
    return p;
}

// the exponent ranges' start values, then k_sha_prep: segment ids, row indices, ranges
static int sha_prep(const uint64_t* d_seq, const int64_t* d_vals, int32_t n_out, int64_t m, const int32_t* d_query,
                    const int32_t* d_keys, int32_t n_keys, uint64_t seq_base, const sha_desc* D, const sha_ws& W,
                    hipStream_t st) {
    int32_t h_range[3 * SHA_MAX_COLS];
    for (int k = 0; k < SHA_MAX_COLS; k++) {
        h_range[3 * k] = 1 << 30;
        h_range[3 * k + 1] = -(1 << 30);
        h_range[3 * k + 2] = 0;
    }
    hipMemcpyAsync(W.range, h_range, sizeof(h_range), hipMemcpyHostToDevice, st);
    hipMemsetAsync(W.range + 3 * SHA_MAX_COLS, 0, 4, st);
    const unsigned g = (unsigned)((m + SHA_TPB - 1) / SHA_TPB);
    hipLaunchKernelGGL(k_sha_prep, dim3((unsigned)std::min<int64_t>(g, 2048)), dim3(SHA_TPB), 0, st, d_seq, d_vals, n_out, m, d_query,
                       d_keys, n_keys, seq_base, *D, W.seg, W.idx, W.range);
    return sha_ok();
}

// from the sorted segment ids sseg and the sorted order sidx on: gather, the scans per
// column, the exactness verdict, scatter (what a segment is does not matter here)
static int sha_tail(int64_t* d_vals, int32_t n_out, int64_t m, const sha_desc* D, const sha_ws& W,
                    const uint32_t* sseg, const uint32_t* sidx, hipStream_t st) {
    const int64_t nt = (m + SHA_TILE - 1) / SHA_TILE;
    const unsigned g = (unsigned)((m + SHA_TPB - 1) / SHA_TPB);
    sha_i128* sv = W.sv;
    int64_t* sc = W.sc;
    sha_el* tiles = W.tiles;
    uint32_t* fh = W.fh;
    int32_t* range = W.range;
    int64_t* scol = W.scol;
    int32_t h_range[3 * SHA_MAX_COLS];
    hipLaunchKernelGGL(k_sha_gather, dim3(g), dim3(SHA_TPB), 0, st, (const int64_t*)d_vals, n_out, sidx, m, *D, scol);
    hipMemcpyAsync(h_range, range, sizeof(h_range), hipMemcpyDeviceToHost, st);
    if (hipStreamSynchronize(st) != hipSuccess) return -3;
    for (int k = 0; k < D->n_cols; k++) {
        const sha_col c = D->c[k];
        int q = 0;
        const bool fp = c.kind == SH_AGG_AVG || (c.kind == SH_AGG_SUM && (c.arg_type == SH_T_FLOAT || c.arg_type == SH_T_DOUBLE));
        if (fp) {
            if (h_range[3 * k + 2]) return 1;  // NaN / infinite addend
            const int lo = h_range[3 * k], hi = h_range[3 * k + 1];
            if (lo <= hi) {
                if (hi - lo + 1 > 96) return 1;  // fixed-point range
                q = lo;
            }
        }
        int64_t* colk = scol + (int64_t)k * m;
        if (shq_minmax(c.kind)) {
            // never "not exact": the scan is the reference's rule itself (sc: the has bytes)
            hipLaunchKernelGGL(k_shm_tile, dim3((unsigned)nt), dim3(SHA_TPB), 0, st, colk, sseg, m, c, (uint8_t*)sc,
                               (shm_el*)tiles, fh);
            hipLaunchKernelGGL(k_shm_carry, dim3(1), dim3(SHA_CARRY_TPB), 0, st, (shm_el*)tiles, nt, c);
            hipLaunchKernelGGL(k_shm_out, dim3(g), dim3(SHA_TPB), 0, st, colk, m, c, (const uint8_t*)sc,
                               (const shm_el*)tiles, (const uint32_t*)fh);
            if (sha_ok()) return -3;
            continue;
        }
        hipLaunchKernelGGL(k_sha_tile, dim3((unsigned)nt), dim3(SHA_TPB), 0, st, (const int64_t*)colk, sseg, m, c, q,
                           sv, sc, tiles, fh);
        hipLaunchKernelGGL(k_sha_carry, dim3(1), dim3(SHA_CARRY_TPB), 0, st, tiles, nt);
        hipLaunchKernelGGL(k_sha_out, dim3(g), dim3(SHA_TPB), 0, st, colk, m, c, q, (const sha_i128*)sv,
                           (const int64_t*)sc, (const sha_el*)tiles, (const uint32_t*)fh, range + 3 * SHA_MAX_COLS);
        if (sha_ok()) return -3;
    }
    // the rows are written only once every addition is known to be exact: a "not
    // exact" answer leaves the aggregators' arguments in place for the sequential
    // pass (shc_running)
    int32_t inexact = 0;
    hipMemcpyAsync(&inexact, range + 3 * SHA_MAX_COLS, 4, hipMemcpyDeviceToHost, st);
    if (hipStreamSynchronize(st) != hipSuccess) return -3;
    if (inexact) return 1;
    hipLaunchKernelGGL(k_sha_scatter, dim3(g), dim3(SHA_TPB), 0, st, d_vals, n_out, sidx, m, *D,
                       (const int64_t*)scol);
    if (sha_ok()) return -3;
    return 0;
}

extern "C" int sha_running(const uint64_t* d_seq, int64_t* d_vals, int32_t n_out, int64_t m, const int32_t* d_query,
                           int32_t n_query, const int32_t* d_keys, int32_t n_keys, uint64_t seq_base,
                           const sha_desc* D, void* d_scratch, void* stream) {
    if (m <= 0 || D->n_cols == 0) return 0;
    if (m >= ((int64_t)1 << 32) || n_out < 1 || !d_seq || !d_vals || !d_scratch) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nseg = (int64_t)(n_query < 1 ? 1 : n_query) * (n_keys < 1 ? 1 : n_keys);
    if (nseg > ((int64_t)1 << 32)) return -1;
    sha_ws W;
    sha_carve(d_scratch, m, D->n_cols, &W);
    if (sha_prep(d_seq, (const int64_t*)d_vals, n_out, m, d_query, d_keys, n_keys, seq_base, D, W, st)) return -3;
    int bits = 0;
    while (bits < 32 && ((int64_t)1 << bits) < nseg) bits++;
    const uint32_t* sseg = W.seg;
    const uint32_t* sidx = W.idx;
    uint32_t* kbuf[2] = {W.kb0, W.kb1};
    uint32_t* vbuf[2] = {W.vb0, W.vb1};
    if (bits > 0 && shd_sort_pairs(W.seg, W.idx, m, bits, kbuf, vbuf, W.hist, W.stmp, stream, &sseg, &sidx)) return -3;
    return sha_tail(d_vals, n_out, m, D, W, sseg, sidx, st);
}

// `group by` (sh_group.h): the same pass over the segments (query, key, group values).
// The workspace is sha_running's followed by the segment pass's.
extern "C" int64_t sha_grouped_scratch_bytes(int64_t m, int n_cols) {
    return ((sha_scratch_bytes(m, n_cols) + 255) & ~(int64_t)255) + shg_scratch_bytes(m);
}

extern "C" int sha_running_grouped(const uint64_t* d_seq, int64_t* d_vals, int32_t n_out, int64_t m,
                                   const int32_t* d_query, int32_t n_query, const int32_t* d_keys, int32_t n_keys,
                                   uint64_t seq_base, const sha_desc* D, const sha_groups* G, void* d_scratch,
                                   void* stream) {
    if (m <= 0 || D->n_cols == 0) return 0;
    if (m >= ((int64_t)1 << 32) || n_out < 1 || !d_seq || !d_vals || !d_scratch || !shg_valid(G, n_out)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nseg = (int64_t)(n_query < 1 ? 1 : n_query) * (n_keys < 1 ? 1 : n_keys);
    if (nseg > ((int64_t)1 << 32)) return -1;
    sha_ws W;
    sha_carve(d_scratch, m, D->n_cols, &W);
    uint8_t* gws = (uint8_t*)d_scratch + ((sha_scratch_bytes(m, D->n_cols) + 255) & ~(int64_t)255);
    // (k_sha_prep for the exponent ranges; its segment ids are the ungrouped ones and unused)
    if (sha_prep(d_seq, (const int64_t*)d_vals, n_out, m, d_query, d_keys, n_keys, seq_base, D, W, st)) return -3;
    const uint32_t* sseg = nullptr;
    const uint32_t* sidx = nullptr;
    const int rc = shg_segments(d_seq, (const int64_t*)d_vals, n_out, m, d_query, n_query, d_keys, n_keys, seq_base, G,
                                gws, stream, &sseg, &sidx);
    if (rc) return rc;
    return sha_tail(d_vals, n_out, m, D, W, sseg, sidx, st);
}

// ---------------------------------------------------------------- carried, sequential pass
// The same rows with no exactness proof: the reference's additions one at a time
// (sh_agg_seq.h), one lane per (query, key) segment, starting from the segment's
// carried state. Behind streaming rule sets (rules_step: the state of every
// (query, key) that ever produced a row lives in an open-addressing table in HBM)
// and behind sh_run_device when the parallel pass above answers "not exact" (no
// table: every segment starts from zero).
//
// Pipeline: k_shc_prep (key and query of every row) -> stable radix sort by key,
// then by query (LSD: the rows of a segment keep their output order, which is the
// addition order) -> k_shc_gather (aggregate columns and 64-bit segment keys into
// sorted order) -> k_shc_walk (segment heads: look the carried state up, walk the
// run, running values into the columns, final state and segment key aside) ->
// k_sha_scatter. The table is not written here: shc_put (k_shc_put) inserts the
// heads' final states, and the caller launches it last, when nothing can refuse
// the step any more. A segment has one head, so no two lanes write one entry; a
// slot is claimed with a 64-bit compare-and-swap on its key.
__global__ void __launch_bounds__(SHA_TPB) k_shc_prep(const uint64_t* __restrict__ seq, int64_t m,
                                                      const int32_t* __restrict__ query,
                                                      const int32_t* __restrict__ rowkey,
                                                      const int32_t* __restrict__ keys, uint64_t seq_base,
                                                      uint32_t* __restrict__ klo, uint32_t* __restrict__ khi,
                                                      uint32_t* __restrict__ idx) {
    const int64_t r = (int64_t)blockIdx.x * SHA_TPB + threadIdx.x;
    if (r >= m) return;
    klo[r] = rowkey ? (uint32_t)rowkey[r] : keys ? (uint32_t)keys[seq[r] - seq_base] : 0u;
    khi[r] = query ? (uint32_t)query[r] : 0u;
    idx[r] = (uint32_t)r;
}

// (order and gv may be one array: a lane reads its entry before it writes it)
__global__ void __launch_bounds__(SHA_TPB) k_shc_pick(const uint32_t* __restrict__ key, const uint32_t* order,
                                                      int64_t m, uint32_t* __restrict__ gk, uint32_t* gv) {
    const int64_t p = (int64_t)blockIdx.x * SHA_TPB + threadIdx.x;
    if (p >= m) return;
    const uint32_t r = order[p];
    gk[p] = key[r];
    gv[p] = r;
}

__global__ void __launch_bounds__(SHA_TPB) k_shc_gather(const int64_t* __restrict__ vals, int n_out,
                                                        const uint32_t* __restrict__ idx, int64_t m, sha_desc D,
                                                        const uint32_t* __restrict__ klo,
                                                        const uint32_t* __restrict__ khi, int64_t* __restrict__ sc,
                                                        uint64_t* __restrict__ sseg) {
    const int64_t p = (int64_t)blockIdx.x * SHA_TPB + threadIdx.x;
    if (p >= m) return;
    const uint32_t r = idx[p];
    const int64_t* row = vals + (int64_t)r * n_out;
    for (int k = 0; k < D.n_cols; k++) sc[(int64_t)k * m + p] = row[D.c[k].col];
    sseg[p] = shq_key((int32_t)khi[r], (int32_t)klo[r]);
}

// pk[p]: the segment key at a head, SHQ_EMPTY elsewhere; fin: the heads' final states
__global__ void __launch_bounds__(SHA_TPB) k_shc_walk(int64_t* __restrict__ sc, const uint64_t* __restrict__ sseg,
                                                      int64_t m, sha_desc D, shq_table T, uint64_t* __restrict__ pk,
                                                      int64_t* __restrict__ fin) {
    const int64_t p = (int64_t)blockIdx.x * SHA_TPB + threadIdx.x;
    if (p >= m) return;
    const uint64_t sg = sseg[p];
    if (p > 0 && sseg[p - 1] == sg) {
        pk[p] = SHQ_EMPTY;
        return;
    }
    pk[p] = sg;
    int64_t e = p + 1;
    while (e < m && sseg[e] == sg) e++;
    const int64_t slot = shq_find(T, sg);
    // column by column: the running state stays in registers
    for (int k = 0; k < D.n_cols; k++)
        shq_walk(sc + (int64_t)k * m, p, e, D.c[k], T, slot, k, fin + (p * D.n_cols + k) * 2);
}

// entries (pk[i] != SHQ_EMPTY) with their states into the table; *entries counts
// the slots claimed, *err |= 1 when a probe found no slot (the caller keeps the
// table at most half full, so that is a bug, not a state)
__global__ void __launch_bounds__(SHA_TPB) k_shc_put(shq_table T, const uint64_t* __restrict__ pk,
                                                     const int64_t* __restrict__ fin, int64_t n,
                                                     unsigned long long* __restrict__ entries,
                                                     int32_t* __restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * SHA_TPB + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = pk[i];
    if (key == SHQ_EMPTY) return;
    const uint64_t mask = (uint64_t)T.cap - 1ull;
    uint64_t s = shq_hash(key) & mask;
    int64_t slot = -1;
    for (int64_t t = 0; t < T.cap; t++) {
        const unsigned long long was =
            atomicCAS((unsigned long long*)&T.keys[s], (unsigned long long)SHQ_EMPTY, (unsigned long long)key);
        if (was == (unsigned long long)SHQ_EMPTY) {
            atomicAdd(entries, 1ull);
            slot = (int64_t)s;
            break;
        }
        if (was == (unsigned long long)key) {
            slot = (int64_t)s;
            break;
        }
        s = (s + 1ull) & mask;
    }
    if (slot < 0) {
        atomicOr(err, 1);
        return;
    }
    for (int k = 0; k < T.n_cols * 2; k++) T.state[slot * T.n_cols * 2 + k] = fin[i * T.n_cols * 2 + k];
}

extern "C" int64_t shc_scratch_bytes(int64_t m, int n_cols) {
    const int64_t rt = (m + 4095) / 4096;
    const int64_t nc = n_cols < 1 ? 1 : n_cols;
    // key, query, idx, picked keys, 2 x 2 sort buffers; sort histogram and scan
    // temporaries; the sorted column copies; segment keys, head keys, final states
    return m * 4 * 8 + 256 * rt * 4 + (int64_t)shd_scan_tmp_words(256 * rt) * 4 + nc * m * 8 + m * 8 * 2 +
           nc * m * 16 + 256 * 16;
}

extern "C" int shc_running(const uint64_t* d_seq, int64_t* d_vals, int32_t n_out, int64_t m, const int32_t* d_query,
                           int32_t n_query, const int32_t* d_rowkey, const int32_t* d_keys, int32_t n_keys,
                           uint64_t seq_base, const sha_desc* D, const shq_table* T, void* d_scratch, void* stream,
                           const uint64_t** put_keys, const int64_t** put_state) {
    if (put_keys) *put_keys = nullptr;
    if (put_state) *put_state = nullptr;
    if (m <= 0 || D->n_cols == 0) return 0;
    if (m >= ((int64_t)1 << 31) || n_out < 1 || !d_vals || !d_scratch || (!d_rowkey && d_keys && !d_seq)) return -1;
    if (T && T->cap > 0 && ((T->cap & (T->cap - 1)) || T->n_cols != D->n_cols || !T->keys || !T->state)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int64_t rt = (m + 4095) / 4096;
    uint8_t* p = (uint8_t*)d_scratch;
    auto take = [&](int64_t bytes) {
        uint8_t* r = p;
        p += (bytes + 255) & ~(int64_t)255;
        return (void*)r;
    };
    uint32_t* klo = (uint32_t*)take(m * 4);
    uint32_t* khi = (uint32_t*)take(m * 4);
    uint32_t* idx = (uint32_t*)take(m * 4);
    uint32_t* gk = (uint32_t*)take(m * 4);
    uint32_t* kbuf[2] = {(uint32_t*)take(m * 4), (uint32_t*)take(m * 4)};
    uint32_t* vbuf[2] = {(uint32_t*)take(m * 4), (uint32_t*)take(m * 4)};
    uint32_t* hist = (uint32_t*)take(256 * rt * 4);
    uint32_t* stmp = (uint32_t*)take((int64_t)shd_scan_tmp_words(256 * rt) * 4);
    int64_t* scol = (int64_t*)take((int64_t)D->n_cols * m * 8);
    uint64_t* sseg = (uint64_t*)take(m * 8);
    uint64_t* pk = (uint64_t*)take(m * 8);
    int64_t* fin = (int64_t*)take((int64_t)D->n_cols * m * 16);
    const unsigned g = (unsigned)((m + SHA_TPB - 1) / SHA_TPB);
    hipLaunchKernelGGL(k_shc_prep, dim3(g), dim3(SHA_TPB), 0, st, d_seq, m, d_query, d_rowkey, d_keys, seq_base, klo,
                       khi, idx);
    if (sha_ok()) return -3;
    int kbits = 0, qbits = 0;
    while (kbits < 32 && ((int64_t)1 << kbits) < (int64_t)(n_keys < 1 ? 1 : n_keys)) kbits++;
    while (qbits < 32 && ((int64_t)1 << qbits) < (int64_t)(n_query < 1 ? 1 : n_query)) qbits++;
    if (!d_rowkey && !d_keys) kbits = 0;
    if (!d_query) qbits = 0;
    const uint32_t* sidx = idx;
    if (kbits > 0) {
        const uint32_t* ko = nullptr;
        if (shd_sort_pairs(klo, idx, m, kbits, kbuf, vbuf, hist, stmp, stream, &ko, &sidx)) return -3;
    }
    if (qbits > 0) {
        // (idx is free once the first stage has read it, and is the order itself when
        // that stage did not run)
        uint32_t* gv = idx;
        hipLaunchKernelGGL(k_shc_pick, dim3(g), dim3(SHA_TPB), 0, st, (const uint32_t*)khi, sidx, m, gk, gv);
        if (sha_ok()) return -3;
        const uint32_t* ko = nullptr;
        if (shd_sort_pairs(gk, gv, m, qbits, kbuf, vbuf, hist, stmp, stream, &ko, &sidx)) return -3;
    }
    shq_table none;
    memset(&none, 0, sizeof(none));
    hipLaunchKernelGGL(k_shc_gather, dim3(g), dim3(SHA_TPB), 0, st, (const int64_t*)d_vals, n_out, sidx, m, *D,
                       (const uint32_t*)klo, (const uint32_t*)khi, scol, sseg);
    hipLaunchKernelGGL(k_shc_walk, dim3(g), dim3(SHA_TPB), 0, st, scol, (const uint64_t*)sseg, m, *D,
                       T && T->cap > 0 ? *T : none, pk, fin);
    hipLaunchKernelGGL(k_sha_scatter, dim3(g), dim3(SHA_TPB), 0, st, d_vals, n_out, sidx, m, *D,
                       (const int64_t*)scol);
    if (sha_ok()) return -3;
    if (put_keys) *put_keys = pk;
    if (put_state) *put_state = fin;
    return 0;
}

extern "C" int shc_put(const shq_table* T, const uint64_t* pk, const int64_t* fin, int64_t n,
                       unsigned long long* d_entries, int32_t* d_err, void* stream) {
    if (n <= 0) return 0;
    if (!T || T->cap <= 0 || (T->cap & (T->cap - 1)) || !T->keys || !T->state || !pk || !fin || !d_entries || !d_err)
        return -1;
    hipLaunchKernelGGL(k_shc_put, dim3((unsigned)((n + SHA_TPB - 1) / SHA_TPB)), dim3(SHA_TPB), 0,
                       (hipStream_t)stream, *T, pk, fin, n, d_entries, d_err);
    return sha_ok();
}
