// sh_rate.hip — `output first|last|all every N events` behind the fast engines: the
// rules of sh_rate.h applied to the ordered raw rows an engine produced (after
// `having`), as a segmented rank followed by a stable compaction.
//
//   k_shl_prep    one lane per row: the row's index and its sort key, query << kbits |
//                 partition key in one 32-bit word when the key bits and the query bits
//                 in use fit one
//   (sort)        one stable LSD radix sort of (sort key, index) over the bits in use
//                 (shd_sort_pairs): the rows of a (query, key) run become contiguous and
//                 keep their output order, and the sorted words are the run keys
//   (wide keys)   more than 32 bits in use: key and query apart, a sort by key, then by
//                 query (k_shl_pick between them) and k_shl_gather, the 64-bit run key
//                 query << 32 | key in sorted order
//   k_shl_tile    tiles of SHL_TILE rows, 8 per lane in registers: a run's head (its
//                 key differs from its predecessor's) looks its carried counter up and
//                 forms head_position << 32 | counter, every other row 0; an inclusive
//                 max-scan (DPP row shifts and broadcasts, one LDS word per wave)
//                 gives every row the pair of the latest head inside the tile
//   k_shl_carry   one workgroup: exclusive max-scan of the tiles' aggregates
//   k_shl_out     ordinal = position - head + 1, shl_keep on it: one keep byte per row,
//                 in row order; a run's last row writes (run key, next counter) for
//                 shc_put (when the caller carries counters)
//   k_shl_mark    64-bit ballots of the keep bytes and one kept count per tile of
//                 SHV_TILE rows, then shv_move_marked (sh_having.hip): scan and move
//
// A set with an `output all every N events` rule (shl_holds) places rows instead
// (shl_place, sh_rate.h): the same prep, sort, tile and carry, then
//   k_shl_rel     in place of k_shl_out: per row, in row order, its release row (the
//                 row index `ahead` places on in its run, SHL_NO_ROW when it stays
//                 held or is dropped), its offset among the rows released there, and
//                 its own weight, the number of rows it releases
//   (scan)        shd_exclusive_scan of the weights in row order: where every row's
//                 released rows start in the output
//   k_shl_src     one lane per row: src_of[start of its release row + offset] = row (the
//                 only scattered store), and the last row's start + weight to *d_kept
//   k_shl_move    one workgroup per tile of SHV_TILE output rows, as k_shv_move with
//                 the tile's sources read from src_of: a lane per row for the 4- and
//                 8-byte columns, lanes across the rows' words for values and null
//                 flags, so every store is coalesced and the gathers read whole rows
//
// The pair of a head at position 0 with counter 0 is the scan's identity, which is
// what a row before any head of its tile has until the carry reaches it.
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "sh_agg_seq.h"
#include "sh_device.h"
#include "sh_having.h"
#include "sh_rate.h"
#include "sh_wave.h"

#define SHL_TPB 256
#define SHL_ITEMS 8
#define SHL_CARRY_TPB 1024
static_assert(SHL_TPB * SHL_ITEMS == SHL_TILE, "tile = lanes x rows per lane");

__device__ __forceinline__ uint64_t shl_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

// inclusive max-scan over the 64 lanes of a wave (sh_wave.h's scan with max in place
// of the addition; a lane without a source reads 0, the identity)
__device__ __forceinline__ uint64_t shl_wave_scan(uint64_t v) {
    const int lane = threadIdx.x & 63, rl = lane & 15;
    uint64_t t;
    t = shw_move64<SHW_ROW_SHR(1)>(v);
    if (rl >= 1) v = shl_max(v, t);
    t = shw_move64<SHW_ROW_SHR(2)>(v);
    if (rl >= 2) v = shl_max(v, t);
    t = shw_move64<SHW_ROW_SHR(4)>(v);
    if (rl >= 4) v = shl_max(v, t);
    t = shw_move64<SHW_ROW_SHR(8)>(v);
    if (rl >= 8) v = shl_max(v, t);
    t = shw_move64<SHW_ROW_BCAST15>(v);
    if ((lane & 31) >= 16) v = shl_max(v, t);
    t = shw_move64<SHW_ROW_BCAST31>(v);
    if (lane >= 32) v = shl_max(v, t);
    return v;
}

// workgroup max-scan of one value per thread: *inc the inclusive value, the return
// value the exclusive one (0 for thread 0); wsum: one word per wave
template <int NT>
__device__ __forceinline__ uint64_t shl_block_scan(uint64_t x, uint64_t* wsum, uint64_t* inc) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t wi = shl_wave_scan(x);
    if (lane == 63) wsum[w] = wi;
    __syncthreads();
    uint64_t pre = 0;
    for (int i = 0; i < w; i++) pre = shl_max(pre, wsum[i]);
    uint64_t up = (uint64_t)__shfl_up((long long)wi, 1, 64);
    if (lane == 0) up = 0;
    __syncthreads();
    *inc = shl_max(pre, wi);
    return shl_max(pre, up);
}

__global__ void __launch_bounds__(SHL_TPB) k_shl_prep(const uint64_t* __restrict__ seq, int64_t m,
                                                      const int32_t* __restrict__ query,
                                                      const int32_t* __restrict__ rowkey,
                                                      const int32_t* __restrict__ keys, uint64_t seq_base,
                                                      int kbits, uint32_t* __restrict__ klo,
                                                      uint32_t* __restrict__ khi, uint32_t* __restrict__ idx) {
    const int64_t r = (int64_t)blockIdx.x * SHL_TPB + threadIdx.x;
    if (r >= m) return;
    const uint32_t k = rowkey ? (uint32_t)rowkey[r] : keys ? (uint32_t)keys[seq[r] - seq_base] : 0u;
    const uint32_t q = query ? (uint32_t)query[r] : 0u;
    idx[r] = (uint32_t)r;
    if (khi) {  // wide keys: apart
        klo[r] = k;
        khi[r] = q;
    } else {
        klo[r] = (q << kbits) | (k & ((1u << kbits) - 1u));
    }
}

// the run key query << 32 | key of sorted position p: from the 64-bit keys (wide), else
// from the sorted 32-bit word query << kbits | key (kbits < 32)
__device__ __forceinline__ uint64_t shl_run_key(const uint32_t* __restrict__ s32, const uint64_t* __restrict__ s64,
                                                int kbits, int64_t p) {
    if (s64) return s64[p];
    const uint32_t c = s32[p];
    return shq_key((int32_t)(c >> kbits), (int32_t)(c & ((1u << kbits) - 1u)));
}

// (order and gv may be one array: a lane reads its entry before it writes it)
__global__ void __launch_bounds__(SHL_TPB) k_shl_pick(const uint32_t* __restrict__ key, const uint32_t* order,
                                                      int64_t m, uint32_t* __restrict__ gk, uint32_t* gv) {
    const int64_t p = (int64_t)blockIdx.x * SHL_TPB + threadIdx.x;
    if (p >= m) return;
    const uint32_t r = order[p];
    gk[p] = key[r];
    gv[p] = r;
}

__global__ void __launch_bounds__(SHL_TPB) k_shl_gather(const uint32_t* __restrict__ idx, int64_t m,
                                                        const uint32_t* __restrict__ klo,
                                                        const uint32_t* __restrict__ khi, uint64_t* __restrict__ sseg) {
    const int64_t p = (int64_t)blockIdx.x * SHL_TPB + threadIdx.x;
    if (p >= m) return;
    const uint32_t r = idx[p];
    sseg[p] = shq_key((int32_t)khi[r], (int32_t)klo[r]);
}

__global__ void __launch_bounds__(SHL_TPB) k_shl_tile(const uint32_t* __restrict__ s32,
                                                      const uint64_t* __restrict__ s64, int kbits, int64_t m,
                                                      shq_table T, uint64_t* __restrict__ loc,
                                                      uint64_t* __restrict__ tiles) {
    __shared__ uint64_t wsum[SHL_TPB / 64];
    const int64_t p0 = (int64_t)blockIdx.x * SHL_TILE + (int64_t)threadIdx.x * SHL_ITEMS;
    uint64_t it[SHL_ITEMS];
    uint64_t acc = 0;
    uint64_t prev = (p0 > 0 && p0 <= m) ? shl_run_key(s32, s64, kbits, p0 - 1) : 0ull;
#pragma unroll
    for (int j = 0; j < SHL_ITEMS; j++) {
        const int64_t p = p0 + j;
        uint64_t x = 0;
        if (p < m) {
            const uint64_t sg = shl_run_key(s32, s64, kbits, p);
            if (p == 0 || sg != prev) {
                const int64_t slot = shq_find(T, sg);
                const uint32_t c0 = slot >= 0 ? (uint32_t)T.state[slot * 2] : 0u;
                x = ((uint64_t)p << 32) | c0;
            }
            prev = sg;
        }
        acc = shl_max(acc, x);
        it[j] = acc;
    }
    uint64_t inc;
    const uint64_t pre = shl_block_scan<SHL_TPB>(acc, wsum, &inc);
#pragma unroll
    for (int j = 0; j < SHL_ITEMS; j++) {
        const int64_t p = p0 + j;
        if (p < m) loc[p] = shl_max(pre, it[j]);
    }
    if (threadIdx.x == SHL_TPB - 1) tiles[blockIdx.x] = inc;
}

// exclusive max-scan of the tile aggregates, in place (one workgroup; a thread walks
// its run of ceil(nt / SHL_CARRY_TPB) tiles)
__global__ void __launch_bounds__(SHL_CARRY_TPB) k_shl_carry(uint64_t* __restrict__ tiles, int64_t nt) {
    __shared__ uint64_t wsum[SHL_CARRY_TPB / 64];
    const int64_t per = (nt + SHL_CARRY_TPB - 1) / SHL_CARRY_TPB;
    const int64_t b = (int64_t)threadIdx.x * per;
    uint64_t acc = 0;
    for (int64_t t = b; t < b + per && t < nt; t++) acc = shl_max(acc, tiles[t]);
    uint64_t inc;
    uint64_t run = shl_block_scan<SHL_CARRY_TPB>(acc, wsum, &inc);
    for (int64_t t = b; t < b + per && t < nt; t++) {
        const uint64_t x = tiles[t];
        tiles[t] = run;
        run = shl_max(run, x);
    }
}

// pk[p]: the run key at the last row of a limited query's run, SHQ_EMPTY elsewhere;
// fin[2p]: that run's next counter (pk NULL: the caller carries nothing)
__global__ void __launch_bounds__(SHL_TPB) k_shl_out(const uint32_t* __restrict__ s32,
                                                     const uint64_t* __restrict__ s64, int kbits,
                                                     const uint32_t* __restrict__ idx, int64_t m,
                                                     const shl_rule* __restrict__ rules, int32_t n_rules,
                                                     const uint64_t* __restrict__ loc,
                                                     const uint64_t* __restrict__ tiles, uint8_t* __restrict__ keepb,
                                                     uint64_t* __restrict__ pk, int64_t* __restrict__ fin) {
    const int64_t p = (int64_t)blockIdx.x * SHL_TPB + threadIdx.x;
    if (p >= m) return;
    const uint64_t sg = shl_run_key(s32, s64, kbits, p);
    const uint64_t v = shl_max(loc[p], tiles[p / SHL_TILE]);
    const uint32_t c0 = (uint32_t)v;
    const uint64_t j = (uint64_t)(p - (int64_t)(v >> 32)) + 1ull;
    const int32_t q = (int32_t)(sg >> 32);
    shl_rule R;
    R.kind = SH_RATE_NONE;
    R.n = 0;
    if (q >= 0 && q < n_rules) R = rules[q];
    keepb[idx[p]] = shl_keep(R, c0, j) ? 1 : 0;
    if (!pk) return;
    const bool tail = (p == m - 1 || shl_run_key(s32, s64, kbits, p + 1) != sg) && shl_limits(R);
    pk[p] = tail ? sg : SHQ_EMPTY;
    if (tail) {
        fin[2 * p] = (int64_t)shl_next(R, c0, j);
        fin[2 * p + 1] = 0;
    }
}

#define SHL_NO_ROW 0xFFFFFFFFu

// rel[r] / choff[r] / wgt[r] of row r = idx[p]: shl_place on its ordinal (every run
// starts from zero); a row `ahead` of its release row leaves only if that position is
// still in its run
__global__ void __launch_bounds__(SHL_TPB) k_shl_rel(const uint32_t* __restrict__ s32,
                                                     const uint64_t* __restrict__ s64, int kbits,
                                                     const uint32_t* __restrict__ idx, int64_t m,
                                                     const shl_rule* __restrict__ rules, int32_t n_rules,
                                                     const uint64_t* __restrict__ loc,
                                                     const uint64_t* __restrict__ tiles, uint32_t* __restrict__ rel,
                                                     uint32_t* __restrict__ choff, uint32_t* __restrict__ wgt) {
    const int64_t p = (int64_t)blockIdx.x * SHL_TPB + threadIdx.x;
    if (p >= m) return;
    const uint64_t sg = shl_run_key(s32, s64, kbits, p);
    const uint64_t v = shl_max(loc[p], tiles[p / SHL_TILE]);
    const uint64_t j = (uint64_t)(p - (int64_t)(v >> 32)) + 1ull;
    const int32_t q = (int32_t)(sg >> 32);
    shl_rule R;
    R.kind = SH_RATE_NONE;
    R.n = 0;
    if (q >= 0 && q < n_rules) R = rules[q];
    const shl_spot S = shl_place(R, j);
    const int64_t pr = p + (int64_t)S.ahead;
    const bool leaves = S.leaves && pr < m && (S.ahead == 0 || shl_run_key(s32, s64, kbits, pr) == sg);
    const uint32_t r = idx[p];
    rel[r] = leaves ? idx[pr] : SHL_NO_ROW;
    choff[r] = S.offset;
    wgt[r] = S.weight;
}

// woff: the exclusive scan of wgt. The places are distinct and below the total, which
// is at most m: the N rows of a chunk share a release row of weight N and differ in
// their offsets (the bound checks only keep a fault in that reasoning inside the arrays)
__global__ void __launch_bounds__(SHL_TPB) k_shl_src(const uint32_t* __restrict__ rel,
                                                     const uint32_t* __restrict__ choff,
                                                     const uint32_t* __restrict__ wgt,
                                                     const uint32_t* __restrict__ woff, int64_t m,
                                                     uint32_t* __restrict__ src_of,
                                                     unsigned long long* __restrict__ d_kept) {
    const int64_t r = (int64_t)blockIdx.x * SHL_TPB + threadIdx.x;
    if (r >= m) return;
    if (r == m - 1) {
        const uint64_t total = (uint64_t)woff[r] + wgt[r];
        *d_kept = total <= (uint64_t)m ? total : 0ull;
    }
    const uint32_t to = rel[r];
    if (to == SHL_NO_ROW || (int64_t)to >= m) return;
    const uint64_t d = (uint64_t)woff[to] + choff[r];
    if (d < (uint64_t)m) src_of[d] = (uint32_t)r;
}

// output rows [tile * SHV_TILE, ...) from their sources src_of[d] (the two row sets never
// overlap)
__global__ void __launch_bounds__(SHV_TILE) k_shl_move(int32_t n_out, int64_t m, shw_rows in, shw_rows_out out,
                                                       const uint32_t* __restrict__ src_of,
                                                       const unsigned long long* __restrict__ d_kept) {
    __shared__ uint32_t src[SHV_TILE];
    const int64_t total = (int64_t)*d_kept;
    const int64_t base = (int64_t)blockIdx.x * SHV_TILE;
    if (base >= total) return;
    const uint32_t rows = (uint32_t)(total - base < SHV_TILE ? total - base : SHV_TILE);
    {
        uint32_t s = threadIdx.x < rows ? src_of[base + threadIdx.x] : 0u;
        if ((int64_t)s >= m) s = 0u;
        src[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x < rows) {
        const int64_t s = src[threadIdx.x], d = base + threadIdx.x;
        if (out.seq) out.seq[d] = in.seq[s];
        if (out.query) out.query[d] = in.query[s];
        if (out.ts) out.ts[d] = in.ts[s];
        if (out.key) out.key[d] = in.key[s];
    }
    const uint32_t words = rows * (uint32_t)n_out;
    for (uint32_t w = threadIdx.x; w < words; w += SHV_TILE) {
        const uint32_t j = w / (uint32_t)n_out, c = w - j * (uint32_t)n_out;
        const int64_t s = (int64_t)src[j] * n_out + c, d = (base + j) * n_out + c;
        out.vals[d] = in.vals[s];
        if (out.nulls) out.nulls[d] = in.nulls[s];
    }
}

// the keep bytes (row order) as ballot words and kept counts per tile of SHV_TILE rows
__global__ void __launch_bounds__(SHV_TILE) k_shl_mark(const uint8_t* __restrict__ keepb, int64_t m,
                                                       uint64_t* __restrict__ mask, uint32_t* __restrict__ cnt) {
    __shared__ uint32_t wc[SHV_TILE / 64];
    const int64_t r = (int64_t)blockIdx.x * SHV_TILE + threadIdx.x;
    const bool keep = r < m && keepb[r] != 0;
    const uint64_t b = __ballot(keep);
    if ((threadIdx.x & 63) == 0) {
        mask[r >> 6] = b;  // (the mask holds whole tiles: SHV_TILE / 64 words each)
        wc[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < SHV_TILE / 64; w++) s += wc[w];
        cnt[blockIdx.x] = s;
    }
}

// ---------------------------------------------------------------- host
namespace {
struct shl_ws {
    uint32_t *klo, *khi, *idx, *gk, *kbuf[2], *vbuf[2], *hist, *stmp, *cnt, *off, *tmp;
    uint32_t *rel, *choff, *wgt, *woff, *src_of, *ptmp;  // the placement: in pk's and fin's room, and its scan's own
    uint64_t *sseg, *loc, *pk, *tiles, *mask;
    int64_t* fin;
    uint8_t* keepb;
    int64_t bytes;
};

// the workspace's parts from `base` (NULL: sizes only), each 256-byte aligned
shl_ws shl_layout(int64_t m, uint8_t* base) {
    shl_ws W;
    int64_t at = 0;
    auto take = [&](int64_t bytes) {
        uint8_t* r = base ? base + at : nullptr;
        at += (bytes + 255) & ~(int64_t)255;
        return (void*)r;
    };
    const int64_t rt = (m + 4095) / 4096, nt = (m + SHL_TILE - 1) / SHL_TILE, vt = (m + SHV_TILE - 1) / SHV_TILE;
    W.sseg = (uint64_t*)take(m * 8);
    W.loc = (uint64_t*)take(m * 8);
    W.pk = (uint64_t*)take(m * 8);
    W.fin = (int64_t*)take(m * 16);
    W.tiles = (uint64_t*)take(nt * 8);
    W.mask = (uint64_t*)take(vt * (SHV_TILE / 64) * 8);
    W.klo = (uint32_t*)take(m * 4);
    W.khi = (uint32_t*)take(m * 4);
    W.idx = (uint32_t*)take(m * 4);
    W.gk = (uint32_t*)take(m * 4);
    for (int i = 0; i < 2; i++) W.kbuf[i] = (uint32_t*)take(m * 4);
    for (int i = 0; i < 2; i++) W.vbuf[i] = (uint32_t*)take(m * 4);
    W.hist = (uint32_t*)take(256 * rt * 4);
    W.stmp = (uint32_t*)take((int64_t)shd_scan_tmp_words(256 * rt) * 4);
    W.cnt = (uint32_t*)take(vt * 4);
    W.off = (uint32_t*)take(vt * 4);
    W.tmp = (uint32_t*)take((int64_t)shd_scan_tmp_words(vt) * 4);
    W.keepb = (uint8_t*)take(m);
    W.ptmp = (uint32_t*)take((int64_t)shd_scan_tmp_words(m) * 4);
    W.rel = (uint32_t*)W.pk;
    W.choff = W.rel ? W.rel + m : nullptr;
    W.wgt = (uint32_t*)W.fin;
    W.woff = W.wgt ? W.wgt + m : nullptr;
    W.src_of = W.wgt ? W.wgt + 2 * m : nullptr;
    W.bytes = at;
    return W;
}

int shl_ok() { return hipGetLastError() == hipSuccess ? 0 : -3; }
}  // namespace

extern "C" int64_t shl_limit_ws_words(int64_t m) { return shl_layout(m > 0 ? m : 1, nullptr).bytes / 4; }

extern "C" int shl_limit(const shl_rule* rules, int32_t n_rules, int64_t m, int32_t n_out, const shw_rows* src,
                         const int32_t* d_keys, int32_t n_keys, uint64_t seq_base, const shq_table* T,
                         const shw_rows_out* dst, uint32_t* ws, unsigned long long* d_kept, void* stream,
                         const uint64_t** put_keys, const int64_t** put_state) {
    if (put_keys) *put_keys = nullptr;
    if (put_state) *put_state = nullptr;
    if (n_rules < 1 || !rules) return -1;
    std::vector<shl_rule> h_rules((size_t)n_rules);
    if (hipMemcpy(h_rules.data(), rules, (size_t)n_rules * sizeof(shl_rule), hipMemcpyDeviceToHost) != hipSuccess)
        return -3;
    return shl_limit_rules(h_rules.data(), rules, n_rules, m, n_out, src, d_keys, n_keys, seq_base, T, dst, ws, d_kept,
                           stream, put_keys, put_state);
}

extern "C" int shl_limit_rules(const shl_rule* h_rules, const shl_rule* rules, int32_t n_rules, int64_t m,
                               int32_t n_out, const shw_rows* src, const int32_t* d_keys, int32_t n_keys,
                               uint64_t seq_base, const shq_table* T, const shw_rows_out* dst, uint32_t* ws,
                               unsigned long long* d_kept, void* stream, const uint64_t** put_keys,
                               const int64_t** put_state) {
    hipStream_t st = (hipStream_t)stream;
    if (put_keys) *put_keys = nullptr;
    if (put_state) *put_state = nullptr;
    if (n_rules < 1 || !rules || !h_rules) return -1;
    bool holds = false;
    for (int32_t q = 0; q < n_rules; q++) holds = holds || shl_holds(h_rules[q]);
    if (holds && (put_keys || put_state || (T && T->cap > 0))) return -1;  // held rows are not carried
    if (!d_kept || m < 0 || m >= 0x7FFFFFFFll || n_out < 1 || n_out > SHV_MAX_OUT || n_rules < 1 || !rules) return -1;
    if (T && T->cap > 0 && ((T->cap & (T->cap - 1)) || T->n_cols != 1 || !T->keys || !T->state)) return -1;
    if (m == 0) return hipMemsetAsync(d_kept, 0, 8, st) == hipSuccess ? 0 : -3;
    if (!src || !dst || !src->vals || !dst->vals || !ws || (dst->seq && !src->seq) || (dst->query && !src->query) ||
        (dst->ts && !src->ts) || (dst->nulls && !src->nulls) || (dst->key && !src->key) ||
        (!src->key && d_keys && !src->seq) || ((uintptr_t)ws & 7))
        return -1;
    const uint64_t* seq = src->seq;
    const int32_t* query = src->query;
    const int32_t* d_rowkey = src->key;
    const shl_ws W = shl_layout(m, (uint8_t*)ws);
    const unsigned g = (unsigned)((m + SHL_TPB - 1) / SHL_TPB);
    const int64_t nt = (m + SHL_TILE - 1) / SHL_TILE, vt = (m + SHV_TILE - 1) / SHV_TILE;
    int kbits = 0, qbits = 0;
    while (kbits < 31 && ((int64_t)1 << kbits) < (int64_t)(n_keys < 1 ? 1 : n_keys)) kbits++;
    while (qbits < 31 && ((int64_t)1 << qbits) < (int64_t)n_rules) qbits++;
    if (!d_rowkey && !d_keys) kbits = 0;
    if (!query) qbits = 0;
    const bool wide = kbits + qbits > 32;
    hipLaunchKernelGGL(k_shl_prep, dim3(g), dim3(SHL_TPB), 0, st, seq, m, query, d_rowkey, d_keys, seq_base, kbits,
                       W.klo, wide ? W.khi : (uint32_t*)nullptr, W.idx);
    if (shl_ok()) return -3;
    const uint32_t* sidx = W.idx;
    const uint32_t* s32 = W.klo;
    const uint64_t* s64 = nullptr;
    if (!wide) {
        if (kbits + qbits > 0 &&
            shd_sort_pairs(W.klo, W.idx, m, kbits + qbits, W.kbuf, W.vbuf, W.hist, W.stmp, stream, &s32, &sidx))
            return -3;
    } else {
        const uint32_t* ko = nullptr;
        if (shd_sort_pairs(W.klo, W.idx, m, kbits, W.kbuf, W.vbuf, W.hist, W.stmp, stream, &ko, &sidx)) return -3;
        // (idx is free once the first sort has read it)
        hipLaunchKernelGGL(k_shl_pick, dim3(g), dim3(SHL_TPB), 0, st, (const uint32_t*)W.khi, sidx, m, W.gk, W.idx);
        if (shl_ok()) return -3;
        if (shd_sort_pairs(W.gk, W.idx, m, qbits, W.kbuf, W.vbuf, W.hist, W.stmp, stream, &ko, &sidx)) return -3;
        hipLaunchKernelGGL(k_shl_gather, dim3(g), dim3(SHL_TPB), 0, st, sidx, m, (const uint32_t*)W.klo,
                           (const uint32_t*)W.khi, W.sseg);
        s32 = nullptr;
        s64 = W.sseg;
    }
    shq_table tab;
    memset(&tab, 0, sizeof(tab));
    if (T && T->cap > 0) tab = *T;
    const bool put = put_keys && put_state;
    hipLaunchKernelGGL(k_shl_tile, dim3((unsigned)nt), dim3(SHL_TPB), 0, st, s32, s64, kbits, m, tab, W.loc, W.tiles);
    hipLaunchKernelGGL(k_shl_carry, dim3(1), dim3(SHL_CARRY_TPB), 0, st, W.tiles, nt);
    if (holds) {
        hipLaunchKernelGGL(k_shl_rel, dim3(g), dim3(SHL_TPB), 0, st, s32, s64, kbits, sidx, m, rules, n_rules,
                           (const uint64_t*)W.loc, (const uint64_t*)W.tiles, W.rel, W.choff, W.wgt);
        if (shl_ok() || shd_exclusive_scan(W.wgt, W.woff, m, W.ptmp, stream)) return -3;
        hipLaunchKernelGGL(k_shl_src, dim3(g), dim3(SHL_TPB), 0, st, (const uint32_t*)W.rel, (const uint32_t*)W.choff,
                           (const uint32_t*)W.wgt, (const uint32_t*)W.woff, m, W.src_of, d_kept);
        hipLaunchKernelGGL(k_shl_move, dim3((unsigned)vt), dim3(SHV_TILE), 0, st, n_out, m, *src, *dst,
                           (const uint32_t*)W.src_of, (const unsigned long long*)d_kept);
        return shl_ok() ? -3 : 0;
    }
    hipLaunchKernelGGL(k_shl_out, dim3(g), dim3(SHL_TPB), 0, st, s32, s64, kbits, sidx, m, rules, n_rules,
                       (const uint64_t*)W.loc, (const uint64_t*)W.tiles, W.keepb, put ? W.pk : (uint64_t*)nullptr,
                       W.fin);
    hipLaunchKernelGGL(k_shl_mark, dim3((unsigned)vt), dim3(SHV_TILE), 0, st, (const uint8_t*)W.keepb, m, W.mask,
                       W.cnt);
    if (shl_ok()) return -3;
    if (shv_move_marked(m, n_out, src, dst, W.mask, W.cnt, W.off, W.tmp, d_kept, stream)) return -3;
    if (put) {
        *put_keys = W.pk;
        *put_state = W.fin;
    }
    return 0;
}
