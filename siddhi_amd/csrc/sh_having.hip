// sh_having.hip — the device row filter behind the fast engines: an output-only
// `having` (sh_having.h) applied to the ordered raw rows an engine produced, as a
// stable compaction into a second set of buffers.
//
//   k_shv_mark   one lane per row: the row's program (through its query id) is
//                evaluated on the row's values; one 64-bit ballot word per wave and
//                one kept count per tile of SHV_TILE rows
//   (scan)       shd_exclusive_scan over the tiles' counts
//   k_shv_move   one workgroup per tile: the kept rows' ranks from the ballot words
//                (popcount prefix), their sources listed in LDS, then the lanes run
//                across the kept rows' words so the stores are contiguous and the
//                loads contiguous per row
//
// Sources and destinations are different buffers: a destination index never exceeds
// its source's, but another workgroup may not have read that source yet.
#include <hip/hip_runtime.h>

#include "sh_device.h"
#include "sh_having.h"

__global__ void __launch_bounds__(SHV_TILE) k_shv_mark(const shv_prog* __restrict__ progs, int32_t n_progs, int64_t m,
                                                       int32_t n_out, const int64_t* __restrict__ vals,
                                                       const int32_t* __restrict__ query,
                                                       const uint8_t* __restrict__ nulls, uint64_t* __restrict__ mask,
                                                       uint32_t* __restrict__ cnt) {
    __shared__ uint32_t wc[SHV_TILE / 64];
    const int64_t r = (int64_t)blockIdx.x * SHV_TILE + threadIdx.x;
    bool keep = false;
    if (r < m) {
        const int32_t q = query ? query[r] : 0;
        keep = (q < 0 || q >= n_progs) ? true
                                       : shv_keep(&progs[q], vals + r * n_out, nulls ? nulls + r * n_out : nullptr);
    }
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

__global__ void __launch_bounds__(SHV_TILE) k_shv_move(int32_t n_out, const uint64_t* __restrict__ seq,
                                                       const int64_t* __restrict__ vals,
                                                       const int32_t* __restrict__ query, const int64_t* __restrict__ ts,
                                                       const uint8_t* __restrict__ nulls, uint64_t* __restrict__ o_seq,
                                                       int64_t* __restrict__ o_vals, int32_t* __restrict__ o_query,
                                                       int64_t* __restrict__ o_ts, uint8_t* __restrict__ o_nulls,
                                                       const uint64_t* __restrict__ mask,
                                                       const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off,
                                                       unsigned long long* __restrict__ d_kept,
                                                       const int32_t* __restrict__ key, int32_t* __restrict__ o_key) {
    __shared__ uint16_t src[SHV_TILE];
    const int64_t tile = blockIdx.x;
    const int64_t row0 = tile * SHV_TILE;
    const uint32_t kept = cnt[tile];
    const int64_t base = off[tile];
    if (tile == (int64_t)gridDim.x - 1 && threadIdx.x == 0) *d_kept = (unsigned long long)(base + kept);
    if (kept == 0) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t before = 0;
    for (int w = 0; w < wave; w++) before += (uint32_t)__popcll(mask[tile * (SHV_TILE / 64) + w]);
    const uint64_t b = mask[tile * (SHV_TILE / 64) + wave];
    if ((b >> lane) & 1ull) src[before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = (uint16_t)threadIdx.x;
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < kept; j += SHV_TILE) {
        const int64_t s = row0 + src[j], d = base + j;
        if (o_seq) o_seq[d] = seq[s];
        if (o_query) o_query[d] = query[s];
        if (o_ts) o_ts[d] = ts[s];
        if (o_key) o_key[d] = key[s];
    }
    const uint32_t words = kept * (uint32_t)n_out;
    for (uint32_t w = threadIdx.x; w < words; w += SHV_TILE) {
        const uint32_t j = w / (uint32_t)n_out, c = w - j * (uint32_t)n_out;
        const int64_t s = (row0 + src[j]) * n_out + c, d = (base + j) * n_out + c;
        o_vals[d] = vals[s];
        if (o_nulls) o_nulls[d] = nulls[s];
    }
}

static inline int64_t shv_tiles(int64_t m) { return (m + SHV_TILE - 1) / SHV_TILE; }

extern "C" int64_t shv_filter_ws_words(int64_t m) {
    const int64_t nt = shv_tiles(m > 0 ? m : 1);
    return nt * (SHV_TILE / 64) * 2 + 2 * nt + (int64_t)shd_scan_tmp_words(nt) + 2;
}

extern "C" int shv_filter(const shv_prog* progs, int32_t n_progs, int64_t m, int32_t n_out, const shw_rows* src,
                          const shw_rows_out* dst, uint32_t* ws, unsigned long long* d_kept, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!d_kept || m < 0 || m >= 0x7FFFFFFFll || n_out < 1 || n_out > SHV_MAX_OUT || n_progs < 1 || !progs) return -1;
    if (m == 0) return hipMemsetAsync(d_kept, 0, 8, st) == hipSuccess ? 0 : -3;
    // (a mismatched pair is refused before anything is launched)
    if (!src || !dst || !src->vals || !dst->vals || !ws || (dst->seq && !src->seq) || (dst->query && !src->query) ||
        (dst->ts && !src->ts) || (dst->nulls && !src->nulls) || (dst->key && !src->key) || ((uintptr_t)ws & 7))
        return -1;
    const int64_t nt = shv_tiles(m);
    uint64_t* mask = (uint64_t*)ws;
    uint32_t* cnt = ws + nt * (SHV_TILE / 64) * 2;
    uint32_t* off = cnt + nt;
    uint32_t* tmp = off + nt;
    hipLaunchKernelGGL(k_shv_mark, dim3((unsigned)nt), dim3(SHV_TILE), 0, st, progs, n_progs, m, n_out, src->vals,
                       src->query, src->nulls, mask, cnt);
    if (hipGetLastError() != hipSuccess) return -3;
    return shv_move_marked(m, n_out, src, dst, (const uint64_t*)mask, (const uint32_t*)cnt, off, tmp, d_kept, stream);
}

extern "C" int shv_move_marked(int64_t m, int32_t n_out, const shw_rows* src, const shw_rows_out* dst,
                               const uint64_t* mask, const uint32_t* cnt, uint32_t* off, uint32_t* tmp,
                               unsigned long long* d_kept, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!d_kept || m <= 0 || m >= 0x7FFFFFFFll || n_out < 1 || n_out > SHV_MAX_OUT || !src || !dst || !src->vals ||
        !dst->vals || !mask || !cnt || !off || !tmp || (dst->seq && !src->seq) || (dst->query && !src->query) ||
        (dst->ts && !src->ts) || (dst->nulls && !src->nulls) || (dst->key && !src->key))
        return -1;
    const int64_t nt = shv_tiles(m);
    if (shd_exclusive_scan(cnt, off, nt, tmp, stream)) return -3;
    hipLaunchKernelGGL(k_shv_move, dim3((unsigned)nt), dim3(SHV_TILE), 0, st, n_out, src->seq, src->vals, src->query,
                       src->ts, src->nulls, dst->seq, dst->vals, dst->query, dst->ts, dst->nulls, mask, cnt,
                       (const uint32_t*)off, d_kept, src->key, dst->key);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
