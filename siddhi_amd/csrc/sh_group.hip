// sh_group.hip — the segments of a grouped select for the aggregate post-pass
// (sh_agg.hip sha_running_grouped): the stable order of the rows by (query, partition
// key, group words) and a dense segment id per sorted position (sh_group.h).
//
//   k_shg_words  one lane per row: query * n_keys + key, the row index, and the
//                canonical group words (shg_word) as 32-bit halves, one array each
//   (sort)       least-significant-first stable passes of shd_sort_pairs: the last
//                group attribute first, its low half and then (8-byte types) its high
//                half, ..., at last query * n_keys + key. Every pass but the first
//                gathers its keys into the order so far (k_shg_pick)
//   k_shg_heads  one lane per sorted position: the row's full key against its
//                predecessor's; one 64-bit ballot word per wave, one count per tile
//   (scan)       shd_exclusive_scan over the tiles' counts
//   k_shg_ids    the heads at or before a position, less one, from the ballot words
//
// Sort passes of 8 bits each: 4 for a 4-byte attribute (int, float, string id), 8 for
// an 8-byte one (long, double), 1 for a bool, and ceil(log2(n_query * n_keys) / 8)
// for the (query, key) pass that sha_running takes alone.
#include <hip/hip_runtime.h>

#include "sh_device.h"
#include "sh_group.h"

#define SHG_TPB 256

__global__ void __launch_bounds__(SHG_TPB) k_shg_words(const uint64_t* __restrict__ seq,
                                                       const int64_t* __restrict__ vals, int n_out, int64_t m,
                                                       const int32_t* __restrict__ query,
                                                       const int32_t* __restrict__ keys, int32_t nkeys,
                                                       uint64_t seq_base, const sha_groups* __restrict__ G, int n_attr,
                                                       uint32_t himask, uint32_t* __restrict__ seg,
                                                       uint32_t* __restrict__ idx, uint32_t* __restrict__ wlo,
                                                       uint32_t* __restrict__ whi) {
    const int64_t r = (int64_t)blockIdx.x * SHG_TPB + threadIdx.x;
    if (r >= m) return;
    const int64_t key = keys ? keys[seq[r] - seq_base] : 0;
    const int64_t q = query ? query[r] : 0;
    seg[r] = (uint32_t)(q * nkeys + key);
    idx[r] = (uint32_t)r;
    const sha_group_q* g = (q >= 0 && q < G->n_query) ? &G->q[q] : nullptr;
    const int n = g ? g->n : 0;
    for (int i = 0; i < n_attr; i++) {
        const uint64_t w = i < n ? shg_word(vals[r * n_out + g->col[i]], g->type[i]) : 0ull;
        wlo[(int64_t)i * m + r] = (uint32_t)w;
        if ((himask >> i) & 1u) whi[(int64_t)i * m + r] = (uint32_t)(w >> 32);
    }
}

// the next pass's keys in the order so far
__global__ void __launch_bounds__(SHG_TPB) k_shg_pick(const uint32_t* __restrict__ key,
                                                      const uint32_t* __restrict__ order, int64_t m,
                                                      uint32_t* __restrict__ gk, uint32_t* __restrict__ gv) {
    const int64_t p = (int64_t)blockIdx.x * SHG_TPB + threadIdx.x;
    if (p >= m) return;
    const uint32_t r = order[p];
    gk[p] = key[r];
    gv[p] = r;
}

// (the mask holds whole tiles: SHG_TILE / 64 words each)
__global__ void __launch_bounds__(SHG_TILE) k_shg_heads(const uint32_t* __restrict__ sidx, int64_t m,
                                                        const uint32_t* __restrict__ seg,
                                                        const uint32_t* __restrict__ wlo,
                                                        const uint32_t* __restrict__ whi, int n_attr, uint32_t himask,
                                                        uint64_t* __restrict__ mask, uint32_t* __restrict__ cnt) {
    __shared__ uint32_t wc[SHG_TILE / 64];
    const int64_t p = (int64_t)blockIdx.x * SHG_TILE + threadIdx.x;
    bool head = false;
    if (p < m) {
        head = p == 0;
        if (!head) {
            const int64_t a = sidx[p - 1], b = sidx[p];
            head = seg[a] != seg[b];
            for (int i = 0; i < n_attr && !head; i++) {
                head = wlo[(int64_t)i * m + a] != wlo[(int64_t)i * m + b];
                if (!head && ((himask >> i) & 1u)) head = whi[(int64_t)i * m + a] != whi[(int64_t)i * m + b];
            }
        }
    }
    const uint64_t bal = __ballot(head);
    if ((threadIdx.x & 63) == 0) {
        mask[p >> 6] = bal;
        wc[threadIdx.x >> 6] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < SHG_TILE / 64; w++) s += wc[w];
        cnt[blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(SHG_TILE) k_shg_ids(int64_t m, const uint64_t* __restrict__ mask,
                                                      const uint32_t* __restrict__ off,
                                                      uint32_t* __restrict__ sseg) {
    const int64_t tile = blockIdx.x;
    const int64_t p = tile * SHG_TILE + threadIdx.x;
    if (p >= m) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t heads = off[tile];
    for (int w = 0; w < wave; w++) heads += (uint32_t)__popcll(mask[tile * (SHG_TILE / 64) + w]);
    const uint64_t b = mask[tile * (SHG_TILE / 64) + wave];
    heads += (uint32_t)__popcll(lane == 63 ? b : (b & ((2ull << lane) - 1ull)));
    sseg[p] = heads - 1u;  // (position 0 is a head)
}

static inline int64_t shg_al(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }

extern "C" int64_t shg_scratch_bytes(int64_t m) {
    if (m < 1) m = 1;
    const int64_t nt = (m + SHG_TILE - 1) / SHG_TILE;
    const int64_t rt = (m + 4095) / 4096;
    // the descriptor; seg, idx, picked keys and order, 2 x 2 sort buffers, the ids;
    // the words' halves; sort histogram and scan temporaries; ballot words, tile
    // counts and offsets with their scan temporaries
    return shg_al(sizeof(sha_groups)) + 9 * shg_al(m * 4) + 2 * shg_al((int64_t)SH_MAX_GROUP * m * 4) +
           shg_al(256 * rt * 4) + shg_al((int64_t)shd_scan_tmp_words(256 * rt) * 4) + shg_al(nt * (SHG_TILE / 64) * 8) +
           2 * shg_al(nt * 4) + shg_al((int64_t)shd_scan_tmp_words(nt) * 4);
}

extern "C" int shg_segments(const uint64_t* d_seq, const int64_t* d_vals, int32_t n_out, int64_t m,
                            const int32_t* d_query, int32_t n_query, const int32_t* d_keys, int32_t n_keys,
                            uint64_t seq_base, const sha_groups* G, void* d_scratch, void* stream,
                            const uint32_t** sseg_out, const uint32_t** sidx_out) {
    if (sseg_out) *sseg_out = nullptr;
    if (sidx_out) *sidx_out = nullptr;
    if (!sseg_out || !sidx_out || m < 0) return -1;
    if (m == 0) return 0;
    if (m >= ((int64_t)1 << 32) || n_out < 1 || !d_vals || !d_scratch || (d_keys && !d_seq) || !shg_valid(G, n_out))
        return -1;
    const int64_t nseg = (int64_t)(n_query < 1 ? 1 : n_query) * (n_keys < 1 ? 1 : n_keys);
    if (nseg > ((int64_t)1 << 32)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nt = (m + SHG_TILE - 1) / SHG_TILE;
    const int64_t rt = (m + 4095) / 4096;
    uint8_t* p = (uint8_t*)d_scratch;
    auto take = [&](int64_t bytes) {
        uint8_t* r = p;
        p += shg_al(bytes);
        return (void*)r;
    };
    sha_groups* dG = (sha_groups*)take(sizeof(sha_groups));
    uint32_t* seg = (uint32_t*)take(m * 4);
    uint32_t* idx = (uint32_t*)take(m * 4);
    uint32_t* gk = (uint32_t*)take(m * 4);
    uint32_t* gv = (uint32_t*)take(m * 4);
    uint32_t* kbuf[2] = {(uint32_t*)take(m * 4), (uint32_t*)take(m * 4)};
    uint32_t* vbuf[2] = {(uint32_t*)take(m * 4), (uint32_t*)take(m * 4)};
    uint32_t* ids = (uint32_t*)take(m * 4);
    uint32_t* wlo = (uint32_t*)take((int64_t)SH_MAX_GROUP * m * 4);
    uint32_t* whi = (uint32_t*)take((int64_t)SH_MAX_GROUP * m * 4);
    uint32_t* hist = (uint32_t*)take(256 * rt * 4);
    uint32_t* stmp = (uint32_t*)take((int64_t)shd_scan_tmp_words(256 * rt) * 4);
    uint64_t* mask = (uint64_t*)take(nt * (SHG_TILE / 64) * 8);
    uint32_t* cnt = (uint32_t*)take(nt * 4);
    uint32_t* off = (uint32_t*)take(nt * 4);
    uint32_t* ctmp = (uint32_t*)take((int64_t)shd_scan_tmp_words(nt) * 4);

    const shg_plan P = shg_passes(G);
    uint32_t himask = 0;
    for (int i = 0; i < P.n_attr; i++)
        if (P.hi[i]) himask |= 1u << i;
    if (hipMemcpyAsync(dG, G, sizeof(sha_groups), hipMemcpyHostToDevice, st) != hipSuccess) return -3;
    const unsigned g = (unsigned)((m + SHG_TPB - 1) / SHG_TPB);
    hipLaunchKernelGGL(k_shg_words, dim3(g), dim3(SHG_TPB), 0, st, d_seq, d_vals, n_out, m, d_query, d_keys, n_keys,
                       seq_base, (const sha_groups*)dG, P.n_attr, himask, seg, idx, wlo, whi);
    if (hipGetLastError() != hipSuccess) return -3;

    // one stable pass over `key` (indexed by row) on top of the order so far
    const uint32_t* order = idx;
    bool first = true;
    auto pass = [&](const uint32_t* key, int bits) {
        if (bits <= 0) return 0;
        const uint32_t* k = key;
        const uint32_t* v = idx;
        if (!first) {
            hipLaunchKernelGGL(k_shg_pick, dim3(g), dim3(SHG_TPB), 0, st, key, order, m, gk, gv);
            if (hipGetLastError() != hipSuccess) return -3;
            k = gk;
            v = gv;
        }
        const uint32_t* ko = nullptr;
        if (shd_sort_pairs(k, v, m, bits, kbuf, vbuf, hist, stmp, stream, &ko, &order)) return -3;
        first = false;
        return 0;
    };
    for (int i = P.n_attr - 1; i >= 0; i--) {
        if (pass(wlo + (int64_t)i * m, P.lo_bits[i])) return -3;
        if (P.hi[i] && pass(whi + (int64_t)i * m, 32)) return -3;
    }
    int bits = 0;
    while (bits < 32 && ((int64_t)1 << bits) < nseg) bits++;
    if (pass(seg, bits)) return -3;

    hipLaunchKernelGGL(k_shg_heads, dim3((unsigned)nt), dim3(SHG_TILE), 0, st, order, m, (const uint32_t*)seg,
                       (const uint32_t*)wlo, (const uint32_t*)whi, P.n_attr, himask, mask, cnt);
    if (hipGetLastError() != hipSuccess) return -3;
    if (shd_exclusive_scan(cnt, off, nt, ctmp, stream)) return -3;
    hipLaunchKernelGGL(k_shg_ids, dim3((unsigned)nt), dim3(SHG_TILE), 0, st, m, (const uint64_t*)mask,
                       (const uint32_t*)off, ids);
    if (hipGetLastError() != hipSuccess) return -3;
    *sseg_out = ids;
    *sidx_out = order;
    return 0;
}
