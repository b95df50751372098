// sh_group.h — `group by` for the aggregate post-pass (sh_agg.hip), as host + device
// code: sh_group.hip turns the ordered raw rows into the sorted order and the dense
// segment ids of (query, partition key, group values), and tests/group_host compiles
// the same rule for the CPU.
//
// With `group by` the selector keys every aggregator's state by the group-by values
// beside the partition key (GroupByKeyGenerator.java:60-71: the values' toString()).
// Two rows of one (query, key) share their aggregators iff every group-by value prints
// alike, which the general engine's group table (sh_nfa.h group_aggs) and the oracle's
// AggState key decide on the raw value:
//   * every NaN of a type is one group (Float / Double.toString: "NaN");
//   * -0.0 and +0.0 are two groups ("-0.0" / "0.0");
//   * int / long / bool / string dictionary ids group by value;
//   * a float column is the 4-byte float it is (the row word's low half).
// shg_word maps a raw row value and its static type to the 64-bit group word with
// exactly that equality.
//
// Nulls: sh_run_device takes columns without null masks, and the group-by values of a
// taken query are plain variable outputs of its select, so a group value is never null
// here and the word carries no null flag (the general engine's table keeps one).
#pragma once
#include <stdint.h>

#include "../../include/sh_query.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SHG_HD __host__ __device__ __forceinline__
#else
#define SHG_HD inline
#endif

#define SHG_MAX_QUERIES 16  // NF_MAX_QUERIES: larger sets stream (mode 2) and never group
#define SHG_TILE 1024       // rows per head-flag tile

SHG_HD uint64_t shg_word(int64_t raw, int type) {
    switch (type) {
        case SH_T_FLOAT: {
            uint32_t b = (uint32_t)raw;
            if ((b & 0x7F800000u) == 0x7F800000u && (b & 0x007FFFFFu)) b = 0x7FC00000u;
            return (uint64_t)b;
        }
        case SH_T_DOUBLE: {
            uint64_t b = (uint64_t)raw;
            if ((b & 0x7FF0000000000000ull) == 0x7FF0000000000000ull && (b & 0x000FFFFFFFFFFFFFull))
                b = 0x7FF8000000000000ull;
            return b;
        }
        case SH_T_LONG: return (uint64_t)raw;
        case SH_T_BOOL: return raw ? 1ull : 0ull;
        default: return (uint64_t)(uint32_t)raw;  // int, string dictionary id: 4 bytes
    }
}

// significant bits of a type's words: what the sort passes have to cover
SHG_HD int shg_bits(int type) {
    return (type == SH_T_LONG || type == SH_T_DOUBLE) ? 64 : (type == SH_T_BOOL ? 1 : 32);
}

// one query's group-by attributes as positions of its raw rows; n == 0: no `group by`
// (the query's segments are (query, key) as without this pass)
struct sha_group_q {
    int32_t n;
    int32_t col[SH_MAX_GROUP];   // row position of the value
    int32_t type[SH_MAX_GROUP];  // its static type (sh_type, SH_T_STRING .. SH_T_BOOL)
    int32_t pad[3];
};
struct sha_groups {
    int32_t n_query;  // entries of q; a row of another query id has no group attributes
    int32_t pad;
    sha_group_q q[SHG_MAX_QUERIES];
};

SHG_HD bool shg_valid(const sha_groups* G, int32_t n_out) {
    if (!G || G->n_query < 1 || G->n_query > SHG_MAX_QUERIES) return false;
    for (int q = 0; q < G->n_query; q++) {
        const sha_group_q& g = G->q[q];
        if (g.n < 0 || g.n > SH_MAX_GROUP) return false;
        for (int i = 0; i < g.n; i++)
            if (g.col[i] < 0 || g.col[i] >= n_out || g.type[i] < SH_T_STRING || g.type[i] > SH_T_BOOL) return false;
    }
    return true;
}

// the sort passes over the group words, least significant first (the last one, over
// query * n_keys + key, is the caller's): for attribute i the low word's bits and
// whether a high word follows; *n_attr the attributes any query has
struct shg_plan {
    int32_t n_attr;
    int32_t lo_bits[SH_MAX_GROUP];  // 32, or 1 when every query's attribute i is a bool
    int32_t hi[SH_MAX_GROUP];       // 1: some query's attribute i is 8 bytes wide
};
SHG_HD shg_plan shg_passes(const sha_groups* G) {
    shg_plan P;
    P.n_attr = 0;
    for (int i = 0; i < SH_MAX_GROUP; i++) {
        P.lo_bits[i] = 0;
        P.hi[i] = 0;
    }
    for (int q = 0; q < G->n_query; q++) {
        const sha_group_q& g = G->q[q];
        if (g.n > P.n_attr) P.n_attr = g.n;
        for (int i = 0; i < g.n; i++) {
            const int b = shg_bits(g.type[i]);
            if (b > 32) P.hi[i] = 1;
            const int lo = b > 32 ? 32 : b;
            if (lo > P.lo_bits[i]) P.lo_bits[i] = lo;
        }
    }
    return P;
}

#ifdef __cplusplus
extern "C" {
#endif
// bytes of workspace for m rows (256-byte aligned by the caller)
int64_t shg_scratch_bytes(int64_t m);
// The m ordered raw rows (d_seq, d_vals [m x n_out], d_query or NULL, keys through
// d_keys[seq - seq_base] or NULL: as sha_running reads them) -> *sidx, the stable order
// by (query, key, word_0, word_1, ...), and *sseg, a dense 32-bit segment id per
// sorted position, non-decreasing from 0; both [m], inside the workspace. G is the
// host's descriptor. Asynchronous on `stream`, no readback. m < 2^32 and
// n_query * n_keys <= 2^32. 0: launched (m == 0: nothing written, both NULL); < 0: error.
int shg_segments(const uint64_t* d_seq, const int64_t* d_vals, int32_t n_out, int64_t m, const int32_t* d_query,
                 int32_t n_query, const int32_t* d_keys, int32_t n_keys, uint64_t seq_base, const sha_groups* G,
                 void* d_scratch, void* stream, const uint32_t** sseg, const uint32_t** sidx);
#ifdef __cplusplus
}
#endif
