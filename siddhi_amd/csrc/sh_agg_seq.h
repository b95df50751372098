// sh_agg_seq.h — the sequential aggregate walk and its carried-state table, as
// host + device code: sh_agg.hip runs it one lane per segment (k_shc_walk), and
// tests/agg_seq_host compiles the same arithmetic for the CPU.
//
// The reference adds one match at a time in output order, per (query, partition
// key) (sh_agg.hip header): sum(int|long) and count() in wrap-around longs,
// sum(float|double) and avg(*) as value += (double) x, avg emitting value / count.
// Plain double additions (built with -ffp-contract=off) round as Java's do, and
// carry NaN and the infinities the same way, so the walk needs no exactness proof.
// max(x) / min(x) keep the winning argument's raw bits in the sum word (shq_better).
#pragma once
#include <stdint.h>

#include "../../include/sh_query.h"
#include "sh_agg.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SHQ_HD __host__ __device__ __forceinline__
#else
#define SHQ_HD inline
#endif

// ---- carried state: open addressing over the 64-bit segment key
// (query << 32 | partition key); a slot holds, per aggregate column, the running
// sum's bits and the count: state[(slot * n_cols + k) * 2 + {0, 1}]
#define SHQ_EMPTY (~0ull)

struct shq_table {
    uint64_t* keys;   // [cap], SHQ_EMPTY: free
    int64_t* state;   // [cap * n_cols * 2]
    int64_t cap;      // a power of two, 0: no table (every segment starts from zero)
    int32_t n_cols;
    int32_t pad;
};

SHQ_HD uint64_t shq_key(int32_t query, int32_t key) { return ((uint64_t)(uint32_t)query << 32) | (uint32_t)key; }

SHQ_HD uint64_t shq_hash(uint64_t x) {  // (splitmix64's finaliser)
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// the slot holding `key`, -1: none (a probe ends at the first free slot)
SHQ_HD int64_t shq_find(const shq_table& T, uint64_t key) {
    if (T.cap <= 0) return -1;
    const uint64_t mask = (uint64_t)T.cap - 1ull;
    uint64_t s = shq_hash(key) & mask;
    for (int64_t i = 0; i < T.cap; i++) {
        const uint64_t k = T.keys[s];
        if (k == key) return (int64_t)s;
        if (k == SHQ_EMPTY) return -1;
        s = (s + 1ull) & mask;
    }
    return -1;
}

// ---- the arithmetic
SHQ_HD double shq_bits_double(int64_t b) {
    double d;
    __builtin_memcpy(&d, &b, 8);
    return d;
}
SHQ_HD int64_t shq_double_bits(double d) {
    int64_t b;
    __builtin_memcpy(&b, &d, 8);
    return b;
}

SHQ_HD bool shq_fp(int kind, int arg_type) {
    return kind == SH_AGG_AVG || (kind == SH_AGG_SUM && (arg_type == SH_T_FLOAT || arg_type == SH_T_DOUBLE));
}

// the double the reference adds for a raw column value (Float / Integer / Long unboxed)
SHQ_HD double shq_as_double(int64_t raw, int arg_type) {
    switch (arg_type) {
        case SH_T_FLOAT: {
            const uint32_t u = (uint32_t)raw;
            float f;
            __builtin_memcpy(&f, &u, 4);
            return (double)f;
        }
        case SH_T_DOUBLE: return shq_bits_double(raw);
        case SH_T_INT: return (double)(int32_t)raw;
        case SH_T_LONG: return (double)raw;
        default: return 0.0;
    }
}

// ---- max / min (MaxAttributeAggregatorExecutor / MinAttributeAggregatorExecutor
// processAdd): an empty state takes the argument, otherwise the argument replaces
// the state iff state < arg (max) / state > arg (min) in the argument's own type,
// and the row carries the state's raw bits. A NaN argument therefore never
// replaces a value, a NaN state (the first argument ever) is never replaced, and
// of -0.0 and +0.0 the first stays.
SHQ_HD bool shq_minmax(int kind) { return kind == SH_AGG_MAX || kind == SH_AGG_MIN; }

SHQ_HD bool shq_arg_nan(int64_t raw, int arg_type) {
    if (arg_type != SH_T_FLOAT && arg_type != SH_T_DOUBLE) return false;
    const double d = shq_as_double(raw, arg_type);
    return d != d;
}

// `arg` replaces `state` (float widens to double exactly: the same IEEE ordering;
// int and long compare as integers, never through a double)
SHQ_HD bool shq_better(int kind, int arg_type, int64_t arg, int64_t state) {
    if (arg_type == SH_T_FLOAT || arg_type == SH_T_DOUBLE) {
        const double a = shq_as_double(arg, arg_type), s = shq_as_double(state, arg_type);
        return kind == SH_AGG_MAX ? s < a : s > a;
    }
    const int64_t a = arg_type == SH_T_INT ? (int64_t)(int32_t)arg : arg;
    const int64_t s = arg_type == SH_T_INT ? (int64_t)(int32_t)state : state;
    return kind == SH_AGG_MAX ? s < a : s > a;
}

// one match into the running state (*sum: long or double bits -- for max / min the
// winning argument's raw bits --, *cnt: the adds, 0 = empty); returns the value the
// row carries
SHQ_HD int64_t shq_add(int64_t* sum, int64_t* cnt, int64_t raw, int kind, int arg_type) {
    *cnt = (int64_t)((uint64_t)*cnt + 1ull);
    if (kind == SH_AGG_COUNT) return *cnt;
    if (shq_minmax(kind)) {
        if (*cnt == 1 || shq_better(kind, arg_type, raw, *sum)) *sum = raw;
        return *sum;
    }
    if (!shq_fp(kind, arg_type)) {
        const int64_t v = arg_type == SH_T_INT ? (int64_t)(int32_t)raw : raw;
        *sum = (int64_t)((uint64_t)*sum + (uint64_t)v);  // wraps like Java's long
        return *sum;
    }
    const double s = shq_bits_double(*sum) + shq_as_double(raw, arg_type);
    *sum = shq_double_bits(s);
    return kind == SH_AGG_AVG ? shq_double_bits(s / (double)*cnt) : *sum;
}

// One segment: the rows [p0, p1) of column k in segment order (col: the column's
// copy in sorted order, arguments in, running values out), from the carried state
// of `slot` (-1: zero); the final state goes to fin[0..1].
SHQ_HD void shq_walk(int64_t* col, int64_t p0, int64_t p1, const sha_col& c, const shq_table& T, int64_t slot, int k,
                     int64_t* fin) {
    int64_t sum = 0, cnt = 0;  // (0 is +0.0 as a double)
    if (slot >= 0) {
        sum = T.state[(slot * T.n_cols + k) * 2];
        cnt = T.state[(slot * T.n_cols + k) * 2 + 1];
    }
    if (shq_minmax(c.kind)) {
        // (a loop of its own: the sums' loop keeps its registers)
        for (int64_t p = p0; p < p1; p++) {
            const int64_t raw = col[p];
            if (cnt == 0 || shq_better(c.kind, c.arg_type, raw, sum)) sum = raw;
            cnt = (int64_t)((uint64_t)cnt + 1ull);
            col[p] = sum;
        }
        fin[0] = sum;
        fin[1] = cnt;
        return;
    }
    for (int64_t p = p0; p < p1; p++) col[p] = shq_add(&sum, &cnt, col[p], c.kind, c.arg_type);
    fin[0] = sum;
    fin[1] = cnt;
}

// ---- the device pass (sh_agg.hip), all launches asynchronous on `stream`
#ifdef __cplusplus
extern "C" {
#endif
int64_t shc_scratch_bytes(int64_t m, int n_cols);
// d_vals [m x n_out] raw rows in output order, the aggregators' arguments in the
// listed columns: they become the running values per (d_query[r] or 0, key), the
// key being d_rowkey[r], else d_keys[d_seq[r] - seq_base], else 0. Segments start
// from their state in T (NULL or cap 0: from zero); T is only read. put_keys /
// put_state (in d_scratch, m entries): what shc_put takes to carry the segments'
// final states. 0: launched, < 0: error.
int shc_running(const uint64_t* d_seq, int64_t* d_vals, int32_t n_out, int64_t m, const int32_t* d_query,
                int32_t n_query, const int32_t* d_rowkey, const int32_t* d_keys, int32_t n_keys, uint64_t seq_base,
                const sha_desc* D, const shq_table* T, void* d_scratch, void* stream, const uint64_t** put_keys,
                const int64_t** put_state);
// the entries pk[i] != SHQ_EMPTY (states fin[i * n_cols * 2 ..]) inserted or
// overwritten; *d_entries += slots claimed, *d_err |= 1 when the table is full.
// The caller keeps (entries + n) * 2 <= cap and zeroes both words before the launch.
int shc_put(const shq_table* T, const uint64_t* pk, const int64_t* fin, int64_t n, unsigned long long* d_entries,
            int32_t* d_err, void* stream);
#ifdef __cplusplus
}
#endif
