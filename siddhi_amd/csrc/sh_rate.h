// sh_rate.h — `output first|last|all every N events` as a rule over the ordered rows
// of one (query, partition key), as host + device code: sh_rate.hip applies it one lane
// per row (k_shl_out, k_shl_rel), and tests/rate_host and tests/rate_all_host compile
// the same code for the CPU.
//
// The reference's event limiters sit behind `having` and in front of the callbacks,
// and a state query's selector sees one state event per chunk, so the fate of a row
// depends only on its ordinal c (1-based) among the rows of its (query, key) that
// reached the limiter:
//   first every N (FirstPerEventOutputRateLimiter.java:47-72): N = 1 keeps c == 1
//     alone (the counter is never reset), N >= 2 keeps (c - 1) mod N == 0;
//   last every N (LastPerEventOutputRateLimiter.java:45-68): keeps c mod N == 0;
//   all every N (AllPerEventOutputRateLimiter.java): every row joins the held chunk and
//     the row with c mod N == 0 sends the chunk, in arrival order, where it stands in the
//     output: nothing is dropped but a run's last c mod N rows, and rows move back to
//     their chunk's N-th (shl_place below).
//
// The word carried between calls is the reduced counter, c0 < max(N, 2): c mod N, and
// for `first every 1` whether any row has passed (0 / 1). It fits 32 bits for every
// N < 2^31 and never wraps; the reference's int counter differs only under `first
// every 1` after 2^32 rows of one (query, key), where it would wrap to 1 and keep one
// more row.
#pragma once
#include <stdint.h>

#include "../../include/sh_query.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SHL_HD __host__ __device__ __forceinline__
#else
#define SHL_HD inline
#endif

// one query's limiter; SH_RATE_NONE (or n < 1) keeps every row and carries nothing
struct shl_rule {
    int32_t kind;  // SH_RATE_NONE / SH_RATE_FIRST_EVENTS / SH_RATE_LAST_EVENTS / SH_RATE_ALL_EVENTS
    int32_t n;
};

SHL_HD bool shl_limits(const shl_rule& R) {
    return (R.kind == SH_RATE_FIRST_EVENTS || R.kind == SH_RATE_LAST_EVENTS || R.kind == SH_RATE_ALL_EVENTS) &&
           R.n >= 1;
}
SHL_HD bool shl_holds(const shl_rule& R) { return R.kind == SH_RATE_ALL_EVENTS && R.n >= 1; }

// the j-th row (1-based) of a run whose carried-in counter is c0 (`all`: the row sends
// its chunk)
SHL_HD bool shl_keep(const shl_rule& R, uint32_t c0, uint64_t j) {
    if (!shl_limits(R)) return true;
    const uint64_t n = (uint64_t)(uint32_t)R.n;
    if (R.kind == SH_RATE_FIRST_EVENTS) return n == 1 ? (c0 == 0 && j == 1) : ((uint64_t)c0 + j - 1) % n == 0;
    return ((uint64_t)c0 + j) % n == 0;
}

// the counter to carry after `rows` more rows
SHL_HD uint32_t shl_next(const shl_rule& R, uint32_t c0, uint64_t rows) {
    if (!shl_limits(R)) return 0;
    const uint64_t n = (uint64_t)(uint32_t)R.n;
    if (R.kind == SH_RATE_FIRST_EVENTS && n == 1) return (c0 || rows) ? 1u : 0u;
    return (uint32_t)(((uint64_t)c0 + rows % n) % n);
}

// Where the j-th row (1-based) of a run that starts from zero leaves. A row that leaves
// does so with its release row, the one `ahead` places further on in its run (itself: 0),
// as number `offset` of the rows that row releases; `weight` is how many rows this row
// releases. Under `all` the release row is the chunk's N-th, so a row leaves only if its
// run is that long (the caller's check: the run key `ahead` places on is its own); the
// other kinds release their kept rows one by one. With the rows' weights w in output
// order, a leaving row's place is exclusive_scan(w)[release row] + offset, and the sum
// of w the number of rows that leave. Every field is below 2^31.
struct shl_spot {
    bool leaves;
    uint32_t ahead, offset, weight;
};
SHL_HD shl_spot shl_place(const shl_rule& R, uint64_t j) {
    shl_spot S;
    if (shl_holds(R)) {
        const uint64_t n = (uint64_t)(uint32_t)R.n, c = j % n;
        S.leaves = true;
        S.ahead = (uint32_t)((n - c) % n);
        S.offset = (uint32_t)((j - 1) % n);
        S.weight = c == 0 ? (uint32_t)n : 0u;
        return S;
    }
    S.leaves = shl_keep(R, 0, j);
    S.ahead = S.offset = 0;
    S.weight = S.leaves ? 1u : 0u;
    return S;
}

// ---- the device pass (sh_rate.hip), all launches asynchronous on `stream`
struct shq_table;
struct shw_rows;
struct shw_rows_out;
#define SHL_TILE 2048  // rows per scan tile

#ifdef __cplusplus
extern "C" {
#endif
// 4-byte words of workspace for m rows (8-byte aligned by the caller)
int64_t shl_limit_ws_words(int64_t m);
// The m ordered raw rows of src (shw_rows, sh_having.h) through their queries'
// limiters (rules[q], n_rules of them in HBM; query ids are in [0, n_rules), a row
// without a query id is query 0's): the kept rows go, in order, to dst, their count
// to *d_kept (8 bytes). A row's key is src->key[r], else d_keys[seq[r] - seq_base],
// else 0; keys are below n_keys. A run starts from its (query << 32 | key) entry of T
// (one column: state[slot * 2] the counter; NULL or cap 0: from zero); T is only
// read. put_keys / put_state (in ws, m entries; both NULL: not written): what shc_put
// takes to carry the runs' counters (limited queries' runs only). 0: launched, < 0:
// error.
// A rule `all every N` (shl_holds) turns the compaction into a placement (shl_place):
// every row that leaves keeps its own columns and the output is no longer in the rows'
// order. Held rows are not carried: such a set is refused (-1) with put_keys / put_state
// or a table that has room (cap > 0), and every run starts from zero.
// shl_limit reads the rules back to know (one blocking copy of n_rules entries);
// shl_limit_rules takes the host's copy beside the device's and never waits.
int shl_limit(const shl_rule* rules, int32_t n_rules, int64_t m, int32_t n_out, const struct shw_rows* src,
              const int32_t* d_keys, int32_t n_keys, uint64_t seq_base, const shq_table* T,
              const struct shw_rows_out* dst, uint32_t* ws, unsigned long long* d_kept, void* stream,
              const uint64_t** put_keys, const int64_t** put_state);
int shl_limit_rules(const shl_rule* h_rules, const shl_rule* rules, int32_t n_rules, int64_t m, int32_t n_out,
                    const struct shw_rows* src, const int32_t* d_keys, int32_t n_keys, uint64_t seq_base,
                    const shq_table* T, const struct shw_rows_out* dst, uint32_t* ws, unsigned long long* d_kept,
                    void* stream, const uint64_t** put_keys, const int64_t** put_state);
#ifdef __cplusplus
}
#endif
